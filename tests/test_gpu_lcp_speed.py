"""The LCP array costs less than the suffix array it describes.

Claim: on the same text, in the same process, the event time around the LCP kernels (bmx_last_lcp_ms) is below the
suffix-array build beside it (bmx_last_suffix_array_ms): best of 3 after one warm-up on each side, the two alternating,
lcp_ms < (1 - 0.04) x sa_ms (4 % is the box-to-box spread the README states for one kernel).  Every run's array is
checked on the device.

Measured on the MI355X (ms, best of 3; tools/lcp_rate.py measures the same texts, best of 5, into
profiles/r09_lcp_rate.jsonl):

    text                                      n             lcp_ms     sa_ms    lcp / sa
    random lower-case                         2^25          2.076      6.795    0.306
    a 61-letter paragraph repeated            2^24 + 4,097  0.665      36.427   0.018
    all 'a'                                   2^25 - 1      0.460      59.858   0.008
"""
import numpy as np
import pytest

import lcp_oracle as lo

pytestmark = pytest.mark.gpu

MARGIN = 0.04


def measure(ctx, d_text, check):
    best_sa = best_lcp = float("inf")
    for it in range(4):  # the first round is the warm-up
        d_sa = ctx.suffix_array_device(d_text)
        sa_ms = ctx.last_suffix_array_ms()
        d_lcp = ctx.lcp_array_device(d_text, d_sa)
        lcp_ms = ctx.last_lcp_ms()
        check(d_sa, d_lcp)
        if it:
            best_sa, best_lcp = min(best_sa, sa_ms), min(best_lcp, lcp_ms)
    print(f"\nLCP speed n={d_text.numel()}: lcp {best_lcp:.3f} ms, suffix array {best_sa:.3f} ms, ratio {best_lcp / best_sa:.3f}, "
          f"long pairs {ctx.last_lcp_long_pairs()}")
    assert best_lcp > 0 and best_sa > 0
    assert best_lcp < (1 - MARGIN) * best_sa, (best_lcp, best_sa)


def test_random_lower_case(ctx):
    import torch

    n = 1 << 25
    gen = torch.Generator(device="cuda:0").manual_seed(25)
    d_text = (torch.randint(0, 26, (n,), generator=gen, device="cuda:0") + 97).to(torch.uint8)
    padded = torch.cat([d_text, torch.zeros(16, dtype=torch.uint8, device="cuda:0")])
    k = torch.arange(16, device="cuda:0")

    def check(d_sa, d_lcp):
        """16 bytes per side give the exact value where it is below 16; it is, everywhere."""
        assert int(d_lcp[0]) == 0
        worst = 0
        for lo_j in range(1, n, 1 << 22):
            hi_j = min(n, lo_j + (1 << 22))
            a, b = d_sa[lo_j - 1:hi_j - 1].long(), d_sa[lo_j:hi_j].long()
            same = padded[a[:, None] + k] == padded[b[:, None] + k]
            same &= (k < (n - torch.maximum(a, b))[:, None])
            h = same.long().cumprod(dim=1).sum(dim=1)
            worst = max(worst, int(h.max()))
            assert bool(torch.equal(h.int(), d_lcp[lo_j:hi_j]))
        assert worst < 16

    measure(ctx, d_text, check)


def test_a_paragraph_repeated(ctx):
    import torch

    n, q = (1 << 24) + 4097, 61
    rng = np.random.default_rng(61)
    para = (rng.integers(0, 26, q) + 97).astype(np.uint8)
    assert lo.primitive_period(para) == q
    x = np.tile(para, n // q + 1)[:n].copy()
    d_text = torch.from_numpy(x).to("cuda:0")

    def check(d_sa, d_lcp):
        """tests/lcp_oracle.py's rule: congruent pairs on the device, the few others on the host."""
        assert int(d_lcp[0]) == 0
        a, b = d_sa[:-1].long(), d_sa[1:].long()
        cong = (a - b) % q == 0
        assert bool(torch.equal(torch.where(cong, n - torch.maximum(a, b), d_lcp[1:].long()), d_lcp[1:].long()))
        other = torch.nonzero(~cong).flatten()
        assert other.numel() < 4 * q
        want = lo.periodic_pairs(x, q, a[other].cpu().numpy(), b[other].cpu().numpy())
        assert np.array_equal(d_lcp[1:][other].cpu().numpy(), want)

    measure(ctx, d_text, check)


def test_one_letter(ctx):
    import torch

    n = (1 << 25) - 1
    d_text = torch.full((n,), ord("a"), dtype=torch.uint8, device="cuda:0")
    want = torch.arange(n, dtype=torch.int32, device="cuda:0")

    def check(d_sa, d_lcp):
        assert bool(torch.equal(d_lcp, want))

    measure(ctx, d_text, check)
