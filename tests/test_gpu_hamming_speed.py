"""The k-mismatch search against what a caller runs for the same question today, before filtering on the host: the
approximate search at the same pattern and k.  On 1 GiB of printable-95 text and a 20-byte pattern copied from the text and
planted with 0..3 substitutions at a few thousand places, k = 3 and must = 0, the two-slice 32-bit Hamming kernel's time
(HIP events around the kernel, best of 3 after a warm-up) has to be below the approximate kernel's, measured in the same
run, by more than the 4 % box-to-box spread the README states for one kernel.  The lists obey the superset rule: every
hit's end is among the approximate ends with an edit distance no larger than its mismatches.  There is no bound for the
four-slice kernels or for 64 bits: tools/hamming_rate.py measures every shape at 4 GiB."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SPREAD = 0.04


def test_two_slice_kernel_beats_the_approximate_kernel_at_k3(ctx):
    import torch

    n, m, k = 1 << 30, 20, 3
    d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
    ctx.gen_text(d_text, 0, 0x4A33E5, 0)
    pat = d_text[123456789:123456789 + m].cpu().numpy().tobytes()
    rng = np.random.default_rng(20)
    offsets = np.sort(rng.choice(n // 4096 - 1, 4000, replace=False)).astype(np.uint64) * 4096 + 77
    planted = {}
    for subs in range(k + 1):  # 1000 copies each with 0, 1, 2 and 3 substitutions
        variant = bytearray(pat)
        for i in rng.choice(m, subs, replace=False):
            variant[i] = 0x20 + (variant[i] - 0x20 + 1 + int(rng.integers(0, 94))) % 95  # another printable byte
        ctx.plant(d_text, 0, bytes(variant), offsets[subs::k + 1])
        planted.update({int(o): subs for o in offsets[subs::k + 1]})
    cap = 1 << 16
    out_h = torch.empty(cap, dtype=torch.int64, device="cuda")
    dist_h = torch.empty(cap, dtype=torch.uint8, device="cuda")
    out_a = torch.empty(cap, dtype=torch.int64, device="cuda")
    dist_a = torch.empty(cap, dtype=torch.uint8, device="cuda")
    ctx.search_hamming_device(d_text, pat, k, out=out_h, dist_out=dist_h)  # warm-up
    ctx.search_approx_device(d_text, pat, k, out=out_a, dist_out=dist_a)
    t_hamming, t_approx = [], []
    for _ in range(3):
        starts, dist, total_h = ctx.search_hamming_device(d_text, pat, k, out=out_h, dist_out=dist_h)
        t_hamming.append(ctx.last_hamming_ms())
        ends, edits, total_a = ctx.search_approx_device(d_text, pat, k, out=out_a, dist_out=dist_a)
        t_approx.append(ctx.last_approx_ms())
    h, a = min(t_hamming), min(t_approx)
    print(f"two-slice 32-bit Hamming kernel {h:.3f} ms, approximate kernel at k = {k} {a:.3f} ms, ratio {h / a:.3f}")
    del d_text
    torch.cuda.empty_cache()
    assert 4000 <= total_h <= total_a <= cap
    s, d = starts.cpu().numpy(), dist.cpu().numpy()
    found = dict(zip(s.tolist(), d.tolist()))
    assert all(found.get(o) == subs for o, subs in planted.items())  # every copy, with its substitutions
    assert found.get(123456789) == 0
    e, ed = ends.cpu().numpy(), edits.cpu().numpy()
    at = np.searchsorted(e, s + m - 1)  # the superset rule
    assert (at < e.size).all() and np.array_equal(e[at], s + m - 1) and (ed[at] <= d).all()
    assert h < (1.0 - SPREAD) * a, (h, a)
