"""Index.match against what a caller had to do without it: n = 2^25 bytes of random lower-case text, 2^13 reads of 128 bytes
cut from the text with one byte replaced at a random place in every 32, which is 2^20 query positions.  Before, the longest
match at every position is a bisection on the length over all positions at once: each of the ceil(log2(129)) = 8 rounds
writes the substring it asks about for every position that is still open into a fresh blob (torch, not charged) and calls
Index.count once; the baseline is the sum of bmx_last_index_ms over the rounds, best of 3 after a warm-up.  Under test:
Index.match, timed by bmx_last_index_ms, best of 3 after a warm-up; the index's construction is not charged.  Both must
give the same len array, and the new time has to be below the baseline by more than the 4 % box-to-box spread the README
states for one kernel.  tools/index_match_rate.py measures other shapes.

Measured on an MI355X: n = 33554432, 8192 reads of 128 bytes (1048576 positions): index match 0.618 ms,
8 rounds of index count 6.801 ms, ratio 0.091; mean len 17.60; index built in 20.0 ms."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SPREAD = 0.04


def reads_with_substitutions(rng, text: np.ndarray, R: int, m: int, every: int) -> np.ndarray:
    at = rng.integers(0, text.size - m, R)
    reads = text[at[:, None] + np.arange(m)]
    for k in range(0, m, every):
        where = k + rng.integers(0, every, R)
        reads[np.arange(R), where] = (rng.integers(0, 26, R) + 97).astype(np.uint8)
    return reads


def bisect_with_count(ctx, idx, d_blob, rest, rounds: int):
    """(ms, len): the longest match at every blob byte among lengths 0 .. rest, by `rounds` calls of Index.count."""
    import torch

    lo, hi, ms = torch.zeros_like(rest), rest.clone(), 0.0
    for _ in range(rounds):
        act = torch.nonzero(lo < hi).squeeze(1)
        if act.numel() == 0:
            break
        mid = (lo[act] + hi[act] + 1) // 2
        ends = torch.cumsum(mid, 0)
        within = torch.arange(int(ends[-1]), device=rest.device) - torch.repeat_interleave(ends - mid, mid)
        sub = d_blob[torch.repeat_interleave(act, mid) + within]
        off = torch.cat([torch.zeros(1, dtype=torch.int64, device=rest.device), ends])
        cnt = idx.count((sub, off))[1]
        ms += ctx.last_index_ms()
        found = cnt > 0
        lo[act] = torch.where(found, mid, lo[act])
        hi[act] = torch.where(found, hi[act], mid - 1)
    assert bool((lo == hi).all())
    return ms, lo


def test_index_match_beats_the_bisection_with_count(ctx):
    import torch

    n, R, m, every = 1 << 25, 1 << 13, 128, 32
    rounds = int(np.ceil(np.log2(m + 1)))
    assert rounds == 8
    rng = np.random.default_rng(0x5EED1DE5)
    text = (rng.integers(0, 26, n) + 97).astype(np.uint8)
    reads = reads_with_substitutions(rng, text, R, m, every)
    d_text = torch.from_numpy(text).cuda()
    d_blob = torch.from_numpy(reads.reshape(-1)).cuda()
    d_off = torch.arange(0, R * m + 1, m, dtype=torch.int64, device="cuda")
    rest = m - torch.arange(R * m, dtype=torch.int64, device="cuda") % m
    idx = ctx.index(d_text)

    t_bisect, want = [], None
    for rep in range(4):  # the first one warms up
        ms, want = bisect_with_count(ctx, idx, d_blob, rest, rounds)
        if rep:
            t_bisect.append(ms)
    t_match, got = [], None
    for rep in range(4):
        got = idx.match((d_blob, d_off))[0]
        if rep:
            t_match.append(ctx.last_index_ms())
    assert torch.equal(got.to(torch.int64), want)
    assert int(want.max()) >= every  # the reads do come from the text

    a, b = min(t_match), min(t_bisect)
    print(f"n = {n}, {R} reads of {m} bytes ({R * m} positions): index match {a:.3f} ms, {rounds} rounds of index count {b:.3f} ms, "
          f"ratio {a / b:.3f}; mean len {float(want.double().mean()):.2f}; index built in {idx.build_ms:.1f} ms")
    idx.close()
    del d_text, d_blob
    torch.cuda.empty_cache()
    assert a < (1.0 - SPREAD) * b, (a, b)
