"""Index.map against what a caller had to do without it for reads short enough: n = 2^25 bytes of random lower-case text,
256 reads of 48 bytes cut from the text with one substitution each, k = 2, min_len = 12, max_occ = 8.  Before: one
bmx_search_approx_device over the whole text per read with the same k; the baseline is the sum of bmx_last_approx_ms over
the 256 calls, best of 3 after a warm-up.  Under test: one Index.map of the 256 reads, timed by bmx_last_index_ms, best of
3 after a warm-up; the index is built once for a resident text and not charged.  Every read's best_end and best_dist must
appear in that read's approximate-search list.

The bar is twice the measured ratio (the factor covers the 4 % box-to-box spread the README states and the weight of
launch overhead in a sub-millisecond call), and below 1 in any case.

Measured on an MI355X: n = 33554432, 256 reads of 48 bytes, k = 2: index map 0.175 ms
(386 candidates), 256 approximate searches 15.575 ms, ratio 0.01125; index built in 29.3 ms.  The bar is 0.0225."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BAR = 0.0225  # twice the measured 0.01125 = Index.map ms / summed approximate-search ms


def test_index_map_beats_one_approximate_search_per_read(ctx):
    import torch

    n, R, m, k, min_len, max_occ = 1 << 25, 256, 48, 2, 12, 8
    rng = np.random.default_rng(0x5EED3A9)
    text = (rng.integers(0, 26, n) + 97).astype(np.uint8)
    at = rng.integers(0, n - m, R)
    reads = text[at[:, None] + np.arange(m)]
    where = rng.integers(0, m, R)
    reads[np.arange(R), where] = (reads[np.arange(R), where] - 97 + rng.integers(1, 26, R)) % 26 + 97  # another letter
    d_text = torch.from_numpy(text).cuda()
    d_blob = torch.from_numpy(reads.reshape(-1)).cuda()
    d_off = torch.arange(0, R * m + 1, m, dtype=torch.int64, device="cuda")
    idx = ctx.index(d_text)

    out = torch.empty(64, dtype=torch.int64, device="cuda")
    dist_out = torch.empty(64, dtype=torch.uint8, device="cuda")
    t_approx, lists = [], []
    for rep in range(4):  # the first one warms up
        ms, lists = 0.0, []
        for r in range(R):
            ends, dist, total = ctx.search_approx_device(d_text, reads[r].tobytes(), k, out=out, dist_out=dist_out)
            ms += ctx.last_approx_ms()
            if rep == 3:
                assert total <= 64
                lists.append(set(zip(ends.tolist(), dist.tolist())))
        if rep:
            t_approx.append(ms)
    t_map, got = [], None
    for rep in range(4):
        got = idx.map((d_blob, d_off), min_len, max_occ, k)
        if rep:
            t_map.append(ctx.last_index_ms())
    best_end, best_dist = got[1].tolist(), got[2].tolist()
    for r in range(R):
        assert (best_end[r], best_dist[r]) in lists[r], (r, best_end[r], best_dist[r], sorted(lists[r]))
    assert max(best_dist) <= 1  # every read maps, with its one substitution at most

    a, b = min(t_map), min(t_approx)
    print(f"n = {n}, {R} reads of {m} bytes, k = {k}: index map {a:.3f} ms ({ctx.last_index_map_candidates()} candidates), "
          f"{R} approximate searches {b:.3f} ms, ratio {a / b:.5f}; index built in {idx.build_ms:.1f} ms")
    idx.close()
    del d_text, d_blob
    torch.cuda.empty_cache()
    assert a < BAR * b, (a, b, BAR)
