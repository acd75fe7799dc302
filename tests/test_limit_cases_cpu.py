"""CPU suite for tests/limit_cases.py: every per-tile count the GPU threshold tests (tests/test_gpu_search_limits.py) rely
on, proved with the oracles alone -- the text of each case is searched by approx_ends / dict_matches, the hits are binned
by tile in aligned coordinates and compared with what the case claims.  No call into the library is made here."""
import numpy as np

import limit_cases as lc
from approx_oracle import approx_ends
from dict_oracle import DictIndex, dict_matches


def test_count_lists_cross_the_pool_on_both_sides():
    counts = [c for lst in lc.COUNT_LISTS for c in lst]
    assert set(range(2040, 2057)) | {0, 1, 4096} <= set(counts)
    assert {lc.STAGE - 1, lc.STAGE, lc.STAGE + 1} <= set(counts)
    joined = ",".join(map(str, lc.COUNT_LISTS[1]))
    assert ",".join(map(str, lc.SEQUENCE)) in joined  # the sparse / dense / sparse / full / dense / empty / 2047 run
    assert all(len(lst) * 65536 <= lc.MAX_TILE_TEXT for lst in lc.COUNT_LISTS)
    assert [lc.approx_tile_bytes(m, k) for m, k in ((1, 0), (2, 1), (16, 3), (33, 0), (33, 1), (64, 63))] == \
        [16384, 16384, 32768, 65536, 65536, 131072]


def test_approx_tile_cases_hold_their_counts():
    seen = set()
    for case in lc.approx_tile_cases():
        assert len(case.text) == len(case.counts) * case.tile - case.first <= lc.MAX_TILE_TEXT
        assert not set(case.pat) & set(range(0x80, 0x100))
        ends, dists = approx_ends(case.text, case.pat, case.k)
        got = lc.bin_by_tile(ends, case.tile, case.first, len(case.counts))
        assert got == case.counts, (case.name, got)
        assert case.k == 0 or len(set(dists.tolist())) > 1, case.name  # k > 0: ends of several distances
        seen |= set(got)
    assert {2047, 2048, 2049, 0, 1, 4096} <= seen


def test_approx_tile_cases_reach_both_tile_edges():
    """The last end of every dense tile is a hit, and the first end of the first dense one (its neighbour's last plant
    leaves room): an off-by-one in a tile's range changes the list."""
    case = lc.approx_tile_case(lc.SEQUENCE, 2, 1, first=1, pat=b"ab", plants=[b"ab", b"a", b"b"])
    ends, _ = approx_ends(case.text, case.pat, case.k)
    aligned = set((ends + case.first).tolist())
    assert case.tile in aligned
    for t in (1, 3, 4, 6):
        assert (t + 1) * case.tile - 1 in aligned


def test_dict_tile_cases_hold_their_counts():
    seen = {}
    for case in lc.dict_tile_cases():
        assert len(case.text) == len(case.counts) * case.tile - case.first <= lc.MAX_TILE_TEXT
        pos, ids = dict_matches(case.text, case.patterns)
        got = lc.bin_by_tile(pos, case.tile, case.first, len(case.counts))
        assert got == case.counts, (case.name, got)
        variant = case.name.split()[0]
        per_pos = np.unique(pos, return_counts=True)[1]
        seen.setdefault(variant, set()).update(per_pos.tolist())
    assert seen["one"] == {1}
    assert seen["two"] == {1, 2}
    assert seen["dup"] == {1, 2047, 2048, 2049, 4200}  # single positions at, above and far above the pool
    assert 4200 > 65535 // 16


def test_dup_sparse_case_is_sparse_around_its_heavy_positions():
    case = lc.dict_tile_case(lc.DUP_SPARSE, "dup", first=15)
    pos, ids = dict_matches(case.text, case.patterns)
    where, per_pos = np.unique(pos, return_counts=True)
    heavy = where[per_pos > 1]
    assert per_pos[per_pos > 1].tolist() == [2049, 4200, 2048, 2047]
    assert where.size == 4 + 8  # four heavy positions, eight single pairs in 88 KiB
    for p in heavy.tolist():  # the ids at one position ascend and are not a contiguous block
        mine = ids[pos == p]
        assert np.all(np.diff(mine) > 0) and int(mine[-1] - mine[0]) > mine.size


def test_plan_plants_windows_hold_every_hit():
    rng = np.random.default_rng(3)
    n = 300000
    pat = b"approximate-sear"
    m, k = len(pat), 3
    centre = 150000
    cluster = [(centre - 2 * m + j * m, pat) for j in range(5)]  # back to back across the centre
    offs = lc.spread_offsets(0, n, 40, 64, rng, keep_clear=[(centre - 2 * m, centre + 3 * m)])
    plants = cluster + [(p, pat[:int(rng.integers(m - 4, m + 1))]) for p in offs] + [(n - m, pat)]
    plan = lc.plan_plants(n, plants, m + k)
    text = lc.host_planted_text(plan, seed=9)
    e, d = approx_ends(text, pat, k)
    we, wd = [], []
    for lo, length in plan.windows:
        a, b = approx_ends(text[lo:lo + length], pat, k)
        we.append(a + lo)
        wd.append(b)
    assert np.array_equal(np.concatenate(we), e) and np.array_equal(np.concatenate(wd), d)
    assert int(e[-1]) == n - 1
    assert all(a + la <= b for (a, la), (b, _) in zip(plan.windows[:-1], plan.windows[1:]))
    # the dictionary's windows: reach 0
    pats = [pat, pat[:5], b"sear", b"e"]
    plan0 = lc.plan_plants(n, plants, 0)
    index = DictIndex(pats)
    wp, wi = [], []
    for lo, length in plan0.windows:
        a, b = index.matches(text[lo:lo + length])
        wp.append(a + lo)
        wi.append(b)
    p, i = dict_matches(text, pats)
    assert np.array_equal(np.concatenate(wp), p) and np.array_equal(np.concatenate(wi), i)
