"""CPU suite for tests/limit_cases.py: every per-tile count the GPU threshold tests (tests/test_gpu_search_limits.py,
tests/test_gpu_tile_geometry.py) rely on, proved with the oracles alone -- the text of each case is searched by the
search's own oracle (approx_ends, dict_matches, class_starts, class_approx_ends, hamming_starts, gap_ends, ends_numpy), the
hits are binned by tile in aligned coordinates and compared with what the case claims.  No call into the library is made
here."""
import numpy as np
import pytest

import limit_cases as lc
from approx_oracle import approx_ends
from dict_oracle import DictIndex, dict_matches
import regex_oracle as ro
import regex_star_oracle as so


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


# ---- the tile frame at a chosen piece size and grid (tests/test_gpu_tile_geometry.py) ----------------------------------

def test_searches_cover_every_kernel_slot_and_stay_inside_the_rule():
    kinds = {}
    for name, s in lc.SEARCHES.items():
        kinds.setdefault(s.kind, []).append(s)
        assert 6 <= s.floor <= s.cap and 1 <= s.min_len <= s.reach, name
        if s.member is not None:
            assert not s.member[:, 0x80:].any(), name  # no class holds a background byte
    assert {s.m > 32 for s in kinds["classes"]} == {False, True} == {s.m > 32 for s in kinds["gaps"]}
    assert {s.m > 32 for s in kinds["approx"]} == {False, True} and 64 < lc.SEARCHES["approx_long2"].m <= 128
    assert {(s.m > 32, s.k > 3) for s in kinds["hamming"]} == {(w, f) for w in (False, True) for f in (False, True)}
    assert {(s.rx.m > 32, ro.split(s.rx)[1] != 0) for s in kinds["regex"]} == {(w, f) for w in (False, True) for f in (False, True)}
    assert [lc.SEARCHES[n].floor for n in ("classes32", "classes64", "gaps64", "hamming64x4", "regex64nl", "approx64", "approx_long2")] == \
        [6, 8, 8, 8, 8, 8, 9]


def test_tiles_per_workgroup():
    assert [lc.tiles_per_workgroup_at_least(14, g) for g in (1, 2, 3, 14, 15)] == [14, 7, 5, 1, 1]
    assert lc.tiles_per_workgroup_at_least(8, 3) == 3 and lc.tiles_per_workgroup_at_least(4, 2) == 2


@pytest.mark.parametrize("name", [n for n in lc.SEARCHES if not n.endswith("_run")])
def test_geometry_cases_hold_their_counts(name):
    """Per-tile counts of the several-tiles-per-workgroup cases, at the three pointer offsets; every grid the GPU test
    uses leaves some workgroup at least two tiles, a grid of one all of them."""
    s = lc.SEARCHES[name]
    ran = 0
    for case in lc.geometry_cases(name):
        n_tiles = len(case.counts)
        assert case.tile == 256 << s.floor and 8 <= n_tiles <= 16 and n_tiles * case.tile <= lc.MAX_TILE_TEXT
        assert len(case.text) == n_tiles * case.tile - case.first
        assert case.counts == lc.SEQUENCE_BOTH_WAYS[:n_tiles] and set(lc.SEQUENCE) <= set(case.counts)
        ends, dists = s.ends(case.text)
        assert lc.bin_by_tile(ends, case.tile, case.first, n_tiles) == case.counts, case.name
        if s.k:
            assert len(set(dists.tolist())) > 1, case.name
        for grid in lc.GRIDS:
            least = lc.tiles_per_workgroup_at_least(n_tiles, grid)
            assert least >= 2 and (grid != 1 or least == n_tiles)
        cut = lc.capacity_inside_second_dense(case)
        dense = [t for t, c in enumerate(case.counts) if c > lc.STAGE][1]
        assert case.prefix(dense) < cut < case.prefix(dense + 1)
        ran += 1
    assert ran == len(lc.OFFSETS)


def test_dict_geometry_cases_hold_their_counts():
    for first in lc.OFFSETS:
        case = lc.dict_geometry_case(first)
        pos, _ = dict_matches(case.text, case.patterns)
        assert lc.bin_by_tile(pos, case.tile, first, len(case.counts)) == case.counts == lc.SEQUENCE_BOTH_WAYS
        assert all(lc.tiles_per_workgroup_at_least(len(case.counts), g) >= 2 for g in lc.GRIDS)


@pytest.mark.parametrize("name,ps", lc.BOUNDARY_CASES)
def test_boundary_cases_have_what_they_claim(name, ps):
    """The large-piece cases: a piece shift the rule can give the pattern, hits on both sides of the lane and tile
    boundaries, a lane whose every end is a hit (its ordinals reach 2^ps - 1), a tile of more hits than the pool with hits
    in (nearly) every lane, an empty tile behind it, hits up to the text's last byte; for the k-mismatch search three
    distances or more in the dense tile.  The windows around the plants give the whole text's list."""
    case = lc.boundary_case(name, ps)
    s, T, P, first = case.search, case.tile, 1 << ps, case.first
    assert s.floor <= ps <= s.cap and len(case.text) == 3 * T + 5 and first == lc.BOUNDARY_OFFSET
    ends, dists = case.ends_by_windows()
    if ps <= 11:  # (the whole text where its oracle takes a second or so: all but the 3 MiB of the long approximate search)
        whole_e, whole_d = s.ends(case.text)
        assert np.array_equal(whole_e, ends) and (dists is None or np.array_equal(whole_d, dists))
    aligned = ends + first
    have = set(aligned.tolist())
    for lane in lc.BOUNDARY_LANES:
        assert {lane * P - 1, lane * P} <= have, (case.name, lane)
    assert {T - 1, T, 2 * T - 1, 3 * T, len(case.text) - 1 + first} <= have and 2 * T not in have
    lane0 = T + lc.FULL_LANE * P
    assert set(range(lane0 - 1, lane0 + P + 1)) <= have
    counts = lc.bin_by_tile(ends, T, first, 4)
    # a tile that is parked (no more hits than the pool) has a lane with min(P, 2000) hits: the ordinals the read-out of
    # the pool takes from the parked words go up to that; for the searches with distances the lane has two or more
    lane_p = lc.PARKED_LANE * P
    in_lane = (aligned >= lane_p) & (aligned < lane_p + P)
    assert counts[0] <= lc.STAGE and lc.parked_lane_hits(ps) - s.k <= int(in_lane.sum()) <= P, (counts[0], int(in_lane.sum()))
    if s.k:
        assert np.unique(dists[in_lane]).size >= 2, case.name
    assert lc.parked_lane_hits(ps) - s.k + 10 <= counts[0] <= lc.STAGE and counts[1] > lc.STAGE + P and counts[2] == 0 and counts[3] == 5 + first, counts
    in_dense = (aligned >= T) & (aligned < 2 * T)
    assert np.unique((aligned[in_dense] - T) // P).size >= 250
    if s.kind == "hamming":
        assert np.unique(dists[in_dense]).size >= 3
    assert lc.tiles_per_workgroup_at_least(4, 2) >= 2


# ---- the star search (tests/test_gpu_regex_star_limits.py) -------------------------------------------------------------

def _states_behind(s, entry):
    """Every state the search's automaton can be in behind `entry` on a text of the search's letters and background bytes,
    and the set of those it is in right behind a background byte."""
    alphabet = list(s.letters) + list(range(0x80, 0x100))
    seen, frontier, behind_background = {entry}, [entry], set()
    while frontier:
        D = frontier.pop()
        for c in alphabet:
            D2 = s.rx.step(D, c)
            if c >= 0x80:
                behind_background.add(D2)
            if D2 not in seen:
                seen.add(D2)
                frontier.append(D2)
    return seen, behind_background


def test_star_searches_cover_every_slot_and_a_background_byte_resets_them():
    """floor 8, cap 12 (bmx_regex_star.hip), every kernel slot, and what reach == 1 rests on: no class of the first family
    holds a background byte, so one such byte empties the state; behind the second family's prefix one background byte
    leaves one and the same state, the one it leaves right behind the prefix (so the oracle on a window that begins with
    a background byte, run behind a copy of the prefix, is the oracle on the whole text)."""
    slots = set()
    for name, s in lc.STAR_SEARCHES.items():
        assert (s.kind, s.floor, s.cap, s.reach) == ("regex_star", 8, 12, 1), name
        k = so.masked(s.rx)
        assert k.all == (1 << s.m) - 1, name  # (every position is useful: the kernels see the automaton as it is)
        irregular = any(f and f != 1 << (i + 1) for i, f in enumerate(k.follow))
        slots.add((bool(s.prefix), s.m > 32, irregular, s.rx.max_len == so.UNBOUNDED))
        entry = so.run(s.prefix, s.rx, 0, True)
        seen, behind_background = _states_behind(s, entry)
        if not s.prefix:
            assert not s.rx.member[:, 0x80:].any(), name
            assert behind_background == {0}, name
        else:
            assert s.prefix == b"c" and s.min_len == 1 and not set(s.prefix) & set(s.letters)
            assert behind_background == {s.rx.step(entry, 0x80)} and 0 not in seen, name
        for hits in (1, 2, 3, 9, 64, 700):  # a run of L letters: L hits (less min_len - 1) at adjacent ends
            assert s.run_unit(hits).count == hits, (name, hits)
    assert slots == {(False, False, True, True), (False, True, True, True), (False, False, False, False), (False, True, False, False),
                     (False, False, True, False), (True, False, True, True), (True, True, True, True)}
    assert [lc.star_warm(ps) for ps in (4, 8, 9, 10, 11, 12)] == [64, 64, 64, 64, 128, 256]


def _star_proof(s, text, first, ps, ends):
    """The taint a case claims, at its piece and the rule's warm-up.  First family: no lane's bounds differ.  Natural
    taint: the first launch's waves are (all but the first few) tainted, its list misses true ends, and so does a slow
    path that carried `base` alone from piece to piece -- the case runs the column term."""
    warm = lc.star_warm(ps)
    if not s.prefix:
        model = so.fast_taint(text, s.rx, first, 0, ps, warm, walk=False)
        assert model.waves == 0 and not model.lanes
        return 0
    assert text[:1] == s.prefix and text.count(s.prefix) == 1
    letters = np.nonzero(np.isin(np.frombuffer(text, np.uint8), list(s.letters)))[0]
    assert np.array_equal(ends, letters)  # the hits are the letters, as for [ab]+
    model = so.fast_taint(text, s.rx, first, 0, ps, warm)
    n_waves = len({(t, l >> 6) for t, l, _, _ in so.tile_lanes(len(text), first, 0, ps)})
    assert n_waves - 1 <= model.waves <= n_waves and len(model.lanes) >= n_waves * 64 - (warm >> ps) - 66
    assert model.ends.size < ends.size // 4 and np.isin(model.ends, ends).all()
    k = so.masked(s.rx)
    e, u = so.pair_bounds(text, k, 1 << ps, first)
    base, cols = so.columns(text, k, 1 << ps, e, u, first)
    assert sum(1 for x in u if x) >= len(u) - 2 and sum(len(c) for c in cols) >= len(u) - 2
    without = so.entry_ends(text, k, first, 0, ps, so.sweep(e, u, base, cols, use_columns=False))
    assert without.size < ends.size // 4 and np.isin(without, ends).all()
    if len(text) <= 1 << 20:  # (and with the columns it is the truth)
        assert np.array_equal(so.entry_ends(text, k, first, 0, ps, so.sweep(e, u, base, cols)), ends)
    return model.waves


def _star_tile_case_proof(case):
    s, n_tiles = case.search, len(case.counts)
    assert case.tile == 256 << 8 == 256 << case.ps and len(case.text) == n_tiles * case.tile - case.first <= lc.MAX_TILE_TEXT
    ends, _ = s.ends(case.text)
    assert lc.bin_by_tile(ends, case.tile, case.first, n_tiles) == case.counts, case.name
    _star_proof(s, case.text, case.first, case.ps, ends)


@pytest.mark.parametrize("name", list(lc.STAR_SEARCHES))
def test_star_geometry_cases_hold_their_counts_and_their_taint(name):
    ran = 0
    for case in lc.star_geometry_cases(name):
        assert case.counts == lc.SEQUENCE_BOTH_WAYS
        _star_tile_case_proof(case)
        assert all(lc.tiles_per_workgroup_at_least(len(case.counts), g) >= 2 for g in lc.GRIDS)
        dense = [t for t, c in enumerate(case.counts) if c > lc.STAGE][1]
        assert case.prefix(dense) < lc.capacity_inside_second_dense(case) < case.prefix(dense + 1)
        ran += 1
    assert ran == len(lc.OFFSETS)


@pytest.mark.parametrize("name,which", [(n, w) for n in ("star32", "taint32") for w in (0, 1)])
def test_star_count_cases_hold_their_counts_and_their_taint(name, which):
    case = lc.star_count_case(name, which)
    assert case.counts == lc.COUNT_LISTS[which] and case.first == lc.STAR_COUNT_OFFSET
    _star_tile_case_proof(case)


@pytest.mark.parametrize("name,ps", lc.STAR_BOUNDARY_CASES + lc.STAR_TAINT_BOUNDARY_CASES)
def test_star_boundary_cases_have_what_they_claim(name, ps):
    """test_boundary_cases_have_what_they_claim for the star search at pieces of 2^9 .. 2^12 ends, the window argument on
    the whole text at every size, and the taint each case claims."""
    case = lc.boundary_case(name, ps)
    s, T, P, first = case.search, case.tile, 1 << ps, case.first
    assert 9 <= ps <= s.cap and len(case.text) == 3 * T + 5 and first == lc.BOUNDARY_OFFSET
    ends, _ = case.ends_by_windows()
    whole, _ = s.ends(case.text)
    assert np.array_equal(whole, ends)
    aligned = ends + first
    have = set(aligned.tolist())
    for lane in lc.BOUNDARY_LANES:
        assert {lane * P - 1, lane * P} <= have, (case.name, lane)
    assert {T - 1, T, 2 * T - 1, 3 * T, len(case.text) - 1 + first} <= have and 2 * T not in have
    lane0 = T + lc.FULL_LANE * P
    assert set(range(lane0 - 1, lane0 + P + 1)) <= have  # (32 lines of the walk's loop at ps 12, every end a hit)
    counts = lc.bin_by_tile(ends, T, first, 4)
    lane_p = lc.PARKED_LANE * P
    in_lane = (aligned >= lane_p) & (aligned < lane_p + P)
    assert int(in_lane.sum()) == lc.parked_lane_hits(ps) == min(P, 2000)  # ordinals up to that less one are parked
    assert lc.parked_lane_hits(ps) + 10 <= counts[0] <= lc.STAGE and counts[1] > lc.STAGE + P and counts[2] == 0 and counts[3] == 5 + first, counts
    in_dense = (aligned >= T) & (aligned < 2 * T)
    assert np.unique((aligned[in_dense] - T) // P).size >= 250
    assert {n for n, _ in lc.STAR_BOUNDARY_CASES} == set(lc.STAR_FAST) and {n for n, _ in lc.STAR_TAINT_BOUNDARY_CASES} == set(lc.STAR_TAINT)
    assert {p for _, p in lc.STAR_BOUNDARY_CASES} == {9, 10, 11, 12} == {p for _, p in lc.STAR_TAINT_BOUNDARY_CASES}
    _star_proof(s, case.text, first, ps, ends)


WARM_EDGE_SETS = [(ps, first, None) for ps in (8, 12) for first in (0, 5, 15)] + [(8, 5, 16), (8, 5, 4096)]


@pytest.mark.parametrize("ps,first,warm", WARM_EDGE_SETS)
def test_warm_edge_cases_straddle_the_edge(ps, first, warm):
    """The placements of tests/test_gpu_regex_star_limits.py around the pair warm-up's edge: the model of the first
    launch counts one tainted wave exactly where the c lies in front of the owning lane's warm-up and that warm-up does
    not begin at view byte 0, none otherwise; either way the one hit is the d."""
    seen = []
    for case in lc.warm_edge_cases(ps, first, warm):
        assert case.warm == (lc.star_warm(ps) if warm is None else warm)
        want = so.ends_numpy(case.text, lc.STAR_EDGE.rx)
        assert want.tolist() == [case.d_at] and case.lead <= case.d_at, case.name
        model = so.fast_taint(case.text, lc.STAR_EDGE.rx, first, case.lead, ps, case.warm)
        assert model.waves == case.tainted_waves == len(model.lanes), case.name
        assert model.ends.tolist() == ([] if model.waves else [case.d_at]), case.name  # a tainted lane's list misses the hit
        assert np.array_equal(so.slow_ends(case.text, lc.STAR_EDGE.rx, first, case.lead, ps), want), case.name
        seen.append(case.tainted_waves)
    assert seen.count(0) >= 3 and seen.count(1) >= 3 and len(seen) == (6 if warm == 16 else 8), seen


def test_star_row_of_windows_gives_the_whole_texts_list():
    """The 4 GiB test's argument on 300,000 bytes: plants of STAR_BIG's letters (and one q in front) on ACGT, the oracle on
    the plants' windows laid end to end, mapped back, is the oracle on the whole text -- for STAR_BIG, whose state an
    ACGT byte empties, and for STAR_BIG_TAINT, whose `.` holds through any run, long or short."""
    rng = np.random.default_rng(0x57A9)
    n = 300000
    text = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].copy()
    centre = 150000
    cluster, at = [], centre - 40
    while at < centre + 40:
        inst = lc.star_big_instance(rng)
        cluster.append((at, inst))
        at += len(inst)
    offs = lc.spread_offsets(0, n, 60, 64, rng, keep_clear=[(centre - 40, at)])
    last = lc.star_big_instance(rng)
    plants = [(5, b"q")] + cluster + [(p, lc.star_big_instance(rng)) for p in offs if p + 64 < n - 100] + [(n - len(last), last)]
    plan = lc.plan_plants(n, plants, lc.STAR_BIG_REACH)
    text[plan.idx] = plan.val
    text = text.tobytes()
    row, row_at, text_at = lc.row_of_windows(lambda lo, ln: text[lo:lo + ln], plan.windows)
    assert len(row) < n // 20
    for rx in (lc.STAR_BIG, lc.STAR_BIG_TAINT):
        whole = so.ends_numpy(text, rx)
        assert whole.size > 40 and int(whole[-1]) == n - 1
        assert np.array_equal(lc.row_to_text(so.ends_numpy(row, rx), row_at, text_at), whole)
    assert not lc.STAR_BIG.member[:, list(b"ACGT")].any()  # (no class of the untainted pattern holds a background letter)
    for longest in (False, True):  # the starts within a window of 64 bytes, for STAR_BIG
        whole = so.ends_numpy(text, lc.STAR_BIG)
        row_e = so.ends_numpy(row, lc.STAR_BIG)
        row_s = so.starts_numpy(row, lc.STAR_BIG, row_e, 64, longest)
        assert np.array_equal(lc.row_to_text(row_s.astype(np.int64), row_at, text_at),
                              so.starts_numpy(text, lc.STAR_BIG, whole, 64, longest).astype(np.int64))
    # the tainted pattern is tainted: on ACGT alone the upper bound keeps the `.`, the lower one has nothing
    k = so.masked(lc.STAR_BIG_TAINT)
    assert so.run(b"ACGT" * 64, k, k.all, True) != so.run(b"ACGT" * 64, k, 0, True) == 0
