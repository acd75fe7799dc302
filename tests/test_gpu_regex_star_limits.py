"""GPU suite for the regular-expression search with unbounded repetition (bmx_search_regex_star_device) at
the places a text of 64 KiB at the rule's piece does not reach:

a. a workgroup that takes SEVERAL tiles, tiles with more hits than the pool (walked twice: on the fast path the second walk
   repeats the pair warm-up, in R2 it reads the swept entry state again), every per-tile count around the pool size, a
   capacity that ends inside a dense tile, count-only calls, the sentinels behind the list of a tainted call;
b. pieces of 2^9 .. 2^12 ends: the walk's loop over up to 32 lines, ordinals up to 2^12 - 1 parked, R1 and R2 at these pieces;
c. the edge of the pair warm-up: the call is tainted exactly when a lane's bounds do not meet;
d. `lead` and `base_offset` on the slow path, and a workspace that grows, shrinks and grows;
e. positions past 2^32 on the product library, untainted and with one chain of pieces as long as the text;
f. starts of matches of exactly `window` and `window + 1` bytes.

Three modes: the fast path (the first launch alone), the slow path forced by "regex_star_force_slow", and the slow path a
naturally tainted call takes by itself (c.*[ab] with the one c at view byte 0).  Every comparison is the complete list
against tests/regex_star_oracle.py: positions, n_matches, the return code and the -1 sentinels behind the list.  Where
a geometry is forced, last_launch("regex_star") and regex_star_last() say that what ran is what was meant, and the number
of tainted waves is the one so.fast_taint predicts.  tests/test_limit_cases_cpu.py proves on the CPU what the cases
claim: per-tile counts, the window argument, predicted taint, and that a tainted case's first list and a sweep without
the column term both miss true ends.
"""
import numpy as np
import pytest

import limit_cases as lc
import regex_star_oracle as so
from test_gpu_regex import _struct
from test_gpu_search_limits import BIG_BASE, BIG_N, _big_plants, _dev
from test_gpu_tile_geometry import _Planted, _force, _full, _past_4g, _three_ways

pytestmark = pytest.mark.gpu

MODES = [(n, mode) for n in lc.STAR_FAST for mode in ("fast", "forced")] + [(n, "taint") for n in lc.STAR_TAINT]


def _predicted_waves(s: lc.Search, text: bytes, first: int, ps: int, mode: str) -> int:
    """The tainted waves of the first launch: none for the first family (proved on the CPU for every case), the model's for
    natural taint."""
    assert (mode == "taint") == bool(s.prefix)
    return so.fast_taint(text, s.rx, first, 0, ps, lc.star_warm(ps), walk=False).waves if s.prefix else 0


def _ran(c, ps: int, grid: int, tiles: int, mode: str, waves: int, what):
    """What the last call did: the forced geometry, the rule's warm-up, the path and the tainted waves."""
    last = c.regex_star_last()
    assert (last["piece_shift"], last["warm"]) == (ps, lc.star_warm(ps)), (what, last)
    assert last["slow"] == int(mode != "fast") and last["tainted"] == waves, (what, mode, waves, last)
    assert (waves > 0) == (mode == "taint"), (what, waves)
    assert c.last_launch("regex_star") == (ps, grid, tiles), (what, c.last_launch("regex_star"))


def _tile_case(c, case: lc.TileCase, mode: str, grids, cut: int):
    s = case.search
    ends, _ = s.ends(case.text)
    assert lc.bin_by_tile(ends, case.tile, case.first, len(case.counts)) == case.counts, case.name
    waves = _predicted_waves(s, case.text, case.first, case.ps, mode)
    d_text = _dev(c, case.text, case.first)
    for grid in grids:
        c.set_knob("tile_max_grid", grid)
        _three_ways(c, s, d_text, ends, None, cut, (case.name, mode, grid))
        _ran(c, case.ps, grid, len(case.counts), mode, waves, (case.name, grid))


# ---- a. several tiles per workgroup, counts around the pool ----------------------------------------------------------------

@pytest.mark.parametrize("name,mode", MODES)
def test_star_several_tiles_per_workgroup(exp_ctx, name, mode):
    """1, 2 and 3 workgroups over the fourteen tiles 3 / 2049 / 5 / 2048 / 2049 / 0 / 2047 and back, 64 KiB each, at pointer
    offsets 0, 1 and 15: count only, a capacity inside the second dense tile, room for all and 64 sentinels."""
    s = lc.STAR_SEARCHES[name]
    _force(exp_ctx, s, s.floor, 1)
    exp_ctx.set_knob("regex_star_force_slow", int(mode == "forced"))
    ran = 0
    for case in lc.star_geometry_cases(name):
        assert all(lc.tiles_per_workgroup_at_least(len(case.counts), g) >= 2 for g in lc.GRIDS)
        _tile_case(exp_ctx, case, mode, lc.GRIDS, lc.capacity_inside_second_dense(case))
        ran += 1
    assert ran == len(lc.OFFSETS)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("name,mode", [("star32", "fast"), ("taint32", "taint")])
def test_star_tiles_at_the_pool_edge(exp_ctx, name, mode, which):
    """Every per-tile count from 2040 to 2056, and 0, 1 and 4096, two workgroups: the first launch parks or walks twice with
    the pair warm-up in front, R2 with the state read from the swept array."""
    s = lc.STAR_SEARCHES[name]
    _force(exp_ctx, s, s.floor, 2)
    case = lc.star_count_case(name, which)
    dense = [t for t, c in enumerate(case.counts) if c > lc.STAGE][-1]  # the capacity ends inside the last dense tile
    _tile_case(exp_ctx, case, mode, (2,), case.prefix(dense) + case.counts[dense] // 2)


# ---- b. large pieces ---------------------------------------------------------------------------------------------------------

BOUNDARY_MODES = [(n, ps, mode) for n, ps in lc.STAR_BOUNDARY_CASES for mode in ("fast", "forced")] + \
    [(n, ps, "taint") for n, ps in lc.STAR_TAINT_BOUNDARY_CASES]


@pytest.mark.parametrize("name,ps,mode", BOUNDARY_MODES)
def test_star_large_pieces(exp_ctx, name, ps, mode):
    """limit_cases.boundary_case at pieces of 2^9 .. 2^12 ends (warm-ups of 64 .. 256 bytes), two workgroups over four
    tiles: hits on both sides of lane and tile boundaries, a parked lane with ordinals up to min(2^ps, 2000) - 1, a lane
    whose every end is a hit in a tile that is walked twice, an empty tile, hits up to the last byte."""
    case = lc.boundary_case(name, ps)
    s = case.search
    _force(exp_ctx, s, ps, 2)
    exp_ctx.set_knob("regex_star_force_slow", int(mode == "forced"))
    ends, _ = case.ends_by_windows()
    counts = lc.bin_by_tile(ends, case.tile, case.first, 4)
    assert lc.parked_lane_hits(ps) <= counts[0] <= lc.STAGE < counts[1] and counts[2] == 0
    waves = _predicted_waves(s, case.text, case.first, ps, mode)
    _three_ways(exp_ctx, s, _dev(exp_ctx, case.text, case.first), ends, None, counts[0] + counts[1] // 2, (case.name, mode))
    _ran(exp_ctx, ps, 2, 4, mode, waves, case.name)


# ---- c. the edge of the pair warm-up --------------------------------------------------------------------------------------------

def _full_list(c, d_text, rx, want, what, lead=0, base=0):
    """One call with room for all and 64 sentinels: total, list, sentinels."""
    import torch

    want = want[want >= lead] + base
    out = torch.full((want.size + 64,), -1, dtype=torch.int64, device=d_text.device)
    got, total = c.search_regex_star_device(d_text, _struct(rx), lead=lead, base_offset=base, out=out)
    assert total == want.size, (what, total, want.size)
    assert torch.equal(out[:total], torch.from_numpy(want).to(out.device)), what
    assert bool((out[total:] == -1).all()), what


def _warm_edge(c, ps, first, warm):
    rx = lc.STAR_EDGE.rx
    seen = set()
    for case in lc.warm_edge_cases(ps, first, warm):
        want = so.ends_numpy(case.text, rx)
        model = so.fast_taint(case.text, rx, first, case.lead, ps, case.warm, walk=False)
        assert model.waves == case.tainted_waves, case.name
        _full_list(c, _dev(c, case.text, first), rx, want, case.name, lead=case.lead)
        last = c.regex_star_last()
        assert (last["piece_shift"], last["warm"]) == (ps, case.warm), (case.name, last)
        assert last["tainted"] == model.waves and last["slow"] == int(model.waves != 0), (case.name, model.waves, last)
        seen.add(model.waves)
    assert seen == {0, 1}


@pytest.mark.parametrize("first", [0, 5, 15])
@pytest.mark.parametrize("ps", [8, 12])
def test_star_warm_up_edge(exp_ctx, ps, first):
    """c[ab]*d with the c one chunk inside the owning lane's warm-up, on its first chunk, one chunk in front of it and
    `warm` bytes exactly in front of start16, and a first lane whose warm-up begins at view byte 0 by rule or one chunk
    behind it: tainted exactly when the model says so, and the list exact either way."""
    _force(exp_ctx, lc.STAR_EDGE, ps, 0)
    _warm_edge(exp_ctx, ps, first, None)


@pytest.mark.parametrize("warm", [16, 4096])
def test_star_warm_up_edge_at_a_chosen_warm_up(exp_ctx, warm):
    _force(exp_ctx, lc.STAR_EDGE, 8, 0)
    exp_ctx.set_knob("regex_star_warm", warm)
    _warm_edge(exp_ctx, 8, 5, warm)


# ---- d. lead and base offset on the slow path -------------------------------------------------------------------------------------

LEAD_BASE = (1 << 41) + 3
LEAD_OFFSET = 5


def _lead_text(n: int, mode: str, seed: int):
    """(text, automaton).  Natural taint: c.*[ab], the one c at view byte 0, a letter in every fourth place.  Forced:
    a[ab]*b on runs of letters of about 30 bytes, so that chains cross the small pieces and `lead` falls inside matches."""
    rng = np.random.default_rng(seed)
    text = lc.background(n, seed)
    letters = np.frombuffer(b"ab", np.uint8)[rng.integers(0, 2, n)]
    keep = rng.random(n) < (0.25 if mode == "taint" else 0.97)
    text[keep] = letters[keep]
    if mode == "taint":
        text[0] = ord("c")
        return text.tobytes(), lc.STAR_SEARCHES["taint32"].rx
    return text.tobytes(), so.parse("a[ab]*b")


@pytest.mark.parametrize("mode", ["taint", "forced"])
@pytest.mark.parametrize("ps", [4, 8, 12])
def test_star_lead_and_base_offset_on_the_slow_path(exp_ctx, ps, mode):
    """R1 and the sweep run from aligned piece 0 whatever `lead` is; R2's first lane enters in the middle of a piece.
    `lead` at 0, 1, around a piece and a tile boundary (aligned coordinates), n - 1 and n; base_offset 2^41 + 3."""
    T, P, first = 256 << ps, 1 << ps, LEAD_OFFSET
    n = {4: 3 * T + 5, 8: 2 * T + 5, 12: T + 5 * P + 5}[ps]
    text, rx = _lead_text(n, mode, 0x1EAD + ps)
    want = so.ends_numpy(text, rx)
    assert want.size > n // 8 and int(want[-1]) >= n - 40
    exp_ctx.set_knob("regex_star_piece_shift", ps)
    exp_ctx.set_knob("regex_star_force_slow", int(mode == "forced"))
    d_text = _dev(exp_ctx, text, first)
    for lead in (0, 1, 3 * P - first - 1, 3 * P - first, 3 * P - first + 1, T - first - 1, T - first, T - first + 1, n - 1, n):
        _full_list(exp_ctx, d_text, rx, want, (ps, mode, lead), lead=lead, base=LEAD_BASE)
        last = exp_ctx.regex_star_last()
        if lead == n:  # (no end is owned: nothing is launched)
            assert last["slow"] == 0 and last["pieces"] == 0
            continue
        assert last["slow"] == 1 and last["piece_shift"] == ps and last["pieces"] == ((n + first - 1) >> ps) + 1, (lead, last)
        assert last["tainted"] > 0 or mode == "forced", (lead, last)
        tiles = ((n + first + T - 1) // T) - ((lead + first) // T)
        assert exp_ctx.last_launch("regex_star")[::2] == (ps, tiles), lead


def test_star_workspace_grows_shrinks_and_grows(exp_ctx):
    """One context, pieces of 16 bytes, naturally tainted texts of 64 KiB, 4 KiB and 1 MiB: the per-piece words, the
    columns and the scan's buffer are made, reused for the smaller call and made again for the larger one."""
    exp_ctx.set_knob("regex_star_piece_shift", 4)
    pieces = []
    for n in (64 << 10, 4 << 10, 1 << 20):
        text, rx = _lead_text(n, "taint", 0x6A0 + n)
        want = so.ends_numpy(text, rx)
        _full_list(exp_ctx, _dev(exp_ctx, text, 9), rx, want, n)
        last = exp_ctx.regex_star_last()
        assert last["slow"] == 1 and last["tainted"] > 0 and last["pieces"] == ((n + 9 - 1) >> 4) + 1, last
        assert last["columns"] >= last["pieces"] - 8, last  # (the `.` is unsure in front of every piece but the first few)
        pieces.append(last["pieces"])
    assert pieces[1] < pieces[0] < pieces[2]


# ---- e. past 2^32, product library ---------------------------------------------------------------------------------------------------

def _matching_instance(rng) -> bytes:
    while True:
        inst = lc.star_big_instance(rng)
        if inst[-1:] in (b"e", b"f"):
            return inst


@pytest.fixture(scope="module")
def star_big(ctx):
    """One text of BIG_N bytes of ACGT for the module: a q at byte 5, about 3400 strings (wx|y)z+[ef] matches over the
    whole text, 400 of them past 2^32, a row of them back to back across 2^32, one ending on the last byte."""
    import torch

    assert lc.STAR_BIG_REACH == 16
    rng = np.random.default_rng(0xB16 + 27)
    last = _matching_instance(rng)
    tail = [(BIG_N - 200, _matching_instance(rng)), (BIG_N - len(last), last)]
    plants = [(5, b"q")] + _big_plants(rng, lc.STAR_BIG_REACH, lambda: lc.star_big_instance(rng), tail,
                                       cluster_copy=lambda: _matching_instance(rng))
    text = _Planted(ctx, BIG_N, plants, 0x5EED4B27)
    yield text
    del text.d_text
    torch.cuda.empty_cache()


def test_star_text_beyond_4GiB(ctx, star_big):
    """(wx|y)z+[ef]: the whole list, then with base_offset 2^40 + 3 the list again and the shortest and the longest start
    within 64 bytes of every end past 2^32."""
    import torch

    rx, row = lc.STAR_BIG, star_big.row
    row_e = so.ends_numpy(row, rx)
    want = star_big.to_text(row_e)
    assert want.size > 2500 and _past_4g(want) and int(want[-1]) == BIG_N - 1
    out = torch.full((want.size + 64,), -1, dtype=torch.int64, device=star_big.d_text.device)
    _full(ctx.search_regex_star_device(star_big.d_text, _struct(rx), out=out), want, "star", out)
    out.fill_(-1)
    ends, total = ctx.search_regex_star_device(star_big.d_text, _struct(rx), base_offset=BIG_BASE, out=out)
    _full((ends, total), want + BIG_BASE, "star, base offset", out)
    high = want > (1 << 32)
    sel = ends[torch.from_numpy(high).to(ends.device)].contiguous()
    for longest in (False, True):
        row_s = so.starts_numpy(row, rx, row_e, 64, longest)
        assert not (row_s == np.uint64(so.NO_START)).any()
        s = ctx.regex_star_starts_device(star_big.d_text, _struct(rx), sel, window=64, longest=longest, base_offset=BIG_BASE)
        assert np.array_equal(s.cpu().numpy(), star_big.to_text(row_s.astype(np.int64))[high] + BIG_BASE), longest


def test_star_tainted_text_beyond_4GiB(ctx, exp_ctx, star_big):
    """q.*[ef] with the one q at byte 5: no lane's bounds meet, more than 2^20 pieces, one sweep lane carries the chain
    from the first piece to the last, R2 reads entry states for ends past 2^32.  The product library's full list; the
    experiments library, count only, says that it was the slow path over that many pieces."""
    import torch

    rx = lc.STAR_BIG_TAINT
    want = star_big.to_text(so.ends_numpy(star_big.row, rx))
    assert want.size > 2500 and _past_4g(want) and int(want[-1]) == BIG_N - 1
    out = torch.full((want.size + 64,), -1, dtype=torch.int64, device=star_big.d_text.device)
    _full(ctx.search_regex_star_device(star_big.d_text, _struct(rx), out=out), want, "tainted star", out)
    _, total = exp_ctx.search_regex_star_device(star_big.d_text, _struct(rx), capacity=0)
    last = exp_ctx.regex_star_last()
    assert total == want.size, (total, want.size)
    assert last["slow"] == 1 and last["piece_shift"] == 12 and last["pieces"] == ((BIG_N - 1) >> 12) + 1 > 1 << 20, last
    assert last["tainted"] > (BIG_N >> 20) and last["columns"] >= last["pieces"] - 8, last


# ---- f. starts at the window's edge ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("window", [16, 64, 65536])
def test_star_starts_at_the_windows_edge(ctx, window):
    """a[bc]*d: a match of exactly `window` bytes has its start, one of `window + 1` bytes has none; an end nearer to view
    byte 0 than the window has the start its match has inside the view, or none."""
    import torch

    rng = np.random.default_rng(window)
    rx = so.parse("a[bc]*d")

    def match(length):
        return b"a" + np.frombuffer(b"bc", np.uint8)[rng.integers(0, 2, length - 2)].tobytes() + b"d"

    text = b"bcd" + match(10) + b"x" * 7 + match(window) + b"xx" + match(window + 1) + b"x" + match(window - 1) + b"x" * 5 + match(2)
    want = so.ends_numpy(text, rx)
    assert want.size == 5 and int(want[0]) == 12 < window  # (the d at view byte 2 has no a in front of it: not an end)
    d_text = _dev(ctx, text, 3)
    got, total = ctx.search_regex_star_device(d_text, _struct(rx), capacity=want.size + 8)
    assert total == want.size and np.array_equal(got.cpu().numpy(), want)
    for longest in (False, True):
        ref = so.starts_numpy(text, rx, want, window, longest)
        lengths = np.where(ref == np.uint64(so.NO_START), 0, want.astype(np.uint64) - ref + np.uint64(1))
        assert {window, window - 1, 10, 2, 0} <= set(lengths.tolist()) and window + 1 not in lengths
        s = ctx.regex_star_starts_device(d_text, _struct(rx), torch.from_numpy(want).to(d_text.device), window=window, longest=longest)
        assert np.array_equal(s.cpu().numpy().astype(np.uint64), ref), (window, longest)
