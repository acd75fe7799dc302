"""GPU suite for the geometry of the searches over the tile frame (csrc/bmx_tile_frame.h: approximate, long approximate,
class-pattern, approximate over classes, gapped, k-mismatch, regular-expression) and of the dictionary search's loop of
the same shape (csrc/bmx_dict.hip), in the three regimes a text of a few MiB does not reach on a device with hundreds of
resident workgroups:

1. a workgroup that takes SEVERAL tiles, so that the pool, the lane bases and the tile words in LDS are the next tile's;
2. pieces of 2^9 .. 2^11 ends per lane in the Shift-And family (2^11 and 2^12 in the two approximate searches), with hits
   on tile and lane boundaries, a lane whose every end is a hit and a tile that is walked twice beside an empty one;
3. positions past 2^32 and base offsets past 2^40 in the four Shift-And searches and their reverse passes.

1 and 2 choose the geometry through libbmx_exp.so's knobs "tile_piece_shift" and "tile_max_grid" (include/bmx_exp.h), with
values the production rule can give the pattern; 3 runs the product library as it is.  Every comparison is the complete
list (positions, distances where the search has them, n_matches, the return code, the sentinels behind the list) against
the search's own oracle.  The per-tile counts and the properties of the texts are proved on the CPU by
tests/test_limit_cases_cpu.py; the texts are rebuilt for every pointer offset.
"""
import ctypes as C

import numpy as np
import pytest

import classes_oracle as co
import gaps_oracle as go
import hamming_oracle as ho
import limit_cases as lc
import regex_oracle as ro
from dict_oracle import dict_matches
from test_gpu_regex import _struct
from test_gpu_search_limits import _dev, _dict_raw, _ptr
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

pytestmark = pytest.mark.gpu


def _raw(ctx, s: lc.Search, d_text, out, dist, cap, base=0):
    """One call of search s over the whole view through the C ABI: (rc, n_matches)."""
    total = C.c_uint64(0)
    L, h, text, n = ctx._L, ctx._h, C.c_void_p(d_text.data_ptr()), d_text.numel()
    tail = (_ptr(out), cap, C.byref(total), None)
    tail_d = (_ptr(out), _ptr(dist), cap, C.byref(total), None)
    if s.kind in ("approx", "approx_long"):
        fn = L.bmx_search_approx_long_device if s.kind == "approx_long" else L.bmx_search_approx_device
        rc = fn(h, text, n, 0, base, s.pat, len(s.pat), s.k, *tail_d)
    elif s.kind in ("regex", "regex_star"):
        re_ = _struct(s.rx)
        fn = L.bmx_search_regex_star_device if s.kind == "regex_star" else L.bmx_search_regex_device
        rc = fn(h, text, n, 0, base, C.byref(re_), *tail)
    else:
        cls = co.pack(s.member)
        cp = C.c_void_p(cls.ctypes.data)
        if s.kind == "classes":
            rc = L.bmx_search_classes_device(h, text, n, n, base, cp, s.m, *tail)
        elif s.kind == "approx_classes":
            rc = L.bmx_search_approx_classes_device(h, text, n, 0, base, cp, s.m, s.k, *tail_d)
        elif s.kind == "hamming":
            rc = L.bmx_search_hamming_classes_device(h, text, n, n, base, cp, s.m, s.k, s.must, *tail_d)
        else:
            assert s.kind == "gaps"
            rc = L.bmx_search_gaps_device(h, text, n, 0, base, cp, s.m, s.optional, *tail)
    return rc, int(total.value)


def _force(ctx, s: lc.Search, ps: int, grid: int):
    """The knobs reach the sessions a context already has: one call of the search first, then the geometry."""
    assert s.floor <= ps <= s.cap  # (only what the production rule can give this pattern)
    rc, total = _raw(ctx, s, _dev(ctx, bytes(range(0x80, 0x100)) * 2), None, None, 0)
    assert (rc, total) == (host.OK, 0)
    ctx.set_knob("tile_piece_shift", ps)
    ctx.set_knob("tile_max_grid", grid)


def _launched(ctx, s: lc.Search):
    """(piece shift, workgroups, tiles) of the search's last launch (bmx_exp_last_launch)."""
    return ctx.last_launch("approx" if s.kind == "approx_classes" else s.kind)


def _expected(s: lc.Search, ends, dists):
    return ends - s.report, dists


def _three_ways(ctx, s, d_text, want_p, want_d, cut, what):
    """Count only (NULL outputs); a capacity of `cut` (the stored entries are the lowest, the slot at `cut` and all
    behind keep their sentinels); room for everything."""
    import torch

    total = want_p.size
    assert 0 < cut < total
    dev = d_text.device
    has_d = want_d is not None
    wp = torch.from_numpy(want_p).to(dev)
    wd = torch.from_numpy(want_d.astype(np.uint8)).to(dev) if has_d else None
    rc, t = _raw(ctx, s, d_text, None, None, 0)
    assert (rc, t) == (host.ERR_CAPACITY, total), (what, "count only", rc, t, total)
    out = torch.empty(total + 64, dtype=torch.int64, device=dev)
    dist = torch.empty(total + 64, dtype=torch.uint8, device=dev) if has_d else None
    for cap in (cut, total + 64):
        out.fill_(-1)
        if has_d:
            dist.fill_(255)
        rc, t = _raw(ctx, s, d_text, out, dist, cap)
        kept = min(cap, total)
        assert (rc, t) == (host.OK if cap >= total else host.ERR_CAPACITY, total), (what, cap, rc, t, total)
        assert torch.equal(out[:kept], wp[:kept]), (what, cap)
        assert bool((out[kept:] == -1).all()), (what, cap)
        if has_d:
            assert torch.equal(dist[:kept], wd[:kept]) and bool((dist[kept:] == 255).all()), (what, cap)


# ---- 1. several tiles per workgroup ------------------------------------------------------------------------------------

GEOMETRY_NAMES = [n for n in lc.SEARCHES if not n.endswith("_run")]


@pytest.mark.parametrize("name", GEOMETRY_NAMES)
def test_several_tiles_per_workgroup(exp_ctx, name):
    """1, 2 and 3 workgroups over the tiles 3 / 2049 / 5 / 2048 / 2049 / 0 / 2047 and the same backwards (the long
    approximate search: the first eight of them, 1 MiB), at the pattern's smallest piece, at pointer offsets 0, 1 and 15:
    one workgroup walks a dense tile twice and then parks a sparse, a full or an empty one, and the other way round."""
    s = lc.SEARCHES[name]
    _force(exp_ctx, s, s.floor, 1)
    ran = 0
    for case in lc.geometry_cases(name):
        ends, dists = s.ends(case.text)
        assert lc.bin_by_tile(ends, case.tile, case.first, len(case.counts)) == case.counts
        want_p, want_d = _expected(s, ends, dists)
        d_text = _dev(exp_ctx, case.text, case.first)
        for grid in lc.GRIDS:
            assert lc.tiles_per_workgroup_at_least(len(case.counts), grid) >= 2
            exp_ctx.set_knob("tile_max_grid", grid)
            _three_ways(exp_ctx, s, d_text, want_p, want_d, lc.capacity_inside_second_dense(case), (case.name, grid))
            assert _launched(exp_ctx, s) == (s.floor, grid, len(case.counts)), (case.name, grid)  # what was forced is what ran
            ran += 1
    assert ran == len(lc.OFFSETS) * len(lc.GRIDS)


def test_several_tiles_per_workgroup_dict(exp_ctx):
    """The dictionary search's loop with 1, 2 and 3 workgroups over the same fourteen tiles (two pairs per position)."""
    import torch

    patterns, _ = lc.dict_variant("two")
    with exp_ctx.dictionary(patterns) as d:
        rc, total = _dict_raw(exp_ctx, d, _dev(exp_ctx, bytes(range(0x80, 0xC0))), None, None, 0)
        assert (rc, total) == (host.OK, 0)
        for first in lc.OFFSETS:
            case = lc.dict_geometry_case(first)
            want_p, want_i = dict_matches(case.text, patterns)
            assert lc.bin_by_tile(want_p, case.tile, first, len(case.counts)) == case.counts
            d_text = _dev(exp_ctx, case.text, first)
            total = want_p.size
            wp, wi = torch.from_numpy(want_p).to(d_text.device), torch.from_numpy(want_i.astype(np.int32)).to(d_text.device)
            out = torch.empty(total + 64, dtype=torch.int64, device=d_text.device)
            pid = torch.empty(total + 64, dtype=torch.int32, device=d_text.device)
            for grid in lc.GRIDS:
                exp_ctx.set_knob("tile_max_grid", grid)
                rc, t = _dict_raw(exp_ctx, d, d_text, None, None, 0)
                assert (rc, t) == (host.ERR_CAPACITY, total), (first, grid)
                for cap in (lc.capacity_inside_second_dense(case), total + 64):
                    out.fill_(-1)
                    pid.fill_(-1)
                    rc, t = _dict_raw(exp_ctx, d, d_text, out, pid, cap)
                    kept = min(cap, total)
                    assert (rc, t) == (host.OK if cap >= total else host.ERR_CAPACITY, total), (first, grid, cap)
                    assert torch.equal(out[:kept], wp[:kept]) and torch.equal(pid[:kept], wi[:kept]), (first, grid, cap)
                    assert bool((out[kept:] == -1).all()) and bool((pid[kept:] == -1).all()), (first, grid, cap)
                assert exp_ctx.last_launch("dict") == (6, grid, len(case.counts)), (first, grid)


# ---- 2. large pieces -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,ps", lc.BOUNDARY_CASES)
def test_large_pieces(exp_ctx, name, ps):
    """Pieces of 2^ps ends, two workgroups over four tiles (three and 5 bytes, at pointer offset 11): hits on both sides
    of lane and tile boundaries; lane 150 of tile 0 with a hit at each of its first min(2^ps, 2000) ends while the tile
    stays inside the pool, so that ordinals up to 2^ps - 1 (1999 at ps 11 and 12) are parked and read back, beside a
    distance that is not the same for the whole lane; lane 100 of tile 1 with a hit at every end in a tile that is walked
    twice (the second walk writes them); tile 2 empty; hits up to the last byte.  The expected
    list is the oracle's on the windows around the plants, which test_limit_cases_cpu.py shows to be the whole text's."""
    case = lc.boundary_case(name, ps)
    s = case.search
    _force(exp_ctx, s, ps, 2)
    ends, dists = case.ends_by_windows()
    counts = lc.bin_by_tile(ends, case.tile, case.first, 4)
    assert lc.parked_lane_hits(ps) - s.k <= counts[0] <= lc.STAGE < counts[1] and counts[2] == 0
    want_p, want_d = _expected(s, ends, dists)
    cut = counts[0] + counts[1] // 2
    _three_ways(exp_ctx, s, _dev(exp_ctx, case.text, case.first), want_p, want_d, cut, case.name)
    assert _launched(exp_ctx, s) == (ps, 2, 4)


# ---- 5. the switches themselves ------------------------------------------------------------------------------------------

def test_switches_reject_what_is_out_of_range(exp_ctx):
    for name, value in (("tile_piece_shift", 5), ("tile_piece_shift", 13), ("tile_piece_shift", -1), ("tile_max_grid", -1),
                        ("tile_geometry", 1)):
        with pytest.raises(host.BmxError) as e:
            exp_ctx.set_knob(name, value)
        assert e.value.rc == host.ERR_ARG, (name, value)
    for value in (0, 6, 12, 0):
        exp_ctx.set_knob("tile_piece_shift", value)
    exp_ctx.set_knob("tile_max_grid", 0)
    with exp_ctx.dictionary([b"ab"]) as d:  # a dictionary tile is at most 2^5 rounds: 11 is the most its session takes
        rc, _ = _dict_raw(exp_ctx, d, _dev(exp_ctx, b"xxabxx"), None, None, 0)
        assert rc == host.ERR_CAPACITY
        exp_ctx.set_knob("tile_piece_shift", 11)
        with pytest.raises(host.BmxError) as e:
            exp_ctx.set_knob("tile_piece_shift", 12)
        assert e.value.rc == host.ERR_ARG
        want_p, want_i = dict_matches(b"xxabxx" * 50000, [b"ab"])
        pos, pid, total = d.search_device(_dev(exp_ctx, b"xxabxx" * 50000, 3), capacity=want_p.size)
        assert total == want_p.size and np.array_equal(pos.cpu().numpy(), want_p)


@pytest.mark.parametrize("name", ["classes32", "hamming64x4", "approx64"])
def test_zero_restores_the_production_geometry(ctx, exp_ctx, name):
    """Forced to pieces of 2^9 and one workgroup, then both switches back at 0: the lists are the product library's."""
    import torch

    s = lc.SEARCHES[name]
    case = lc.search_tile_case(s, lc.SEQUENCE, 9, 1)
    ends, dists = s.ends(case.text)
    want_p, want_d = _expected(s, ends, dists)
    lists = []
    for c, forced in ((exp_ctx, True), (exp_ctx, False), (ctx, False)):
        d_text = _dev(c, case.text, case.first)
        if forced:
            _force(c, s, 9, 1)
        elif c is exp_ctx:
            c.set_knob("tile_piece_shift", 0)
            c.set_knob("tile_max_grid", 0)
        out = torch.full((want_p.size + 64,), -1, dtype=torch.int64, device=d_text.device)
        dist = torch.full((want_p.size + 64,), 255, dtype=torch.uint8, device=d_text.device) if want_d is not None else None
        rc, total = _raw(c, s, d_text, out, dist, out.numel())
        assert (rc, total) == (host.OK, want_p.size), (name, forced)
        if c is exp_ctx:  # one workgroup over seven tiles of 256 << 9 ends, then the rule's piece and a workgroup per tile
            shift, grid, tiles = _launched(c, s)
            assert (shift, grid, tiles) == ((9, 1, 7) if forced else (s.floor, tiles, 7 << (9 - s.floor))), (name, forced)
        lists.append((out.cpu().numpy(), None if dist is None else dist.cpu().numpy()))
    for got_p, got_d in lists:
        assert np.array_equal(got_p, lists[-1][0]) and (got_d is None or np.array_equal(got_d, lists[-1][1]))
    assert np.array_equal(lists[-1][0][:want_p.size], want_p) and bool((lists[-1][0][want_p.size:] == -1).all())


# ---- 3. past 2^32 and 2^40: the Shift-And searches and their reverse passes, product library ---------------------------------

BIG_REACH = 16  # no match of the patterns below is longer, edits included
P_CLASSES = co.parse("[ab][cd]e[fg]h")
P_HAMMING = (co.singletons(b"klmnopqrstuv"), 2)
P_GAPS = go.parse("[ab][cd]?[ef]{1,3}")
P_REGEX = ro.parse("(wx|y)z{1,2}[ef]")


def _instance(rng, which: int) -> bytes:
    """A string one of the four patterns matches (the k-mismatch pattern: with 0 to 3 substitutions)."""
    buf = np.full(32, ord("z"), np.uint8)
    if which == 0:
        end = go.plant(rng, buf, P_CLASSES, 0, 0)
    elif which == 1:
        pat = bytearray(b"klmnopqrstuv")
        for i in rng.choice(len(pat), int(rng.integers(0, 4)), replace=False):
            pat[i] = ord("Z")
        return bytes(pat)
    elif which == 2:
        end = go.plant(rng, buf, P_GAPS[0], P_GAPS[1], 0)
    else:
        end = ro.plant_path(rng, buf, P_REGEX, 0)
    return buf[:end].tobytes()


class _Planted:
    """A device text of ACGT (no pattern above holds one of these letters) with instances planted in it, and the plants'
    windows laid end to end on the host: every hit lies in a window, a window begins and ends with BIG_REACH bytes of
    background, so an oracle on the row of windows finds the text's hits and no other."""

    def __init__(self, ctx, n: int, plants, seed: int):
        import torch

        self.n = n
        plan = lc.plan_plants(n, plants, BIG_REACH)
        assert max(plan.val) < 0x80 and not set(b"ACGT") & set(plan.val.tolist())
        self.d_text = torch.empty(n, dtype=torch.uint8, device=f"cuda:{ctx.device}")
        ctx.gen_text(self.d_text, 0, seed, kind=1)
        step = 1 << 30
        for a in range(0, n, step):
            lo, hi = np.searchsorted(plan.idx, [a, min(a + step, n)])
            if hi > lo:
                self.d_text[a:a + step][torch.from_numpy(plan.idx[lo:hi] - a).to(self.d_text.device)] = \
                    torch.from_numpy(plan.val[lo:hi]).to(self.d_text.device)
        self.windows = plan.windows
        rows = [self.d_text[lo:lo + ln].cpu().numpy() for lo, ln in plan.windows]
        self.row = np.concatenate(rows).tobytes()
        self.row_at = np.cumsum([0] + [ln for _, ln in plan.windows])  # where window i begins in the row
        self.text_at = np.array([lo for lo, _ in plan.windows], np.int64)
        for lo, ln in plan.windows:  # (what the argument above rests on)
            assert lo == 0 or lo + ln == n or ln >= 2 * BIG_REACH  # (clipped only at the text's two ends: the row's too)

    def to_text(self, row_pos):
        """Row positions -> text positions."""
        row_pos = np.asarray(row_pos, np.int64)
        w = np.searchsorted(self.row_at, row_pos, side="right") - 1
        return row_pos - self.row_at[w] + self.text_at[w]


@pytest.fixture(scope="module")
def big(ctx):
    """One text of BIG_N bytes for the module: about 3400 instances of the four patterns over the whole text, 400 of
    them past 2^32, a row of them back to back across 2^32, and one of each in the last 200 bytes, the last one ending on
    the last byte (at this size a tile is 512 KiB of ends: the last tile holds the text's last 5 bytes)."""
    import torch

    from test_gpu_search_limits import BIG_N, _big_plants

    rng = np.random.default_rng(0xB16 + 4)
    last = _instance(rng, 0)
    tail = [(BIG_N - 200 + 50 * j, _instance(rng, j)) for j in (1, 2, 3)] + [(BIG_N - len(last), last)]
    turn = iter(range(1 << 30))
    plants = _big_plants(rng, BIG_REACH, lambda: _instance(rng, next(turn) % 4), tail)
    text = _Planted(ctx, BIG_N, plants, 0x5EED4B16)
    yield text
    del text.d_text
    torch.cuda.empty_cache()


def _past_4g(pos):
    return int((pos > (1 << 32)).sum()) > 50 and int((pos < (1 << 32)).sum()) > 100 and \
        int(((pos >= (1 << 32) - 40) & (pos <= (1 << 32) + 40)).sum()) >= 2


def _full(out_total, want, what, sentinel_of=None):
    got, total = out_total
    assert total == want.size, (what, total, want.size)
    assert np.array_equal(got.cpu().numpy().astype(np.int64), want), what
    if sentinel_of is not None:
        assert bool((sentinel_of[total:] == -1).all()), what


def test_classes_text_beyond_4GiB(ctx, big):
    """The class search's whole list, and the starts of the approximate search over the same classes (k = 1) for its ends
    past 2^32 (bmx_approx_spans_classes_device)."""
    import torch

    from spans_oracle import span_starts

    m = len(P_CLASSES)
    want = big.to_text(co.class_starts(big.row, P_CLASSES))
    assert want.size > 700 and _past_4g(want) and int(want[-1]) == big.n - m
    out = torch.full((want.size + 64,), -1, dtype=torch.int64, device=big.d_text.device)
    _full(ctx.search_classes_device(big.d_text, co.pack(P_CLASSES), out=out), want, "classes", out)
    row_e, row_d = co.class_approx_ends(big.row, P_CLASSES, 1)
    want_e = big.to_text(row_e)
    e, d, total = ctx.search_approx_classes_device(big.d_text, co.pack(P_CLASSES), 1, capacity=want_e.size + 64)
    assert total == want_e.size and np.array_equal(e.cpu().numpy(), want_e) and np.array_equal(d.cpu().numpy(), row_d)
    high = want_e > (1 << 32)
    assert int(high.sum()) > 150
    row_s, row_sd = span_starts(big.row, P_CLASSES, 1, row_e[high])
    sel = torch.from_numpy(np.nonzero(high)[0]).to(e.device)
    s, e2, d2, t = ctx.approx_spans_device(big.d_text, co.pack(P_CLASSES), 1, e[sel].contiguous(), d[sel].contiguous())
    assert t == int(high.sum()) and np.array_equal(row_sd, row_d[high])
    assert np.array_equal(s.cpu().numpy(), big.to_text(row_s)), "starts past 2^32"


def test_hamming_text_beyond_4GiB(ctx, big):
    import torch

    member, k = P_HAMMING
    row_s, row_d = ho.hamming_starts(big.row, member, k)
    want = big.to_text(row_s)
    assert want.size > 300 and _past_4g(want) and set(row_d.tolist()) == {0, 1, 2}
    out = torch.full((want.size + 64,), -1, dtype=torch.int64, device=big.d_text.device)
    dist = torch.full((want.size + 64,), 255, dtype=torch.uint8, device=big.d_text.device)
    s, d, total = ctx.search_hamming_device(big.d_text, co.pack(member), k, out=out, dist_out=dist)
    _full((s, total), want, "hamming", out)
    assert np.array_equal(d.cpu().numpy().astype(np.int64), row_d) and bool((dist[total:] == 255).all())


def test_gaps_text_beyond_4GiB(ctx, big):
    """The gapped search's whole list; then, for its ends past 2^32, the shortest and the longest match's start."""
    import torch

    member, optional = P_GAPS
    want = big.to_text(go.gap_ends(big.row, member, optional))
    assert want.size > 1000 and _past_4g(want)
    out = torch.full((want.size + 64,), -1, dtype=torch.int64, device=big.d_text.device)
    ends, total = ctx.search_gaps_device(big.d_text, (co.pack(member), optional), out=out)
    _full((ends, total), want, "gaps", out)
    high = want > (1 << 32)
    for longest in (False, True):
        row_e, row_s = go.gap_starts(big.row, member, optional, longest)
        s = ctx.gaps_starts_device(big.d_text, (co.pack(member), optional), ends[torch.from_numpy(high).to(ends.device)].contiguous(),
                                   longest=longest)
        assert np.array_equal(s.cpu().numpy(), big.to_text(np.asarray(row_s, np.int64))[high]), longest


def test_regex_text_beyond_4GiB(ctx, big):
    import torch

    want = big.to_text(ro.ends_numpy(big.row, P_REGEX))
    assert want.size > 700 and _past_4g(want)
    out = torch.full((want.size + 64,), -1, dtype=torch.int64, device=big.d_text.device)
    ends, total = ctx.search_regex_device(big.d_text, _struct(P_REGEX), out=out)
    _full((ends, total), want, "regex", out)
    high = want > (1 << 32)
    for longest in (False, True):
        row_e, row_s = ro.starts_numpy(big.row, P_REGEX, longest)
        s = ctx.regex_starts_device(big.d_text, _struct(P_REGEX), ends[torch.from_numpy(high).to(ends.device)].contiguous(),
                                    longest=longest)
        assert np.array_equal(s.cpu().numpy(), big.to_text(np.asarray(row_s, np.int64))[high]), longest


# ... shards with a base offset past 2^40

SHARD_N = (2 << 20) + 3
SHARD_CUTS = [0, 700003, 700004, 1500000, SHARD_N]


@pytest.fixture(scope="module")
def shard_text():
    """2 MiB of ACGT with an instance about every 600 bytes, and every search's whole list."""
    rng = np.random.default_rng(0x5A4D)
    text = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, SHARD_N)].copy()
    at, j = 7, 0
    while at < SHARD_N - 40:
        inst = np.frombuffer(_instance(rng, j % 4), np.uint8)
        text[at:at + inst.size] = inst
        at += inst.size + int(rng.integers(0, 1200))
        j += 1
    for cut in SHARD_CUTS[1:-1]:  # matches across the cuts
        inst = np.frombuffer(_instance(rng, 2) + _instance(rng, 3) + _instance(rng, 0) + _instance(rng, 1), np.uint8)
        text[cut - 9:cut - 9 + inst.size] = inst
    return text.tobytes()


@pytest.mark.parametrize("offset", [0, 7])
def test_shards_with_a_base_offset_past_2_40(ctx, shard_text, offset):
    """base_offset = 2^40 + 3: the class and the k-mismatch search over views with a halo of m - 1 bytes behind n_own, the
    gapped and the regex search over views that begin their longest match less one byte before their first end; the
    lists of the shards concatenate to the oracle's of the whole text plus the offset, and so do the starts the reverse
    passes give for each shard's ends."""
    import torch

    from spans_oracle import span_starts
    from test_gpu_search_limits import BIG_BASE

    text = shard_text
    n = len(text)
    d_text = _dev(ctx, text, offset)
    cuts = list(zip(SHARD_CUTS[:-1], SHARD_CUTS[1:]))

    def cat(parts):
        return np.concatenate([p.cpu().numpy().astype(np.int64) for p in parts])

    # class search: starts in [a, b), halo m - 1
    m = len(P_CLASSES)
    want = co.class_starts(text, P_CLASSES)
    got = [ctx.search_classes_device(d_text[a:min(b + m - 1, n)], co.pack(P_CLASSES), n_own=b - a, base_offset=BIG_BASE + a)[0]
           for a, b in cuts]
    assert want.size > 500 and np.array_equal(cat(got), want + BIG_BASE), "classes"
    # k-mismatch search
    member, k = P_HAMMING
    want_s, want_d = ho.hamming_starts(text, member, k)
    parts = [ctx.search_hamming_device(d_text[a:min(b + len(member) - 1, n)], co.pack(member), k, n_own=b - a, base_offset=BIG_BASE + a)
             for a, b in cuts]
    assert want_s.size > 300 and np.array_equal(cat([p[0] for p in parts]), want_s + BIG_BASE), "hamming"
    assert np.array_equal(cat([p[1] for p in parts]), want_d)
    # gapped search and its starts
    member, optional = P_GAPS
    pair = (co.pack(member), optional)
    lead_of = lambda a, reach: min(a, reach - 1)
    want = go.gap_ends(text, member, optional)
    views = [(a - lead_of(a, len(member)), b, lead_of(a, len(member))) for a, b in cuts]
    ends = [ctx.search_gaps_device(d_text[v:b], pair, lead=lead, base_offset=BIG_BASE + v)[0] for v, b, lead in views]
    assert want.size > 1000 and np.array_equal(cat(ends), want + BIG_BASE), "gaps"
    for longest in (False, True):
        starts = [ctx.gaps_starts_device(d_text[v:b], pair, e, longest=longest, base_offset=BIG_BASE + v)
                  for (v, b, _), e in zip(views, ends)]
        assert np.array_equal(cat(starts), np.asarray(go.gap_starts(text, member, optional, longest)[1], np.int64) + BIG_BASE), longest
    # regex search and its starts
    re_ = _struct(P_REGEX)
    want = ro.ends_numpy(text, P_REGEX)
    views = [(a - lead_of(a, P_REGEX.max_len), b, lead_of(a, P_REGEX.max_len)) for a, b in cuts]
    ends = [ctx.search_regex_device(d_text[v:b], re_, lead=lead, base_offset=BIG_BASE + v)[0] for v, b, lead in views]
    assert want.size > 500 and np.array_equal(cat(ends), want + BIG_BASE), "regex"
    for longest in (False, True):
        starts = [ctx.regex_starts_device(d_text[v:b], re_, e, longest=longest, base_offset=BIG_BASE + v)
                  for (v, b, _), e in zip(views, ends)]
        assert np.array_equal(cat(starts), np.asarray(ro.starts_numpy(text, P_REGEX, longest)[1], np.int64) + BIG_BASE), longest
    # approximate search over the classes (k = 1) and the starts of its matches
    reach = m + 1
    want_e, want_d = co.class_approx_ends(text, P_CLASSES, 1)
    want_st, _ = span_starts(text, P_CLASSES, 1, want_e)
    views = [(a - lead_of(a, reach), b, lead_of(a, reach)) for a, b in cuts]
    got_e, got_s = [], []
    for v, b, lead in views:
        e, d, total = ctx.search_approx_classes_device(d_text[v:b], co.pack(P_CLASSES), 1, lead=lead, base_offset=BIG_BASE + v)
        s, _, _, t = ctx.approx_spans_device(d_text[v:b], co.pack(P_CLASSES), 1, e, d, base_offset=BIG_BASE + v)
        assert t == total
        got_e.append(e), got_s.append(s)
    assert np.array_equal(cat(got_e), want_e + BIG_BASE) and np.array_equal(cat(got_s), want_st + BIG_BASE), "approx over classes"
