"""GPU suite for the begins search and the ends pass of expressions with * + {a,} (bmx_search_regex_star_begins_device /
bmx_regex_star_ends_device and their host-buffer forms) and for ``posix=True`` with ``kind="regex_star"``: full lists compared
with tests/regex_star_begins_oracle.py on the fast path, on the slow path forced by the experiments knob and on the slow
path a tainted call takes by itself."""
import ctypes as C

import numpy as np
import pytest

import classes_oracle as co
import regex_oracle as ro
import regex_star_begins_oracle as sb
import regex_star_oracle as so
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

pytestmark = pytest.mark.gpu

NONE = np.uint64(sb.NONE)


def _dev(ctx, data, offset: int = 0, behind: bytes = b""):
    """data on the device, starting `offset` bytes into a buffer (any alignment); ``behind`` lies right behind the view."""
    import torch

    data = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data
    buf = torch.zeros((data.size + offset + len(behind) + 32,), dtype=torch.uint8, device=f"cuda:{ctx.device}")
    both = np.concatenate([data, np.frombuffer(behind, np.uint8)])
    if both.size:
        buf[offset:offset + both.size] = torch.from_numpy(both.copy()).to(buf.device)
    return buf[offset:offset + data.size]


def _struct(rx) -> host.Regex:
    r = host.Regex()
    r.m, r.first, r.last = rx.m, rx.first, rx.last
    for i, f in enumerate(rx.follow):
        r.follow[i] = f
    packed = co.pack(rx.member).tobytes()
    C.memmove(r.classes, packed, len(packed))
    return r


def _gpu(ctx, d_text, rx, **kw):
    n = kw.get("n", d_text.numel())
    cap = kw.pop("capacity", max(n, 1))
    starts, total = ctx.search_regex_star_begins_device(d_text, rx if isinstance(rx, host.Regex) else _struct(rx), capacity=cap, **kw)
    return starts.cpu().numpy().astype(np.int64), total


def _check(ctx, text, rx, offset=0, what=None, behind=b""):
    text = bytes(text)
    want = sb.begins_numpy(text, rx)
    got, total = _gpu(ctx, _dev(ctx, text, offset, behind), rx)
    assert total == want.size, (what, len(text), rx.m, offset, total, want.size)
    assert np.array_equal(got, want), (what, len(text), rx.m, offset)
    return want


def _planted(rng, rx, n, base=0x61, sigma=4, copies=6):
    text = (rng.integers(0, sigma, n) + base).astype(np.uint8)
    for _ in range(copies):
        if n:
            so.plant_path(rng, text, rx, int(rng.integers(0, n)), stop=0.1)
    return text


# ---- against the oracles ---------------------------------------------------------------------------------------------

def test_random_cyclic_expressions_at_every_alignment_and_length(ctx):
    """256 expressions with a cycle, one for each of the 16 alignments of the view x the 16 lengths mod 16; the bytes behind
    the view continue its text with more planted matches, so they would complete or extend matches."""
    rng = np.random.default_rng(0x5B7A00)
    lengths, empty = set(), 0
    for case in range(256):
        sigma = (2, 4, 95)[case % 3]
        base = 0x20 if sigma == 95 else 0x61
        n = (int(rng.integers(0, 130 if case % 10 else 3)) << 4) + case // 16
        expr, rx = so.random_regex(rng, np.arange(base, base + sigma), max_m=(8, 32, 64)[case % 7 % 3], cyclic=True)
        whole = _planted(rng, rx, n + 40, base, sigma, copies=8)
        want = _check(ctx, whole[:n], rx, offset=case % 16, what=expr, behind=whole[n:].tobytes())
        lengths.add((case % 16, n % 16))
        empty += want.size == 0
    assert len(lengths) == 256
    assert 4 * empty < 256, empty


@pytest.mark.parametrize("expr", ["a+", "x{31}a+", "x{32}a+", "x{63}a+", "a+x{31}", "a+x{32}", "zy+x{30}", "zy+x{31}", "zy+x{32}",
                                  "z(abcd)+x{30}", "y(x{32})+", "dx{20}(a|bc)+x{20}"])
def test_word_widths_loops_and_back_edges(ctx, expr):
    """m = 1, 32, 33 and 64; a+x{31} / a+x{32} put the self-loop on bit 31 / 32 of the REVERSED automaton; back edges that
    cross the word halves; with and without irregular positions."""
    rng = np.random.default_rng(len(expr) * 977)
    rx = so.parse(expr)
    text = _planted(rng, rx, 3000, sigma=3, copies=10)
    text[rng.integers(0, 3000, 300)] = ord("x")
    want = _check(ctx, text, rx, offset=5, what=expr, behind=b"x" * 40)
    assert want.size > 0, expr


def test_a_star_free_automaton_gives_the_begins_searchs_list(ctx):
    rng = np.random.default_rng(0x5B7A01)
    for case in range(20):
        expr, rx = ro.random_regex(rng, np.arange(97, 101), 12)
        text = (rng.integers(0, 4, 3000 + case) + 97).astype(np.uint8)
        d_text = _dev(ctx, text, case % 16)
        re_ = host.compile_regex(expr)
        a, ta = ctx.search_regex_begins_device(d_text, re_, capacity=4000)
        b, tb = ctx.search_regex_star_begins_device(d_text, re_, capacity=4000)
        assert ta == tb and np.array_equal(a.cpu().numpy(), b.cpu().numpy()), expr


# ---- fast against slow -----------------------------------------------------------------------------------------------

def _forced(c, text, rx, offset=0, **kw):
    c.set_knob("regex_star_begins_force_slow", 1)
    got = _gpu(c, _dev(c, text, offset), rx, **kw)
    last = c.regex_star_begins_last()
    c.set_knob("regex_star_begins_force_slow", 0)
    assert last["slow"] == 1
    return got, last


@pytest.mark.parametrize("ps,grid", [(4, 1), (5, 2), (6, 3)])
def test_forced_slow_path_equals_fast_path_equals_oracle(exp_ctx, ps, grid):
    """64 KiB, pieces of 16 to 64 bytes and one to three workgroups: chains cross pieces, tiles and workgroups."""
    rng = np.random.default_rng(0x5B7A10 + ps)
    exp_ctx.set_knob("regex_star_begins_piece_shift", ps)
    _gpu(exp_ctx, _dev(exp_ctx, b"abc"), so.parse("a+"))  # (the shared geometry knobs reach the sessions a context already has)
    exp_ctx.set_knob("tile_max_grid", grid)
    n = (1 << 16) - 3
    for case, expr in enumerate(["c[ab]+", "a(b|cd)*a", "a.*d", "[cd]{2,}(ab|ba)+", r"[ab]+c[ab]+", "c(a|b)+x{33}"]):
        rx = so.parse(expr)
        text = _planted(rng, rx, n, sigma=4, copies=40)
        want = sb.begins_numpy(text, rx)
        (slow, total), last = _forced(exp_ctx, text, rx, offset=case)
        assert last["piece_shift"] == ps and exp_ctx.last_launch("regex_star_begins")[:2] == (ps, grid), last
        assert last["pieces"] == ((n + case - 1) >> ps) + 1
        assert total == want.size and np.array_equal(slow, want), (expr, ps)
        fast, total = _gpu(exp_ctx, _dev(exp_ctx, text, case), rx)
        assert total == want.size and np.array_equal(fast, want), (expr, ps)
        assert want.size > 0, expr
    exp_ctx.set_knob("tile_max_grid", 0)
    exp_ctx.set_knob("regex_star_begins_piece_shift", 0)


def test_natural_taint_takes_the_slow_path_and_is_exact(exp_ctx):
    """[ab].*c with the one c on the view's last byte: above every lane but the highest the lower bound knows no c, the
    upper bound keeps the loop.  Then the dense .*a: every start in front of the last a is a hit, the tiles are dense, the
    second walk writes downwards, and capacities cut the list short."""
    rng = np.random.default_rng(0x5B7A20)
    n = (1 << 16) + 11
    rx = so.parse("[ab].*c")
    text = (rng.integers(0, 3, n) + 0x61).astype(np.uint8)
    text[text == ord("c")] = ord("d")
    text[n - 1] = ord("c")
    want = sb.begins_numpy(text, rx)
    assert want.size > 20000
    for offset in (0, 9):
        got, total = _gpu(exp_ctx, _dev(exp_ctx, text, offset), rx)
        last = exp_ctx.regex_star_begins_last()
        assert last["tainted"] > 0 and last["slow"] == 1 and last["columns"] > 0, last
        assert total == want.size and np.array_equal(got, want), offset
    rx = so.parse(".*a")
    text = np.full(n, ord("x"), np.uint8)
    text[n - 300] = ord("a")
    want = np.arange(n - 299, dtype=np.int64)
    d_text = _dev(exp_ctx, text, 3)
    got, total = _gpu(exp_ctx, d_text, rx)
    assert exp_ctx.regex_star_begins_last()["slow"] == 1
    assert total == want.size and np.array_equal(got, want)
    for cap in (0, 1, 2047, 2049, 5000):
        import torch

        out = torch.full((cap + 8,), -7, dtype=torch.int64, device=d_text.device)
        s, total = exp_ctx.search_regex_star_begins_device(d_text, _struct(rx), out=out, capacity=cap)
        assert total == want.size and np.array_equal(s.cpu().numpy(), want[:cap]), cap
        assert (out[cap:] == -7).all(), cap  # nothing past the capacity


@pytest.mark.parametrize("ps", [8, 12])
def test_warm_up_edge(exp_ctx, ps):
    """c[ab]*d with the d at warm - 16, warm - 1, warm, warm + 1 and warm + 16 bytes above the owning lane's roundup16(hi):
    inside the warm-up both bounds see the d and meet; above it only the upper bound keeps the loop.  ``tainted`` is the
    model's wave count and the list is exact either way."""
    exp_ctx.set_knob("regex_star_begins_piece_shift", ps)
    rx = so.parse("c[ab]*d")
    piece = 1 << ps
    warm = max(64, piece // 16)
    n = 40 * piece + 77
    seen = set()
    for offset in (0, 5):
        for delta in (warm - 16, warm - 1, warm, warm + 1, warm + 16):
            text = np.full(n, ord("x"), np.uint8)  # (one x empties both bounds: no other lane is unsure)
            lane_hi = 7 * piece  # aligned coordinates: the lane of the aligned bytes [6 * piece, 7 * piece)
            d_at = lane_hi + delta - offset
            text[lane_hi - offset - 10:d_at] = ord("a")
            text[lane_hi - offset - 10] = ord("c")
            text[d_at] = ord("d")
            model = sb.fast_taint_down(text, rx, offset, 0, ps, warm)
            got, total = _gpu(exp_ctx, _dev(exp_ctx, text, offset), rx)
            last = exp_ctx.regex_star_begins_last()
            assert last["warm"] == warm and last["piece_shift"] == ps
            assert last["tainted"] == model.waves and last["slow"] == (1 if model.waves else 0), (offset, delta, last, model.waves)
            assert total == 1 and got.tolist() == [lane_hi - offset - 10], (offset, delta)
            seen.add(model.waves > 0)
    assert seen == {False, True}
    exp_ctx.set_knob("regex_star_begins_piece_shift", 0)


# ---- geometry and shards ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shards", [3, 7])
def test_shards_with_tail_and_base_offset(ctx, shards):
    """Each shard's list is the whole list minus the starts whose every match ends past its view."""
    rng = np.random.default_rng(0x5B7A30 + shards)
    rx = so.parse("(ab|c)[ab]+d")
    n = 50000 + shards
    text = _planted(rng, rx, n, sigma=4, copies=200)
    starts = sb.begins_numpy(text, rx)
    short, _ = sb.ends_numpy(text, rx, starts, 1 << 16)
    base = (1 << 40) - n
    cut = [n * i // shards for i in range(shards + 1)]
    for i in range(shards):
        lo, own_hi = cut[i], cut[i + 1]
        hi = min(n, own_hi + 37)  # the view runs 37 bytes past the last owned start
        d_view = _dev(ctx, text[lo:hi], (3 * i) % 16, behind=text[hi:hi + 30].tobytes())
        got, total = _gpu(ctx, d_view, rx, tail=hi - own_hi, base_offset=base + lo)
        keep = (starts >= lo) & (starts < own_hi) & (short.astype(np.int64) < hi)
        assert total == keep.sum() and np.array_equal(got, starts[keep] + base), (i, lo, hi)
    got, total = _gpu(ctx, _dev(ctx, text), rx, tail=n)
    assert total == 0 and got.size == 0


def test_count_only_and_host_entries(ctx):
    rng = np.random.default_rng(0x5B7A40)
    rx = so.parse("[ab]+c")
    text = _planted(rng, rx, 9000, sigma=4, copies=50)
    want = sb.begins_numpy(text, rx)
    _, total = ctx.search_regex_star_begins_device(_dev(ctx, text, 1), _struct(rx), capacity=0)
    assert total == want.size
    assert np.array_equal(ctx.search_regex_star_begins(text, "[ab]+c").astype(np.int64), want)
    assert np.array_equal(host.search_regex_star_begins(text, "[ab]+c").astype(np.int64), want)
    for longest in (False, True):
        s, e, clipped = ctx.search_regex_star_begins_spans(text, "[ab]+c", longest=longest, window=64)
        want_e, want_c = sb.ends_numpy(text, rx, want, 64, longest=longest)
        assert np.array_equal(s.astype(np.int64), want) and np.array_equal(e, want_e) and clipped == want_c
    assert ctx.last_regex_star_begins_ms() > 0


# ---- the ends pass ---------------------------------------------------------------------------------------------------

def _ends(ctx, text, rx, starts, offset=0, **kw):
    import torch

    d_text = _dev(ctx, text, offset, behind=b"ab" * 20)
    d_starts = torch.from_numpy(np.asarray(starts, np.int64)).to(d_text.device)
    if kw.get("limit") is not None:
        kw["limit"] = torch.from_numpy(np.asarray(kw["limit"], np.int64)).to(d_text.device)
    e, clipped = ctx.regex_star_ends_device(d_text, _struct(rx), d_starts, **kw)
    return e.cpu().numpy().astype(np.uint64), clipped


def test_ends_on_random_pairs_at_every_start_mod_8(ctx):
    rng = np.random.default_rng(0x5B7A50)
    mods = set()
    for case in range(60):
        sigma = (2, 4)[case % 2]
        expr, rx = so.random_regex(rng, np.arange(97, 97 + sigma), max_m=(8, 32, 64)[case % 3], cyclic=None if case % 4 else True)
        text = _planted(rng, rx, int(rng.integers(1, 3000)), sigma=sigma, copies=8)
        starts = sb.begins_numpy(text, rx)
        if starts.size == 0:
            continue
        for window in (1, 7, 64, 4096):
            if rx.max_len != so.UNBOUNDED and rx.max_len <= window:
                pass  # (every start has a match: no sentinel, no error)
            elif rx.max_len != so.UNBOUNDED:
                continue  # an acyclic automaton longer than the window may leave a start without a match: not this test
            for longest in (False, True):
                want, want_c = sb.ends_numpy(text, rx, starts, window, longest=longest)
                got, clipped = _ends(ctx, text, rx, starts, case % 16, window=window, longest=longest)
                assert np.array_equal(got, want) and clipped == want_c, (expr, window, longest)
        mods |= {(int(s) + case) % 8 for s in starts}
    assert mods == set(range(8))


@pytest.mark.parametrize("window", [16, 64, 65536])
def test_ends_at_the_windows_edge(ctx, window):
    """Matches of window - 1, window and window + 1 bytes of a[bc]*d, each followed by text that ends the run: the clipped
    count is 0 / 0 / 1 and the one clipped entry reports no match, never a shorter one."""
    rx = so.parse("a[bc]*d")
    for length, want_clipped in ((window - 1, 0), (window, 0), (window + 1, 1)):
        text = np.full(3 * 65536 + 100, ord("x"), np.uint8)
        s = 12345
        text[s] = ord("a")
        text[s + 1:s + length - 1] = ord("b")
        text[s + length - 1] = ord("d")
        for longest in (False, True):
            got, clipped = _ends(ctx, text, rx, [s], 3, window=window, longest=longest)
            assert clipped == want_clipped, (window, length)
            assert got.tolist() == ([s + length - 1] if length <= window else [int(NONE)]), (window, length)
    # the view's end or the limit stops the run at the window's edge: not clipped
    text = np.full(200, ord("b"), np.uint8)
    text[5] = ord("a")
    got, clipped = _ends(ctx, text[:5 + 16], rx, [5], 0, window=16)
    assert got.tolist() == [int(NONE)] and clipped == 0
    got, clipped = _ends(ctx, text, rx, [5], 0, window=16, limit=[20])
    assert got.tolist() == [int(NONE)] and clipped == 0
    got, clipped = _ends(ctx, text, rx, [5], 0, window=16, limit=[21])
    assert got.tolist() == [int(NONE)] and clipped == 1


def test_ends_limits_sentinels_errors_and_the_early_exit(exp_ctx):
    rng = np.random.default_rng(0x5B7A60)
    rx = so.parse("[a-c]+d?")
    text = (rng.integers(0, 5, 20000) + 0x61).astype(np.uint8)
    text[rng.integers(0, 20000, 2000)] = 10
    starts = sb.begins_numpy(text, rx)
    cuts = np.nonzero(text == 10)[0]
    nxt = np.searchsorted(cuts, starts)
    limit = np.where(nxt < cuts.size, cuts[np.minimum(nxt, cuts.size - 1)], text.size - 1)
    limit[::7] = starts[::7] - 1  # no room at all: the sentinel
    for longest in (False, True):
        want, want_c = sb.ends_numpy(text, rx, starts, 4096, limit=limit, longest=longest)
        got, clipped = _ends(exp_ctx, text, rx, starts, 7, window=4096, longest=longest, limit=limit)
        assert np.array_equal(got, want) and clipped == want_c == 0
        assert (got[::7] == NONE).all()
        # the early exit changes no answer
        exp_ctx.set_knob("regex_star_ends_no_early_exit", 1)
        for window in (4096, 65536):
            full, c2 = _ends(exp_ctx, text, rx, starts, 7, window=window, longest=longest, limit=limit)
            assert np.array_equal(full, want) and c2 == 0
        exp_ctx.set_knob("regex_star_ends_no_early_exit", 0)
        wide, c3 = _ends(exp_ctx, text, rx, starts, 7, window=65536, longest=longest, limit=limit)
        assert np.array_equal(wide, want) and c3 == 0
    # a cyclic automaton: a start without a match in the window is the sentinel, no error; an acyclic one that fits: an error
    got, clipped = _ends(exp_ctx, b"xxabbbxx", so.parse("ab+c"), [2], 0, window=16)
    assert got.tolist() == [int(NONE)] and clipped == 0
    with pytest.raises(host.BmxError):
        _ends(exp_ctx, b"xxabbbxx", so.parse("abc"), [2], 0, window=16)
    with pytest.raises(host.BmxError):  # a start outside the view
        _ends(exp_ctx, b"xxabbbxx", so.parse("ab+"), [2, 8], 0, window=16)


# ---- through the public routes ---------------------------------------------------------------------------------------

def test_findall_and_sub_posix_with_the_star_kind(ctx):
    rng = np.random.default_rng(0x5B7A70)
    for expr in ("[0-9]+", "ab|bc+", "[a-c][a-c0-9]*", "[0-9]+x[0-9]+"):
        rx = so.parse(expr)
        text = rng.choice(np.frombuffer(b"abc0189x \n", np.uint8), 4000).tobytes()
        want = sb.posix_matches(text, rx)
        assert host.findall(text, expr, kind="regex_star", posix=True) == [text[s:e + 1] for s, e in want], expr
        out, at = [], 0
        for s, e in want:
            out += [text[at:s], b"<>"]
            at = e + 1
        assert host.sub(text, expr, b"<>", kind="regex_star", posix=True) == b"".join(out + [text[at:]]), expr
        cuts = [i for i, c in enumerate(text) if c == 10]
        row_end = lambda s, cuts=np.array(cuts): int(cuts[np.searchsorted(cuts, s)]) if np.searchsorted(cuts, s) < cuts.size else len(text) - 1
        want = [(s, e) for s, e in sb.posix_matches(text, rx, limit_of=row_end) if 10 not in text[s:e + 1]]
        assert host.findall(text, expr, kind="regex_star", posix=True, rows=True) == [text[s:e + 1] for s, e in want], expr
    assert host.findall(b"abcc", "ab|bc+", kind="regex_star", posix=True) == [b"ab"]
    assert host.findall(b"abcc", "ab|bc+", kind="regex_star", merge=True) == [b"abcc"]
    assert host.findall(b"x123y45", "[0-9]+", kind="regex_star") == [b"1", b"2", b"3", b"4", b"5"]  # posix=False: unchanged
    assert host.findall(b"x123y45", "[0-9]+", kind="regex_star", posix=True) == [b"123", b"45"]
    assert host.findall(b"x123y45", "[0-9]{1,8}", posix=True) == [b"123", b"45"]  # kind "regex": the star-free entries


def test_a_clipped_run_raises(ctx):
    text = b"x" + b"7" * 100 + b"y"
    with pytest.raises(ValueError, match=r"1 match.*window of 50"):
        host.findall(text, "[0-9]+", kind="regex_star", posix=True, window=50)
    with pytest.raises(ValueError, match=r"window of 50"):
        host.sub(text, "[0-9]+", b"#", kind="regex_star", posix=True, window=50)
    with pytest.raises(ValueError, match=r"window of 100"):  # the run fills the window: the byte behind it is not looked at
        host.findall(text, "[0-9]+", kind="regex_star", posix=True, window=100)
    assert host.findall(text, "[0-9]+", kind="regex_star", posix=True, window=101) == [b"7" * 100]
    assert host.sub(text, "[0-9]+", b"#", kind="regex_star", posix=True) == b"x#y"


# ---- streams and workspace -------------------------------------------------------------------------------------------

def test_a_callers_stream_behind_a_pending_copy_on_both_paths(exp_ctx):
    import torch

    rng = np.random.default_rng(0x5B7A80)
    n = 1 << 19
    dev = f"cuda:{exp_ctx.device}"
    for expr, tainted in (("[ab]+c", False), ("[ab].*c", True)):
        rx = so.parse(expr)
        text = np.full(n, ord("x"), np.uint8)  # (an x empties both bounds of [ab]+c and keeps the upper one of [ab].*c)
        for at in rng.integers(0, n - 8, 300):
            text[at:at + 5] = np.frombuffer(b"abbac", np.uint8)
        text[n - 1] = ord("c")
        want = sb.begins_numpy(text, rx)
        decoy = np.full(n, ord("x"), np.uint8)
        pinned = torch.from_numpy(text).pin_memory()
        d_text = torch.from_numpy(decoy).to(dev)
        stream = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            d_text.copy_(pinned, non_blocking=True)  # the text is still on its way when the search is enqueued
            got, total = exp_ctx.search_regex_star_begins_device(d_text, _struct(rx), capacity=n, stream=stream)
        assert (exp_ctx.regex_star_begins_last()["slow"] == 1) == tainted
        assert total == want.size and np.array_equal(got.cpu().numpy(), want), expr


def test_workspace_grows_shrinks_and_grows(exp_ctx):
    exp_ctx.set_knob("regex_star_begins_piece_shift", 4)
    rx = so.parse("[ab].*c")
    rng = np.random.default_rng(0x5B7A90)
    for n in (1 << 16, 1 << 12, 1 << 18, 100):
        text = (rng.integers(0, 2, n) + 0x61).astype(np.uint8)
        text[rng.integers(0, n, n // 50)] = ord("x")
        text[n - 1] = ord("c")
        want = sb.begins_numpy(text, rx)
        got, total = _gpu(exp_ctx, _dev(exp_ctx, text, 11), rx)
        last = exp_ctx.regex_star_begins_last()
        assert last["slow"] == 1 and last["pieces"] == ((n + 11 - 1) >> 4) + 1, last
        assert total == want.size and np.array_equal(got, want), n
    exp_ctx.set_knob("regex_star_begins_piece_shift", 0)


# ---- tiles around the pool, several per workgroup ----------------------------------------------------------------------------

STAGE = 2048  # TILE_STAGE of csrc/bmx_tile_frame.h: a tile with more hits walks itself a second time and writes directly
TILE_COUNTS = [3, 2049, 5, 2048, 2049, 0, 2047, 4096, 2040, 2056, 0, 2041, 2055, 1]


def _pool_text(first: int, ps: int):
    """(text, starts): tile t of 256 << ps aligned bytes holds TILE_COUNTS[t] copies of ``abx`` on a background of x, the
    view begins ``first`` bytes into its 16-byte line and ends with a c."""
    tile = 256 << ps
    assert 3 * max(TILE_COUNTS) + 32 <= tile
    n = len(TILE_COUNTS) * tile - first - 5
    text = np.full(n, ord("x"), np.uint8)
    starts = []
    for t, count in enumerate(TILE_COUNTS):
        at = t * tile - first + 16 + 3 * np.arange(count)
        text[at], text[at + 1] = ord("a"), ord("b")
        starts += at.tolist()
    text[n - 1] = ord("c")
    return text, np.array(starts, np.int64)


@pytest.mark.parametrize("mode", ["fast", "forced", "taint"])
def test_several_tiles_per_workgroup_with_counts_around_the_pool(exp_ctx, mode):
    """Fourteen tiles of 16 KiB with 0, 1, 3, 5, 2040..2056 and 4096 starts each (parked, or walked a second time and written
    downwards), empty and overflowing tiles side by side, 1, 2 and 3 workgroups, pointer offsets 0 and 15: count only, a
    capacity inside a dense tile, room for all.  ab+ on the first launch alone and with the slow path forced (the walk
    from the swept states); a.*c with the one c on the last byte takes the slow path by itself."""
    import torch

    ps = 6
    rx = so.parse("a.*c" if mode == "taint" else "ab+")
    exp_ctx.set_knob("regex_star_begins_piece_shift", ps)
    _gpu(exp_ctx, _dev(exp_ctx, b"abc"), rx)  # (the shared geometry knobs reach the sessions a context already has)
    exp_ctx.set_knob("regex_star_begins_force_slow", int(mode == "forced"))
    for first in (0, 15):
        text, want = _pool_text(first, ps)
        d_text = _dev(exp_ctx, text, first)
        inside = sum(TILE_COUNTS[:7]) + TILE_COUNTS[7] // 2  # the capacity ends inside the tile of 4096
        for grid in (1, 2, 3):
            exp_ctx.set_knob("tile_max_grid", grid)
            for cap in (0, inside, want.size):
                out = torch.full((cap + 64,), -7, dtype=torch.int64, device=d_text.device)
                got, total = exp_ctx.search_regex_star_begins_device(d_text, _struct(rx), out=out, capacity=cap)
                last = exp_ctx.regex_star_begins_last()
                assert exp_ctx.last_launch("regex_star_begins") == (ps, grid, len(TILE_COUNTS)), (mode, first, grid)
                assert last["slow"] == int(mode != "fast") and (last["tainted"] > 0) == (mode == "taint"), (mode, last)
                assert total == want.size and np.array_equal(got.cpu().numpy(), want[:cap]), (mode, first, grid, cap)
                assert bool((out[cap:] == -7).all()), (mode, first, grid, cap)
    exp_ctx.set_knob("regex_star_begins_force_slow", 0)
    exp_ctx.set_knob("tile_max_grid", 0)
    exp_ctx.set_knob("regex_star_begins_piece_shift", 0)


# ---- one large case ------------------------------------------------------------------------------------------------------------

# tests/test_gpu_regex_star_limits.py::test_star_text_beyond_4GiB and its tainted twin took at most 0.91 s on one MI355X
# (DESIGN.md s27), text included.  This case makes its own text of the same size and runs five searches and two ends passes
# over it, one of them the forced slow path (12 ms of R1 on 4 GiB by s27's figures): about twice that work.  Ten times the
# recorded duration leaves room for a busy machine and still fails a call that falls back to anything text-sized on the host.
BIG_LIMIT_S = 10.0


def test_text_beyond_4GiB(ctx, exp_ctx):
    """2^32 + 4,097 bytes of ACGT with (wx|y)z+[ef] planted at byte 5, in front of, across and behind 2^32 and on the last
    bytes: exactly the planted starts, their longest and shortest ends, the same at base_offset 2^40 + 3 and on the forced
    slow path; the oracle runs on the windows around the plants."""
    import time

    import torch

    B = 1 << 32
    n = B + 4097
    base = (1 << 40) + 3
    rx = so.parse("(wx|y)z+[ef]")
    began = time.perf_counter()
    d_text = torch.empty(n, dtype=torch.uint8, device=f"cuda:{ctx.device}")
    ctx.gen_text(d_text, 0, 0x5EED4B31, kind=1)
    plants = ((5, b"wxzzze"), (B - 9, b"wxzzf"), (B - 1, b"yzzzze"), (B + 5, b"yze"), (n - 4, b"yzzf"))
    for at, p in plants:
        d_text[at:at + len(p)] = torch.frombuffer(bytearray(p), dtype=torch.uint8).to(d_text.device)
    want_s, want_short, want_long = [], [], []
    for lo, hi in ((0, 64), (B - 64, B + 64), (n - 64, n)):
        window = d_text[lo:hi].cpu().numpy().tobytes()
        s_ = sb.begins_numpy(window, rx)
        want_s += (s_ + lo).tolist()
        want_short += (sb.ends_numpy(window, rx, s_, 64)[0].astype(np.int64) + lo).tolist()
        want_long += (sb.ends_numpy(window, rx, s_, 64, longest=True)[0].astype(np.int64) + lo).tolist()
    assert want_s == [at for at, _ in plants] and want_long == [at + len(p) - 1 for at, p in plants] == want_short
    re_ = _struct(rx)
    out = torch.full((64,), -1, dtype=torch.int64, device=d_text.device)
    starts, total = ctx.search_regex_star_begins_device(d_text, re_, out=out)
    assert total == len(want_s) and starts.cpu().tolist() == want_s and bool((out[total:] == -1).all())
    for longest, want in ((True, want_long), (False, want_short)):
        ends, clipped = ctx.regex_star_ends_device(d_text, re_, starts, window=64, longest=longest)
        assert ends.cpu().tolist() == want and clipped == 0
    out.fill_(-1)
    starts, total = ctx.search_regex_star_begins_device(d_text, re_, out=out, base_offset=base)
    assert total == len(want_s) and starts.cpu().tolist() == [s + base for s in want_s] and bool((out[total:] == -1).all())
    ends, clipped = ctx.regex_star_ends_device(d_text, re_, starts, window=64, longest=True, base_offset=base)
    assert ends.cpu().tolist() == [e + base for e in want_long] and clipped == 0
    ends, clipped = ctx.regex_star_ends_device(d_text, re_, starts, window=4, longest=True, base_offset=base)
    fits = {B + 5: B + 7, n - 4: n - 1}  # yze and yzzf; the z+ of the three others is still running after four bytes
    assert ends.cpu().tolist() == [base + fits[s] if s in fits else -1 for s in want_s] and clipped == 3
    exp_ctx.set_knob("regex_star_begins_force_slow", 1)
    out.fill_(-1)
    starts, total = exp_ctx.search_regex_star_begins_device(d_text, re_, out=out, base_offset=base)
    last = exp_ctx.regex_star_begins_last()
    exp_ctx.set_knob("regex_star_begins_force_slow", 0)
    assert last["slow"] == 1 and last["pieces"] == ((n - 1) >> last["piece_shift"]) + 1 > 1 << 20, last
    assert total == len(want_s) and starts.cpu().tolist() == [s + base for s in want_s] and bool((out[total:] == -1).all())
    torch.cuda.synchronize()
    took = time.perf_counter() - began
    del d_text
    torch.cuda.empty_cache()
    assert took < BIG_LIMIT_S, took


# ---- the driver ----------------------------------------------------------------------------------------------------------------

def _cli(path, args, rc=0):
    import os
    import subprocess

    from conftest import ROOT

    exe = os.path.join(ROOT, host.__name__.split(".")[0], "bin", "bmx_cli")
    out = subprocess.run([exe, "--text", str(path)] + args, capture_output=True, timeout=120)
    assert out.returncode == rc, (args, out.returncode, out.stderr)
    return out.stdout, out.stderr.decode()


def test_cli(tmp_path):
    text = b"a1 22 x333333333333 4444\n5 abcc a12\nb66 a-b\n"
    path = tmp_path / "t.txt"
    path.write_bytes(text)
    out, _ = _cli(path, ["--regex-star", "[0-9]+", "--only-matching", "--posix", "--window", "64"])
    assert out.split(b"\n")[:-1] == [b"1", b"22", b"333333333333", b"4444", b"5", b"12", b"66"]
    out, _ = _cli(path, ["--regex-star", "[0-9]+", "--replace", "N", "--posix", "--window", "64"])
    assert out == b"aN N xN N\nN abcc aN\nbN a-b\n"
    out, _ = _cli(path, ["--regex-star", "ab|bc+", "--only-matching", "--posix", "--window", "64"])
    assert out == b"ab\n"  # (abcc: ab alone, as POSIX takes it)
    rx = so.parse("a[^x]+b")
    cuts = np.array([i for i, c in enumerate(text) if c == 10])
    row_end = lambda s: int(cuts[np.searchsorted(cuts, s)])
    whole, lines = sb.posix_matches(text, rx), sb.posix_matches(text, rx, limit_of=row_end)
    assert whole != lines and len(lines) > 0
    out, _ = _cli(path, ["--regex-star", "a[^x]+b", "--only-matching", "--posix", "--window", "64"])
    assert out == b"".join(text[s:e + 1] + b"\n" for s, e in whole)
    out, _ = _cli(path, ["--regex-star", "a[^x]+b", "--only-matching", "--posix", "--window", "64", "--lines"])
    assert out == b"".join(text[s:e + 1] + b"\n" for s, e in lines)
    _, err = _cli(path, ["--regex-star", "[0-9]+", "--only-matching", "--posix", "--window", "8"], rc=1)  # never a shorter match
    assert "5 match(es) may be longer than the window of 8 bytes" in err  # (every start whose run of digits outlasts the window)
    _, err = _cli(path, ["--regex-star", "[0-9]+", "--only-matching", "--posix", "--window", "8", "--lines"], rc=1)
    assert "may be longer than the window of 8 bytes" in err
    rd = so.parse("[0-9]+")
    starts = sb.begins_numpy(text, rd)
    out, _ = _cli(path, ["--regex-star", "[0-9]+", "--begins", "--positions", "--max-print", "1000"])
    assert [int(l.split(b":")[1]) for l in out.split(b"\n") if l.startswith(b"Start at")] == starts.tolist()
    assert f"regex match starts: {starts.size}".encode() in out
    for window, flag in ((64, ["--longest"]), (64, []), (8, ["--longest"])):
        ends, clipped = sb.ends_numpy(text, rd, starts, window, longest=bool(flag))
        out, _ = _cli(path, ["--regex-star", "[0-9]+", "--begins", "--spans", "--window", str(window), "--positions", "--max-print", "1000"] + flag)
        got = [tuple(map(int, l.split(b":")[1].split())) for l in out.split(b"\n") if l.startswith(b"Match at")]
        assert got == list(zip(starts.tolist(), ends.tolist())), (window, flag)
        assert f"clipped by the window of {window} bytes: {clipped}".encode() in out
    for bad in (["--regex-star", "a+", "--posix", "--only-matching"], ["--regex-star", "a+", "--begins", "--spans"],
                ["--regex-star", "a+", "--begins", "--window", "4"], ["--regex-star", "a+", "--begins", "--spans", "--window", "0"],
                ["--regex-star", "a+", "--posix", "--merge", "--only-matching", "--window", "4"],
                ["--regex", "a", "--begins", "--spans", "--window", "4"]):
        _cli(path, bad, rc=2)
