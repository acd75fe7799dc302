"""GPU suite for the regular-expression search of up to 128 positions (bmx_search_regex_long_device / bmx_search_regex_long /
bmx_search_regex_long_spans / bmx_regex_long_starts_device / bmx_cli --regex-long): full lists compared with the numpy
matcher (tests/regex_oracle.py on automata from tests/regex_long_oracle.py), and with the 64-position entries through
widen_regex where the expression fits them."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import classes_oracle as co
import regex_long_oracle as rl
import regex_oracle as ro
from conftest import ROOT, golden_file_bytes
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "parallel_implementation_of_string_matching_algorithms_opencl_amd", "bin", "bmx_cli")
WORDS = ["ERROR", "FATAL", "PANIC", "WARNING", "CRITICAL", "EXCEPTION", "TIMEOUT", "REFUSED", "DENIED", "ABORTED"]
KEYWORDS = "(" + "|".join(WORDS) + "): [0-9]{2,4}"


def _golden() -> bytes:
    """The first 60,000 bytes of the golden text: the numpy matcher walks one array per position and link."""
    return golden_file_bytes("input5L.txt.gz")[:60000]


def piece(max_len: int) -> int:
    """The host's piece rule for a text far smaller than the resident lanes: 2^ps ends per lane with
    ps = max(6, ceil(log2(4 max_len))); a tile is 256 pieces."""
    return max(64, 1 << (4 * max_len - 1).bit_length())


def _dev(ctx, data, offset: int = 0, front: int = 0):
    """data on the device, starting `offset` bytes into a buffer (any alignment); the bytes in front of it hold `front`."""
    import torch

    data = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data
    buf = torch.full((data.size + offset + 16,), front, dtype=torch.uint8, device=f"cuda:{ctx.device}")
    if data.size:
        buf[offset:offset + data.size] = torch.from_numpy(data.copy()).to(buf.device)
    return buf[offset:offset + data.size]


def _struct(rx: ro.Rx) -> host.RegexLong:
    """An oracle automaton as the library's plain data (the length fields left at 0: the entries do not read them)."""
    r = host.RegexLong()
    r.m = rx.m
    r.first[0], r.first[1] = rl.words(rx.first)
    r.last[0], r.last[1] = rl.words(rx.last)
    for i, f in enumerate(rx.follow):
        r.follow[i][0], r.follow[i][1] = rl.words(f)
    packed = co.pack(rx.member).tobytes()
    C.memmove(r.classes, packed, len(packed))
    return r


def _gpu(ctx, d_text, rx, **kw):
    n = kw.get("n", d_text.numel())
    cap = kw.pop("capacity", max(n, 1))
    ends, total = ctx.search_regex_long_device(d_text, rx if isinstance(rx, host.RegexLong) else _struct(rx), capacity=cap, **kw)
    return ends.cpu().numpy().astype(np.int64), total


def _check(ctx, text, rx: ro.Rx, offset: int = 0, starts: bool = False, what=None, want=None):
    text = bytes(text)
    if want is None:
        want = ro.ends_numpy(text, rx)
    d_text = _dev(ctx, text, offset)
    got, total = _gpu(ctx, d_text, rx)
    assert total == want.size, (what, len(text), rx.m, offset, total, want.size)
    assert np.array_equal(got, want), (what, len(text), rx.m, offset)
    if starts and want.size:
        import torch

        d_ends = torch.from_numpy(want).to(d_text.device)
        for longest in (False, True):
            s = ctx.regex_long_starts_device(d_text, _struct(rx), d_ends, longest=longest)
            assert np.array_equal(s.cpu().numpy(), ro.starts_numpy(text, rx, longest)[1]), (what, rx.m, longest)
    return want


def _planted(rng, rx, n, sigma_base=0x61, sigma=5, copies=12):
    text = (rng.integers(0, sigma, n) + sigma_base).astype(np.uint8)
    at = 3
    for _ in range(copies):
        at = ro.plant_path(rng, text, rx, at) + int(rng.integers(0, 40))
    return text


def _tables(rx) -> int:
    """The follow tables the expression needs: the bytes of the 128-bit word that hold an irregular position."""
    nl = ro.split(rx)[1]
    return sum(1 for b in range(16) if (nl >> (8 * b)) & 0xFF)


def test_random_expressions_against_oracle(ctx):
    """240 expressions of 65..128 positions over 2, 4 and 95 symbols at the sixteen alignments of the view: the ends, and
    for every end the shortest and the longest match."""
    rng = np.random.default_rng(0x331C00)
    hits, upper, classes = 0, 0, set()
    for case in range(240):
        sigma = (2, 4, 95)[case % 3]
        n = int(rng.integers(0, 5001)) if case % 10 else int(rng.integers(0, 140))  # every tenth: n around or below max_len
        base = 0x20 if sigma == 95 else 0x61
        symbols = np.arange(base, base + sigma)
        expr, rx = rl.random_regex(rng, symbols, 65, 128, bar=(1 / 6, 0.5)[case % 2])
        text = (rng.integers(0, sigma, n) + base).astype(np.uint8)
        for _ in range(int(rng.integers(0, 4))):
            if n:
                ro.plant_path(rng, text, rx, int(rng.integers(0, n)))
        hits += _check(ctx, text, rx, offset=case % 16, starts=True, what=expr).size
        upper += rx.m > 96
        t = _tables(rx)
        classes.add(0 if t == 0 else 7 if t <= 7 else 12 if t <= 12 else 16)
    assert hits > 5000 and upper >= 40 and classes >= {12, 16}, (hits, upper, classes)  # (none and up to 7 tables: the tests below)


def test_word_widths(ctx):
    """m = 1, 32, 33, 64, 65, 96, 97, 127, 128, with and without irregular positions."""
    rng = np.random.default_rng(151)
    exprs = ("a", "a{31}b", "a{32}b", "a{63}b", "a{64}b", "a{95}b", "a{96}b", "a{126}b", "a{127}b", "a{28}(b|cd)e", "a{29}(b|cd)e",
             "a{60}(b|cd)e", "a{61}(b|cd)e", "a{92}(b|cd)e", "a{93}(b|cd)e", "a{123}(b|cd)e", "a{124}(b|cd)e", "(a|b){1,64}")
    ms = [rl.parse(e).m for e in exprs]
    assert ms == [1, 32, 33, 64, 65, 96, 97, 127, 128, 32, 33, 64, 65, 96, 97, 127, 128, 128]
    for expr in exprs:
        rx = rl.parse(expr)
        text = _planted(rng, rx, 6000, sigma=3)
        want = _check(ctx, text, rx, offset=rx.m % 16, starts=True, what=expr)
        assert want.size >= 12, expr


def _literal_with_group(k: int) -> str:
    """a{k}(b|cd)e: the irregular positions are k - 1 and k, nothing else."""
    return "a{%d}(b|cd)e" % k


@pytest.mark.parametrize("b", range(16))
def test_irregular_positions_in_one_byte_of_the_word(ctx, b):
    rng = np.random.default_rng(160 + b)
    expr = _literal_with_group(8 * b + 2)
    rx = rl.parse(expr)
    nl = ro.split(rx)[1]
    assert nl == 0b110 << (8 * b), bin(nl)  # positions 8b + 1 and 8b + 2: byte b only
    text = _planted(rng, rx, 5000, sigma=3)
    assert _check(ctx, text, rx, offset=b, starts=True, what=expr).size >= 12


@pytest.mark.parametrize("k", [32, 64, 96])
def test_a_follow_link_across_a_dword_boundary(ctx, k):
    rng = np.random.default_rng(170 + k)
    rx = rl.parse(_literal_with_group(k))
    assert ro.split(rx)[1] == 0b11 << (k - 1)  # positions k - 1 and k: the last bit of one dword, the first of the next
    assert rx.follow[k - 1] == 0b11 << k and rx.follow[k] == 1 << (k + 3)
    assert _check(ctx, _planted(rng, rx, 5000, sigma=3), rx, offset=9, starts=True).size >= 12
    rx = rl.parse("x{%d}" % (k + 5))  # and the shift alone
    assert _check(ctx, _planted(rng, rx, 5000, sigma=3, sigma_base=ord("w")), rx, offset=3, starts=True).size >= 12


@pytest.mark.parametrize("expr,tables", [("a.{0,100}b", 16), ("x{120}", 0), (KEYWORDS, 12), ("(ERROR|FATAL|PANIC): [0-9]{2,4}x{60}", 7), ("x{50}(ab|c)x{50}(d|ef)", 7),
                                         ("((ab|c)defgh){7}x{70}", 7), ("((ab|c)defgh){8}x{60}", 12), ("((ab|c)defgh){12}x{30}", 12),
                                         ("((ab|c)defgh){13}x{20}", 16), ("((ab|c)defgh){16}", 16), ("(a|b){1,64}", 16)])
def test_one_expression_per_table_count_class(ctx, expr, tables):
    rng = np.random.default_rng(180 + tables)
    rx = rl.parse(expr)
    t = _tables(rx)
    assert (0 if t == 0 else 7 if t <= 7 else 12 if t <= 12 else 16) == tables, t  # the kernels have 0, 7, 12 and 16 table slots
    if expr == "((ab|c)defgh){16}":
        assert rx.m == 128 and t == 16
    text = _planted(rng, rx, 9000, sigma=8, sigma_base=0x41 if expr == KEYWORDS else 0x61)
    if expr == KEYWORDS:
        text[text == ord("B")] = ord("7")
    assert _check(ctx, text, rx, offset=1, starts=True, what=expr).size >= 12


def test_long_entries_equal_the_64_position_entries_through_widen(ctx):
    import torch

    rng = np.random.default_rng(0x331C01)
    seen = 0
    for case in range(60):
        sigma = (2, 4)[case % 2]
        symbols = np.arange(0x61, 0x61 + sigma)
        expr, rx = ro.random_regex(rng, symbols, max_m=(32, 64)[case % 2])
        text = (rng.integers(0, sigma, 4000) + 0x61).astype(np.uint8)
        for _ in range(3):
            ro.plant_path(rng, text, rx, int(rng.integers(0, 4000)))
        d_text = _dev(ctx, text, case % 16)
        short = host.compile_regex(expr)
        wide = host.widen_regex(short)
        e64, t64 = ctx.search_regex_device(d_text, short, capacity=4000)
        e128, t128 = ctx.search_regex_long_device(d_text, wide, capacity=4000)
        assert t64 == t128 and torch.equal(e64, e128), expr
        e128c, _ = ctx.search_regex_long_device(d_text, expr, capacity=4000)  # compiled by the long compiler
        assert torch.equal(e128c, e64), expr
        if t64:
            for longest in (False, True):
                s64 = ctx.regex_starts_device(d_text, short, e64, longest=longest)
                s128 = ctx.regex_long_starts_device(d_text, wide, e128, longest=longest)
                assert torch.equal(s64, s128), (expr, longest)
        seen += t64
    assert seen > 5000


def test_nothing_begins_in_front_of_an_unaligned_view(ctx):
    """The view begins 7 bytes into a 16-byte line and the bytes in front of it would fit: a match that begins out there
    and ends on one of the first ends is no match of the view."""
    rx = rl.parse("(..|.{9})y.{0,70}")
    view = b"y" * 40
    for front in (0, ord("y")):
        got, total = _gpu(ctx, _dev(ctx, view, 7, front), rx)
        assert total == 38 and np.array_equal(got, np.arange(2, 40)), (front, got[:4])
    rx = rl.parse("(x.{5}|abcdefgh)y|q{70}")
    view = b"qqqyqqqqx12345yqq"
    got, total = _gpu(ctx, _dev(ctx, view, 7, ord("x")), rx)  # an x three bytes in front would end a match at view[3]
    assert got.tolist() == [14] == ro.ends_numpy(view, rx).tolist()
    rx = rl.parse("(a|b){1,64}")  # every alignment, every end a hit from byte 0 on
    for off in range(16):
        got, total = _gpu(ctx, _dev(ctx, b"ab" * 50, off, ord("a")), rx)
        assert total == 100 and np.array_equal(got, np.arange(100)), off
    rx = rl.parse("a{100}")  # a run that begins in front of the view counts from the view's first byte
    for off in (1, 7, 15):
        got, total = _gpu(ctx, _dev(ctx, b"a" * 150, off, ord("a")), rx)
        assert total == 51 and np.array_equal(got, np.arange(99, 150)), off


@pytest.mark.parametrize("expr", ["([ab]c?){60}a", "(a[abc]{2}|b){30}c?c", "a(b|c){30,63}a"])
def test_lengths_at_piece_and_tile_edges(ctx, expr):
    rx = rl.parse(expr)
    p = piece(rx.max_len)
    assert p == 512 and rx.m > 64 and rx.max_len > 64  # a tile is 128 KiB
    rng = np.random.default_rng(rx.m)
    big = (rng.integers(0, 3, 3 * 256 * p + 5) + 0x61).astype(np.uint8)
    for at in range(0, big.size - rx.m, 2999):
        ro.plant_path(rng, big, rx, at)
    whole = ro.ends_numpy(big.tobytes(), rx)  # (an end depends on the bytes up to it only: every prefix's list is a prefix)
    for n in (0, 1, rx.min_len - 1, rx.min_len):  # views shorter than the shortest match, and one that can hold one
        got, total = _gpu(ctx, _dev(ctx, big[:n], 5), rx)
        want = whole[whole < n]
        assert total == want.size and np.array_equal(got, want) and (n >= rx.min_len or total == 0)
    for n in (p - 1, p, p + 1, 256 * p - 1, 256 * p, 256 * p + 1, 3 * 256 * p + 5):
        for off in (0, 9):
            assert _check(ctx, big[:n], rx, offset=off, what=(expr, n), want=whole[whole < n]).size > 0


def test_dense_tiles_next_to_empty_ones(ctx):
    """(a|b){1,64} on stretches of a and b: every end of a stretch is a hit, far more than a tile's pool parks, so those
    tiles walk twice; the tiles between them hold nothing."""
    rng = np.random.default_rng(19)
    rx = rl.parse("(a|b){1,64}")
    tile = 256 * piece(rx.max_len)
    n = 3 * tile + 5
    text = np.full(n, ord("z"), np.uint8)
    for lo, hi in ((0, tile), (2 * tile - 100, n)):
        text[lo:hi] = rng.integers(0, 2, hi - lo) + 0x61
    want = _check(ctx, text, rx, offset=7)
    assert want.size == np.count_nonzero(text != ord("z")) > tile
    _, total = _gpu(ctx, _dev(ctx, text, 7), rx, capacity=0)
    assert total == want.size
    rx = rl.parse("a.{0,100}(a|b)")  # and 103 positions over the same stretches (tiles of 128 KiB)
    small = text[:2 * 256 * piece(rx.max_len)]
    _check(ctx, small, rx, offset=3)


def test_capacity_keeps_the_lowest_ends(ctx):
    import torch

    rng = np.random.default_rng(21)
    expr = "AC([ACGT]|[AC]{2,3})G(T|A)N{0,60}"
    rx = rl.parse(expr, ro.IUPAC)
    re_ = host.compile_regex_long(expr, host.CLASS_IUPAC)
    text = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 300000)]
    want = ro.ends_numpy(text.tobytes(), rx)
    total = want.size
    assert total > 5000  # more than a tile parks
    d_text = _dev(ctx, text, 4)
    for cap in (0, 1, total - 1, total // 2):
        out = torch.full((max(cap, 1),), -1, dtype=torch.int64, device=d_text.device)
        n_matches = C.c_uint64(0)
        rc = ctx._L.bmx_search_regex_long_device(ctx._h, C.c_void_p(d_text.data_ptr()), d_text.numel(), 0, 0, C.byref(re_),
                                                 C.c_void_p(out.data_ptr()), cap, C.byref(n_matches), None)
        assert rc == host.ERR_CAPACITY and n_matches.value == total, (cap, rc, n_matches.value)
        if cap:
            assert np.array_equal(out.cpu().numpy(), want[:cap]), cap
        else:
            assert int(out[0].item()) == -1
    got, t = _gpu(ctx, d_text, re_, capacity=total)  # exact
    assert t == total and np.array_equal(got, want)
    with pytest.raises(host.BmxError) as e:
        ctx.search_regex_long(text.tobytes(), re_, capacity=3)
    assert e.value.rc == host.ERR_CAPACITY


def test_lead_and_base_offset(ctx):
    rng = np.random.default_rng(14)
    text = (rng.integers(0, 2, 4000) + 0x61).astype(np.uint8).tobytes()
    rx = rl.parse("a(ab|b){1,2}b(.|aa)?a.{0,60}b")
    want = ro.ends_numpy(text, rx)
    assert want.size > 300 and rx.m > 64
    d_text = _dev(ctx, text, 3)
    base = 10 ** 12 + 7
    for n, lead in ((4000, 0), (4000, 1), (4000, 5), (4000, 1234), (4000, 3999), (4000, 4000), (2000, 1990), (6, 2), (0, 0)):
        got, total = _gpu(ctx, d_text, rx, n=n, lead=lead, base_offset=base)
        w = want[(want >= lead) & (want < n)] + base  # matches may begin in front of lead, never end behind n
        assert total == w.size and np.array_equal(got, w), (n, lead)


def test_five_shards_concatenate_to_the_whole_list(ctx):
    rng = np.random.default_rng(15)
    expr = "ATG([ACGT]{3}){2,38}(TAA|TAG|TGA)"
    re_ = host.compile_regex_long(expr)
    rx = rl.parse(expr)
    assert re_.max_len == rx.max_len == 120 and re_.m == 126
    text = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 400000)]
    d_text = _dev(ctx, text, 6)
    n = text.size
    whole, whole_t = _gpu(ctx, d_text, re_)
    assert whole_t > 1000 and np.array_equal(whole, ro.ends_numpy(text.tobytes(), rx))
    cuts = [0, 70003, 131072, 131073, 300000 + 12345, n]
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        begin = max(a - (re_.max_len - 1), 0)  # the shard and its halo in front
        got, t = _gpu(ctx, d_text[begin:b], re_, lead=a - begin, base_offset=begin)
        parts.append(got)
    assert len(parts) == 5 and np.array_equal(np.concatenate(parts), whole)


def test_starts_errors(ctx):
    import torch

    text = _golden()
    d_text = _dev(ctx, text, 5)
    expr = "(occur{1,2}|refer)ences?.{0,60}"
    re_ = host.compile_regex_long(expr)
    rx = rl.parse(expr)
    assert rx.m > 64
    ends, total = ctx.search_regex_long_device(d_text, re_, capacity=len(text), base_offset=100)
    assert total > 100
    s = ctx.regex_long_starts_device(d_text, re_, ends, base_offset=100)
    want_e, want_s = ro.starts_numpy(text, rx)
    assert np.array_equal(ends.cpu().numpy(), want_e + 100) and np.array_equal(s.cpu().numpy(), want_s + 100)
    for bad in (99, 100 + len(text)):  # an end outside [base_offset, base_offset + n)
        broken = ends.clone()
        broken[total // 2] = bad
        with pytest.raises(host.BmxError) as e:
            ctx.regex_long_starts_device(d_text, re_, broken, base_offset=100)
        assert e.value.rc == host.ERR_ARG and "outside the view" in str(e.value)
    with pytest.raises(host.BmxError) as e:  # the list of another expression
        ctx.regex_long_starts_device(d_text, "z(q|zz)zz.{70}", ends, base_offset=100)
    assert e.value.rc == host.ERR_ARG and "no match" in str(e.value)
    assert ctx.regex_long_starts_device(d_text, re_, ends[:0]).numel() == 0  # count == 0: no launch
    again = ctx.regex_long_starts_device(d_text, re_, ends, base_offset=100)  # and the status word is clean again
    assert torch.equal(again, s)
    # no position of `last` can be reached: an empty list, no launch, and the timer says so
    dead = host.compile_regex_long("x{70}y")
    dead.follow[3][0] = dead.follow[3][1] = 0
    ends, total = ctx.search_regex_long_device(_dev(ctx, b"x" * 70 + b"y"), dead, capacity=8)
    assert total == 0 and ends.numel() == 0 and ctx.last_regex_long_ms() == 0.0


def test_on_a_callers_non_blocking_stream(ctx):
    """The rig of tests/test_gpu_streams.py: the buffers hold DECOYS, the caller's non-blocking stream holds a long delay and
    then the copies of the real inputs, and each entry is called while those copies are still outstanding.  The copy of
    the automaton's tables goes on the same stream, in front of the launch."""
    import torch

    from test_gpu_streams import Pending, delay, side_stream

    text = _golden()
    decoy = text.replace(b"he", b"eh")  # the same length, other ends
    expr = "([Tt]he|an).{0,2}e.{0,60}s"
    re_ = host.compile_regex_long(expr)
    rx = rl.parse(expr)
    want_e, want_s = ro.starts_numpy(text, rx)
    _, want_l = ro.starts_numpy(text, rx, longest=True)
    assert rx.m > 64 and len(decoy) == len(text) and not np.array_equal(ro.ends_numpy(decoy, rx), want_e)
    assert want_e.size > 300 and not np.array_equal(want_s, want_l)
    real_text = _dev(ctx, text, 0)
    real_ends = torch.from_numpy(want_e).to(real_text.device)
    out = torch.full((len(text),), -1, dtype=torch.int64, device=real_text.device)

    # the search, on a context of its own: its first call allocates the block, the look-back words and the ticket
    with host.Context(0) as fresh:
        for c, what in ((fresh, "search_regex_long_device, first call of a context"), (ctx, "search_regex_long_device")):
            d_text = _dev(ctx, decoy, 2)
            s = side_stream()
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                delay(s)
                d_text.copy_(real_text, non_blocking=True)
                pending = Pending(s)
                pending.assert_outstanding(what)
                ends, total = c.search_regex_long_device(d_text, re_, out=out)
                taken = ends.clone()  # consumed on the stream
            assert total == want_e.size and np.array_equal(taken.cpu().numpy(), want_e), what

    # the starts: the text is a decoy and the list is the real one turned round (every entry a true end, other starts)
    for longest, want in ((False, want_s), (True, want_l)):
        d_text = _dev(ctx, decoy, 2)
        d_ends = real_ends.flip(0).contiguous()
        s = side_stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            delay(s)
            d_text.copy_(real_text, non_blocking=True)
            d_ends.copy_(real_ends, non_blocking=True)
            pending = Pending(s)
            pending.assert_outstanding("regex_long_starts_device")
            got = ctx.regex_long_starts_device(d_text, re_, d_ends, longest=longest)
        assert np.array_equal(got.cpu().numpy(), want), longest
    side = side_stream()  # and the stream as an argument, torch's current one being the null stream
    torch.cuda.synchronize()
    ends, total = ctx.search_regex_long_device(real_text, re_, out=out, stream=side)
    got = ctx.regex_long_starts_device(real_text, re_, ends, stream=side)
    assert total == want_e.size and np.array_equal(ends.cpu().numpy(), want_e) and np.array_equal(got.cpu().numpy(), want_s)


def test_repeat_calls_interleaved_with_the_other_searches(ctx):
    """The long regex, the 64-position regex and the class search share the look-back code, not their state; two long
    expressions in turn share the block, each call with its own tables."""
    text = _golden()
    d_text = _dev(ctx, text, 11)
    expr = "(occur{1,2}|refer)ences?.{0,60}"
    other = "([Tt]h(e|is|at) ){1,2}[a-z]{1,60}"
    rx, rx2 = rl.parse(expr, ro.ICASE), rl.parse(other)
    short = "(occur{1,2}|refer)ences?"
    rxs = ro.parse(short, ro.ICASE)
    member = co.parse("occurrences", co.ICASE)
    want, want2, want_s = ro.ends_numpy(text, rx), ro.ends_numpy(text, rx2), ro.ends_numpy(text, rxs)
    want_c = co.class_starts(text, member)
    assert rx.m > 64 and rx2.m > 64 and want.size > 100 and want2.size > 100
    for _ in range(3):
        ends, t = ctx.search_regex_long_device(d_text, expr, flags=host.CLASS_ICASE, capacity=len(text))
        assert t == want.size and np.array_equal(ends.cpu().numpy(), want)
        assert ctx.last_regex_long_ms() > 0
        ends, t = ctx.search_regex_device(d_text, short, flags=host.CLASS_ICASE, capacity=len(text))
        assert t == want_s.size and np.array_equal(ends.cpu().numpy(), want_s)
        ends, t = ctx.search_regex_long_device(d_text, other, capacity=len(text))
        assert t == want2.size and np.array_equal(ends.cpu().numpy(), want2)
        s = ctx.regex_long_starts_device(d_text, other, ends)
        assert np.array_equal(s.cpu().numpy(), ro.starts_numpy(text, rx2)[1])
        pos, t = ctx.search_classes_device(d_text, co.pack(member), capacity=len(text))
        assert t == want_c.size and np.array_equal(pos.cpu().numpy(), want_c)


def _log(rng, lines=400):
    out = []
    for i in range(lines):
        w = WORDS[int(rng.integers(0, len(WORDS)))]
        r = int(rng.integers(0, 4))
        if r == 0:
            out.append(b"%d ok nothing to see" % i)
        elif r == 1:
            out.append(b"%d %s: %03d disk" % (i, w.encode(), int(rng.integers(0, 1000))))
        elif r == 2:
            out.append(b"%d %s: %03d then %s: %03d" % (i, w.encode(), int(rng.integers(0, 1000)), WORDS[i % 10].encode(), i % 1000))
        else:
            out.append(b"%d %s; %s: x12" % (i, w.encode(), w.lower().encode()))
    return b"\n".join(out) + b"\n"


def test_grep_findall_sub_with_the_long_kind_against_re(ctx):
    rng = np.random.default_rng(16)
    text = _log(rng)
    expr = "(" + "|".join(WORDS) + "): [0-9]{3}"
    pat = re.compile(b"(?:" + "|".join(WORDS).encode() + b"): [0-9]{3}")  # (the same expression, its group not capturing)
    assert rl.parse(expr).m == 71
    with pytest.raises(host.BmxError):
        host.grep(text, expr, kind="regex")  # more than 64 positions: the 64-position kind still refuses
    lines = text.split(b"\n")[:-1]
    counts = np.array([len(pat.findall(ln)) for ln in lines])
    rows, cnt = host.grep(text, expr, kind="regex_long")
    assert np.array_equal(rows, np.nonzero(counts)[0]) and np.array_equal(cnt, counts[counts > 0]) and rows.size > 100
    rows, cnt = host.grep(text, expr, kind="regex_long", invert=True)
    assert np.array_equal(rows, np.nonzero(counts == 0)[0]) and cnt is None
    assert host.findall(text, expr, kind="regex_long") == pat.findall(text)
    assert host.sub(text, expr, b"<hit>", kind="regex_long") == pat.sub(b"<hit>", text)
    assert host.sub(text, expr, b"", kind="regex_long", merge=True) == pat.sub(b"", text)
    d_text = _dev(ctx, text, 0)
    blob, off = ctx.findall_device(d_text, expr, kind="regex_long")
    blob, off = blob.cpu().numpy().tobytes(), off.cpu().numpy()
    assert [blob[off[i]:off[i + 1]] for i in range(off.size - 1)] == pat.findall(text)
    with pytest.raises(ValueError):
        host.sub(text, expr, b"", kind="regex_long", posix=True)


def test_entry_points_and_the_cli(ctx, tmp_path):
    rng = np.random.default_rng(17)
    text = _golden() + _log(rng, 200)
    path = tmp_path / "text.txt"
    path.write_bytes(text)
    cases = [(KEYWORDS, 0, []), ("(occur{1,2}|refer)ences?.{0,60}", 0, []), ("(the|and) [a-z]{2,5} .{0,60}", host.CLASS_ICASE, ["--icase"]),
             ("a.{0,100}b", 0, [])]
    for expr, flags, opts in cases:
        rx = rl.parse(expr, flags)
        want_e, want_s = ro.starts_numpy(text, rx)
        _, want_l = ro.starts_numpy(text, rx, longest=True)
        assert want_e.size > 50 and rx.m > 64, expr
        assert np.array_equal(ctx.search_regex_long(text, expr, flags).astype(np.int64), want_e)  # host entry point, expression
        assert np.array_equal(ctx.search_regex_long(text, host.compile_regex_long(expr, flags)).astype(np.int64), want_e)
        assert np.array_equal(host.search_regex_long(text, expr, flags).astype(np.int64), want_e)  # module level
        s, e = host.search_regex_long(text, expr, flags, spans=True)
        assert np.array_equal(e.astype(np.int64), want_e) and np.array_equal(s.astype(np.int64), want_s)
        s, e = host.search_regex_long(text, expr, flags, spans=True, longest=True)
        assert np.array_equal(e.astype(np.int64), want_e) and np.array_equal(s.astype(np.int64), want_l)
        s, e = ctx.search_regex_long_spans(text, expr, flags, longest=True)
        assert np.array_equal(e.astype(np.int64), want_e) and np.array_equal(s.astype(np.int64), want_l)
        assert ctx.last_regex_long_ms() > 0
        args = [CLI, "--regex-long", expr, "--text", str(path), "--iters", "2", "--positions", "--max-print", "3"] + opts
        r = subprocess.run(args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert f"{rx.m} positions, matches of {rx.min_len} to {rx.max_len} bytes" in r.stdout
        assert f"regex matches: {want_e.size}" in r.stdout
        assert f"first end: {want_e[0]}\n" in r.stdout and f"last end: {want_e[-1]}\n" in r.stdout
        assert [int(x) for x in re.findall(r"End at : (\d+)", r.stdout)] == want_e[:3].tolist()
        assert "Average time" in r.stdout
        for more, starts in ((["--starts"], want_s), (["--starts", "--longest"], want_l)) if expr == cases[1][0] else ():
            r = subprocess.run(args + more, capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stderr
            got = [(int(a), int(b)) for a, b in re.findall(r"Match at : (\d+) (\d+)", r.stdout)]
            assert got == list(zip(starts[:3].tolist(), want_e[:3].tolist())), (expr, more)
    # the companions of --regex: --lines, --only-matching, --replace with --merge
    expr = "(" + "|".join(WORDS) + "): [0-9]{3}"
    pat = re.compile(b"(?:" + "|".join(WORDS).encode() + b"): [0-9]{3}")  # (the same expression, its group not capturing)
    r = subprocess.run([CLI, "--regex-long", expr, "--text", str(path), "--lines", "--max-print", "1000000"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    counts = [len(pat.findall(ln)) for ln in text.split(b"\n")[:-1]]
    body = [tuple(map(int, ln.split("\t"))) for ln in r.stdout.splitlines() if ln and ln[0].isdigit()]
    assert body == [(i, c) for i, c in enumerate(counts) if c] and len(body) > 50
    r = subprocess.run([CLI, "--regex-long", expr, "--text", str(path), "--replace", "<hit>", "--merge"], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == pat.sub(b"<hit>", text)
    r = subprocess.run([CLI, "--regex-long", expr, "--text", str(path), "--only-matching", "--max-print", "1000000"], capture_output=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split(b"\n")[:-1] == pat.findall(text)
    # what it refuses
    r = subprocess.run([CLI, "--regex-long", "x{129}", "--text", str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "bad regular expression" in r.stderr and "more than 128 positions" in r.stderr
    r = subprocess.run([CLI, "--regex", "x{65}", "--text", str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "more than 64 positions" in r.stderr
    for more in (["--gaps", "a"], ["--classes", "a"], ["--regex", "a"], ["--approx", "1"]):
        r = subprocess.run([CLI, "--regex-long", "a", "--text", str(path)] + more, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2, (more, r.stderr)
    for more in (["--begins"], ["--posix", "--only-matching"]):
        r = subprocess.run([CLI, "--regex-long", "a", "--text", str(path)] + more, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--regex-long goes with neither" in r.stderr, (more, r.stderr)
