"""GPU suite for the regular-expression search (bmx_search_regex_device / bmx_search_regex / bmx_search_regex_spans /
bmx_regex_starts_device / bmx_cli --regex): full lists compared with the numpy matcher (tests/regex_oracle.py), with the
gapped search where there are no groups, with the class search for a literal, and with the merged lists of the class
search over every fixed-length variant of an expression."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import classes_oracle as co
import regex_oracle as ro
from conftest import ROOT, golden_file_bytes
from parallel_implementation_of_string_matching_algorithms_opencl_amd import corpus, host

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "parallel_implementation_of_string_matching_algorithms_opencl_amd", "bin", "bmx_cli")
WHY = ["ATG([ACGT]{3}){2,4}(TAA|TAG|TGA)", "(ERROR|FATAL|PANIC): [0-9]{2,4}", r"([0-9]{1,3}\.){3}[0-9]{1,3}", "(RGD|KGD)x{2,5}[ST]"]


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


def _struct(rx: ro.Rx) -> host.Regex:
    """An oracle automaton as the library's plain data (the length fields left at 0: the entries do not read them)."""
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
    ends, total = ctx.search_regex_device(d_text, rx if isinstance(rx, host.Regex) else _struct(rx), capacity=cap, **kw)
    return ends.cpu().numpy().astype(np.int64), total


def _check(ctx, text, rx: ro.Rx, offset: int = 0, starts: bool = False, what=None):
    text = bytes(text)
    want = ro.ends_numpy(text, rx)
    d_text = _dev(ctx, text, offset)
    got, total = _gpu(ctx, d_text, rx)
    assert total == want.size, (what, len(text), rx.m, offset, total, want.size)
    assert np.array_equal(got, want), (what, len(text), rx.m, offset)
    if starts and want.size:
        import torch

        d_ends = torch.from_numpy(want).to(d_text.device)
        for longest in (False, True):
            s = ctx.regex_starts_device(d_text, _struct(rx), d_ends, longest=longest)
            assert np.array_equal(s.cpu().numpy(), ro.starts_numpy(text, rx, longest)[1]), (what, rx.m, longest)
    return want


def test_random_expressions_against_oracle(ctx):
    """300 expressions over 2, 4 and 95 symbols at the sixteen alignments of the view: the ends, and for every end the
    shortest and the longest match."""
    rng = np.random.default_rng(0x2E6E00)
    hits, wide, irregular = 0, 0, 0
    for case in range(300):
        sigma = (2, 4, 95)[case % 3]
        n = int(rng.integers(0, 5001)) if case % 10 else int(rng.integers(0, 70))  # every tenth: n around or below max_len
        base = 0x20 if sigma == 95 else 0x61
        symbols = np.arange(base, base + sigma)
        expr, rx = ro.random_regex(rng, symbols, max_m=(8, 32, 64)[case % 7 % 3])
        text = (rng.integers(0, sigma, n) + base).astype(np.uint8)
        for _ in range(int(rng.integers(0, 4))):
            if n:
                ro.plant_path(rng, text, rx, int(rng.integers(0, n)))
        hits += _check(ctx, text, rx, offset=case % 16, starts=True, what=expr).size
        wide += rx.m > 32
        irregular += ro.split(rx)[1] != 0
    assert hits > 10000 and wide >= 10 and irregular >= 100, (hits, wide, irregular)


def _literal_with_group(k: int) -> str:
    """a{k}(b|cd)e: the irregular positions are k - 1 and k, nothing else."""
    return "a{%d}(b|cd)e" % k


def _planted(rng, rx, n, sigma_base=0x61, sigma=5, copies=12):
    text = (rng.integers(0, sigma, n) + sigma_base).astype(np.uint8)
    at = 3
    for _ in range(copies):
        at = ro.plant_path(rng, text, rx, at) + int(rng.integers(0, 40))
    return text


def test_word_widths(ctx):
    """m = 1; m = 32 and 33 (the word switch); 64 positions; with and without irregular positions."""
    rng = np.random.default_rng(51)
    for expr in ("a", "[ab]", "a{31}b", "a{32}b", "a{28}(b|cd)e", "a{29}(b|cd)e", "x{64}", "(a|b){1,32}", "a{58}(b|cd)e", "(ab|c){1,21}d"):
        rx = ro.parse(expr)
        text = _planted(rng, rx, 6000)
        want = _check(ctx, text, rx, offset=rx.m % 16, starts=True, what=expr)
        assert want.size >= 12, expr
    assert [ro.parse(e).m for e in ("a{31}b", "a{32}b", "a{28}(b|cd)e", "a{29}(b|cd)e", "(a|b){1,32}", "(ab|c){1,21}d")] == [32, 33, 32, 33, 64, 64]


@pytest.mark.parametrize("b", range(8))
def test_irregular_positions_in_one_byte_of_the_word(ctx, b):
    rng = np.random.default_rng(60 + b)
    expr = _literal_with_group(8 * b + 2)
    rx = ro.parse(expr)
    nl = ro.split(rx)[1]
    assert nl == 0b110 << (8 * b), bin(nl)  # positions 8b + 1 and 8b + 2: byte b only
    text = _planted(rng, rx, 5000)
    assert _check(ctx, text, rx, offset=b + 3, starts=True, what=expr).size >= 12


def test_irregular_positions_across_the_halves_and_in_all_eight_bytes(ctx):
    rng = np.random.default_rng(70)
    rx = ro.parse(_literal_with_group(32))
    assert ro.split(rx)[1] == 0b11 << 31  # positions 31 and 32: the last bit of the low half, the first of the high half
    assert _check(ctx, _planted(rng, rx, 5000), rx, offset=9, starts=True).size >= 12
    expr = "((ab|c)defgh){8}"
    rx = ro.parse(expr)
    nl = ro.split(rx)[1]
    assert rx.m == 64 and all((nl >> (8 * b)) & 0xFF for b in range(8))
    assert _check(ctx, _planted(rng, rx, 9000, sigma=8), rx, offset=1, starts=True, what=expr).size >= 12
    expr = "((ab|c)d){8}"  # the same at 32 bits
    rx = ro.parse(expr)
    nl = ro.split(rx)[1]
    assert rx.m == 32 and all((nl >> (8 * b)) & 0xFF for b in range(4))
    assert _check(ctx, _planted(rng, rx, 9000, sigma=4), rx, offset=15, starts=True, what=expr).size >= 12


@pytest.mark.parametrize("kind", [0, 1])
def test_a_literal_is_the_class_search(ctx, kind):
    import torch

    for m in (1, 16, 32, 33, 64):
        spec = corpus.CorpusSpec(f"regex_exact_{kind}_{m}", 4 * corpus.MiB + 5, m, kind, seed=0x5EED2E10 + m,
                                 plant_period=1 << 12, boundary_period=1 << 20)
        d_text = spec.device_text(ctx)
        member = co.singletons(spec.pattern())
        member[m // 2] = True  # one wildcard
        rx = ro.Rx(member, 1, 1 << (m - 1), [1 << (i + 1) for i in range(m - 1)] + [0])
        assert ro.split(rx)[1] == 0
        out = torch.empty(d_text.numel(), dtype=torch.int64, device=d_text.device)
        starts, total = ctx.search_classes_device(d_text, co.pack(member), out=out)
        ends, total_r = ctx.search_regex_device(d_text, _struct(rx), capacity=max(total, 1))
        assert total_r == total >= 500 and torch.equal(ends, starts + (m - 1)), (kind, m)


def test_nothing_begins_in_front_of_an_unaligned_view(ctx):
    """The view begins 7 bytes into a 16-byte line and the bytes in front of it would fit: a match that begins out there
    and ends on one of the first ends is no match of the view."""
    rx = ro.parse("(..|.{9})y")
    view = b"y" * 40
    for front in (0, ord("y")):
        got, total = _gpu(ctx, _dev(ctx, view, 7, front), rx)
        assert total == 38 and np.array_equal(got, np.arange(2, 40)), (front, got[:4])
    rx = ro.parse("(x.{5}|abcdefgh)y")
    view = b"qqqyqqqqx12345yqq"
    got, total = _gpu(ctx, _dev(ctx, view, 7, ord("x")), rx)  # an x three bytes in front would end a match at view[3]
    assert got.tolist() == [14] == ro.ends_numpy(view, rx).tolist()
    rx = ro.parse("(a|b){1,32}")  # every alignment, every end a hit from byte 0 on
    for off in range(16):
        got, total = _gpu(ctx, _dev(ctx, b"ab" * 50, off, ord("a")), rx)
        assert total == 100 and np.array_equal(got, np.arange(100)), off


@pytest.mark.parametrize("expr", ["(ab|c)d[ab]?", "(a[abc]{2}|b){3,4}c", "([ab]c?){20}a"])
def test_lengths_at_piece_and_tile_edges(ctx, expr):
    rx = ro.parse(expr)
    p = piece(rx.max_len)
    assert p == {4: 64, 13: 64, 41: 256}[rx.max_len]
    rng = np.random.default_rng(rx.m)
    big = (rng.integers(0, 3, 3 * 256 * p + 5) + 0x61).astype(np.uint8)
    for at in range(0, big.size - rx.m, 997):
        ro.plant_path(rng, big, rx, at)
    for n in (0, 1, rx.min_len - 1, rx.min_len):  # views shorter than the shortest match, and one that can hold one
        got, total = _gpu(ctx, _dev(ctx, big[:n], 5), rx)
        want = ro.ends_numpy(big[:n].tobytes(), rx)
        assert total == want.size and np.array_equal(got, want) and (n >= rx.min_len or total == 0)
    for n in (p - 1, p, p + 1, 256 * p - 1, 256 * p, 256 * p + 1, 3 * 256 * p + 5):
        for off in (0, 9):
            assert _check(ctx, big[:n], rx, offset=off, what=(expr, n)).size > 0


def test_dense_tiles_next_to_empty_ones(ctx):
    """(a|b) on stretches of a and b: every end of a stretch is a hit, eight times what a tile's pool parks, so those
    tiles walk twice; the tiles between them hold nothing."""
    rng = np.random.default_rng(9)
    tile = 256 * piece(1)
    n = 5 * tile + 5
    text = np.full(n, ord("z"), np.uint8)
    for lo, hi in ((0, tile), (2 * tile - 100, 3 * tile + 77), (4 * tile + 3, n)):
        text[lo:hi] = rng.integers(0, 2, hi - lo) + 0x61
    rx = ro.parse("(a|b)")
    want = _check(ctx, text, rx, offset=7, starts=True)
    assert want.size == np.count_nonzero(text != ord("z")) > 2 * tile
    rx = ro.parse("(a|b)(a|bb)?")  # and with a table in the step
    assert ro.split(rx)[1] != 0
    _check(ctx, text, rx, offset=3, starts=True)
    _, total = _gpu(ctx, _dev(ctx, text, 7), rx, capacity=0)
    assert total == ro.ends_numpy(text.tobytes(), rx).size


def test_capacity_keeps_the_lowest_ends(ctx):
    import torch

    spec = corpus.CorpusSpec("regex_cap", 2 * corpus.MiB, 12, 1, seed=0x5EED2E00, plant_period=1 << 12)
    text = spec.host_text().tobytes()
    re_ = host.compile_regex("AC([ACGT]|[AC]{2,3})G(T|A)")
    rx = ro.parse("AC([ACGT]|[AC]{2,3})G(T|A)")
    want = ro.ends_numpy(text, rx)
    total = want.size
    assert total > 5000  # more than a tile parks
    d_text = spec.device_text(ctx)
    for cap in (0, 1, total - 1, total // 2):
        out = torch.full((max(cap, 1),), -1, dtype=torch.int64, device=d_text.device)
        n_matches = C.c_uint64(0)
        rc = ctx._L.bmx_search_regex_device(ctx._h, C.c_void_p(d_text.data_ptr()), d_text.numel(), 0, 0, C.byref(re_),
                                            C.c_void_p(out.data_ptr()), cap, C.byref(n_matches), None)
        assert rc == host.ERR_CAPACITY and n_matches.value == total, (cap, rc, n_matches.value)
        if cap:
            assert np.array_equal(out.cpu().numpy(), want[:cap]), cap
        else:
            assert int(out[0].item()) == -1
    got, t = _gpu(ctx, d_text, re_, capacity=total)  # exact
    assert t == total and np.array_equal(got, want)
    with pytest.raises(host.BmxError) as e:
        ctx.search_regex(text, re_, capacity=3)
    assert e.value.rc == host.ERR_CAPACITY


def test_lead_and_base_offset(ctx):
    rng = np.random.default_rng(4)
    text = (rng.integers(0, 2, 4000) + 0x61).astype(np.uint8).tobytes()
    rx = ro.parse("a(ab|b){1,2}b(.|aa)?a")
    want = ro.ends_numpy(text, rx)
    assert want.size > 300
    d_text = _dev(ctx, text, 3)
    base = 10 ** 12 + 7
    for n, lead in ((4000, 0), (4000, 1), (4000, 5), (4000, 1234), (4000, 3999), (4000, 4000), (2000, 1990), (6, 2), (0, 0)):
        got, total = _gpu(ctx, d_text, rx, n=n, lead=lead, base_offset=base)
        w = want[(want >= lead) & (want < n)] + base  # matches may begin in front of lead, never end behind n
        assert total == w.size and np.array_equal(got, w), (n, lead)


def test_shards_concatenate_to_the_whole_list(ctx):
    spec = corpus.CorpusSpec("regex_shards", 16 * corpus.MiB, 16, 1, seed=0x5EED2E01, plant_period=1 << 13,
                             boundary_period=1 << 20)
    d_text = spec.device_text(ctx)
    pat = spec.pattern().decode("latin-1")
    expr = pat[:3] + "(" + pat[3:6] + "|N{2})" + pat[6:9] + ".?" + pat[10:] + "(A|CG|T{1,3})?"
    re_ = host.compile_regex(expr, host.CLASS_IUPAC)
    rx = ro.parse(expr, ro.IUPAC)
    assert re_.max_len == rx.max_len == 19
    n = d_text.numel()
    whole, whole_t = _gpu(ctx, d_text, re_)
    assert whole_t > 1000 and whole.size == whole_t
    cuts = [0, 3 * corpus.MiB + 3, 5 * corpus.MiB, 5 * corpus.MiB + 1, 11 * corpus.MiB + 12345, n]
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        begin = max(a - (re_.max_len - 1), 0)  # the shard and its halo in front
        got, t = _gpu(ctx, d_text[begin:b], re_, lead=a - begin, base_offset=begin)
        parts.append(got)
    assert np.array_equal(np.concatenate(parts), whole)
    head = spec.host_text()[:corpus.MiB].tobytes()  # and the whole against the matcher on the first MiB
    assert np.array_equal(whole[whole < corpus.MiB], ro.ends_numpy(head, rx))


@pytest.mark.parametrize("expr,flags,kind", [("AC.{0,3}GT[AC].{0,3}TTG", 0, 1), ("ACN{1,3}GT", host.CLASS_IUPAC, 1),
                                            ("[Tt]he.{0,2}e?", 0, 0), ("x{30}a?b{1,3}", 0, 0)])
def test_without_groups_the_list_is_the_gapped_searchs(ctx, expr, flags, kind):
    import torch

    spec = corpus.CorpusSpec(f"regex_gaps_{kind}", 4 * corpus.MiB + 5, 16, kind, seed=0x5EED2E30 + kind, plant_period=1 << 14)
    text = spec.host_text().copy()
    rng = np.random.default_rng(23)
    rx = ro.parse(expr, flags)
    for at in range(100, text.size - 100, 4099):
        ro.plant_path(rng, text, rx, at)
    d_text = torch.from_numpy(text).to(f"cuda:{ctx.device}")[3:]
    want, total_g = ctx.search_gaps_device(d_text, expr, flags=flags, capacity=1 << 20)
    ends, total = ctx.search_regex_device(d_text, expr, flags=flags, capacity=1 << 20)
    assert total == total_g >= 1000 and torch.equal(ends, want)
    for longest in (False, True):
        s = ctx.regex_starts_device(d_text, expr, ends, longest=longest, flags=flags)
        assert torch.equal(s, ctx.gaps_starts_device(d_text, expr, want, longest=longest, flags=flags)), longest


@pytest.mark.parametrize("expr,flags,kind,count", [(WHY[0], 0, 1, 9), (WHY[1], 0, 0, 9), (WHY[3], host.CLASS_ICASE, 0, 8),
                                                  ("(a|bc|def){2}(g|hi)?", 0, 0, 27)])
def test_list_is_the_union_over_the_variants(ctx, expr, flags, kind, count):
    """On a 16 MiB corpus with copies of every variant planted: one pass of the regex kernel against one class-search
    pass per variant, merged."""
    import torch

    spec = corpus.CorpusSpec(f"regex_union_{kind}", 16 * corpus.MiB, 16, kind, seed=0x5EED2E20 + kind, plant_period=1 << 14)
    re_ = host.compile_regex(expr, flags)
    rx = ro.parse(expr, flags)
    vs = ro.variants(rx)
    assert len(vs) == count
    text = spec.host_text().copy()
    rng = np.random.default_rng(17)
    at = 1000
    for rep in range(40):
        for v in vs:
            at = ro.plant(rng, text, v, at) + 4099
    assert at < text.size
    d_text = torch.from_numpy(text).to(f"cuda:{ctx.device}")
    lists = []
    for v in vs:
        starts, total = ctx.search_classes_device(d_text, co.pack(v), capacity=1 << 20)
        assert total == starts.numel()
        lists.append(starts + (len(v) - 1))
    want = torch.unique(torch.cat(lists))  # sorted, each end once
    ends, total = ctx.search_regex_device(d_text, re_, capacity=1 << 20)
    assert total == want.numel() >= 40 * count and torch.equal(ends, want)
    s_short = ctx.regex_starts_device(d_text, re_, ends)
    s_long = ctx.regex_starts_device(d_text, re_, ends, longest=True)
    lens = {len(v) for v in vs}
    assert set((ends - s_short + 1).unique().tolist()) <= lens and set((ends - s_long + 1).unique().tolist()) <= lens
    assert bool((s_long <= s_short).all())


def test_starts_errors(ctx):
    import torch

    text = golden_file_bytes("input5L.txt.gz")
    d_text = _dev(ctx, text, 5)
    expr = "(occur{1,2}|refer)ences?"
    re_ = host.compile_regex(expr)
    rx = ro.parse(expr)
    ends, total = ctx.search_regex_device(d_text, re_, capacity=len(text), base_offset=100)
    assert total > 100
    s = ctx.regex_starts_device(d_text, re_, ends, base_offset=100)
    want_e, want_s = ro.starts_numpy(text, rx)
    assert np.array_equal(ends.cpu().numpy(), want_e + 100) and np.array_equal(s.cpu().numpy(), want_s + 100)
    for bad in (99, 100 + len(text)):  # an end outside [base_offset, base_offset + n)
        broken = ends.clone()
        broken[total // 2] = bad
        with pytest.raises(host.BmxError) as e:
            ctx.regex_starts_device(d_text, re_, broken, base_offset=100)
        assert e.value.rc == host.ERR_ARG and "outside the view" in str(e.value)
    with pytest.raises(host.BmxError) as e:  # the list of another expression
        ctx.regex_starts_device(d_text, "z(q|zz)zz", ends, base_offset=100)
    assert e.value.rc == host.ERR_ARG and "no match" in str(e.value)
    assert ctx.regex_starts_device(d_text, re_, ends[:0]).numel() == 0  # count == 0: no launch
    again = ctx.regex_starts_device(d_text, re_, ends, base_offset=100)  # and the status word is clean again
    assert torch.equal(again, s)


def test_entry_points_and_the_cli(ctx, tmp_path):
    text = golden_file_bytes("input5L.txt.gz")
    path = tmp_path / "input5L.txt"
    path.write_bytes(text)
    cases = [("(occur{1,2}|refer)ences?", 0, []), ("(THE|AND) [a-z]{2,5} ", host.CLASS_ICASE, ["--icase"]),
             ("([Tt]h(e|is|at) ){1,2}[a-z]", 0, []), ("(a|e|i|o|u){2}(r|n|)s", 0, [])]
    for expr, flags, opts in cases:
        rx = ro.parse(expr, flags)
        want_e, want_s = ro.starts_numpy(text, rx)
        _, want_l = ro.starts_numpy(text, rx, longest=True)
        assert want_e.size > 50, expr
        assert np.array_equal(ctx.search_regex(text, expr, flags).astype(np.int64), want_e)  # host entry point, expression
        assert np.array_equal(ctx.search_regex(text, host.compile_regex(expr, flags)).astype(np.int64), want_e)  # a Regex
        assert np.array_equal(host.search_regex(text, expr, flags).astype(np.int64), want_e)  # module level
        s, e = host.search_regex(text, expr, flags, spans=True)
        assert np.array_equal(e.astype(np.int64), want_e) and np.array_equal(s.astype(np.int64), want_s)
        s, e = host.search_regex(text, expr, flags, spans=True, longest=True)
        assert np.array_equal(e.astype(np.int64), want_e) and np.array_equal(s.astype(np.int64), want_l)
        s, e = ctx.search_regex_spans(text, expr, flags, longest=True)
        assert np.array_equal(e.astype(np.int64), want_e) and np.array_equal(s.astype(np.int64), want_l)
        ends, total = ctx.search_regex_device(_dev(ctx, text, 5), expr, flags=flags, capacity=len(text))
        assert total == want_e.size and np.array_equal(ends.cpu().numpy().astype(np.int64), want_e)
        assert ctx.last_regex_ms() > 0
        args = [CLI, "--regex", expr, "--text", str(path), "--iters", "2", "--positions", "--max-print", "3"] + opts
        r = subprocess.run(args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert f"regex matches: {want_e.size}" in r.stdout
        assert f"first end: {want_e[0]}\n" in r.stdout and f"last end: {want_e[-1]}\n" in r.stdout
        assert [int(x) for x in re.findall(r"End at : (\d+)", r.stdout)] == want_e[:3].tolist()
        assert "Average time" in r.stdout
        with_starts = ((["--starts"], want_s), (["--starts", "--longest"], want_l))
        for more, starts in with_starts if expr in (cases[0][0], cases[2][0]) else with_starts[:0]:
            r = subprocess.run(args + more, capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stderr
            got = [(int(a), int(b)) for a, b in re.findall(r"Match at : (\d+) (\d+)", r.stdout)]
            assert got == list(zip(starts[:3].tolist(), want_e[:3].tolist())), (expr, more)
    r = subprocess.run([CLI, "--regex", "a*", "--text", str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "bad regular expression" in r.stderr and "unbounded repetition" in r.stderr
    r = subprocess.run([CLI, "--regex", "a", "--gaps", "a", "--text", str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--regex goes with none of" in r.stderr


def test_on_a_callers_non_blocking_stream(ctx):
    """The rig of tests/test_gpu_streams.py, as tests/test_gpu_gaps.py uses it: the buffers hold DECOYS, the caller's
    non-blocking stream holds a long delay and then the copies of the real inputs, and each entry is called while those
    copies are still outstanding."""
    import torch

    from test_gpu_streams import Pending, delay, side_stream

    text = golden_file_bytes("input5L.txt.gz")
    decoy = text.replace(b"he", b"eh")  # the same length, other ends
    expr = "([Tt]he|an).{0,2}e"
    re_ = host.compile_regex(expr)
    rx = ro.parse(expr)
    want_e, want_s = ro.starts_numpy(text, rx)
    _, want_l = ro.starts_numpy(text, rx, longest=True)
    assert len(decoy) == len(text) and not np.array_equal(ro.ends_numpy(decoy, rx), want_e)
    assert want_e.size > 1000 and not np.array_equal(want_s[::-1], want_s)
    real_text = _dev(ctx, text, 0)
    real_ends = torch.from_numpy(want_e).to(real_text.device)
    out = torch.full((len(text),), -1, dtype=torch.int64, device=real_text.device)

    # the search, on a context of its own: its first call allocates and clears the look-back words and the ticket
    with host.Context(0) as fresh:
        for c, what in ((fresh, "search_regex_device, first call of a context"), (ctx, "search_regex_device")):
            d_text = _dev(ctx, decoy, 2)
            s = side_stream()
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                delay(s)
                d_text.copy_(real_text, non_blocking=True)
                pending = Pending(s)
                pending.assert_outstanding(what)
                ends, total = c.search_regex_device(d_text, re_, out=out)
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
            pending.assert_outstanding("regex_starts_device")
            got = ctx.regex_starts_device(d_text, re_, d_ends, longest=longest)
        assert np.array_equal(got.cpu().numpy(), want), longest
    side = side_stream()  # and the stream as an argument, torch's current one being the null stream
    torch.cuda.synchronize()
    ends, total = ctx.search_regex_device(real_text, re_, out=out, stream=side)
    got = ctx.regex_starts_device(real_text, re_, ends, stream=side)
    assert total == want_e.size and np.array_equal(ends.cpu().numpy(), want_e) and np.array_equal(got.cpu().numpy(), want_s)


def test_repeat_calls_interleaved_with_the_other_searches(ctx):
    """The regex, the gapped and the class search share the look-back code, not their state."""
    import gaps_oracle as go

    text = golden_file_bytes("input5L.txt.gz")
    d_text = _dev(ctx, text, 11)
    expr = "(occur{1,2}|refer)ences?"
    rx = ro.parse(expr, ro.ICASE)
    pair = host.compile_gaps("occur{1,2}ences?", host.CLASS_ICASE)
    member = co.parse("occurrences", co.ICASE)
    want = ro.ends_numpy(text, rx)
    want_g = go.gap_ends(text, co.unpack(pair[0]), pair[1])
    want_c = co.class_starts(text, member)
    for _ in range(3):
        ends, t = ctx.search_regex_device(d_text, expr, flags=host.CLASS_ICASE, capacity=len(text))
        assert t == want.size and np.array_equal(ends.cpu().numpy(), want)
        assert ctx.last_regex_ms() >= 0
        ends, t = ctx.search_gaps_device(d_text, pair, capacity=len(text))
        assert t == want_g.size and np.array_equal(ends.cpu().numpy(), want_g)
        pos, t = ctx.search_classes_device(d_text, co.pack(member), capacity=len(text))
        assert t == want_c.size and np.array_equal(pos.cpu().numpy(), want_c)
    assert set(want_g.tolist()) <= set(want.tolist()) and want_g.size > 100
