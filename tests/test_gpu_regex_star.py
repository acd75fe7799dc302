"""GPU suite for the regular-expression search with unbounded repetition (bmx_search_regex_star_device /
bmx_search_regex_star / bmx_search_regex_star_spans / bmx_regex_star_starts_device): full lists compared with the
set-carrying matcher of tests/regex_star_oracle.py, on the fast path, on the slow path forced by the experiments knob and
on the slow path that a tainted call takes by itself, at geometries where chains of pieces cross tiles and workgroups."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import classes_oracle as co
import regex_oracle as ro
import regex_star_oracle as so
from conftest import ROOT
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "parallel_implementation_of_string_matching_algorithms_opencl_amd", "bin", "bmx_cli")

NO_START = np.uint64(so.NO_START)


def _dev(ctx, data, offset: int = 0, front: int = 0):
    """data on the device, starting `offset` bytes into a buffer (any alignment); the bytes in front of it hold `front`."""
    import torch

    data = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data
    buf = torch.full((data.size + offset + 16,), front, dtype=torch.uint8, device=f"cuda:{ctx.device}")
    if data.size:
        buf[offset:offset + data.size] = torch.from_numpy(data.copy()).to(buf.device)
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
    ends, total = ctx.search_regex_star_device(d_text, rx if isinstance(rx, host.Regex) else _struct(rx), capacity=cap, **kw)
    return ends.cpu().numpy().astype(np.int64), total


def _check(ctx, text, rx, offset: int = 0, what=None, front: int = 0):
    text = bytes(text)
    want = so.ends_numpy(text, rx)
    got, total = _gpu(ctx, _dev(ctx, text, offset, front), rx)
    assert total == want.size, (what, len(text), rx.m, offset, total, want.size)
    assert np.array_equal(got, want), (what, len(text), rx.m, offset)
    return want


def _planted(rng, rx, n, base=0x61, sigma=4, copies=6):
    text = (rng.integers(0, sigma, n) + base).astype(np.uint8)
    for _ in range(copies):
        if n:
            so.plant_path(rng, text, rx, int(rng.integers(0, n)), stop=0.1)
    return text


def test_random_expressions_against_oracle(ctx):
    """210 expressions over 2, 4 and 95 symbols, texts of 0 to 4,096 bytes at the sixteen alignments of the view."""
    rng = np.random.default_rng(0x57A700)
    empty = cyclic = wide = 0
    cases = 210
    for case in range(cases):
        sigma = (2, 4, 95)[case % 3]
        n = int(rng.integers(0, 4097)) if case % 10 else int(rng.integers(0, 40))
        base = 0x20 if sigma == 95 else 0x61
        symbols = np.arange(base, base + sigma)
        expr, rx = so.random_regex(rng, symbols, max_m=(8, 32, 64)[case % 7 % 3])
        text = _planted(rng, rx, n, base, sigma, copies=8)
        want = _check(ctx, text, rx, offset=case % 16, what=expr)
        empty += want.size == 0
        cyclic += rx.max_len == so.UNBOUNDED
        wide += rx.m > 32
        if 0 < want.size <= 300:  # the starts of the shortest and the longest match within a window
            import torch

            d_text = _dev(ctx, text, case % 16)
            d_ends = torch.from_numpy(want).to(d_text.device)
            for longest in (False, True):
                if rx.max_len != so.UNBOUNDED and rx.max_len > 64:
                    continue
                s = ctx.regex_star_starts_device(d_text, _struct(rx), d_ends, window=64, longest=longest)
                assert np.array_equal(s.cpu().numpy().astype(np.uint64), so.starts_numpy(text, rx, want, 64, longest)), (expr, longest)
    assert 10 * empty < cases, empty
    assert cyclic >= 100 and wide >= 5, (cyclic, wide)


@pytest.mark.parametrize("expr", ["a+", "x{31}a+", "x{32}a+", "x{63}a+", "x{30}y+z", "x{31}y+z", "x{32}y+z", "x{30}(abcd)+z",
                                  "(x{32})+y", "x{20}(a|bc)+x{20}d"])
def test_word_widths_loops_and_back_edges(ctx, expr):
    """m = 1, 32, 33 and 64, a self-loop on position 31 / 32 and back edges that cross the word halves."""
    rng = np.random.default_rng(len(expr) * 977)
    rx = so.parse(expr)
    text = _planted(rng, rx, 3000, sigma=3, copies=10)
    text[rng.integers(0, 3000, 300)] = ord("x")
    want = _check(ctx, text, rx, offset=5, what=expr)
    assert want.size > 0, expr


def _forced(c, text, rx, offset=0, **kw):
    c.set_knob("regex_star_force_slow", 1)
    got = _gpu(c, _dev(c, text, offset), rx, **kw)
    last = c.regex_star_last()
    c.set_knob("regex_star_force_slow", 0)
    assert last["slow"] == 1
    return got, last


@pytest.mark.parametrize("ps,grid", [(4, 1), (5, 2), (6, 3)])
def test_forced_slow_path_equals_fast_path_equals_oracle(exp_ctx, ps, grid):
    """64 KiB, pieces of 16 to 64 bytes and one to three workgroups: chains cross pieces, tiles and workgroups."""
    rng = np.random.default_rng(0x57A710 + ps)
    exp_ctx.set_knob("regex_star_piece_shift", ps)
    _gpu(exp_ctx, _dev(exp_ctx, b"abc"), so.parse("a+"))  # (the shared geometry knobs reach the sessions a context already has)
    exp_ctx.set_knob("tile_max_grid", grid)
    n = 1 << 16
    for case, expr in enumerate(["[ab]+c", "a(b|cd)*a", "a.*d", "(ab|ba)+[cd]{2,}", r"[ab]+c[ab]+", "x{33}(a|b)+c"]):
        rx = so.parse(expr)
        text = _planted(rng, rx, n, sigma=4, copies=40)
        want = so.ends_numpy(text, rx)
        (slow, total), last = _forced(exp_ctx, text, rx, offset=case)
        assert last["piece_shift"] == ps and exp_ctx.last_launch("regex_star")[:2] == (ps, grid), last
        assert total == want.size and np.array_equal(slow, want), (expr, ps)
        fast, total = _gpu(exp_ctx, _dev(exp_ctx, text, case), rx)
        assert total == want.size and np.array_equal(fast, want), (expr, ps)
        assert want.size > 0, expr


def test_natural_taint_takes_the_slow_path_and_is_exact(exp_ctx):
    """a.*b on a text whose only a lies in the last 1,000 bytes: every lane's upper bound keeps the loop alive, the lower
    one does not.  Then the single a at view byte 0, where every later end is a hit: dense tiles, the second walk, and
    capacities cut short."""
    rng = np.random.default_rng(0x57A720)
    n = 1 << 16
    rx = so.parse("a.*b")
    text = (rng.integers(1, 4, n) + 0x61).astype(np.uint8)  # b, c, d
    text[n - 700] = ord("a")
    want = so.ends_numpy(text, rx)
    assert 100 < want.size < 700
    for ps in (0, 4):
        exp_ctx.set_knob("regex_star_piece_shift", ps)
        got, total = _gpu(exp_ctx, _dev(exp_ctx, text, 3), rx)
        last = exp_ctx.regex_star_last()
        assert last["tainted"] > 0 and last["slow"] == 1 and last["columns"] > 0, last
        assert total == want.size and np.array_equal(got, want), ps
    rx = so.parse("a.*")
    text = (rng.integers(1, 4, n) + 0x61).astype(np.uint8)
    text[0] = ord("a")
    for ps, cap in ((0, n), (0, 1000), (5, 5000), (0, 0)):
        exp_ctx.set_knob("regex_star_piece_shift", ps)
        got, total = _gpu(exp_ctx, _dev(exp_ctx, text, 7), rx, capacity=cap)
        last = exp_ctx.regex_star_last()
        assert last["tainted"] > 0 and last["slow"] == 1, last
        assert total == n and np.array_equal(got, np.arange(min(cap, n))), (ps, cap)


def test_many_columns_codon_loop(exp_ctx):
    """ATG([ACGT]{3})+(TAA|TAG|TGA) on ACGT with the stop codons taken out of a long stretch."""
    rng = np.random.default_rng(0x57A730)
    rx = so.parse("ATG([ACGT]{3})+(TAA|TAG|TGA)")
    n = 1 << 16
    text = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].copy()
    stretch = text[8000:56000]
    s = stretch.tobytes().replace(b"ATG", b"ACG")  # one open frame only: the lower bound knows one, the upper one three
    for stop in (b"TAA", b"TAG", b"TGA"):
        s = s.replace(stop, b"TCC")
    text[8000:56000] = np.frombuffer(s, np.uint8)
    text[8100:8103] = np.frombuffer(b"ATG", np.uint8)
    want = so.ends_numpy(text, rx)
    assert want.size > 50
    for ps in (0, 4, 6):
        exp_ctx.set_knob("regex_star_piece_shift", ps)
        got, total = _gpu(exp_ctx, _dev(exp_ctx, text, 1), rx)
        assert total == want.size and np.array_equal(got, want), ps
    assert exp_ctx.regex_star_last()["slow"] == 1


def test_lead_base_offset_and_short_views(ctx):
    rng = np.random.default_rng(0x57A740)
    rx = so.parse("a[bc]+d")
    text = _planted(rng, rx, 9000, sigma=4, copies=60)
    want = so.ends_numpy(text, rx)
    d_text = _dev(ctx, text, 9)
    for lead in (0, 1, 255, 256, 257, 4097, 8999, 9000):
        got, total = _gpu(ctx, d_text, rx, lead=lead, base_offset=1 << 41)
        sel = want[want >= lead]
        assert total == sel.size and np.array_equal(got, sel + (1 << 41)), lead
    # a view shorter than min_len, and one piece and one tile +- 1 (a piece is 256 ends here, a tile 256 pieces)
    for n in (0, 1, 2, 3, 255, 256, 257, 65535, 65536, 65537):
        t = _planted(rng, rx, n, sigma=4, copies=n // 100)
        _check(ctx, t, rx, offset=n % 16, what=n)
    # a match that would begin in front of an unaligned view is not reported: the bytes in front are all 'a'
    rx = so.parse("a+b")
    t = np.frombuffer(b"bbbab" + b"c" * 40 + b"b", np.uint8)
    for offset in range(1, 16):
        assert _check(ctx, t, rx, offset=offset, front=ord("a")).tolist() == [4]


def test_acyclic_automaton_gives_the_star_free_list(ctx):
    rng = np.random.default_rng(0x57A750)
    for case in range(30):
        symbols = np.arange(0x61, 0x64)
        expr, rx = ro.random_regex(rng, symbols, (8, 32, 64)[case % 3])
        text = (rng.integers(0, 3, 5000) + 0x61).astype(np.uint8)
        ro.plant_path(rng, text, rx, 100)
        d_text = _dev(ctx, text, case % 16)
        a, ta = ctx.search_regex_device(d_text, expr, capacity=5000)
        b, tb = ctx.search_regex_star_device(d_text, expr, capacity=5000)
        assert ta == tb and np.array_equal(a.cpu().numpy(), b.cpu().numpy()), expr


def test_starts_windows_sentinel_and_status_errors(ctx):
    import torch

    rng = np.random.default_rng(0x57A760)
    rx = so.parse("a[bc]*d")
    text = (rng.integers(1, 3, 6000) + 0x61).astype(np.uint8)  # b, c
    for at, length in ((10, 2), (100, 7), (300, 9), (1000, 70), (2000, 5000 - 2000)):
        text[at], text[at + length - 1] = ord("a"), ord("d")
    want = so.ends_numpy(text, rx)
    assert want.tolist() == [11, 106, 308, 1069, 4999]
    d_text = _dev(ctx, text, 11)
    d_ends = torch.from_numpy(want + 77).to(d_text.device)
    for window in (1, 8, 64, 4096):
        for longest in (False, True):
            s = ctx.regex_star_starts_device(d_text, _struct(rx), d_ends, window=window, longest=longest, base_offset=77)
            ref = so.starts_numpy(text, rx, want, window, longest)
            ref = np.where(ref == NO_START, NO_START, ref + np.uint64(77))
            assert np.array_equal(s.cpu().numpy().astype(np.uint64), ref), (window, longest)
    assert so.starts_numpy(text, rx, want, 8).tolist() == [10, 100, so.NO_START, so.NO_START, so.NO_START]
    assert so.starts_numpy(text, rx, want, 4096, True).tolist() == [10, 100, 300, 1000, 2000]
    # a one-byte match is told from no match
    rx1 = so.parse("d|ab+d")
    w1 = so.ends_numpy(text, rx1)
    s = ctx.regex_star_starts_device(d_text, _struct(rx1), torch.from_numpy(w1).to(d_text.device), window=1)
    assert np.array_equal(s.cpu().numpy(), w1)
    # the status errors: an end outside the view; an end without a match when no longer match can exist
    with pytest.raises(host.BmxError) as e:
        ctx.regex_star_starts_device(d_text, _struct(rx), torch.tensor([6000], device=d_text.device), window=8)
    assert e.value.rc == host.ERR_ARG
    with pytest.raises(host.BmxError) as e:
        ctx.regex_star_starts_device(d_text, "ab{0,3}d", torch.tensor([5], device=d_text.device), window=8)
    assert e.value.rc == host.ERR_ARG
    s = ctx.regex_star_starts_device(d_text, "ab{0,30}d", torch.tensor([5], device=d_text.device), window=8)  # a longer one may exist
    assert s.cpu().numpy().astype(np.uint64).tolist() == [so.NO_START]


def test_host_entries_streams_and_interleaved_calls(ctx, exp_ctx):
    import torch

    rng = np.random.default_rng(0x57A770)
    expr = r"[0-9]+\.[0-9]+"
    rx = so.parse(expr)
    text = np.frombuffer(b".0123456789", np.uint8)[rng.integers(0, 11, 20000)].copy()
    text[5] = ord("/")  # the only one: the warm-up of no lane sees it
    want = so.ends_numpy(text, rx)
    assert want.size > 1000
    assert np.array_equal(ctx.search_regex_star(text, expr).astype(np.int64), want)
    assert np.array_equal(host.search_regex_star(text, expr).astype(np.int64), want)
    with pytest.raises(host.BmxError) as e:
        ctx.search_regex_star(text, expr, capacity=10)
    assert e.value.rc == host.ERR_CAPACITY
    starts, ends = ctx.search_regex_star_spans(text, expr, window=64)
    assert np.array_equal(ends.astype(np.int64), want) and np.array_equal(starts, so.starts_numpy(text, rx, want, 64))
    starts, ends = host.search_regex_star(text, expr, spans=True, longest=True, window=16)
    assert np.array_equal(starts, so.starts_numpy(text, rx, want, 16, True))
    assert ctx.last_regex_star_ms() > 0
    # a caller's non-blocking stream
    d_text = _dev(ctx, text, 3)
    stream = torch.cuda.Stream(device=d_text.device)
    with torch.cuda.stream(stream):
        got, total = ctx.search_regex_star_device(d_text, expr, capacity=20000, stream=stream)
    assert total == want.size and np.array_equal(got.cpu().numpy(), want)
    # interleaved with the star-free search on one context, and the fast and the slow path in turn: the workspace is
    # reused and no status tag goes stale
    free = "[0-9]{1,3}\\."
    free_want = ro.ends_numpy(text, ro.parse(free))
    tainted = so.parse("/.*\\.\\.")
    tainted_want = so.ends_numpy(text, tainted)
    d_text = _dev(exp_ctx, text, 3)
    for turn in range(6):
        got, total = _gpu(exp_ctx, d_text, rx)
        assert total == want.size and np.array_equal(got, want), turn
        assert exp_ctx.regex_star_last()["slow"] == 0
        a, ta = exp_ctx.search_regex_device(d_text, free, capacity=20000)
        assert ta == free_want.size and np.array_equal(a.cpu().numpy(), free_want), turn
        got, total = _gpu(exp_ctx, d_text[: 20000 - 1000 * turn], tainted)
        sel = tainted_want[tainted_want < 20000 - 1000 * turn]
        assert total == sel.size and np.array_equal(got, sel), turn
        assert exp_ctx.regex_star_last()["slow"] == 1


def test_cli(ctx, tmp_path):
    rng = np.random.default_rng(0x57A780)
    expr = "a[bc]+d"
    rx = so.parse(expr)
    text = _planted(rng, rx, 5000, sigma=4, copies=30)
    want = so.ends_numpy(text, rx)
    path = tmp_path / "text.bin"
    path.write_bytes(text.tobytes())
    common = [CLI, "--regex-star", expr, "--text", str(path), "--iters", "1", "--positions", "--max-print", "100000"]
    out = subprocess.run(common, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "matches of 3 or more bytes" in out.stdout and f"regex matches: {want.size}" in out.stdout
    assert [int(x) for x in re.findall(r"End at : (\d+)", out.stdout)] == want.tolist()
    for longest in (False, True):
        out = subprocess.run(common + ["--starts", "--window", "8"] + (["--longest"] if longest else []), capture_output=True,
                             text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        pairs = [(int(a), int(b)) for a, b in re.findall(r"Match at : (\d+) (\d+)", out.stdout)]
        assert [b for _, b in pairs] == want.tolist()
        assert [a for a, _ in pairs] == so.starts_numpy(text, rx, want, 8, longest).tolist()
    for bad in (["--regex", "ab"], ["--gaps", "ab"], ["--classes", "ab"], ["--approx", "1"], ["--starts"], ["--window", "8"],
                ["--starts", "--window", "0"], ["--starts", "--window", "65537"]):
        out = subprocess.run(common + bad, capture_output=True, text=True, timeout=120)
        assert out.returncode == 2, (bad, out.stdout, out.stderr)
    out = subprocess.run([CLI, "--regex-star", "a**", "--text", str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 1 and "bmx_compile_regex_star" in out.stderr
