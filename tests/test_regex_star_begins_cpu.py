"""CPU suite of the begins search and the ends pass for expressions with * + {a,} and of leftmost-longest matching with
them: the oracles of regex_star_begins_oracle.py against each other, the selection rule against the sequential POSIX
definition, the example that separates POSIX from the merge and the shortest routes, the downward slow path and the model
of the first launch, every argument error of the new C entries with ctx = NULL, the exports and the ValueErrors of
``posix``.  No GPU is touched."""
import ctypes as C

import numpy as np
import pytest

import regex_star_begins_oracle as sb
import regex_star_oracle as sr
import subst_oracle as so
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host
import parallel_implementation_of_string_matching_algorithms_opencl_amd as pkg

PAIRS = 300


def _pairs():
    """300 (text, expression, automaton with a cycle): alphabets of 2 and 3 symbols, texts of up to 13 bytes (``re``
    backtracks: nested loops on longer texts take minutes, as test_regex_star_cpu.py found)."""
    rng = np.random.default_rng(0x5B6145)
    for case in range(PAIRS):
        symbols = np.arange(97, 97 + 2 + case % 2)
        text = rng.choice(symbols, int(rng.integers(0, 14))).astype(np.uint8).tobytes()
        expr, rx = sr.random_regex(rng, symbols, 6, cyclic=True)
        yield text, expr, rx


@pytest.fixture(scope="module")
def pairs():
    return [(t, e, rx, sb.begins_brute(t, e)) for t, e, rx in _pairs()]


def test_the_oracles_agree(pairs):
    seen = 0
    for text, expr, rx, (starts, short, long_) in pairs:
        assert sb.begins_numpy(text, rx).tolist() == starts, (text, expr)
        for longest, want in ((False, short), (True, long_)):
            ends, clipped = sb.ends_numpy(text, rx, starts, 64, longest=longest)
            assert ends.tolist() == want and clipped == 0, (text, expr, longest)
        assert sb.posix_matches(text, rx) == sb.posix_brute(text, expr), (text, expr)
        seen += len(starts)
    assert seen > 500  # (the pairs are not vacuous)


def test_a_window_shortens_and_counts_what_it_cut(pairs):
    clipped_seen = 0
    for text, expr, rx, (starts, short, long_) in pairs:
        for window in (1, 2, 5):
            ends, clipped = sb.ends_numpy(text, rx, starts, window, longest=True)
            pat = sr.to_re(expr)
            for s, e, full in zip(starts, ends.tolist(), long_):
                inside = [j for j in range(s, min(s + window, len(text))) if pat.fullmatch(text, s, j + 1)]
                assert e == (inside[-1] if inside else sb.NONE), (text, expr, window, s)
                assert full - s + 1 <= window or clipped > 0, (text, expr, window, s)  # a longer match never goes unseen
            clipped_seen += clipped
    assert clipped_seen > 100


def test_disjoint_selection_on_the_start_sorted_list_is_leftmost_longest(pairs):
    differs = 0
    for text, expr, rx, (starts, short, long_) in pairs:
        spans = so.spans_of(starts=np.array(starts, np.uint64), ends=np.array(long_, np.uint64))
        assert so.ordered(spans), (text, expr)
        s, e, _ = so.select(spans)
        want = sb.posix_matches(text, rx)
        assert list(zip(s.tolist(), e.tolist())) == want, (text, expr)
        st, en = so.all_matches(sr.to_re(expr).pattern, text)
        s3, e3, _ = so.select(so.spans_of(starts=st, ends=en))
        differs += list(zip(s3.tolist(), e3.tolist())) != want
    assert differs > 10


def test_posix_is_neither_the_merge_nor_the_shortest_route():
    """ab|bc+ on abcc: POSIX takes ab alone; the union of overlapping matches is abcc; and for [0-9]+ the shortest route
    takes single digits."""
    text, expr = b"abcc", "ab|bc+"
    rx = sr.parse(expr)
    assert sb.posix_matches(text, rx) == sb.posix_brute(text, expr) == [(0, 1)]
    pat = sr.to_re(expr).pattern
    st, en = so.all_matches(pat, text, longest=True)
    ms, me, _ = so.merge(so.spans_of(starts=st, ends=en))
    assert list(zip(ms.tolist(), me.tolist())) == [(0, 3)]
    st, en = so.all_matches(pat, text)
    ss, se, _ = so.select(so.spans_of(starts=st, ends=en))
    assert list(zip(ss.tolist(), se.tolist())) == [(0, 1)]  # the shortest route agrees here ...
    digits, rd = b"x123y45", sr.parse("[0-9]+")
    st, en = so.all_matches(sr.to_re("[0-9]+").pattern, digits)
    ss, se, _ = so.select(so.spans_of(starts=st, ends=en))
    assert list(zip(ss.tolist(), se.tolist())) == [(1, 1), (2, 2), (3, 3), (5, 5), (6, 6)]  # ... and not here
    assert sb.posix_matches(digits, rd) == [(1, 3), (5, 6)]


def test_per_row_limit_and_window_in_the_sequential_definition():
    text = b"ab\nbb a\nb"
    rx = sr.parse("a[^c]*b")
    cuts = [i for i, c in enumerate(text) if c == 10]
    limit_of = lambda s: next((c for c in cuts if c >= s), len(text) - 1)
    assert sb.posix_matches(text, rx) == [(0, 8)]
    assert sb.posix_matches(text, rx, limit_of=limit_of) == [(0, 1)]  # the a of row 1 has no b in its row
    assert sb.posix_matches(text, rx, window=4) == [(0, 3), (6, 8)]


@pytest.mark.parametrize("expr", ["[ab]+", "c[ab]*d", "(ab|b)+c", "a.*b", "[ab].*c", "(a|bb)*c{2,}"])
def test_the_downward_slow_path_is_the_oracle(expr):
    rng = np.random.default_rng(len(expr))
    rx = sr.parse(expr)
    for ps in (4, 5, 6):
        for first in range(16):
            n = int(rng.integers(1, 200))
            text = rng.choice(np.frombuffer(b"abcd", np.uint8), n).tobytes()
            tail = int(rng.integers(0, 3)) * int(rng.integers(0, n + 1)) // 2
            want = sb.begins_numpy(text, rx)
            want = want[want < n - tail]
            assert np.array_equal(sb.slow_begins(text, rx, first, tail, ps), want), (expr, ps, first, n, tail)


def test_a_sweep_without_columns_misses_starts():
    text = b"a" + b"x" * 100 + b"c"
    rx = sr.parse("[ab].*c")
    assert sb.slow_begins(text, rx, 3, 0, 4).tolist() == [0]
    assert sb.slow_begins(text, rx, 3, 0, 4, use_columns=False).tolist() == []


def test_the_model_of_the_first_launch():
    """No taint for [ab]+ on one-byte background (one other byte empties both states); taint for [ab].*c with the single c
    on the view's last byte (above a lane the lower bound never saw the c's `.*`, the upper bound keeps it)."""
    n, ps, warm = 20000, 4, 64
    text = bytearray(b"x" * n)
    for at in (5, 300, 301, 302, 4095, 4096, 19999):
        text[at] = ord("a")
    rx = sr.parse("[ab]+")
    for first in (0, 7):
        m = sb.fast_taint_down(text, rx, first, 0, ps, warm)
        assert m.waves == 0 and np.array_equal(m.starts, sb.begins_numpy(text, rx))
    text = bytearray(b"x" * n)
    text[10], text[9000], text[n - 1] = ord("a"), ord("b"), ord("c")
    rx = sr.parse("[ab].*c")
    m = sb.fast_taint_down(text, rx, 5, 0, ps, warm)
    assert m.waves > 0 and m.starts.tolist() == []  # every lane far below the c walks from the empty lower bound
    assert sb.begins_numpy(text, rx).tolist() == [10, 9000]
    assert sb.slow_begins(text, rx, 5, 0, ps).tolist() == [10, 9000]
    near = sb.fast_taint_down(text[n - 200:], rx, 5, 0, 8, 4096)  # a warm-up that reaches the view's end is exact
    assert near.waves == 0


def _broken():
    def edit(**kw):
        r = host.compile_regex_star("(a|bc)+d")
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    return [("m = 0", edit(m=0)), ("m = 65", edit(m=65)), ("first empty", edit(first=0)), ("last beyond m", edit(last=1 << 63))]


def test_every_argument_error_before_any_device_call(built):
    L = host.lib()
    text = b"some text to search in"
    n = len(text)
    out = (C.c_uint64 * 8)()
    total, clipped = C.c_uint64(0), C.c_uint64(7)
    t, c = C.byref(total), C.byref(clipped)
    r = host.compile_regex_star("(a|bc)+d")
    p = C.byref(r)
    dev, ends = L.bmx_search_regex_star_begins_device, L.bmx_regex_star_ends_device
    hb, hs = L.bmx_search_regex_star_begins, L.bmx_search_regex_star_begins_spans
    for what, bad in _broken():
        b = C.byref(bad)
        assert dev(None, None, 10, 0, 0, b, None, 0, t, None) == host.ERR_ARG, what
        assert ends(None, None, 10, 0, b, out, 0, None, 16, 0, out, c, None) == host.ERR_ARG, what  # even with count == 0
        assert hb(None, text, n, b, out, 8, t) == host.ERR_ARG, what
        assert hs(None, text, n, b, 16, 0, out, out, 8, t, c) == host.ERR_ARG, what
    assert dev(None, None, 10, 0, 0, None, None, 0, t, None) == host.ERR_ARG  # no automaton
    assert dev(None, None, 10, 11, 0, p, None, 0, t, None) == host.ERR_ARG  # tail > n
    assert dev(None, None, 1 << 40, 0, 0, p, None, 0, t, None) == host.ERR_ARG
    assert dev(None, None, 10, 0, 0, p, None, 8, t, None) == host.ERR_ARG  # capacity, no starts
    assert dev(None, None, 10, 0, 0, p, None, 0, t, None) == host.ERR_ARG  # no context
    assert dev(None, None, 10, 10, 0, p, None, 0, t, None) == host.ERR_ARG  # ... even where tail == n owns nothing
    assert ends(None, None, 10, 0, None, out, 8, None, 16, 0, out, c, None) == host.ERR_ARG
    assert ends(None, None, 10, 0, p, out, 8, None, 16, 2, out, c, None) == host.ERR_ARG  # an unknown flag bit
    assert ends(None, None, 10, 0, p, out, 8, None, 0, 0, out, c, None) == host.ERR_ARG  # window out of range
    assert ends(None, None, 10, 0, p, out, 8, None, host.MAX_REGEX_STAR_WINDOW + 1, 0, out, c, None) == host.ERR_ARG
    assert ends(None, None, 1 << 40, 0, p, out, 8, None, 16, 0, out, c, None) == host.ERR_ARG
    assert ends(None, None, 10, 0, p, None, 8, None, 16, 0, out, c, None) == host.ERR_ARG
    assert ends(None, None, 10, 0, p, out, 8, None, 16, 0, None, c, None) == host.ERR_ARG
    assert ends(None, None, 10, 0, p, out, 8, out, 16, host.REGEX_LONGEST, out, c, None) == host.ERR_ARG  # no context
    assert ends(None, None, 10, 0, p, None, 0, None, 16, 0, None, c, None) == host.OK and clipped.value == 0  # count == 0
    assert ends(None, None, 10, 0, p, None, 0, None, 16, 0, None, None, None) == host.OK  # the count is optional
    assert hb(None, text, n, None, out, 8, t) == host.ERR_ARG
    assert hb(None, text, n, p, None, 8, t) == host.ERR_ARG  # a capacity needs room
    assert hb(None, None, n, p, out, 8, t) == host.ERR_ARG
    assert hb(None, text, 1 << 40, p, out, 8, t) == host.ERR_ARG
    assert hb(None, text, 0, p, out, 8, t) == host.OK and total.value == 0  # an empty text: no device needed
    assert hs(None, text, n, None, 16, 0, out, out, 8, t, c) == host.ERR_ARG
    assert hs(None, text, n, p, 16, 0, None, out, 8, t, c) == host.ERR_ARG
    assert hs(None, text, n, p, 16, 0, out, None, 8, t, c) == host.ERR_ARG
    assert hs(None, None, n, p, 16, 0, out, out, 8, t, c) == host.ERR_ARG
    assert hs(None, text, n, p, 16, 2, out, out, 8, t, c) == host.ERR_ARG  # an unknown flag bit
    assert hs(None, text, n, p, 0, 0, out, out, 8, t, c) == host.ERR_ARG  # window out of range
    assert hs(None, text, n, p, host.MAX_REGEX_STAR_WINDOW + 1, 0, out, out, 8, t, c) == host.ERR_ARG
    assert hs(None, text, 1 << 40, p, 16, 0, out, out, 8, t, c) == host.ERR_ARG
    assert hs(None, text, 0, p, 16, 0, out, out, 8, t, None) == host.OK
    assert L.bmx_last_regex_star_begins_ms(None) < 0
    # the star-free begins search still refuses a cycle
    assert L.bmx_search_regex_begins_device(None, None, 10, 0, 0, p, None, 0, t, None) == host.ERR_ARG


def test_exports(built):
    L, X = C.CDLL(host.LIB_PATH), C.CDLL(host.EXP_LIB_PATH)
    for name in ("bmx_search_regex_star_begins_device", "bmx_last_regex_star_begins_ms", "bmx_regex_star_ends_device",
                 "bmx_search_regex_star_begins", "bmx_search_regex_star_begins_spans"):
        assert hasattr(L, name) and hasattr(X, name), name
        assert name in [s for s, _, _ in host.SYMBOLS]
    assert hasattr(X, "bmx_exp_regex_star_begins_last") and not hasattr(L, "bmx_exp_regex_star_begins_last")
    assert pkg.search_regex_star_begins is host.search_regex_star_begins
    for name in ("search_regex_star_begins_device", "regex_star_ends_device", "search_regex_star_begins",
                 "search_regex_star_begins_spans", "last_regex_star_begins_ms"):
        assert callable(getattr(host.Context, name))


def test_posix_takes_the_star_kind_and_refuses_what_it_refused():
    host._posix_args(kind="regex_star")
    host._posix_args(kind="regex")
    for kw in (dict(kind="gaps"), dict(kind="regex_star", merge=True), dict(kind="regex_star", longest=True),
               dict(kind="regex_star", longest=False), dict(kind="classes")):
        with pytest.raises(ValueError):
            host._posix_args(**kw)
        with pytest.raises(ValueError):
            host.sub(b"abc", "b+", b"x", posix=True, **kw)
        with pytest.raises(ValueError):
            host.findall(b"abc", "b+", posix=True, **kw)


class _Stub:
    """A context whose star entries answer without a GPU: one start, its end, and a clipped count."""

    def __init__(self, clipped):
        self.clipped, self.windows = clipped, []

    def search_regex_star_begins_device(self, d_text, re_, out=None):
        import torch

        return torch.tensor([1]), 1

    def regex_star_ends_device(self, d_text, re_, starts, window, longest, limit):
        assert longest and limit is None
        self.windows.append(window)
        import torch

        return torch.tensor([3]), self.clipped


def test_a_clipped_run_is_a_value_error_naming_count_and_window(built):
    stub = _Stub(2)
    with pytest.raises(ValueError, match=r"2 match.*window of 4096"):
        host.Context._posix_spans_device(stub, None, "[0-9]+", None, 0, "regex_star", None)
    with pytest.raises(ValueError, match=r"window of 77"):
        host.Context._posix_spans_device(stub, None, "[0-9]+", None, 0, "regex_star", 77)
    ok = _Stub(0)
    starts, ends, ids = host.Context._posix_spans_device(ok, None, "[0-9]+", None, 0, "regex_star", None)
    assert starts.tolist() == [1] and ends.tolist() == [3] and ids is None and ok.windows == [4096]
