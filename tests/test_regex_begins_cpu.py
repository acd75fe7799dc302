"""CPU suite of the begins search, the ends pass and leftmost-longest matching: the three oracles of
regex_begins_oracle.py against each other, the selection rule on the start-sorted list against the sequential POSIX
definition, the counter-example that motivates the begins search, bmx_regex_reverse against the oracle's reversal, and every
argument error of the new C entries with ctx = NULL.  No GPU is touched."""
import ctypes as C

import numpy as np
import pytest

import classes_oracle as co
import regex_begins_oracle as bo
import regex_oracle as ro
import subst_oracle as so
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host
import parallel_implementation_of_string_matching_algorithms_opencl_amd as pkg

PAIRS = 300


def _pairs():
    """300 (text, expression, automaton): alphabets of 2 and 4 symbols, texts of up to 40 bytes."""
    rng = np.random.default_rng(0xBE6145)
    for case in range(PAIRS):
        symbols = np.arange(97, 97 + (2 if case % 2 else 4))
        text = rng.choice(symbols, int(rng.integers(0, 41))).astype(np.uint8).tobytes()
        expr, rx = ro.random_regex(rng, symbols, 10)
        yield text, expr, rx


@pytest.fixture(scope="module")
def pairs():
    return [(t, e, rx, bo.begins_brute(t, e)) for t, e, rx in _pairs()]


def test_the_three_oracles_agree(pairs):
    seen = 0
    for text, expr, rx, (starts, short, long_) in pairs:
        s_np, short_np, long_np = bo.begins_numpy(text, rx)
        assert s_np.tolist() == starts and short_np.tolist() == short and long_np.tolist() == long_, (text, expr)
        by_start = dict(zip(starts, long_))
        for s, e in bo.posix_matches(text, expr):  # the sequential definition takes its matches from that list
            assert by_start[s] == e, (text, expr)
        seen += len(starts)
    assert seen > 1000


def test_disjoint_selection_on_the_start_sorted_list_is_leftmost_longest(pairs):
    differs = 0
    for text, expr, rx, (starts, short, long_) in pairs:
        spans = so.spans_of(starts=np.array(starts, np.uint64), ends=np.array(long_, np.uint64))
        assert so.ordered(spans), (text, expr)  # s[i] <= s[j] <= e[j] for i < j
        s, e, _ = so.select(spans)
        want = bo.posix_matches(text, expr)
        assert list(zip(s.tolist(), e.tolist())) == want, (text, expr)
        s2, e2, _ = so.select_pm(spans)
        assert np.array_equal(s, s2) and np.array_equal(e, e2)
        # what the lists of one start per end select instead (leftmost-shortest)
        st, en = so.all_matches(ro.to_re(expr).pattern, text)
        s3, e3, _ = so.select(so.spans_of(starts=st, ends=en))
        differs += list(zip(s3.tolist(), e3.tolist())) != want
    assert differs > 10  # the new route is not the old one under another name


def test_per_row_limit_in_the_sequential_definition():
    text = b"a1\nxb a1b\nab\n"
    assert bo.posix_matches(text, "a.{0,3}b") == [(0, 4), (6, 8), (10, 11)]
    assert bo.posix_matches(text, "a.{0,3}b", bo.row_end(text)) == [(6, 8), (10, 11)]
    text = b"axb\nb"
    assert bo.posix_matches(text, "a.{0,3}b") == [(0, 4)]
    assert bo.posix_matches(text, "a.{0,3}b", bo.row_end(text)) == [(0, 2)]
    assert bo.posix_replace(text, "a.{0,3}b", b"<>", bo.row_end(text)) == b"<>\nb"


def test_one_start_per_end_cannot_answer():
    """ab|b: end 1 of "ab" has the starts {0, 1}; each flag of the starts pass keeps one, only their union has both.  On
    "cab" the LONGEST list lacks start 2 and the default list lacks start 1."""
    pat = ro.to_re("ab|b").pattern
    short, ends = so.all_matches(pat, b"ab")
    long_, ends2 = so.all_matches(pat, b"ab", longest=True)
    assert ends.tolist() == ends2.tolist() == [1] and short.tolist() == [1] and long_.tolist() == [0]
    assert sorted(set(short.tolist()) | set(long_.tolist())) == bo.begins_brute(b"ab", "ab|b")[0] == [0, 1]
    short, _ = so.all_matches(pat, b"cab")
    long_, _ = so.all_matches(pat, b"cab", longest=True)
    assert 2 not in long_.tolist() and 1 not in short.tolist()
    assert bo.begins_brute(b"cab", "ab|b") == ([1, 2], [2, 2], [2, 2])
    assert bo.posix_matches(b"cab", "ab|b") == [(1, 2)]
    assert bo.posix_matches(b"abcd", "(a|ab)(c|bcd)") == [(0, 3)]


def _same(got: host.Regex, want: ro.Rx, what):
    assert got.m == want.m, what
    assert np.array_equal(co.unpack(got.class_array()), want.member), what
    assert got.first == want.first and got.last == want.last, what
    assert list(got.follow)[: want.m] == want.follow and not any(list(got.follow)[want.m:]), what


def test_reverse_equals_the_oracle(built):
    rng = np.random.default_rng(0x7E5E)
    cases = [ro.random_regex(rng, np.arange(97, 101), 16) for _ in range(200)]
    cases.append(("(a|b)x{59}(c|dd)", ro.parse("(a|b)x{59}(c|dd)")))  # 64 positions
    assert cases[-1][1].m == 64
    for expr, rx in cases:
        r = host.compile_regex(expr)
        rev = host.reverse_regex(r)
        _same(rev, ro.reverse(rx), expr)
        assert (rev.min_len, rev.max_len) == (r.min_len, r.max_len) == (rx.min_len, rx.max_len), expr
        assert bytes(host.reverse_regex(rev)) == bytes(r), expr  # twice: the input
        assert bytes(pkg.reverse_regex(expr)) == bytes(rev)
        again = host.Regex()
        C.memmove(C.byref(again), C.byref(r), C.sizeof(r))
        assert host.lib().bmx_regex_reverse(C.byref(again), C.byref(again)) == host.OK and bytes(again) == bytes(rev)  # in place
    rv = host.lib().bmx_regex_reverse
    out = host.Regex()
    assert rv(None, C.byref(out)) == host.ERR_ARG and rv(C.byref(host.compile_regex("ab")), None) == host.ERR_ARG
    star = host.compile_regex_star("a(bc)+d")  # the starts pass of the star search reverses automata with a cycle
    assert rv(C.byref(star), C.byref(out)) == host.OK and bytes(host.reverse_regex(out)) == bytes(star)


def _broken():
    """(what, automaton) that the begins search and the ends pass must refuse."""
    def edit(**kw):
        r = host.compile_regex("(a|bc)d")
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    return [("cyclic", host.compile_regex_star("a(bc)+d")), ("m = 0", edit(m=0)), ("m = 65", edit(m=65)),
            ("first empty", edit(first=0)), ("last beyond m", edit(last=1 << 63))]


def test_every_argument_error_before_any_device_call(built):
    L = host.lib()
    text = b"some text to search in"
    n = len(text)
    out = (C.c_uint64 * 8)()
    total = C.c_uint64(0)
    t = C.byref(total)
    r = host.compile_regex("(a|bc)d")
    p = C.byref(r)
    dev, ends = L.bmx_search_regex_begins_device, L.bmx_regex_ends_device
    hb, hs = L.bmx_search_regex_begins, L.bmx_search_regex_begins_spans
    for what, bad in _broken():
        b = C.byref(bad)
        assert dev(None, None, 10, 0, 0, b, None, 0, t, None) == host.ERR_ARG, what
        assert ends(None, None, 10, 0, b, out, 0, None, 0, out, None) == host.ERR_ARG, what  # even with count == 0
        assert hb(None, text, n, b, out, 8, t) == host.ERR_ARG, what
        assert hs(None, text, n, b, 0, out, out, 8, t) == host.ERR_ARG, what
    assert dev(None, None, 10, 0, 0, None, None, 0, t, None) == host.ERR_ARG  # no automaton
    assert dev(None, None, 10, 11, 0, p, None, 0, t, None) == host.ERR_ARG  # tail > n
    assert dev(None, None, 1 << 40, 0, 0, p, None, 0, t, None) == host.ERR_ARG
    assert dev(None, None, 10, 0, 0, p, None, 8, t, None) == host.ERR_ARG  # capacity, no starts
    assert dev(None, None, 10, 0, 0, p, None, 0, t, None) == host.ERR_ARG  # no context
    assert dev(None, None, 10, 10, 0, p, None, 0, t, None) == host.ERR_ARG  # ... even where tail == n owns nothing
    assert ends(None, None, 10, 0, None, out, 8, None, 0, out, None) == host.ERR_ARG
    assert ends(None, None, 10, 0, p, out, 8, None, 2, out, None) == host.ERR_ARG  # an unknown flag bit
    assert ends(None, None, 1 << 40, 0, p, out, 8, None, 0, out, None) == host.ERR_ARG
    assert ends(None, None, 10, 0, p, None, 8, None, 0, out, None) == host.ERR_ARG
    assert ends(None, None, 10, 0, p, out, 8, None, 0, None, None) == host.ERR_ARG
    assert ends(None, None, 10, 0, p, out, 8, out, host.REGEX_LONGEST, out, None) == host.ERR_ARG  # no context
    assert ends(None, None, 10, 0, p, None, 0, None, 0, None, None) == host.OK  # count == 0: nothing to do
    assert hb(None, text, n, None, out, 8, t) == host.ERR_ARG
    assert hb(None, text, n, p, None, 8, t) == host.ERR_ARG  # a capacity needs room
    assert hb(None, None, n, p, out, 8, t) == host.ERR_ARG
    assert hb(None, text, 1 << 40, p, out, 8, t) == host.ERR_ARG
    assert hb(None, text, 0, p, out, 8, t) == host.OK and total.value == 0  # an empty text: no device needed
    assert hs(None, text, n, None, 0, out, out, 8, t) == host.ERR_ARG
    assert hs(None, text, n, p, 0, None, out, 8, t) == host.ERR_ARG
    assert hs(None, text, n, p, 0, out, None, 8, t) == host.ERR_ARG
    assert hs(None, None, n, p, 0, out, out, 8, t) == host.ERR_ARG
    assert hs(None, text, n, p, 2, out, out, 8, t) == host.ERR_ARG  # an unknown flag bit
    assert hs(None, text, 1 << 40, p, 0, out, out, 8, t) == host.ERR_ARG
    assert L.bmx_last_regex_begins_ms(None) < 0


def test_posix_goes_with_the_regex_kind_only():
    for kw in (dict(kind="gaps"), dict(merge=True), dict(longest=True), dict(longest=False)):
        with pytest.raises(ValueError):
            host.sub(b"abc", "b", b"x", posix=True, **kw)
        with pytest.raises(ValueError):
            host.findall(b"abc", "b", posix=True, **kw)
        with pytest.raises(ValueError):  # the shared route refuses before it touches its context
            host.Context._selected_spans_device(None, None, "b", kw.get("kind", "regex"), None, kw.get("merge", False),
                                                kw.get("longest"), 0, 0, None, posix=True)


def test_exports(built):
    L, X = C.CDLL(host.LIB_PATH), C.CDLL(host.EXP_LIB_PATH)
    for name in ("bmx_regex_reverse", "bmx_search_regex_begins_device", "bmx_last_regex_begins_ms", "bmx_regex_ends_device",
                 "bmx_search_regex_begins", "bmx_search_regex_begins_spans"):
        assert hasattr(L, name) and hasattr(X, name), name
        assert name in [s for s, _, _ in host.SYMBOLS]
    for name in ("reverse_regex", "search_regex_begins"):
        assert getattr(pkg, name) is getattr(host, name)
    for name in ("search_regex_begins_device", "regex_ends_device", "search_regex_begins", "search_regex_begins_spans",
                 "last_regex_begins_ms"):
        assert callable(getattr(host.Context, name))
