"""CPU suite for the regular-expression search with unbounded repetition (bmx_compile_regex_star, bmx_search_regex_star*,
bmx_regex_star_starts_device): the oracle against a brute force over Python's ``re``, the expression compiler against the
oracle on a fixed table, on random expressions and on random byte strings, byte-identity with bmx_compile_regex on
star-free input, every compiler error with *out untouched, the validation of a caller's automaton and the argument errors
that return before any HIP call, the slow path's identity (pair bounds, columns and sweep reproduce the true states) on
Python ints, and the new C-ABI symbols and constants.  No compute call is made on a device here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import classes_oracle as co
import regex_oracle as ro
import regex_star_oracle as so
import test_regex_cpu as base
from conftest import ROOT
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host
import parallel_implementation_of_string_matching_algorithms_opencl_amd as pkg

ICASE, IUPAC = host.CLASS_ICASE, host.CLASS_IUPAC
U = host.REGEX_UNBOUNDED
WHY = ["ERROR.*timeout", r"[0-9]+\.[0-9]+", "ATG([ACGT]{3})+(TAA|TAG|TGA)", r"[A-Za-z_][A-Za-z0-9_]*\("]

# (expression, flags, m, first, last, follow as {position: successors}, min_len, max_len)
TABLE = [
    ("a+", 0, 1, [0], [0], {0: [0]}, 1, U),
    ("a*b", 0, 2, [0, 1], [1], {0: [0, 1]}, 1, U),
    ("ab*", 0, 2, [0], [0, 1], {0: [1], 1: [1]}, 1, U),
    ("a{2,}", 0, 2, [0], [1], {0: [1], 1: [1]}, 2, U),
    ("a{1,}", 0, 1, [0], [0], {0: [0]}, 1, U),
    ("a{0,}b", 0, 2, [0, 1], [1], {0: [0, 1]}, 1, U),
    ("a{3,}", 0, 3, [0], [2], {0: [1], 1: [2], 2: [2]}, 3, U),
    ("(ab)+", 0, 2, [0], [1], {0: [1], 1: [0]}, 2, U),
    ("(ab)*c", 0, 3, [0, 2], [2], {0: [1], 1: [0, 2]}, 1, U),
    ("(ab){2,}", 0, 4, [0], [3], {0: [1], 1: [2], 2: [3], 3: [2]}, 4, U),
    ("(a|b)+c", 0, 3, [0, 1], [2], {0: [0, 1, 2], 1: [0, 1, 2]}, 2, U),
    ("((ab)+c)*d", 0, 4, [0, 3], [3], {0: [1], 1: [0, 2], 2: [0, 3]}, 1, U),
    ("(a?b)+", 0, 2, [0, 1], [1], {0: [1], 1: [0, 1]}, 1, U),
    ("(a*b)+", 0, 2, [0, 1], [1], {0: [0, 1], 1: [0, 1]}, 1, U),
    ("a(b+|c)d", 0, 4, [0], [3], {0: [1, 2], 1: [1, 3], 2: [3]}, 3, U),
    ("(a+)?b", 0, 2, [0, 1], [1], {0: [0, 1]}, 1, U),
    ("()a+(){3}", 0, 1, [0], [0], {0: [0]}, 1, U),
    (r"\*\+a+", 0, 3, [0], [2], {0: [1], 1: [2], 2: [2]}, 3, U),
    ("[*+]+", 0, 1, [0], [0], {0: [0]}, 1, U),
    ("aB+", ICASE, 2, [0], [1], {0: [1], 1: [1]}, 2, U),
    ("AN+T", IUPAC, 3, [0], [2], {0: [1], 1: [1, 2]}, 3, U),
    ("x{63}y+", 0, 64, [0], [63], dict([(i, [i + 1]) for i in range(63)] + [(63, [63])]), 64, U),
    ("(x{32})+", 0, 32, [0], [31], dict([(i, [i + 1]) for i in range(31)] + [(31, [0])]), 32, U),
    ("abc", 0, 3, [0], [2], {0: [1], 1: [2]}, 3, 3),  # no cycle: a longest match
    ("(ab){2,3}", 0, 6, [0], [3, 5], {0: [1], 1: [2], 2: [3], 3: [4], 4: [5]}, 4, 6),
]
ERRORS = [
    ("", 0), ("a*", 0), ("(ab)*", 0), ("a*b*", 0), ("(a+)?", 0), ("a{0,}", 0), ("(a|b*)", 0), ("*", 0), ("+", 0), ("*a", 0), ("+a", 0),
    ("a|*b", 0), ("(*a)", 0), ("a**", 0), ("a++", 0), ("a+*", 0), ("a*+", 0), ("a+?", 0), ("a*?", 0), ("a?+", 0), ("a?*", 0),
    ("a{2,}?", 0), ("a{2,}+", 0), ("a+{2}", 0), ("a{2}*", 0), ("a{,}", 0), ("a{2,", 0), ("a{2,}{3}", 0), ("(", 0), (")", 0), ("(a", 0),
    ("a)", 0), ("(a+", 0), ("a+)", 0), ("?a", 0), ("{2}a", 0), ("(?:a)", 0), ("a??", 0), ("a{0}", 0), ("a{3,2}", 0), ("a{", 0), ("a{}", 0),
    ("(" * 33 + "a+" + ")" * 33, 0), ("a{65,}", 0), ("a{64}b+", 0), ("(ab){33,}", 0), ("x" * 64 + "+y", 0), ("a{99999999999999999999,}", 0),
    ("()", 0), ("()+", 0), ("(|)*", 0), ("a?", 0), ("[abc+", 0), ("[c-a]+", 0), ("a+\\", 0), (r"\x4+", 0), ("a+", 4), ("a+", 8),
    ("a+", 1 << 31),
]


def _bits(positions):
    return sum(1 << i for i in positions)


def _compile_raw(expr, flags, entry="bmx_compile_regex_star"):
    """(rc, struct, untouched?) through the C ABI, with a sentinel pattern in *out."""
    e = expr.encode("latin-1") if isinstance(expr, str) else bytes(expr)
    out = host.Regex()
    C.memset(C.byref(out), 0xA5, C.sizeof(out))
    rc = getattr(host.lib(), entry)(e, len(e), flags, C.byref(out))
    return rc, out, bytes(out) == b"\xa5" * C.sizeof(out)


def _same(got: host.Regex, want, what):
    assert got.m == want.m, what
    assert np.array_equal(co.unpack(got.class_array()), want.member), what
    assert got.first == want.first and got.last == want.last, what
    assert list(got.follow)[: want.m] == want.follow and not any(list(got.follow)[want.m:]), what
    assert (got.min_len, got.max_len) == (want.min_len, want.max_len), what


def _tiny_case(rng, case):
    alpha = 2 + case % 2
    symbols = np.arange(97, 97 + alpha)
    text = rng.choice(symbols, int(rng.integers(0, 14))).astype(np.uint8).tobytes()  # (re backtracks: nested loops on longer texts take minutes)
    expr, rx = so.random_regex(rng, symbols, 6)
    return text, expr, rx


def test_oracle_equals_the_brute_force_on_tiny_cases():
    rng = np.random.default_rng(0x57A2)
    non_empty = cyclic = sentinels = 0
    for case in range(450):
        text, expr, rx = _tiny_case(rng, case)
        ends, short, long_ = so.ends_brute(text, expr)
        assert ro.match_ends(text, rx) == (ends, short, long_), (case, expr, text)
        assert so.ends_numpy(text, rx).tolist() == ends, (case, expr, text)
        for window in (1, 2, 5, 64):
            e_w, s_w, l_w = so.ends_brute(text, expr, window=window)
            want_s = [s_w[e_w.index(j)] if j in e_w else so.NO_START for j in ends]
            want_l = [l_w[e_w.index(j)] if j in e_w else so.NO_START for j in ends]
            assert so.starts_numpy(text, rx, ends, window).tolist() == want_s, (case, expr, text, window)
            assert so.starts_numpy(text, rx, ends, window, longest=True).tolist() == want_l, (case, expr, text, window)
            sentinels += so.NO_START in want_s
        assert 1 <= rx.min_len and (rx.max_len == so.UNBOUNDED or rx.min_len <= rx.max_len <= rx.m), expr
        if ends:
            assert min(j - s + 1 for j, s in zip(ends, short)) >= rx.min_len
            if rx.max_len != so.UNBOUNDED:
                assert max(j - s + 1 for j, s in zip(ends, long_)) <= rx.max_len
        non_empty += bool(ends)
        cyclic += rx.max_len == so.UNBOUNDED
    assert 3 * non_empty > 450, non_empty
    assert cyclic >= 200 and sentinels >= 50, (cyclic, sentinels)


def test_oracle_is_regex_oracle_where_there_is_no_cycle():
    rng = np.random.default_rng(0x57A3)
    symbols = np.arange(97, 100)
    for case in range(200):
        expr, rx = ro.random_regex(rng, symbols, 12)
        sx = so.parse(expr)
        assert (sx.m, sx.first, sx.last, sx.follow, sx.min_len, sx.max_len) == (rx.m, rx.first, rx.last, rx.follow, rx.min_len, rx.max_len)
        text = rng.choice(symbols, int(rng.integers(0, 80))).astype(np.uint8).tobytes()
        assert np.array_equal(so.ends_numpy(text, sx), ro.ends_numpy(text, rx)), expr


def test_expression_table(built):
    for expr, flags, m, first, last, follow, min_len, max_len in TABLE:
        got = host.compile_regex_star(expr, flags)
        what = (expr, flags)
        assert got.m == m and got.first == _bits(first) and got.last == _bits(last), what
        assert [got.follow[i] for i in range(m)] == [_bits(follow.get(i, [])) for i in range(m)], what
        assert (got.min_len, got.max_len) == (min_len, max_len), what
        _same(got, so.parse(expr, flags), what)
    for expr in WHY:
        for flags in (0, ICASE, IUPAC, ICASE | IUPAC):
            _same(host.compile_regex_star(expr, flags), so.parse(expr, flags), (expr, flags))
    assert [host.compile_regex_star(e).m for e in WHY] == [13, 3, 15, 3]
    assert [(r.min_len, r.max_len) for r in map(host.compile_regex_star, WHY)] == [(12, U), (3, U), (9, U), (2, U)]
    # a self-loop on position 31 / 32 and a back edge across the word halves
    r = host.compile_regex_star("x{31}y+z")
    assert r.follow[31] == 1 << 31 | 1 << 32
    r = host.compile_regex_star("x{32}y+z")
    assert r.follow[32] == 1 << 32 | 1 << 33
    r = host.compile_regex_star("x{30}(abcd)+z")
    assert r.follow[33] == 1 << 30 | 1 << 34


def test_compiler_equals_the_oracle_on_random_expressions(built):
    rng = np.random.default_rng(0x57A4)
    cyclic = 0
    for case in range(400):
        symbols = np.arange(97, 97 + 2 + case % 3)
        expr, rx = so.random_regex(rng, symbols, (8, 32, 64)[case % 3])
        _same(host.compile_regex_star(expr), rx, expr)
        cyclic += rx.max_len == U
    assert cyclic >= 150, cyclic
    # random byte strings over the grammar's own alphabet: the same verdict, and the same automaton where there is one
    alphabet = np.frombuffer(b"ab]^-[\\.xN?{},0123*+()|\xe9", np.uint8)
    agreed = starred = 0
    for case in range(3000):
        e = alphabet[rng.integers(0, alphabet.size, int(rng.integers(0, 14)))].tobytes()
        flags = case % 4
        rc, out, untouched = _compile_raw(e, flags)
        try:
            rx = so.parse(e, flags)
        except so.ExprError:
            assert rc == host.ERR_ARG and untouched, (e, flags)
            continue
        assert rc == host.OK, (e, flags)
        _same(out, rx, (e, flags))
        agreed += 1
        starred += rx.max_len == U
    assert agreed > 300 and starred > 30, (agreed, starred)


def test_star_free_input_compiles_byte_for_byte_as_before(built):
    rng = np.random.default_rng(0x57A5)
    exprs = [(e, f) for e, f, *_ in base.TABLE] + [(e, f) for e in base.WHY for f in (0, ICASE, IUPAC)]
    exprs += [(ro.random_regex(rng, np.arange(97, 100), (8, 32, 64)[i % 3])[0], 0) for i in range(200)]
    for expr, flags in exprs:
        a = host.compile_regex(expr, flags)
        b = host.compile_regex_star(expr, flags)
        assert bytes(a) == bytes(b), (expr, flags)
    # and what the star-free compiler refuses apart from * + {a,} the other one refuses too
    for expr, flags in base.ERRORS:
        if not re.search(r"[*+]|,\}", expr):
            assert _compile_raw(expr, flags)[0] == host.ERR_ARG, (expr, flags)


def test_expression_errors(built):
    L = host.lib()
    for expr, flags in ERRORS:
        rc, out, untouched = _compile_raw(expr, flags)
        assert rc == host.ERR_ARG and untouched, (expr, flags)
        assert L.bmx_last_error().startswith(b"bmx_compile_regex_star: "), (expr, flags)
        with pytest.raises(so.ExprError):
            so.parse(expr, flags)
    for expr in ("a*", "(ab)*", "(a+)?"):
        _compile_raw(expr, 0)
        assert b"matches the empty string" in L.bmx_last_error(), expr
    assert host.compile_regex_star("(" * 32 + "a+" + ")" * 32).m == 1  # 32 levels are fine
    assert host.compile_regex_star("a{64,}").m == 64
    out = host.Regex()
    assert L.bmx_compile_regex_star(None, 0, 0, C.byref(out)) == host.ERR_ARG
    assert L.bmx_compile_regex_star(b"a", 1, 0, None) == host.ERR_ARG
    with pytest.raises(host.BmxError) as e:
        host.compile_regex_star("a**")
    assert e.value.rc == host.ERR_ARG
    # the star-free entry is what it was
    for expr in ("a*", "a+", "a{2,}"):
        assert _compile_raw(expr, 0, "bmx_compile_regex")[0] == host.ERR_ARG
        assert L.bmx_last_error().startswith(b"bmx_compile_regex: ") and b"out of scope" in L.bmx_last_error()


def _broken():
    """(what, automaton) for every validation rule of the entries that take a cycle."""
    def edit(f, expr="(a|bc)+d"):
        r = host.compile_regex_star(expr)
        f(r)
        return r

    def set_(name, value):
        return lambda r: setattr(r, name, value)

    def follow(i, value):
        def f(r):
            r.follow[i] = value
        return f

    return [("m == 0", edit(set_("m", 0))), ("m < 0", edit(set_("m", -1))), ("m > 64", edit(set_("m", 65))),
            ("first == 0", edit(set_("first", 0))), ("last == 0", edit(set_("last", 0))),
            ("first beyond m", edit(set_("first", 1 | 1 << 4))), ("last beyond m", edit(set_("last", 1 << 63))),
            ("follow beyond m", edit(follow(2, 1 << 3 | 1 << 4))), ("follow[0] beyond m", edit(follow(0, 1 << 63)))]


def test_automaton_validation_before_any_device_call(built):
    L = host.lib()
    text = b"some text to search in"
    out = (C.c_uint64 * 8)()
    total = C.c_uint64(0)
    for what, r in _broken():
        p = C.byref(r)
        assert L.bmx_search_regex_star(None, text, len(text), p, out, 8, C.byref(total)) == host.ERR_ARG, what
        assert L.bmx_search_regex_star_spans(None, text, len(text), p, 64, 0, out, out, 8, C.byref(total)) == host.ERR_ARG, what
        assert L.bmx_search_regex_star_device(None, None, 10, 0, 0, p, None, 0, C.byref(total), None) == host.ERR_ARG, what
        assert L.bmx_regex_star_starts_device(None, None, 10, 0, p, out, 0, 64, 0, out, None) == host.ERR_ARG, what
    # a cycle passes the new entries and not the old ones: self-loops, back edges, follow[63] to anything
    for expr in ("a+", "(ab)+c", "((ab)+c)*d", "x{63}y+"):
        r = host.compile_regex_star(expr)
        p = C.byref(r)
        assert L.bmx_regex_star_starts_device(None, None, 10, 0, p, None, 0, 64, 0, None, None) == host.OK, expr
        assert L.bmx_search_regex_star(None, text, 0, p, out, 8, C.byref(total)) == host.OK and total.value == 0, expr
        assert L.bmx_regex_starts_device(None, None, 10, 0, p, None, 0, 0, None, None) == host.ERR_ARG, expr
        assert L.bmx_search_regex(None, text, 0, p, out, 8, C.byref(total)) == host.ERR_ARG, expr
    # legal oddities: an empty class, positions that no match can use, min_len / max_len fields that say nothing
    r = host.compile_regex_star("(a|bc)+d")
    C.memset(r.classes, 0, 32)
    r.follow[0] = 1
    r.min_len = r.max_len = -5
    assert L.bmx_regex_star_starts_device(None, None, 10, 0, C.byref(r), None, 0, 1, 0, None, None) == host.OK
    assert L.bmx_search_regex_star(None, text, 0, C.byref(r), out, 8, C.byref(total)) == host.OK and total.value == 0


def test_argument_errors_before_any_device_call(built):
    L = host.lib()
    text = b"some text to search in"
    out = (C.c_uint64 * 8)()
    total = C.c_uint64(0)
    r = host.compile_regex_star("(a|bc)+d")
    p = C.byref(r)
    s = L.bmx_search_regex_star
    assert s(None, text, len(text), None, out, 8, C.byref(total)) == host.ERR_ARG
    assert s(None, text, len(text), p, None, 8, C.byref(total)) == host.ERR_ARG  # a capacity needs room
    assert s(None, None, len(text), p, out, 8, C.byref(total)) == host.ERR_ARG
    assert s(None, text, 1 << 40, p, out, 8, C.byref(total)) == host.ERR_ARG
    sp = L.bmx_search_regex_star_spans
    assert sp(None, text, len(text), None, 64, 0, out, out, 8, C.byref(total)) == host.ERR_ARG
    assert sp(None, text, len(text), p, 64, 0, None, out, 8, C.byref(total)) == host.ERR_ARG
    assert sp(None, text, len(text), p, 64, 0, out, None, 8, C.byref(total)) == host.ERR_ARG
    assert sp(None, None, len(text), p, 64, 0, out, out, 8, C.byref(total)) == host.ERR_ARG
    assert sp(None, text, len(text), p, 64, 2, out, out, 8, C.byref(total)) == host.ERR_ARG  # an unknown flag bit
    assert sp(None, text, len(text), p, 0, 0, out, out, 8, C.byref(total)) == host.ERR_ARG  # window
    assert sp(None, text, len(text), p, 65537, 0, out, out, 8, C.byref(total)) == host.ERR_ARG
    assert sp(None, text, 1 << 40, p, 64, 0, out, out, 8, C.byref(total)) == host.ERR_ARG
    dev = L.bmx_search_regex_star_device
    assert dev(None, None, 10, 0, 0, None, None, 0, C.byref(total), None) == host.ERR_ARG
    assert dev(None, None, 10, 11, 0, p, None, 0, C.byref(total), None) == host.ERR_ARG  # lead > n
    assert dev(None, None, 1 << 40, 0, 0, p, None, 0, C.byref(total), None) == host.ERR_ARG
    assert dev(None, None, 10, 0, 0, p, None, 8, C.byref(total), None) == host.ERR_ARG  # capacity, no ends
    assert dev(None, None, 10, 0, 0, p, None, 0, C.byref(total), None) == host.ERR_ARG  # no context
    st = L.bmx_regex_star_starts_device
    assert st(None, None, 10, 0, None, out, 8, 64, 0, out, None) == host.ERR_ARG
    assert st(None, None, 10, 0, p, out, 8, 64, 2, out, None) == host.ERR_ARG  # an unknown flag bit
    assert st(None, None, 10, 0, p, out, 8, 0, 0, out, None) == host.ERR_ARG  # window
    assert st(None, None, 10, 0, p, out, 8, 65537, 0, out, None) == host.ERR_ARG
    assert st(None, None, 1 << 40, 0, p, out, 8, 64, 0, out, None) == host.ERR_ARG
    assert st(None, None, 10, 0, p, None, 8, 64, 0, out, None) == host.ERR_ARG
    assert st(None, None, 10, 0, p, out, 8, 64, 0, None, None) == host.ERR_ARG
    assert st(None, None, 10, 0, p, out, 8, 65536, host.REGEX_LONGEST, out, None) == host.ERR_ARG  # no context
    assert st(None, None, 10, 0, p, None, 0, 65536, 0, None, None) == host.OK  # count == 0: nothing to do
    assert L.bmx_last_regex_star_ms(None) < 0


def test_slow_path_identity_on_python_ints():
    """Pair bounds, columns and sweep give the true state in front of every piece; the bounds bracket it; and the state
    behind a stretch entered with X is c | OR of the columns of X."""
    rng = np.random.default_rng(0x57A6)
    unsure = chained = 0
    for case in range(240):
        symbols = np.arange(97, 97 + 2 + case % 2)
        expr, rx = so.random_regex(rng, symbols, (8, 16, 40)[case % 3], cyclic=True)
        text = rng.choice(symbols, int(rng.integers(0, 201))).astype(np.uint8).tobytes()
        truth = [0] + so.states(text, rx)
        # linearity on a random stretch and a random entry set
        a = int(rng.integers(0, len(text) + 1))
        b = int(rng.integers(a, len(text) + 1))
        X = int(rng.integers(0, 1 << rx.m))
        c = so.run(text[a:b], rx, 0, True)
        cols = 0
        for u in so.bits(X):
            cols |= so.run(text[a:b], rx, 1 << u, False)
        assert so.run(text[a:b], rx, X, True) == c | cols, (expr, text, a, b, X)
        for piece in (1, 3, 16):
            e, u = so.pair_bounds(text, rx, piece)
            for l in range(len(e)):
                t = truth[l * piece]
                assert e[l] & ~t == 0 and t & ~(e[l] | u[l]) == 0, (expr, text, piece, l)
            base_, cols_ = so.columns(text, rx, piece, e, u)
            entry = so.sweep(e, u, base_, cols_)
            assert entry == [truth[l * piece] for l in range(len(e))], (expr, text, piece)
            unsure += sum(1 for x in u if x)
            chained += sum(1 for l in range(1, len(u)) if u[l] and u[l - 1])
    assert unsure > 1000 and chained > 500, (unsure, chained)


def test_slow_path_identity_with_a_lead_and_an_unaligned_view():
    """The same identity in the kernels' aligned coordinates: the view begins ``first`` = 0..15 bytes into piece 0 (those
    bytes leave the empty state), the bounds, columns and sweep run from aligned piece 0 whatever ``lead`` is, and the
    walk from the swept states reports the true ends from ``lead`` on -- its first lane entering in the middle of a
    piece."""
    rng = np.random.default_rng(0x57A7)
    unsure = inside = 0
    for case in range(240):
        symbols = np.arange(97, 97 + 2 + case % 2)
        expr, rx = so.random_regex(rng, symbols, (8, 16, 40)[case % 3], cyclic=True)
        n = int(rng.integers(1, 1500 if case % 8 == 0 else 300))
        text = rng.choice(symbols, n).astype(np.uint8).tobytes()
        first, ps = case % 16, (0, 2, 4)[case // 16 % 3]
        truth = [0] + so.states(text, rx)
        k = so.masked(rx)
        e, u = so.pair_bounds(text, k, 1 << ps, first)
        base_, cols_ = so.columns(text, k, 1 << ps, e, u, first)
        entry = so.sweep(e, u, base_, cols_)
        assert len(e) == ((n + first - 1) >> ps) + 1
        assert entry == [truth[max((l << ps) - first, 0)] & k.all for l in range(len(e))], (expr, text, first, ps)
        unsure += sum(1 for x in u if x)
        want = so.ends_numpy(text, rx)
        for lead in sorted({0, 1, n - 1, n, int(rng.integers(0, n + 1)), min(n, max(0, (1 << ps) * int(rng.integers(0, 9)) - first))}):
            got = so.slow_ends(text, rx, first, lead, ps)
            assert np.array_equal(got, want[want >= lead]), (expr, text, first, ps, lead)
            inside += (lead + first) % (1 << ps) != 0
    assert unsure > 1000 and inside > 300, (unsure, inside)


def test_fast_taint_model_reports_a_lower_bound_and_the_truth_when_untainted():
    """so.fast_taint on random expressions and small geometries: the list of the first launch is a subset of the true
    list, and the true list where no lane is tainted; tainted or not, the slow path's model gives the true list."""
    rng = np.random.default_rng(0x57A8)
    tainted = clean = short = 0
    for case in range(300):
        symbols = np.arange(97, 97 + 2 + case % 3)
        expr, rx = so.random_regex(rng, symbols, (8, 16, 40)[case % 3], cyclic=None if case % 5 else False)
        ps = (4, 5, 6)[case % 3]
        n = int(rng.integers(1, (600 << ps) // 4))
        text = rng.choice(symbols, n).astype(np.uint8)
        for _ in range(4):
            so.plant_path(rng, text, rx, int(rng.integers(0, n)), stop=0.1)
        text = text.tobytes()
        first, lead, warm = case % 16, (0, int(rng.integers(0, n + 1)))[case % 2], (0, 16, 32, 64, 4096)[case % 5]
        want = so.ends_numpy(text, rx)
        want = want[want >= lead]
        m = so.fast_taint(text, rx, first, lead, ps, warm)
        assert np.all(np.diff(m.ends) > 0) and np.isin(m.ends, want).all(), (expr, first, lead, ps, warm)
        assert (m.waves == 0) == (not m.lanes) and m.waves <= len(m.lanes)
        assert m.waves == len({(t, l >> 6) for t, l in m.lanes})
        if not m.lanes:
            assert np.array_equal(m.ends, want), (expr, first, lead, ps, warm)
            clean += 1
        else:
            tainted += 1
            short += m.ends.size < want.size
        if (n + first - 1) & ~15 <= warm:  # every warm-up begins at view byte 0: exact by rule
            assert not m.lanes
        if case % 3 == 0:
            assert np.array_equal(so.slow_ends(text, rx, first, lead, ps), want), (expr, first, lead, ps)
    assert tainted >= 60 and clean >= 60 and short >= 10, (tainted, clean, short)


def test_library_exports_regex_star_symbols(built):
    L = C.CDLL(host.LIB_PATH)
    X = C.CDLL(host.EXP_LIB_PATH)
    for name in ("bmx_compile_regex_star", "bmx_search_regex_star_device", "bmx_search_regex_star", "bmx_search_regex_star_spans",
                 "bmx_last_regex_star_ms", "bmx_regex_star_starts_device"):
        assert hasattr(L, name) and hasattr(X, name), name
        assert name in [s for s, _, _ in host.SYMBOLS]
    assert hasattr(X, "bmx_exp_regex_star_last") and not hasattr(L, "bmx_exp_regex_star_last")
    for name in ("compile_regex_star", "search_regex_star", "REGEX_UNBOUNDED", "MAX_REGEX_STAR_WINDOW"):
        assert getattr(pkg, name) is getattr(host, name)
    for name in ("search_regex_star_device", "search_regex_star", "search_regex_star_spans", "regex_star_starts_device",
                 "last_regex_star_ms"):
        assert callable(getattr(host.Context, name))


def test_header_constants():
    src = open(os.path.join(ROOT, "include", "bmx.h")).read()
    assert int(re.search(r"#define BMX_REGEX_UNBOUNDED \((-?\d+)\)", src).group(1)) == host.REGEX_UNBOUNDED == so.UNBOUNDED == -1
    assert int(re.search(r"#define BMX_MAX_REGEX_STAR_WINDOW (\d+)u", src).group(1)) == host.MAX_REGEX_STAR_WINDOW == 65536
    assert so.NO_START == np.iinfo(np.uint64).max
