"""CPU suite for the regular-expression search (bmx_compile_regex, bmx_search_regex*, bmx_regex_starts_device): the oracle
against a brute force over Python's ``re`` (its matcher, its numpy answers and the kernel's word-level recurrence at both
widths), the expression compiler against the oracle on a fixed table and on random expressions and against
bmx_compile_gaps where there are no groups, every compiler error with *out untouched, the validation of a caller's
automaton, the new C-ABI symbols and constants, and the argument errors that return before any HIP call.  No compute call
is made on a device here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import classes_oracle as co
import gaps_oracle as go
import regex_oracle as ro
from conftest import ROOT
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host
import parallel_implementation_of_string_matching_algorithms_opencl_amd as pkg

ICASE, IUPAC = host.CLASS_ICASE, host.CLASS_IUPAC
WHY = ["ATG([ACGT]{3}){2,4}(TAA|TAG|TGA)", "(ERROR|FATAL|PANIC): [0-9]{2,4}", r"([0-9]{1,3}\.){3}[0-9]{1,3}", "(RGD|KGD)x{2,5}[ST]"]

# (expression, flags, m, first, last, follow as {position: successors}, min_len, max_len)
TABLE = [
    ("a", 0, 1, [0], [0], {}, 1, 1),
    ("abc", 0, 3, [0], [2], {0: [1], 1: [2]}, 3, 3),
    ("a|b", 0, 2, [0, 1], [0, 1], {}, 1, 1),
    ("(a|)b", 0, 2, [0, 1], [1], {0: [1]}, 1, 2),
    ("(ab){2,3}", 0, 6, [0], [3, 5], {0: [1], 1: [2], 2: [3], 3: [4], 4: [5]}, 4, 6),
    ("(a|bc)d", 0, 4, [0, 1], [3], {0: [3], 1: [2], 2: [3]}, 2, 3),
    ("a(b|c)?d", 0, 4, [0], [3], {0: [1, 2, 3], 1: [3], 2: [3]}, 2, 3),
    ("a{2}b?", 0, 3, [0], [1, 2], {0: [1], 1: [2]}, 2, 3),
    ("(a?b?){2}c", 0, 5, [0, 1, 2, 3, 4], [4], {0: [1, 2, 3, 4], 1: [2, 3, 4], 2: [3, 4], 3: [4]}, 1, 5),
    ("()a(){3}", 0, 1, [0], [0], {}, 1, 1),
    (r"\(\)\|\?\{\*\+", 0, 7, [0], [6], {i: [i + 1] for i in range(6)}, 7, 7),
    (r"[()|?{*+]{2}", 0, 2, [0], [1], {0: [1]}, 2, 2),
    (r"\x41(\.|\\)", 0, 3, [0], [1, 2], {0: [1, 2]}, 2, 2),
    ("aB|c", ICASE, 3, [0, 2], [1, 2], {0: [1]}, 1, 2),
    ("AC(N|R{2})T", IUPAC, 6, [0], [5], {0: [1], 1: [2, 3], 2: [5], 3: [4], 4: [5]}, 4, 5),
    ("(r|Y)n", IUPAC | ICASE, 3, [0, 1], [2], {0: [2], 1: [2]}, 2, 2),
    ("x{64}", 0, 64, [0], [63], {i: [i + 1] for i in range(63)}, 64, 64),
]
ERRORS = [
    ("", 0), ("a*", 0), ("a+", 0), ("*", 0), ("(a)*", 0), ("(a)+", 0), ("a{2,}", 0), ("(ab){1,}", 0), ("(", 0), (")", 0), ("(a", 0),
    ("a)", 0), ("((a)", 0), ("(a))", 0), ("?a", 0), ("{2}a", 0), ("(?:a)", 0), ("(?a)", 0), ("a|?b", 0), ("a??", 0), ("a{2}?", 0),
    ("a?{2}", 0), ("(a)?{2}", 0), ("a{2}{3}", 0), ("a{0}", 0), ("(a){0,0}", 0), ("a{3,2}", 0), ("a{", 0), ("a{2", 0), ("a{2,3", 0),
    ("a{,3}", 0), ("a{}", 0), ("a{ 2}", 0), ("a{2,3,4}", 0), ("a{-1}", 0), ("(" * 33 + "a" + ")" * 33, 0), ("a{65}", 0),
    ("(ab){33}", 0), ("(a|b){1,33}", 0), ("x" * 65, 0), ("a{99999999999999999999}", 0), ("()", 0), ("(|)", 0), ("(){3}", 0),
    ("a?", 0), ("a|", 0), ("|a", 0), ("(a|)", 0), ("a?b{0,3}", 0), ("(a?b?){2}", 0), ("[abc", 0), ("[c-a]", 0), ("a\\", 0),
    (r"\x4", 0), ("(a|[b)", 0), ("abc", 4), ("abc", 8), ("abc", 1 << 31),
]


def _bits(positions):
    return sum(1 << i for i in positions)


def _compile_raw(expr, flags):
    """(rc, struct, untouched?) through the C ABI, with a sentinel pattern in *out."""
    e = expr.encode("latin-1") if isinstance(expr, str) else bytes(expr)
    out = host.Regex()
    C.memset(C.byref(out), 0xA5, C.sizeof(out))
    rc = host.lib().bmx_compile_regex(e, len(e), flags, C.byref(out))
    return rc, out, bytes(out) == b"\xa5" * C.sizeof(out)


def _same(got: host.Regex, want: ro.Rx, what):
    assert got.m == want.m, what
    assert np.array_equal(co.unpack(got.class_array()), want.member), what
    assert got.first == want.first and got.last == want.last, what
    assert list(got.follow)[: want.m] == want.follow and not any(list(got.follow)[want.m:]), what
    assert (got.min_len, got.max_len) == (want.min_len, want.max_len), what


def _tiny_case(rng, case):
    alpha = 2 + case % 2
    symbols = np.arange(97, 97 + alpha)
    text = rng.choice(symbols, int(rng.integers(0, 40))).astype(np.uint8).tobytes()
    expr, rx = ro.random_regex(rng, symbols, 10)
    return text, expr, rx


def test_oracle_equals_the_brute_force_on_tiny_cases():
    rng = np.random.default_rng(0x2E6E)
    non_empty = with_variants = 0
    for case in range(400):
        text, expr, rx = _tiny_case(rng, case)
        ends, short, long_ = ro.ends_brute(text, expr)
        assert ro.match_ends(text, rx) == (ends, short, long_), (case, expr, text)
        assert ro.ends_numpy(text, rx).tolist() == ends, (case, expr, text)
        assert ro.word_ends(text, rx, 32).tolist() == ends, (case, expr, text)
        assert ro.word_ends(text, rx, 64).tolist() == ends, (case, expr, text)
        e1, s1 = ro.starts_numpy(text, rx)
        e2, s2 = ro.starts_numpy(text, rx, longest=True)
        assert e1.tolist() == ends and s1.tolist() == short, (case, expr, text)
        assert e2.tolist() == ends and s2.tolist() == long_, (case, expr, text)
        try:  # (defined for expressions with at most 64 paths)
            assert ro.variant_ends(text, rx).tolist() == ends, (case, expr, text)
            with_variants += 1
        except ValueError:
            pass
        assert all(f >> (i + 1) << (i + 1) == f for i, f in enumerate(rx.follow)), expr  # follow points upward only
        assert 1 <= rx.min_len <= rx.max_len <= rx.m
        non_empty += bool(ends)
    assert 3 * non_empty >= 400, non_empty
    assert with_variants >= 300, with_variants


def test_word_recurrence_at_both_widths_on_larger_automata():
    rng = np.random.default_rng(0x2E6F)
    symbols = np.arange(97, 100)
    widths = set()
    for case in range(300):
        max_m = (12, 32, 64)[case % 3]
        expr, rx = ro.random_regex(rng, symbols, max_m)
        text = rng.choice(symbols, int(rng.integers(0, 160))).astype(np.uint8).tobytes()
        want = ro.ends_numpy(text, rx).tolist()
        if rx.m <= 32:
            assert ro.word_ends(text, rx, 32).tolist() == want, (case, expr)
        assert ro.word_ends(text, rx, 64).tolist() == want, (case, expr)
        widths.add(rx.m > 32)
        # the reversed automaton is upward-only again and finds the starts: anchored at an end, going down
        rev = ro.reverse(rx)
        assert all(f >> (i + 1) << (i + 1) == f for i, f in enumerate(rev.follow)), expr
        assert (rev.min_len, rev.max_len) == (rx.min_len, rx.max_len), expr
    assert widths == {False, True}


def test_expression_table(built):
    for expr, flags, m, first, last, follow, min_len, max_len in TABLE:
        got = host.compile_regex(expr, flags)
        what = (expr, flags)
        assert got.m == m and got.first == _bits(first) and got.last == _bits(last), what
        assert [got.follow[i] for i in range(m)] == [_bits(follow.get(i, [])) for i in range(m)], what
        assert (got.min_len, got.max_len) == (min_len, max_len), what
        _same(got, ro.parse(expr, flags), what)
    for expr in WHY:
        for flags in (0, ICASE, IUPAC, ICASE | IUPAC):
            _same(host.compile_regex(expr, flags), ro.parse(expr, flags), (expr, flags))
    assert [host.compile_regex(e).m for e in WHY] == [24, 21, 15, 12]
    assert [(r.min_len, r.max_len) for r in map(host.compile_regex, WHY)] == [(12, 18), (9, 11), (7, 15), (6, 9)]
    sets = [bytes(np.nonzero(row)[0].astype(np.uint8)) for row in co.unpack(host.compile_regex(r"\x41(\.|\\)").class_array())]
    assert sets == [b"A", b".", b"\\"]
    sets = [bytes(np.nonzero(row)[0].astype(np.uint8)) for row in co.unpack(host.compile_regex("(r|Y)n", ICASE | IUPAC).class_array())]
    assert sets == [b"Rr", b"CTct", b"Nn"]  # (a lower-case letter is no IUPAC code)


def test_compiler_equals_the_oracle_on_random_expressions(built):
    rng = np.random.default_rng(0x2E70)
    for case in range(400):
        symbols = np.arange(97, 97 + 2 + case % 3)
        expr, rx = ro.random_regex(rng, symbols, (8, 32, 64)[case % 3])
        _same(host.compile_regex(expr), rx, expr)
    # random byte strings over the grammar's own alphabet: the same verdict, and the same automaton where there is one
    alphabet = np.frombuffer(b"ab]^-[\\.xN?{},0123*+()|\xe9", np.uint8)
    agreed = 0
    for case in range(3000):
        e = alphabet[rng.integers(0, alphabet.size, int(rng.integers(0, 14)))].tobytes()
        flags = case % 4
        rc, out, untouched = _compile_raw(e, flags)
        try:
            rx = ro.parse(e, flags)
        except ro.ExprError:
            assert rc == host.ERR_ARG and untouched, (e, flags)
            continue
        assert rc == host.OK, (e, flags)
        _same(out, rx, (e, flags))
        agreed += 1
    assert agreed > 300, agreed


def test_without_groups_the_language_is_compile_gaps(built):
    rng = np.random.default_rng(0x2E71)
    symbols = np.arange(97, 100)
    exprs = ["abc", "colou?r", "a{1,3}b", "a.{0,2}b", "a?b?c", "[a-c]{2,3}[^x]?y", "a{2}b?c{0,2}a"]
    for expr in exprs:
        rx = ro.parse(expr)
        classes, optional = host.compile_gaps(expr)
        _same(host.compile_regex(expr), rx, expr)
        for _ in range(20):
            text = rng.choice(symbols, int(rng.integers(0, 60))).astype(np.uint8).tobytes()
            want = go.gap_starts(text, co.unpack(classes), optional)
            got = ro.starts_numpy(text, rx)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (expr, text)
            assert np.array_equal(ro.starts_numpy(text, rx, True)[1], go.gap_starts(text, co.unpack(classes), optional, True)[1])


def test_expression_errors(built):
    L = host.lib()
    for expr, flags in ERRORS:
        rc, out, untouched = _compile_raw(expr, flags)
        assert rc == host.ERR_ARG and untouched, (expr, flags)
        assert L.bmx_last_error().startswith(b"bmx_compile_regex: "), (expr, flags)
        with pytest.raises(ro.ExprError):
            ro.parse(expr, flags)
    for expr in ("a*", "(ab)+", "a{2,}"):
        _compile_raw(expr, 0)
        assert b"unbounded repetition is out of scope" in L.bmx_last_error(), expr
    assert host.compile_regex("(" * 32 + "a" + ")" * 32).m == 1  # 32 levels are fine
    out = host.Regex()
    assert L.bmx_compile_regex(None, 0, 0, C.byref(out)) == host.ERR_ARG
    assert L.bmx_compile_regex(b"a", 1, 0, None) == host.ERR_ARG
    with pytest.raises(host.BmxError) as e:
        host.compile_regex("a*")
    assert e.value.rc == host.ERR_ARG


def _automaton(expr="(a|bc)d"):
    return host.compile_regex(expr)


def _broken():
    """(what, automaton) for every validation rule of struct bmx_regex."""
    def edit(f, expr="(a|bc)d"):
        r = _automaton(expr)
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
            ("follow beyond m", edit(follow(2, 1 << 3 | 1 << 4))), ("follow to itself", edit(follow(1, 1 << 1 | 1 << 2))),
            ("follow downward", edit(follow(3, 1 << 0))), ("follow[63] upward", edit(follow(63, 1 << 63), "x{64}"))]


def test_automaton_validation_before_any_device_call(built):
    L = host.lib()
    text = b"some text to search in"
    out = (C.c_uint64 * 8)()
    total = C.c_uint64(0)
    for what, r in _broken():
        p = C.byref(r)
        assert L.bmx_search_regex(None, text, len(text), p, out, 8, C.byref(total)) == host.ERR_ARG, what
        assert L.bmx_search_regex_spans(None, text, len(text), p, 0, out, out, 8, C.byref(total)) == host.ERR_ARG, what
        assert L.bmx_search_regex_device(None, None, 10, 0, 0, p, None, 0, C.byref(total), None) == host.ERR_ARG, what
        assert L.bmx_regex_starts_device(None, None, 10, 0, p, out, 0, 0, out, None) == host.ERR_ARG, what  # even with count == 0
    # legal oddities pass the validation (the call then fails for want of a device or returns at once): an empty class,
    # positions that no match can use, min_len / max_len fields that say nothing
    r = _automaton()
    C.memset(r.classes, 0, 32)
    r.follow[0] = 0
    r.min_len = r.max_len = -5
    assert L.bmx_regex_starts_device(None, None, 10, 0, C.byref(r), None, 0, 0, None, None) == host.OK
    assert L.bmx_search_regex(None, text, 0, C.byref(r), out, 8, C.byref(total)) == host.OK and total.value == 0


def test_argument_errors_before_any_device_call(built):
    L = host.lib()
    text = b"some text to search in"
    out = (C.c_uint64 * 8)()
    total = C.c_uint64(0)
    r = _automaton()
    p = C.byref(r)
    assert L.bmx_search_regex(None, text, len(text), None, out, 8, C.byref(total)) == host.ERR_ARG
    assert L.bmx_search_regex(None, text, len(text), p, None, 8, C.byref(total)) == host.ERR_ARG  # a capacity needs room
    assert L.bmx_search_regex(None, None, len(text), p, out, 8, C.byref(total)) == host.ERR_ARG
    assert L.bmx_search_regex(None, text, 1 << 40, p, out, 8, C.byref(total)) == host.ERR_ARG
    sp = L.bmx_search_regex_spans
    assert sp(None, text, len(text), None, 0, out, out, 8, C.byref(total)) == host.ERR_ARG
    assert sp(None, text, len(text), p, 0, None, out, 8, C.byref(total)) == host.ERR_ARG
    assert sp(None, text, len(text), p, 0, out, None, 8, C.byref(total)) == host.ERR_ARG
    assert sp(None, None, len(text), p, 0, out, out, 8, C.byref(total)) == host.ERR_ARG
    assert sp(None, text, len(text), p, 2, out, out, 8, C.byref(total)) == host.ERR_ARG  # an unknown flag bit
    assert sp(None, text, 1 << 40, p, 0, out, out, 8, C.byref(total)) == host.ERR_ARG
    dev = L.bmx_search_regex_device
    assert dev(None, None, 10, 0, 0, None, None, 0, C.byref(total), None) == host.ERR_ARG
    assert dev(None, None, 10, 11, 0, p, None, 0, C.byref(total), None) == host.ERR_ARG  # lead > n
    assert dev(None, None, 1 << 40, 0, 0, p, None, 0, C.byref(total), None) == host.ERR_ARG
    assert dev(None, None, 10, 0, 0, p, None, 8, C.byref(total), None) == host.ERR_ARG  # capacity, no ends
    assert dev(None, None, 10, 0, 0, p, None, 0, C.byref(total), None) == host.ERR_ARG  # no context
    st = L.bmx_regex_starts_device
    assert st(None, None, 10, 0, None, out, 8, 0, out, None) == host.ERR_ARG
    assert st(None, None, 10, 0, p, out, 8, 2, out, None) == host.ERR_ARG  # an unknown flag bit
    assert st(None, None, 1 << 40, 0, p, out, 8, 0, out, None) == host.ERR_ARG
    assert st(None, None, 10, 0, p, None, 8, 0, out, None) == host.ERR_ARG
    assert st(None, None, 10, 0, p, out, 8, 0, None, None) == host.ERR_ARG
    assert st(None, None, 10, 0, p, out, 8, host.REGEX_LONGEST, out, None) == host.ERR_ARG  # no context
    assert st(None, None, 10, 0, p, None, 0, 0, None, None) == host.OK  # count == 0: nothing to do, no context needed
    assert L.bmx_last_regex_ms(None) < 0


def test_library_exports_regex_symbols(built):
    L = C.CDLL(host.LIB_PATH)
    X = C.CDLL(host.EXP_LIB_PATH)
    for name in ("bmx_compile_regex", "bmx_search_regex_device", "bmx_search_regex", "bmx_search_regex_spans", "bmx_last_regex_ms",
                 "bmx_regex_starts_device"):
        assert hasattr(L, name) and hasattr(X, name), name
        assert name in [s for s, _, _ in host.SYMBOLS]
    for name in ("compile_regex", "search_regex", "Regex", "REGEX_LONGEST", "MAX_REGEX_POSITIONS"):
        assert getattr(pkg, name) is getattr(host, name)
    for name in ("search_regex_device", "search_regex", "search_regex_spans", "regex_starts_device", "last_regex_ms"):
        assert callable(getattr(host.Context, name))


def test_header_constants_and_struct_layout():
    src = open(os.path.join(ROOT, "include", "bmx.h")).read()

    def define(name):
        return int(re.search(rf"#define {name} (\d+)", src).group(1))

    assert define("BMX_MAX_REGEX_POSITIONS") == host.MAX_REGEX_POSITIONS == ro.MAX_M == 64
    assert define("BMX_REGEX_LONGEST") == host.REGEX_LONGEST == 1
    assert define("BMX_MAX_GAPS_PATTERN") == 64 and define("BMX_GAPS_LONGEST") == 1  # unchanged
    R = host.Regex
    assert (R.m.offset, R.min_len.offset, R.max_len.offset, R.first.offset, R.last.offset) == (0, 4, 8, 16, 24)
    assert (R.follow.offset, R.classes.offset, C.sizeof(R)) == (32, 32 + 512, 32 + 512 + 2048)
