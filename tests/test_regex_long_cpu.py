"""CPU suite for the regular-expression search of up to 128 positions (bmx_compile_regex_long, bmx_regex_long_widen,
bmx_search_regex_long*, bmx_regex_long_starts_device): the oracle against a brute force over Python's ``re`` on expressions
of 65..128 positions, the four-dword recurrence of the kernel against the matcher that carries position sets, the
expression compiler against the oracle on a fixed table and on random expressions, every compiler error with *out
untouched, byte identity with bmx_compile_regex up to 64 positions, the widening, the validation of a caller's automaton,
the new C-ABI symbols, constants and the struct layout, and the argument errors that return before any HIP call.  No
compute call is made on a device here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import classes_oracle as co
import regex_long_oracle as rl
import regex_oracle as ro
from conftest import ROOT
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host
import parallel_implementation_of_string_matching_algorithms_opencl_amd as pkg
from test_regex_cpu import ERRORS as ERRORS_64

ICASE, IUPAC = host.CLASS_ICASE, host.CLASS_IUPAC
KEYWORDS = "(ERROR|FATAL|PANIC|WARNING|CRITICAL|EXCEPTION|TIMEOUT|REFUSED|DENIED|ABORTED): [0-9]{2,4}"
# the expressions that motivate the entries.  The ORF expression as written, with {2,40}, expands to 3 + 120 + 9 = 132
# positions: compiler and oracle must agree on refusing it; {2,38} is the longest repeat that fits (126).
WHY = ["a.{0,100}b", "ATG([ACGT]{3}){2,40}(TAA|TAG|TGA)", "ATG([ACGT]{3}){2,38}(TAA|TAG|TGA)",
       "C.{2,4}C.{20,40}[LIVMFYWC].{8,16}H.{3,5}H",  # a PROSITE-style motif with x(20,40)
       KEYWORDS]
WHY_M = [102, None, 126, 70, 72]
WHY_LEN = [(2, 102), None, (12, 120), (38, 70), (9, 15)]
# (expression, m, min_len, max_len), None where it must be refused
TABLE = [("x{64}", 64, 64, 64), ("x{65}", 65, 65, 65), ("x{128}", 128, 128, 128), ("(ab){64}", 128, 128, 128),
         ("(a|b){1,64}", 128, 1, 64), ("x{127}", 127, 127, 127), ("x{63}y?", 64, 63, 64), ("x{64}y?", 65, 64, 65),
         ("(abc|de){1,25}f", 126, 3, 76), ("x{129}", None, 0, 0), ("(ab){65}", None, 0, 0), ("(a|b){1,65}", None, 0, 0),
         ("x{128}y", None, 0, 0)]
# what bmx_compile_regex refuses only for its 64 positions
FIT_128 = {"a{65}", "(ab){33}", "(a|b){1,33}", "x" * 65}
ERRORS = [(e, f) for e, f in ERRORS_64 if e not in FIT_128] + [("x{129}", 0), ("(ab){65}", 0), ("x" * 129, 0), ("(a|b){1,65}", 0),
                                                               ("a{999}", 0), ("(x{64}){3}", 0)]


def _compile_raw(expr, flags):
    """(rc, struct, untouched?) through the C ABI, with a sentinel pattern in *out."""
    e = expr.encode("latin-1") if isinstance(expr, str) else bytes(expr)
    out = host.RegexLong()
    C.memset(C.byref(out), 0xA5, C.sizeof(out))
    rc = host.lib().bmx_compile_regex_long(e, len(e), flags, C.byref(out))
    return rc, out, bytes(out) == b"\xa5" * C.sizeof(out)


def _same(got: host.RegexLong, want: ro.Rx, what):
    assert got.m == want.m and got.pad == 0, what
    assert np.array_equal(co.unpack(got.class_array()), want.member), what
    assert got.first_set == want.first and got.last_set == want.last, what
    assert [got.follow_set(i) for i in range(want.m)] == want.follow, what
    assert not any(got.follow_set(i) for i in range(want.m, 128)), what
    assert not any(bytes(got.classes)[want.m * 32:]), what
    assert (got.min_len, got.max_len) == (want.min_len, want.max_len), what


def test_oracle_equals_the_brute_force_on_tiny_cases():
    rng = np.random.default_rng(0x331C)
    non_empty = 0
    sizes = set()
    for case in range(300):
        symbols = np.arange(97, 97 + 2 + case % 2)
        text = rng.choice(symbols, int(rng.integers(0, 36))).astype(np.uint8).tobytes()
        expr, rx = rl.random_regex(rng, symbols, 65, 128, bar=0.7)
        assert 65 <= rx.m <= 128
        sizes.add(rx.m > 96)
        ends, short, long_ = ro.ends_brute(text, expr)
        assert ro.match_ends(text, rx) == (ends, short, long_), (case, expr, text)
        assert ro.ends_numpy(text, rx).tolist() == ends, (case, expr, text)
        assert rl.word_ends(text, rx)[0].tolist() == ends, (case, expr, text)
        e1, s1 = ro.starts_numpy(text, rx)
        e2, s2 = ro.starts_numpy(text, rx, longest=True)
        assert e1.tolist() == ends and s1.tolist() == short, (case, expr, text)
        assert e2.tolist() == ends and s2.tolist() == long_, (case, expr, text)
        assert all(f >> (i + 1) << (i + 1) == f for i, f in enumerate(rx.follow)), expr  # follow points upward only
        assert 1 <= rx.min_len <= rx.max_len <= rx.m
        non_empty += bool(ends)
    assert 3 * non_empty > 300, non_empty
    assert sizes == {False, True}


def test_word_recurrence_on_four_dwords():
    rng = np.random.default_rng(0x331D)
    symbols = np.arange(97, 100)
    slots_seen = set()
    for case in range(150):
        lo, hi = ((1, 32), (33, 64), (65, 96), (97, 128), (120, 128))[case % 5]
        expr, rx = rl.random_regex(rng, symbols, lo, hi, bar=(0.1, 0.5)[case % 2])
        text = bytearray(rng.choice(symbols, int(rng.integers(0, 400))).astype(np.uint8).tobytes())
        arr = np.frombuffer(text, np.uint8)
        for _ in range(3):
            if arr.size:
                ro.plant_path(rng, arr, rx, int(rng.integers(0, arr.size)))
        want = ro.match_ends(bytes(text), rx)[0]
        got, slots = rl.word_ends(bytes(text), rx)
        assert got.tolist() == want, (case, expr)
        assert ro.ends_numpy(bytes(text), rx).tolist() == want, (case, expr)
        slots_seen.add(0 if slots == 0 else 7 if slots <= 7 else 12 if slots <= 12 else 16)
        # the reversed automaton is upward-only again and anchored at an end it finds the starts
        rev = ro.reverse(rx)
        assert all(f >> (i + 1) << (i + 1) == f for i, f in enumerate(rev.follow)), expr
        assert (rev.min_len, rev.max_len) == (rx.min_len, rx.max_len), expr
    assert slots_seen == {0, 7, 12, 16}, slots_seen
    # a carry across every dword boundary, by shift and by table
    text = b"x" * 30 + b"y" + b"x" * 30 + b"z" + b"x" * 30 + b"y" + b"x" * 140
    for expr in ("x{128}", "x{30}(y|z)x{30}(y|z)x{30}(y|z)x{31}"):
        rx = rl.parse(expr)
        assert rx.m in (127, 128)
        assert rl.word_ends(text, rx)[0].tolist() == ro.ends_numpy(text, rx).tolist() != [], expr


def test_expression_table(built):
    for expr, m, min_len, max_len in TABLE:
        rc, got, untouched = _compile_raw(expr, 0)
        if m is None:
            assert rc == host.ERR_ARG and untouched, expr
            with pytest.raises(rl.ExprError):
                rl.parse(expr)
            continue
        assert rc == host.OK and (got.m, got.min_len, got.max_len) == (m, min_len, max_len), expr
        _same(got, rl.parse(expr), expr)
    for expr, m, lens in zip(WHY, WHY_M, WHY_LEN):
        for flags in (0, ICASE, IUPAC, ICASE | IUPAC):
            rc, got, untouched = _compile_raw(expr, flags)
            if m is None:
                assert rc == host.ERR_ARG and untouched and rl.positions(expr) == 132, expr
                with pytest.raises(rl.ExprError):
                    rl.parse(expr, flags)
                continue
            assert rc == host.OK and got.m == m, (expr, flags)
            _same(got, rl.parse(expr, flags), (expr, flags))
        if m is not None:
            got = host.compile_regex_long(expr)
            assert (got.min_len, got.max_len) == lens, expr
    # x{128}: one chain through both words; (a|b){1,64}: every position is a last one and every later copy may follow
    r = host.compile_regex_long("x{128}")
    assert r.first_set == 1 and r.last_set == 1 << 127 and [r.follow_set(i) for i in range(128)] == [1 << (i + 1) for i in range(127)] + [0]
    r = host.compile_regex_long("(a|b){1,64}")
    assert r.first_set == 3 and r.last_set == (1 << 128) - 1 and r.follow_set(63) == ((1 << 64) - 1) << 64 and r.follow_set(126) == 0


def test_compiler_equals_the_oracle_on_random_expressions(built):
    rng = np.random.default_rng(0x331E)
    for case in range(300):
        symbols = np.arange(97, 97 + 2 + case % 3)
        lo, hi = ((1, 64), (65, 128), (100, 128))[case % 3]
        expr, rx = rl.random_regex(rng, symbols, lo, hi, bar=(1 / 6, 0.6)[case % 2])
        _same(host.compile_regex_long(expr), rx, expr)
    # random byte strings over the grammar's own alphabet: the same verdict, and the same automaton where there is one
    alphabet = np.frombuffer(b"ab]^-[\\.xN?{},0123*+()|\xe9", np.uint8)
    agreed = big = 0
    for case in range(3000):
        e = alphabet[rng.integers(0, alphabet.size, int(rng.integers(0, 14)))].tobytes()
        if case % 3 == 0:  # counts that reach past 64 and past 128 positions
            e += b"{%d}" % int(rng.integers(30, 140))
        flags = case % 4
        rc, out, untouched = _compile_raw(e, flags)
        try:
            rx = rl.parse(e, flags)
        except rl.ExprError:
            assert rc == host.ERR_ARG and untouched, (e, flags)
            continue
        assert rc == host.OK, (e, flags)
        _same(out, rx, (e, flags))
        agreed += 1
        big += rx.m > 64
    assert agreed > 300 and big > 20, (agreed, big)


def test_expression_errors(built):
    L = host.lib()
    assert {e for e, _ in ERRORS_64} >= FIT_128
    for expr in FIT_128:
        assert host.compile_regex_long(expr).m in (65, 66)
    for expr, flags in ERRORS:
        rc, out, untouched = _compile_raw(expr, flags)
        assert rc == host.ERR_ARG and untouched, (expr, flags)
        assert L.bmx_last_error().startswith(b"bmx_compile_regex_long: "), (expr, flags, L.bmx_last_error())
        with pytest.raises(rl.ExprError):
            rl.parse(expr, flags)
    for expr in ("a*", "(ab)+", "a{2,}"):
        _compile_raw(expr, 0)
        assert b"unbounded repetition is out of scope" in L.bmx_last_error(), expr
    _compile_raw("x{129}", 0)
    assert b"more than 128 positions" in L.bmx_last_error()
    assert host.compile_regex_long("(" * 32 + "a" + ")" * 32).m == 1  # 32 levels are fine
    out = host.RegexLong()
    assert L.bmx_compile_regex_long(None, 0, 0, C.byref(out)) == host.ERR_ARG
    assert L.bmx_compile_regex_long(b"a", 1, 0, None) == host.ERR_ARG
    with pytest.raises(host.BmxError) as e:
        host.compile_regex_long("a*")
    assert e.value.rc == host.ERR_ARG
    # the 64-position entry still refuses what only the long one takes, with its own text
    with pytest.raises(host.BmxError):
        host.compile_regex("x{65}")
    assert L.bmx_last_error().startswith(b"bmx_compile_regex: more than 64 positions")


def _widened_by_hand(r: host.Regex) -> host.RegexLong:
    w = host.RegexLong()
    w.m, w.min_len, w.max_len = r.m, r.min_len, r.max_len
    w.first[0], w.last[0] = r.first, r.last
    for i in range(64):
        w.follow[i][0] = r.follow[i]
    C.memmove(w.classes, r.classes, 64 * 32)
    return w


def test_byte_identity_up_to_64_positions_and_widen(built):
    rng = np.random.default_rng(0x331F)
    exprs = ["a", "x{64}", "(a|bc)d", "a(b|c)?d", "(a?b?){2}c", "ATG([ACGT]{3}){2,4}(TAA|TAG|TGA)", "(ERROR|FATAL|PANIC): [0-9]{2,4}"]
    exprs += [rl.random_regex(rng, np.arange(97, 100), 1, 64)[0] for _ in range(100)]
    for expr in exprs:
        for flags in (0, ICASE | IUPAC):
            short = host.compile_regex(expr, flags)
            long_ = host.compile_regex_long(expr, flags)
            want = _widened_by_hand(short)
            assert bytes(long_) == bytes(want), expr
            assert long_.first[1] == long_.last[1] == 0 and not any(long_.follow[i][1] for i in range(128)), expr
            assert bytes(host.widen_regex(short)) == bytes(want), expr
    # widen recomputes the lengths and refuses what bmx_search_regex_device refuses
    L = host.lib()
    r = host.compile_regex("(a|bc)d")
    r.min_len = r.max_len = -7
    w = host.widen_regex(r)
    assert (w.min_len, w.max_len) == (2, 3)
    out = host.RegexLong()
    C.memset(C.byref(out), 0xA5, C.sizeof(out))
    assert L.bmx_regex_long_widen(None, C.byref(out)) == host.ERR_ARG
    assert L.bmx_regex_long_widen(C.byref(r), None) == host.ERR_ARG
    for bad in ("m", "first", "last"):
        b = host.compile_regex("(a|bc)d")
        setattr(b, bad, 0)
        assert L.bmx_regex_long_widen(C.byref(b), C.byref(out)) == host.ERR_ARG, bad
    b = host.compile_regex_star("(ab)+c")  # a cycle
    assert L.bmx_regex_long_widen(C.byref(b), C.byref(out)) == host.ERR_ARG
    assert bytes(out) == b"\xa5" * C.sizeof(out)


def _automaton(expr="(a|bc)d"):
    return host.compile_regex_long(expr)


def _broken():
    """(what, automaton) for every validation rule of struct bmx_regex_long."""
    def edit(f, expr="(a|bc)d"):
        r = _automaton(expr)
        f(r)
        return r

    def set_(name, value):
        return lambda r: setattr(r, name, value)

    def words(name, lo, hi):
        def f(r):
            getattr(r, name)[0], getattr(r, name)[1] = lo, hi
        return f

    def follow(i, lo, hi):
        def f(r):
            r.follow[i][0], r.follow[i][1] = lo, hi
        return f

    return [("m == 0", edit(set_("m", 0))), ("m < 0", edit(set_("m", -1))), ("m > 128", edit(set_("m", 129))),
            ("first empty", edit(words("first", 0, 0))), ("last empty", edit(words("last", 0, 0))),
            ("first beyond m", edit(words("first", 1 | 1 << 4, 0))), ("first beyond m, high word", edit(words("first", 1, 1))),
            ("last beyond m", edit(words("last", 1 << 63, 0))), ("last beyond m, high word", edit(words("last", 8, 1 << 63))),
            ("follow beyond m", edit(follow(2, 1 << 3 | 1 << 4, 0))), ("follow beyond m, high word", edit(follow(2, 1 << 3, 1))),
            ("follow to itself", edit(follow(1, 1 << 1 | 1 << 2, 0))), ("follow downward", edit(follow(3, 1 << 0, 0))),
            ("follow to itself, high word", edit(follow(70, 0, 1 << 6 | 1 << 7), "x{128}")),
            ("follow downward across the words", edit(follow(64, 1 << 63, 2), "x{128}")),
            ("follow[127] upward", edit(follow(127, 0, 1 << 63), "x{128}")),
            ("beyond m = 65", edit(follow(3, 0, 2), "x{65}"))]


def test_automaton_validation_before_any_device_call(built):
    L = host.lib()
    text = b"some text to search in"
    out = (C.c_uint64 * 8)()
    total = C.c_uint64(0)
    for what, r in _broken():
        p = C.byref(r)
        assert L.bmx_search_regex_long(None, text, len(text), p, out, 8, C.byref(total)) == host.ERR_ARG, what
        assert L.bmx_search_regex_long_spans(None, text, len(text), p, 0, out, out, 8, C.byref(total)) == host.ERR_ARG, what
        assert L.bmx_search_regex_long_device(None, None, 10, 0, 0, p, None, 0, C.byref(total), None) == host.ERR_ARG, what
        assert L.bmx_regex_long_starts_device(None, None, 10, 0, p, out, 0, 0, out, None) == host.ERR_ARG, what  # even with count == 0
    # legal oddities pass the validation (the call then returns at once): an empty class, positions that no match can use,
    # min_len / max_len / pad fields that say nothing, m at both ends of its range
    for expr in ("(a|bc)d", "x{128}", "a"):
        r = _automaton(expr)
        C.memset(r.classes, 0, 32)
        r.follow[0][0] = r.follow[0][1] = 0
        r.min_len = r.max_len = -5
        r.pad = 77
        assert L.bmx_regex_long_starts_device(None, None, 10, 0, C.byref(r), None, 0, 0, None, None) == host.OK, expr
        assert L.bmx_search_regex_long(None, text, 0, C.byref(r), out, 8, C.byref(total)) == host.OK and total.value == 0, expr
    r = _automaton("x{65}")  # a link across the two words is legal
    r.follow[0][1] = 1
    assert L.bmx_regex_long_starts_device(None, None, 10, 0, C.byref(r), None, 0, 0, None, None) == host.OK


def test_argument_errors_before_any_device_call(built):
    L = host.lib()
    text = b"some text to search in"
    out = (C.c_uint64 * 8)()
    total = C.c_uint64(0)
    r = _automaton()
    p = C.byref(r)
    assert L.bmx_search_regex_long(None, text, len(text), None, out, 8, C.byref(total)) == host.ERR_ARG
    assert L.bmx_search_regex_long(None, text, len(text), p, None, 8, C.byref(total)) == host.ERR_ARG  # a capacity needs room
    assert L.bmx_search_regex_long(None, None, len(text), p, out, 8, C.byref(total)) == host.ERR_ARG
    assert L.bmx_search_regex_long(None, text, 1 << 40, p, out, 8, C.byref(total)) == host.ERR_ARG
    sp = L.bmx_search_regex_long_spans
    assert sp(None, text, len(text), None, 0, out, out, 8, C.byref(total)) == host.ERR_ARG
    assert sp(None, text, len(text), p, 0, None, out, 8, C.byref(total)) == host.ERR_ARG
    assert sp(None, text, len(text), p, 0, out, None, 8, C.byref(total)) == host.ERR_ARG
    assert sp(None, None, len(text), p, 0, out, out, 8, C.byref(total)) == host.ERR_ARG
    assert sp(None, text, len(text), p, 2, out, out, 8, C.byref(total)) == host.ERR_ARG  # an unknown flag bit
    assert sp(None, text, 1 << 40, p, 0, out, out, 8, C.byref(total)) == host.ERR_ARG
    dev = L.bmx_search_regex_long_device
    assert dev(None, None, 10, 0, 0, None, None, 0, C.byref(total), None) == host.ERR_ARG
    assert dev(None, None, 10, 11, 0, p, None, 0, C.byref(total), None) == host.ERR_ARG  # lead > n
    assert dev(None, None, 1 << 40, 0, 0, p, None, 0, C.byref(total), None) == host.ERR_ARG
    assert dev(None, None, 10, 0, 0, p, None, 8, C.byref(total), None) == host.ERR_ARG  # capacity, no ends
    assert dev(None, None, 10, 0, 0, p, None, 0, C.byref(total), None) == host.ERR_ARG  # no context
    st = L.bmx_regex_long_starts_device
    assert st(None, None, 10, 0, None, out, 8, 0, out, None) == host.ERR_ARG
    assert st(None, None, 10, 0, p, out, 8, 2, out, None) == host.ERR_ARG  # an unknown flag bit
    assert st(None, None, 1 << 40, 0, p, out, 8, 0, out, None) == host.ERR_ARG
    assert st(None, None, 10, 0, p, None, 8, 0, out, None) == host.ERR_ARG
    assert st(None, None, 10, 0, p, out, 8, 0, None, None) == host.ERR_ARG
    assert st(None, None, 10, 0, p, out, 8, host.REGEX_LONGEST, out, None) == host.ERR_ARG  # no context
    assert st(None, None, 10, 0, p, None, 0, 0, None, None) == host.OK  # count == 0: nothing to do, no context needed
    assert L.bmx_last_regex_long_ms(None) < 0
    # the Python layer: kind="regex" still refuses an expression of more than 64 positions, posix refuses the long kind
    with pytest.raises(host.BmxError):
        host._regex("x{65}")
    with pytest.raises(ValueError):
        host._posix_args("regex_long")
    with pytest.raises(ValueError):
        host._regex_long(host.compile_regex("a"))


def test_library_exports_regex_long_symbols(built):
    L = C.CDLL(host.LIB_PATH)
    X = C.CDLL(host.EXP_LIB_PATH)
    for name in ("bmx_compile_regex_long", "bmx_regex_long_widen", "bmx_search_regex_long_device", "bmx_search_regex_long",
                 "bmx_search_regex_long_spans", "bmx_last_regex_long_ms", "bmx_regex_long_starts_device"):
        assert hasattr(L, name) and hasattr(X, name), name
        assert name in [s for s, _, _ in host.SYMBOLS]
    for name in ("compile_regex_long", "widen_regex", "search_regex_long", "RegexLong", "MAX_REGEX_LONG_POSITIONS"):
        assert getattr(pkg, name) is getattr(host, name)
    for name in ("search_regex_long_device", "search_regex_long", "search_regex_long_spans", "regex_long_starts_device",
                 "last_regex_long_ms"):
        assert callable(getattr(host.Context, name))


def test_header_constants_and_struct_layout():
    src = open(os.path.join(ROOT, "include", "bmx.h")).read()

    def define(name):
        return int(re.search(rf"#define {name} (\d+)", src).group(1))

    assert define("BMX_MAX_REGEX_LONG_POSITIONS") == host.MAX_REGEX_LONG_POSITIONS == rl.MAX_M == 128
    assert define("BMX_MAX_REGEX_POSITIONS") == host.MAX_REGEX_POSITIONS == 64  # unchanged
    R = host.RegexLong
    assert (R.m.offset, R.min_len.offset, R.max_len.offset, R.pad.offset, R.first.offset, R.last.offset) == (0, 4, 8, 12, 16, 32)
    assert (R.follow.offset, R.classes.offset, C.sizeof(R)) == (48, 48 + 2048, 48 + 2048 + 4096)
    assert C.sizeof(host.Regex) == 32 + 512 + 2048  # unchanged
    body = src[src.index("typedef struct bmx_regex_long {"):src.index("} bmx_regex_long;")]
    at = [body.index(" " + name) for name, _ in R._fields_]  # the fields in the header's order
    assert at == sorted(at) and [name for name, _ in R._fields_] == ["m", "min_len", "max_len", "pad", "first", "last", "follow", "classes"]
