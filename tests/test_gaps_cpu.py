"""CPU suite for the gapped pattern search (bmx_compile_gaps, bmx_search_gaps*, bmx_gaps_starts_device): the expression
compiler against a table of exact positions and against the grammar restated in Python, the numpy matcher against a brute
force over regular expressions, the recurrence of the kernel word by word against the matcher (which pins the four mask
words), the two identities of include/bmx.h, the new C-ABI symbols and constants, and the argument errors that return
before any HIP call.  No compute call is made on a device here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import classes_oracle as co
import gaps_oracle as go
from conftest import ROOT
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host
import parallel_implementation_of_string_matching_algorithms_opencl_amd as pkg

ALL = bytes(range(256))
ZINC = "C-x(2,4)-C-x(3)-[LIVMFYWC]-x(8)-H-x(3,5)-H"
ICASE, IUPAC, PROSITE = host.CLASS_ICASE, host.CLASS_IUPAC, host.GAPS_PROSITE


def _without(*drop):
    return bytes(b for b in range(256) if b not in drop)


def _sets(classes):
    return [bytes(np.nonzero(row)[0].astype(np.uint8)) for row in co.unpack(classes)]


def _bits(*positions):
    return sum(1 << i for i in positions)


# (expression, flags, the exact classes, the optional positions)
TABLE = [
    ("abc", 0, [b"a", b"b", b"c"], 0),
    ("colou?r", 0, [b"c", b"o", b"l", b"o", b"u", b"r"], _bits(4)),
    ("a{3}", 0, [b"a"] * 3, 0),
    ("a{1,3}b", 0, [b"a"] * 3 + [b"b"], _bits(1, 2)),
    ("a.{0,2}b", 0, [b"a", ALL, ALL, b"b"], _bits(1, 2)),
    ("a{0,1}b", 0, [b"a", b"b"], _bits(0)),
    ("a?b?c", 0, [b"a", b"b", b"c"], _bits(0, 1)),
    ("ab?", 0, [b"a", b"b"], _bits(1)),
    ("[a-c]{2,3}[^x]?y", 0, [b"abc"] * 3 + [_without(0x78), b"y"], _bits(2, 3)),
    (r"\?\{\*\+", 0, [b"?", b"{", b"*", b"+"], 0),
    (r"[?{*+]{2}", 0, [b"*+?{"] * 2, 0),
    (r"\x41{2}\.?", 0, [b"A", b"A", b"."], _bits(2)),
    ("a}b", 0, [b"a", b"}", b"b"], 0),
    ("a{02,003}", 0, [b"a"] * 3, _bits(2)),
    ("x{64}", 0, [b"x"] * 64, 0),
    ("a.{0,62}b", 0, [b"a"] + [ALL] * 62 + [b"b"], _bits(*range(1, 63))),
    ("a{1,64}", 0, [b"a"] * 64, _bits(*range(1, 64))),
    ("aB?", ICASE, [b"Aa", b"Bb"], _bits(1)),
    ("ACN{1,3}GT", IUPAC, [b"A", b"C", b"ACGT", b"ACGT", b"ACGT", b"G", b"T"], _bits(3, 4)),
    ("R?y", IUPAC | ICASE, [b"AGag", b"Yy"], _bits(0)),
    (ZINC, PROSITE, [b"C"] + [ALL] * 4 + [b"C"] + [ALL] * 3 + [b"CFILMVWY"] + [ALL] * 8 + [b"H"] + [ALL] * 5 + [b"H"],
     _bits(3, 4, 22, 23)),
    ("A-x-{PG}(2)-[ST](0,1)-B.", PROSITE, [b"A", ALL, _without(0x50, 0x47), _without(0x50, 0x47), b"ST", b"B"], _bits(4)),
    ("a-[bc]-{d}", PROSITE | ICASE, [b"Aa", b"BCbc", _without(0x44, 0x64)], 0),
    ("X-x(2)", PROSITE, [b"X", ALL, ALL], 0),
    ("?-*(1,2)-+", PROSITE, [b"?", b"*", b"*", b"+"], _bits(2)),
    ("[a-c]", PROSITE, [b"-ac"], 0),
]
ERRORS = [
    ("", 0), ("a*", 0), ("a+", 0), ("*", 0), ("a{2,}", 0), ("?a", 0), ("{2}a", 0), ("a??", 0), ("a{2}?", 0), ("a?{2}", 0),
    ("a{2}{3}", 0), ("a{0}", 0), ("a{0,0}", 0), ("a{3,2}", 0), ("a{", 0), ("a{2", 0), ("a{2,3", 0), ("a{,3}", 0), ("a{}", 0),
    ("a{ 2}", 0), ("a{2,3,4}", 0), ("a{-1}", 0), (r"a{\x32}", 0), ("a{65}", 0), ("a{33}b{32}", 0), ("a{1,65}", 0), ("x" * 65, 0),
    ("a?", 0), ("a?b{0,3}", 0), (".{0,64}", 0), ("[abc", 0), ("[c-a]", 0), ("a\\", 0), (r"\x4", 0), ("a{99999999999999999999}", 0),
    ("", PROSITE), (".", PROSITE), ("-", PROSITE), ("A-", PROSITE), ("-A", PROSITE), ("A--B", PROSITE), ("AB", PROSITE),
    ("<A-x", PROSITE), ("A-x>", PROSITE), ("A-[B>]", PROSITE), ("A-[]", PROSITE), ("A-{}", PROSITE), ("A-[BC", PROSITE),
    ("A-x(0)", PROSITE), ("A-x(2,1)", PROSITE), ("A-x(2,)", PROSITE), ("A-x(2", PROSITE), ("A-x()", PROSITE), ("A(2)(3)", PROSITE),
    ("x(0,3)", PROSITE), ("A(1,3", PROSITE), ("A-x(65)", PROSITE), ("A..", PROSITE), ("A-)", PROSITE), ("A,B", PROSITE),
    ("A-x", PROSITE | IUPAC), ("abc", 8), ("A-x", PROSITE | 16), ("abc", 1 << 31),
]


def _compile_raw(expr, flags):
    """(rc, classes, optional, m) through the C ABI, with sentinels in the outputs."""
    e = expr.encode("latin-1") if isinstance(expr, str) else bytes(expr)
    buf = np.full((64, 32), 0xA5, np.uint8)
    opt, m = C.c_uint64(0xDEAD), C.c_int32(-7)
    rc = host.lib().bmx_compile_gaps(e, len(e), flags, C.c_void_p(buf.ctypes.data), C.byref(opt), C.byref(m))
    return rc, buf, opt.value, m.value


def test_expression_table(built):
    for expr, flags, want, optional in TABLE:
        got, opt = host.compile_gaps(expr, flags)
        assert got.shape == (len(want), 32) and got.dtype == np.uint8, (expr, flags)
        assert _sets(got) == [bytes(sorted(w)) for w in want], (expr, flags)
        assert opt == optional, (expr, flags, bin(opt))
        member, opt2 = go.parse(expr, flags)
        assert np.array_equal(co.unpack(got), member) and opt2 == optional, (expr, flags)
    zinc, _ = host.compile_gaps(ZINC, PROSITE)
    assert zinc.shape[0] == 25


def test_expression_errors(built):
    for expr, flags in ERRORS:
        rc, buf, opt, m = _compile_raw(expr, flags)
        assert rc == host.ERR_ARG, (expr, flags)
        assert m == -7 and opt == 0xDEAD and (buf == 0xA5).all(), (expr, flags)  # untouched
        with pytest.raises(go.ExprError):
            go.parse(expr, flags)
    L = host.lib()
    buf = (C.c_uint8 * (64 * 32))()
    opt, m = C.c_uint64(0), C.c_int32(0)
    assert L.bmx_compile_gaps(None, 0, 0, buf, C.byref(opt), C.byref(m)) == host.ERR_ARG
    assert L.bmx_compile_gaps(b"a", 1, 0, None, C.byref(opt), C.byref(m)) == host.ERR_ARG
    assert L.bmx_compile_gaps(b"a", 1, 0, buf, None, C.byref(m)) == host.ERR_ARG
    assert L.bmx_compile_gaps(b"a", 1, 0, buf, C.byref(opt), None) == host.ERR_ARG


def test_class_expressions_compile_to_the_same_classes(built):
    """Without a quantifier the default syntax is bmx_compile_classes'."""
    for expr, flags in (("a.c", 0), ("[]a][^]]", 0), (r"[\x00-\x1f]\.", 0), ("GTGYCAGCMGCCGCGGTAA", IUPAC), ("aB1", ICASE)):
        got, opt = host.compile_gaps(expr, flags)
        assert opt == 0 and np.array_equal(got, host.compile_classes(expr, flags)), expr


def test_compiler_equals_the_python_grammar_on_random_expressions(built):
    rng = np.random.default_rng(0x6A95)
    alphabets = (np.frombuffer(b"ab]^-[\\.xN?{},0123*+\xe9", np.uint8), np.frombuffer(b"ACx-[]{}(),.<0123?\xe9", np.uint8))
    agreed = 0
    for case in range(3000):
        prosite = case % 3 == 2
        alphabet = alphabets[prosite]
        e = alphabet[rng.integers(0, alphabet.size, int(rng.integers(0, 14)))].tobytes()
        flags = (case % 4) | (PROSITE if prosite else 0)
        rc, buf, opt, m = _compile_raw(e, flags)
        try:
            member, optional = go.parse(e, flags)
        except go.ExprError:
            assert rc == host.ERR_ARG, (e, flags)
            continue
        assert rc == host.OK and m == member.shape[0] and opt == optional, (e, flags)
        assert np.array_equal(co.unpack(buf[:m]), member), (e, flags)
        agreed += 1
    assert agreed > 300, agreed


random_pattern = go.random_pattern


def test_matcher_equals_the_brute_force_on_tiny_cases():
    rng = np.random.default_rng(0x6A95B)
    non_empty = 0
    for case in range(400):
        alpha = 2 + case % 2
        symbols = np.arange(97, 97 + alpha)
        text = rng.choice(symbols, int(rng.integers(0, 25))).astype(np.uint8).tobytes()
        member, optional = random_pattern(rng, symbols)
        ends, short, long_ = go.gap_ends_brute(text, member, optional)
        assert go.gap_ends(text, member, optional).tolist() == ends, (case, text, optional)
        e1, s1 = go.gap_starts(text, member, optional)
        e2, s2 = go.gap_starts(text, member, optional, longest=True)
        assert e1.tolist() == ends and s1.tolist() == short, (case, text, optional)
        assert e2.tolist() == ends and s2.tolist() == long_, (case, text, optional)
        assert go.variant_ends(text, member, optional).tolist() == ends, (case, text, optional)
        non_empty += bool(ends)
    assert 3 * non_empty >= 400, non_empty


def test_word_recurrence_equals_the_matcher():
    """The three lines of csrc/bmx_gaps_kernel.h with O, I, F, S as defined there, in 32- and 64-bit words shifted up."""
    rng = np.random.default_rng(0x6A95C)
    symbols = np.arange(97, 100)
    for case in range(600):
        max_m = (7, 32, 64)[case % 3]
        member, optional = random_pattern(rng, symbols, max_m)
        m = len(member)
        text = rng.choice(symbols, int(rng.integers(0, 120))).astype(np.uint8).tobytes()
        want = go.gap_ends(text, member, optional).tolist()
        if m <= 32:
            assert go.word_ends(text, member, optional, 32).tolist() == want, (case, optional)
        assert go.word_ends(text, member, optional, 64).tolist() == want, (case, optional)


def test_mask_words_of_the_header_example():
    # positions: 0 opt, 1 opt, 2 mandatory, 3 opt, 4 mandatory, 5 opt (block at 0, one-position blocks, a block at the top)
    O, I, F, S = go.masks(_bits(0, 1, 3, 5), 6, 6)
    assert (O, I, F, S) == (0b101011, 0b010101, 0b101010, 0b000111)
    assert go.masks(_bits(0, 1, 3, 5), 6, 32) == tuple(x << 26 for x in (O, I, F, S))


def test_no_optional_position_is_the_class_search():
    rng = np.random.default_rng(0x6A95D)
    for case in range(100):
        symbols = np.arange(97, 97 + 2 + case % 3)
        member, _ = random_pattern(rng, symbols)
        text = rng.choice(symbols, int(rng.integers(0, 200))).astype(np.uint8).tobytes()
        want = (co.class_starts(text, member) + (len(member) - 1)).tolist()
        assert go.gap_ends(text, member, 0).tolist() == want
        assert go.word_ends(text, member, 0, 32).tolist() == want


def test_zinc_finger_has_nine_variants_and_matches_its_instances(built):
    classes, optional = host.compile_gaps(ZINC, PROSITE)
    member = co.unpack(classes)
    vs = go.variants(member, optional)
    assert sorted(len(v) for v in vs) == [21, 22, 22, 23, 23, 23, 24, 24, 25]
    text = b"AACAACAAALAAAAAAAAHAAAHAAC" + b"AAAACAAAACAAAIAAAAAAAAHAAAAAHAA"
    assert go.gap_ends(text, member, optional).tolist() == [22, 26 + 28]
    assert go.gap_starts(text, member, optional)[1].tolist() == [2, 26 + 4]


def test_library_exports_gaps_symbols(built):
    L = C.CDLL(host.LIB_PATH)
    X = C.CDLL(host.EXP_LIB_PATH)
    for name in ("bmx_compile_gaps", "bmx_search_gaps_device", "bmx_search_gaps", "bmx_last_gaps_ms", "bmx_gaps_starts_device"):
        assert hasattr(L, name) and hasattr(X, name), name
        assert name in [s for s, _, _ in host.SYMBOLS]
    for name in ("compile_gaps", "search_gaps", "GAPS_PROSITE", "GAPS_LONGEST", "MAX_GAPS_PATTERN"):
        assert getattr(pkg, name) is getattr(host, name)
    for name in ("search_gaps_device", "search_gaps", "gaps_starts_device", "last_gaps_ms"):
        assert callable(getattr(host.Context, name))


def test_header_constants():
    src = open(os.path.join(ROOT, "include", "bmx.h")).read()

    def define(name):
        return int(re.search(rf"#define {name} (\d+)", src).group(1))

    assert define("BMX_MAX_GAPS_PATTERN") == host.MAX_GAPS_PATTERN == go.MAX_M == 64
    assert define("BMX_GAPS_PROSITE") == host.GAPS_PROSITE == go.PROSITE == 4
    assert define("BMX_GAPS_LONGEST") == host.GAPS_LONGEST == 1
    assert host.GAPS_PROSITE & (host.CLASS_ICASE | host.CLASS_IUPAC) == 0
    assert define("BMX_MAX_CLASS_PATTERN") == 64 and define("BMX_CLASS_ICASE") == 1 and define("BMX_CLASS_IUPAC") == 2  # unchanged


def test_argument_errors_before_any_device_call(built):
    L = host.lib()
    text = b"some text to search in"
    out = (C.c_uint64 * 8)()
    total = C.c_uint64(0)
    cls = co.pack(co.singletons(b"x" * 64))
    p = C.c_void_p(cls.ctypes.data)

    def call(c, m, optional=0, cap=8, o=out, t=text, n=len(text)):
        return L.bmx_search_gaps(None, t, n, c, m, optional, o, cap, C.byref(total))

    assert call(p, 0) == host.ERR_ARG
    assert call(p, 65) == host.ERR_ARG
    assert call(p, -1) == host.ERR_ARG
    assert call(None, 4) == host.ERR_ARG
    assert call(p, 4, optional=0b1111) == host.ERR_ARG  # no mandatory position: it would match the empty string
    assert call(p, 4, optional=0b10000) == host.ERR_ARG  # an optional position outside the pattern
    assert call(p, 64, optional=(1 << 64) - 1) == host.ERR_ARG
    assert call(p, 4, o=None) == host.ERR_ARG  # a capacity needs somewhere to put the ends
    assert call(p, 4, t=None) == host.ERR_ARG
    assert call(p, 4, n=1 << 40) == host.ERR_ARG
    dev = L.bmx_search_gaps_device
    assert dev(None, None, 10, 0, 0, p, 0, 0, None, 0, C.byref(total), None) == host.ERR_ARG
    assert dev(None, None, 10, 0, 0, p, 65, 0, None, 0, C.byref(total), None) == host.ERR_ARG
    assert dev(None, None, 10, 0, 0, None, 4, 0, None, 0, C.byref(total), None) == host.ERR_ARG
    assert dev(None, None, 10, 0, 0, p, 4, 0b1111, None, 0, C.byref(total), None) == host.ERR_ARG
    assert dev(None, None, 10, 0, 0, p, 4, 0b10001, None, 0, C.byref(total), None) == host.ERR_ARG
    assert dev(None, None, 10, 11, 0, p, 4, 1, None, 0, C.byref(total), None) == host.ERR_ARG  # lead > n
    assert dev(None, None, 1 << 40, 0, 0, p, 4, 1, None, 0, C.byref(total), None) == host.ERR_ARG
    assert dev(None, None, 10, 0, 0, p, 4, 1, None, 8, C.byref(total), None) == host.ERR_ARG  # capacity, no ends
    assert dev(None, None, 10, 0, 0, p, 4, 1, None, 0, C.byref(total), None) == host.ERR_ARG  # no context
    st = L.bmx_gaps_starts_device
    assert st(None, None, 10, 0, p, 0, 0, out, 8, 0, out, None) == host.ERR_ARG
    assert st(None, None, 10, 0, p, 65, 0, out, 8, 0, out, None) == host.ERR_ARG
    assert st(None, None, 10, 0, None, 4, 0, out, 8, 0, out, None) == host.ERR_ARG
    assert st(None, None, 10, 0, p, 4, 0b1111, out, 8, 0, out, None) == host.ERR_ARG
    assert st(None, None, 10, 0, p, 4, 1, out, 8, 2, out, None) == host.ERR_ARG  # an unknown flag bit
    assert st(None, None, 1 << 40, 0, p, 4, 1, out, 8, 0, out, None) == host.ERR_ARG
    assert st(None, None, 10, 0, p, 4, 1, None, 8, 0, out, None) == host.ERR_ARG
    assert st(None, None, 10, 0, p, 4, 1, out, 8, 0, None, None) == host.ERR_ARG
    assert st(None, None, 10, 0, p, 4, 1, out, 8, host.GAPS_LONGEST, out, None) == host.ERR_ARG  # no context
    assert st(None, None, 10, 0, p, 4, 1, None, 0, 0, None, None) == host.OK  # count == 0: nothing to do, no context needed
    assert L.bmx_last_gaps_ms(None) < 0
    assert L.bmx_search_classes(None, text, len(text), p, 65, out, 8, C.byref(total)) == host.ERR_ARG  # unchanged
