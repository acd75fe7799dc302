"""CPU suite for the class-pattern search (bmx_compile_classes, bmx_search_classes*, bmx_search_approx_classes_device):
the expression compiler against a table of exact classes and against the grammar restated in Python, the test oracle
against the definitions, the new C-ABI symbols and constants, and the argument errors that return before any HIP call.
No compute call is made on a device here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import classes_oracle as co
from conftest import ROOT, golden_file_bytes
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host
import parallel_implementation_of_string_matching_algorithms_opencl_amd as pkg

ALL = bytes(range(256))
PRIMER = "GTGYCAGCMGCCGCGGTAA"


def _sets(classes):
    """The classes as a list of bytes objects (members ascending)."""
    return [bytes(np.nonzero(row)[0].astype(np.uint8)) for row in co.unpack(classes)]


def _without(*drop):
    return bytes(b for b in range(256) if b not in drop)


# (expression, flags, the exact classes)
TABLE = [
    ("a.c", 0, [b"a", ALL, b"c"]),
    ("[abc]", 0, [b"abc"]),
    ("[a-c]", 0, [b"abc"]),
    ("[^a]", 0, [_without(0x61)]),
    ("[]a]", 0, [b"]a"]),
    ("[^]]", 0, [_without(0x5D)]),
    ("[a-]x]", 0, [b"-a", b"x", b"]"]),
    (r"\.", 0, [b"."]),
    (r"\x41", 0, [b"A"]),
    (r"\[\\", 0, [b"[", b"\\"]),
    (r"[\x00-\x1f]", 0, [bytes(range(32))]),
    (r"[\]\x7f-\xff]", 0, [b"]" + bytes(range(0x7F, 0x100))]),
    (b"\x00\xff]", 0, [b"\x00", b"\xff", b"]"]),
    ("x" * 64, 0, [b"x"] * 64),
    ("aB1", host.CLASS_ICASE, [b"Aa", b"Bb", b"1"]),
    ("[a-c][^x]", host.CLASS_ICASE, [b"ABCabc", _without(0x58, 0x78)]),
    (r"\x41.", host.CLASS_ICASE, [b"Aa", ALL]),
    (PRIMER, host.CLASS_IUPAC, [b"G", b"T", b"G", b"CT", b"C", b"A", b"G", b"C", b"AC", b"G", b"C", b"C", b"G", b"C", b"G",
                                b"G", b"T", b"A", b"A"]),
    ("RYSWKMBDHVN", host.CLASS_IUPAC, [b"AG", b"CT", b"CG", b"AT", b"GT", b"AC", b"CGT", b"AGT", b"ACT", b"ACG", b"ACGT"]),
    (r"[N]\Nn", host.CLASS_IUPAC, [b"N", b"N", b"n"]),
    ("NRa", host.CLASS_IUPAC | host.CLASS_ICASE, [b"ACGTacgt", b"AGag", b"Aa"]),
]
ERRORS = ["", "[abc", "[", "[^", "[]", "[c-a]", "\\", "ab\\", r"\x4", r"\xg0", r"[\x4]", "[a-\\", "x" * 65, "." * 65]


def test_expression_table(built):
    for expr, flags, want in TABLE:
        got = host.compile_classes(expr, flags)
        assert got.shape == (len(want), 32) and got.dtype == np.uint8
        assert _sets(got) == [bytes(sorted(w)) for w in want], (expr, flags)
        assert np.array_equal(co.unpack(got), co.parse(expr, flags)), (expr, flags)


def test_expression_errors(built):
    L = host.lib()
    buf = (C.c_uint8 * (64 * 32))()
    for expr in ERRORS:
        e = expr.encode("latin-1")
        m = C.c_int32(-7)
        assert L.bmx_compile_classes(e, len(e), 0, buf, C.byref(m)) == host.ERR_ARG, expr
        assert m.value == -7  # untouched
        with pytest.raises(co.ExprError):
            co.parse(expr)
    m = C.c_int32(-7)
    assert L.bmx_compile_classes(None, 0, 0, buf, C.byref(m)) == host.ERR_ARG
    assert L.bmx_compile_classes(b"a", 1, 0, None, C.byref(m)) == host.ERR_ARG
    assert L.bmx_compile_classes(b"a", 1, 0, buf, None) == host.ERR_ARG
    assert L.bmx_compile_classes(b"a" * 64, 64, 0, buf, C.byref(m)) == host.OK and m.value == 64


def test_compiler_equals_the_python_grammar_on_random_expressions(built):
    rng = np.random.default_rng(0xC1A55)
    alphabet = np.frombuffer(b"ab]^-[\\.xN4Af\xe9\x00", np.uint8)
    L = host.lib()
    buf = np.zeros((64, 32), np.uint8)
    agreed = 0
    for case in range(3000):
        e = alphabet[rng.integers(0, alphabet.size, int(rng.integers(0, 12)))].tobytes()
        flags = case % 4
        m = C.c_int32(0)
        rc = L.bmx_compile_classes(e, len(e), flags, C.c_void_p(buf.ctypes.data), C.byref(m))
        try:
            want = co.parse(e, flags)
        except co.ExprError:
            assert rc == host.ERR_ARG, (e, flags)
            continue
        assert rc == host.OK and m.value == want.shape[0], (e, flags)
        assert np.array_equal(co.unpack(buf[:m.value]), want), (e, flags)
        agreed += 1
    assert agreed > 500


def test_oracle_matches_brute_force():
    rng = np.random.default_rng(0xC1A550)
    for case in range(400):
        alpha = int(rng.integers(1, 5))
        n = int(rng.integers(0, 31))
        m = int(rng.integers(1, 8))
        k = int(rng.integers(0, m))
        text = (rng.integers(0, alpha, n) + 97).astype(np.uint8).tobytes()
        member = np.zeros((m, 256), dtype=bool)
        for i in range(m):
            if rng.integers(0, 4) == 0:
                member[i] = True  # any
            else:
                member[i][rng.integers(0, alpha, int(rng.integers(1, 4))) + 97] = True  # 1..3 members
        assert class_starts_list(text, member) == co.class_starts_brute(text, member), (case, text)
        e1, d1 = co.class_approx_ends(text, member, k)
        e2, d2 = co.class_approx_ends_brute(text, member, k)
        assert np.array_equal(e1, e2) and np.array_equal(d1, d2), (case, text, k)


def class_starts_list(text, member):
    return co.class_starts(text, member).tolist()


def test_case_folding_equals_re_on_the_sample_text(built):
    text = golden_file_bytes("input5L.txt.gz")
    for expr, flags, rx, rflags in (("occurrences", host.CLASS_ICASE, rb"(?=occurrences)", re.I), ("[Tt]he", 0, rb"(?=[Tt]he)", 0),
                                    ("t.e", host.CLASS_ICASE, rb"(?=t.e)", re.I | re.S)):
        want = [mt.start() for mt in re.finditer(rx, text, rflags)]
        got = co.class_starts(text, co.unpack(host.compile_classes(expr, flags))).tolist()
        assert len(want) > 100 and got == want, expr


def test_singletons_and_pack_round_trip():
    member = co.singletons(b"ab\xff")
    assert np.array_equal(co.unpack(co.pack(member)), member)
    assert co.class_starts(b"xxab\xffab\xff", member).tolist() == [2, 5]
    assert co.pack(member)[2, 31] == 0x80 and co.pack(member)[0, 12] == 0x02  # bit (b & 7) of byte (b >> 3)


def test_library_exports_class_symbols(built):
    L = C.CDLL(host.LIB_PATH)
    X = C.CDLL(host.EXP_LIB_PATH)
    for name in ("bmx_compile_classes", "bmx_search_classes_device", "bmx_search_classes", "bmx_last_classes_ms",
                 "bmx_search_approx_classes_device", "bmx_search_approx_classes"):
        assert hasattr(L, name) and hasattr(X, name), name
        assert name in [s for s, _, _ in host.SYMBOLS]
    for name in ("compile_classes", "search_classes", "CLASS_ICASE", "CLASS_IUPAC", "MAX_CLASS_PATTERN"):
        assert getattr(pkg, name) is getattr(host, name)


def test_header_constants():
    src = open(os.path.join(ROOT, "include", "bmx.h")).read()

    def define(name):
        return int(re.search(rf"#define {name} (\d+)", src).group(1))

    assert define("BMX_MAX_CLASS_PATTERN") == host.MAX_CLASS_PATTERN == 64
    assert define("BMX_CLASS_BYTES") == host.CLASS_BYTES == 32
    assert define("BMX_CLASS_ICASE") == host.CLASS_ICASE == co.ICASE == 1
    assert define("BMX_CLASS_IUPAC") == host.CLASS_IUPAC == co.IUPAC == 2
    assert define("BMX_MAX_APPROX_PATTERN") == 64  # unchanged
    assert "no counterpart in the reference" in src


def test_argument_errors_before_any_device_call(built):
    L = host.lib()
    text = b"some text to search in"
    out = (C.c_uint64 * 8)()
    dist = (C.c_uint8 * 8)()
    total = C.c_uint64(0)
    cls = co.pack(co.singletons(b"x" * 65))
    p = C.c_void_p(cls.ctypes.data)

    def call(c, m, cap=8, o=out, t=text):
        return L.bmx_search_classes(None, t, len(text), c, m, o, cap, C.byref(total))

    assert call(p, 0) == host.ERR_ARG
    assert call(p, 65) == host.ERR_ARG
    assert call(p, -1) == host.ERR_ARG
    assert call(None, 4) == host.ERR_ARG
    assert call(p, 4, cap=8, o=None) == host.ERR_ARG  # a capacity needs somewhere to put the starts
    assert call(p, 4, t=None) == host.ERR_ARG
    dev = L.bmx_search_classes_device
    assert dev(None, None, 10, 10, 0, p, 0, None, 0, C.byref(total), None) == host.ERR_ARG
    assert dev(None, None, 10, 10, 0, p, 65, None, 0, C.byref(total), None) == host.ERR_ARG
    assert dev(None, None, 10, 10, 0, None, 4, None, 0, C.byref(total), None) == host.ERR_ARG
    assert dev(None, None, 1 << 40, 10, 0, p, 4, None, 0, C.byref(total), None) == host.ERR_ARG
    assert dev(None, None, 10, 10, 0, p, 4, None, 0, C.byref(total), None) == host.ERR_ARG  # no context
    adev = L.bmx_search_approx_classes_device
    assert adev(None, None, 10, 11, 0, p, 4, 1, None, None, 0, C.byref(total), None) == host.ERR_ARG  # lead > n
    assert adev(None, None, 10, 0, 0, p, 4, 4, None, None, 0, C.byref(total), None) == host.ERR_ARG  # k = m
    assert adev(None, None, 10, 0, 0, p, 65, 1, None, None, 0, C.byref(total), None) == host.ERR_ARG
    assert adev(None, None, 10, 0, 0, None, 4, 1, None, None, 0, C.byref(total), None) == host.ERR_ARG
    assert adev(None, None, 10, 0, 0, p, 4, 1, None, dist, 8, C.byref(total), None) == host.ERR_ARG  # capacity, no ends
    assert adev(None, None, 10, 0, 0, p, 4, 1, None, None, 0, C.byref(total), None) == host.ERR_ARG  # no context
    ahost = L.bmx_search_approx_classes
    assert ahost(None, text, len(text), p, 65, 1, out, dist, 8, C.byref(total)) == host.ERR_ARG
    assert ahost(None, text, len(text), p, 4, 4, out, dist, 8, C.byref(total)) == host.ERR_ARG
    assert ahost(None, text, len(text), None, 4, 1, out, dist, 8, C.byref(total)) == host.ERR_ARG
    assert ahost(None, text, len(text), p, 4, 1, None, dist, 8, C.byref(total)) == host.ERR_ARG
    assert ahost(None, None, len(text), p, 4, 1, out, dist, 8, C.byref(total)) == host.ERR_ARG
    assert L.bmx_last_classes_ms(None) < 0
    assert L.bmx_search_approx(None, text, len(text), b"x" * 65, 65, 1, out, dist, 8, C.byref(total)) == host.ERR_ARG  # unchanged
