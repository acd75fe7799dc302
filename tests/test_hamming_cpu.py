"""CPU suite for the k-mismatch search (bmx_search_hamming*): the test oracle against the per-window definition, the new
C-ABI symbols and constants, and the argument errors that return before any HIP call.  No compute call is made on a
device here."""
import ctypes as C
import os
import re

import numpy as np

import classes_oracle as co
import hamming_oracle as ho
from conftest import ROOT
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host
import parallel_implementation_of_string_matching_algorithms_opencl_amd as pkg

NAMES = ("bmx_search_hamming_device", "bmx_search_hamming_classes_device", "bmx_search_hamming", "bmx_search_hamming_classes",
         "bmx_last_hamming_ms")


def test_oracle_matches_the_definition():
    rng = np.random.default_rng(0x4A3317)
    hits = 0
    for case in range(400):
        alpha = int(rng.integers(1, 5))
        n = int(rng.integers(0, 41))
        m = int(rng.integers(1, 9))
        k = int(rng.integers(0, m))
        text = (rng.integers(0, alpha, n) + 97).astype(np.uint8).tobytes()
        member = np.zeros((m, 256), dtype=bool)
        for i in range(m):
            kind = int(rng.integers(0, 6))
            if kind == 0:
                member[i] = True  # any
            elif kind > 1:  # (kind 1: an empty class)
                member[i][rng.integers(0, alpha, int(rng.integers(1, 4))) + 97] = True
        must = int(rng.integers(0, 1 << m)) if case % 3 else 0
        n_own = None if case % 4 else int(rng.integers(0, n + 3))
        s1, d1 = ho.hamming_starts(text, member, k, must, n_own)
        s2, d2 = ho.hamming_starts_brute(text, member, k, must, n_own)
        assert np.array_equal(s1, s2) and np.array_equal(d1, d2), (case, text, k, must, n_own)
        hits += s1.size
    assert hits > 1000


def test_oracle_edge_rules():
    member = co.singletons(b"abc")
    assert ho.hamming_starts(b"abcabdxbc", member, 0)[0].tolist() == co.class_starts(b"abcabdxbc", member).tolist() == [0]
    s, d = ho.hamming_starts(b"abcabdxbc", member, 1)
    assert s.tolist() == [0, 3, 6] and d.tolist() == [0, 1, 1]
    assert ho.hamming_starts(b"abcabdxbc", member, 1, must=0b100)[0].tolist() == [0, 6]  # position 2 must match
    assert ho.hamming_starts(b"abcabdxbc", member, 1, n_own=4)[0].tolist() == [0, 3]
    empty = member.copy()
    empty[1] = False  # an empty class always mismatches: it counts 1 ...
    s, d = ho.hamming_starts(b"abcabdxbc", empty, 1)
    assert s.tolist() == [0] and d.tolist() == [1]
    assert ho.hamming_starts(b"abcabdxbc", empty, 2, must=0b010)[0].size == 0  # ... or rules the window out
    assert ho.must_mask([0, 5, 63]) == (1 << 63) | 0b100001


def test_library_exports_hamming_symbols(built):
    L = C.CDLL(host.LIB_PATH)
    X = C.CDLL(host.EXP_LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name) and hasattr(X, name), name
        assert name in [s for s, _, _ in host.SYMBOLS]
    for name in ("search_hamming", "MAX_HAMMING_PATTERN", "MAX_HAMMING_K"):
        assert getattr(pkg, name) is getattr(host, name)
    for name in ("search_hamming_device", "search_hamming", "last_hamming_ms"):
        assert callable(getattr(host.Context, name))


def test_header_constants():
    src = open(os.path.join(ROOT, "include", "bmx.h")).read()

    def define(name):
        return int(re.search(rf"#define {name} (\d+)", src).group(1))

    assert define("BMX_MAX_HAMMING_PATTERN") == host.MAX_HAMMING_PATTERN == 64
    assert define("BMX_MAX_HAMMING_K") == host.MAX_HAMMING_K == 15
    assert define("BMX_MAX_CLASS_PATTERN") == 64 and define("BMX_MAX_APPROX_PATTERN") == 64  # unchanged
    for name in NAMES:
        assert re.search(rf"\b{name}\(", src), name


def test_must_argument_forms():
    assert host._must_mask(None) == 0
    assert host._must_mask(0b1010) == 0b1010
    assert host._must_mask([1, 3]) == host._must_mask(range(1, 4, 2)) == 0b1010
    assert host._must_mask(np.uint64(1 << 63)) == 1 << 63


def test_argument_errors_before_any_device_call(built):
    L = host.lib()
    text = b"some text to search in, longer than the longest pattern that is allowed here"
    out = (C.c_uint64 * 8)()
    dist = (C.c_uint8 * 8)()
    total = C.c_uint64(0)
    cls = co.pack(co.singletons(b"x" * 65))
    as_classes = C.c_void_p(cls.ctypes.data)
    as_string = b"x" * 65

    def entries(pat):
        """The host and the device entry for this kind of pattern, with one signature."""
        string = isinstance(pat, bytes) or pat is None
        h = L.bmx_search_hamming if string else L.bmx_search_hamming_classes
        d = L.bmx_search_hamming_device if string else L.bmx_search_hamming_classes_device

        def on_host(p, m, k, must=0, o=out, cap=8, t=text, n=len(text)):
            return h(None, t, n, p, m, k, must, o, dist, cap, C.byref(total))

        def on_device(p, m, k, must=0, o=None, cap=0, t=None, n=len(text)):
            return d(None, t, n, n, 0, p, m, k, must, o, None, cap, C.byref(total), None)

        return on_host, on_device

    for pat, none in ((as_string, None), (as_classes, C.c_void_p(None))):
        for call in entries(pat):
            assert call(pat, 0, 0) == host.ERR_ARG  # m of 0 and 65
            assert call(pat, 65, 1) == host.ERR_ARG
            assert call(pat, -1, 0) == host.ERR_ARG
            assert call(pat, 8, -1) == host.ERR_ARG  # k < 0, k >= m, k = 16
            assert call(pat, 8, 8) == host.ERR_ARG
            assert call(pat, 8, 9) == host.ERR_ARG
            assert call(pat, 1, 1) == host.ERR_ARG
            assert call(pat, 64, 16) == host.ERR_ARG
            assert call(pat, 20, 16) == host.ERR_ARG
            assert call(pat, 8, 2, must=1 << 8) == host.ERR_ARG  # a bit of `must` at m, or above
            assert call(pat, 8, 2, must=1 << 63) == host.ERR_ARG
            assert call(pat, 63, 2, must=1 << 63) == host.ERR_ARG
            assert call(pat, 1, 0, must=2) == host.ERR_ARG
            assert call(pat, 8, 2, o=None, cap=8) == host.ERR_ARG  # a capacity needs somewhere to put the starts
            assert call(pat, 8, 2, n=1 << 40) == host.ERR_ARG  # n >= 2^40
            assert call(none, 8, 2) == host.ERR_ARG
        on_host, on_device = entries(pat)
        assert on_host(pat, 8, 2, t=None) == host.ERR_ARG  # a text of n > 0 bytes
        # all arguments in range: the device entry then asks for its context (the host entry would open device 0)
        assert on_device(pat, 8, 2, must=0xFF) == host.ERR_ARG
        assert on_device(pat, 64, 15, must=(1 << 64) - 1) == host.ERR_ARG
        # ... and the host entry answers a text shorter than the pattern without a device
        total.value = 99
        assert on_host(pat, 8, 2, n=7) == host.OK and total.value == 0
    assert L.bmx_last_hamming_ms(None) < 0
