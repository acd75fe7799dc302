"""CPU suite for the approximate search (bmx_search_approx*): the test oracle against the definition and against the
known answers, the new C-ABI symbols and constants, and the argument errors that return before any HIP call.  No
compute call is made on a device here."""
import ctypes as C
import os
import re

import numpy as np

from approx_oracle import approx_ends, approx_ends_brute
from conftest import ROOT, golden_file_bytes
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

# (text, pattern, k) -> hits, first ends (dist), last end, count per distance -- see also tests/test_gpu_approx.py
KNOWN = [
    ("small", b"abcd", 1, 5, [(4, 1), (5, 0), (6, 1), (11, 1), (16, 1)], 16, [1, 4]),
    ("input5L", b"occurrences", 0, 1098, [(47, 0), (312, 0), (601, 0)], 499677, [1098]),
    ("input5L", b"occurrences", 1, 3765, [(46, 1), (47, 0), (48, 1)], 499678, [1098, 2667]),
    ("input5L", b"occurrences", 2, 6275, [(45, 2), (46, 1), (47, 0)], 499679, [1098, 2667, 2510]),
    ("input5L", b"is", 1, 73991, [(9, 1), (10, 1), (30, 1)], 499964, [3291, 70700]),
]
SMALL_TEXT = b"xxabcdxxabxdxxacdxx"


def known_text(name: str) -> bytes:
    return SMALL_TEXT if name == "small" else golden_file_bytes("input5L.txt.gz")


def test_oracle_matches_brute_force():
    rng = np.random.default_rng(0xA770)
    for case in range(400):
        alpha = int(rng.integers(1, 5))
        n = int(rng.integers(0, 31))
        m = int(rng.integers(1, 8))
        k = int(rng.integers(0, m))
        text = (rng.integers(0, alpha, n) + 97).astype(np.uint8).tobytes()
        pat = (rng.integers(0, alpha, m) + 97).astype(np.uint8).tobytes()
        e1, d1 = approx_ends(text, pat, k)
        e2, d2 = approx_ends_brute(text, pat, k)
        assert np.array_equal(e1, e2) and np.array_equal(d1, d2), (case, text, pat, k)


def test_oracle_known_answers():
    assert len(golden_file_bytes("input5L.txt.gz")) == 500007
    for name, pat, k, hits, first, last, per_dist in KNOWN:
        ends, dists = approx_ends(known_text(name), pat, k)
        assert ends.size == hits, (name, pat, k)
        assert [(int(e), int(d)) for e, d in zip(ends[:len(first)], dists[:len(first)])] == first
        assert int(ends[-1]) == last
        assert np.bincount(dists, minlength=k + 1).tolist() == per_dist


def test_k0_is_exact_search_shifted(port):
    text = golden_file_bytes("input5L.txt.gz")
    starts = port.search(np.frombuffer(text, np.uint8), b"occurrences")
    ends, _ = approx_ends(text, b"occurrences", 0)
    assert starts.size == 1098 and int(starts[0]) == 37
    assert np.array_equal(ends, starts.astype(np.int64) + 10)


def test_library_exports_approx_symbols(built):
    L = C.CDLL(host.LIB_PATH)
    for name in ("bmx_search_approx_device", "bmx_search_approx", "bmx_last_approx_ms"):
        assert hasattr(L, name), name
        assert name in [s for s, _, _ in host.SYMBOLS]


def test_max_approx_pattern_constant():
    src = open(os.path.join(ROOT, "include", "bmx.h")).read()
    assert int(re.search(r"#define BMX_MAX_APPROX_PATTERN (\d+)", src).group(1)) == host.MAX_APPROX_PATTERN == 64


def test_argument_errors_before_any_device_call(built):
    L = host.lib()
    text = b"some text to search in"
    ends = (C.c_uint64 * 8)()
    dist = (C.c_uint8 * 8)()
    total = C.c_uint64(0)

    def call(pat, m, k, cap=8, e=ends):
        return L.bmx_search_approx(None, text, len(text), pat, m, k, e, dist, cap, C.byref(total))

    assert call(b"", 0, 0) == host.ERR_ARG
    assert call(b"x" * 65, 65, 1) == host.ERR_ARG
    assert call(b"text", 4, -1) == host.ERR_ARG
    assert call(b"text", 4, 4) == host.ERR_ARG
    assert call(None, 4, 1) == host.ERR_ARG
    assert call(b"text", 4, 1, cap=8, e=None) == host.ERR_ARG  # a capacity needs somewhere to put the ends
    dev = L.bmx_search_approx_device
    assert dev(None, None, 10, 11, 0, b"text", 4, 1, None, None, 0, C.byref(total), None) == host.ERR_ARG  # lead > n
    assert dev(None, None, 10, 0, 0, b"text", 4, 4, None, None, 0, C.byref(total), None) == host.ERR_ARG
    assert dev(None, None, 10, 0, 0, b"text", 4, 1, None, None, 0, C.byref(total), None) == host.ERR_ARG  # no context
    assert L.bmx_last_approx_ms(None) < 0
