"""CPU suite for the approximate search with patterns of up to 512 bytes (bmx_search_approx_long*,
bmx_approx_long_spans_device, bmx_search_approx_long_spans): the constants, the symbols, and every argument error, which
returns before any HIP call (ctx = NULL on a machine without a GPU).  The old entries keep their limit of 64."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

NAMES = ("bmx_search_approx_long_device", "bmx_search_approx_long", "bmx_approx_long_spans_device",
         "bmx_search_approx_long_spans")


def _header() -> str:
    return open(os.path.join(ROOT, "include", "bmx.h")).read()


def test_constants():
    src = _header()
    assert int(re.search(r"#define BMX_MAX_APPROX_LONG_PATTERN (\d+)", src).group(1)) == host.MAX_APPROX_LONG_PATTERN == 512
    assert int(re.search(r"#define BMX_MAX_APPROX_LONG_K (\d+)", src).group(1)) == host.MAX_APPROX_LONG_K == 255
    assert int(re.search(r"#define BMX_MAX_APPROX_PATTERN (\d+)", src).group(1)) == host.MAX_APPROX_PATTERN == 64


def test_symbols_declared_and_exported(built):
    src = _header()
    L = C.CDLL(host.LIB_PATH)
    X = C.CDLL(host.EXP_LIB_PATH)
    declared = [s for s, _, _ in host.SYMBOLS]
    for name in NAMES:
        assert re.search(rf"\bint {name}\(", src), name
        assert hasattr(L, name) and hasattr(X, name), name
        assert name in declared, name


def test_search_argument_errors_before_any_device_call(built):
    L = host.lib()
    text = b"some text to search in, not that any call below gets to read it"
    ends = (C.c_uint64 * 8)()
    dist = (C.c_uint8 * 8)()
    total = C.c_uint64(0)
    p = C.c_void_p(C.addressof(ends))  # stands for any non-NULL device pointer

    def hcall(pat, m, k, cap=8, e=ends, t=text):
        return L.bmx_search_approx_long(None, t, len(text), pat, m, k, e, dist, cap, C.byref(total))

    def dcall(pat, m, k, n=1000, lead=0, cap=8, e=p, d_text=p):
        return L.bmx_search_approx_long_device(None, d_text, n, lead, 0, pat, m, k, e, None, cap, C.byref(total), None)

    for call in (hcall, dcall):
        assert call(b"", 0, 0) == host.ERR_ARG
        assert call(b"x" * 513, 513, 1) == host.ERR_ARG
        for m in (1, 4, 64, 65, 300, 512):
            assert call(b"x" * m, m, m) == host.ERR_ARG  # k = m
        assert call(b"x" * 300, 300, 256) == host.ERR_ARG  # a distance stays one byte
        assert call(b"x" * 300, 300, -1) == host.ERR_ARG
        assert call(None, 100, 1) == host.ERR_ARG
        assert call(b"x" * 100, 100, 1, cap=8, e=None) == host.ERR_ARG  # a capacity needs somewhere to put the ends
    assert dcall(b"x" * 100, 100, 1, n=10, lead=11) == host.ERR_ARG  # lead > n
    assert dcall(b"x" * 100, 100, 1, n=1 << 40) == host.ERR_ARG
    assert hcall(b"x" * 100, 100, 1, t=None) == host.ERR_ARG
    # in the domain: what is left is the missing context (device entry) -- still no device call
    for m, k in ((1, 0), (64, 63), (65, 0), (300, 255), (512, 255)):
        assert dcall(b"x" * m, m, k) == host.ERR_ARG
        assert dcall(b"x" * m, m, k, cap=0, e=None) == host.ERR_ARG
    # the old entries keep their limit
    assert L.bmx_search_approx(None, text, len(text), b"x" * 65, 65, 1, ends, dist, 8, C.byref(total)) == host.ERR_ARG


def test_spans_argument_errors_and_the_empty_list(built):
    L = host.lib()
    total = C.c_uint64(77)
    buf = np.zeros(8, np.uint64)
    p = C.c_void_p(buf.ctypes.data)  # stands for any non-NULL pointer: no call below gets as far as using it
    pat = b"y" * 300

    def call(n=1000, pat=pat, m=300, k=5, ends=p, dist=p, count=3, flags=0, starts=p, sel_ends=p, sel_dist=p):
        return L.bmx_approx_long_spans_device(None, p, n, 0, pat, m, k, ends, dist, count, flags, starts, sel_ends, sel_dist,
                                              C.byref(total), None)

    assert call(m=0) == host.ERR_ARG
    assert call(pat=b"y" * 513, m=513) == host.ERR_ARG
    assert call(k=-1) == host.ERR_ARG
    assert call(k=300) == host.ERR_ARG
    assert call(k=256) == host.ERR_ARG
    assert call(n=1 << 40) == host.ERR_ARG
    assert call(pat=None) == host.ERR_ARG
    assert call(ends=None) == host.ERR_ARG
    assert call(starts=None) == host.ERR_ARG
    assert call(flags=2) == host.ERR_ARG and call(flags=3) == host.ERR_ARG  # unknown bits
    assert call(flags=1, dist=None) == host.ERR_ARG  # the selection reads the distances
    assert call(flags=1, sel_ends=None) == host.ERR_ARG
    assert call() == host.ERR_ARG  # no context
    assert call(flags=1) == host.ERR_ARG
    # an empty list: nothing to do, nothing launched, whatever else is missing
    for m in (4, 64, 65, 512):
        total.value = 77
        assert call(count=0, pat=b"y" * m, m=m, k=3) == host.OK and total.value == 0
        assert call(count=0, pat=b"y" * m, m=m, k=3, flags=1, ends=None, dist=None, starts=None, sel_ends=None,
                    sel_dist=None) == host.OK
    assert call(count=0, pat=b"y" * 513, m=513) == host.ERR_ARG and call(count=0, flags=4) == host.ERR_ARG

    text = b"xxabcdxx" * 50
    out = np.zeros(8, np.uint64)
    o = C.c_void_p(out.ctypes.data)

    def hcall(t=text, pat=pat, m=300, k=5, flags=0, starts=o, ends=o, dist=o, cap=8):
        return L.bmx_search_approx_long_spans(None, t, len(text), pat, m, k, flags, starts, ends, dist, cap, C.byref(total))

    assert hcall(pat=b"y" * 513, m=513) == host.ERR_ARG
    assert hcall(m=0) == host.ERR_ARG
    assert hcall(k=300) == host.ERR_ARG
    assert hcall(k=256) == host.ERR_ARG
    assert hcall(pat=None) == host.ERR_ARG
    assert hcall(t=None) == host.ERR_ARG
    assert hcall(flags=8) == host.ERR_ARG
    assert hcall(starts=None) == host.ERR_ARG
    assert hcall(ends=None) == host.ERR_ARG
    # the old entries keep their limit
    assert L.bmx_approx_spans_device(None, p, 1000, 0, b"y" * 65, 65, 1, p, p, 0, 0, p, p, p, C.byref(total), None) == host.ERR_ARG
    assert L.bmx_search_approx_spans(None, text, len(text), b"y" * 65, 65, 1, 0, o, o, o, 8, C.byref(total)) == host.ERR_ARG
