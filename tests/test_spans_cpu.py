"""CPU suite for the match spans of the approximate search (bmx_approx_spans_device and its relatives): the oracle
(tests/spans_oracle.py) against the definition by brute force, the span-length bound, the worked example of include/bmx.h,
and what the library answers without a device (argument errors, an empty list, the exported symbols)."""
import ctypes as C

import numpy as np

import classes_oracle as co
from approx_oracle import approx_ends, edit_distance
from spans_oracle import select_best, span_starts
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

EXAMPLE_TEXT, EXAMPLE_PAT, EXAMPLE_K = b"xxabcdxxabxdxxacdxx", b"abcd", 1
EXAMPLE_ALL = [(2, 4, 1), (2, 5, 0), (2, 6, 1), (8, 11, 1), (14, 16, 1)]
EXAMPLE_BEST = [(2, 5, 0), (8, 11, 1), (14, 16, 1)]


def _random_case(rng, case):
    sigma = (2, 4, 95)[case % 3]
    base = 0x20 if sigma == 95 else 0x61
    m = int(rng.integers(1, 13))
    k = int(rng.integers(0, m))
    n = int(rng.integers(0, 41))
    text = (rng.integers(0, sigma, n) + base).astype(np.uint8)
    pat = (rng.integers(0, sigma, m) + base).astype(np.uint8)
    if n > m and rng.integers(0, 2):
        at = int(rng.integers(0, n - m + 1))
        text[at:at + m] = pat
        for _ in range(int(rng.integers(0, k + 1))):
            text[int(rng.integers(at, at + m))] = base + int(rng.integers(0, sigma))
    return text.tobytes(), pat.tobytes(), k


def test_oracle_against_the_definition_and_the_length_bound():
    rng = np.random.default_rng(0x5BA45)
    seen = 0
    for case in range(400):
        text, pat, k = _random_case(rng, case)
        m = len(pat)
        ends, dist = approx_ends(text, pat, k)
        starts, d2 = span_starts(text, pat, k, ends)
        assert np.array_equal(d2, dist), (text, pat, k)
        for j, d, s in zip(ends.tolist(), dist.tolist(), starts.tolist()):
            by_start = [edit_distance(pat, text[x:j + 1]) for x in range(j + 1)]
            assert min(by_start) == d
            assert s == max(x for x in range(j + 1) if by_start[x] == d), (text, pat, k, j)
            assert m - d <= j - s + 1 <= m + d and s <= j
            seen += 1
    assert seen > 3000


def test_oracle_on_classes_against_the_definition():
    rng = np.random.default_rng(0x5BA46)
    for case in range(60):
        text, pat, k = _random_case(rng, case)
        member = co.singletons(pat)
        member[rng.integers(0, len(pat))] |= rng.integers(0, 2, 256).astype(bool)  # one position becomes a wide set
        ends, dist = co.class_approx_ends(text, member, k)
        starts, d2 = span_starts(text, member, k, ends)
        assert np.array_equal(d2, dist)
        for j, d, s in zip(ends.tolist(), dist.tolist(), starts.tolist()):
            by_start = [co.class_edit_distance(member, text[x:j + 1]) for x in range(j + 1)]
            assert s == max(x for x in range(j + 1) if by_start[x] == d)


def test_selection_rule():
    assert select_best([], [], 3).tolist() == []
    assert select_best([7], [2], 3).tolist() == [0]
    assert select_best([4, 5, 6, 11, 16], [1, 0, 1, 1, 1], 1).tolist() == [1, 3, 4]
    assert select_best([1, 2, 3, 4], [1, 2, 2, 3], 3).tolist() == [0, 2]  # a rising plateau keeps its last 2 as well
    assert select_best([1, 2, 3, 4, 5], [2, 1, 1, 1, 2], 2).tolist() == [3]  # the last end of a flat minimum
    assert select_best([1, 2, 4, 5], [0, 0, 0, 0], 0).tolist() == [1, 3]  # a gap ends a run
    assert select_best([5, 4, 3], [1, 1, 1], 1).tolist() == [0, 1, 2]  # list neighbours, taken literally: none adjacent
    # brute force over random lists
    rng = np.random.default_rng(3)
    for _ in range(200):
        k = int(rng.integers(0, 4))
        ends = np.cumsum(rng.integers(1, 3, int(rng.integers(0, 30))))
        dist = rng.integers(0, k + 1, ends.size)
        want = []
        for i in range(ends.size):
            dp = dist[i - 1] if i > 0 and ends[i - 1] == ends[i] - 1 else k + 1
            dn = dist[i + 1] if i + 1 < ends.size and ends[i + 1] == ends[i] + 1 else k + 1
            if dist[i] <= dp and dist[i] < dn:
                want.append(i)
        assert select_best(ends, dist, k).tolist() == want


def test_worked_example():
    ends, dist = approx_ends(EXAMPLE_TEXT, EXAMPLE_PAT, EXAMPLE_K)
    assert ends.tolist() == [4, 5, 6, 11, 16] and dist.tolist() == [1, 0, 1, 1, 1]
    starts, d = span_starts(EXAMPLE_TEXT, EXAMPLE_PAT, EXAMPLE_K, ends)
    assert list(zip(starts.tolist(), ends.tolist(), d.tolist())) == EXAMPLE_ALL
    keep = select_best(ends, dist, EXAMPLE_K)
    assert [EXAMPLE_ALL[i] for i in keep.tolist()] == EXAMPLE_BEST


def test_library_exports_span_symbols(built):
    L = C.CDLL(host.LIB_PATH)
    X = C.CDLL(host.EXP_LIB_PATH)
    for name in ("bmx_approx_spans_device", "bmx_approx_spans_classes_device", "bmx_search_approx_spans",
                 "bmx_search_approx_spans_classes", "bmx_last_spans_ms"):
        assert hasattr(L, name) and hasattr(X, name), name
    assert host.SPANS_BEST == 1


def test_argument_errors_without_a_device(built):
    L = host.lib()
    total = C.c_uint64(77)
    buf = np.zeros(8, np.uint64)
    p = C.c_void_p(buf.ctypes.data)  # stands for any non-NULL pointer: no call below gets as far as using it
    cls = co.pack(co.singletons(b"abcd"))
    c = C.c_void_p(cls.ctypes.data)
    for dev, pat in ((L.bmx_approx_spans_device, b"abcd"), (L.bmx_approx_spans_classes_device, c)):
        def call(n=10, pat=pat, m=4, k=1, ends=p, dist=p, count=3, flags=0, starts=p, sel_ends=p, sel_dist=p):
            return dev(None, p, n, 0, pat, m, k, ends, dist, count, flags, starts, sel_ends, sel_dist, C.byref(total), None)

        assert call(m=0) == host.ERR_ARG
        assert call(m=65) == host.ERR_ARG
        assert call(k=-1) == host.ERR_ARG
        assert call(k=4) == host.ERR_ARG
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
        total.value = 77
        assert call(count=0) == host.OK and total.value == 0
        assert call(count=0, flags=1, ends=None, dist=None, starts=None, sel_ends=None, sel_dist=None) == host.OK
        assert call(count=0, m=65) == host.ERR_ARG and call(count=0, flags=4) == host.ERR_ARG
    text = b"xxabcdxx"
    out = np.zeros(8, np.uint64)
    o = C.c_void_p(out.ctypes.data)
    for hostfn, pat in ((L.bmx_search_approx_spans, b"abcd"), (L.bmx_search_approx_spans_classes, c)):
        def hcall(t=text, pat=pat, m=4, k=1, flags=0, starts=o, ends=o, dist=o, cap=8):
            return hostfn(None, t, len(text), pat, m, k, flags, starts, ends, dist, cap, C.byref(total))

        assert hcall(m=65) == host.ERR_ARG
        assert hcall(m=0) == host.ERR_ARG
        assert hcall(k=4) == host.ERR_ARG
        assert hcall(pat=None) == host.ERR_ARG
        assert hcall(t=None) == host.ERR_ARG
        assert hcall(flags=8) == host.ERR_ARG
        assert hcall(starts=None) == host.ERR_ARG
        assert hcall(ends=None) == host.ERR_ARG
    assert L.bmx_last_spans_ms(None) < 0
