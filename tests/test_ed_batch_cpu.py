"""CPU suite for the batched edit distance (bmx_edit_distance_batch*): the case generators and their expected values
against the properties of the distance (and against the reference build where it is present), the new C-ABI symbols and
constants, and the argument errors that return before any HIP call.  No compute call is made on a device here."""
import ctypes as C
import os
import re

import numpy as np

import ed_batch_cases as cases
from conftest import ROOT
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

NAMES = ("bmx_edit_distance_batch_device", "bmx_edit_distance_batch", "bmx_last_ed_batch_ms", "bmx_last_ed_batch_fallbacks")


def check_properties(port, a, b, sample):
    for i in sample:
        x, y = a[i], b[i]
        d = port.edit_distance(x, y)
        assert d == port.edit_distance(y, x), i  # symmetric
        assert abs(len(x) - len(y)) <= d <= max(len(x), len(y)), i
        if x == y:
            assert d == 0
        if not set(x) & set(y):
            assert d == max(len(x), len(y)), i
        for limit in cases.LIMITS:
            got = int(cases.clamp(np.array([d], np.uint32), limit)[0])
            assert got == (d if limit is None or d <= limit else limit + 1)
            if limit is not None and abs(len(x) - len(y)) > limit:
                assert got == limit + 1  # what the kernel answers without the bytes


def test_random_pairs_are_self_consistent(port):
    a, b = cases.random_pairs()
    assert len(a) == len(b) >= 20000
    la, lb = np.array([len(x) for x in a]), np.array([len(y) for y in b])
    assert la.min() == lb.min() == 0 and la.max() == lb.max() == 80
    assert cases.n_fallback(a, b) == cases.MAX_FALLBACK_PAIRS
    for alpha, k in zip(cases.ALPHABETS, range(4)):
        assert max(len(set(x)) for x in a[k::4]) <= alpha
    assert sum(x == y for x, y in zip(a, b)) > 100  # zero edits happen
    check_properties(port, a, b, range(0, len(a), 7))
    want = cases.expected(port, a[:500], b[:500])
    assert want.dtype == np.uint32 and np.array_equal(want, cases.expected(port, b[:500], a[:500]))


def test_grid_and_long_pairs_are_self_consistent(port):
    a, b = cases.grid_pairs()
    assert len(a) == 3 * len(cases.GRID_LA) * len(cases.GRID_LB)
    assert {(len(x), len(y)) for x, y in zip(a, b)} == {(p, q) for p in cases.GRID_LA for q in cases.GRID_LB}
    assert cases.n_fallback(a, b) == 9 <= cases.MAX_FALLBACK_PAIRS
    check_properties(port, a, b, range(len(a)))
    a, b = cases.long_pairs()
    assert cases.n_fallback(a, b, host.ED_BATCH_LONG) <= cases.MAX_FALLBACK_PAIRS
    assert max(max(len(x), len(y)) for x, y in zip(a, b)) == host.ED_BATCH_LONG + 1
    want = cases.expected(port, a, b)
    for i in range(len(a)):  # the banded checker's answers against the full table where that is affordable
        if len(a[i]) * len(b[i]) < 1 << 26:
            assert want[i] == port.edit_distance(a[i], b[i]), i
        else:
            assert abs(len(a[i]) - len(b[i])) <= want[i] <= 64 + abs(len(a[i]) - len(b[i])), i


def test_one_vs_many_cases(port):
    for qlen in cases.QUERY_LENGTHS:
        q, cand = cases.one_vs_many(qlen, n=600)
        assert len(q) == qlen and len(cand) == 600 and max(len(c) for c in cand) <= 80
        assert cases.n_fallback([q] * len(cand), cand) <= cases.MAX_FALLBACK_PAIRS
        want = cases.expected(port, [q], cand)
        assert np.array_equal(want, cases.expected(port, [q] * len(cand), cand))
        check_properties(port, [q] * len(cand), cand, range(0, 600, 11))
    q, cand = cases.one_vs_many(300)
    assert cases.n_fallback([q] * len(cand), cand) == cases.MAX_FALLBACK_PAIRS // 2


def test_port_equals_reference_on_a_sample(port, reference):
    if reference is None:
        return  # the reference build is not on this machine: the port stands alone, as in the other suites
    a, b = cases.random_pairs(n=2000, seed=0x5A3)
    for x, y in list(zip(a, b))[::5]:
        assert port.edit_distance(x, y) == reference.edit_distance(x, y)
    a, b = cases.grid_pairs()
    for x, y in zip(a, b):
        if max(len(x), len(y)) <= 20000:  # editDistDP's limit
            assert port.edit_distance(x, y) == reference.edit_distance(x, y)


def test_pack_strings():
    blob, off = host.pack_strings([b"ab", "", "cde"])
    assert blob.tobytes() == b"abcde" and off.tolist() == [0, 2, 2, 5] and off.dtype == np.uint64
    blob, off = host.pack_strings([])
    assert blob.size == 0 and off.tolist() == [0]
    b2, o2 = host.pack_strings((np.frombuffer(b"xyz", np.uint8), np.array([0, 1, 3], np.uint64)))
    assert b2.tobytes() == b"xyz" and o2.tolist() == [0, 1, 3]


def test_library_exports_batch_symbols(built):
    L = C.CDLL(host.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in [s for s, _, _ in host.SYMBOLS]
    assert callable(host.edit_distance_batch) and callable(host.Context.edit_distance_batch_device)
    import parallel_implementation_of_string_matching_algorithms_opencl_amd as pkg

    assert pkg.edit_distance_batch is host.edit_distance_batch


def test_header_constants_equal_host_constants():
    src = open(os.path.join(ROOT, "include", "bmx.h")).read()
    assert int(re.search(r"#define BMX_ED_BATCH_WORD (\d+)", src).group(1)) == host.ED_BATCH_WORD == 64 == cases.BATCH_WORD
    assert int(re.search(r"#define BMX_ED_BATCH_LONG (\d+)", src).group(1)) == host.ED_BATCH_LONG
    assert int(re.search(r"#define BMX_ED_NO_LIMIT (0x[0-9A-Fa-f]+)u", src).group(1), 16) == host.ED_NO_LIMIT == 2**32 - 1


def test_argument_errors_before_any_device_call(built):
    L = host.lib()
    blob = np.frombuffer(b"kittensitting", np.uint8).copy()
    a_off = np.array([0, 6], np.uint64)
    b_off = np.array([6, 13], np.uint64)
    two_off = np.array([0, 6, 13], np.uint64)
    dist = np.zeros(4, np.uint32)
    p = lambda x: None if x is None else C.c_void_p(x.ctypes.data)

    def call(fn, a=blob, a_bytes=13, ao=a_off, a_count=1, b=blob, b_bytes=13, bo=b_off, count=1, out=dist):
        if fn is L.bmx_edit_distance_batch:
            return fn(None, p(a), a_bytes, p(ao), a_count, p(b), b_bytes, p(bo), count, host.ED_NO_LIMIT, p(out))
        return fn(None, p(a), a_bytes, p(ao), a_count, p(b), b_bytes, p(bo), count, host.ED_NO_LIMIT, p(out), None)

    for fn in (L.bmx_edit_distance_batch, L.bmx_edit_distance_batch_device):
        assert call(fn, a=None) == host.ERR_ARG
        assert call(fn, b=None) == host.ERR_ARG
        assert call(fn, ao=None) == host.ERR_ARG
        assert call(fn, bo=None) == host.ERR_ARG
        assert call(fn, out=None) == host.ERR_ARG
        assert call(fn, ao=two_off, a_count=2, bo=two_off, count=3) == host.ERR_ARG  # a_count not in {1, count}
        assert call(fn, ao=two_off, a_count=0, bo=two_off, count=2) == host.ERR_ARG
        # count == 0: OK, nothing launched, whatever the other arguments are
        assert call(fn, count=0, a_count=0) == host.OK
        assert call(fn, a=None, b=None, ao=None, bo=None, out=None, count=0, a_count=5) == host.OK
    # no context: the device entry has nothing to run on
    assert call(L.bmx_edit_distance_batch_device) == host.ERR_ARG
    # the host entry checks the offsets on the host
    host_fn = L.bmx_edit_distance_batch
    assert call(host_fn, bo=np.array([13, 6], np.uint64)) == host.ERR_ARG  # decreasing
    assert call(host_fn, ao=np.array([6, 0], np.uint64)) == host.ERR_ARG
    assert call(host_fn, bo=np.array([6, 14], np.uint64)) == host.ERR_ARG  # the last one past the blob
    assert call(host_fn, ao=np.array([0, 14], np.uint64)) == host.ERR_ARG
    assert call(host_fn, bo=np.array([0, 6, 5], np.uint64), ao=two_off, a_count=2, count=2) == host.ERR_ARG
    assert call(host_fn, b_bytes=1 << 33, bo=np.array([0, 1 << 31], np.uint64)) == host.ERR_ARG  # a string of 2^31 bytes
    assert np.all(dist == 0)
    assert L.bmx_last_ed_batch_ms(None) < 0
    assert L.bmx_last_ed_batch_fallbacks(None) < 0
