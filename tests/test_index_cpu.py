"""CPU suite for the text index (bmx_index_*): the comparator the query kernels implement (tests/index_oracle.py) against
the oracle's suffix array, the interval it yields against brute force, the new C-ABI symbols, and the argument errors
that return before any HIP call.  No device call is made here.

Queries: every string of 1..5 bytes over the alphabet's bytes below 0x80 for the three small alphabets (at most 4 + 16 +
64 + 256 + 1,024 strings).  Over the 95 printable bytes that set has 7.7e9 members, so there the queries are every string
of 1..2 bytes over the bytes of the text and 95, 96, 97 (the bytes around the virtual symbol), every substring of 1..5
bytes, and every such substring with 95, 96 and 97 in place of its last byte and appended to it: the strings that reach
into a suffix's end from both sides of the virtual symbol."""
import ctypes as C

import numpy as np

import index_oracle as io
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

NAMES = ("bmx_index_create_device", "bmx_index_destroy", "bmx_index_sa", "bmx_index_count_device", "bmx_index_locate_device",
         "bmx_index_count", "bmx_index_locate", "bmx_last_index_ms", "bmx_index_build_ms")


def texts():
    """(alphabet name, text) for n = 1..64 over the four alphabets, two texts per (n, alphabet)."""
    rng = np.random.default_rng(0x1DE5)
    for name, alpha in io.ALPHABETS.items():
        for n in range(1, 65):
            for _ in range(2):
                yield name, io.random_text(rng, n, alpha)


def queries_for(name: str, text: bytes):
    if name != "printable":
        return io.all_queries(io.ALPHABETS[name], 5)
    letters = bytes(sorted(set(text) | {95, 96, 97}))
    out = set(io.all_queries(letters, 2))
    for i in range(len(text)):
        for m in range(1, 6):
            s = text[i:i + m]
            out.add(s)
            for b in (95, 96, 97):
                out.add(s[:-1] + bytes([b]))
                out.add(s + bytes([b]))
    return sorted(out)


def test_no_generated_text_ends_in_two_bytes_96():
    seen = 0
    for _, t in texts():
        assert not t.endswith(b"``")
        seen += 1
    assert seen == 4 * 64 * 2
    rng = np.random.default_rng(1)
    assert all(not io.random_text(rng, 2, b"`_").endswith(b"``") for _ in range(50))  # the rewrite happens


def test_model_order_equals_the_oracles_suffix_array(port):
    for name, t in texts():
        want = port.suffix_array(np.frombuffer(t, np.uint8))
        got = io.model_order(t)
        assert np.array_equal(got, want), (name, t, got.tolist(), want.tolist())


def test_interval_of_the_comparator_is_the_set_of_occurrences(port):
    checked = 0
    for name, t in texts():
        sa = port.suffix_array(np.frombuffer(t, np.uint8))
        keys = io.suffix_keys(t, sa)
        for q in queries_for(name, t):
            lo, cnt = io.sa_range(t, sa, q, keys)
            assert 0 <= lo <= lo + cnt <= len(t)
            got = np.sort(sa[lo:lo + cnt].astype(np.int64))
            assert np.array_equal(got, io.occurrences(t, q)), (name, t, q, lo, cnt)
            checked += 1
    assert checked > 70000


def test_hand_example():
    t = b"xA`"  # the one-byte suffix "`" carries the virtual symbol, "A`" does not, "xA`" does
    assert io.model_order(t).tolist() == [1, 2, 0]
    sa = io.model_order(t)
    assert io.sa_range(t, sa, b"`") == (1, 1) and io.sa_range(t, sa, b"A`") == (0, 1)
    assert io.sa_range(t, sa, b"A``")[1] == 0 and io.sa_range(t, sa, b"``")[1] == 0
    assert io.occurrences(b"aaaa", b"aa").tolist() == [0, 1, 2]


def test_library_exports_index_symbols(built):
    L = C.CDLL(host.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in [s for s, _, _ in host.SYMBOLS]
    assert callable(host.index_count) and callable(host.Context.index) and callable(host.Context.last_index_ms)
    for attr in ("count", "locate", "sa", "close", "__enter__", "__exit__"):
        assert hasattr(host.Index, attr), attr
    import parallel_implementation_of_string_matching_algorithms_opencl_amd as pkg

    assert pkg.index_count is host.index_count and pkg.Index is host.Index


def test_argument_errors_before_any_device_call(built):
    L = host.lib()
    text = np.frombuffer(b"abracadabra", np.uint8).copy()
    blob = np.frombuffer(b"abracad", np.uint8).copy()
    off = np.array([0, 4, 7], np.uint64)
    cnt = np.zeros(4, np.uint32)
    total = C.c_uint64(77)
    fake = C.c_void_p(text.ctypes.data)  # stands where a device pointer or an index would: never dereferenced
    p = lambda x: None if x is None else C.c_void_p(x.ctypes.data)

    # create: no context, NULL text, NULL out, n == 0, n >= 2^31
    h = C.c_void_p()
    assert L.bmx_index_create_device(None, fake, 11, None, None, C.byref(h)) == host.ERR_ARG
    assert L.bmx_index_create_device(fake, None, 11, None, None, C.byref(h)) == host.ERR_ARG
    assert L.bmx_index_create_device(fake, fake, 11, None, None, None) == host.ERR_ARG
    assert L.bmx_index_create_device(fake, fake, 0, None, None, C.byref(h)) == host.ERR_ARG
    assert L.bmx_index_create_device(fake, fake, 1 << 31, None, None, C.byref(h)) == host.ERR_ARG
    assert not h.value
    L.bmx_index_destroy(None)
    assert L.bmx_index_sa(None, C.byref(h)) == host.ERR_ARG
    assert L.bmx_index_build_ms(None) < 0 and L.bmx_last_index_ms(None) < 0

    def count_dev(ctx=None, ix=None, pat=blob, po=off, count=2, lo=None, out=cnt):
        return L.bmx_index_count_device(ctx, ix, p(pat), 7, p(po), count, p(lo), p(out), None)

    def locate_dev(ctx=None, ix=None, pat=blob, po=off, count=2, out_off=off, pos=off, cap=4):
        return L.bmx_index_locate_device(ctx, ix, p(pat), 7, p(po), count, 0, p(out_off), p(pos), cap, C.byref(total), None)

    for fn in (count_dev, locate_dev):
        assert fn(pat=None) == host.ERR_ARG
        assert fn(po=None) == host.ERR_ARG
        assert fn() == host.ERR_ARG  # no context, no index
        assert fn(ctx=fake) == host.ERR_ARG  # no index
        assert fn(count=0) == host.OK  # nothing to do, nothing launched
        assert fn(count=0, pat=None, po=None) == host.OK
    assert count_dev(out=None) == host.ERR_ARG
    assert locate_dev(out_off=None) == host.ERR_ARG
    assert locate_dev(pos=None) == host.ERR_ARG  # a capacity needs room
    assert locate_dev(count=0) == host.OK and total.value == 0

    def count_host(t=text, n=11, pat=blob, nbytes=7, po=off, count=2, out=cnt):
        return L.bmx_index_count(None, p(t), n, p(pat), nbytes, p(po), count, p(out))

    assert count_host(t=None) == host.ERR_ARG
    assert count_host(n=0) == host.ERR_ARG
    assert count_host(n=1 << 31) == host.ERR_ARG
    assert count_host(pat=None) == host.ERR_ARG
    assert count_host(po=None) == host.ERR_ARG
    assert count_host(out=None) == host.ERR_ARG
    assert count_host(count=0) == host.OK
    # the host entry checks offsets, lengths and bytes on the host
    assert count_host(po=np.array([4, 0, 7], np.uint64)) == host.ERR_ARG  # decreasing
    assert count_host(po=np.array([0, 4, 8], np.uint64)) == host.ERR_ARG  # an end past the blob
    assert count_host(po=np.array([0, 4, 4], np.uint64)) == host.ERR_ARG  # an empty query
    long_blob = np.full(host.MAX_PATTERN + 1, ord("a"), np.uint8)
    assert count_host(pat=long_blob, nbytes=long_blob.size, po=np.array([0, long_blob.size], np.uint64), count=1) == host.ERR_ARG
    high = np.frombuffer(b"ab\x80c", np.uint8).copy()
    assert count_host(pat=high, nbytes=4, po=np.array([0, 4], np.uint64), count=1) == host.ERR_DOMAIN
    assert np.all(cnt == 0)
    out_off = np.zeros(3, np.uint64)

    def locate_host(t=text, n=11, pat=blob, po=off, count=2, oo=out_off, pos=cnt, cap=2):
        return L.bmx_index_locate(None, p(t), n, p(pat), 7, p(po), count, p(oo), p(pos), cap, C.byref(total))

    assert locate_host(t=None) == host.ERR_ARG
    assert locate_host(n=0) == host.ERR_ARG
    assert locate_host(pat=None) == host.ERR_ARG
    assert locate_host(oo=None) == host.ERR_ARG
    assert locate_host(pos=None) == host.ERR_ARG
    assert locate_host(po=np.array([0, 4, 8], np.uint64)) == host.ERR_ARG
    assert locate_host(count=0) == host.OK
