"""CPU suite for the dictionary search (bmx_dict_*): the test oracle against the port's per-pattern scan and against the
known answer, the new C-ABI symbols and constants, and the argument errors that return before any HIP call.  No
compute call is made on a device here."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT, golden_file_bytes
from dict_oracle import dict_matches, dict_matches_brute
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host


def _merged_port(port, text: bytes, pats):
    ps, ids = [], []
    for i, p in enumerate(pats):
        got = port.search(np.frombuffer(text, np.uint8), p).astype(np.int64) if len(p) <= len(text) else np.zeros(0, np.int64)
        ps.append(got)
        ids.append(np.full(got.size, i, np.int64))
    pos = np.concatenate(ps) if ps else np.zeros(0, np.int64)
    idx = np.concatenate(ids) if ids else np.zeros(0, np.int64)
    order = np.lexsort((idx, pos))
    return pos[order], idx[order]


def test_oracle_matches_port_per_pattern(port):
    rng = np.random.default_rng(0xD1C7)
    for case in range(300):
        alpha = int(rng.integers(1, 5))
        n = int(rng.integers(0, 200))
        text = (rng.integers(0, alpha, n) + 97).astype(np.uint8).tobytes()
        K = int(rng.integers(1, 12))
        pats = []
        for _ in range(K):
            if n > 2 and rng.integers(0, 2):  # a piece of the text: it occurs
                a = int(rng.integers(0, n - 1))
                pats.append(text[a:a + int(rng.integers(1, 12))])
            else:
                pats.append((rng.integers(0, alpha, int(rng.integers(1, 12))) + 97).astype(np.uint8).tobytes())
        if K > 2:
            pats.append(pats[0])  # a duplicate under another index
        p1, i1 = dict_matches(text, pats)
        p2, i2 = _merged_port(port, text, pats)
        assert np.array_equal(p1, p2) and np.array_equal(i1, i2), (case, text, pats)
        if case < 60:
            p3, i3 = dict_matches_brute(text, pats)
            assert np.array_equal(p1, p3) and np.array_equal(i1, i3), (case, text, pats)


def test_oracle_shard_window():
    text = b"abcabcabc"
    p, i = dict_matches(text, [b"abc", b"c"], n_own=5)
    assert p.tolist() == [0, 2, 3] and i.tolist() == [0, 1, 0]


def test_oracle_known_answer():
    text = golden_file_bytes("input5L.txt.gz")
    pos, pid = dict_matches(text, [b"occurrences"])
    assert pos.size == 1098 and int(pos[0]) == 37 and int(pos[-1]) == 499667 and int(pid.max()) == 0
    # the approximate search at k = 0 reports the ends of the same windows: 47 .. 499,677
    assert int(pos[0]) + 10 == 47 and int(pos[-1]) + 10 == 499677


def test_library_exports_dict_symbols(built):
    L = C.CDLL(host.LIB_PATH)
    names = ("bmx_dict_create", "bmx_dict_destroy", "bmx_dict_search_device", "bmx_dict_search", "bmx_last_dict_ms",
             "bmx_last_dict_candidates")
    for name in names:
        assert hasattr(L, name), name
        assert name in [s for s, _, _ in host.SYMBOLS]
    E = C.CDLL(host.EXP_LIB_PATH)
    for name in names:
        assert hasattr(E, name), name


def test_max_dict_constant():
    src = open(os.path.join(ROOT, "include", "bmx.h")).read()
    assert int(re.search(r"#define BMX_MAX_DICT (\d+)", src).group(1)) == host.MAX_DICT == 65536


def _arrays(pats, ms=None):
    arr = (C.c_char_p * max(len(pats), 1))(*pats)
    m = (C.c_int32 * max(len(pats), 1))(*(ms if ms is not None else [len(p) for p in pats]))
    return arr, m


def test_argument_errors_before_any_device_call(built):
    L = host.lib()
    text = b"some text to search in"
    pos = (C.c_uint64 * 8)()
    pid = (C.c_uint32 * 8)()
    total = C.c_uint64(0)

    def call(pats, ms=None, K=None, cap=8, p=pos):
        arr, m = _arrays(pats, ms)
        return L.bmx_dict_search(None, text, len(text), arr, m, len(pats) if K is None else K, p, pid, cap,
                                 C.byref(total))

    assert call([b"text"], K=0) == host.ERR_ARG
    assert call([b"text"] * 65537) == host.ERR_ARG
    assert call([b"text"], K=65537) == host.ERR_ARG
    assert call([b"text", b""], ms=[4, 0]) == host.ERR_ARG
    assert call([b"x" * 513]) == host.ERR_ARG
    assert call([b"text", b"t\x80xt"]) == host.ERR_DOMAIN
    assert call([b"text", b"\xff"]) == host.ERR_DOMAIN
    assert call([b"text", None], ms=[4, 3]) == host.ERR_ARG  # a NULL pattern
    assert call([b"text"], cap=8, p=None) == host.ERR_ARG  # a capacity needs somewhere to put the positions
    arr, m = _arrays([b"text"])
    assert L.bmx_dict_search(None, text, len(text), None, m, 1, pos, pid, 8, C.byref(total)) == host.ERR_ARG
    assert L.bmx_dict_search(None, text, len(text), arr, None, 1, pos, pid, 8, C.byref(total)) == host.ERR_ARG
    assert L.bmx_dict_search(None, None, 10, arr, m, 1, pos, pid, 8, C.byref(total)) == host.ERR_ARG
    d = C.c_void_p()
    assert L.bmx_dict_create(None, arr, m, 1, C.byref(d)) == host.ERR_ARG  # no context
    assert L.bmx_dict_create(None, arr, m, 0, C.byref(d)) == host.ERR_ARG
    bad, mb = _arrays([b"\x80"])
    assert L.bmx_dict_create(None, bad, mb, 1, C.byref(d)) == host.ERR_DOMAIN
    assert L.bmx_dict_create(None, None, m, 1, C.byref(d)) == host.ERR_ARG
    dev = L.bmx_dict_search_device
    assert dev(None, None, None, 10, 10, 0, None, None, 0, C.byref(total), None) == host.ERR_ARG
    assert not d.value
    assert L.bmx_last_dict_ms(None) < 0 and L.bmx_last_dict_candidates(None) < 0
    L.bmx_dict_destroy(None)  # a no-op
