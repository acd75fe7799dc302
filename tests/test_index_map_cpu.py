"""CPU suite for the text index's read mapping (bmx_index_map*): the oracle (tests/map_oracle.py) against brute force on
tiny texts, the properties the definition promises, the kernel's multi-word lane written out in Python against the oracle,
the planted case of the issue, the new C-ABI symbols and the argument errors that return before any HIP call.  No device
call is made here."""
import ctypes as C
import re

import numpy as np

import approx_oracle as ao
import index_oracle as io
import map_oracle as mp
import match_oracle as mo
from conftest import ROOT
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host
from test_index_match_cpu import queries_for

NAMES = ("bmx_index_map_device", "bmx_index_map", "bmx_last_index_map_candidates", "bmx_last_index_map_phases")
M64 = (1 << 64) - 1


def small_cases(count=300):
    """(alphabet name, text, queries, min_len, max_occ, k): `count` random small cases over the four alphabets."""
    rng = np.random.default_rng(0x3A9)
    names = list(io.ALPHABETS)
    for c in range(count):
        name = names[c % 4]
        text = io.random_text(rng, int(rng.integers(1, 25)), io.ALPHABETS[name])
        queries = [q[:int(rng.integers(1, 10))] for q in queries_for(rng, name, text, k=3)]  # short: brute force is O(w^3 m)
        yield name, text, queries, int(rng.integers(1, 4)), int(rng.integers(1, 5)), int(rng.integers(0, 3))


_BRUTE = {}


def brute_view(view: bytes, query: bytes):
    """(start, end, dist) inside a view by the definition itself: approx_ends_brute for D at every end, edit_distance over
    every start for the span.  (The answer depends on the window's bytes only: equal windows are computed once.)"""
    if (view, query) not in _BRUTE:
        ends, dists = ao.approx_ends_brute(view, query, len(query))
        dist = int(dists.min())
        end = int(ends[np.flatnonzero(dists == dist)[-1]])
        start = max(s for s in range(end + 2) if ao.edit_distance(query, view[s:end + 1]) == dist)
        _BRUTE[(view, query)] = (start, end, dist)
    return _BRUTE[(view, query)]


def brute_candidate(text: bytes, query: bytes, i: int, p: int, k: int):
    w0, w1 = mp.window(len(text), len(query), i, p, k)
    start, end, dist = brute_view(text[w0:w1], query)
    return None if dist > k else (w0 + start, w0 + end, dist)


def test_candidates_are_the_seeds_occurrences_in_array_order():
    for name, text, queries, min_len, max_occ, _ in small_cases(120):
        sa = io.model_order(text)
        rank = np.argsort(sa)
        seed_off, qpos, _, lo, cnt = mo.seeds(text, sa, queries, min_len, max_occ)
        for q, query in enumerate(queries):
            got = mp.seed_occurrences(text, rank, query, min_len, max_occ)
            want = [(int(qpos[s]), sa[int(lo[s]):int(lo[s]) + int(cnt[s])].tolist()) for s in range(int(seed_off[q]), int(seed_off[q + 1]))]
            assert [(i, occ.tolist()) for i, occ in got] == want, (name, text, query)


def test_oracle_equals_brute_force_and_keeps_its_properties():
    n_cand = n_hit = 0
    for name, text, queries, min_len, max_occ, k in small_cases():
        sa = io.model_order(text)
        rank = np.argsort(sa)
        bs, be, bd, cand_off, cs, ce, cd = mp.index_map(text, sa, queries, min_len, max_occ, k)
        assert cand_off[0] == 0 and cand_off[-1] == cs.size == ce.size == cd.size and np.all(np.diff(cand_off) >= 0)
        c = 0
        for q, query in enumerate(queries):
            lens = mo.matching_statistics(text, query)
            mine = []
            for i, occ in mp.seed_occurrences(text, rank, query, min_len, max_occ):
                for p in occ:
                    p, m = int(p), len(query)
                    want = brute_candidate(text, query, i, p, k)
                    w0, w1 = mp.window(len(text), m, i, p, k)
                    assert w0 <= p and p + int(lens[i]) <= w1  # the window holds the seed's occurrence
                    # dist <= m - len before the cut at k: the seed's bytes match, the rest is at worst replaced or inserted
                    full = mp.candidate(text, query, i, p, m)
                    assert full[2] <= m - int(lens[i]) and full[2] < m, (name, text, query, i, p)
                    if want is None:
                        assert cd[c] == mp.NO_HIT and cs[c] == mp.NO_POS and ce[c] == mp.NO_POS
                    else:
                        assert (int(cs[c]), int(ce[c]), int(cd[c])) == want, (name, text, query, i, p, k)
                        assert want[0] >= w0 and want[1] < w1 and want[2] <= k
                        assert ao.edit_distance(query, text[want[0]:want[1] + 1]) == want[2]
                        n_hit += 1
                    mine.append(want)
                    c += 1
            assert c == cand_off[q + 1]
            hits = [h for h in mine if h is not None]
            if hits:
                d, e = min((h[2], h[1]) for h in hits)
                assert (int(bd[q]), int(be[q])) == (d, e) and (int(bs[q]), e, d) in hits
            else:
                assert bd[q] == mp.NO_HIT and bs[q] == mp.NO_POS and be[q] == mp.NO_POS
        n_cand += c
    assert n_cand > 1000 and n_hit > 100, (n_cand, n_hit)


def test_base_offset_and_duplicate_candidates():
    text = b"xxabcdefghijxx"
    sa = io.model_order(text)
    base = (1 << 40) + 3
    # the read has two seeds, "abcde" at 0 and "ghij" at 6, both on diagonal 2: two candidates with one window and one
    # answer, and both are listed
    res = mp.index_map(text, sa, [b"abcdeQghij", b"qq"], 3, 4, 1, base_offset=base)
    bs, be, bd, cand_off, cs, ce, cd = res
    assert cand_off.tolist() == [0, 2, 2]
    assert cs.tolist() == [base + 2, base + 2] and ce.tolist() == [base + 11, base + 11] and cd.tolist() == [1, 1]
    assert (int(bs[0]), int(be[0]), int(bd[0])) == (base + 2, base + 11, 1)
    assert bs[1] == mp.NO_POS and be[1] == mp.NO_POS and bd[1] == mp.NO_HIT


# ---- the lane of index_map_verify_kernel / index_map_start_kernel, step for step (csrc/bmx_index_map_kernel.h) ----------

def column(pv, mv, score, peq, c, hp, lw, hb):
    """map_column: one text byte through W 64-bit words, the horizontal delta carried from word to word."""
    hm = 0
    for b in range(len(pv)):
        eq = peq[b].get(c, 0)
        xv = eq | mv[b]
        eq |= hm
        xh = ((((eq & pv[b]) + pv[b]) & M64) ^ pv[b]) | eq
        ph = (mv[b] | ~(xh | pv[b])) & M64
        mh = pv[b] & xh
        if b == lw:
            score += ((ph >> hb) & 1) - ((mh >> hb) & 1)
        op, om = ph >> 63, mh >> 63
        ph = ((ph << 1) | hp) & M64
        mh = ((mh << 1) | hm) & M64
        pv[b] = (mh | ~(xv | ph)) & M64
        mv[b] = ph & xv
        hp, hm = op, om
    return score


def lane(text: bytes, query: bytes, i: int, p: int, k: int, W: int):
    """(start, end, dist) or None as the two kernels compute it for one candidate, with W words (64 W >= m)."""
    m, n = len(query), len(text)
    assert m <= 64 * W
    w0, w1 = mp.window(n, m, i, p, k)
    lw, hb = (m - 1) >> 6, (m - 1) & 63

    def peq_of(q):
        t = [dict() for _ in range(W)]
        for x, c in enumerate(q):
            t[x >> 6][c] = t[x >> 6].get(c, 0) | (1 << (x & 63))
        return t

    peq = peq_of(query)
    pv, mv, score, best, end = [M64] * W, [0] * W, m, 1 << 30, 0
    for pos in range(w0, w1):
        score = column(pv, mv, score, peq, text[pos], 0, lw, hb)
        if score <= best:
            best, end = score, pos
    if best > k:
        return None
    peq = peq_of(query[::-1])
    pv, mv, score, best2, best_len = [M64] * W, [0] * W, m, 1 << 30, 0
    for ln in range(1, min(end - w0 + 1, m + k) + 1):
        score = column(pv, mv, score, peq, text[end - ln + 1], 1, lw, hb)
        if score < best2:
            best2, best_len = score, ln
    assert best2 == best
    return end - best_len + 1, end, best


def test_the_multi_word_lane_equals_the_oracle():
    rng = np.random.default_rng(0x18)
    letters = b"abcd"
    text = bytes(letters[int(x)] for x in rng.integers(0, 4, 900))
    checked = 0
    for m in (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512):
        for k in (0, 1, 4, 64):
            for trial in range(2):
                at = int(rng.integers(0, len(text) - m + 1)) if trial else (0 if m % 2 else len(text) - m)
                read, _, _ = mp.edit_reads(rng, text[at:at + m], 1, m, min(k, 5), letters)
                read = read[0][:host.MAX_PATTERN]
                i = int(rng.integers(0, len(read)))
                p = min(max(at + i + int(rng.integers(-2, 3)), 0), len(text) - 1)
                W = next(w for w in (1, 2, 4, 8) if 64 * w >= len(read))
                want = mp.candidate(text, read, i, p, k)
                assert lane(text, read, i, p, k, W) == want, (m, k, at, i, p)
                assert lane(text, read, i, p, k, 8) == want  # upper words only compute
                checked += 1
    assert checked == 128


def planted_case():
    rng = np.random.default_rng(0x9A7)
    letters = bytes(range(97, 123))
    text = bytes(letters[int(x)] for x in rng.integers(0, 26, 20_000))
    reads, starts, edits = mp.edit_reads(rng, text, 48, 150, 4, letters, at_ends=4)
    return text, reads, starts, edits


PLANTED = dict(min_len=20, max_occ=8, k=4)


def check_planted(bs, bd, starts, edits, k):
    mapped = 0
    for q in range(len(starts)):
        if int(bd[q]) != mp.NO_HIT:
            assert abs(int(bs[q]) - starts[q]) <= k and int(bd[q]) <= edits[q], (q, int(bs[q]), starts[q], int(bd[q]), edits[q])
            mapped += 1
    return mapped


def test_planted_reads_all_map():
    text, reads, starts, edits = planted_case()
    assert sorted(starts[:4]) == [0, 0, len(text) - 150, len(text) - 150]
    bs, be, bd, *_ = mp.index_map(text, mp.lower_case_order(text), reads, **PLANTED)
    assert check_planted(bs, bd, starts, edits, PLANTED["k"]) == 48


def test_lower_case_order_is_the_model_order():
    rng = np.random.default_rng(5)
    for n in (1, 2, 9, 40):
        t = bytes(rng.integers(97, 100, n).astype(np.uint8))
        assert np.array_equal(mp.lower_case_order(t, prefix=64), io.model_order(t))


def test_library_exports_map_symbols_and_constants(built):
    L = C.CDLL(host.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in [s for s, _, _ in host.SYMBOLS]
    assert callable(host.Index.map) and callable(host.Context.index_map) and callable(host.index_map)
    import parallel_implementation_of_string_matching_algorithms_opencl_amd as pkg

    assert pkg.index_map is host.index_map
    header = open(f"{ROOT}/include/bmx.h").read()
    define = lambda name: re.search(rf"#define {name} (.+)", header).group(1).strip()
    assert int(define("BMX_MAP_MAX_K")) == host.MAP_MAX_K == 64
    assert define("BMX_MAP_NO_HIT") == "255u" and host.MAP_NO_HIT == mp.NO_HIT == 255
    assert define("BMX_MAP_NO_POS") == "UINT64_MAX" and host.MAP_NO_POS == mp.NO_POS == (1 << 64) - 1
    assert define("BMX_MAP_MAX_CANDIDATES") == "(1ull << 27)" and host.MAP_MAX_CANDIDATES == 1 << 27


def test_argument_errors_before_any_device_call(built):
    L = host.lib()
    text = np.frombuffer(b"abracadabra", np.uint8).copy()
    blob = np.frombuffer(b"abracad", np.uint8).copy()
    off = np.array([0, 4, 7], np.uint64)
    o64 = np.full(8, 77, np.uint64)
    o8 = np.full(8, 77, np.uint8)
    total = C.c_uint64(77)
    fake = C.c_void_p(text.ctypes.data)  # stands where a device pointer or an index would: never dereferenced
    p = lambda x: None if x is None else C.c_void_p(x.ctypes.data)

    def dev(ctx=None, ix=None, pat=blob, po=off, count=2, min_len=1, max_occ=1, k=1, bs=o64, be=o64, bd=o8, co=o64, cs=o64,
            ce=o64, cd=o8, cap=4):
        return L.bmx_index_map_device(ctx, ix, p(pat), 7, p(po), count, min_len, max_occ, k, 0, p(bs), p(be), p(bd), p(co), p(cs),
                                      p(ce), p(cd), cap, C.byref(total), None)

    def hst(t=text, n=11, pat=blob, nbytes=7, po=off, count=2, min_len=1, max_occ=1, k=1, bs=o64, be=o64, bd=o8, co=o64, cs=o64,
            ce=o64, cd=o8, cap=4):
        return L.bmx_index_map(None, p(t), n, p(pat), nbytes, p(po), count, min_len, max_occ, k, p(bs), p(be), p(bd), p(co), p(cs),
                               p(ce), p(cd), cap, C.byref(total))

    for fn in (dev, hst):
        assert fn(max_occ=0) == host.ERR_ARG
        assert fn(min_len=0) == host.ERR_ARG
        assert fn(k=host.MAP_MAX_K + 1) == host.ERR_ARG
        assert fn(k=-1) == host.ERR_ARG
        assert fn(max_occ=0, count=0) == host.ERR_ARG and fn(k=65, count=0) == host.ERR_ARG
        for name in ("pat", "po", "bs", "be", "bd"):
            assert fn(**{name: None}) == host.ERR_ARG, name  # NULL where count > 0
        for name in ("cs", "ce", "cd"):
            assert fn(**{name: None}) == host.ERR_ARG, name  # a capacity needs room
        total.value = 77
        assert fn(count=0) == host.OK and total.value == 0  # nothing to do, nothing launched
        assert fn(count=0, pat=None, po=None, bs=None, be=None, bd=None, cs=None, ce=None, cd=None, co=None) == host.OK
    assert dev() == host.ERR_ARG  # no context, no index
    assert dev(ctx=fake) == host.ERR_ARG  # no index
    assert dev(cs=None, ce=None, cd=None, co=None, cap=0) == host.ERR_ARG  # a valid call but for the missing context
    assert hst(t=None) == host.ERR_ARG and hst(n=0) == host.ERR_ARG and hst(n=1 << 31) == host.ERR_ARG
    # the host entry checks offsets, lengths and bytes on the host
    assert hst(po=np.array([4, 0, 7], np.uint64)) == host.ERR_ARG
    assert hst(po=np.array([0, 4, 8], np.uint64)) == host.ERR_ARG
    assert hst(po=np.array([0, 4, 4], np.uint64)) == host.ERR_ARG
    long_blob = np.full(host.MAX_PATTERN + 1, ord("a"), np.uint8)
    assert hst(pat=long_blob, nbytes=long_blob.size, po=np.array([0, long_blob.size], np.uint64), count=1) == host.ERR_ARG
    high = np.frombuffer(b"ab\x80c", np.uint8).copy()
    assert hst(pat=high, nbytes=4, po=np.array([0, 4], np.uint64), count=1) == host.ERR_DOMAIN
    assert np.all(o64 == 77) and np.all(o8 == 77)
    assert L.bmx_last_index_map_candidates(None) < 0
    assert L.bmx_last_index_map_phases(None, (C.c_float * 5)()) == host.ERR_ARG
