"""CPU suite for the text index's matching statistics and seeds (bmx_index_match*, bmx_index_seeds*): the oracle
(tests/match_oracle.py) against the argument the kernel rests on, the kernel's search written out in Python against the
oracle, the properties of seeds, the new C-ABI symbols and the argument errors that return before any HIP call.  No device
call is made here.

The argument: in the builder's order (index_oracle.model_order) the longest match of a string is the larger of its common
prefixes with the two neighbours of its insertion point, and the interval of that prefix is exactly its set of
occurrences.  Texts: the 512 of tests/test_index_cpu.py's kind (1..64 bytes over the four alphabets).  Queries per text: 6
of 1..40 bytes, half of them spliced from pieces of the text, bytes >= 0x80 left out (they are no query bytes)."""
import ctypes as C

import numpy as np

import index_oracle as io
import match_oracle as mo
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host
from test_index_cpu import texts

NAMES = ("bmx_index_match_device", "bmx_index_seeds_device", "bmx_index_match", "bmx_index_seeds")


def queries_for(rng, name: str, text: bytes, k: int = 6):
    letters = bytes(b for b in io.ALPHABETS[name] if b < 0x80)
    if name == "printable":
        letters = bytes(sorted({b for b in text if b < 0x80} | {95, 96, 97}))
    out = []
    for j in range(k):
        m = int(rng.integers(1, 41))
        q = bytearray(letters[int(x)] for x in rng.integers(0, len(letters), m))
        if j % 2 == 0:  # spliced: pieces of the text over random bytes
            at = 0
            while at < m:
                ln = int(rng.integers(1, 12))
                src = int(rng.integers(0, len(text)))
                piece = bytes(b for b in text[src:src + ln] if b < 0x80)
                q[at:at + len(piece)] = piece
                at += len(piece) + int(rng.integers(0, 3))
            q = q[:m]
        out.append(bytes(q))
    return out


def cases():
    rng = np.random.default_rng(0x5EED5)
    for name, t in texts():
        yield name, t, queries_for(rng, name, t)


def common_prefix(a: bytes, b: bytes) -> int:
    k = 0
    while k < len(a) and k < len(b) and a[k] == b[k]:
        k += 1
    return k


def test_incremental_oracle_equals_the_plain_one():
    for _, t, queries in cases():
        for q in queries:
            want = [mo.longest_match_at(t, q[i:]) for i in range(len(q))]
            assert mo.matching_statistics(t, q).tolist() == want, (t, q)


def test_longest_match_is_the_larger_common_prefix_with_the_neighbours_of_the_insertion_point():
    import bisect

    checked = 0
    for name, t, queries in cases():
        sa = io.model_order(t)
        keys = io.suffix_keys(t, sa)
        for q in queries:
            lens = mo.matching_statistics(t, q)
            for i in range(len(q)):
                rest = q[i:]
                x = bisect.bisect_left(keys, tuple(io._signed2(b) for b in rest))
                near = [common_prefix(t[int(sa[j]):], rest) for j in (x - 1, x) if 0 <= j < len(t)]
                assert max(near) == lens[i], (name, t, q, i)
                if lens[i]:
                    lo, cnt = io.sa_range(t, sa, rest[:int(lens[i])], keys)
                    assert cnt >= 1 and lo <= x <= lo + cnt
                    got = np.sort(sa[lo:lo + cnt].astype(np.int64))
                    assert np.array_equal(got, io.occurrences(t, rest[:int(lens[i])])), (name, t, q, i)
                checked += 1
    assert checked > 30000


# ---- the lane of index_match_kernel, step for step (csrc/bmx_index_match_kernel.h; its bucket and its first search are
# ---- index_bucket and index_bound<false> of csrc/bmx_index_kernel.h, written out here) -----------------------------------

def compare(t: bytes, p: int, pat: bytes, m: int, lcp: int):
    """index_compare: (-1 below / 0 the pattern is a prefix / +1 above, common bytes); the hint must be true."""
    ln = len(t) - p
    lim = min(m, ln)
    k = min(lcp, lim)
    assert t[p:p + k] == pat[:k], "a common-prefix hint that does not hold"
    while k < lim:
        a, b = io._signed2(t[p + k]), io._signed2(pat[k])
        if a != b:
            return (-1 if a < b else 1), k
        k += 1
    if lim == m:
        return 0, lim
    return (1 if (ln - 1) % 2 == 0 and pat[ln] < 96 else -1), lim


def lane(t: bytes, sa, rest: bytes, directory):
    """(len, lo, cnt, probes) of one lane; directory: {(a, b): (lo, cnt)} of the non-empty buckets, or None."""
    m, lo0, hi0, known, probes = len(rest), 0, len(t), 0, 0
    if directory is not None and m >= 2:
        dl, dc = directory.get((rest[0], rest[1]), (0, 0))
        if dc:
            lo0, hi0, known = dl, dl + dc, 2
        else:
            m = 1
    x, y, lx, ly = lo0, hi0, known, known
    while x < y:
        mid = x + (y - x) // 2
        c, l = compare(t, int(sa[mid]), rest, m, min(lx, ly))
        probes += 1
        if c < 0:
            x, lx = mid + 1, l
        else:
            y, ly = mid, l
    ln = max(lx, ly)
    first = end = 0
    if ln > 0 and ln == known:
        first, end = lo0, hi0
    elif ln > 0:
        first = end = x
        if x > lo0 and lx == ln:
            f, b, lf, lb, step = lo0, x - 1, known, ln, 1
            while b - f >= step:
                j = b - step
                c, l = compare(t, int(sa[j]), rest, ln, min(lf, lb))
                probes += 1
                if c < 0:
                    f, lf = j + 1, l
                    break
                b, lb, step = j, l, step * 2
            while f < b:
                mid = f + (b - f) // 2
                c, l = compare(t, int(sa[mid]), rest, ln, min(lf, lb))
                probes += 1
                if c < 0:
                    f, lf = mid + 1, l
                else:
                    b, lb = mid, l
            first = b
        if x < hi0 and ly == ln:
            f, b, lf, lb, step = x, hi0, ln, known, 1
            while b - f > step:
                j = f + step
                c, l = compare(t, int(sa[j]), rest, ln, min(lf, lb))
                probes += 1
                if c > 0:
                    b, lb = j, l
                    break
                f, lf, step = j, l, step * 2
            while b - f > 1:
                mid = f + (b - f) // 2
                c, l = compare(t, int(sa[mid]), rest, ln, min(lf, lb))
                probes += 1
                if c > 0:
                    b, lb = mid, l
                else:
                    f, lf = mid, l
            end = b
    return ln, first, end - first, probes


def test_the_kernels_search_in_python_equals_the_oracle():
    checked = 0
    for name, t, queries in cases():
        sa = io.model_order(t)
        keys = io.suffix_keys(t, sa)
        directory = {}
        for a in set(t):
            for b in set(t):
                if a < 0x80 and b < 0x80:
                    lo, cnt = io.sa_range(t, sa, bytes([a, b]), keys)
                    if cnt:
                        directory[(a, b)] = (lo, cnt)
        for q in queries:
            lens = mo.matching_statistics(t, q)
            lo, cnt = mo.intervals(t, sa, q, lens, keys)
            for i in range(len(q)):
                for d in (directory, None):
                    got = lane(t, sa, q[i:], d)[:3]
                    assert got == (lens[i], lo[i], cnt[i]), (name, t, q, i, d is None, got)
                checked += 1
    assert checked > 30000


def test_an_occurrence_that_stands_alone_costs_one_probe_beyond_the_insertion_point():
    rng = np.random.default_rng(3)
    t = bytes(rng.integers(97, 123, 2000).astype(np.uint8))
    sa = io.model_order(t)
    rest = t[700:720] + b"~"
    ln, lo, cnt, probes = lane(t, sa, rest, None)
    assert (ln, cnt) == (20, 1) and int(sa[lo]) == 700
    assert probes <= int(np.ceil(np.log2(len(t)))) + 1 + 1


def test_seed_properties():
    """No seed's match lies inside another's of the same query, none can be extended in the text on either side, and
    len[i + 1] >= len[i] - 1 at every position."""
    n_seeds = 0
    for name, t, queries in cases():
        for q in queries:
            lens = mo.matching_statistics(t, q)
            assert all(lens[i + 1] >= lens[i] - 1 for i in range(len(q) - 1)), (t, q)
            cnts = [io.occurrences(t, q[i:i + int(l)]).size if l else 0 for i, l in enumerate(lens)]
            s = mo.seed_positions(lens, cnts, 1)
            spans = [(i, i + int(lens[i])) for i in s]
            every = [(i, i + int(lens[i])) for i in range(len(q)) if lens[i]]
            for a, b in spans:
                assert not any((c <= a and b <= d) and (c, d) != (a, b) for c, d in every), (t, q, a, b)
                # maximal in the text: no occurrence can be extended by the query's neighbouring byte
                if a > 0:
                    assert t.find(q[a - 1:b]) < 0
                if b < len(q):
                    assert t.find(q[a:b + 1]) < 0
            # and every match that is contained in no other is a seed
            top = [(a, b) for a, b in every if not any((c <= a and b <= d) and (c, d) != (a, b) for c, d in every)]
            assert top == spans, (t, q)
            for min_len, max_occ in ((2, 0), (3, 1), (1, 2)):
                got = mo.seed_positions(lens, cnts, min_len, max_occ)
                assert got == [i for i in s if lens[i] >= min_len and (max_occ == 0 or cnts[i] <= max_occ)]
            n_seeds += len(s)
    assert n_seeds > 5000


def test_hand_example():
    t = b"abracadabra"
    q = b"cadabrix"
    assert mo.matching_statistics(t, q).tolist() == [6, 5, 4, 3, 2, 1, 0, 0]
    sa = io.model_order(t)
    seed_off, qpos, ln, lo, cnt = mo.seeds(t, sa, [q, b"zz", b"braca"], 2)
    assert seed_off.tolist() == [0, 1, 1, 2] and qpos.tolist() == [0, 0] and ln.tolist() == [6, 5] and cnt.tolist() == [1, 1]
    assert [int(sa[x]) for x in lo] == [4, 1]
    lens = mo.matching_statistics(t, b"abrabra")  # "abra" at 0 and "abra" at 3: both seeds, "bra" at 1 is inside the first
    assert lens.tolist() == [4, 3, 2, 4, 3, 2, 1]
    assert mo.seed_positions(lens, [2, 2, 2, 2, 2, 2, 5], 1) == [0, 3]
    assert mo.seed_positions(lens, [2, 2, 2, 2, 2, 2, 5], 1, max_occ=1) == []


def test_library_exports_match_symbols(built):
    L = C.CDLL(host.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in [s for s, _, _ in host.SYMBOLS]
    for attr in ("match", "seeds"):
        assert callable(getattr(host.Index, attr))
    assert callable(host.index_seeds) and callable(host.Context.index_seeds) and callable(host.Context.index_match)
    import parallel_implementation_of_string_matching_algorithms_opencl_amd as pkg

    assert pkg.index_seeds is host.index_seeds


def test_argument_errors_before_any_device_call(built):
    L = host.lib()
    text = np.frombuffer(b"abracadabra", np.uint8).copy()
    blob = np.frombuffer(b"abracad", np.uint8).copy()
    off = np.array([0, 4, 7], np.uint64)
    out = np.full(8, 77, np.uint32)
    seed_off = np.zeros(3, np.uint64)
    total = C.c_uint64(77)
    fake = C.c_void_p(text.ctypes.data)  # stands where a device pointer or an index would: never dereferenced
    p = lambda x: None if x is None else C.c_void_p(x.ctypes.data)

    def match_dev(ctx=None, ix=None, pat=blob, po=off, count=2, ln=out, lo=None, cnt=None):
        return L.bmx_index_match_device(ctx, ix, p(pat), 7, p(po), count, p(ln), p(lo), p(cnt), None)

    def seeds_dev(ctx=None, ix=None, pat=blob, po=off, count=2, min_len=1, so=seed_off, qpos=out, ln=out, lo=out, cnt=out, cap=4):
        return L.bmx_index_seeds_device(ctx, ix, p(pat), 7, p(po), count, min_len, 0, p(so), p(qpos), p(ln), p(lo), p(cnt), cap,
                                        C.byref(total), None)

    for fn in (match_dev, seeds_dev):
        assert fn(pat=None) == host.ERR_ARG
        assert fn(po=None) == host.ERR_ARG
        assert fn(ln=None) == host.ERR_ARG
        assert fn() == host.ERR_ARG  # no context, no index
        assert fn(ctx=fake) == host.ERR_ARG  # no index
        assert fn(count=0) == host.OK  # nothing to do, nothing launched
        assert fn(count=0, pat=None, po=None) == host.OK
    assert seeds_dev(min_len=0) == host.ERR_ARG
    assert seeds_dev(min_len=0, count=0) == host.ERR_ARG
    assert seeds_dev(so=None) == host.ERR_ARG
    for name in ("qpos", "lo", "cnt"):
        assert seeds_dev(**{name: None}) == host.ERR_ARG  # a capacity needs room
    total.value = 77
    assert seeds_dev(count=0) == host.OK and total.value == 0

    def match_host(t=text, n=11, pat=blob, nbytes=7, po=off, count=2, ln=out, lo=None, cnt=None):
        return L.bmx_index_match(None, p(t), n, p(pat), nbytes, p(po), count, p(ln), p(lo), p(cnt))

    def seeds_host(t=text, n=11, pat=blob, nbytes=7, po=off, count=2, min_len=1, so=seed_off, qpos=out, ln=out, cap=4):
        return L.bmx_index_seeds(None, p(t), n, p(pat), nbytes, p(po), count, min_len, 0, p(so), p(qpos), p(ln), p(out), p(out), cap,
                                 C.byref(total))

    for fn in (match_host, seeds_host):
        assert fn(t=None) == host.ERR_ARG
        assert fn(n=0) == host.ERR_ARG
        assert fn(n=1 << 31) == host.ERR_ARG
        assert fn(pat=None) == host.ERR_ARG
        assert fn(po=None) == host.ERR_ARG
        assert fn(ln=None) == host.ERR_ARG
        assert fn(count=0) == host.OK
        # the host entries check offsets, lengths and bytes on the host
        assert fn(po=np.array([4, 0, 7], np.uint64)) == host.ERR_ARG  # decreasing
        assert fn(po=np.array([0, 4, 8], np.uint64)) == host.ERR_ARG  # an end past the blob
        assert fn(po=np.array([0, 4, 4], np.uint64)) == host.ERR_ARG  # an empty query
        long_blob = np.full(host.MAX_PATTERN + 1, ord("a"), np.uint8)
        assert fn(pat=long_blob, nbytes=long_blob.size, po=np.array([0, long_blob.size], np.uint64), count=1) == host.ERR_ARG
        high = np.frombuffer(b"ab\x80c", np.uint8).copy()
        assert fn(pat=high, nbytes=4, po=np.array([0, 4], np.uint64), count=1) == host.ERR_DOMAIN
    assert seeds_host(min_len=0) == host.ERR_ARG
    assert seeds_host(so=None) == host.ERR_ARG
    assert seeds_host(qpos=None) == host.ERR_ARG
    assert np.all(out == 77) and np.all(seed_off == 0)
