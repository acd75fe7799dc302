"""CPU suite for the batched edit distance (bmx_edit_distance_batch*): the case generators and their expected values
against the properties of the distance (and against the reference build where it is present), the kernel's lane
functions built for the host under AddressSanitizer against a plain table (tests/ed_batch_check.hip), the model of the
kernel's dispatch (cases.kernel_paths) applied to every generator that aims at one path, the two bounds on pairs for the
pair-by-pair path, the new C-ABI symbols and constants, and the argument errors that return before any HIP call.  No
compute call is made on a device here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import ed_batch_cases as cases
from conftest import ROOT
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

CSRC = os.path.join(ROOT, "parallel_implementation_of_string_matching_algorithms_opencl_amd", "csrc")
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


def _hipcc() -> str:
    mk = open(os.path.join(CSRC, "Makefile")).read()
    return os.environ.get("HIPCC") or re.search(r"^HIPCC\s*\?=\s*(\S+)", mk, re.M).group(1)


def test_lane_functions_match_the_plain_table(tmp_path):
    """tests/ed_batch_check.hip: ed_batch_load_pattern, ed_batch_walk and ed_batch_step built for the host with
    AddressSanitizer and UBSan, every pattern and walked string in a heap allocation of exactly its blob's size.  Without
    the sanitizers' runtime (the linker does not find it) the same program is built plain: the distances and the
    register layout are still checked, a load past the blob no longer is."""
    exe = str(tmp_path / "ed_batch_check")
    cmd = [_hipcc(), "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-I", CSRC,
           os.path.join(ROOT, "tests", "ed_batch_check.hip"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    build = subprocess.run(cmd + san, capture_output=True, text=True, timeout=300)
    if build.returncode != 0 and "libclang_rt" in build.stderr:
        build = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")  # (the leak check needs ptrace, which a sandbox may deny)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "pattern loads = 32640" in run.stdout and "pairs = 65280" in run.stdout and "bad = 0" in run.stdout, run.stdout


def test_kernel_paths_on_worked_examples():
    """The dispatch model by hand, before it judges the generators."""
    K = cases.kernel_paths
    # offsets alone: an empty side, a length difference over the limit; listed: both over 64, a walk over 65,536
    assert K([0, 5, 9, 65, 64], [7, 0, 3, 65, 65537]) == [(cases.OFFSETS, False), (cases.OFFSETS, False),
                                                           (cases.PAIR32, False), (cases.LISTED, False), (cases.LISTED, False)]
    assert K([9, 9], [5, 20], limit=5) == [(cases.PAIR32, False), (cases.OFFSETS, False)]
    # b = 3 bytes at offset 0 of a 3-byte blob: byte path; with 13 more bytes stated: one load
    assert K([9], [3], b_bytes=15)[0] == (cases.PAIR32, True) and K([9], [3], b_bytes=16)[0] == (cases.PAIR32, False)
    # a wave is 64 consecutive pairs: one bit vector of 33 bytes makes its 64 lanes wide, and not the 65th pair's
    got = K([8] * 63 + [33, 8], [40] * 65)
    assert [p for p, _ in got] == [cases.PAIR64] * 64 + [cases.PAIR32]
    assert [f for _, f in got] == [False] * 63 + [True, True]  # a's last 33 + 8 bytes: chunk 2 of 33, chunk 0 of 8
    # the shorter side is the bit vector, a on a tie: 20 against 20 reads a's blob (16 bytes + 4 at its end)
    assert K([20], [20], b_bytes=100)[0] == (cases.PAIR32, True) and K([20], [20], a_bytes=32)[0] == (cases.PAIR32, False)
    # one against many: a query of 1..64 bytes is shared, whatever the candidate's length; 65 bytes is pairwise or listed
    assert K([32], [5, 0, 70000], one=True) == [(cases.SHARED32, False), (cases.OFFSETS, False), (cases.SHARED32, False)]
    assert K([33], [5, 70000], one=True) == [(cases.SHARED64, False)] * 2
    assert K([65], [5, 66, 7], one=True) == [(cases.PAIR32, False), (cases.LISTED, False), (cases.PAIR32, True)]
    assert K([7], [9], one=True) == [(cases.PAIR32, True)]  # a single pair is pairwise


def _tally(paths):
    return {p: sum(1 for q, _ in paths if q == p) for p in {q for q, _ in paths}}


def test_word_column_reaches_both_words(port):
    a, b = cases.word_column()
    la, lb = cases.lengths(a), cases.lengths(b)
    for x, y in ((la, lb), (lb, la)):  # the GPU test runs both orders
        paths = cases.kernel_paths(x, y)
        assert set(_tally(paths)) == {cases.PAIR32, cases.PAIR64}  # none listed, none from its offsets
        seen = {}  # (path, alphabet index, bit vector on the first side) -> the m's
        walked = {cases.PAIR32: set(), cases.PAIR64: set()}
        n_eq_m = {cases.PAIR32: set(), cases.PAIR64: set()}
        for i, (path, _) in enumerate(paths):
            m, n = min(x[i], y[i]), max(x[i], y[i])
            seen.setdefault((path, (i - 1024) // 512 if i >= 1024 else i // 256, x[i] <= y[i]), set()).add(m)
            walked[path].add(n)
            if n == m:
                n_eq_m[path].add(m)
        for alpha in range(4):
            for first in (True, False):
                assert seen[(cases.PAIR32, alpha, first)] == set(range(1, 33)), (alpha, first)
                assert seen[(cases.PAIR64, alpha, first)] == set(range(1, 65)), (alpha, first)  # (with m <= 32 on wide waves)
        for path in walked:
            assert {n % 16 for n in walked[path]} == set(range(16)) and set(range(1, 16)) <= walked[path], path
        assert n_eq_m[cases.PAIR32] == set(range(1, 33)) and n_eq_m[cases.PAIR64] == set(range(1, 65))
    for k, alpha in enumerate(cases.ALPHABETS):  # the groups of 256 pairs are one alphabet each, and use it
        for lo in list(range(256 * k, 256 * k + 256)) + list(range(1024 + 512 * k, 1536 + 512 * k)):
            assert len(set(a[lo]) | set(b[lo])) <= alpha
    assert max(max(s) for s in a + b) >= 0x80
    assert cases.n_fallback(a, b, cases.BATCH_LONG) == 0
    check_properties(port, a, b, range(0, len(a), 5))


def test_blob_end_calls_reach_the_byte_path(port):
    n_calls = 0
    for col in cases.blob_end_calls():
        word, pat, txt, calls = col["word"], col["pat"], col["txt"], col["calls"]
        want_path = cases.PAIR64 if word == 64 else cases.PAIR32
        lp, lt = cases.lengths(pat), cases.lengths(txt)
        off = np.concatenate(([0], np.cumsum(lp)))
        assert len(pat) == len(txt) + 1 and lp[-1] == 16  # the memory behind the last pattern
        assert {(lp[c - 1], s) for c, s in calls} == {(m, s) for m in range(1, word + 1) for s in cases.blob_end_slacks(m)}
        for count, slack in calls:
            m = lp[count - 1]
            r = (16 - m % 16) % 16
            assert slack in (0, r - 1, r) and off[count] + slack <= off[-1]
            for pattern_first in (True, False):
                if pattern_first:
                    paths = cases.kernel_paths(lp[:count], lt[:count], a_bytes=int(off[count]) + slack)
                else:
                    paths = cases.kernel_paths(lt[:count], lp[:count], b_bytes=int(off[count]) + slack)
                assert [p for p, _ in paths] == [want_path] * count  # every earlier pair is still compared, on this word
                assert paths[-1][1] == (slack < r), (word, m, slack)
                n_calls += 1
        assert all(len(t) > len(p) for p, t in zip(pat, txt))
        check_properties(port, pat[:-1], txt, range(len(txt)))
    assert n_calls == 540 <= 576


def test_shared_and_long_shared_cases(port):
    calls = cases.shared_calls()
    assert [len(q) for q, _ in calls] == list(range(1, 65))
    for q, cand in calls:
        assert max(q) >= 0x80 and (len(q) == 1 or min(q) < 0x80)
        assert len(cand) >= 257 and min(map(len, cand)) == 0 and max(map(len, cand)) <= 80
        paths = cases.kernel_paths([len(q)], cases.lengths(cand), one=True)
        want = cases.SHARED32 if len(q) <= 32 else cases.SHARED64
        assert all(p == (want if c else cases.OFFSETS) for (p, _), c in zip(paths, cand))
        assert cases.n_fallback([q] * len(cand), cand, cases.BATCH_LONG) == 0  # and none as the pairwise call either
    for length in cases.SHARED_LIMIT_LENGTHS:
        q, cand = calls[length - 1]
        assert len(q) == length
        paths = cases.kernel_paths([length], cases.lengths(cand), one=True, limit=3)
        assert sum(p != cases.OFFSETS for p, _ in paths) >= 8  # (some candidates are still walked under the limit)
    q, cand = calls[6]
    check_properties(port, [q] * len(cand), cand, range(0, len(cand), 3))
    longs = cases.long_shared()
    assert [len(q) for q, _ in longs] == [7, 64]
    for q, cand in longs:
        lc = cases.lengths(cand)
        assert sorted(lc)[-3:] == [65536, 65537, 200000] == sorted(cases.LONG_SHARED) and sorted(lc)[-4] <= 80
        assert cand[290].count(longs[1][0]) > 3000  # the 64-byte query repeated, with edits
        paths = cases.kernel_paths([len(q)], lc, one=True)
        assert cases.LISTED not in _tally(paths)  # expected fallbacks: 0
        assert {paths[i][0] for i in (5, 70, 290)} == {cases.SHARED32 if len(q) <= 32 else cases.SHARED64}
        assert len({i // cases.WAVE for i in (5, 70, 290)}) == 3
        # as the pairwise call with the query repeated: the two candidates over BATCH_LONG are listed
        assert _tally(cases.kernel_paths([len(q)] * len(cand), lc)).get(cases.LISTED, 0) == 2 <= cases.MAX_FALLBACK_PAIRS
        assert cases.n_fallback([q] * len(cand), cand, cases.BATCH_LONG) == 2


def test_growth_pairs_and_both_fallback_bounds():
    cols = cases.growth_pairs()
    listed = {}
    for k, (a, b) in enumerate(cols):
        la, lb = cases.lengths(a), cases.lengths(b)
        both = [(x, y) for x, y in zip(la, lb) if min(x, y) > cases.BATCH_WORD]
        assert len(both) == cases.GROWTH_LISTED[k] and all(65 <= x <= 70 and 65 <= y <= 70 for x, y in both)
        assert len(a) - len(both) == cases.GROWTH_SHORT and max(max(x, y) for x, y in zip(la, lb) if min(x, y) <= 64) <= 40
        for limit in (None, 2):
            listed[(k, limit)] = _tally(cases.kernel_paths(la, lb, limit=limit)).get(cases.LISTED, 0)
        assert listed[(k, None)] == cases.GROWTH_LISTED[k] == cases.n_fallback(a, b, cases.BATCH_LONG)
    assert cases.GROWTH_LISTED[0] > 4096 and cases.GROWTH_LISTED[1] > cases.GROWTH_LISTED[0] > cases.GROWTH_LISTED[2] > 0
    assert 256 < listed[(0, 2)] < cases.GROWTH_LISTED[0]  # the limit answers some of them from their offsets
    for name, seq in cases.GROWTH_SEQUENCES.items():  # the one case past MAX_FALLBACK_PAIRS has a bound of its own
        assert sum(listed[c] for c in seq) <= cases.MAX_GROWTH_LISTED, name
    # every other case keeps the cap of MAX_FALLBACK_PAIRS
    others = [cases.random_pairs(), cases.grid_pairs(), cases.long_pairs(), cases.word_column()]
    others += [(c["pat"][:-1], c["txt"]) for c in cases.blob_end_calls()]
    others += [([q] * len(cand), cand) for q, cand in cases.shared_calls() + cases.long_shared()]
    others += [([q] * len(cand), cand) for q, cand in (cases.one_vs_many(n) for n in cases.QUERY_LENGTHS)]
    for a, b in others:
        assert cases.n_fallback(a, b, cases.BATCH_LONG) <= cases.MAX_FALLBACK_PAIRS


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
