"""CPU suite for the LCP array (bmx_lcp_*): the references of tests/lcp_oracle.py against each other and against a Python
restatement of the algorithm the kernels implement (csrc/bmx_lcp_kernel.h: Phi, the four-condition reducible test, the
fill from the nearest irreducible position), the statistics' meaning against brute force, the new C-ABI symbols, and the
argument errors that return before any HIP call.  No device call is made here."""
import ctypes as C

import numpy as np

import index_oracle as io
import lcp_oracle as lo
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host
from test_index_cpu import texts

NAMES = ("bmx_lcp_array_device", "bmx_lcp_array", "bmx_lcp_stats_device", "bmx_last_lcp_ms", "bmx_last_lcp_long_pairs")


def phi_lcp(text: bytes, sa, fourth: bool = True) -> np.ndarray:
    """The kernels' algorithm, serially: phi[sa[j]] = sa[j - 1]; position i is reducible iff i >= 1, phi[i] >= 1,
    text[i - 1] == text[phi[i] - 1] and (``fourth``) phi[i - 1] == phi[i] - 1; an irreducible pair is compared, a reducible
    position takes plcp[r] - (i - r) from the nearest irreducible r below it; lcp[j] = plcp[sa[j]]."""
    n = len(text)
    sa = [int(v) for v in sa]
    phi = [None] * n
    for j in range(n):
        phi[sa[j]] = sa[j - 1] if j else -1
    plcp = [0] * n
    r = 0
    for i in range(n):
        p = phi[i]
        if i >= 1 and p >= 1 and text[i - 1] == text[p - 1] and (not fourth or phi[i - 1] == p - 1):
            plcp[i] = plcp[r] - (i - r)
        else:
            r = i
            plcp[i] = lo.common_prefix(text, i, p) if p >= 0 else 0
    out = np.array([plcp[i] for i in sa], dtype=np.int32)
    out[0] = 0
    return out


def test_references_and_the_four_condition_algorithm_agree(port):
    seen = lexicographic = 0
    for name, t in texts():
        sa = port.suffix_array(np.frombuffer(t, np.uint8))
        want = lo.brute(t, sa)
        assert np.array_equal(phi_lcp(t, sa), want), (name, t)
        if sa.tolist() == sorted(range(len(t)), key=lambda i: t[i:]):  # kasai is valid for lexicographic arrays only
            assert np.array_equal(lo.kasai(t, sa), want), (name, t)
            lexicographic += 1
        seen += 1
    assert seen == 4 * 64 * 2 and lexicographic >= 2 * 64  # (every "ab" text at the least)


def test_any_permutation():
    rng = np.random.default_rng(0x1C9)
    for it in range(50):
        name = list(io.ALPHABETS)[it % 4]
        t = io.random_text(rng, int(rng.integers(1, 65)), io.ALPHABETS[name])
        perm = rng.permutation(len(t))
        assert np.array_equal(phi_lcp(t, perm), lo.brute(t, perm)), (name, t, perm.tolist())


def test_the_fourth_condition_is_needed(port):
    """Without phi[i - 1] == phi[i] - 1 the algorithm is wrong on the builder's order outside lower-case text."""
    wrong = 0
    for name, t in texts():
        if name != "_`aA":
            continue
        sa = port.suffix_array(np.frombuffer(t, np.uint8))
        wrong += not np.array_equal(phi_lcp(t, sa, fourth=False), lo.brute(t, sa))
    assert wrong >= 1
    rng = np.random.default_rng(7)
    for _ in range(40):  # ... and lexicographic order implies it: the textbook form is right there
        t = io.random_text(rng, int(rng.integers(1, 65)), b"ab")
        sa = sorted(range(len(t)), key=lambda i: t[i:])
        assert np.array_equal(phi_lcp(t, sa, fourth=False), lo.brute(t, sa))


def test_the_vector_check_accepts_brute_force_and_rejects_its_neighbours(port):
    rng = np.random.default_rng(5)
    for name, t in texts():
        sa = port.suffix_array(np.frombuffer(t, np.uint8))
        lcp = lo.brute(t, sa)
        assert lo.wrong_entries(t, sa, lcp).size == 0, (name, t)
        perm = rng.permutation(len(t))
        assert lo.wrong_entries(t, perm, lo.brute(t, perm)).size == 0
        j = int(rng.integers(0, len(t)))
        for d in (-1, 1):
            off = lcp.copy()
            off[j] += d
            assert lo.wrong_entries(t, sa, off).tolist() == [j], (name, t, j, d)


def test_periodic_rule_equals_brute_force():
    rng = np.random.default_rng(61)
    for it in range(300):
        p, n = int(rng.integers(1, 12)), int(rng.integers(1, 120))
        if it % 3:
            para = (rng.integers(0, 26, p) + 97).astype(np.uint8)
        else:  # a paragraph that is itself a repetition: the primitive period divides p
            q = [d for d in range(1, p + 1) if p % d == 0][int(rng.integers(0, sum(p % d == 0 for d in range(1, p + 1))))]
            para = np.tile((rng.integers(0, 3, q) + 97).astype(np.uint8), p // q)
        x = np.tile(para, n // p + 1)[:n].copy()
        b = x.tobytes()
        sa = np.array(sorted(range(n), key=lambda i: b[i:]))
        for arr in (sa, rng.permutation(n)):
            assert np.array_equal(lo.periodic(x, p, arr), lo.brute(b, arr)), (p, n, b, arr.tolist())


def test_statistics_mean_longest_repeat_and_distinct_substrings(port):
    checked = 0
    for name, t in texts():
        n = len(t)
        if n > 40:
            continue
        sa = port.suffix_array(np.frombuffer(t, np.uint8))
        lcp = lo.brute(t, sa)
        subs = {}
        for i in range(n):
            for m in range(1, n - i + 1):
                subs.setdefault(t[i:i + m], []).append(i)
        assert n * (n + 1) // 2 - int(lcp.sum()) == len(subs), (name, t)
        longest = max((len(s) for s, at in subs.items() if len(at) >= 2), default=0)
        assert int(lcp.max()) == longest, (name, t)
        if longest:
            j = int(lcp.argmax())
            a, b = int(sa[j - 1]), int(sa[j])
            assert a != b and t[a:a + longest] == t[b:b + longest]
        checked += 1
    assert checked == 4 * 40 * 2


def test_embedded_pair_has_one_pair_of_exactly_L(port):
    """Every L in 1 .. 3 x LCP_LANE_BYTES, and every pad for the lengths tests/test_gpu_lcp.py uses around the budget."""
    around = [host.LCP_LANE_BYTES + d for d in (-9, -8, -1, 0, 1, 7, 8, 9)]
    for L in range(1, 3 * host.LCP_LANE_BYTES + 1):
        for pad in range(8) if L in around else (L % 8,):
            t, p, q = lo.embedded_pair(L, pad)
            assert len(t) == pad + 2 * L + 2 and t[p:p + L] == t[q:q + L] and t[p + L] != t[q + L]
            sa = port.suffix_array(np.frombuffer(t, np.uint8))
            lcp = lo.brute(t, sa)
            assert int(lcp.max()) == L and int((lcp == L).sum()) == 1, (L, pad, t)
            j = int(lcp.argmax())
            assert {int(sa[j - 1]), int(sa[j])} == {p, q}


def test_library_exports_lcp_symbols(built):
    L = C.CDLL(host.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in [s for s, _, _ in host.SYMBOLS]
    assert host.LCP_LANE_BYTES == 64 and host.LCP_LANE_BYTES % 8 == 0
    for attr in ("lcp_array_device", "lcp_array", "lcp_stats_device", "last_lcp_ms", "last_lcp_long_pairs"):
        assert callable(getattr(host.Context, attr)), attr
    for attr in ("lcp", "longest_repeat", "distinct_substrings"):
        assert callable(getattr(host.Index, attr)), attr
    import parallel_implementation_of_string_matching_algorithms_opencl_amd as pkg

    assert pkg.lcp_array is host.lcp_array and pkg.longest_repeat is host.longest_repeat


def test_argument_errors_before_any_device_call(built):
    L = host.lib()
    text = np.frombuffer(b"abracadabra", np.uint8).copy()
    sa = np.zeros(11, np.int32)
    lcp = np.full(11, 77, np.int32)
    out = (C.c_uint64 * 4)(5, 5, 5, 5)
    fake = C.c_void_p(text.ctypes.data)  # stands where a context or a device pointer would: never dereferenced
    p = lambda x: None if x is None else C.c_void_p(x.ctypes.data)

    def dev(ctx=None, t=text, n=11, s=sa, o=lcp):
        return L.bmx_lcp_array_device(ctx, p(t), n, p(s), p(o), None)

    def stats(ctx=None, o=lcp, n=11, res=out):
        return L.bmx_lcp_stats_device(ctx, p(o), n, 0, res, None)

    for ctx in (None, fake):
        assert dev(ctx, t=None) == host.ERR_ARG
        assert dev(ctx, s=None) == host.ERR_ARG
        assert dev(ctx, o=None) == host.ERR_ARG
        assert dev(ctx, n=0) == host.ERR_ARG
        assert dev(ctx, n=1 << 31) == host.ERR_ARG
        assert stats(ctx, o=None) == host.ERR_ARG
        assert stats(ctx, res=None) == host.ERR_ARG
        assert stats(ctx, n=0) == host.ERR_ARG
        assert stats(ctx, n=1 << 31) == host.ERR_ARG
    assert dev() == host.ERR_ARG and stats() == host.ERR_ARG  # no context

    def hst(t=text, n=11, s=sa, o=lcp):
        return L.bmx_lcp_array(None, p(t), n, p(s), p(o))

    assert hst(t=None) == host.ERR_ARG
    assert hst(o=None) == host.ERR_ARG
    assert hst(n=0) == host.ERR_ARG
    assert hst(n=1 << 31) == host.ERR_ARG
    assert L.bmx_last_lcp_ms(None) < 0 and L.bmx_last_lcp_long_pairs(None) < 0
    assert np.all(lcp == 77) and list(out) == [5, 5, 5, 5]
