"""GPU suite for the text index family (count, locate, match, seeds, map) and the LCP array at the top of their domain and
across their workspace thresholds.

Part A: a staircase text of n = 2^31 - 1 bytes (tests/stair_cases.py: a^(2^30+5) b c^2 d^3 e^(2^29+77) f^600 g^.. h^300) whose
suffix array and LCP array have closed forms, so the index is created over a caller's array made by two torch.arange calls
and no expected value is typed in.  Array indices, positions and interval sizes lie on both sides of 2^30 and reach 2^31 - 2:
where a 32-bit sign or carry mistake in a bisection, a galloping step, a segment offset or a window can show.
Part B: a^4111, where one 16-byte read has exactly 4,096 candidates, to drive the per-candidate and the per-position
workspace across the 256 MiB above which they are freed, and the candidate total to BMX_MAP_MAX_CANDIDATES and one read
beyond; every crossing is followed by small calls that must still be right.

Peak device memory of the module: about 40 GiB (text 2 GiB, array 8 GiB; beside them either the LCP array and its workspace,
8 GiB each, with the chunks they are compared with, or locate's honestly allocated 16 GiB position list, with what torch's
allocator keeps of the other).  Part A skips only when less than that is free.  Measured on the MI355X by polling the
device's free memory every 20 ms through the whole module: 27.4 GiB.

Wall time per test on one MI355X (the module: 13 cases, 3.0 s, unskipped): the 42-million-position locate with its four
following calls 0.71 s; the LCP array of 2^31 - 1 bytes twice with both comparisons and the small one between 0.62 s; the
fixture of the big text 0.20 s; the candidate workspace 0.12 s; match and seeds 0.11 s; the n = 2^31 refusals 0.10 s; two
indexes 0.06 s; map 0.02 .. 0.04 s per k; the 2^27-candidate cap with the refusal behind it 0.03 s; count 0.03 s; the
per-position workspace and the device builders 0.01 s each.

The locate case takes 70,000 copies of `f` (600 occurrences each: 42 million positions, > 65,536 queries), not of `g`: one
`g` alone has 5.4 * 10^8 occurrences, so 70,000 of them would be refused, and a single query of 10^8 or more occurrences is
a performance question of its own."""
import ctypes as C
import types

import numpy as np
import pytest

import index_oracle as io
import map_oracle as mp
import stair_cases as sc
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host
from test_gpu_index import on_device
from test_gpu_index_map import raw_map, same
from test_gpu_index_match import MARK, check_seeds, column, run_match
from test_gpu_index_match import verify as match_verify

pytestmark = pytest.mark.gpu

PEAK_BYTES = 40 << 30
BASE = (1 << 40) + 3
CHUNK = 1 << 26
N31 = 1 << 31
A, B, CC, D, E, F, G, H = (bytes([c]) for c in b"abcdefgh")


def u32(t):
    """An int32 tensor that holds uint32 values, as int64 numpy."""
    return t.cpu().numpy().view(np.uint32).astype(np.int64)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def current_stream():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def big(ctx):
    """The big staircase on the device and its index over the closed-form array, made once."""
    import torch

    free, _ = torch.cuda.mem_get_info()
    if free < PEAK_BYTES:
        pytest.skip("%.1f GiB of device memory free, the module needs %d" % (free / 2 ** 30, PEAK_BYTES >> 30))
    s = sc.Staircase(sc.big_runs())
    assert s.n == N31 - 1
    text, sa = s.device_text(), s.device_sa()
    idx = ctx.index(text, sa=sa)
    ns = types.SimpleNamespace(s=s, text=text, sa=sa, idx=idx)
    yield ns
    idx.close()
    ns.text = ns.sa = ns.idx = None  # (pytest still holds the namespace here)
    del text, sa, idx
    torch.cuda.empty_cache()


# ---- the device builders ---------------------------------------------------------------------------------------------------

def test_device_builders_equal_the_closed_forms(ctx, big):
    """device_text / device_sa / device_sa_chunk / device_lcp_chunk against the numpy closed forms: a small staircase in full
    (and the builder's own array of it), the big one in windows around every run boundary and at both ends."""
    small = sc.Staircase(sc.letters("a:7 b:1 c:2 d:300 k:64 z:5"))
    t, sa = small.device_text(), small.device_sa()
    assert t.cpu().numpy().tobytes() == small.text()
    assert np.array_equal(sa.cpu().numpy(), small.sa_chunk(0, small.n))
    assert np.array_equal(ctx.suffix_array_device(t).cpu().numpy(), small.sa_chunk(0, small.n))
    for lo, hi in ((0, small.n), (3, 9), (8, 311), (small.n - 4, small.n)):
        assert np.array_equal(small.device_sa_chunk(lo, hi).cpu().numpy(), small.sa_chunk(lo, hi))
        assert np.array_equal(small.device_lcp_chunk(lo, hi).cpu().numpy(), small.lcp_chunk(lo, hi))
    s = big.s
    for at in [0, s.n] + s.start[1:-1]:
        lo, hi = max(0, at - 700), min(s.n, at + 700)
        assert big.text[lo:hi].cpu().numpy().tobytes() == s.slice(lo, hi)
        assert np.array_equal(big.sa[lo:hi].cpu().numpy(), s.sa_chunk(lo, hi))
        assert np.array_equal(s.device_sa_chunk(lo, hi).cpu().numpy(), s.sa_chunk(lo, hi))
        assert np.array_equal(s.device_lcp_chunk(lo, hi).cpu().numpy(), s.lcp_chunk(lo, hi))


def test_two_to_the_31_is_refused(ctx, big):
    """n = 2^31 over the same buffers: BMX_ERR_ARG from both entries, no index made."""
    import torch

    h = C.c_void_p()
    rc = ctx._L.bmx_index_create_device(ctx._h, ptr(big.text), N31, ptr(big.sa), current_stream(), C.byref(h))
    assert rc == host.ERR_ARG and not h
    rc = ctx._L.bmx_index_create_device(ctx._h, ptr(big.text), N31, None, current_stream(), C.byref(h))
    assert rc == host.ERR_ARG and not h
    lcp = torch.full((16,), MARK, dtype=torch.int32, device="cuda")
    rc = ctx._L.bmx_lcp_array_device(ctx._h, ptr(big.text), N31, ptr(big.sa), ptr(lcp), current_stream())
    assert rc == host.ERR_ARG and bool((lcp == MARK).all())


# ---- count -----------------------------------------------------------------------------------------------------------------

def boundary_queries(s):
    """c^x d^y of up to 512 bytes around every boundary c | d of the staircase, with 1, 2 and the largest number of letters
    that fits on either side (the whole run, or what 512 bytes leave), and one letter more than a short run holds."""
    out = set()
    for (c, rc), (d, rd) in zip(s.runs, s.runs[1:]):
        c, d = bytes([c]), bytes([d])
        for x in {1, 2, min(rc, 256), min(rc, 510), min(rc, 511)}:
            for y in {1, 2, min(rd, 512 - x)} - {0}:
                out.add((c * x + d * y)[-512:])
        for y in {1, 2, min(rd, 256), min(rd, 510), min(rd, 511)}:
            for x in {1, 2, min(rc, 512 - y)} - {0}:
                out.add((c * x + d * y)[:512])
        if rc <= 3:
            out.add(c * (rc + 1) + d)
        if rd <= 3:
            out.add(c + d * (rd + 1))
    out |= {A * 20 + B + CC * 2 + D * 3 + E * 20, B + CC * 2 + D * 3, A + B + CC * 2 + D * 3 + E, B + CC + D * 3, A * 505 + B + CC * 2 + D * 3 + E,
            F * 10 + G, F * 512, F * 511 + G, G * 212 + H * 300, G * 211 + H * 301}
    assert all(1 <= len(q) <= 512 for q in out)
    return sorted(out)


SMALL = [B, CC, CC * 2, CC * 3, D * 3, D * 4, F * 512, H * 300, H * 301]
ABSENT = [B + A, b"A", b"z", b"`", H * 10 + b"i"]


def count_queries(s):
    powers = [bytes([c]) * m for c, _ in s.runs for m in (1, 2, 511, 512)]
    return powers + SMALL + boundary_queries(s) + ABSENT


def check_count(s, idx, queries):
    lo, cnt = idx.count(queries)
    lo, cnt = u32(lo), u32(cnt)
    hits = 0
    for q, l, c in zip(queries, lo.tolist(), cnt.tolist()):
        first, count = s.occurrence_range(q)
        assert c == count, (q[:20], len(q), c, count)
        if count:
            assert (l, c) == s.interval(q), (q[:20], len(q), l)
            hits += 1
        else:
            assert s.is_insertion_point(q, l), (q[:20], len(q), l)
    return hits, lo, cnt


def test_count_on_both_sides_of_two_to_the_30(ctx, exp_ctx, big):
    s = big.s
    queries = count_queries(s)
    hits, lo, cnt = check_count(s, big.idx, queries)
    assert hits > 50 and len(queries) - hits >= 15
    assert cnt.max() == (1 << 30) + 5 and int((cnt > 1 << 29).sum()) >= 6 and int(((lo > 1 << 30) & (cnt > 0)).sum()) > 50
    assert all(s.occurrence_range(q)[1] == 0 for q in ABSENT) and s.occurrence_range(H * 300) == (s.n - 300, 1)
    # the same answers when every query searches the whole array (the experiments build's switch)
    exp_ctx.set_knob("index_no_dir", 1)
    with exp_ctx.index(big.text, sa=big.sa) as plain:
        _, lo0, cnt0 = check_count(s, plain, queries)
    assert np.array_equal(lo0, lo) and np.array_equal(cnt0, cnt)


# ---- locate ----------------------------------------------------------------------------------------------------------------

def raw_locate(ctx, idx, d_blob, d_off, count, capacity, d_pos, base=BASE):
    import torch

    out_off = torch.full((count + 2,), MARK, dtype=torch.int64, device="cuda")
    total = C.c_uint64(0)
    rc = ctx._L.bmx_index_locate_device(ctx._h, idx._h, ptr(d_blob), d_blob.numel(), ptr(d_off), count, base, ptr(out_off),
                                        ptr(d_pos), capacity, C.byref(total), current_stream())
    assert int(out_off[count + 1]) == MARK
    return rc, int(total.value), out_off[:count + 1]


def expected_positions(first, counts, base=BASE):
    """The positions of every query, ascending within a query, as one int64 device tensor (the occurrences of a query on a
    staircase are the range [first, first + count))."""
    import torch

    c = torch.from_numpy(np.asarray(counts, np.int64)).cuda()
    f = torch.from_numpy(np.asarray(first, np.int64)).cuda()
    start = torch.cumsum(c, 0) - c
    return torch.repeat_interleave(f - start + base, c) + torch.arange(int(c.sum()), device="cuda")


def check_small_locate(s, idx, queries):
    offsets, pos, total = idx.locate(queries, base_offset=BASE)
    rng = [s.occurrence_range(q) for q in queries]
    counts = [c for _, c in rng]
    assert total == sum(counts) and offsets.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    assert pos.tolist() == [BASE + p for f, c in rng for p in range(f, f + c)]


def test_locate_across_the_workspace_threshold(ctx, big):
    """> 65,536 queries (the per-query workspace grows) that store 42 million positions (the per-position workspace passes 256
    MiB and is freed), then a small call at once, a capacity one below the total, the refusal of 2^31 - 1 positions or more
    with an honestly allocated list, and a small call again."""
    import torch

    s, idx = big.s, big.idx
    small = SMALL + ABSENT
    queries = [q for i in range(70_000) for q in (F, small[i % len(small)])]
    while s.occurrence_range(queries[-1])[1] == 0:  # the capacity case below wants an occupied last segment
        queries.pop()
    blob, off = host.pack_strings(queries)
    d_blob, d_off, count = torch.from_numpy(blob.copy()).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(), len(queries)
    kinds = {q: s.occurrence_range(q) for q in set(queries)}
    first = np.array([kinds[q][0] for q in queries], np.int64)
    counts = np.array([kinds[q][1] for q in queries], np.int64)
    ends = np.cumsum(counts)
    total = int(ends[-1])
    assert count > 65_536 and total > 42_000_000 and 2 * 4 * total > 256 << 20
    want = expected_positions(first, counts)
    want_off = torch.from_numpy(np.concatenate([[0], ends])).cuda()

    d_pos = torch.full((total + 4,), MARK, dtype=torch.int64, device="cuda")
    rc, got_total, out_off = raw_locate(ctx, idx, d_blob, d_off, count, total, d_pos)
    assert rc == host.OK and got_total == total
    assert torch.equal(out_off, want_off)
    assert torch.equal(d_pos[:total], want) and bool((d_pos[total:] == MARK).all())
    five = [F * 512, A * 20 + B + CC * 2, H * 299, b"z", G + H * 300]
    check_small_locate(s, idx, five)  # at once: the workspace is made again

    d_pos.fill_(MARK)
    rc, got_total, out_off = raw_locate(ctx, idx, d_blob, d_off, count, total - 1, d_pos)
    assert rc == host.ERR_CAPACITY and got_total == total and torch.equal(out_off, want_off)
    stored = int(ends[ends <= total - 1][-1])  # every query whose segment ends at or below the capacity
    assert stored == total - counts[-1] and 0 < stored < total
    assert torch.equal(d_pos[:stored], want[:stored])
    # nothing is written at or behind the capacity; the entries between the stored prefix and the capacity are
    # unspecified (include/bmx.h), so they are not held to the mark
    assert bool((d_pos[total - 1:] == MARK).all())
    del d_pos, want
    torch.cuda.empty_cache()

    two = torch.from_numpy(np.frombuffer(A + A, np.uint8).copy()).cuda()
    two_off = torch.tensor([0, 1, 2], dtype=torch.int64, device="cuda")
    cnt_a = (1 << 30) + 5
    d_pos = torch.empty(2 * cnt_a, dtype=torch.int64, device="cuda")
    rc, got_total, out_off = raw_locate(ctx, idx, two, two_off, 2, 2 * cnt_a, d_pos)
    assert rc == host.ERR_ARG and got_total == 2 * cnt_a and got_total > N31
    assert "2^31 - 1 positions" in host.lib().bmx_last_error().decode()
    assert out_off.tolist() == [0, cnt_a, 2 * cnt_a]
    del d_pos
    torch.cuda.empty_cache()
    check_small_locate(s, idx, five[::-1] + [B, D * 3])


# ---- match and seeds -------------------------------------------------------------------------------------------------------

def limit_reads(s):
    """The long one-letter reads, the read that ends at n - 1 and the boundary reads of the count test, each alone and with
    one foreign letter put in at the boundary (the middle of a one-letter read): above every text letter, so that the
    lane gallops BACK from behind its interval, and below every one, so that it gallops forward from in front of it."""
    whole = [A * 512, E * 512, G * 212 + H * 300]
    reads = whole + [q for q in boundary_queries(s) if len(q) >= 3]
    out = list(reads)
    for r in reads:
        at = next((i for i in range(1, len(r)) if r[i] != r[i - 1]), len(r) // 2)
        for foreign in (b"z", b"A") if r in whole else (b"z",):
            out.append((r[:at] + foreign + r[at:])[:512])
    return out


def test_match_and_seeds_gallop_across_two_to_the_30(ctx, big):
    s, idx = big.s, big.idx
    reads = limit_reads(s)
    blob, off = column(reads)
    lens, lo, cnt = run_match(idx, blob, off)
    want = [np.full(blob.size, MARK, np.int64) for _ in range(3)]
    memo = {}
    for a, r in zip(off[:-1], reads):
        if r not in memo:
            memo[r] = s.match(r)
        for w, x in zip(want, memo[r]):
            w[int(a):int(a) + len(r)] = x
    for g, w, name in zip((lens, lo, cnt), want, ("len", "lo", "cnt")):
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (name, bad[:5], g[bad[:5]], w[bad[:5]])
    # intervals of more than 2^30 entries were crossed in both directions: from their first entry and from their last
    wl, wlo, wc = memo[A * 512]
    assert wc[-5:].min() > 1 << 30 and wc.min() > (1 << 30) - 512 and np.all(wlo == 0)  # the rests a^5 .. a: forward
    wl, wlo, wc = memo[A * 256 + b"z" + A * 255]
    assert wl[0] == 256 and wl[251] == 5 and wc[251:256].min() > 1 << 30 and wl[257] == 255  # a^5 z .. a z: back
    check_seeds(idx, blob, off, want[0], want[1], want[2], ((12, 0), (12, 8), (1, 1)))


# ---- map -------------------------------------------------------------------------------------------------------------------

def map_reads():
    exact = A * 20 + B + CC * 2 + D * 3 + E * 20
    at = 20  # the b
    edits = []
    for side in (at - 3, at + 4):  # in the a's in front of the b, in the d's behind it
        sub = bytearray(exact)
        sub[side] = ord("x")
        edits += [bytes(sub), exact[:side] + b"x" + exact[side:], exact[:side] + exact[side + 1:]]
    return [exact] + edits + [F * 40 + G * 40, E * 24 + b"x" + F * 25, G * 30 + H * 300, G * 30 + H * 300 + H * 2, G * 30 + H * 298]


def check_map(ctx, idx, oracle, reads, min_len, max_occ, k, base=BASE):
    blob, off = column(reads)
    rc, total, best, coff, cand = raw_map(ctx, idx, blob, off, min_len, max_occ, k, base)
    assert rc == host.OK
    w = oracle(reads, min_len, max_occ, k, base)
    assert total == w[3][-1] and np.array_equal(coff, w[3]), (k, coff, w[3])
    for g, x, name in zip(cand, w[4:], ("cand_start", "cand_end", "cand_dist")):
        assert same(g, x), (name, k, g, x)
    for g, x, name in zip(best, w[:3], ("best_start", "best_end", "best_dist")):
        assert same(g, x), (name, k, g, x)
    return w


@pytest.mark.parametrize("k", (0, 2, 4))
def test_map_at_both_ends_of_the_big_text(k, ctx, big):
    s = big.s
    reads = map_reads()
    w = check_map(ctx, big.idx, s.index_map, reads, 12, 8, k)
    dist = w[2].tolist()
    assert dist[0] == 0 and dist[7] == 0 and dist[9] == 0 and dist[11] == 0
    assert dist[8] == mp.NO_HIT and w[3][9] == w[3][8]  # e^24 x f^25: no seed under max_occ, no candidate
    assert dist[10] == (2 if k >= 2 else mp.NO_HIT) and w[3][11] - w[3][10] >= 1  # the window is clipped at n
    if k >= 2:
        assert all(d <= 1 for d in dist[1:7]) and int(w[1][10]) == BASE + s.n - 1 and int(w[1][9]) == BASE + s.n - 1
        assert int(w[0][0]) == BASE + (1 << 30) + 5 - 20


# ---- LCP -------------------------------------------------------------------------------------------------------------------

def check_lcp(s, lcp):
    import torch

    assert lcp.numel() == s.n
    for lo in range(0, s.n, CHUNK):
        hi = min(s.n, lo + CHUNK)
        want = s.device_lcp_chunk(lo, hi)
        if not torch.equal(lcp[lo:hi], want):
            bad = torch.nonzero(lcp[lo:hi] != want)[:5, 0]
            raise AssertionError((lo, bad.tolist(), lcp[lo:hi][bad].tolist(), want[bad].tolist()))


def test_lcp_at_the_limit_and_its_workspace(ctx, big):
    """The LCP array of the big text (workspace of 8 GiB: freed when the call returns), then of a small one on the same
    context, then of the big one again."""
    import torch

    s = big.s
    lcp = torch.full((s.n,), MARK, dtype=torch.int32, device="cuda")
    got = ctx.lcp_array_device(big.text, big.sa, out=lcp)
    assert got.data_ptr() == lcp.data_ptr()
    check_lcp(s, lcp)
    assert ctx.last_lcp_long_pairs() >= 1
    for min_len in (0, 1, 1 << 30, (1 << 30) + 4, (1 << 30) + 5):
        st = ctx.lcp_stats_device(lcp, min_len)
        assert (st["max"], st["argmax"], st["sum"], st["count"]) == s.stats(min_len), min_len
    small = sc.Staircase(sc.letters("a:400 b:1 c:2 d:97 e:500"))
    assert small.n == 1000
    small_lcp = ctx.lcp_array_device(small.device_text(), small.device_sa())
    assert np.array_equal(small_lcp.cpu().numpy(), small.lcp_chunk(0, small.n))
    st = ctx.lcp_stats_device(small_lcp, 3)
    assert (st["max"], st["argmax"], st["sum"], st["count"]) == small.stats(3)
    lcp.fill_(MARK)
    ctx.lcp_array_device(big.text, big.sa, out=lcp)
    check_lcp(s, lcp)
    assert ctx.last_lcp_long_pairs() >= 1
    del lcp
    torch.cuda.empty_cache()


# ---- two indexes on one context --------------------------------------------------------------------------------------------

def test_two_indexes_on_one_context(ctx, big):
    s = big.s
    rng = np.random.default_rng(0x2D1)
    text = bytes((rng.integers(0, 4, 5000) + 97).astype(np.uint8))
    reads, _, _ = mp.edit_reads(rng, text, 12, 40, 2, b"abcd")
    big_reads = map_reads()[:3] + [G * 30 + H * 300]
    big_queries = SMALL + ABSENT + [A * 512, E + F]
    with ctx.index(on_device(text, 3)) as other:
        sa = other.sa.cpu().numpy()
        small_oracle = lambda q, min_len, max_occ, k, base: mp.index_map(text, sa, q, min_len, max_occ, k, base)
        queries = reads + [b"ab", b"zz", text[100:108]]
        occ = [io.occurrences(text, q) for q in queries]
        want_seeds = s.seeds(big_reads, 12, 8)
        for turn in range(2):
            check_count(s, big.idx, big_queries)
            lo, cnt = other.count(queries)
            for l, c, o in zip(u32(lo).tolist(), u32(cnt).tolist(), occ):
                assert c == o.size and np.array_equal(np.sort(sa[l:l + c]), o)
            got = big.idx.seeds(big_reads, 12, 8)
            assert all(np.array_equal(g.cpu().numpy().astype(np.int64), w) for g, w in zip(got, want_seeds))
            match_verify(ctx, None, text, reads, full=False, seed_settings=((6, 8),), idx=other)
            check_map(ctx, big.idx, s.index_map, big_reads, 12, 8, 2 + turn)
            check_map(ctx, other, small_oracle, reads, 6, 8, 2, base=7)


# ---- part B: workspace thresholds on a small text --------------------------------------------------------------------------

N_B, READ = 4111, A * 16
PER_READ = 4096  # candidates of one read with max_occ = 4096: every occurrence of a^16


@pytest.fixture(scope="module")
def stairs_b(ctx):
    """a^4111 with the array n-1 .. 0 (checked once against the builder), its index, and the one-read answer of the oracle."""
    import torch

    s = sc.Staircase([("a", N_B)])
    text, sa = s.device_text(), s.device_sa()
    assert torch.equal(ctx.suffix_array_device(text), sa) and sa.tolist() == list(range(N_B - 1, -1, -1))
    idx = ctx.index(text, sa=sa)
    one = mp.index_map(s.text(), sa.cpu().numpy(), [READ], 4, PER_READ, 1)
    assert one[3].tolist() == [0, PER_READ] and np.all(one[6] == 0)
    p = np.arange(N_B - 16, -1, -1)  # the candidates in array order: descending positions
    end = np.minimum(N_B, p + 17) - 1
    assert np.array_equal(one[5], end.astype(np.uint64)) and np.array_equal(one[4], (end - 15).astype(np.uint64))
    assert (int(one[0][0]), int(one[1][0]), int(one[2][0])) == (int(end.min()) - 15, int(end.min()), 0)  # the best: the smallest end
    ns = types.SimpleNamespace(s=s, text=text, sa=sa, idx=idx, one=one)
    yield ns
    idx.close()
    ns.text = ns.sa = ns.idx = None
    del text, sa, idx
    torch.cuda.empty_cache()


def reads_on_device(count):
    import torch

    blob = torch.full((16 * count,), ord("a"), dtype=torch.uint8, device="cuda")
    return blob, torch.arange(0, 16 * count + 1, 16, dtype=torch.int64, device="cuda")


def device_map(ctx, idx, count, max_occ, capacity, lists=True, min_len=4, k=1):
    """bmx_index_map_device over `count` copies of the read, everything on the device: (rc, total, best, cand_off, cand)."""
    import torch

    blob, off = reads_on_device(count)
    best = [torch.full((count + 1,), MARK, dtype=torch.int64, device="cuda") for _ in range(2)]
    best.append(torch.full((count + 1,), 0xA5, dtype=torch.uint8, device="cuda"))
    coff = torch.full((count + 2,), MARK, dtype=torch.int64, device="cuda")
    cand = [None] * 3
    if lists:
        cand = [torch.full((capacity + 1,), MARK, dtype=torch.int64, device="cuda") for _ in range(2)]
        cand.append(torch.full((capacity + 1,), 0xA5, dtype=torch.uint8, device="cuda"))
    total = C.c_uint64(0)
    rc = ctx._L.bmx_index_map_device(ctx._h, idx._h, ptr(blob), blob.numel(), ptr(off), count, min_len, max_occ, k, 0,
                                     *[ptr(b) for b in best], ptr(coff), *[ptr(c) for c in cand], capacity, C.byref(total),
                                     current_stream())
    assert int(best[0][count]) == MARK and int(best[2][count]) == 0xA5 and int(coff[count + 1]) == MARK
    if lists:
        assert int(cand[0][capacity]) == MARK and int(cand[1][capacity]) == MARK and int(cand[2][capacity]) == 0xA5
    return rc, int(total.value), [b[:count] for b in best], coff[:count + 1], [c if c is None else c[:capacity] for c in cand]


def check_tiled(b, count, best, coff, cand=None):
    """`count` copies of the one-read answer, compared on the device."""
    import torch

    dev = lambda x, dt: torch.from_numpy(x.astype(np.int64)).cuda().to(dt)
    for g, x in zip(best, b.one[:3]):
        assert bool((g == dev(x, g.dtype)[0]).all())
    assert torch.equal(coff, torch.arange(count + 1, dtype=torch.int64, device="cuda") * PER_READ)
    if cand is not None:
        for g, x in zip(cand, b.one[4:]):
            assert torch.equal(g.view(count, PER_READ), dev(x, g.dtype).expand(count, PER_READ))


def small_calls_are_right(ctx, b):
    """A small seeds call, a small map call and a small locate call on the same context."""
    got = b.idx.seeds([READ, A * 5, b"ab"], 4, 0)
    assert got[0].tolist() == [0, 1, 2, 2] and got[1].tolist() == [0, 0] and got[2].tolist() == [16, 5]
    assert got[3].tolist() == [b.s.interval(READ)[0], b.s.interval(A * 5)[0]] and got[4].tolist() == [PER_READ, N_B - 4]
    rc, total, best, coff, cand = device_map(ctx, b.idx, 3, PER_READ, 3 * PER_READ)
    assert rc == host.OK and total == 3 * PER_READ
    check_tiled(b, 3, best, coff, cand)
    offsets, pos, total = b.idx.locate([A * 512, b"b", A * 500])
    assert total == 7212 and offsets.tolist() == [0, 3600, 3600, 7212] and pos.tolist() == list(range(3600)) + list(range(3612))


def test_candidate_workspace_across_256_mib(ctx, stairs_b):
    import torch

    b, count = stairs_b, 3000
    total = count * PER_READ
    assert 6 * 4 * total > 256 << 20
    rc, got, best, coff, cand = device_map(ctx, b.idx, count, PER_READ, total)
    assert rc == host.OK and got == total == ctx.last_index_map_candidates()
    check_tiled(b, count, best, coff, cand)
    small_calls_are_right(ctx, b)  # 3 reads, at once: the workspace is made again
    rc, got, best2, coff2, cand2 = device_map(ctx, b.idx, count, PER_READ, total)
    assert rc == host.OK and got == total
    for x, y in zip(best + [coff] + cand, best2 + [coff2] + cand2):  # no atomics: the same bytes in every run
        assert torch.equal(x, y)
    del cand, cand2
    torch.cuda.empty_cache()


def test_position_workspace_across_256_mib(ctx, stairs_b):
    import torch

    b, count = stairs_b, 900_000
    blob, off = reads_on_device(count)
    assert blob.numel() == 14_400_000 and 5 * 4 * blob.numel() > 256 << 20
    seed_off, qpos, ln, lo, cnt = b.idx.seeds((blob, off), 4, 0)
    assert torch.equal(seed_off, torch.arange(count + 1, dtype=torch.int64, device="cuda"))
    for g, v in ((qpos, 0), (ln, 16), (lo, b.s.interval(READ)[0]), (cnt, PER_READ)):
        assert g.numel() == count and bool((g == v).all())
    small_calls_are_right(ctx, b)
    rc, total, best, coff, _ = device_map(ctx, b.idx, count, 1, 0, lists=False)
    assert rc == host.OK and total == 0 and ctx.last_index_map_candidates() == 0
    assert bool((best[0] == -1).all()) and bool((best[1] == -1).all()) and bool((best[2] == mp.NO_HIT).all())
    assert bool((coff == 0).all())
    small_calls_are_right(ctx, b)


def test_the_candidate_cap(ctx, stairs_b):
    import torch

    b = stairs_b
    count = 32_768
    assert count * PER_READ == host.MAP_MAX_CANDIDATES == 1 << 27
    rc, total, best, coff, _ = device_map(ctx, b.idx, count, PER_READ, 0, lists=False)
    assert rc == host.OK and total == 1 << 27 and ctx.last_index_map_candidates() == 1 << 27
    check_tiled(b, count, best, coff)
    torch.cuda.empty_cache()
    rc, total, best, coff, _ = device_map(ctx, b.idx, count + 1, PER_READ, 0, lists=False)
    assert rc == host.ERR_ARG
    assert total == (1 << 27) + PER_READ == ctx.last_index_map_candidates()
    assert str(1 << 27) in host.lib().bmx_last_error().decode()
    small_calls_are_right(ctx, b)
