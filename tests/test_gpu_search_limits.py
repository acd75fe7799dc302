"""GPU suite for the thresholds of the approximate search (bmx_search_approx_device, csrc/bmx_approx_kernel.h) and the
dictionary search (bmx_dict_search_device, csrc/bmx_dict_kernel.h): tiles with exactly as many hits as the LDS pool
holds, one fewer and one more; capacities that end inside a tile that is walked twice; texts and base offsets past 2^32;
`lead` and `n_own` at their edges; many shapes on one context.

Every comparison is the complete list (positions, distances or pattern ids, n_matches) against tests/approx_oracle.py,
tests/dict_oracle.py or the C oracle (`port`), on the whole text or -- for the texts too large for that -- on the windows
around the plants, outside which no hit can lie (tests/limit_cases.py: plan_plants).  The per-tile counts of the tile
cases are proved on the CPU by tests/test_limit_cases_cpu.py; each case is REBUILT for every pointer offset, so the
counts hold in the aligned coordinates the kernels cut their tiles in.

The wrap of the status words' 22-bit tag takes 2^22 calls on one context; tests/test_gpu_streams.py
(test_tag_wrap_clears_the_status_words) reaches it with libbmx_exp.so's knob "ordered_seq" for every search with ordered
output.  The same searches with several tiles per workgroup, at large pieces and -- the class-pattern, gapped, k-mismatch
and regular-expression search -- past 4 GiB: tests/test_gpu_tile_geometry.py.
"""
import ctypes as C

import numpy as np
import pytest

import limit_cases as lc
from approx_oracle import approx_ends
from dict_oracle import DictIndex, dict_matches
from parallel_implementation_of_string_matching_algorithms_opencl_amd import corpus, host

pytestmark = pytest.mark.gpu

BIG_N = (4 << 30) + (64 << 20) + 5
BIG_BASE = (1 << 40) + 3


def _dev(ctx, data: bytes, offset: int = 0):
    """data on the device, starting `offset` bytes into a buffer (any alignment)."""
    import torch

    buf = torch.zeros(len(data) + offset + 16, dtype=torch.uint8, device=f"cuda:{ctx.device}")
    if data:
        buf[offset:offset + len(data)] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(buf.device)
    assert buf.data_ptr() % 16 == 0
    return buf[offset:offset + len(data)]


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _approx_raw(ctx, d_text, pat, k, out, dist, cap, lead=0, base=0, n=None):
    total = C.c_uint64(0)
    rc = ctx._L.bmx_search_approx_device(ctx._h, C.c_void_p(d_text.data_ptr()), d_text.numel() if n is None else n, lead,
                                         base, pat, len(pat), k, _ptr(out), _ptr(dist), cap, C.byref(total), None)
    return rc, int(total.value)


def _dict_raw(ctx, d, d_text, out, pid, cap, n_own=None, base=0, n=None):
    total = C.c_uint64(0)
    n = d_text.numel() if n is None else n
    rc = ctx._L.bmx_dict_search_device(ctx._h, d._h, C.c_void_p(d_text.data_ptr()), n, n if n_own is None else n_own, base,
                                       _ptr(out), _ptr(pid), cap, C.byref(total), None)
    return rc, int(total.value)


def _approx_full(ctx, d_text, pat, k, want_e, want_d, what, **kw):
    """One call with room for everything: rc, total, ends and distances against the expected lists."""
    import torch

    out = torch.full((want_e.size + 64,), -1, dtype=torch.int64, device=d_text.device)
    dist = torch.full((want_e.size + 64,), 255, dtype=torch.uint8, device=d_text.device)
    rc, total = _approx_raw(ctx, d_text, pat, k, out, dist, out.numel(), **kw)
    assert rc == host.OK and total == want_e.size, (what, rc, total, want_e.size)
    assert np.array_equal(out[:total].cpu().numpy(), want_e), what
    assert np.array_equal(dist[:total].cpu().numpy().astype(np.int64), want_d), what
    assert bool((out[total:] == -1).all()) and bool((dist[total:] == 255).all()), what


def _dict_full(ctx, d, d_text, want_p, want_i, what, **kw):
    import torch

    out = torch.full((want_p.size + 64,), -1, dtype=torch.int64, device=d_text.device)
    pid = torch.full((want_p.size + 64,), -1, dtype=torch.int32, device=d_text.device)
    rc, total = _dict_raw(ctx, d, d_text, out, pid, out.numel(), **kw)
    assert rc == host.OK and total == want_p.size, (what, rc, total, want_p.size)
    assert np.array_equal(out[:total].cpu().numpy(), want_p), what
    assert np.array_equal(pid[:total].cpu().numpy().astype(np.int64), want_i), what
    assert bool((out[total:] == -1).all()) and bool((pid[total:] == -1).all()), what


# ---- 1. the pool's edge ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [s[0] for s in lc.APPROX_TILE_SETS])
def test_approx_tiles_at_the_pool_edge(ctx, name):
    """Tiles of 2040..2056, 0, 1 and 4096 hits and the run sparse / 2049 / sparse / 2048 / 2049 / 0 / 2047, at pointer
    offsets 0, 1 and 15 (the case is rebuilt per offset), with the 32-bit word (m = 1 exact, m = 2 with one edit: three
    ends per plant) and the 64-bit word (m = 33 exact and with one edit; there 2600 stands in for 4096)."""
    ran = 0
    for case in lc.approx_tile_cases(name):
        want_e, want_d = approx_ends(case.text, case.pat, case.k)
        assert lc.bin_by_tile(want_e, case.tile, case.first, len(case.counts)) == case.counts
        _approx_full(ctx, _dev(ctx, case.text, case.first), case.pat, case.k, want_e, want_d, case.name)
        ran += 1
    assert ran == 2 * len(lc.OFFSETS)


@pytest.mark.parametrize("variant", lc.DICT_VARIANTS)
def test_dict_tiles_at_the_pool_edge(ctx, variant):
    """The same counts per 8 KiB tile with one pair per position, with two patterns at each position, and with single
    positions that carry 2047, 2048, 2049 and 4200 pairs through duplicate patterns ("dup": also the text in which
    those positions stand alone among a few single pairs)."""
    patterns, _ = lc.dict_variant(variant)
    ran = 0
    with ctx.dictionary(patterns) as d:
        for case in lc.dict_tile_cases(variant):
            assert case.patterns == patterns
            want_p, want_i = dict_matches(case.text, patterns)
            assert lc.bin_by_tile(want_p, case.tile, case.first, len(case.counts)) == case.counts
            _dict_full(ctx, d, _dev(ctx, case.text, case.first), want_p, want_i, case.name)
            ran += 1
    assert ran == len(lc.dict_count_lists(variant)) * len(lc.OFFSETS)


# ---- 2. capacity inside the second walk ----------------------------------------------------------------------------------

def _caps_around(prefix: int, count: int, total: int):
    return {0, 1, prefix, prefix + 1, prefix + count // 2, prefix + count, total - 1, total}


def _approx_capacities(ctx, d_text, pat, k, want_e, want_d, caps, what):
    import torch

    total = want_e.size
    dev = d_text.device
    we, wd = torch.from_numpy(want_e).to(dev), torch.from_numpy(want_d.astype(np.uint8)).to(dev)
    out = torch.empty(total + 64, dtype=torch.int64, device=dev)
    dist = torch.empty(total + 64, dtype=torch.uint8, device=dev)
    for cap in sorted(c for c in caps if 0 <= c <= total):
        out.fill_(-1)
        dist.fill_(255)
        rc, t = _approx_raw(ctx, d_text, pat, k, out, dist, cap)
        assert rc == (host.OK if cap == total else host.ERR_CAPACITY) and t == total, (what, cap, rc, t, total)
        assert torch.equal(out[:cap], we[:cap]) and torch.equal(dist[:cap], wd[:cap]), (what, cap)
        assert bool((out[cap:] == -1).all()) and bool((dist[cap:] == 255).all()), (what, cap)
        if cap:  # no distances wanted
            out.fill_(-1)
            rc, t = _approx_raw(ctx, d_text, pat, k, out, None, cap)
            assert rc == (host.OK if cap == total else host.ERR_CAPACITY) and t == total, (what, cap)
            assert torch.equal(out[:cap], we[:cap]) and bool((out[cap:] == -1).all()), (what, cap)
    rc, t = _approx_raw(ctx, d_text, pat, k, None, None, 0)  # count only
    assert rc == host.ERR_CAPACITY and t == total, (what, rc, t)


def _dict_capacities(ctx, d, d_text, want_p, want_i, caps, what):
    import torch

    total = want_p.size
    dev = d_text.device
    wp, wi = torch.from_numpy(want_p).to(dev), torch.from_numpy(want_i.astype(np.int32)).to(dev)
    out = torch.empty(total + 64, dtype=torch.int64, device=dev)
    pid = torch.empty(total + 64, dtype=torch.int32, device=dev)
    for cap in sorted(c for c in caps if 0 <= c <= total):
        out.fill_(-1)
        pid.fill_(-1)
        rc, t = _dict_raw(ctx, d, d_text, out, pid, cap)
        assert rc == (host.OK if cap == total else host.ERR_CAPACITY) and t == total, (what, cap, rc, t, total)
        assert torch.equal(out[:cap], wp[:cap]) and torch.equal(pid[:cap], wi[:cap]), (what, cap)
        assert bool((out[cap:] == -1).all()) and bool((pid[cap:] == -1).all()), (what, cap)
        if cap:  # no ids wanted
            out.fill_(-1)
            rc, t = _dict_raw(ctx, d, d_text, out, None, cap)
            assert rc == (host.OK if cap == total else host.ERR_CAPACITY) and t == total, (what, cap)
            assert torch.equal(out[:cap], wp[:cap]) and bool((out[cap:] == -1).all()), (what, cap)
    rc, t = _dict_raw(ctx, d, d_text, None, None, 0)  # count only
    assert rc == host.ERR_CAPACITY and t == total, (what, rc, t)


@pytest.mark.parametrize("name", ["m2_k1", "m33_k0_runs"])
def test_approx_capacity_inside_a_tile_walked_twice(ctx, name):
    """Capacities 0, 1, total - 1, total and, for each tile of the run 3 / 2049 / 5 / 2048 / 2049 / 0 / 2047: its prefix,
    prefix + 1, the middle of the tile, prefix + count.  The stored entries are the oracle's first `cap`, every slot
    from `cap` on keeps its sentinel, n_matches is the total, and count-only (NULL outputs) returns the total."""
    _, m, k, pat, plants, _ = next(s for s in lc.APPROX_TILE_SETS if s[0] == name)
    for first in (0, 15):
        case = lc.approx_tile_case(lc.SEQUENCE, m, k, first, pat, plants)
        want_e, want_d = approx_ends(case.text, pat, k)
        assert lc.bin_by_tile(want_e, case.tile, first, len(case.counts)) == case.counts
        caps = set()
        for t, count in enumerate(case.counts):
            caps |= _caps_around(case.prefix(t), count, want_e.size)
        _approx_capacities(ctx, _dev(ctx, case.text, first), pat, k, want_e, want_d, caps, (name, first))


@pytest.mark.parametrize("variant", ["two", "dup"])
def test_dict_capacity_inside_a_tile_walked_twice(ctx, variant):
    """As above for the dictionary.  "two": an odd capacity inside a dense tile ends between the two ids of one position;
    "dup": the capacities end among the 2049 and the 4200 ids of a single position."""
    counts = lc.DUP_SPARSE if variant == "dup" else lc.SEQUENCE
    patterns, _ = lc.dict_variant(variant)
    with ctx.dictionary(patterns) as d:
        for first in (0, 15):
            case = lc.dict_tile_case(counts, variant, first)
            want_p, want_i = dict_matches(case.text, patterns)
            assert lc.bin_by_tile(want_p, case.tile, first, len(counts)) == counts
            caps = set()
            for t, count in enumerate(counts):
                caps |= _caps_around(case.prefix(t), count, want_p.size)
            dense = counts.index(2049)
            between = next(c for c in range(case.prefix(dense) + 1000, want_p.size) if want_p[c - 1] == want_p[c])
            assert between < case.prefix(dense) + 2049  # inside the dense tile, between two ids of one position
            caps.add(between)
            _dict_capacities(ctx, d, _dev(ctx, case.text, first), want_p, want_i, caps, (variant, first))


def test_approx_capacity_on_dense_acgt(ctx):
    """The 8 MiB ACGT input of test_dense_tiles_walk_twice (every tile is walked twice).  The tile size depends on the
    device's occupancy, so the prefix / middle / end capacities are taken for tile 5 of every possible size."""
    spec = corpus.CorpusSpec("approx_dense", 8 * corpus.MiB, 8, 1, seed=0x5EEDA100, plant_period=0, boundary_period=0)
    pat, k = b"ACGTTGCA", 3
    want_e, want_d = approx_ends(spec.host_text().tobytes(), pat, k)
    assert want_e.size > spec.n // 16
    caps = {0, 1, want_e.size - 1, want_e.size}
    for ps in range(6, 12):
        tile = 256 << ps
        lo, hi = np.searchsorted(want_e, [5 * tile, 6 * tile])
        assert hi - lo > lc.STAGE
        caps |= {int(lo), int(lo) + 1, int(lo + hi) // 2, int(hi)}
    _approx_capacities(ctx, spec.device_text(ctx), pat, k, want_e, want_d, caps, "acgt")


def test_dict_capacity_on_dense_acgt(ctx):
    """The 8 MiB ACGT input of test_dense_output: two pairs at every position, every tile walked twice."""
    spec = corpus.CorpusSpec("dict_dense", 8 * corpus.MiB, 8, 1, seed=0x5EEDD200, plant_period=0, boundary_period=0)
    text = spec.host_text().tobytes()
    acgt = b"ACGT"
    pats = [bytes([a, b, c, e]) for a in acgt for b in acgt for c in acgt for e in acgt] + [bytes([x]) for x in acgt]
    want_p, want_i = dict_matches(text, pats)
    assert want_p.size == 2 * len(text) - 3
    first = 3
    caps = {0, 1, want_p.size - 1, want_p.size}
    for rs in range(0, 6):
        tile = lc.DICT_TILE << rs
        lo, hi = np.searchsorted(want_p, [5 * tile - first, 6 * tile - first])
        caps |= {int(lo), int(lo) + 1, int(lo + hi) // 2, int(lo + hi) // 2 + 1, int(hi)}
    with ctx.dictionary(pats) as d:
        _dict_capacities(ctx, d, _dev(ctx, text, first), want_p, want_i, caps, "acgt")


# ---- 3. past 4 GiB -----------------------------------------------------------------------------------------------------

def _edit(rng, pat: bytes, edits: int) -> bytes:
    s = bytearray(pat)
    for _ in range(edits):
        op = int(rng.integers(0, 3))
        i = int(rng.integers(0, len(s)))
        c = int(rng.integers(0x20, 0x7F))
        if op == 0:
            s[i] = c
        elif op == 1:
            s.insert(i, c)
        elif len(s) > 1:
            del s[i]
    return bytes(s)


def _device_planted_text(plan: lc.PlantPlan, seed: int):
    """The plan's text in HBM: background bytes 0x80..0xFF, filled and planted in chunks of 1 GiB."""
    import torch

    d_text = torch.empty(plan.n, dtype=torch.uint8, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(seed)
    step = 1 << 30
    for a in range(0, plan.n, step):
        b = min(a + step, plan.n)
        d_text[a:b] = torch.randint(0x80, 0x100, (b - a,), dtype=torch.uint8, device="cuda", generator=gen)
        lo, hi = np.searchsorted(plan.idx, [a, b])
        if hi > lo:
            d_text[a:b][torch.from_numpy(plan.idx[lo:hi] - a).cuda()] = torch.from_numpy(plan.val[lo:hi]).cuda()
    return d_text


def _big_plants(rng, m: int, copy, tail, cluster_copy=None):
    """Plants for a text of BIG_N bytes: about 3000 over the whole text, 400 more past 2^32, a cluster of back-to-back
    plants whose starts run from 2^32 - 2m to 2^32 + 2m, and `tail` (offset, bytes) at the very end.  copy() -> at most
    600 bytes."""
    centre = 1 << 32
    cluster, s = [], centre - 2 * m
    while s <= centre + 2 * m:
        c = (cluster_copy or copy)()
        cluster.append((s, c))
        s += len(c)
    clear = [(cluster[0][0], s), (BIG_N - 4096, BIG_N)]
    offs = sorted(lc.spread_offsets(0, BIG_N, 3000, 640, rng, clear) +
                  lc.spread_offsets(centre + (1 << 20), BIG_N - (1 << 20), 400, 640, rng, clear))
    apart = [p for j, p in enumerate(offs) if j == 0 or p >= offs[j - 1] + 2 * 640]
    return cluster + [(p, copy()) for p in apart] + list(tail)


@pytest.mark.parametrize("pat,k", [(b"approximate-sear", 3), (b"a pattern of forty bytes for 64-bit word", 2)])
def test_approx_text_beyond_4GiB(ctx, pat, k):
    """4 GiB + 64 MiB + 5 bytes.  Plants are copies of the pattern with 0 .. k + 1 edits; the expected list is the
    oracle's on the windows of m + k bytes around them.  At this size a tile is 512 KiB of ends, so the last tile
    holds the text's last 5 ends: those of the plant that ends at the last byte; the plant in front of it ends in the
    tile before."""
    import torch

    m = len(pat)
    assert m in (16, 40)
    rng = np.random.default_rng(0xB16 + m)
    tail = [(BIG_N - 300, _edit(rng, pat, 1)), (BIG_N - m, pat)]
    plants = _big_plants(rng, m, lambda: _edit(rng, pat, int(rng.integers(0, k + 2))), tail,
                         cluster_copy=lambda: _edit(rng, pat, int(rng.integers(0, 2))))
    plan = lc.plan_plants(BIG_N, plants, m + k)
    d_text = _device_planted_text(plan, 0xB16A)
    exp_e, exp_d = [], []
    for lo, length in plan.windows:
        e, d = approx_ends(d_text[lo:lo + length].cpu().numpy().tobytes(), pat, k)
        exp_e.append(e + lo)
        exp_d.append(d)
    exp_e, exp_d = np.concatenate(exp_e), np.concatenate(exp_d)
    assert exp_e.size > 3000 and int((exp_e > (1 << 32)).sum()) > 100 and int((exp_e < (1 << 32)).sum()) > 100
    assert int(exp_e[-1]) == BIG_N - 1 and int(exp_d[-1]) == 0
    assert ((exp_e >= (1 << 32) - 2 * m) & (exp_e <= (1 << 32) + 3 * m)).sum() >= 4
    _approx_full(ctx, d_text, pat, k, exp_e, exp_d, "4 GiB")
    del d_text
    torch.cuda.empty_cache()


def test_dict_text_beyond_4GiB(ctx):
    """The 65,536 patterns of test_one_gib_with_planted_dictionary on 4 GiB + 64 MiB + 5 bytes.  A tile is 256 KiB of
    match starts, so the last tile is the last 5 bytes: a 2-byte pattern starts there, a 3-byte pattern ends at the last
    byte.  The expected list is the dictionary's on every run of plant bytes (the background is in no pattern)."""
    import torch

    rng = np.random.default_rng(0xD1C7B16)
    K = 65536
    lens = rng.integers(4, 33, K)
    lens[:64] = rng.integers(100, 513, 64)
    lens[64:96] = rng.integers(1, 4, 32)
    pats = [(rng.integers(0x20, 0x7F, int(m))).astype(np.uint8).tobytes() for m in lens]
    two = next(p for p in pats[64:96] if len(p) == 2)
    three = next(p for p in pats[64:96] if len(p) == 3)
    tail = [(BIG_N - 5, two), (BIG_N - 3, three)]
    plants = _big_plants(rng, 16, lambda: pats[int(rng.integers(0, K))], tail)
    plan = lc.plan_plants(BIG_N, plants, 0)
    d_text = _device_planted_text(plan, 0xD1C7)
    index = DictIndex(pats)
    memo = {}
    exp_p, exp_i = [], []
    for lo, length in plan.windows:
        w = d_text[lo:lo + length].cpu().numpy().tobytes()
        if w not in memo:
            memo[w] = index.matches(w)
        p, i = memo[w]
        exp_p.append(p + lo)
        exp_i.append(i)
    exp_p, exp_i = np.concatenate(exp_p), np.concatenate(exp_i)
    assert exp_p.size > 3000 and int((exp_p > (1 << 32)).sum()) > 100 and int((exp_p < (1 << 32)).sum()) > 100
    assert BIG_N - 5 in exp_p[-12:].tolist() and BIG_N - 3 in exp_p[-12:].tolist() and int(exp_p[-1]) >= BIG_N - 3
    assert ((exp_p >= (1 << 32) - 32) & (exp_p <= (1 << 32) + 32)).sum() >= 2
    with ctx.dictionary(pats) as d:
        _dict_full(ctx, d, d_text, exp_p, exp_i, "4 GiB")
    del d_text
    torch.cuda.empty_cache()


def test_multi_text_beyond_4GiB(ctx, port):
    """bmx_search_device_multi, K = 8, on the synthetic corpus at 4 GiB + 64 MiB + 5 bytes.  Pattern 0 is the planted
    one (a forced plant lies across 2^32): its list is planted_offsets().  The seven others are 20 to 64 bytes cut from
    the text around 2^32 (before, across and behind it), each with at least 13 bytes outside every plant; the chance
    that one of them occurs a second time in 4 GiB of 95-symbol text is below 1e-15, so their lists are the C oracle's
    on the 2 MiB window around 2^32."""
    import torch

    spec = corpus.CorpusSpec("4GiB+", BIG_N, 16, 0, 0x5EED0B16, 1 << 19, 1 << 28, -1)
    d_text = spec.device_text(ctx)
    a = (1 << 32) - (1 << 20)
    chunk = d_text[a:a + (2 << 20)].cpu().numpy()
    mid = 1 << 20
    cuts = [(mid - 5000, 33), (mid - 20, 40), (mid - 63, 64), (mid, 24), (mid + 1, 20), (mid + 70000, 48), (mid - 1, 30)]
    pats = [spec.pattern()] + [chunk[s:s + m].tobytes() for s, m in cuts]
    out = torch.full((1 << 16,), -1, dtype=torch.int64, device=d_text.device)
    lists = [x.cpu().numpy().astype(np.uint64) for x in ctx.search_device_multi(d_text, pats, out=out)]
    want = spec.planted_offsets()
    assert want.size > 8000 and int((want > np.uint64(1 << 32)).sum()) > 100
    assert np.array_equal(lists[0], want) and int(lists[0][-1]) == BIG_N - 16
    window = lists[0][(lists[0] >= a) & (lists[0] <= a + (2 << 20) - 16)]
    assert np.array_equal(port.search(chunk, pats[0]) + np.uint64(a), window)
    for j, (s, m) in enumerate(cuts, start=1):
        ow = port.search(chunk, pats[j]) + np.uint64(a)
        assert a + s in ow.tolist()
        assert np.array_equal(lists[j], ow), (j, lists[j], ow)
    assert sum(x.size for x in lists) == want.size + len(cuts)
    assert bool((out[sum(x.size for x in lists):] == -1).all())
    del d_text, out
    torch.cuda.empty_cache()


# ---- 4. a large base offset ----------------------------------------------------------------------------------------------

def _shard_spec():
    return corpus.CorpusSpec("limits_shards", 16 * corpus.MiB, 16, 0, seed=0x5EEDB400, plant_period=1 << 14,
                             boundary_period=1 << 21)


@pytest.mark.parametrize("offset", [0, 7])
def test_approx_shards_with_a_base_offset_past_2_40(ctx, offset):
    """16 MiB, base_offset = 2^40 + 3.  Views that begin m + k - 1 bytes before their first end (lead = m + k - 1)
    concatenate to the oracle's list of the whole text plus the offset; a view with lead = 0 gives the oracle's list of
    the view's own bytes (alignments cannot begin before it)."""
    spec = _shard_spec()
    text = spec.host_text().tobytes()
    pat = bytearray(spec.pattern())
    pat[5] = 0x7E  # one substitution against the plants
    pat, k = bytes(pat), 2
    m, n = len(pat), len(text)
    want_e, want_d = approx_ends(text, pat, k)
    assert want_e.size > 1000
    d_text = _dev(ctx, text, offset)
    cuts = [0, 5 * corpus.MiB + 3, 5 * corpus.MiB + 4, 11 * corpus.MiB, n]
    for a, b in zip(cuts[:-1], cuts[1:]):
        lead = min(a, m + k - 1)
        sel = (want_e >= a) & (want_e < b)
        _approx_full(ctx, d_text[a - lead:b], pat, k, want_e[sel] + BIG_BASE, want_d[sel], ("lead", a, b), lead=lead,
                     base=BIG_BASE + a - lead)
    a, b = 11 * corpus.MiB, 13 * corpus.MiB + 1
    own_e, own_d = approx_ends(text[a:b], pat, k)
    _approx_full(ctx, d_text[a:b], pat, k, own_e + (BIG_BASE + a), own_d, "lead 0", lead=0, base=BIG_BASE + a)


@pytest.mark.parametrize("offset", [0, 7])
def test_dict_shards_with_a_base_offset_past_2_40(ctx, offset):
    """16 MiB, base_offset = 2^40 + 3.  Shards with a halo concatenate to the whole list plus the offset; then views whose
    n_own ends 0, 1, 2 and 3 bytes before a tile end (a multiple of 256 KiB in aligned coordinates: a tile end for every
    tile size), each with 0, 1, 2 and 3 bytes of view behind n_own, against the oracle on the view."""
    spec = _shard_spec()
    h = spec.host_text()
    text = h.tobytes()
    pat = spec.pattern()
    edge = (1 << 20) - offset  # view coordinate of an aligned multiple of 256 KiB
    pats = [pat, pat[:5], pat[4:], h[123456:123456 + 200].tobytes(), b"~", pat[-3:], h[9_000_000:9_000_004].tobytes(),
            text[edge - 3:edge + 1], text[edge - 2:edge], text[edge - 1:edge + 4], text[edge - 4:edge - 1]]
    halo = max(len(p) for p in pats) - 1
    n = len(text)
    want_p, want_i = dict_matches(text, pats)
    assert want_p.size > 1000
    d_text = _dev(ctx, text, offset)
    with ctx.dictionary(pats) as d:
        cuts = [0, 3 * corpus.MiB + 3, 11 * corpus.MiB, 11 * corpus.MiB + 1, n]
        for a, b in zip(cuts[:-1], cuts[1:]):
            sel = (want_p >= a) & (want_p < b)
            _dict_full(ctx, d, d_text[a:min(b + halo, n)], want_p[sel] + BIG_BASE, want_i[sel], ("halo", a, b), n_own=b - a,
                       base=BIG_BASE + a)
        for before in range(4):
            for behind in range(4):
                n_own = edge - before
                view = text[:n_own + behind]
                vp, vi = dict_matches(view, pats, n_own)
                _dict_full(ctx, d, d_text[:len(view)], vp + BIG_BASE, vi, ("n_own", before, behind), n_own=n_own, base=BIG_BASE)


@pytest.mark.parametrize("offset", [0, 7])
def test_multi_shards_with_a_base_offset_past_2_40(ctx, port, offset):
    """bmx_search_device_multi over shards of the 16 MiB text with base_offset = 2^40 + 3 and a halo of max(m) - 1 bytes:
    every pattern's lists concatenate to the C oracle's list of the whole text plus the offset."""
    import torch

    spec = _shard_spec()
    h = spec.host_text()
    pats = [spec.pattern(), h[777:777 + 31].tobytes(), spec.pattern()[:6], h[5 * corpus.MiB:5 * corpus.MiB + 9].tobytes()]
    halo = max(len(p) for p in pats) - 1
    n = h.size
    d_text = _dev(ctx, h.tobytes(), offset)
    want = [port.search(h, p) + np.uint64(BIG_BASE) for p in pats]
    assert want[0].size > 1000
    got = [[] for _ in pats]
    cuts = [0, 5 * corpus.MiB + 3, 5 * corpus.MiB + 4, 11 * corpus.MiB, n]
    out = torch.empty(1 << 18, dtype=torch.int64, device=d_text.device)
    for a, b in zip(cuts[:-1], cuts[1:]):
        lists = ctx.search_device_multi(d_text[a:min(b + halo, n)], pats, n_own=b - a, base_offset=BIG_BASE + a, out=out)
        for j, x in enumerate(lists):
            got[j].append(x.cpu().numpy().astype(np.uint64))
    for j in range(len(pats)):
        assert np.array_equal(np.concatenate(got[j]), want[j]), j


# ---- 5. lead and n_own at their edges ------------------------------------------------------------------------------------

SMALL_N = (1, 15, 16, 17, 100)


@pytest.mark.parametrize("offset", [0, 5, 15])
def test_approx_lead_edges_on_small_texts(ctx, offset):
    """lead in {0, 1, m + k - 1, n - 1, n, n + 1} on texts of 1, 15, 16, 17 and 100 bytes: the ends >= lead of the
    oracle's list, plus the base offset.  lead = n reports nothing and returns BMX_OK; lead = n + 1 is outside the view
    and is the argument error include/bmx.h documents (BMX_ERR_ARG, as tests/test_approx_cpu.py asserts without a
    device)."""
    rng = np.random.default_rng(50 + offset)
    for n in SMALL_N:
        text = (rng.integers(0, 2, n) + 0x61).astype(np.uint8).tobytes()
        d_text = _dev(ctx, text, offset)
        for m, k in ((1, 0), (2, 1), (4, 1), (8, 2), (33, 1), (40, 30)):
            pat = (rng.integers(0, 2, m) + 0x61).astype(np.uint8).tobytes()
            want_e, want_d = approx_ends(text, pat, k)
            for lead in sorted({0, 1, m + k - 1, max(n - 1, 0), n, n + 1}):
                if lead > n:
                    rc, total = _approx_raw(ctx, d_text, pat, k, None, None, 0, lead=lead, base=7)
                    assert rc == host.ERR_ARG, (n, m, k, lead)
                    continue
                sel = want_e >= lead
                _approx_full(ctx, d_text, pat, k, want_e[sel] + 7, want_d[sel], (n, m, k, lead), lead=lead, base=7)
                if lead >= n:
                    assert not sel.any()


@pytest.mark.parametrize("offset", [0, 5, 15])
def test_dict_n_own_edges_on_small_texts(ctx, offset):
    """n_own in {0, 1, n - 3 .. n, n + 10} with patterns of 1 to 5 bytes that all end at the last byte of the view (the
    4-byte key of the last starts reaches past the view), on texts of 1, 15, 16, 17 and 100 bytes and on views that end
    within 3 bytes of the first tile's end."""
    rng = np.random.default_rng(60 + offset)
    pats = [b"z", b"yz", b"xyz", b"wxyz", b"vwxyz", b"zz", b"v"]
    with ctx.dictionary(pats) as d:
        for n in SMALL_N + tuple(lc.DICT_TILE - offset + j for j in (-3, -2, -1, 0, 1, 4)):
            text = bytearray((rng.integers(0, 5, n) + 0x76).astype(np.uint8).tobytes())  # v .. z
            text[max(n - 5, 0):] = b"vwxyz"[-n:]
            text = bytes(text)
            d_text = _dev(ctx, text, offset)
            for n_own in sorted({0, 1, n + 10} | {x for x in range(n - 3, n + 1) if x >= 0}):
                want_p, want_i = dict_matches(text, pats, n_own)
                if n_own >= n:
                    assert want_p.size and int(want_p[-1]) == n - 1 and int(want_i[-1]) == 0
                _dict_full(ctx, d, d_text, want_p + 9, want_i, (n, n_own), n_own=n_own, base=9)


# ---- 6. one context, many shapes -----------------------------------------------------------------------------------------

def test_one_context_many_shapes(ctx, port):
    """60 calls in a seeded random order on ONE new context: approximate search with the 32- and the 64-bit word, two
    dictionaries and the exact search, on texts of 0 bytes to 48 MiB (the per-tile status arrays grow past their first
    1024 words and are reused under new tags), a quarter of them count-only or with half the capacity they need
    (BMX_ERR_CAPACITY).  Texts up to 300,000 bytes are checked against the oracles in full; the planted ones (3, 16
    and 48 MiB) on the windows around their plants."""
    import torch

    rng = np.random.default_rng(0x60CA115)
    alpha = np.frombuffer(b"abcd", np.uint8)
    p32 = alpha[rng.integers(0, 4, 12)].tobytes()
    p64 = alpha[rng.integers(0, 4, 40)].tobytes()
    exact = alpha[rng.integers(0, 4, 9)].tobytes()
    dict1 = [p32[:7], b"abca", b"dd", exact, p64[3:30], b"cab"]
    dict2 = [alpha[rng.integers(0, 4, int(rng.integers(3, 13)))].tobytes() for _ in range(300)]
    kinds = {"a32": (p32, 2), "a64": (p64, 2), "d1": dict1, "d2": dict2, "x": exact}
    reach = 40 + 2

    def expect(kind, pieces):
        """pieces: [(offset, bytes)] that hold every hit."""
        ps, qs = [], []
        for lo, w in pieces:
            if kind in ("a32", "a64"):
                p, q = approx_ends(w, *kinds[kind])
            elif kind == "x":
                p, q = dict_matches(w, [exact])
            else:
                p, q = dict_matches(w, kinds[kind])
            ps.append(p + lo)
            qs.append(q)
        return (np.concatenate(ps), np.concatenate(qs)) if ps else (np.zeros(0, np.int64), np.zeros(0, np.int64))

    texts = []  # (device text, pieces)
    own = host.Context(0)
    try:
        for j, n in enumerate((0, 1, 700, 40000, 300000)):
            t = alpha[rng.integers(0, 4, n)].copy()
            for at in range(50, n - 64, 3001):
                src = (p32, p64, exact, dict1[4])[at % 4]
                t[at:at + len(src)] = np.frombuffer(src, np.uint8)
            texts.append((_dev(own, t.tobytes(), (3 * j) % 16), [(0, t.tobytes())]))
        for n, count in ((3 * corpus.MiB + 5, 300), (16 * corpus.MiB, 500), (48 * corpus.MiB, 700)):
            srcs = (p32, p64, exact) + tuple(dict1) + tuple(dict2[:20])
            offs = lc.spread_offsets(0, n - 64, count, 64, rng)
            plants = [(p, _edit_abcd(rng, srcs[int(rng.integers(0, len(srcs)))])) for p in offs] + [(n - 40, p64)]
            plan = lc.plan_plants(n, plants, reach)
            d_text = _device_planted_text(plan, n)
            texts.append((d_text, [(lo, d_text[lo:lo + ln].cpu().numpy().tobytes()) for lo, ln in plan.windows]))
        memo = {}
        d1, d2 = own.dictionary(dict1), own.dictionary(dict2)
        seen = set()
        first_calls = [(2, "a32"), (7, "a32"), (0, "a64"), (1, "d2"), (7, "d1"), (7, "a64"), (7, "x"), (6, "d2")]
        for call in range(60):
            ti = int(rng.integers(0, len(texts)))
            kind = ("a32", "a64", "d1", "d2", "x")[int(rng.integers(0, 5))]
            mode = ("full", "full", "full", "count", "half")[int(rng.integers(0, 5))]
            if call < len(first_calls):  # small texts first, then the largest: both status arrays grow, both words follow
                (ti, kind), mode = first_calls[call], "full"
            d_text, pieces = texts[ti]
            if (ti, kind) not in memo:
                memo[(ti, kind)] = expect(kind, pieces)
            wp, wq = memo[(ti, kind)]
            total = wp.size
            cap = {"full": total + 8, "count": 0, "half": total // 2}[mode]
            want_rc = host.OK if cap >= total else host.ERR_CAPACITY
            what = (call, ti, kind, mode, total)
            seen.add((kind, mode))
            out = torch.full((cap + 8,), -1, dtype=torch.int64, device=d_text.device) if cap else None
            if kind in ("a32", "a64"):
                aux = torch.full((cap + 8,), 255, dtype=torch.uint8, device=d_text.device) if cap else None
                rc, t = _approx_raw(own, d_text, kinds[kind][0], kinds[kind][1], out, aux, cap)
            elif kind in ("d1", "d2"):
                aux = torch.full((cap + 8,), -1, dtype=torch.int32, device=d_text.device) if cap else None
                rc, t = _dict_raw(own, d1 if kind == "d1" else d2, d_text, out, aux, cap)
            else:
                aux = None
                keep = out if out is not None else torch.full((1,), -1, dtype=torch.int64, device=d_text.device)
                pos, t = own.search_device(d_text, exact, out=keep, capacity=cap)
                rc = host.OK if t <= cap else host.ERR_CAPACITY
            assert rc == want_rc and t == total, (what, rc, t)
            got = min(cap, total)
            if cap and kind == "x" and cap < total:
                continue  # bmx_search_device promises the count when the capacity is too small, not which offsets it keeps
            if cap:
                assert np.array_equal(out[:got].cpu().numpy(), wp[:got]), what
                assert bool((out[got:] == -1).all()), what
                if aux is not None:
                    assert np.array_equal(aux[:got].cpu().numpy().astype(np.int64), wq[:got]), what
        assert len(seen) >= 12 and {m for _, m in seen} == {"full", "count", "half"}
        d1.close()
        d2.close()
    finally:
        own.close()
    del texts
    torch.cuda.empty_cache()


def _edit_abcd(rng, src: bytes) -> bytes:
    """src with zero to two of its bytes replaced by other letters of the alphabet."""
    s = bytearray(src)
    for _ in range(int(rng.integers(0, 3))):
        s[int(rng.integers(0, len(s)))] = 0x61 + int(rng.integers(0, 4))
    return bytes(s)
