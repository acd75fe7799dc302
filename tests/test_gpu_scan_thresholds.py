"""GPU suite: the match list at the thresholds that switch how a search produces it, against the oracle.

Each search's list goes through one of several machines, and each is switched by a threshold: the per-tile parking
ledger (`stage_cap`, 64..1024 entries by variant and m) and the dense-tile fill pass behind it; the 8192 position buckets
of 8 entries, the in-LDS sort up to 8192 entries and the radix sort beyond; the capacity contract; the automatic kernel
choice, which goes by the text's alphabet as sampled by the previous search on the same (pointer, length); the shared
stage of the multi-pattern pass; and the stolen tail of the product kernels on texts large enough to reach it.  The
tests here put results exactly on those edges.  Every list is compared with the port oracle (`port.search`), together
with the true total.

Most texts are a background of bytes >= 0x80 with printable patterns planted in them.  No pattern byte is >= 0x80, so
the plants are the only matches, and a test places exactly the count it wants where it wants it.  Every pattern starts
with a byte that occurs nowhere else in it, so it has no proper border and copies laid end to end match once each.
"""
import ctypes as C

import numpy as np
import pytest

from parallel_implementation_of_string_matching_algorithms_opencl_amd import corpus, host
from test_gpu_parity import PRODUCT_VARIANTS

pytestmark = pytest.mark.gpu

AUTO = -1
SAD_SLOTS = (87, 88)  # quad-SAD skip loops: lanes own 80-byte filter segments
SAD_SEG = 80  # bmx_scan_common.h SAD_SEG: a constant of the walker that bmx_scan_geometry does not report
# Matches in one tile: every stage_cap that stage_cap_for (bmx_scan.hip) can choose, and its neighbours.
KS = [63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025]
# The slots pick_variant can return.  Slots 79 and 82 need safe non-canonical tables on a large alphabet (82 only once the
# text's alphabet is known, i.e. on a resident text); 54 needs a text over 2 or 3 symbols and m = 6..8.
AUTO_REACHABLE = {0, 2, 29, 53, 54, 79, 82, 87, 88}
BG_BYTES = 96 << 20
BUCKETS = 8192  # ORDER_BUCKETS (bmx_scan_common.h), 8 entries each


@pytest.fixture(scope="module")
def background(built):
    """Bytes 0x80..0xff: never in a pattern."""
    return np.random.default_rng(0xB6).integers(0x80, 0x100, BG_BYTES).astype(np.uint8)


class Rig:
    """One context, one persistent device text buffer and one output buffer (so that a text of a given length stays at
    one address, as a resident text does)."""

    def __init__(self, port, ctx=None):
        import torch

        self.torch = torch
        self.port = port
        self.ctx = ctx if ctx is not None else host.Context(0)
        self.d = torch.empty(BG_BYTES + 4096, dtype=torch.uint8, device="cuda")
        self.out = torch.empty(1 << 21, dtype=torch.int64, device="cuda")

    def close(self):
        self.ctx.close()

    def put(self, text):
        d = self.d[: text.size]
        d.copy_(self.torch.from_numpy(text))
        return d

    def check(self, text, pat, what, d=None, **kw):
        """Search text (uploaded unless d is given) and compare list and total with the oracle; returns the list."""
        if d is None:
            d = self.put(text)
        pos, total = self.ctx.search_device(d, pat, out=self.out, **kw)
        got = pos.cpu().numpy().astype(np.uint64)
        want = self.port.search(text, pat)
        assert total == want.size and got.size == want.size and np.array_equal(got, want), (what, total, want.size)
        return got

    def raw(self, d, pat, cap):
        """bmx_search_device itself: (rc, total) for a capacity of `cap` entries of self.out."""
        total = C.c_uint64(0)
        stream = C.c_void_p(self.torch.cuda.current_stream().cuda_stream)
        rc = self.ctx._L.bmx_search_device(self.ctx._h, C.c_void_p(d.data_ptr()), d.numel(), d.numel(), 0, pat, len(pat),
                                           None, None, C.c_void_p(self.out.data_ptr()), cap, C.byref(total), stream)
        return rc, int(total.value)

    def capacity_contract(self, text, pat, what):
        """capacity = total, total - 1, total // 2, 2, 1 and 0: the true total always; BMX_ERR_CAPACITY exactly when the
        total does not fit; `capacity` entries (or all of them), strictly ascending, each one of the oracle's."""
        d = self.put(text)
        want = self.port.search(text, pat)
        total = int(want.size)
        for cap in sorted({total, total - 1, total // 2, 2, 1, 0}):
            if cap < 0:
                continue
            self.out.fill_(-1)
            rc, got_total = self.raw(d, pat, cap)
            assert got_total == total, (what, cap, got_total, total)
            assert rc == (host.ERR_CAPACITY if total > cap else host.OK), (what, cap, total, rc)
            got = self.out[: min(cap, total)].cpu().numpy().astype(np.uint64)
            assert got.size == min(cap, total)
            assert np.all(got[1:] > got[:-1]), (what, cap, "not strictly ascending")
            assert np.all(np.isin(got, want)), (what, cap, "entries that are not matches")


def _pattern(rng, m, lead=0x21, zero=False):
    """m printable bytes; `lead` first and nowhere else (body bytes are 0x30..0x7e), so the pattern has no border."""
    p = rng.integers(0x30, 0x7F, m).astype(np.uint8)
    p[0] = lead
    if zero:
        p[1] = 0
    return p.tobytes()


def _plant(text, pat, starts):
    m = len(pat)
    starts = np.asarray(starts, dtype=np.int64)
    idx = (starts[:, None] + np.arange(m, dtype=np.int64)[None, :]).ravel()
    text[idx] = np.tile(np.frombuffer(pat, dtype=np.uint8), starts.size)
    return text


def _lengths(slot):
    """(m, zero byte) that reach the slot's own walker when it is set explicitly (pick_variant): the q-gram walkers need
    canonical tables and m >= 4 without being a short pattern (a 4-byte pattern has to hold a zero byte), the 8-gram one
    m >= 8; the quad-SAD slots take any m; the others have a short-pattern kernel of their own for m = 1..4."""
    every = [(1, False), (2, False), (3, False), (4, False), (4, True), (5, False), (8, False), (9, False), (16, False),
             (64, False), (512, False)]
    if slot in (24, 25, 54):
        return [x for x in every if x[0] >= 5 or x == (4, True)]
    if slot == 53:
        return [x for x in every if x[0] >= 8]
    return every


def _tile(rig, background, pat):
    """Tile bytes of the kernel that searches `pat` on this background: bmx_scan_geometry of the explicitly set slot, or --
    under the automatic choice -- of what the second search of a 1 MiB background ran (the resident-text choice)."""
    m = len(pat)
    for _ in range(2):
        rig.check(background[:1 << 20], pat, (m, "probe"))
    return rig.ctx.geometry(m)["tile_bytes"]


# ---------------------------------------------------------------- 1. parking capacity per tile
@pytest.mark.parametrize("slot", PRODUCT_VARIANTS + [AUTO])
def test_parking_capacity_per_tile(port, background, slot):
    """Exactly k matches in one tile for k around every parking cap, on every product kernel and the automatic choice:
    spread over the tile, packed into one wave piece (and into one lane's 80-byte filter segment on the quad-SAD slots),
    and k in every tile of a text with more tiles than workgroups, so that each workgroup's running stage count crosses
    the cap over the tiles it walks.  A k that does not fit the tile / piece / segment at this m is skipped."""
    rig = Rig(port)
    rng = np.random.default_rng(4000 + slot)
    try:
        rig.ctx.set_variant(slot)
        for m, zero in _lengths(slot):
            pat = _pattern(rng, m, zero=zero)
            n = 5 * _tile(rig, background, pat) + m  # five tiles of the kernel that runs
            base = background[:n]
            # the second search on this (pointer, length) runs what every later one does; its geometry is the one to place by
            for _ in range(2):
                rig.check(base, pat, (slot, m, "empty"))
            ran = rig.ctx.last_variant()
            if slot != AUTO:
                assert ran == slot, (slot, m, ran)
            g = rig.ctx.geometry(m)
            tile, piece = g["tile_bytes"], 64 * g["seg"]
            assert 2 * tile <= n
            areas = [("spread", tile), ("piece", piece)]
            if ran in SAD_SLOTS:
                areas.append(("lane", SAD_SEG))
            for name, room in areas:
                for k in KS:
                    if k * m > room:  # k copies of m bytes do not fit this area
                        continue
                    stride = room // k if name == "spread" else m
                    text = _plant(base.copy(), pat, tile + np.arange(k) * stride)
                    rig.check(text, pat, (slot, m, zero, name, k))
        # every tile: k matches spread over each of (2 x grid + 3) tiles
        for m, zero in [x for x in _lengths(slot) if x[0] >= 2][:1] + [(16, False)]:
            pat = _pattern(rng, m, zero=zero)
            rig.check(background[:1 << 20], pat, (slot, m, "probe"))
            rig.check(background[:1 << 20], pat, (slot, m, "probe"))
            g = rig.ctx.geometry(m)
            tile = g["tile_bytes"]
            tiles = 2 * g["grid"] + 3
            n = tiles * tile + m
            assert n <= BG_BYTES
            for k in KS:
                if k * m > tile:
                    continue
                stride = tile // k
                starts = (np.arange(tiles)[:, None] * tile + np.arange(k)[None, :] * stride).ravel()
                text = _plant(background[:n].copy(), pat, starts)
                got = rig.check(text, pat, (slot, m, "every tile", k))
                assert got.size == tiles * k
    finally:
        rig.close()


# ---------------------------------------------------------------- 2 + 3. ordering paths and the capacity contract
def _clusters(background, pat, total, tile, per_tile=56, at=1000):
    """`total` matches packed end to end, `per_tile` at the front of each tile: position buckets overflow, tiles do not
    fill their parking buffers."""
    m = len(pat)
    tiles = (total + per_tile - 1) // per_tile
    n = tiles * tile + m
    j = np.arange(total)
    starts = (j // per_tile) * tile + at + (j % per_tile) * m
    return _plant(background[:n].copy(), pat, starts)


@pytest.mark.parametrize("m", [1, 3, 16, 64])
def test_ordering_paths_at_their_edges(port, background, m):
    """Under the automatic choice: 8 matches in each of 1024 position buckets (ordered from the buckets, no sort) and
    the same with a 9th match in one of them (the bucket overflows: sorted); 8 matches in every one of the 8192 buckets;
    8191 / 8192 / 8193 and 65,535 / 65,536 / 65,537 clustered matches (bucket overflow: the in-LDS sort, the radix sort);
    n_starts at 8192 << s and +-1 (the bucket width steps); base offsets on both sides of a power of two (the radix key
    width steps).  Texts are sized so that no tile holds more matches than it can park.  The capacity contract is
    checked on the bucket-ordered, in-LDS-sorted and radix-sorted results.  (Patterns of 1-3 bytes may be laid out by
    their fill pass instead of sorted: bmx_search_device_finish's rule.)

    The buckets take a workgroup's parked matches only while (matches it parks) x (workgroups) <= 4 x 8192
    (bmx_scan_kernel.h, the end of the scan loop): 65,536 matches spread evenly over 256 workgroups exceed that, and the
    list is sorted by design.  The sort-free path and its 8-to-9 edge are pinned with 8 matches in every eighth bucket
    (8192 in all)."""
    rig = Rig(port)
    rng = np.random.default_rng(5000 + m)
    try:
        pat = _pattern(rng, m)
        w = 1 << 13  # bucket width at n_starts = 8192 << 13
        n = BUCKETS * w + m - 1
        r = rng.integers(0, 256, (BUCKETS, 8))
        starts = (np.arange(BUCKETS)[:, None] * w + np.arange(8)[None, :] * 1024 + r).ravel()
        # 8 in every eighth bucket: ordered from the buckets, no sort
        sparse = _plant(background[:n].copy(), pat, starts.reshape(BUCKETS, 8)[::8].ravel())
        for rep in range(2):  # first search on the text and the resident one
            got = rig.check(sparse, pat, (m, "8 per bucket, every 8th", rep))
            assert got.size == 8192 and not rig.ctx.last_search_sorted(), (m, rep)
        rig.capacity_contract(sparse, pat, (m, "bucket-ordered"))
        # ... and a 9th in one of those buckets (4320 = 8 x 540): it overflows, the list is sorted (m = 1..3: or laid out by the
        # fill pass) and must still be exact -- a 9th entry stored past the bucket's 8 would land in the next bucket's slot 0
        nine = _plant(sparse.copy(), pat, [4320 * w + 3 * 1024 + 600])
        got = rig.check(nine, pat, (m, "one bucket with 9"))
        assert got.size == 8193
        if m >= 4:
            assert rig.ctx.last_search_sorted(), m
        rig.capacity_contract(nine, pat, (m, "one bucket with 9"))
        # 8 in every bucket: more than the buckets take from the parking buffers (see the docstring), ordered all the same
        text = _plant(background[:n].copy(), pat, starts)
        for rep in range(2):
            got = rig.check(text, pat, (m, "8 per bucket", rep))
            assert got.size == 65536, (m, rep)
        rig.capacity_contract(text, pat, (m, "65,536"))
        # geometry of what runs on this background (resident)
        g = rig.ctx.geometry(m)
        tile = g["tile_bytes"]
        for total in (8191, 8192, 8193, 65535, 65536, 65537):
            text = _clusters(background, pat, total, tile)
            got = rig.check(text, pat, (m, "clustered", total))
            assert got.size == total
            if m >= 4:
                assert rig.ctx.last_search_sorted(), (m, total)
            if total in (8192, 8193, 65537):
                rig.capacity_contract(text, pat, (m, "clustered", total))
        # the bucket width steps at n_starts = 8192 << s
        for s in (0, 3, 10):
            for dn in (-1, 0, 1):
                n_starts = (8192 << s) + dn
                n = n_starts + m - 1
                step = max(m + 1, tile // 50)
                starts = np.unique(np.concatenate([np.arange(0, n_starts - m, step), [n_starts - 1]]))
                text = _plant(background[:n].copy(), pat, starts)
                got = rig.check(text, pat, (m, "n_starts", s, dn))
                assert got.size == starts.size and not rig.ctx.last_search_sorted()
        # base offsets around powers of two: the radix sort's key width
        text = _clusters(background, pat, 8193, tile)
        d = rig.put(text)
        n_starts = text.size - m + 1
        want = port.search(text, pat)
        for b in ((1 << 32) - n_starts // 2, (1 << 40) - n_starts - 1, (1 << 40) - n_starts, (1 << 40) - n_starts + 1,
                  (1 << 48) - n_starts // 2):
            pos, total = rig.ctx.search_device(d, pat, out=rig.out, base_offset=b)
            got = pos.cpu().numpy().astype(np.uint64)
            assert total == want.size and np.array_equal(got, want + np.uint64(b)), (m, b)
    finally:
        rig.close()


@pytest.mark.parametrize("slot", [0, 29, 87, AUTO])
def test_capacity_contract_on_dense_results(port, background, slot):
    """A tile with more matches than it can park: the dense path (count, tile scan, fill pass) under the capacity
    contract, for a short pattern and a walked one."""
    rig = Rig(port)
    rng = np.random.default_rng(6000 + slot)
    try:
        rig.ctx.set_variant(slot)
        for m in (1, 3, 8):
            pat = _pattern(rng, m)
            tile = _tile(rig, background, pat)
            n = 6 * tile + m
            # 1025 packed into tile 1 (above every parking cap), a few more spread over tiles 3 and 4
            starts = np.concatenate([np.arange(1025) * m + tile, np.arange(3 * tile, 5 * tile, 997)])
            text = _plant(background[:n].copy(), pat, starts)
            got = rig.check(text, pat, (slot, m, "dense"))
            assert not rig.ctx.last_search_sorted()
            rig.capacity_contract(text, pat, (slot, m, "dense"))
    finally:
        rig.close()


# ---------------------------------------------------------------- 4. the automatic choice in each of its states
def _alphabet_text(rng, sigma, n):
    """Uniform over `sigma` symbols: printable ones up to 95, all 256 byte values (NUL and >= 0x80 included) for 256."""
    if sigma == 256:
        return rng.integers(0, 256, n).astype(np.uint8)
    if sigma == 4:
        return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)]
    if sigma == 1:
        return np.full(n, ord("a"), dtype=np.uint8)
    return (rng.integers(0, sigma, n) + 0x20).astype(np.uint8)


AUTO_LENGTHS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 15, 16, 27, 28, 512]
AUTO_SIGMAS = [1, 2, 3, 4, 8, 9, 64, 65, 95, 256]


def _tables(pat, kind):
    """Canonical, safe non-canonical (every shift at most the canonical one) or all ones."""
    bad, good = host.build_tables(pat)
    if kind == "canonical":
        return None
    if kind == "ones":
        return np.ones(128, np.int32), np.ones(len(pat), np.int32)
    return np.maximum(bad - 1, 1).astype(np.int32), np.maximum(good // 2, 1).astype(np.int32)


def test_automatic_choice_in_each_of_its_states(port):
    """One context, one persistent buffer A and one B.  For every (content X, pattern, table kind) and a stale content Z:
    (a) the first search of X in A, (b) the next one (resident); Z written into B and searched twice, then X copy_'d into
    B -- same pointer, same length -- and searched: (c) the first search after the new content, still chosen by Z's
    sample, (d) the one after that.  Each case has a length of its own, so that (A, n) and (B, n) are new to the context's
    sample cache.  The lists are the oracle's in all four states, and (d) runs what a fresh text's second search runs
    -- (b) -- the sample corrected one search late.  Over the whole matrix the automatic choice reaches exactly the
    slots AUTO_REACHABLE lists (pick_variant's returns)."""
    import torch

    rng = np.random.default_rng(0xA070)
    N = (256 << 10) + 4096
    texts = {s: _alphabet_text(rng, s, N) for s in AUTO_SIGMAS}
    # (stale, new, explicit): printable -> ACGT, printable -> 'aaaa...', ACGT -> printable, where the short patterns'
    # `sparse` hint is wrong; then every alphabet with a far one in front of it
    pairs = [(95, 4, True), (95, 1, True), (4, 95, True)]
    pairs += [(AUTO_SIGMAS[(i + 5) % len(AUTO_SIGMAS)], s, False) for i, s in enumerate(AUTO_SIGMAS)]
    ctx = host.Context(0)
    out = torch.empty(N + 16, dtype=torch.int64, device="cuda")
    A = torch.empty(N, dtype=torch.uint8, device="cuda")
    B = torch.empty(N, dtype=torch.uint8, device="cuda")
    seen = set()
    case = 0

    def search(buf, n, want, pat, tables, what):
        pos, total = ctx.search_device(buf[:n], pat, out=out, tables=tables)
        got = pos.cpu().numpy().astype(np.uint64)
        assert total == want.size and np.array_equal(got, want), (what, total, want.size)
        seen.add(ctx.last_variant())
        return ctx.last_variant()

    try:
        for z_sigma, x_sigma, explicit in pairs:
            for m in AUTO_LENGTHS:
                if explicit and m > 4 and m not in (9, 16, 28):
                    continue  # (these pairs are about the short patterns; a few long ones for company)
                for kind in ("canonical", "safe", "ones"):
                    case += 1
                    n = N - case
                    x = texts[x_sigma][:n].copy()
                    z = texts[z_sigma][:n]
                    pat = bytes(x[1000:1000 + m] & 0x7F)
                    _plant(x, pat, [7 * m + 5, n // 2, n - m])
                    tables = _tables(pat, kind)
                    what = (z_sigma, x_sigma, m, kind)
                    want_x, want_z = port.search(x, pat), port.search(z, pat)
                    A[:n].copy_(torch.from_numpy(x))
                    search(A, n, want_x, pat, tables, what + ("a",))
                    vb = search(A, n, want_x, pat, tables, what + ("b",))
                    B[:n].copy_(torch.from_numpy(z))
                    search(B, n, want_z, pat, tables, what + ("z1",))
                    search(B, n, want_z, pat, tables, what + ("z2",))
                    B[:n].copy_(torch.from_numpy(x))
                    search(B, n, want_x, pat, tables, what + ("c",))
                    vd = search(B, n, want_x, pat, tables, what + ("d",))
                    assert vd == vb, (what, vd, vb)
        assert seen == AUTO_REACHABLE, sorted(seen)
    finally:
        ctx.close()


def test_seventeen_resident_texts_through_one_context(port):
    """More resident texts than the context's sample cache holds (16): cycled through three times, every list exact."""
    import torch

    rng = np.random.default_rng(17)
    ctx = host.Context(0)
    out = torch.empty(1 << 21, dtype=torch.int64, device="cuda")
    try:
        texts, bufs = [], []
        for i in range(17):
            t = _alphabet_text(rng, AUTO_SIGMAS[i % len(AUTO_SIGMAS)], (1 << 20) + 64 * i)
            texts.append(t)
            bufs.append(torch.from_numpy(t).cuda())
        for rep in range(3):
            for i, (t, d) in enumerate(zip(texts, bufs)):
                for m in (3, 9, 16):
                    pat = bytes(t[5000 + rep:5000 + rep + m] & 0x7F)
                    pos, total = ctx.search_device(d, pat, out=out)
                    want = port.search(t, pat)
                    assert total == want.size and np.array_equal(pos.cpu().numpy().astype(np.uint64), want), (rep, i, m)
    finally:
        ctx.close()


# ---------------------------------------------------------------- 5. the multi-pattern pass
def _multi(ctx, d, pats, out, cap):
    """bmx_search_device_multi itself: (rc, counts, first)."""
    import torch

    K = len(pats)
    counts, first = (C.c_uint64 * K)(), (C.c_uint64 * K)()
    rc = ctx._L.bmx_search_device_multi(ctx._h, C.c_void_p(d.data_ptr()), d.numel(), d.numel(), 0, (C.c_char_p * K)(*pats),
                                        (C.c_int32 * K)(*[len(p) for p in pats]), K, C.c_void_p(out.data_ptr()), cap, counts,
                                        first, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, [int(c) for c in counts], [int(f) for f in first]


def _scans(ctx):
    """Scan kernels this context has launched, as far as its ring of 64 timing-event pairs counts them."""
    return len(ctx.scan_ms_history(64))


def _multi_check(rig, text, pats, what, cap=None):
    """One bmx_search_device_multi call against the oracle.  Returns (total, scan kernels the call launched): 1 when the
    one-pass kernel's result stood, 1 + K when the call went the exact way pattern by pattern (bmx_scan.hip: one_by_one)."""
    d = rig.put(text)
    wants = [rig.port.search(text, p) for p in pats]
    total = sum(w.size for w in wants)
    cap = total if cap is None else cap
    if _scans(rig.ctx) > 64 - (len(pats) + 1):  # a fresh context, so that the ring counts every launch of this call
        rig.ctx.close()
        rig.ctx = host.Context(0)
    before = _scans(rig.ctx)
    rc, counts, first = _multi(rig.ctx, d, pats, rig.out, cap)
    launched = _scans(rig.ctx) - before
    assert counts == [w.size for w in wants], (what, counts)
    assert rc == (host.ERR_CAPACITY if total > cap else host.OK), (what, rc, total, cap)
    if rc == host.OK:
        for k, w in enumerate(wants):
            got = rig.out[first[k]:first[k] + counts[k]].cpu().numpy().astype(np.uint64)
            assert np.array_equal(got, w), (what, k)
    return total, launched


# The multi-pattern pass parks up to 512 matches per tile (bmx_scan.hip, the stage_cap loop of bmx_search_device_multi:
# the largest of 512/256/128/64 with lds_fixed + 2 x cap x 8 + 32 <= 160 KiB).  On these backgrounds (sigma 128: no 8-gram
# rule, 68 KiB tiles) lds_fixed = 2 x (69632 + halo16) + tables + 512 + 2 x ceil8(m_max) + ceil16(m_max) + 512, and the
# tables are 512 + ceil16(2m) + ceil16(m) bytes per pattern:
#   the boundary set (m_max 512, tables 5648 B): 148,496 + 8,224 = 156,720 <= 163,840, the 8 x 8-byte set: 144,704 + 8,224.
MULTI_STAGE_CAP = 512


def test_multi_pattern_pass_around_every_1k_boundary(port, background):
    """A mixed set (1, 3, 4, 9, 64, 512 bytes; two equal patterns; prefixes of the longest): one pattern at a time planted
    at b + delta for every multiple b of 1 KiB in 300 KiB and every delta in [-m-1, m+1] -- the pass's tile boundaries
    (68 / 52 KiB) are among them.  Each list equals the oracle's, and every case is the one-pass kernel's result: a
    512-byte plant matches 4 patterns of the set, 68 plants per 68 KiB tile make 272 matches (below MULTI_STAGE_CAP),
    and at 1 KiB apart no pattern has more than one match per position bucket (512 bytes wide here)."""
    rng = np.random.default_rng(0x3A17)
    P = _pattern(rng, 512)
    pats = [P, P[:64], P[:9], _pattern(rng, 4, lead=0x23), _pattern(rng, 3, lead=0x24), b"%", P[:64]]
    rig = Rig(port)
    try:
        n = 300 * 1024 + 600
        bs = np.arange(1, 300) * 1024
        for k in range(6):
            m = len(pats[k])
            for delta in range(-m - 1, m + 2):
                text = _plant(background[:n].copy(), pats[k], bs + delta)
                total, launched = _multi_check(rig, text, pats, (k, delta))
                assert launched == 1, (k, delta, launched)
    finally:
        rig.close()


def test_multi_pattern_shared_stage_per_tile(port, background):
    """Per-tile totals, summed over 8 patterns, at 63/64/65 ... 511/512/513 while each pattern alone stays below the
    cap: the shared double-buffered stage and the switch to the exact way, which is taken exactly when a tile holds more
    than MULTI_STAGE_CAP matches.  The matches are spread over the first 48 KiB of a tile (at most 3 per pattern in a
    2 KiB position bucket), in tile 0 and in the tile at 884 KiB (a boundary of both the 68 and the 52 KiB tiling).
    Then capacity = the sum and the sum - 1."""
    rng = np.random.default_rng(0x5157)
    pats = [_pattern(rng, 8, lead=0x21 + k) for k in range(8)]
    rig = Rig(port)
    try:
        n = 2 << 20
        for s in (63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513):
            text = background[:n].copy()
            stride = (48 << 10) // s
            for at in (0, 884 << 10):
                for j in range(s):
                    _plant(text, pats[j % 8], [at + j * stride])
            total, launched = _multi_check(rig, text, pats, s)
            assert total == 2 * s
            assert launched == (1 if s <= MULTI_STAGE_CAP else 1 + len(pats)), (s, launched)
            _multi_check(rig, text, pats, (s, "cap - 1"), cap=total - 1)
    finally:
        rig.close()


# ---------------------------------------------------------------- 6. the product library's stolen tail
def test_stolen_tail_of_the_product_kernels(port):
    """libbmx.so as shipped, 1 GiB texts (some 54 tiles per workgroup: the last ones go out by ticket): printable m = 16
    (slot 87), ACGT m = 12 (slot 88) and m = 64 (slot 53), each with a clustered stretch, searched twice so that the
    second search runs the resident-text choice, and a shard view -- whole lists against the oracle."""
    import torch

    n = (1 << 30) + 77
    ctx = host.Context(0)
    out = torch.empty(1 << 20, dtype=torch.int64, device="cuda")
    try:
        for kind, seed, cases in ((0, 0x5EED0087, [(16, 87)]), (1, 0x5EED0088, [(12, 88), (64, 53)])):
            d = torch.empty(n, dtype=torch.uint8, device="cuda")
            ctx.gen_text(d, 0, seed, kind)
            h = corpus.stream_bytes(0, n, seed, kind)
            rng = np.random.default_rng(seed)
            pats = []
            for i, (m, slot) in enumerate(cases):
                pat = h[12345 + 1000 * i:12345 + 1000 * i + m].tobytes()
                region = n // 4 * (i + 1)
                grid = rng.choice(np.arange(0, n // 8 // (2 * m)), 3000, replace=False) * (2 * m) + (n // 8) * (5 + i)
                stretch = region + np.arange(3000) * m
                for offs in (grid, stretch):
                    ctx.plant(d, 0, pat, offs)
                    _plant(h, pat, offs)
                pats.append((pat, slot))
            torch.cuda.synchronize()
            for pat, slot in pats:
                want = port.search(h, pat)
                for rep in range(2):
                    pos, total = ctx.search_device(d, pat, out=out)
                    assert total == want.size and np.array_equal(pos.cpu().numpy().astype(np.uint64), want), (kind, len(pat), rep)
                assert ctx.last_variant() == slot, (kind, len(pat), ctx.last_variant())
                lo, own = 100_000_003, 600_000_000
                shard = want[(want >= lo) & (want < lo + own)]
                for rep in range(2):
                    pos, total = ctx.search_device(d[lo:lo + own + len(pat) - 1], pat, n_own=own, base_offset=lo, out=out)
                    assert total == shard.size and np.array_equal(pos.cpu().numpy().astype(np.uint64), shard), (kind, len(pat), "shard")
            del d
    finally:
        ctx.close()
