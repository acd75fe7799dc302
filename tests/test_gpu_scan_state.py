"""GPU suite: what the exact search hands from one call to the next on one context.

The scan keeps state between calls -- counters that the ordering kernel re-arms, the geometry of the last launch for the
fill pass, the ring of timing events, the flag that says whether the last finish sorted, the ordering kernel's own stream
-- and every finish path leaves it for whatever call comes next.  The tests here run the paths one after another on ONE
context and check each call against the port oracle (`port.search`): a call refused before its launch, every finish path
in turn, and two enqueues without a finish between them.

Texts are a background of bytes >= 0x80 (or ACGT) of 350,001 bytes -- an odd length, five to ten tiles of 36, 68 or 76
KiB -- with printable patterns planted in them, as in test_gpu_scan_thresholds.py.  One step cannot be had at that size:
the radix sort takes a list of more than 8192 matches that overflowed a position bucket while no tile held more than it
can park (a fuller tile sends the call to the fill pass), and six 68 KiB tiles park 6 x 1024 at most.  That step alone
uses the smallest clustered text of test_gpu_scan_thresholds.py that reaches it (8193 matches, 56 per tile).
"""
import ctypes as C

import numpy as np
import pytest

from parallel_implementation_of_string_matching_algorithms_opencl_amd import host
from test_gpu_parity import PRODUCT_VARIANTS
from test_gpu_scan_thresholds import _clusters, _multi, _pattern, _plant, _scans

pytestmark = pytest.mark.gpu

N = 350_001
BG_BYTES = 12 << 20  # the radix step's text: 147 tiles of 76 KiB at the most
SMALL_SORT_MAX = 8192  # bmx_order_kernels.h: longer lists go to the radix sort


@pytest.fixture(scope="module")
def background(built):
    """Bytes 0x80..0xff: never in a pattern."""
    return np.random.default_rng(0x57A7E).integers(0x80, 0x100, BG_BYTES).astype(np.uint8)


class Bench:
    """One context, one device text buffer (a text of a given length stays at one address) and one output buffer."""

    def __init__(self, port):
        import torch

        self.torch = torch
        self.port = port
        self.ctx = host.Context(0)
        self.d = torch.empty(BG_BYTES, dtype=torch.uint8, device="cuda")
        self.out = torch.empty(1 << 18, dtype=torch.int64, device="cuda")

    def close(self):
        self.ctx.close()

    def put(self, text):
        d = self.d[: text.size]
        d.copy_(self.torch.from_numpy(text))
        return d

    def raw(self, d, pat, cap):
        """bmx_search_device itself: (rc, total) for a capacity of `cap` entries of self.out."""
        total = C.c_uint64(0)
        stream = C.c_void_p(self.torch.cuda.current_stream().cuda_stream)
        rc = self.ctx._L.bmx_search_device(self.ctx._h, C.c_void_p(d.data_ptr()), d.numel(), d.numel(), 0, pat, len(pat),
                                           None, None, C.c_void_p(self.out.data_ptr()) if cap else None, cap, C.byref(total),
                                           stream)
        return rc, int(total.value)

    def single(self, text, pat, what, launches=1):
        """One search against the oracle: list, total, a product slot, `launches` more timed kernels.  Returns whether
        the finish sorted."""
        d = self.put(text)
        before = _scans(self.ctx)
        self.out.fill_(-1)
        pos, total = self.ctx.search_device(d, pat, out=self.out)
        got = pos.cpu().numpy().astype(np.uint64)
        want = self.port.search(text, pat)
        assert total == want.size and got.size == want.size and np.array_equal(got, want), (what, total, want.size)
        assert self.ctx.last_variant() in PRODUCT_VARIANTS, (what, self.ctx.last_variant())
        assert _scans(self.ctx) - before == launches, (what, _scans(self.ctx) - before)
        return self.ctx.last_search_sorted()

    def multi(self, text, pats, what):
        """One bmx_search_device_multi call against the oracle; returns the timed kernels it launched."""
        d = self.put(text)
        wants = [self.port.search(text, p) for p in pats]
        before = _scans(self.ctx)
        self.out.fill_(-1)
        rc, counts, first = _multi(self.ctx, d, pats, self.out, self.out.numel())
        assert rc == host.OK and counts == [w.size for w in wants], (what, rc, counts)
        for k, w in enumerate(wants):
            got = self.out[first[k]:first[k] + counts[k]].cpu().numpy().astype(np.uint64)
            assert np.array_equal(got, w), (what, k)
        assert self.ctx.last_variant() in PRODUCT_VARIANTS, (what, self.ctx.last_variant())
        return _scans(self.ctx) - before


def _sparse(background, rng, pats, per_pattern=40):
    """N bytes of background with each pattern planted `per_pattern` times, one plant per 2 KiB at the most (no position
    bucket -- 64 bytes wide for one pattern, 256 for up to four -- holds two), the first window and the last among them."""
    text = background[:N].copy()
    slots = rng.permutation(np.arange(1, N // 2048 - 1))[: per_pattern * len(pats)].reshape(len(pats), per_pattern)
    for k, pat in enumerate(pats):
        _plant(text, pat, slots[k] * 2048 + 100 * k + int(rng.integers(0, 64)))
    _plant(text, pats[0], [0, N - len(pats[0])])
    return text


def test_refused_call_leaves_the_context_armed(port, background):
    """The first calls on a fresh context are refused for a pattern byte >= 0x80 (BMX_ERR_DOMAIN): a single search, which
    has cleared the device counters by then and launches nothing, and a multi-pattern call.  The ordinary single and
    multi-pattern searches behind them find counters that are zero and give the oracle's lists and counts."""
    rng = np.random.default_rng(0xA53D)
    pats = [_pattern(rng, 16), _pattern(rng, 8, lead=0x22), _pattern(rng, 5, lead=0x23)]
    text = _sparse(background, rng, pats)
    b = Bench(port)
    try:
        d = b.put(text)
        rc, total = b.raw(d, b"ab\x80cd", b.out.numel())
        assert rc == host.ERR_DOMAIN and total == 0
        rc, counts, first = _multi(b.ctx, d, [pats[0], b"xy\xffz"], b.out, b.out.numel())
        assert rc == host.ERR_DOMAIN and counts == [0, 0], (rc, counts)
        assert _scans(b.ctx) == 0  # nothing was launched
        assert not b.single(text, pats[0], "single after the refused calls")
        assert b.multi(text, pats, "multi after the refused calls") == 1
        rc, total = b.raw(d, b"\x80", b.out.numel())  # ... and between two searches
        assert rc == host.ERR_DOMAIN
        assert not b.single(text, pats[1], "single after a refused call")
    finally:
        b.close()


def test_every_finish_path_in_turn_on_one_context(port, background):
    """A sparse list ordered from the position buckets; m = 1 on ACGT text (a dense result: per-tile counts, tile scan,
    fill pass); clusters that overflow their position buckets while every tile parks its matches -- sorted in LDS, and
    with more than 8192 matches by the radix sort; three patterns in one pass; a count-only call (capacity 0:
    BMX_ERR_CAPACITY and the true total); the first search again.  After each step: the oracle's list, whether the finish
    sorted, a product slot as the last variant, and one more timed scan kernel (the multi-pattern pass: one, its sparse
    result stands -- 1 + K had it gone the exact way, as test_gpu_scan_thresholds.py counts it)."""
    rng = np.random.default_rng(0xF1F0)
    pats = [_pattern(rng, 16), _pattern(rng, 8, lead=0x22), _pattern(rng, 5, lead=0x23)]
    sparse = _sparse(background, rng, pats)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, N)]
    cluster_pat = _pattern(rng, 5, lead=0x24)  # 5 bytes end to end: 12 matches in a 64-byte bucket of 8 entries
    b = Bench(port)
    try:
        assert not b.single(sparse, pats[0], "sparse")
        assert not b.single(acgt, b"A", "dense, m = 1")
        # the tile of the kernel that searches cluster_pat on this background: 56 matches at the front of every whole tile
        for _ in range(2):  # (the second search on a text runs what every later one does)
            b.single(background[:N], cluster_pat, "probe")
        tile = b.ctx.geometry(len(cluster_pat))["tile_bytes"]
        j = np.arange(56 * (N // tile))
        small = _plant(background[:N].copy(), cluster_pat, (j // 56) * tile + 1000 + (j % 56) * len(cluster_pat))
        assert 1 < j.size <= SMALL_SORT_MAX
        assert b.single(small, cluster_pat, "clustered, in-LDS sort")
        large = _clusters(background, cluster_pat, SMALL_SORT_MAX + 1, tile)
        assert b.single(large, cluster_pat, "clustered, radix sort")
        assert b.multi(sparse, pats, "three patterns") == 1
        assert not b.ctx.last_search_sorted()
        d = b.put(sparse)
        before = _scans(b.ctx)
        rc, total = b.raw(d, pats[1], 0)
        assert rc == host.ERR_CAPACITY and total == port.search(sparse, pats[1]).size, (rc, total)
        assert _scans(b.ctx) - before == 1 and not b.ctx.last_search_sorted()
        assert b.ctx.last_variant() in PRODUCT_VARIANTS
        assert not b.single(sparse, pats[0], "sparse again")
    finally:
        b.close()


@pytest.mark.parametrize("overlap", [False, True])
def test_two_enqueues_without_a_finish_between(port, background, overlap):
    """Two searches enqueued on one context before any finish, with the ordering kernel on the caller's stream and on the
    context's own (bmx_set_order_overlap): the second scan runs behind the first one's ordering kernel, which re-arms
    the counters; bmx_count_to_device delivers the second search's count, the finish its list and count."""
    import torch

    rng = np.random.default_rng(0x2E9 + overlap)
    pats = [_pattern(rng, 16), _pattern(rng, 9, lead=0x22)]
    text = _sparse(background, rng, pats, per_pattern=30 + 7 * overlap)
    _plant(text, pats[1], [1000])  # (a spot no other plant has) the two totals differ
    wants = [port.search(text, p) for p in pats]
    assert wants[0].size != wants[1].size
    b = Bench(port)
    try:
        b.ctx.set_order_overlap(overlap)
        d = b.put(text)
        out1 = torch.full((1024,), -1, dtype=torch.int64, device="cuda")
        out2 = torch.full((1024,), -1, dtype=torch.int64, device="cuda")
        d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
        for rep in range(2):  # the first pair on this text and the resident one
            b.ctx.enqueue(d, pats[0], out1)
            b.ctx.enqueue(d, pats[1], out2)
            b.ctx.count_to_device(d_count)
            total = b.ctx.finish(out2)
            assert total == wants[1].size, (rep, total)
            assert np.array_equal(out2[:total].cpu().numpy().astype(np.uint64), wants[1]), rep
            torch.cuda.synchronize()
            assert int(d_count.item()) == wants[1].size, (rep, int(d_count.item()))
            # (the first search's list was written by its own ordering kernel, whose status the second one's replaced)
            assert np.array_equal(out1[:wants[0].size].cpu().numpy().astype(np.uint64), wants[0]), rep
            assert not b.ctx.last_search_sorted()
    finally:
        b.close()
