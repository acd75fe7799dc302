"""GPU suite for the approximate search and the match spans with patterns of up to 512 bytes
(bmx_search_approx_long_device, bmx_approx_long_spans_device and what sits on them): ends, distances and starts compared
with the Sellers oracle (tests/approx_oracle.py) and the spans oracle (tests/spans_oracle.py), for k = 0 with the exact
search.

Texts are sized from the documented piece rule (csrc/bmx_approx_long.hip): a lane owns 2^ps ends,
ps = max(clamp(ceil_log2(ceil(n / resident lanes)), 6, 12), min(ceil_log2(4 (m + k)), 12)), a tile is 256 lanes.  Every
text here has fewer than 64 bytes per resident lane (at least 256 CUs x 256 lanes), so ps follows from m + k alone.

The starts oracle fills an (ends x (m + 1)) table m + k times, 60 to 170 M cells a second.  Every start is compared
with it.  So that this stays affordable, the spans test of a random case whose list would cost more than SPANS_CELLS cells
runs on a PREFIX of the case's text: the text cut right before the first end that no longer fits the budget (the ends of
a prefix are a prefix of the ends, so nothing else of the case changes).  That shortens 22 of the 200 texts, all with
k = min(m - 1, 255), to 511 .. 3,087 bytes; nine of them keep ends with the whole walk of m + k bytes behind them at
m >= 320 (cases 11, 119 and 191: every end), and test_spans_whole_walk_at_the_largest_m_and_k has 511 such ends at
m = 512, k = 255.  The search is compared on the whole text of every case."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from approx_oracle import approx_ends
from conftest import ROOT, golden_file_bytes
from spans_oracle import select_best, span_starts
from test_gpu_approx import _dev
from parallel_implementation_of_string_matching_algorithms_opencl_amd import corpus, host

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "parallel_implementation_of_string_matching_algorithms_opencl_amd", "bin", "bmx_cli")
LONG_M = (65, 66, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 383, 384, 385, 448, 511, 512)
N_CASES, CHUNK = 200, 8
SPANS_CELLS = 100_000_000  # one to two seconds of the oracle


def piece_shift(n: int, m: int, k: int, resident: int = 256 * 256) -> int:
    """The documented rule; `resident` only matters from 64 bytes per lane on."""
    clog2 = lambda x: max(int(x) - 1, 0).bit_length()
    per = -(-n // resident)
    assert per <= 64, "the text is large enough for the occupancy to enter the rule"
    return max(min(max(clog2(per), 6), 12), min(clog2(4 * (m + k)), 12))


def _long(ctx, d_text, pat: bytes, k: int, *, n=None, lead=0, base_offset=0, capacity=None, with_dist=True, stream=None):
    """bmx_search_approx_long_device itself (host.py sends m <= 64 to the old entry): (ends, dist or None, total, rc)."""
    import torch

    n = d_text.numel() if n is None else n
    cap = max(n, 1) if capacity is None else capacity
    out = torch.full((max(cap, 1),), -1, dtype=torch.int64, device=d_text.device)
    dist = torch.full((max(cap, 1),), 255, dtype=torch.uint8, device=d_text.device) if with_dist else None
    total = C.c_uint64(0)
    s = C.c_void_p((stream if stream is not None else torch.cuda.current_stream(d_text.device)).cuda_stream)
    rc = ctx._L.bmx_search_approx_long_device(ctx._h, C.c_void_p(d_text.data_ptr()), n, lead, base_offset, pat, len(pat), int(k),
                                              C.c_void_p(out.data_ptr()), C.c_void_p(dist.data_ptr()) if with_dist else None,
                                              cap, C.byref(total), s)
    got = min(int(total.value), cap)
    return (out[:got].cpu().numpy().astype(np.int64), dist[:got].cpu().numpy().astype(np.int64) if with_dist else None,
            int(total.value), rc)


def _check(ctx, text: bytes, pat: bytes, k: int, offset: int = 0, want=None):
    want_e, want_d = approx_ends(text, pat, k) if want is None else want
    e, d, total, rc = _long(ctx, _dev(ctx, text, offset), pat, k)
    assert rc == host.OK, (rc, len(text), len(pat), k)
    assert total == want_e.size, (len(text), len(pat), k, offset, total, want_e.size)
    assert np.array_equal(e, want_e), (len(text), len(pat), k, offset)
    assert np.array_equal(d, want_d), (len(text), len(pat), k, offset)
    return e, d


def _edit_in(rng, pat: bytes, edits: int, base: int, sigma: int) -> bytes:
    """`edits` substitutions, insertions and deletions at random rows, letters from the alphabet."""
    s = bytearray(pat)
    for _ in range(edits):
        op = int(rng.integers(0, 3))
        i = int(rng.integers(0, len(s)))
        c = base + int(rng.integers(0, sigma))
        if op == 0:
            s[i] = c
        elif op == 1:
            s.insert(i, c)
        elif len(s) > 1:
            del s[i]
    return bytes(s)


@functools.lru_cache(maxsize=None)
def _case(i: int):
    """Random case i: (text, pat, k, offset, oracle ends, oracle distances).  Computed once, shared by the search and the
    spans tests."""
    rng = np.random.default_rng(0xA7710 + i)
    sigma = (2, 4, 95)[i % 3]
    base = 0x20 if sigma == 95 else 0x61
    m = int(rng.integers(1, 65)) if rng.random() < 0.2 else int(rng.choice(LONG_M))
    k = min((0, 1, m // 8, min(m - 1, 255))[(i // 3) % 4], m - 1)
    n = int(rng.integers(0, m + 40)) if i % 10 == 0 else int(rng.integers(0, 5001))  # every tenth: below or around m
    text = (rng.integers(0, sigma, n) + base).astype(np.uint8)
    pat = (rng.integers(0, sigma, m) + base).astype(np.uint8).tobytes()
    if i % 2 and n > m + k:  # a copy with up to k substitutions, insertions and deletions
        copy = np.frombuffer(_edit_in(rng, pat, int(rng.integers(0, k + 1)), base, sigma), np.uint8)
        if copy.size <= n:
            at = int(rng.integers(0, n - copy.size + 1))
            text[at:at + copy.size] = copy
    text = text.tobytes()
    e, d = approx_ends(text, pat, k)
    return text, pat, k, i % 16, e, d


@pytest.mark.parametrize("chunk", range(N_CASES // CHUNK))
def test_random_cases_against_oracle(ctx, chunk):
    for i in range(chunk * CHUNK, (chunk + 1) * CHUNK):
        text, pat, k, off, want_e, want_d = _case(i)
        e, d = _check(ctx, text, pat, k, off, want=(want_e, want_d))
        if len(pat) <= host.MAX_APPROX_PATTERN:  # handed to the one-word kernels: the old entry's list
            d_text = _dev(ctx, text, off)
            e0, d0, t0 = ctx.search_approx_device(d_text, pat, k, capacity=max(len(text), 1))
            assert t0 == e.size and np.array_equal(e0.cpu().numpy(), e) and np.array_equal(d0.cpu().numpy(), d), i


def _spans(ctx, d_text, pat, k, e, d, best):
    """bmx_approx_long_spans_device itself over the list (e, d): (starts, ends, dist) on the host."""
    import torch

    dev = d_text.device
    ends = torch.from_numpy(np.asarray(e, np.int64)).to(dev)
    dist = torch.from_numpy(np.asarray(d, np.uint8)).to(dev)
    count = ends.numel()
    starts = torch.full((max(count, 1),), -1, dtype=torch.int64, device=dev)
    sel_e = torch.full((max(count, 1),), -1, dtype=torch.int64, device=dev)
    sel_d = torch.full((max(count, 1),), 255, dtype=torch.uint8, device=dev)
    total = C.c_uint64(0)
    rc = ctx._L.bmx_approx_long_spans_device(ctx._h, C.c_void_p(d_text.data_ptr()), d_text.numel(), 0, pat, len(pat), int(k),
                                             C.c_void_p(ends.data_ptr()), C.c_void_p(dist.data_ptr()), count,
                                             host.SPANS_BEST if best else 0, C.c_void_p(starts.data_ptr()),
                                             C.c_void_p(sel_e.data_ptr()), C.c_void_p(sel_d.data_ptr()), C.byref(total),
                                             C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == host.OK, (rc, len(pat), k, count)
    t = int(total.value)
    if best:
        return starts[:t].cpu().numpy(), sel_e[:t].cpu().numpy(), sel_d[:t].cpu().numpy().astype(np.int64)
    assert t == count
    return starts[:t].cpu().numpy(), np.asarray(e, np.int64), np.asarray(d, np.int64)


def _spans_prefix(text: bytes, pat: bytes, k: int, e, d):
    """(text, ends, distances) of the longest prefix of the text whose list costs the starts oracle at most SPANS_CELLS."""
    room = SPANS_CELLS // ((len(pat) + 1) * (len(pat) + k))
    if e.size <= room:
        return text, e, d
    cut = int(e[room])  # the first end that no longer fits: the prefix ends right before it
    return text[:cut], e[:room], d[:room]


@pytest.mark.parametrize("chunk", range(N_CASES // CHUNK))
def test_spans_on_the_random_lists(ctx, chunk):
    for i in range(chunk * CHUNK, (chunk + 1) * CHUNK):
        text, pat, k, off, e, d = _case(i)
        text, e, d = _spans_prefix(text, pat, k, e, d)
        if e.size == 0:
            continue
        d_text = _dev(ctx, text, off)
        e_dev, d_dev, total, rc = _long(ctx, d_text, pat, k)  # the list as the device returns it for this text
        assert rc == host.OK and np.array_equal(e_dev, e) and np.array_equal(d_dev, d), i
        want_s, want_d = span_starts(text, pat, k, e)  # every entry
        assert np.array_equal(want_d, d), i
        s_all, _, _ = _spans(ctx, d_text, pat, k, e, d, best=False)
        assert np.array_equal(s_all, want_s), i
        keep = select_best(e, d, k)
        s_best, e_best, d_best = _spans(ctx, d_text, pat, k, e, d, best=True)
        assert np.array_equal(e_best, e[keep]) and np.array_equal(d_best, d[keep]), i
        assert np.array_equal(s_best, want_s[keep]), i


def test_spans_whole_walk_at_the_largest_m_and_k(ctx):
    """m = 512, k = 255: one copy in 95-letter text gives the 511 ends around it, each with all 767 bytes of the backward
    walk (96 chunks of the starts kernel) inside the text."""
    rng = np.random.default_rng(512255)
    text = (rng.integers(0, 95, 2000) + 0x20).astype(np.uint8)
    pat = (rng.integers(0, 95, 512) + 0x20).astype(np.uint8)
    text[900:1412] = pat
    text, pat = text.tobytes(), pat.tobytes()
    e, d = _check(ctx, text, pat, 255, offset=13)
    assert e.size == 511 and int(e.min()) >= 512 + 255 - 1
    want_s, want_d = span_starts(text, pat, 255, e)
    assert np.array_equal(want_d, d)
    d_text = _dev(ctx, text, 13)
    s_all, _, _ = _spans(ctx, d_text, pat, 255, e, d, best=False)
    assert np.array_equal(s_all, want_s)
    keep = select_best(e, d, 255)
    s_best, e_best, d_best = _spans(ctx, d_text, pat, 255, e, d, best=True)
    assert np.array_equal(e_best, e[keep]) and np.array_equal(d_best, d[keep]) and np.array_equal(s_best, want_s[keep])


def test_spans_reject_an_altered_distance(ctx):
    import torch

    rng = np.random.default_rng(77)
    text = (rng.integers(0, 95, 4000) + 0x20).astype(np.uint8)
    for m in (100, 300):
        pat = (rng.integers(0, 95, m) + 0x20).astype(np.uint8)
        text[500:500 + m] = pat
        text[520] ^= 1
        text[2500:2500 + m] = pat
        d_text = _dev(ctx, text.tobytes(), 7)
        e, d, total = ctx.search_approx_device(d_text, pat.tobytes(), 3, capacity=4000)
        assert total >= 8
        s, e2, d2, t = ctx.approx_spans_device(d_text, pat.tobytes(), 3, e, d)  # (host.py routes m > 64 to the long entry)
        assert t == total
        bad = d.clone()
        bad[total // 2] = (int(bad[total // 2]) + 1) % 4
        with pytest.raises(host.BmxError) as err:
            ctx.approx_spans_device(d_text, pat.tobytes(), 3, e, bad)
        assert err.value.rc == host.ERR_ARG
        with pytest.raises(host.BmxError) as err:  # all zero: the selection keeps the last end of every run, at distance 3
            ctx.approx_spans_device(d_text, pat.tobytes(), 3, e, torch.zeros_like(d), best=True)
        assert err.value.rc == host.ERR_ARG
        bad_e = e.clone()
        bad_e[1] = 4000 + 16  # an end outside the view
        with pytest.raises(host.BmxError) as err:
            ctx.approx_spans_device(d_text, pat.tobytes(), 3, bad_e, None)
        assert err.value.rc == host.ERR_ARG
        far = torch.tensor([2000], dtype=torch.int64, device=d_text.device)  # an end with no match within k edits
        with pytest.raises(host.BmxError) as err:
            ctx.approx_spans_device(d_text, pat.tobytes(), 3, far, None)
        assert err.value.rc == host.ERR_ARG


@pytest.mark.parametrize("m", [65, 128, 129, 512])
def test_one_edit_at_the_word_boundaries(ctx, m):
    """One read per edit kind at pattern rows 0, 62, 63, 64, 65, 127, 128 and m - 1, k = 1: the rows at which a dropped or
    doubled carry between words shows."""
    rng = np.random.default_rng(1000 + m)
    pat = (rng.integers(0, 95, m) + 0x20).astype(np.uint8).tobytes()
    for row in sorted({r for r in (0, 62, 63, 64, 65, 127, 128, m - 1) if r < m}):
        for kind in ("substitution", "insertion", "deletion"):
            other = 0x20 + (pat[row] - 0x20 + 1 + int(rng.integers(0, 93))) % 95  # != pat[row]
            read = bytearray(pat)
            if kind == "substitution":
                read[row] = other
            elif kind == "insertion":
                read.insert(row, other)
            else:
                del read[row]
            text = (rng.integers(0, 95, 2200) + 0x20).astype(np.uint8)
            at = 700 + int(rng.integers(0, 300))
            text[at:at + len(read)] = np.frombuffer(bytes(read), np.uint8)
            text = text.tobytes()
            want_e, want_d = approx_ends(text, pat, 1)
            assert at + len(read) - 1 in want_e.tolist(), (m, row, kind)
            e, d = _check(ctx, text, pat, 1, offset=row % 16, want=(want_e, want_d))
            s, _, _ = _spans(ctx, _dev(ctx, text, row % 16), pat, 1, e, d, best=False)
            want_s, want_sd = span_starts(text, pat, 1, e)
            assert np.array_equal(s, want_s) and np.array_equal(want_sd, d), (m, row, kind)


def test_one_letter_closed_form_is_the_oracles():
    """'a' * n against 'a' * m, k = 3: every end from m - k - 1 on, at distance max(0, m - 1 - j)."""
    for m in (65, 130, 512):
        e, d = approx_ends(b"a" * 2000, b"a" * m, 3)
        assert np.array_equal(e, np.arange(m - 4, 2000))
        assert np.array_equal(d, np.maximum(0, m - 1 - e))


@pytest.mark.parametrize("m", [65, 130, 512])
def test_one_letter_text(ctx, m):
    """Every tile is dense (the second walk), and every column carries through whole words."""
    import torch

    n, k = 300_000, 3
    d_text = torch.full((n + 32,), ord("a"), dtype=torch.uint8, device=f"cuda:{ctx.device}")[5:5 + n]
    e, d, total, rc = _long(ctx, d_text, b"a" * m, k)
    assert rc == host.OK and total == n - (m - k - 1)
    want_e = np.arange(m - k - 1, n)
    assert np.array_equal(e, want_e)
    assert np.array_equal(d, np.maximum(0, m - 1 - want_e))


@pytest.mark.parametrize("m,k", [(100, 8), (500, 8)])  # the smallest and the largest instantiated word count
def test_copies_across_tile_and_lane_boundaries(ctx, m, k):
    rng = np.random.default_rng(m)
    ps = piece_shift(3 << 20, m, k)
    tile = 256 << ps
    offset = 11  # view byte 0 sits at aligned coordinate 11: boundaries are at multiples of the tile minus 11
    n = 3 * tile + 4321
    assert piece_shift(n, m, k) == ps and n + offset > 3 * tile
    text = (rng.integers(0, 95, n) + 0x20).astype(np.uint8)
    pat = (rng.integers(0, 95, m) + 0x20).astype(np.uint8).tobytes()
    cuts = [t * tile - offset for t in (1, 2, 3)]  # every tile boundary
    cuts += [tile - offset + (37 << ps), 2 * tile - offset + (200 << ps), (5 << ps) - offset]  # a few lane boundaries
    windows = []
    for j, cut in enumerate(cuts):
        copy = _edit_in(rng, pat, j % (k + 1) if j else k, 0x20, 95)
        at = cut - (len(copy) * (j + 1)) // (len(cuts) + 1)  # the boundary falls at a different row of every copy
        text[at:at + len(copy)] = np.frombuffer(copy, np.uint8)
        windows.append((at - m - k, at + m + k))
    exp_e, exp_d = [], []
    for lo, hi in sorted(windows):
        assert lo >= 0 and hi <= n and (not exp_e or lo > exp_e[-1][-1])
        we, wd = approx_ends(text[lo:hi].tobytes(), pat, k)
        assert we.size > 0
        exp_e.append(we + lo)
        exp_d.append(wd)
    exp_e, exp_d = np.concatenate(exp_e), np.concatenate(exp_d)
    e, d, total, rc = _long(ctx, _dev(ctx, text.tobytes(), offset), pat, k, capacity=exp_e.size + 1000)
    assert rc == host.OK
    assert total == exp_e.size  # (a hit outside the windows shows here)
    assert np.array_equal(e, exp_e) and np.array_equal(d, exp_d)


@pytest.mark.parametrize("m", [65, 256, 512])
def test_k0_equals_exact_search(ctx, m):
    spec = corpus.CorpusSpec(f"approx_long_k0_{m}", 16 * corpus.MiB + 5, m, 0, seed=0x5EEDB000 + m, plant_period=1 << 14,
                             boundary_period=1 << 20)
    d_text = spec.device_text(ctx)
    pat = spec.pattern()
    pos, total = ctx.search_device(d_text, pat, capacity=d_text.numel())
    want = pos.cpu().numpy().astype(np.int64)
    assert total == want.size and total > 500
    e, d, t, rc = _long(ctx, d_text, pat, 0, capacity=total + 8)
    assert rc == host.OK and t == total
    assert np.array_equal(e - (m - 1), want)
    assert int(d.max()) == 0


@functools.lru_cache(maxsize=None)
def _planted(m: int, k: int, n: int = 200_000):
    rng = np.random.default_rng(m * 7 + k)
    text = (rng.integers(0, 95, n) + 0x20).astype(np.uint8)
    pat = (rng.integers(0, 95, m) + 0x20).astype(np.uint8).tobytes()
    for at in range(300, n - 2 * m, 9973):
        copy = _edit_in(rng, pat, int(rng.integers(0, k + 1)), 0x20, 95)
        text[at:at + len(copy)] = np.frombuffer(copy, np.uint8)
    text = text.tobytes()
    return text, pat, approx_ends(text, pat, k)


def test_capacity_keeps_the_lowest_ends(ctx):
    m, k = 130, 4
    text, pat, (want_e, want_d) = _planted(m, k)
    total = want_e.size
    assert total > 40
    d_text = _dev(ctx, text, 3)
    for cap in (0, 1, total - 1, total):
        e, d, t, rc = _long(ctx, d_text, pat, k, capacity=cap)
        assert t == total and rc == (host.OK if cap == total else host.ERR_CAPACITY), (cap, rc, t)
        assert np.array_equal(e, want_e[:cap]) and np.array_equal(d, want_d[:cap]), cap
    e, d, t, rc = _long(ctx, d_text, pat, k, capacity=total, with_dist=False)  # d_dist = NULL
    assert rc == host.OK and t == total and d is None and np.array_equal(e, want_e)


def test_shards_concatenate_to_the_whole_list(ctx):
    m, k = 300, 6
    text, pat, (want_e, want_d) = _planted(m, k)
    assert want_e.size > 40
    d_text = _dev(ctx, text, 9)
    n = len(text)
    cuts = [0, 30_011, 150_000, n]
    es, ds = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        lead = min(a, m + k - 1)
        e, d, t, rc = _long(ctx, d_text[a - lead:b], pat, k, lead=lead, base_offset=a - lead)
        assert rc == host.OK and t == e.size
        es.append(e)
        ds.append(d)
    assert np.array_equal(np.concatenate(es), want_e) and np.array_equal(np.concatenate(ds), want_d)


def test_device_entries_on_a_non_blocking_stream(ctx):
    """Both device entries on a caller's non-blocking stream: the text is still being produced on that stream when the
    search is called, and work queued behind the calls (the text is wiped) does not reach them."""
    import torch

    from test_gpu_streams import Pending, delay, side_stream

    m, k = 200, 5
    text, pat, (want_e, want_d) = _planted(m, k)
    want_s, _ = span_starts(text, pat, k, want_e)
    real = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
    buf = torch.full_like(real, ord("z"))  # the decoy: no hit at all
    s = side_stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        delay(s)
        buf.copy_(real, non_blocking=True)
        pending = Pending(s)
        pending.assert_outstanding("bmx_search_approx_long_device")
        e, d, total = ctx.search_approx_device(buf, pat, k, capacity=want_e.size + 8)
        st, e2, d2, t2 = ctx.approx_spans_device(buf, pat, k, e, d)
        got = [x.clone() for x in (e, d, st)]
        buf.zero_()  # queued behind
    s.synchronize()
    assert total == want_e.size == t2
    assert np.array_equal(got[0].cpu().numpy(), want_e) and np.array_equal(got[1].cpu().numpy().astype(np.int64), want_d)
    assert np.array_equal(got[2].cpu().numpy(), want_s)
    assert ctx.last_approx_ms() > 0 and ctx.last_spans_ms() > 0


def test_host_entries_and_the_module_level_functions(ctx):
    m, k = 100, 2
    text, pat, (want_e, want_d) = _planted(m, k, n=60_000)
    assert want_e.size > 5
    want_s, _ = span_starts(text, pat, k, want_e)
    e, d = ctx.search_approx(text, pat, k)
    assert np.array_equal(e.astype(np.int64), want_e) and np.array_equal(d.astype(np.int64), want_d)
    with pytest.raises(host.BmxError) as err:
        ctx.search_approx(text, pat, k, capacity=want_e.size - 1)
    assert err.value.rc == host.ERR_CAPACITY
    e, d = host.search_approx(text, pat, k)  # a 100-byte pattern through the module-level entry
    assert np.array_equal(e.astype(np.int64), want_e) and np.array_equal(d.astype(np.int64), want_d)
    s, e, d = ctx.search_approx_spans(text, pat, k, best=False)
    assert np.array_equal(s.astype(np.int64), want_s) and np.array_equal(e.astype(np.int64), want_e)
    keep = select_best(want_e, want_d, k)
    s, e, d = host.search_approx_spans(text, pat, k)
    assert np.array_equal(s.astype(np.int64), want_s[keep]) and np.array_equal(e.astype(np.int64), want_e[keep])
    assert np.array_equal(d.astype(np.int64), want_d[keep])
    # the last-call timers follow the entry that ran last
    ctx.search_approx(text, pat, k)
    assert ctx.last_approx_ms() > 0
    ctx.search_approx(text, pat[:20], 1)
    assert ctx.last_approx_ms() > 0


def test_a_100_byte_pattern_through_the_cli(ctx, tmp_path):
    text = golden_file_bytes("input5L.txt.gz")
    pat = bytearray(text[250_000:250_100])
    pat[40] ^= 1  # one substitution against the text: the source is a hit at distance 1 (or less, if it repeats)
    pat = bytes(pat)
    want_e, want_d = approx_ends(text, pat, 2)
    want_s, _ = span_starts(text, pat, 2, want_e)
    keep = select_best(want_e, want_d, 2)
    assert want_e.size >= 1 and 250_099 in want_e.tolist()
    (tmp_path / "input5L.txt").write_bytes(text)
    (tmp_path / "pat.txt").write_bytes(pat)
    r = subprocess.run([CLI, "--approx", "2", "--spans", "--best", "--text", str(tmp_path / "input5L.txt"), "--pattern",
                        str(tmp_path / "pat.txt"), "--iters", "2", "--max-print", "3"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = r.stdout
    assert f"approximate matches (k = 2): {want_e.size}" in out
    assert f"first end: {int(want_e[0])} (distance {int(want_d[0])})" in out
    assert re.search(rf"match spans \(best\): {keep.size} ", out)
    first = keep[0]
    assert f"\n{int(want_s[first])} {int(want_e[first])} {int(want_d[first])}\n" in out
