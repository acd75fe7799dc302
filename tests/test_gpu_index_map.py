"""GPU suite for the text index's read mapping (bmx_index_map*, host.Index.map): every candidate's (start, end, dist),
every cand_off and every per-query best against tests/map_oracle.py, at the smallest shapes at which each part can go
wrong: small texts in full, the word boundaries of the multi-word walker, windows clipped at both ends of the text, ties
and many candidates, capacities, bad input, streams and the planted case of the CPU suite.  Outputs arrive filled with a
mark that must survive beyond `count` and `capacity`; blobs carry unused bytes in front and behind."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import index_oracle as io
import map_oracle as mp
from conftest import ROOT
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host
from test_gpu_index import on_device, side_stream_with_delay
from test_index_map_cpu import PLANTED, check_planted, planted_case
from test_index_match_cpu import queries_for

pytestmark = pytest.mark.gpu

MARK, MARK8 = -7, 0xA5
FRONT, BACK = 3, 5
EXTRA = 4  # marked entries behind count and behind capacity


def column(queries, front=FRONT, back=BACK):
    blob, off = host.pack_strings(queries)
    pad = lambda k: np.full(k, ord("a"), np.uint8)
    return np.concatenate([pad(front), blob, pad(back)]), off + np.uint64(front)


def raw_map(ctx, idx, blob, off, min_len, max_occ, k, base_offset=0, capacity=None, cand_off=True):
    """bmx_index_map_device into marked arrays: (rc, total, best triple, cand_off, candidate triple) as numpy; capacity
    None: a counting call first (capacity 0, NULL lists), then the full list."""
    import torch

    d_blob = torch.from_numpy(blob).cuda()
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    count = off.size - 1
    total = C.c_uint64(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def call(cap, lists):
        best = [torch.full((count + EXTRA,), MARK, dtype=torch.int64, device="cuda") for _ in range(2)]
        best.append(torch.full((count + EXTRA,), MARK8, dtype=torch.uint8, device="cuda"))
        coff = torch.full((count + 1 + EXTRA,), MARK, dtype=torch.int64, device="cuda") if cand_off else None
        cand = [None] * 3
        if lists:
            cand = [torch.full((cap + EXTRA,), MARK, dtype=torch.int64, device="cuda") for _ in range(2)]
            cand.append(torch.full((cap + EXTRA,), MARK8, dtype=torch.uint8, device="cuda"))
        rc = ctx._L.bmx_index_map_device(ctx._h, idx._h, ptr(d_blob), d_blob.numel(), ptr(d_off), count, min_len, max_occ, k,
                                         base_offset, *[ptr(b) for b in best], ptr(coff), *[ptr(c) for c in cand], cap,
                                         C.byref(total), stream)
        return rc, best, coff, cand

    if capacity is None:
        rc, best0, _, _ = call(0, False)
        assert rc == host.OK, host.lib().bmx_last_error()
        capacity = int(total.value)
        rc, best, coff, cand = call(capacity, True)
        for a, b in zip(best0, best):
            assert torch.equal(a, b), "the per-query answer depends on the capacity"
    else:
        rc, best, coff, cand = call(capacity, capacity > 0)
    if rc not in (host.OK, host.ERR_CAPACITY):
        return rc, int(total.value), None, None, None
    assert ctx.last_index_map_candidates() == total.value
    best = [b.cpu().numpy() for b in best]
    assert np.all(best[0][count:] == MARK) and np.all(best[1][count:] == MARK) and np.all(best[2][count:] == MARK8)
    if coff is not None:
        coff = coff.cpu().numpy()
        assert np.all(coff[count + 1:] == MARK)
        coff = coff[:count + 1]
    stored = min(capacity, int(total.value))
    if cand[0] is not None:
        cand = [c.cpu().numpy() for c in cand]
        assert np.all(cand[0][stored:] == MARK) and np.all(cand[1][stored:] == MARK) and np.all(cand[2][stored:] == MARK8)
        cand = [c[:stored] for c in cand]
    return rc, int(total.value), [b[:count] for b in best], coff, cand


def same(got, want):
    return np.array_equal(np.asarray(got).astype(np.uint64), np.asarray(want).astype(np.uint64))


def check(ctx, idx, text, sa, queries, min_len, max_occ, k, base_offset=0, front=FRONT, back=BACK):
    """One call against the oracle: all three of the candidates, cand_off and the per-query best."""
    blob, off = column(queries, front, back)
    rc, total, best, coff, cand = raw_map(ctx, idx, blob, off, min_len, max_occ, k, base_offset)
    assert rc == host.OK
    w = mp.index_map(text, sa, queries, min_len, max_occ, k, base_offset)
    what = (text[:30], min_len, max_occ, k)
    assert total == w[3][-1] and np.array_equal(coff, w[3]), what
    for g, x, name in zip(cand, w[4:], ("cand_start", "cand_end", "cand_dist")):
        bad = np.flatnonzero(g.astype(np.uint64) != x.astype(np.uint64))
        assert bad.size == 0, (name, what, bad[:5], g[bad[:5]], x[bad[:5]])
    for g, x, name in zip(best, w[:3], ("best_start", "best_end", "best_dist")):
        assert same(g, x), (name, what, g, x)
    return w


@pytest.mark.parametrize("name", list(io.ALPHABETS))
def test_small_texts_in_full(name, ctx):
    alpha = io.ALPHABETS[name]
    rng = np.random.default_rng(0x4D + len(alpha))
    for n in (1, 2, 3, 7, 8, 9, 33, 64):
        text = io.random_text(rng, n, alpha)
        queries = queries_for(rng, name, text, k=4) + [text[:40] or b"a"] * (max(text) < 0x80)
        with ctx.index(on_device(text, n % 3)) as idx:
            sa = idx.sa.cpu().numpy()
            for k in (0, 1, 3):
                for min_len, max_occ in ((1, 1), (1, 4), (2, 64)):
                    check(ctx, idx, text, sa, queries, min_len, max_occ, k, front=3 + n % 4)


# ---- word boundaries of the walker ---------------------------------------------------------------------------------------

LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512)
LETTERS = bytes(range(97, 123))


def boundary_text():
    rng = np.random.default_rng(0xB0D)
    return bytes(LETTERS[int(x)] for x in rng.integers(0, 26, 1500))


ROWS = (0, 62, 63, 64, 65, -1)  # -1: row m - 1


def boundary_reads(text):
    """Per length one read for every (row, kind) that exists: row in 0, 62, 63, 64, 65, m - 1 below m, kind in
    substitution, insertion, deletion.  Each read is cut from the text at a place of its own and carries that one edit:
    row r replaced; a byte put in front of row r (the rows behind move up, the last one falls off); or the text byte of
    row r left out (the rows behind move down, the next text byte fills the end).  234 reads in all."""
    rng = np.random.default_rng(0xB0E)
    reads = {}
    for m in LENGTHS:
        out = []
        for r in sorted({m - 1 if r < 0 else r for r in ROWS if r < m}):
            for kind in range(3):
                at = int(rng.integers(0, len(text) - m - 1))
                src = bytearray(text[at:at + m + 1])
                c = next(x for x in LETTERS if x != src[r])
                if kind == 0:
                    src[r] = c
                elif kind == 1:
                    src.insert(r, c)
                else:
                    del src[r]
                out.append(bytes(src[:m]))
        reads[m] = out
    assert sum(map(len, reads.values())) == 234
    return reads


@pytest.mark.parametrize("k", (0, 1, 4, 64))
def test_word_boundaries_of_the_walker(k, ctx):
    text = boundary_text()
    reads = boundary_reads(text)
    with ctx.index(on_device(text, 1)) as idx:
        sa = idx.sa.cpu().numpy()
        mixed = [r for m in LENGTHS for r in reads[m]]
        order = np.random.default_rng(3).permutation(len(mixed))
        mixed = [mixed[int(j)] for j in order]  # masked upper words and lanes that finish early share waves
        w = check(ctx, idx, text, sa, mixed, 12 if k < 64 else 8, 8, k)
        if k:  # one edit each: every read long enough to have a seed maps, which the reads of 1 and 2 bytes are not
            assert int((w[2] != mp.NO_HIT).sum()) == len(mixed) - len(reads[1]) - len(reads[2])
        if k == 4:  # every instance alone: the longest seeded read decides
            for top in (64, 128, 256, 512):
                alone = [r for m in LENGTHS if top // 2 < m <= top or (top == 64 and m <= 64) for r in reads[m]]
                assert max(map(len, alone)) == top
                check(ctx, idx, text, sa, alone, 12, 8, 4)
        if k <= 1:  # reads of 1 and 2 bytes with seeds of their own: every occurrence of their bytes is a candidate
            w = check(ctx, idx, text, sa, reads[1] + reads[2], 1, 4096, k)
            assert w[3][-1] > 100 and np.all(w[2] <= k)


# ---- window clipping -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pad", (0, 1, 7))
def test_window_clipping(pad, ctx):
    rng = np.random.default_rng(0xC1 + pad)
    text = bytes(LETTERS[int(x)] for x in rng.integers(0, 26, 400))
    k = 3
    reads = [text[:70], text[2:72], text[-70:], text[-72:-2],       # occurrences within k of both ends
             b"qrs" + text[:60], text[-60:] + b"zyx",                # diagonals -3 and past n - m: seeds at qpos > p
             text[1:40] + b"q" + text[40:90], text[300:340] + text[341:]]
    assert b"qrs" not in text and b"zyx" not in text
    with ctx.index(on_device(text, pad)) as idx:
        sa = idx.sa.cpu().numpy()
        w = check(ctx, idx, text, sa, reads, 10, 4, k)
        assert np.all(w[2] <= k)  # all of them map
        assert int(w[0][4]) <= k and int(w[1][5]) >= len(text) - 1 - k  # ... the two with clipped windows at the very ends
    short = text[100:130]  # n < m: the window is the whole text
    with ctx.index(on_device(short, pad)) as idx:
        w = check(ctx, idx, short, idx.sa.cpu().numpy(), [text[98:134], text[100:130] + b"abcdefgh", text[90:140]], 8, 4, 6)
        assert w[2].tolist() == [6, mp.NO_HIT, mp.NO_HIT]


# ---- ties and many candidates ----------------------------------------------------------------------------------------------

def test_ties_and_many_candidates(ctx):
    one = b"a" * 3000
    unit = b"abaabab"
    seven = (unit * 430)[:3000]
    for text in (one, seven):
        src = text[11:111]
        reads = [src[:40], src[:100], src[:20] + b"b" + src[21:40] if text is one else src[:20] + b"bb" + src[22:40]]
        with ctx.index(on_device(text, 3)) as idx:
            sa = idx.sa.cpu().numpy()
            for max_occ in (1, 16, 4096):
                w = check(ctx, idx, text, sa, reads, 15, max_occ, 2)
                if max_occ < 4096:
                    assert np.all(w[2] == mp.NO_HIT)  # every seed is dropped: nothing replaces it
                else:
                    assert w[2][0] == 0 and w[3][-1] > 1000
    # most queries without a seed at all
    rng = np.random.default_rng(0x7E)
    text = bytes(LETTERS[int(x)] for x in rng.integers(0, 13, 2000))
    reads = [bytes(LETTERS[13 + int(x)] for x in rng.integers(0, 13, 30)) for _ in range(600)]
    for j in (5, 299, 300, 599):
        reads[j] = text[j:j + 30]
    with ctx.index(on_device(text)) as idx:
        w = check(ctx, idx, text, idx.sa.cpu().numpy(), reads, 10, 4, 1)
        assert np.flatnonzero(w[2] != mp.NO_HIT).tolist() == [5, 299, 300, 599]


# ---- capacity and outputs ----------------------------------------------------------------------------------------------

def small_case():
    rng = np.random.default_rng(0xCA)
    text = bytes(LETTERS[int(x)] for x in rng.integers(0, 4, 600))
    reads, _, _ = mp.edit_reads(rng, text, 40, 30, 2, LETTERS[:4])
    return text, reads


def test_capacity_and_outputs(ctx):
    text, reads = small_case()
    base = (1 << 40) + 3
    with ctx.index(on_device(text, 7)) as idx:
        sa = idx.sa.cpu().numpy()
        w = check(ctx, idx, text, sa, reads, 6, 8, 2, base_offset=base, front=5, back=9)  # capacity 0, then == total
        total = int(w[3][-1])
        assert total > 50 and int((w[2] != mp.NO_HIT).sum()) > 20
        blob, off = column(reads, 5, 9)
        assert int(off[0]) % 8 and any(int(o) % 8 for o in off[1:])
        for cap in (total - 1, 1, total + 3):
            rc, got_total, best, coff, cand = raw_map(ctx, idx, blob, off, 6, 8, 2, base, capacity=cap)
            assert rc == (host.ERR_CAPACITY if cap < total else host.OK) and got_total == total
            assert np.array_equal(coff, w[3])
            for g, x in zip(cand, w[4:]):
                assert g.size == min(cap, total) and same(g, x[:cap])  # the stored prefix
            for g, x in zip(best, w[:3]):
                assert same(g, x)  # complete either way
        rc, got_total, best, coff, cand = raw_map(ctx, idx, blob, off, 6, 8, 2, base, capacity=0, cand_off=False)
        assert rc == host.OK and got_total == total and coff is None and all(same(g, x) for g, x in zip(best, w[:3]))
        # Index.map: tensors made here, and the caller's used as given
        import torch

        got = idx.map((blob, off), 6, 8, 2, base_offset=base, candidates=True)
        want = list(w[:3]) + [w[3]] + list(w[4:])
        assert all(same(g.cpu().numpy(), x) for g, x in zip(got, want))
        out = (torch.empty(len(reads), dtype=torch.int64, device="cuda"), torch.empty(len(reads), dtype=torch.int64, device="cuda"),
               torch.empty(len(reads), dtype=torch.uint8, device="cuda"))
        got = idx.map(reads, 6, 8, 2, out=out)
        assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out)) and len(got) == 3
        assert all(same(g.cpu().numpy(), x) for g, x in zip(got, mp.index_map(text, sa, reads, 6, 8, 2)[:3]))


# ---- bad input on the device ---------------------------------------------------------------------------------------------

def test_device_side_errors(ctx):
    import torch

    text = b"the quick brown fox jumps over the lazy dog"
    blob = np.frombuffer(b"quickfoxdog", np.uint8).copy()
    good = np.array([0, 5, 8, 11], np.uint64)
    with ctx.index(on_device(text, 0)) as idx:
        sa = idx.sa.cpu().numpy()

        def rc_of(blob_np, off_np):
            with pytest.raises(host.BmxError) as e:
                idx.map((torch.from_numpy(blob_np.copy()).cuda(), torch.from_numpy(off_np.astype(np.int64)).cuda()), 2, 4, 1)
            return e.value.rc

        def fine():
            got = idx.map((blob, good), 2, 4, 1)
            assert got[0].tolist() == [4, 16, 40] and got[1].tolist() == [8, 18, 42] and got[2].tolist() == [0, 0, 0]

        fine()
        assert rc_of(blob, np.array([0, 8, 5, 11])) == host.ERR_ARG  # a decreasing offset
        fine()
        assert rc_of(blob, np.array([0, 5, 8, 12])) == host.ERR_ARG  # an end past pat_bytes
        high = blob.copy()
        high[9] = 0x80
        assert rc_of(high, good) == host.ERR_DOMAIN  # a byte >= 0x80
        fine()
        long_blob = np.full(host.MAX_PATTERN + 1, ord("a"), np.uint8)
        assert rc_of(long_blob, np.array([0, long_blob.size])) == host.ERR_ARG  # 513 bytes
        fine()
        other = host.Context(0)  # an index of another context
        try:
            d_blob, d_off, count = idx._queries((blob, good))
            o = torch.zeros(3, dtype=torch.int64, device="cuda")
            o8 = torch.zeros(3, dtype=torch.uint8, device="cuda")
            total = C.c_uint64(0)
            rc = ctx._L.bmx_index_map_device(other._h, idx._h, C.c_void_p(d_blob.data_ptr()), d_blob.numel(),
                                             C.c_void_p(d_off.data_ptr()), count, 2, 4, 1, 0, C.c_void_p(o.data_ptr()),
                                             C.c_void_p(o.data_ptr()), C.c_void_p(o8.data_ptr()), None, None, None, None, 0,
                                             C.byref(total), None)
            assert rc == host.ERR_ARG
        finally:
            other.close()
        fine()
        check(ctx, idx, text, sa, [b"quick", b"fax", b"lazy dig"], 2, 4, 1)


# ---- streams ---------------------------------------------------------------------------------------------------------------

def test_streams(ctx):
    """The null stream; a caller's non-blocking stream with delayed work in front (the blob the call reads holds a decoy
    until a copy behind the delay replaces it); two calls with different k on one context in a row."""
    import torch

    text, reads = small_case()
    decoy = [r[::-1] for r in reads]
    with ctx.index(on_device(text, 0)) as idx:
        sa = idx.sa.cpu().numpy()
        want = {k: mp.index_map(text, sa, reads, 6, 8, k) for k in (0, 2)}
        assert not np.array_equal(want[0][2], want[2][2])
        assert not np.array_equal(mp.index_map(text, sa, decoy, 6, 8, 2)[2], want[2][2])
        blob, off = host.pack_strings(reads)
        dblob, doff = host.pack_strings(decoy)
        assert np.array_equal(off, doff)
        for k in (2, 0, 2):  # the null stream, different k in a row
            got = idx.map((blob, off), 6, 8, k, candidates=True)
            assert all(same(g.cpu().numpy(), x) for g, x in zip(got, list(want[k][:3]) + [want[k][3]] + list(want[k][4:])))
        real = torch.from_numpy(blob.copy()).cuda()
        d_blob = torch.from_numpy(dblob.copy()).cuda()
        d_off = torch.from_numpy(off.astype(np.int64)).cuda()
        s, keep = side_stream_with_delay()
        with torch.cuda.stream(s):
            d_blob.copy_(real, non_blocking=True)
            pending = torch.cuda.Event()
            pending.record(s)
            assert not pending.query(), "delay too short: the producer had finished before the call"
            got = idx.map((d_blob, d_off), 6, 8, 2, candidates=True)
            assert all(same(g.cpu().numpy(), x) for g, x in zip(got, list(want[2][:3]) + [want[2][3]] + list(want[2][4:])))
        del keep
        torch.cuda.empty_cache()


# ---- the planted case of the CPU suite -------------------------------------------------------------------------------------

def test_planted_case_through_every_entry(ctx, tmp_path):
    text, reads, starts, edits = planted_case()
    k = PLANTED["k"]
    with ctx.index(on_device(text, 0)) as idx:
        w = check(ctx, idx, text, idx.sa.cpu().numpy(), reads, PLANTED["min_len"], PLANTED["max_occ"], k)
        bs, be, bd = (x.cpu().numpy() for x in idx.map(reads, PLANTED["min_len"], PLANTED["max_occ"], k))
        assert check_planted(bs, bd, starts, edits, k) == 48
    hs, he, hd = ctx.index_map(text, reads, PLANTED["min_len"], PLANTED["max_occ"], k)  # the host entry
    assert same(hs, w[0]) and same(he, w[1]) and same(hd, w[2])
    full = ctx.index_map(text, reads, PLANTED["min_len"], PLANTED["max_occ"], k, candidates=True)
    assert all(same(g, x) for g, x in zip(full, list(w[:3]) + [w[3]] + list(w[4:])))
    # the host entry's own lists: a capacity above the total, the total, and one below it (the stored prefix)
    blob, off = host.pack_strings(reads)
    total = int(w[3][-1])
    for cap in (total + 5, total, total - 1):
        best = [np.full(48 + EXTRA, MARK, np.int64), np.full(48 + EXTRA, MARK, np.int64), np.full(48 + EXTRA, MARK8, np.uint8)]
        coff = np.full(49 + EXTRA, MARK, np.int64)
        cand = [np.full(cap + EXTRA, MARK, np.int64), np.full(cap + EXTRA, MARK, np.int64), np.full(cap + EXTRA, MARK8, np.uint8)]
        got_total = C.c_uint64(0)
        rc = ctx._L.bmx_index_map(ctx._h, text, len(text), C.c_void_p(blob.ctypes.data), blob.size, C.c_void_p(off.ctypes.data), 48,
                                  PLANTED["min_len"], PLANTED["max_occ"], k, *[C.c_void_p(o.ctypes.data) for o in best],
                                  C.c_void_p(coff.ctypes.data), *[C.c_void_p(o.ctypes.data) for o in cand], cap, C.byref(got_total))
        assert rc == (host.ERR_CAPACITY if cap < total else host.OK) and got_total.value == total
        stored = min(cap, total)
        assert all(same(g[:48], x) for g, x in zip(best, w[:3])) and same(coff[:49], w[3])
        assert all(same(g[:stored], x[:stored]) for g, x in zip(cand, w[4:]))
        marks = (MARK, MARK, MARK8)
        assert all(np.all(g[48:] == v) for g, v in zip(best, marks)) and np.all(coff[49:] == MARK)
        assert all(np.all(g[stored:] == v) for g, v in zip(cand, marks))
    (tmp_path / "text.txt").write_bytes(text)
    (tmp_path / "reads.txt").write_bytes(b"\n".join(reads) + b"\n")
    cli = os.path.join(ROOT, "parallel_implementation_of_string_matching_algorithms_opencl_amd", "bin", "bmx_cli")
    out = subprocess.run([cli, "--index-map", str(tmp_path / "reads.txt"), "--text", str(tmp_path / "text.txt"), "--min-len",
                          str(PLANTED["min_len"]), "--max-occ", str(PLANTED["max_occ"]), "--approx", str(k)], check=True,
                         capture_output=True, timeout=120).stdout
    both = subprocess.run([cli, "--index-map", str(tmp_path / "reads.txt"), "--index-seeds", str(tmp_path / "reads.txt"), "--text",
                           str(tmp_path / "text.txt"), "--min-len", "20", "--max-occ", "8", "--approx", "4"], capture_output=True,
                          timeout=120)
    assert both.returncode == 2 and b"exclude each other" in both.stderr and both.stdout == b""
    lines = out.decode().split("\n")[:-1]
    assert lines[:-1] == ["%d %d %d %d" % (q, w[0][q], w[1][q], w[2][q]) for q in range(48)]
    assert lines[-1] == "mapped 48 of 48, candidates %d" % w[3][-1]
