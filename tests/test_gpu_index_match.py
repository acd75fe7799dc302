"""GPU suite for the text index's matching statistics and seeds (bmx_index_match*, bmx_index_seeds*, host.Index.match /
.seeds): every len, lo, cnt and every seed against tests/match_oracle.py, at the smallest shapes at which each part can go
wrong.  Small texts are held to the oracle in full (len by bytes.find, the interval by index_oracle.sa_range over the
index's array).  On the larger texts len is held to bytes.find and (lo, cnt) to Index.count of the matched prefixes
written out as queries of their own, which tests/test_gpu_index.py holds to brute force.  Blobs carry unused bytes in front
and behind, offsets that are no multiples of 8, and outputs that arrive filled with a mark that must survive outside the
queries."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import index_oracle as io
import match_oracle as mo
from conftest import ROOT
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host
from test_gpu_index import on_device, side_stream_with_delay
from test_index_match_cpu import queries_for

pytestmark = pytest.mark.gpu

MARK = -7
FRONT, BACK = 3, 5


def column(queries, front=FRONT, back=BACK):
    """(blob, offsets) with `front` unused bytes before the first query and `back` behind the last."""
    blob, off = host.pack_strings(queries)
    pad = lambda k: np.full(k, ord("a"), np.uint8)
    return np.concatenate([pad(front), blob, pad(back)]), off + np.uint64(front)


def run_match(idx, blob, off):
    """Index.match into marked arrays of the caller: (len, lo, cnt) as int64 numpy, the marks checked."""
    import torch

    d_blob = torch.from_numpy(blob).cuda()
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    outs = [torch.full((blob.size,), MARK, dtype=torch.int32, device="cuda") for _ in range(3)]
    got = idx.match((d_blob, d_off), *outs)
    a, b = int(off[0]), int(off[-1])
    res = []
    for g, o in zip(got, outs):
        assert g.data_ptr() == o.data_ptr()
        v = o.cpu().numpy().astype(np.int64)
        assert np.all(v[:a] == MARK) and np.all(v[b:] == MARK), "a blob byte outside every query was written"
        res.append(v)
    return res


def prefixes_as_queries(blob, lens):
    """The matched prefix blob[b : b + lens[b]] of every byte with lens[b] > 0 as a column: (bytes with one, (blob, offsets))."""
    at = np.flatnonzero(lens > 0)
    ln = lens[at]
    ends = np.cumsum(ln)
    within = np.arange(int(ends[-1]) if at.size else 0) - np.repeat(ends - ln, ln)
    return at, (blob[np.repeat(at, ln) + within], np.concatenate([[0], ends]).astype(np.uint64))


def want_lens(text, blob, off):
    want = np.full(blob.size, MARK, np.int64)
    cache = {}
    for a, b in zip(off[:-1], off[1:]):
        q = blob[int(a):int(b)].tobytes()
        if q not in cache:
            cache[q] = mo.matching_statistics(text, q)
        want[int(a):int(b)] = cache[q]
    return want


def check_seeds(idx, blob, off, lens, lo, cnt, settings):
    for min_len, max_occ in settings:
        want = mo.seeds_from_arrays(off, lens, lo, cnt, min_len, max_occ)
        got = idx.seeds((blob, off), min_len, max_occ)
        for w, g, what in zip(want, got, ("seed_off", "qpos", "len", "lo", "cnt")):
            assert np.array_equal(g.cpu().numpy().astype(np.int64), w), (what, min_len, max_occ)


def verify(ctx, d_text, text: bytes, queries, full=True, seed_settings=((1, 0), (2, 0), (2, 2)), front=FRONT, back=BACK, idx=None):
    """match and seeds of a column against the oracle; returns (blob, off, len, lo, cnt) as checked."""
    blob, off = column(queries, front, back)
    own = idx is None
    idx = ctx.index(d_text) if own else idx
    try:
        lens, lo, cnt = run_match(idx, blob, off)
        want = want_lens(text, blob, off)
        bad = np.flatnonzero(lens != want)
        assert bad.size == 0, (text[:40], bad[:5], lens[bad[:5]], want[bad[:5]])
        inside = lens != MARK
        assert np.all(lo[inside & (lens == 0)] == 0) and np.all(cnt[inside & (lens == 0)] == 0)
        if full:
            sa = idx.sa.cpu().numpy()
            keys = io.suffix_keys(text, sa)
            for a, b in zip(off[:-1], off[1:]):
                a, b = int(a), int(b)
                wlo, wcnt = mo.intervals(text, sa, blob[a:b].tobytes(), lens[a:b], keys)
                assert np.array_equal(lo[a:b], wlo) and np.array_equal(cnt[a:b], wcnt), (text[:40], blob[a:b].tobytes())
        else:
            at, pre = prefixes_as_queries(blob, np.where(inside, lens, 0))
            clo, ccnt = idx.count(pre)
            assert np.array_equal(lo[at], clo.cpu().numpy()) and np.array_equal(cnt[at], ccnt.cpu().numpy())
            assert np.all(cnt[at] >= 1)
        check_seeds(idx, blob, off, lens, lo, cnt, seed_settings)
    finally:
        if own:
            idx.close()
    return blob, off, lens, lo, cnt


@pytest.mark.parametrize("name", list(io.ALPHABETS))
def test_small_texts_in_full(name, ctx):
    alpha = io.ALPHABETS[name]
    rng = np.random.default_rng(0x3A + len(alpha))
    for n in (1, 2, 3, 7, 8, 9, 33, 64):
        text = io.random_text(rng, n, alpha)
        queries = queries_for(rng, name, text, k=24)
        queries += [queries[0][:1], queries[1][:2], queries[2][:3]]  # one byte left, a bucket alone, one byte behind it
        verify(ctx, on_device(text, n % 3), text, queries, front=3 + n % 4, back=5)


def test_end_of_text_rule(ctx):
    """Queries that run past the text's last bytes with 95, 96 and 97 as the next byte (the virtual symbol sits between 95 and
    96), on texts of both parities whose last bytes are neighbours of byte 96."""
    tails = [bytes([a]) for a in b"_`aA"] + [bytes([a, b]) for a in b"_`a" for b in b"_`aA"]
    texts = sorted({p + t for p in (b"x", b"xa") for t in tails if not (p + t).endswith(b"``")} | {b"xA`", b"Ab`A`", b"`", b"a`", b"_`a`"})
    assert {len(t) % 2 for t in texts} == {0, 1} and len(texts) > 30
    for text in texts:
        queries = [text[i:] + bytes([b]) + more for i in range(len(text)) for b in (95, 96, 97) for more in (b"", b"x")]
        queries += [b"z" + text[-1:] + b"`", text + text]
        verify(ctx, on_device(text, len(text) % 3), text, queries, seed_settings=((1, 0),))


def test_query_limits_and_a_whole_long_query(ctx):
    rng = np.random.default_rng(0x512)
    text = bytes((rng.integers(0, 4, 3000) + 97).astype(np.uint8))
    whole = text[1203:1203 + host.MAX_PATTERN]
    blob, off, lens, lo, cnt = verify(ctx, on_device(text, 1), text, [b"a", whole, b"z", whole[:511] + b"z"], full=False)
    a = int(off[1])
    assert np.array_equal(lens[a:a + 512], 512 - np.arange(512)) and lens[int(off[0])] == 1 and lens[int(off[2])] == 0
    assert np.array_equal(lens[int(off[3]):int(off[3]) + 512], np.concatenate([511 - np.arange(511), [0]]))


def test_long_common_prefixes_one_letter(ctx):
    n, m = 70_000, host.MAX_PATTERN
    text = b"a" * n
    blob, off = column([b"a" * m, b"a" * 300 + b"b" + b"a" * 100])
    with ctx.index(on_device(text, 3)) as idx:
        lens, lo, cnt = run_match(idx, blob, off)
        a, b = int(off[0]), int(off[1])
        # a suffix of l bytes is entry l - 1 of the array (shorter ones are below longer ones)
        want = m - np.arange(m)
        assert np.array_equal(lens[a:b], want) and np.array_equal(lo[a:b], want - 1) and np.array_equal(cnt[a:b], n - want + 1)
        want2 = np.concatenate([300 - np.arange(300), [0], 100 - np.arange(100)])
        assert np.array_equal(lens[b:b + 401], want2)
        assert np.array_equal(lo[b:b + 401], np.maximum(want2 - 1, 0)) and np.array_equal(cnt[b:b + 401], np.where(want2 > 0, n - want2 + 1, 0))
        check_seeds(idx, blob, off, lens, lo, cnt, ((1, 0), (101, 0), (1, n - 300)))
        seed_off, qpos, ln, _, _ = idx.seeds((blob, off), 1)
        assert seed_off.tolist() == [0, 1, 3] and qpos.tolist() == [0, 0, 301] and ln.tolist() == [512, 300, 100]


def test_long_common_prefixes_period_seven(ctx):
    unit, n = b"abaabab", 1 << 16
    text = (unit * (n // 7 + 1))[:n]
    long_unit = unit * 75
    broken = bytearray(long_unit[3:3 + 512])
    broken[200] = ord("b") if broken[200] == ord("a") else ord("a")
    queries = [long_unit[2:2 + 512], bytes(broken), long_unit[5:5 + 97]]
    verify(ctx, on_device(text, 1), text, queries, full=False, seed_settings=((1, 0), (150, 0), (1, 9000)))


def test_directory_edges(ctx, exp_ctx):
    """A query's last position (one byte left: no bucket), an empty two-byte bucket whose first byte occurs (len 1), a byte
    that occurs nowhere (len 0), a text with bytes >= 0x80; and the same answers with the directory switched off."""
    rng = np.random.default_rng(0xD1)
    pool = np.array([0, 1, 0x5F, 0x60, 0x61, 0x7E, 0x7F, 0x80, 0xFF, 0x62], np.uint8)
    t = bytearray(pool[rng.integers(0, pool.size, 300)].tobytes())
    t[10:12], t[20:22], t[-1] = b"\x00\x00", b"\x7f\x7f", 0x7F
    text = bytes(t)
    while b"ab" in text:  # 'a' and 'b' occur, "ab" does not
        text = text.replace(b"ab", b"aa")
    assert b"a" in text and b"b" in text and b"ab" not in text and b"q" not in text and max(text) >= 0x80
    valid = [i for i in range(len(text) - 9) if max(text[i:i + 9]) < 0x80]
    assert len(valid) >= 1
    queries = [b"ab", b"abab\x00", b"q", b"qa", b"aq", b"a", b"\x7f\x7f\x7f", b"\x00\x00\x00", b"\x01q\x01"]
    queries += [text[i:i + 9] for i in valid[:6]] + [text[i:i + 4] + b"q" + text[i + 4:i + 9] for i in valid[:6]]
    d_text = on_device(text, 5)
    blob, off, lens, lo, cnt = verify(ctx, d_text, text, queries)
    a = int(off[0])
    assert lens[a:a + 2].tolist() == [1, 1] and cnt[a] == text.count(b"a") and lens[int(off[2])] == 0
    exp_ctx.set_knob("index_no_dir", 1)
    with exp_ctx.index(d_text) as plain:
        again = run_match(plain, blob, off)
        assert all(np.array_equal(x, y) for x, y in zip(again, (lens, lo, cnt)))
    exp_ctx.set_knob("index_no_dir", 0)


def mutated_reads(rng, text: bytes, count: int, m: int, letters: bytes, every: int):
    """`count` reads of m bytes cut from the text with one byte in every `every` replaced by a random letter."""
    out = []
    for at in rng.integers(0, len(text) - m, count):
        r = bytearray(text[int(at):int(at) + m])
        for k in range(0, m, every):
            r[k + int(rng.integers(0, min(every, m - k)))] = letters[int(rng.integers(0, len(letters)))]
        out.append(bytes(r))
    return out


def test_beyond_one_workgroup_long_queries(ctx):
    """Queries of 300 bytes: query boundaries and the predecessors of seeds fall across workgroups of 256 lanes."""
    rng = np.random.default_rng(0x300)
    letters = b"abcdefgh"
    text = bytes(np.frombuffer(letters, np.uint8)[rng.integers(0, 8, 4096)])
    queries = mutated_reads(rng, text, 24, 300, letters, 40)
    blob, off, lens, lo, cnt = verify(ctx, on_device(text, 2), text, queries, full=False, seed_settings=((1, 0), (12, 0), (4, 3)))
    assert any(int(o) % 256 not in (0, 255) for o in off[1:-1]) and lens.max() >= 40 and (lens == 0).sum() == 0


def test_beyond_one_grid_turn_many_short_queries(ctx):
    rng = np.random.default_rng(0x10003)
    letters = b"abcdefgh"
    text = bytes(np.frombuffer(letters, np.uint8)[rng.integers(0, 8, 4096)]) + b"z"
    Q = (1 << 16) + 3
    ms = rng.integers(1, 7, Q)
    raw = np.frombuffer(letters + b"zq", np.uint8)[rng.integers(0, 10, int(ms.sum()))]
    ends = np.cumsum(ms)
    queries = [raw[int(e - m):int(e)].tobytes() for e, m in zip(ends, ms)]
    verify(ctx, on_device(text, 0), text, queries, full=False, seed_settings=((3, 0), (2, 5)))


def test_a_match_stops_at_its_querys_end(ctx):
    rng = np.random.default_rng(0xB0)
    text = bytes((rng.integers(0, 26, 500) + 97).astype(np.uint8))
    queries = [text[100:110], text[110:125], text[125:126], text[126:140], text[300:310], text[310:320]]
    blob, off, lens, lo, cnt = verify(ctx, on_device(text, 0), text, queries)
    for a, b in zip(off[:-1], off[1:]):
        assert np.array_equal(lens[int(a):int(b)], int(b - a) - np.arange(int(b - a)))
    assert text.find(blob[int(off[0]):int(off[2])].tobytes()) == 100  # the neighbours together do occur


def seed_case():
    rng = np.random.default_rng(0x5EED)
    letters = b"abcd"
    text = bytes(np.frombuffer(letters, np.uint8)[rng.integers(0, 4, 1500)])
    queries = mutated_reads(rng, text, 30, 60, letters + b"z", 15)
    queries += [text[int(a):int(a) + 2 + k % 3] for k, a in enumerate(rng.integers(0, 1400, 24))]  # short and frequent ones
    return text, queries + [b"zzzz", b"z", text[40:90]]


def test_seeds_min_len_and_max_occ(ctx):
    text, queries = seed_case()
    d_text = on_device(text, 1)
    blob, off, lens, lo, cnt = verify(ctx, d_text, text, queries, full=False, seed_settings=())
    inside = lens != MARK
    top = int(lens[inside].max())
    assert top >= 50
    some = sorted({int(c) for c in mo.seeds_from_arrays(off, lens, lo, cnt, 2, 0)[4]})  # the seeds' numbers of occurrences
    assert len(some) > 3 and some[0] == 1
    with ctx.index(d_text) as idx:
        check_seeds(idx, blob, off, lens, lo, cnt, ((top - 1, 0), (top, 0), (top + 1, 0), (2, 1), (2, some[len(some) // 2]), (1, 1)))
        seed_off, qpos, ln, slo, scnt = idx.seeds((blob, off), top + 1)
        assert seed_off.tolist() == [0] * (len(queries) + 1) and qpos.numel() == ln.numel() == slo.numel() == scnt.numel() == 0
        seed_off = idx.seeds((blob, off), 1)[0].tolist()
        assert seed_off[-4] == seed_off[-3] == seed_off[-2], "queries without a seed"
        a = mo.seeds_from_arrays(off, lens, lo, cnt, 2, 0)[0][-1]
        b = mo.seeds_from_arrays(off, lens, lo, cnt, 2, some[len(some) // 2])[0][-1]
        c = mo.seeds_from_arrays(off, lens, lo, cnt, 2, 1)[0][-1]
        assert 0 < c < b < a, "max_occ drops some seeds and keeps some"


def test_seeds_capacity(ctx):
    import torch

    text, queries = seed_case()
    d_text = on_device(text, 0)
    blob, off, lens, lo, cnt = verify(ctx, d_text, text, queries, full=False, seed_settings=())
    want = mo.seeds_from_arrays(off, lens, lo, cnt, 4, 0)
    total = int(want[0][-1])
    assert total > 50
    with ctx.index(d_text) as idx:
        d_blob, d_off, count = idx._queries((blob, off))
        d_seed_off = torch.zeros(count + 1, dtype=torch.int64, device="cuda")
        outs = [torch.full((total + 2,), MARK, dtype=torch.int32, device="cuda") for _ in range(4)]
        n_seeds = C.c_uint64(0)

        def raw(cap, with_lists=True):
            d_seed_off.fill_(-1)
            for o in outs:
                o.fill_(MARK)
            ptrs = [C.c_void_p(o.data_ptr()) if with_lists else None for o in outs]
            return ctx._L.bmx_index_seeds_device(ctx._h, idx._h, C.c_void_p(d_blob.data_ptr()), d_blob.numel(),
                                                 C.c_void_p(d_off.data_ptr()), count, 4, 0, C.c_void_p(d_seed_off.data_ptr()),
                                                 *ptrs, cap, C.byref(n_seeds), None)

        for cap, rc in ((total, host.OK), (total + 2, host.OK), (total - 1, host.ERR_CAPACITY), (7, host.ERR_CAPACITY)):
            assert raw(cap) == rc and n_seeds.value == total
            assert np.array_equal(d_seed_off.cpu().numpy(), want[0])  # always in full
            for o, w in zip(outs, want[1:]):
                v = o.cpu().numpy()
                assert np.array_equal(v[:min(cap, total)], w[:cap]) and np.all(v[min(cap, total):] == MARK)
        assert raw(0, with_lists=False) == host.ERR_CAPACITY and n_seeds.value == total
        assert np.array_equal(d_seed_off.cpu().numpy(), want[0])
        got = idx.seeds((blob, off), 4, capacity=9)
        assert int(got[0][-1]) == total and all(np.array_equal(g.cpu().numpy(), w[:9]) for g, w in zip(got[1:], want[1:]))


def test_device_side_errors(ctx):
    import torch

    text = b"the quick brown fox jumps over the lazy dog"
    d_text = on_device(text, 0)
    blob = np.frombuffer(b"quickfoxdog", np.uint8).copy()
    good = np.array([0, 5, 8, 11], np.uint64)
    with ctx.index(d_text) as idx:
        assert idx.match((blob, good))[0].tolist() == [5, 4, 3, 2, 1, 3, 2, 1, 3, 2, 1]

        def rc_of(blob_np, off_np, fn):
            with pytest.raises(host.BmxError) as e:
                fn((torch.from_numpy(blob_np.copy()).cuda(), torch.from_numpy(off_np.astype(np.int64)).cuda()))
            return e.value.rc

        for fn in (idx.match, lambda p: idx.seeds(p, 1), lambda p: idx.seeds(p, 1, capacity=4)):
            assert rc_of(blob, np.array([0, 8, 5, 11]), fn) == host.ERR_ARG  # a decreasing offset
            assert rc_of(blob, np.array([0, 5, 8, 12]), fn) == host.ERR_ARG  # an end past pat_bytes
            assert rc_of(blob, np.array([0, 5, 5, 11]), fn) == host.ERR_ARG  # a length of 0
            long_blob = np.full(host.MAX_PATTERN + 1, ord("a"), np.uint8)
            assert rc_of(long_blob, np.array([0, long_blob.size]), fn) == host.ERR_ARG  # above BMX_MAX_PATTERN
            high = blob.copy()
            high[9] = 0x80
            assert rc_of(high, good, fn) == host.ERR_DOMAIN  # a byte >= 0x80
            fn((blob, good))  # and the next valid call works
        with pytest.raises(host.BmxError) as e:
            idx.seeds((blob, good), 0)
        assert e.value.rc == host.ERR_ARG
        other = host.Context(0)
        try:
            d_blob, d_off, count = idx._queries((blob, good))
            out = torch.zeros(11, dtype=torch.int32, device="cuda")
            n_seeds = C.c_uint64(0)
            pat = (C.c_void_p(d_blob.data_ptr()), d_blob.numel(), C.c_void_p(d_off.data_ptr()), count)
            assert ctx._L.bmx_index_match_device(other._h, idx._h, *pat, C.c_void_p(out.data_ptr()), None, None, None) == host.ERR_ARG
            assert ctx._L.bmx_index_seeds_device(other._h, idx._h, *pat, 1, 0, C.c_void_p(d_off.data_ptr()), None, None, None, None,
                                                 0, C.byref(n_seeds), None) == host.ERR_ARG
            assert out.sum().item() == 0
        finally:
            other.close()


def test_callers_array_and_repeated_calls(ctx):
    """A caller's array answers like an owned one; a larger column, then a smaller one, then the larger again reuse and grow
    the workspace without a trace of the call before."""
    text, queries = seed_case()
    d_text = on_device(text, 2)
    sa = ctx.suffix_array_device(d_text)
    small, large = column(queries[:3]), column(queries * 8, front=1, back=0)
    with ctx.index(d_text, sa=sa) as borrowed, ctx.index(d_text) as owned:
        first = None
        for col in (small, large, small, large):
            a, b = run_match(borrowed, *col), run_match(owned, *col)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.array_equal(a[0], want_lens(text, *col))
            sa_, sb = borrowed.seeds(col, 3, 2), owned.seeds(col, 3, 2)
            assert all(np.array_equal(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(sa_, sb))
            want = mo.seeds_from_arrays(col[1], *a, 3, 2)
            assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(sa_, want))
            if col is small:
                first = first or (a, [x.cpu().numpy() for x in sa_])
                assert all(np.array_equal(x, y) for x, y in zip(a, first[0]))
                assert all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(sa_, first[1]))


@pytest.mark.parametrize("entry", ["match", "seeds"])
def test_device_entries_on_a_callers_stream_with_pending_work(entry, ctx):
    """The buffers the entry reads hold a decoy; the real queries are copied over them on the caller's non-blocking stream
    behind a long delay, and the entry is called while that copy is outstanding."""
    import torch

    text, queries = seed_case()
    rng = np.random.default_rng(99)
    decoy = mutated_reads(rng, text, len(queries), 60, b"abcdz", 7)
    blob, off = (x.copy() for x in host.pack_strings(queries))
    dblob, doff = (x.copy() for x in host.pack_strings(decoy))
    size = max(blob.size, dblob.size)
    real_blob = torch.zeros(size, dtype=torch.uint8, device="cuda")
    real_blob[:blob.size] = torch.from_numpy(blob).cuda()
    d_blob = torch.zeros(size, dtype=torch.uint8, device="cuda")
    d_blob[:dblob.size] = torch.from_numpy(dblob).cuda()
    real_off = torch.from_numpy(off.astype(np.int64)).cuda()
    d_off = torch.from_numpy(doff.astype(np.int64)).cuda()
    idx = ctx.index(on_device(text, 0))
    lens, lo, cnt = [x.cpu().numpy().astype(np.int64) for x in idx.match((real_blob, real_off))]
    assert np.array_equal(lens[:blob.size], want_lens(text, blob, off))
    want = mo.seeds_from_arrays(off, lens, lo, cnt, 5, 0)
    decoy_lens = idx.match((d_blob, d_off))[0].cpu().numpy()
    assert not np.array_equal(decoy_lens, lens)
    s, keep = side_stream_with_delay()
    with torch.cuda.stream(s):
        d_blob.copy_(real_blob, non_blocking=True)
        d_off.copy_(real_off, non_blocking=True)
        pending = torch.cuda.Event()
        pending.record(s)
        assert not pending.query(), "delay too short: the producer had finished before the call"
        if entry == "match":
            got = idx.match((d_blob, d_off))
            assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, (lens, lo, cnt)))
        else:
            got = idx.seeds((d_blob, d_off), 5)
            assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))
    idx.close()
    del keep
    torch.cuda.empty_cache()


def test_host_entries_and_cli(ctx, tmp_path):
    text = b"abracadabra abracadabra`"
    queries = [b"cadabrix", b"zebra", b"a`a", b"q", b"abra abra"]
    sa = io.model_order(text)
    blob, off = host.pack_strings(queries)
    lens = want_lens(text, blob, off)
    lo, cnt = (np.concatenate(x) for x in zip(*[mo.intervals(text, sa, q, lens[int(a):int(b)]) for q, a, b in zip(queries, off[:-1], off[1:])]))
    got = ctx.index_match(text, queries)
    assert all(np.array_equal(g.astype(np.int64), w) for g, w in zip(got, (lens, lo, cnt)))
    for min_len, max_occ in ((1, 0), (3, 0), (2, 2)):
        want = mo.seeds(text, sa, queries, min_len, max_occ)
        for got in (ctx.index_seeds(text, queries, min_len, max_occ), host.index_seeds(text, queries, min_len, max_occ)):
            assert all(np.array_equal(g.astype(np.int64), w) for g, w in zip(got, want)), (min_len, max_occ)
    # the C entry with a capacity below the total: the first seeds, the offsets in full
    want = mo.seeds(text, sa, queries, 1)
    seed_off = np.zeros(len(queries) + 1, np.uint64)
    outs = [np.full(3, 77, np.uint32) for _ in range(4)]
    n_seeds = C.c_uint64(0)
    p = lambda x: C.c_void_p(x.ctypes.data)
    t = np.frombuffer(text, np.uint8).copy()
    rc = ctx._L.bmx_index_seeds(ctx._h, p(t), t.size, p(blob), blob.size, p(off), len(queries), 1, 0, p(seed_off), *[p(o) for o in outs],
                                3, C.byref(n_seeds))
    assert rc == host.ERR_CAPACITY and n_seeds.value == want[0][-1] > 3 and np.array_equal(seed_off.astype(np.int64), want[0])
    assert all(np.array_equal(o.astype(np.int64), w[:3]) for o, w in zip(outs, want[1:]))

    (tmp_path / "text.txt").write_bytes(text)
    (tmp_path / "reads.txt").write_bytes(b"\n".join(queries) + b"\n\n")
    cli = os.path.join(ROOT, "parallel_implementation_of_string_matching_algorithms_opencl_amd", "bin", "bmx_cli")
    base = [cli, "--index-seeds", str(tmp_path / "reads.txt"), "--text", str(tmp_path / "text.txt")]
    for min_len, max_occ in ((1, 0), (3, 2)):
        seed_off, qpos, ln, slo, scnt = mo.seeds(text, sa, queries, min_len, max_occ)
        lines = []
        for q in range(len(queries)):
            for s in range(int(seed_off[q]), int(seed_off[q + 1])):
                first = int(io.occurrences(text, queries[q][int(qpos[s]):int(qpos[s] + ln[s])])[0])
                lines.append(b"%d %d %d %d %d\n" % (q, qpos[s], ln[s], scnt[s], first))
        lines.append(b"seeds %d\n" % seed_off[-1])
        args = base + ["--min-len", str(min_len)] + (["--max-occ", str(max_occ)] if max_occ else [])
        out = subprocess.run(args, check=True, capture_output=True, timeout=120).stdout
        assert out == b"".join(lines), (out, lines)
    assert subprocess.run(base, capture_output=True, timeout=120).returncode == 2  # --min-len is required
