"""GPU suite for the text index (bmx_index_*, host.Index): count and locate against brute force (tests/index_oracle.py),
against Context.search_device and Context.search_dict, at the smallest shapes at which each part can go wrong: every
short query over the alphabet on small texts at three buffer alignments, the end-of-text rule of the builder's order,
long common prefixes, the directory's edges, more queries than one workgroup, a caller's array and stream, capacities,
every error the device entries report, and locate, seeds, map and match in alternation over the workspaces they share."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import index_oracle as io
import map_oracle as mp
import match_oracle as mo
from conftest import ROOT
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

pytestmark = pytest.mark.gpu

SMALL_N = (1, 2, 3, 7, 8, 9, 63, 64, 65, 300)  # both parities, around one and eight 8-byte words, a few hundred
PADS = (0, 1, 7)


def on_device(text: bytes, pad: int = 0):
    """The text at byte offset `pad` of a device buffer (a view), with other bytes around it."""
    import torch

    buf = torch.full((pad + len(text) + 9,), 0x60, dtype=torch.uint8, device="cuda")
    buf[pad:pad + len(text)] = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
    return buf[pad:pad + len(text)]


def pack(queries):
    """(blob, offsets) numpy pair of a list of bytes, or of such pairs and lists concatenated."""
    blobs, offs, base = [], [np.zeros(1, np.uint64)], 0
    for part in queries if isinstance(queries, list) and queries and isinstance(queries[0], (tuple, list)) else [queries]:
        b, o = host.pack_strings(part)
        blobs.append(b)
        offs.append(o[1:] + np.uint64(base))
        base += b.size
    return np.concatenate(blobs) if blobs else np.zeros(0, np.uint8), np.concatenate(offs)


@functools.lru_cache(maxsize=None)
def exhaustive(letters: bytes, L: int):
    """Every string of L bytes over `letters`, in the order of its code sum(index(b_j) * A^(L-1-j)): (blob, offsets)."""
    A = len(letters)
    idx = np.indices((A,) * L).reshape(L, -1).T
    blob = np.frombuffer(letters, np.uint8)[idx].reshape(-1)
    return blob.copy(), np.arange(0, blob.size + 1, L, dtype=np.uint64)


def exhaustive_expected(text: bytes, letters: bytes, L: int):
    """(counts, positions in query order, ascending within a query) of every exhaustive(letters, L) query, by numpy."""
    A, t = len(letters), np.frombuffer(text, np.uint8)
    lut = np.full(256, -1, np.int64)
    lut[np.frombuffer(letters, np.uint8)] = np.arange(A)
    n_win = t.size - L + 1
    if n_win <= 0:
        return np.zeros(A ** L, np.int64), np.zeros(0, np.int64)
    digits = np.stack([lut[t[j:j + n_win]] for j in range(L)])
    ok = (digits >= 0).all(axis=0)
    code = (digits * (A ** np.arange(L - 1, -1, -1))[:, None]).sum(axis=0)[ok]
    p = np.arange(n_win)[ok]
    return np.bincount(code, minlength=A ** L), p[np.lexsort((p, code))]


def verify(ctx, d_text, text: bytes, parts, expected=None, search_device_too=()):
    """count and locate of the queries `parts` (a list of (blob, offsets) pairs and lists of bytes) against brute force:
    the counts, sa[lo : lo + cnt] as a set, the offsets, every segment ascending and equal to the occurrences."""
    import torch

    blob, off = pack(parts)
    count = off.size - 1
    if expected is None:
        occ = [io.occurrences(text, blob[int(off[i]):int(off[i + 1])].tobytes()) for i in range(count)]
        want_cnt = np.array([o.size for o in occ], np.int64)
        want_pos = np.concatenate(occ) if occ else np.zeros(0, np.int64)
    else:
        want_cnt, want_pos = expected
    with ctx.index(d_text) as idx:
        lo, cnt = idx.count((blob, off))
        lo, cnt = lo.cpu().numpy().astype(np.int64), cnt.cpu().numpy().astype(np.int64)
        assert np.array_equal(cnt, want_cnt), (text[:40], np.flatnonzero(cnt != want_cnt)[:5])
        sa = idx.sa.cpu().numpy().astype(np.int64)
        assert np.array_equal(sa, ctx.suffix_array_device(d_text).cpu().numpy())
        assert np.all(lo >= 0) and np.all(lo + cnt <= len(text))
        # sa[lo : lo + cnt] of every query, gathered in one step and sorted within its segment
        seg = np.repeat(np.arange(count), cnt)
        start = np.concatenate([[0], np.cumsum(cnt)])
        within = np.arange(seg.size) - start[seg]
        from_sa = sa[lo[seg] + within]
        assert np.array_equal(from_sa[np.lexsort((from_sa, seg))], want_pos)
        offsets, pos, total = idx.locate((blob, off), base_offset=1000)
        assert total == want_pos.size == pos.numel()
        assert np.array_equal(offsets.cpu().numpy(), start)
        assert np.array_equal(pos.cpu().numpy(), want_pos + 1000)
        out = torch.empty(len(text) + 1, dtype=torch.int64, device="cuda")
        for i in search_device_too:
            q = blob[int(off[i]):int(off[i + 1])].tobytes()
            got = pos[int(start[i]):int(start[i + 1])] - 1000
            if len(q) > len(text):
                assert got.numel() == 0
                continue
            ref, ref_total = ctx.search_device(d_text, q, out=out)
            assert ref_total == got.numel() and torch.equal(ref, got), q


def extra_queries(rng, text: bytes, letters: bytes):
    """200 substrings of up to min(n, 512) bytes, each also with 1..3 bytes appended, the suffix from each one's start with
    1..3 bytes appended (it runs over the end), the whole text and the whole text plus one byte; queries with a byte >=
    0x80 or more than 512 bytes are not valid queries and are left out."""
    n, out = len(text), []
    for _ in range(200):
        ln = int(rng.integers(1, min(n, 512) + 1))
        at = int(rng.integers(0, n - ln + 1))
        tail = bytes(letters[int(j)] for j in rng.integers(0, len(letters), int(rng.integers(1, 4))))
        out += [text[at:at + ln], text[at:at + ln] + tail, text[at:] + tail]
    out += [text, text + letters[:1], text + letters[-1:]]
    return sorted({q for q in out if 1 <= len(q) <= host.MAX_PATTERN and max(q) < 0x80})


@pytest.mark.parametrize("name", list(io.ALPHABETS))
def test_small_texts_in_full(name, ctx):
    alpha = io.ALPHABETS[name]
    letters = bytes(b for b in alpha if b < 0x80)
    rng = np.random.default_rng(0x1D + len(alpha))
    short = [exhaustive(letters, L) for L in (1, 2, 3)]
    n_short = sum(len(letters) ** L for L in (1, 2, 3))
    for n in SMALL_N:
        text = io.random_text(rng, n, alpha)
        exp = [exhaustive_expected(text, letters, L) for L in (1, 2, 3)]
        extra = extra_queries(rng, text, letters)
        occ = [io.occurrences(text, q) for q in extra]
        want = (np.concatenate([e[0] for e in exp] + [np.array([o.size for o in occ], np.int64)]),
                np.concatenate([e[1] for e in exp] + occ))
        for pad in PADS:
            verify(ctx, on_device(text, pad), text, short + [extra], expected=want,
                   search_device_too=range(n_short, n_short + len(extra)))


def test_end_of_text_rule(ctx):
    """Texts whose last 1..3 bytes are neighbours of byte 96, at both parities of n, and the named examples; queries: every
    string of 1..4 bytes over the bytes in play, every suffix plus a byte below, at and above 96."""
    letters = b"A_`ax"
    tails = [bytes(t) for L in (1, 2, 3) for t in np.frombuffer(exhaustive(b"_`aA", L)[0], np.uint8).reshape(-1, L)]
    texts = [p + t for p in (b"x", b"xx") for t in tails] + [b"xA`", b"xa`", b"x_", b"Ab`A`", b"yAb`A`", b"`", b"a`", b"_`a`"]
    texts = sorted({t for t in texts if not t.endswith(b"``")})
    assert {len(t) % 2 for t in texts} == {0, 1} and len(texts) > 100
    short = [exhaustive(letters, L) for L in (1, 2, 3, 4)]
    for text in texts:
        over = [text[i:] + bytes([b]) for i in range(len(text)) for b in (65, 95, 96, 97, 120)]
        over += [text[i:] + b"`" + bytes([b]) for i in range(len(text)) for b in (95, 96, 97)]
        assert any(q.endswith(b"`") and q[:-1] == text[len(text) - len(q) + 1:] for q in over)
        verify(ctx, on_device(text, len(text) % 3), text, short + [sorted(set(over))])


def test_long_common_prefixes_one_letter(ctx):
    import torch

    n = 70_000
    text = b"a" * n
    ms = (1, 2, 8, 9, 511, 512)
    queries = [b"a" * m for m in ms] + [b"a" * 511 + b"b", b"b", b"a" * 511 + b"`", b"a" * 300 + b"A"]
    with ctx.index(on_device(text, 3)) as idx:
        lo, cnt = idx.count(queries)
        assert cnt.tolist() == [n - m + 1 for m in ms] + [0, 0, 0, 0]
        offsets, pos, total = idx.locate(queries)
        assert total == sum(n - m + 1 for m in ms)
        off = offsets.tolist()
        for i, m in enumerate(ms):
            assert torch.equal(pos[off[i]:off[i + 1]], torch.arange(n - m + 1, device="cuda"))


def test_long_common_prefixes_period_seven(ctx):
    unit, n = b"abaabab", 1 << 16
    text = (unit * (n // 7 + 1))[:n]
    long_unit = unit * 75
    queries, want = [], []
    for phase in range(7):
        for m in range(1, 513):
            q = long_unit[phase:phase + m]
            queries.append(q)
            want.append(sum((n - m - psi) // 7 + 1 for psi in range(7) if long_unit[psi:psi + m] == q))
    with ctx.index(on_device(text, 1)) as idx:
        lo, cnt = idx.count(queries)
        assert np.array_equal(cnt.cpu().numpy(), np.array(want))
        some = [i for i, q in enumerate(queries) if len(q) in (1, 6, 7, 8, 511, 512)]
        offsets, pos, total = idx.locate([queries[i] for i in some])
        pos, off = pos.cpu().numpy(), offsets.tolist()
        assert total == sum(want[i] for i in some)
        for j, i in enumerate(some):
            assert np.array_equal(pos[off[j]:off[j + 1]], io.occurrences(text, queries[i])), queries[i][:16]


def directory_text(rng, n=5000):
    """Bytes >= 0x80 in front of and behind every bucket's bytes, the lowest bucket (0, 0) and the highest (0x7f, 0x7f)."""
    pool = np.array([0, 1, 0x5F, 0x60, 0x61, 0x7E, 0x7F, 0x80, 0xFF, 0x80], np.uint8)
    t = bytearray(pool[rng.integers(0, pool.size, n)].tobytes())
    t[10:12], t[20:22], t[-1] = b"\x00\x00", b"\x7f\x7f", 0x7F
    return bytes(t)


def test_directory_edges(ctx, exp_ctx):
    rng = np.random.default_rng(0xD12)
    text = directory_text(rng)
    every = bytes(range(128))
    parts = [exhaustive(every, 1), exhaustive(every, 2)]  # one-byte queries for every byte < 0x80, every bucket
    exp = [exhaustive_expected(text, every, L) for L in (1, 2)]
    assert exp[1][0][0] > 0 and exp[1][0][-1] > 0 and (exp[1][0] == 0).sum() > 16000  # lowest and highest bucket occupied
    valid = [i for i in range(len(text) - 8) if max(text[i:i + 3]) < 0x80]
    subs = sorted({text[i:i + int(m)] for i in valid[:400] for m in (3, 4, 8) if max(text[i:i + int(m)]) < 0x80})
    absent = [b"\x02\x03", b"\x02\x03abc", b"zz", b"zzz", b"\x00\x00\x7f\x7f\x7f", b"\x7f\x7f\x7f\x7f", b"\x7f\x7f\x00"]
    extra = subs + absent
    occ = [io.occurrences(text, q) for q in extra]
    want = (np.concatenate([e[0] for e in exp] + [np.array([o.size for o in occ], np.int64)]),
            np.concatenate([e[1] for e in exp] + occ))
    d_text = on_device(text, 5)
    verify(ctx, d_text, text, parts + [extra], expected=want)
    # the same answers when every query searches the whole array (the experiments build's switch)
    blob, off = pack(parts + [extra])
    exp_ctx.set_knob("index_no_dir", 1)
    with exp_ctx.index(d_text) as plain, ctx.index(d_text) as idx:
        lo0, cnt0 = plain.count((blob, off))
        lo1, cnt1 = idx.count((blob, off))
        assert np.array_equal(cnt0.cpu().numpy(), cnt1.cpu().numpy()) and np.array_equal(lo0.cpu().numpy(), lo1.cpu().numpy())


def test_beyond_one_grid(ctx):
    import torch

    n, Q, m = 65_536 * 256 + 4_097, 1 << 16, 10
    rng = np.random.default_rng(0xB16)
    text = (rng.integers(0, 26, n) + 97).astype(np.uint8)
    at = rng.integers(0, n - m, Q // 2)
    cut = text[at[:, None] + np.arange(m)]
    rnd = (rng.integers(0, 26, (Q // 2, m)) + 97).astype(np.uint8)
    blob = np.concatenate([cut, rnd]).reshape(-1)
    off = np.arange(0, blob.size + 1, m, dtype=np.uint64)
    pos, pid = ctx.search_dict(text, [bytes(r) for r in blob.reshape(Q, m)])
    want = np.bincount(pid, minlength=Q)
    d_text = torch.from_numpy(text).cuda()
    with ctx.index(d_text) as idx:
        lo, cnt = idx.count((blob, off))
        assert np.array_equal(cnt.cpu().numpy(), want)
        assert want[:Q // 2].min() >= 1
        offsets, p, total = idx.locate((blob, off))
        assert total == pos.size
        # every pair of the dictionary search, regrouped by pattern (ascending positions within a pattern)
        order = np.lexsort((pos, pid))
        assert np.array_equal(p.cpu().numpy().astype(np.uint64), pos[order])
    del d_text
    torch.cuda.empty_cache()


def small_case(seed=7, n=3001):
    rng = np.random.default_rng(seed)
    text = io.random_text(rng, n, b"abc`")
    queries = [text[int(a):int(a) + int(m)] for a, m in zip(rng.integers(0, n - 8, 300), rng.integers(1, 8, 300))] + [b"zz", b"c`z"]
    return text, queries


def test_callers_array_answers_like_an_owned_one(ctx):
    text, queries = small_case()
    d_text = on_device(text, 2)
    sa = ctx.suffix_array_device(d_text)
    with ctx.index(d_text, sa=sa) as borrowed, ctx.index(d_text) as owned:  # two indexes alive on one context
        assert borrowed.sa.data_ptr() == sa.data_ptr() and owned.sa.data_ptr() != sa.data_ptr()
        assert owned.build_ms > 0 and 0 < borrowed.build_ms < owned.build_ms
        a, b = borrowed.count(queries), owned.count(queries)
        assert all(np.array_equal(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(a, b))
        la, lb = borrowed.locate(queries), owned.locate(queries)
        assert la[2] == lb[2] and all(np.array_equal(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(la[:2], lb[:2]))
        want = np.concatenate([io.occurrences(text, q) for q in queries])
        assert np.array_equal(la[1].cpu().numpy(), want)
    # a destroy followed by a create at another n
    text2, queries2 = small_case(seed=8, n=777)
    verify(ctx, on_device(text2, 0), text2, [queries2])


# ---- a caller's non-blocking stream with pending work in front (the pattern of tests/stream_cases.py) -------------------

DELAY_BYTES, DELAY_COPIES = 256 << 20, 24


def side_stream_with_delay():
    import torch

    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    buf = torch.zeros(2 * DELAY_BYTES, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for i in range(DELAY_COPIES):
            a, b = (0, DELAY_BYTES) if i & 1 else (DELAY_BYTES, 0)
            buf[a:a + DELAY_BYTES].copy_(buf[b:b + DELAY_BYTES], non_blocking=True)
    return s, buf


@pytest.mark.parametrize("entry", ["create", "count", "locate"])
def test_device_entries_on_a_callers_stream_with_pending_work(entry, ctx):
    """The buffer the entry reads holds a decoy; the real input is copied over it on the caller's non-blocking stream behind
    a long delay, and the entry is called while that copy is outstanding.  Work of the library that is not ordered behind
    the caller's stream reads the decoy, whose answer differs."""
    import torch

    text, queries = small_case(seed=11)
    decoy_text, decoy_queries = small_case(seed=12)
    blob, off = pack(queries)
    dblob, doff = pack(decoy_queries)
    size = max(blob.size, dblob.size)
    want_cnt = np.array([io.occurrences(text, q).size for q in queries])
    want_pos = np.concatenate([io.occurrences(text, q) for q in queries])
    assert not np.array_equal(want_cnt, [io.occurrences(decoy_text, q).size for q in queries])
    assert not np.array_equal(want_cnt[:200], [io.occurrences(text, q).size for q in decoy_queries][:200])
    real_text = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
    d_text = torch.from_numpy(np.frombuffer(decoy_text if entry == "create" else text, np.uint8).copy()).cuda()
    real_blob = torch.zeros(size, dtype=torch.uint8, device="cuda")
    real_blob[:blob.size] = torch.from_numpy(blob).cuda()
    d_blob = torch.zeros(size, dtype=torch.uint8, device="cuda")
    d_blob[:dblob.size] = torch.from_numpy(dblob).cuda()
    real_off = torch.from_numpy(off.astype(np.int64)).cuda()
    d_off = torch.from_numpy((off if entry == "create" else doff).astype(np.int64)).cuda()
    if entry == "create":
        d_blob.copy_(real_blob)
    idx = None if entry == "create" else ctx.index(d_text)
    s, keep = side_stream_with_delay()
    with torch.cuda.stream(s):
        if entry == "create":
            d_text.copy_(real_text, non_blocking=True)
        else:
            d_blob.copy_(real_blob, non_blocking=True)
            d_off.copy_(real_off, non_blocking=True)
        pending = torch.cuda.Event()
        pending.record(s)
        assert not pending.query(), "delay too short: the producer had finished before the call"
        if entry == "create":
            idx = ctx.index(d_text)
        if entry == "locate":
            offsets, pos, total = idx.locate((d_blob, d_off))
            assert total == want_pos.size and np.array_equal(pos.cpu().numpy(), want_pos)
        else:
            lo, cnt = idx.count((d_blob, d_off))
            assert np.array_equal(cnt.cpu().numpy(), want_cnt)
    idx.close()
    del keep
    torch.cuda.empty_cache()


# ---- locate, seeds, map and match in alternation on one context: the workspaces they share -----------------------------

@functools.lru_cache(maxsize=None)
def alternation_case():
    """A text of 4,099 bytes on four letters and, in the order of the calls, what every call has to answer.  Intervals by
    the rank of the occurrences (the interval of a match is exactly its set of occurrences, test_index_match_cpu.py)."""
    rng = np.random.default_rng(0xA17E)
    letters = b"acgt"
    text = io.random_text(rng, 4099, letters)
    sa = mp.lower_case_order(text)
    rank = np.empty(len(text), np.int64)
    rank[sa.astype(np.int64)] = np.arange(len(text))

    def cut(m, edits):
        at = int(rng.integers(0, len(text) - m))
        read = bytearray(text[at:at + m])
        for j in rng.integers(0, m, edits):
            read[int(j)] = letters[int(rng.integers(0, 4))]
        return bytes(read)

    def located(queries):
        occ = [io.occurrences(text, q) for q in queries]
        return np.concatenate([[0], np.cumsum([o.size for o in occ])]), np.concatenate(occ)

    def matched(queries):
        """(len, lo, cnt) per blob byte of the packed queries."""
        cols = []
        for q in queries:
            for i, l in enumerate(mo.matching_statistics(text, q)):
                occ = io.occurrences(text, q[i:i + int(l)]) if l else np.zeros(0, np.int64)
                r = rank[occ]
                assert r.size == 0 or int(r.max() - r.min()) + 1 == r.size
                cols.append((int(l), int(r.min()) if r.size else 0, r.size))
        return [np.array(c, np.int64) for c in zip(*cols)]

    def seeded(queries, min_len):
        return mo.seeds_from_arrays(host.pack_strings(queries)[1], *matched(queries), min_len)

    six = [text[100:106], text[2000:2006], b"acgtac"]
    reads = [cut(128, 6) for _ in range(64)]
    ones = [b"a", b"c", b"g", b"t"]
    # exact, one substitution, a deletion and an insertion, random
    r2 = bytearray(text[3000:3049])
    del r2[10]
    r2.insert(30, ord("a") if r2[30] != ord("a") else ord("c"))
    maps = [text[500:548], cut(48, 1), bytes(r2[:48]), bytes(letters[int(j)] for j in rng.integers(0, 4, 48))]
    five, one_read = [text[4000:4005]], [cut(64, 3)]
    assert sum(len(r) for r in reads) == 8192 and all(len(r) == 48 for r in maps)
    want = {"six": located(six), "reads": seeded(reads, 8), "ones": located(ones), "maps": mp.index_map(text, sa, maps, 8, 8, 2),
            "five": matched(five), "one_read": seeded(one_read, 8)}
    assert want["six"][0][-1] >= 2 and min(np.diff(want["ones"][0])) > 900 and want["reads"][0][-1] > 64
    assert want["maps"][3][-1] >= 3 and sorted(want["maps"][2].tolist())[:3] == [0, 1, 2] and want["one_read"][0][-1] >= 1
    return text, sa, {"six": six, "reads": reads, "ones": ones, "maps": maps, "five": five, "one_read": one_read}, want


@pytest.mark.parametrize("stream", ["null", "side"])
def test_locate_seeds_map_and_match_in_alternation(stream, ctx):
    """One index, seven calls in a row: the per-position workspace holds sort keys, then the per-byte arrays of 8,192 blob
    bytes, then larger keys, then map's arrays with the 64-bit scan behind them, then ever less; nothing stale is read."""
    import contextlib

    import torch

    text, sa, q, want = alternation_case()
    same = lambda got, w: np.array_equal(got.cpu().numpy().astype(np.uint64), np.asarray(w).astype(np.uint64))

    def locate(name):
        offsets, pos, total = idx.locate(q[name])
        assert total == want[name][1].size and same(offsets, want[name][0]) and same(pos, want[name][1]), name

    def seeds(name):
        for g, w, what in zip(idx.seeds(q[name], 8), want[name], ("seed_off", "qpos", "len", "lo", "cnt")):
            assert same(g, w), (name, what)

    side = torch.cuda.Stream() if stream == "side" else None
    assert side is None or side.cuda_stream != 0
    with torch.cuda.stream(side) if side else contextlib.nullcontext():
        with ctx.index(on_device(text, 0)) as idx:
            assert np.array_equal(idx.sa.cpu().numpy(), sa)
            locate("six")
            seeds("reads")
            locate("ones")
            got = idx.map(q["maps"], 8, 8, 2, candidates=True)
            w = want["maps"]
            assert all(same(g, x) for g, x in zip(got, list(w[:3]) + [w[3]] + list(w[4:])))
            assert all(same(g, x) for g, x in zip(idx.match(q["five"]), want["five"]))
            seeds("one_read")
            locate("six")


def test_capacity(ctx):
    text, queries = small_case(seed=21)
    d_text = on_device(text, 0)
    occ = [io.occurrences(text, q) for q in queries]
    ends = np.cumsum([o.size for o in occ])
    total = int(ends[-1])
    last_hit = max(i for i, o in enumerate(occ) if o.size)
    assert occ[-1].size == 0 and occ[last_hit].size >= 1 and total > 100
    with ctx.index(d_text) as idx:
        offsets, pos, got = idx.locate(queries, capacity=0)
        assert got == total and pos.numel() == 0 and offsets.tolist() == [0] + ends.tolist()
        # one below the total, one segment short (the last occupied one is not stored), inside a segment, exact, roomy
        for cap in (total - 1, int(ends[last_hit]) - occ[last_hit].size, 57, total, total + 5):
            offsets, pos, got = idx.locate(queries, capacity=cap, base_offset=5)
            assert got == total and offsets.tolist() == [0] + ends.tolist()  # always written in full
            pos = pos.cpu().numpy()
            assert pos.size == min(cap, total)
            stored = [i for i in range(len(queries)) if ends[i] <= cap]  # every query whose segment ends at or below it
            assert stored == list(range(len(stored)))
            for i in stored:
                assert np.array_equal(pos[ends[i] - occ[i].size:ends[i]], occ[i] + 5), (cap, i)
        # the C entry reports the overflow
        import torch

        L, blob_off = ctx._L, idx._queries(queries)

        d_out_off = torch.zeros(len(queries) + 1, dtype=torch.int64, device="cuda")
        d_pos = torch.zeros(total, dtype=torch.int64, device="cuda")
        n_matches = C.c_uint64(0)

        def raw(cap):
            return L.bmx_index_locate_device(ctx._h, idx._h, C.c_void_p(blob_off[0].data_ptr()), blob_off[0].numel(),
                                             C.c_void_p(blob_off[1].data_ptr()), len(queries), 0, C.c_void_p(d_out_off.data_ptr()),
                                             C.c_void_p(d_pos.data_ptr()), cap, C.byref(n_matches), None)

        assert raw(total - 1) == host.ERR_CAPACITY and n_matches.value == total
        assert raw(0) == host.ERR_CAPACITY and n_matches.value == total
        assert raw(total) == host.OK and n_matches.value == total
        assert int(d_out_off[-1]) == total


def test_device_side_errors(ctx):
    import torch

    text = b"the quick brown fox jumps over the lazy dog"
    d_text = on_device(text, 0)
    blob = np.frombuffer(b"quickfoxdog", np.uint8).copy()
    good = np.array([0, 5, 8, 11], np.uint64)
    with ctx.index(d_text) as idx:
        assert idx.count((blob, good))[1].tolist() == [1, 1, 1]

        def rc_of(blob_np, off_np, fn):
            with pytest.raises(host.BmxError) as e:
                fn((torch.from_numpy(blob_np.copy()).cuda(), torch.from_numpy(off_np.astype(np.int64)).cuda()))
            return e.value.rc

        for fn in (idx.count, idx.locate):
            assert rc_of(blob, np.array([0, 8, 5, 11]), fn) == host.ERR_ARG  # a decreasing offset
            assert rc_of(blob, np.array([0, 5, 8, 12]), fn) == host.ERR_ARG  # an end past pat_bytes
            assert rc_of(blob, np.array([0, 5, 5, 11]), fn) == host.ERR_ARG  # a length of 0
            long_blob = np.full(host.MAX_PATTERN + 1, ord("a"), np.uint8)
            assert rc_of(long_blob, np.array([0, long_blob.size]), fn) == host.ERR_ARG  # above BMX_MAX_PATTERN
            high = blob.copy()
            high[9] = 0x80
            assert rc_of(high, good, fn) == host.ERR_DOMAIN  # a byte >= 0x80
            fn((blob, good))  # and the next valid call works
        assert idx.count((blob, good))[1].tolist() == [1, 1, 1]
        # an index of another context
        other = host.Context(0)
        try:
            d_blob, d_off, count = idx._queries((blob, good))
            cnt = torch.zeros(3, dtype=torch.int32, device="cuda")
            rc = ctx._L.bmx_index_count_device(other._h, idx._h, C.c_void_p(d_blob.data_ptr()), d_blob.numel(),
                                               C.c_void_p(d_off.data_ptr()), count, None, C.c_void_p(cnt.data_ptr()), None)
            assert rc == host.ERR_ARG
            n_matches = C.c_uint64(0)
            rc = ctx._L.bmx_index_locate_device(other._h, idx._h, C.c_void_p(d_blob.data_ptr()), d_blob.numel(),
                                                C.c_void_p(d_off.data_ptr()), count, 0, C.c_void_p(d_off.data_ptr()), None, 0,
                                                C.byref(n_matches), None)
            assert rc == host.ERR_ARG
        finally:
            other.close()
    # a text ending in two bytes 96
    for bad in (b"ab``", b"``", b"x```"):
        with pytest.raises(host.BmxError) as e:
            ctx.index(on_device(bad, 1))
        assert e.value.rc == host.ERR_DOMAIN
    verify(ctx, on_device(b"ab`", 1), b"ab`", [[b"`", b"b`", b"ab`", b"``", b"a"]])  # one is fine


def test_host_entry_and_cli(ctx, tmp_path):
    text = b"abracadabra abracadabra`"
    pats = [b"abra", b"a", b"cad", b"ra`", b"zebra", b"a`"]
    want = [io.occurrences(text, q) for q in pats]
    assert host.Context.index_count(ctx, text, pats).tolist() == [w.size for w in want] == [4, 10, 2, 1, 0, 1]
    (tmp_path / "text.txt").write_bytes(text)
    (tmp_path / "pats.txt").write_bytes(b"\n".join(pats) + b"\n\n")
    cli = os.path.join(ROOT, "parallel_implementation_of_string_matching_algorithms_opencl_amd", "bin", "bmx_cli")
    base = [cli, "--index-count", str(tmp_path / "pats.txt"), "--text", str(tmp_path / "text.txt"), "--iters", "2"]
    out = subprocess.run(base, check=True, capture_output=True, timeout=120).stdout
    assert out == b"".join(q + b"\t%d\n" % w.size for q, w in zip(pats, want))
    out = subprocess.run(base + ["--positions", "--max-print", "3"], check=True, capture_output=True, timeout=120).stdout
    lines = out.split(b"\n")[:-1]
    with ctx.index(on_device(text)) as idx:
        offsets, pos, total = idx.locate(pats)
        off, pos = offsets.tolist(), pos.tolist()
    for i, (q, line) in enumerate(zip(pats, lines)):
        seg = pos[off[i]:off[i + 1]]
        assert seg == want[i].tolist()
        assert line == q + b"\t%d\t" % len(seg) + b" ".join(b"%d" % p for p in seg[:3])
