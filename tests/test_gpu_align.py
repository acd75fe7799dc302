"""GPU suite for the alignments (bmx_align*, host.Context.align_device): every distance, every offset and every op word
against tests/align_oracle.py, at the smallest shapes at which each part can go wrong: the word boundaries of every
instance crossed with k, spans shorter and longer than the pattern, spans at both ends of the text, every alignment of
the text, counts around a wave, mixed lengths in one wave, every way to name an entry's pattern, entries without an
alignment among good ones, gap-heavy pairs, capacities, base offsets, bad entries, a caller's stream, one context over
many calls, several launches per call, and the entries that pass a CIGAR through (spans, map, the CLI).  Outputs arrive
filled with a mark that must survive beyond `count` and `capacity`."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import align_oracle as al
from conftest import ROOT
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host
from test_gpu_index import on_device, side_stream_with_delay

pytestmark = pytest.mark.gpu

MARK, MARK8, MARK32 = -7, 0xA5, 0x5EEDBEEF
EXTRA = 4  # marked entries behind count and behind capacity
NO_POS = al.NO_POS
LENGTHS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512)
CLI = os.path.join(ROOT, "parallel_implementation_of_string_matching_algorithms_opencl_amd", "bin", "bmx_cli")


def raw_align(ctx, d_text, patterns, starts, ends, k, pid=None, base_offset=0, capacity=None, pat_count=None, stream=None,
              n=None):
    """bmx_align_device into marked arrays: (rc, total, dist, op_off, ops) as numpy.  capacity None: a counting call first
    (capacity 0, NULL ops, NULL dist), then the exact room.  patterns: a list of bytes or a (blob, off) numpy pair."""
    import torch

    blob, off = host.pack_strings(patterns)
    d_blob = torch.from_numpy(np.concatenate([blob, np.zeros(1, np.uint8)])).cuda()
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    d_start = torch.from_numpy(np.asarray(starts, dtype=np.uint64).view(np.int64).copy()).cuda()
    d_end = torch.from_numpy(np.asarray(ends, dtype=np.uint64).view(np.int64).copy()).cuda()
    d_pid = None if pid is None else torch.from_numpy(np.asarray(pid, dtype=np.uint32).view(np.int32).copy()).cuda()
    count = d_start.numel()
    total = C.c_uint64(0)
    s = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def call(cap, with_out):
        dist = torch.full((count + EXTRA,), MARK8, dtype=torch.uint8, device="cuda") if with_out else None
        op_off = torch.full((count + 1 + EXTRA,), MARK, dtype=torch.int64, device="cuda")
        ops = torch.full((cap + EXTRA,), MARK32, dtype=torch.int32, device="cuda") if with_out else None
        rc = ctx._L.bmx_align_device(ctx._h, ptr(d_text), d_text.numel() if n is None else n, base_offset, ptr(d_blob), blob.size,
                                     ptr(d_off), off.size - 1 if pat_count is None else pat_count, ptr(d_pid), ptr(d_start),
                                     ptr(d_end), count, k, ptr(dist), ptr(op_off), ptr(ops), cap, C.byref(total), s)
        return rc, dist, op_off, ops

    if capacity is None:
        rc, _, off0, _ = call(0, False)
        assert rc == host.OK, host.lib().bmx_last_error()
        capacity = int(total.value)
        rc, dist, op_off, ops = call(capacity, True)
        assert torch.equal(off0, op_off), "the offsets depend on the capacity"
    else:
        rc, dist, op_off, ops = call(capacity, True)
    if rc not in (host.OK, host.ERR_CAPACITY):
        return rc, int(total.value), None, None, None
    dist, op_off, ops = dist.cpu().numpy(), op_off.cpu().numpy(), ops.cpu().numpy().view(np.uint32)
    assert np.all(dist[count:] == MARK8) and np.all(op_off[count + 1:] == MARK) and np.all(ops[capacity:] == MARK32)
    assert int(op_off[count]) == total.value
    return rc, int(total.value), dist[:count], op_off[:count + 1].astype(np.uint64), ops[:capacity]


def check(ctx, text, patterns, starts, ends, k, pid=None, base_offset=0, pad=0, want=None, ctx_text=None):
    """One call against the oracle; returns the oracle's answer."""
    d_text = ctx_text if ctx_text is not None else on_device(text, pad)
    rc, total, dist, op_off, ops = raw_align(ctx, d_text, patterns, starts, ends, k, pid, base_offset)
    assert rc == host.OK
    w = want or al.align(text, patterns, starts, ends, k, pid, base_offset)
    bad = np.flatnonzero(dist != w[0])
    assert bad.size == 0, ("dist", k, bad[:5], dist[bad[:5]], w[0][bad[:5]])
    bad = np.flatnonzero(op_off != w[1])
    assert bad.size == 0, ("op_off", k, bad[:5], op_off[bad[:5]], w[1][bad[:5]])
    assert total == w[2].size and np.array_equal(ops, w[2]), ("ops", k, host.cigar_strings(op_off, ops)[:5],
                                                                host.cigar_strings(w[1], w[2])[:5])
    return w


def letters(rng, n, sigma=4):
    return bytes((97 + rng.integers(0, sigma, n)).astype(np.uint8))


def edited(rng, pat: bytes, subs=0, ins=0, dels=0, sigma=4) -> bytes:
    """A span made from the pattern: `subs` bytes changed, `ins` pattern bytes dropped, `dels` text bytes added."""
    s = bytearray(pat)
    for _ in range(subs):
        at = int(rng.integers(0, len(s)))
        s[at] = 97 + (s[at] - 97 + 1 + int(rng.integers(0, sigma - 1))) % sigma
    for _ in range(ins):
        if len(s) > 1:
            del s[int(rng.integers(0, len(s)))]
    for _ in range(dels):
        s.insert(int(rng.integers(0, len(s) + 1)), 97 + int(rng.integers(0, sigma)))
    return bytes(s)


class Layout:
    """A text made of spans with filler between them, and the entries that name them."""

    def __init__(self, rng):
        self.rng, self.parts, self.at = rng, [], 0
        self.patterns, self.starts, self.ends = [], [], []

    def add(self, pat: bytes, span: bytes, gap=None):
        gap = int(self.rng.integers(0, 6)) if gap is None else gap
        self.parts += [letters(self.rng, gap), span]
        self.patterns.append(pat)
        self.starts.append(self.at + gap)
        self.ends.append(self.at + gap + len(span) - 1)
        self.at += gap + len(span)

    def add_no_hit(self, pat: bytes):
        self.patterns.append(pat)
        self.starts.append(NO_POS)
        self.ends.append(NO_POS)

    def text(self, tail=None) -> bytes:
        return b"".join(self.parts) + letters(self.rng, int(self.rng.integers(0, 6)) if tail is None else tail)


# ---- word boundaries of every instance, crossed with k ------------------------------------------------------------------------

@pytest.mark.parametrize("m", LENGTHS)
def test_word_boundaries_crossed_with_k(m, ctx):
    rng = np.random.default_rng(0xA1 + m)
    for k in (0, 1, 3, 8, 64):
        if k > 2 * m:  # (k <= m + L: the entry is meaningful)
            continue
        lay = Layout(rng)
        for d in sorted({0, 1, k // 2, k}):
            if d > k:
                continue
            pat = letters(rng, m)
            lay.add(pat, edited(rng, pat, subs=d))
            if m - d >= 1:
                lay.add(pat, edited(rng, pat, ins=d))  # a span of m - d bytes
            lay.add(pat, edited(rng, pat, dels=d))  # ... and of m + d
            lay.add(pat, edited(rng, pat, subs=d // 3, ins=min(d // 3, m - 1), dels=d - 2 * (d // 3)))
        pat = letters(rng, m)
        lay.add(pat, edited(rng, pat, dels=k + 1))  # |L - m| > k
        lay.add(pat, letters(rng, m, sigma=26))  # unrelated: over k unless k is large
        lay.add_no_hit(pat)
        w = check(ctx, lay.text(), lay.patterns, lay.starts, lay.ends, k, pad=m % 8)
        assert np.count_nonzero(w[0] != al.NONE) >= 3 and w[0][-1] == al.NONE and w[0][-3] == al.NONE


def test_k_254_at_m_512(ctx):
    rng = np.random.default_rng(0x254)
    lay = Layout(rng)
    pat = letters(rng, 512)
    lay.add(pat, edited(rng, pat, subs=80, ins=80, dels=80))
    lay.add(b"a" * 512, b"a" * (512 - 254))
    lay.add(b"a" * 512, b"a" * (512 + 254))
    lay.add(pat, letters(rng, 512))  # unrelated: about 0.4 m edits
    lay.add(b"a" * 512, b"a" * 257)  # |L - m| = 255 > k
    w = check(ctx, lay.text(), lay.patterns, lay.starts, lay.ends, 254)
    assert host.cigar_strings(w[1], w[2])[1:3] == ["254I258=", "254D512="] and w[0][4] == al.NONE and w[0][0] <= 240


@pytest.mark.parametrize("m,k", [(9, 3), (40, 8), (200, 64)])
def test_gap_heavy_pairs(m, k, ctx):
    rng = np.random.default_rng(m)
    lay = Layout(rng)
    for pat, span in ((b"a" * m, b"a" * (m - k)), (b"a" * m, b"a" * (m + k)), (b"ab" * (m // 2), b"ba" * (m // 2)),
                      (b"a" * m, b"b" * m), (b"a" * m, b"a" * (m - k - 1)), (b"a" * m, b"a" * (m + k + 1))):
        lay.add(pat, span, gap=3)  # (the filler is over a, b, c, d: the spans' neighbours may continue a run)
    w = check(ctx, lay.text(), lay.patterns, lay.starts, lay.ends, k)
    assert host.cigar_strings(w[1], w[2])[:2] == [f"{k}I{m - k}=", f"{k}D{m}="] and list(w[0][-2:]) == [al.NONE] * 2


# ---- where the span lies: both ends of the text, every alignment of the buffer ----------------------------------------------

@pytest.mark.parametrize("pad", range(16))
def test_spans_at_both_ends_of_the_text_at_every_alignment(pad, ctx):
    rng = np.random.default_rng(0xE0 + pad)
    lay = Layout(rng)
    first = letters(rng, 20 + pad)
    lay.add(first, edited(rng, first, subs=1, dels=1), gap=0)  # begins at text byte 0
    for m in (5, 13, 70):
        pat = letters(rng, m)
        lay.add(pat, edited(rng, pat, subs=1, ins=1), gap=pad % 5)
    last = letters(rng, 33)
    lay.add(last, edited(rng, last, ins=2), gap=1)
    text = lay.text(tail=0)  # ends at byte n - 1
    assert lay.starts[0] == 0 and lay.ends[-1] == len(text) - 1
    whole = edited(rng, text, subs=2, ins=1)  # ... and one span that is the whole text
    lay.patterns.append(whole), lay.starts.append(0), lay.ends.append(len(text) - 1)
    w = check(ctx, text, lay.patterns, lay.starts, lay.ends, 3, pad=pad)
    assert np.all(w[0] != al.NONE)


# ---- counts, mixed lengths, the three ways to name an entry's pattern, entries without an alignment -------------------------

@functools.lru_cache(maxsize=None)
def mixed_case(count: int, longest: int, seed: int):
    """`count` entries over patterns of 1 .. longest bytes (every length of a wave differs), up to 3 edits each; one
    entry in eight is a read without a hit, one has one edit too many spread over the span, one is too long for k."""
    rng = np.random.default_rng(seed)
    lay, k = Layout(rng), 3
    for e in range(count):
        m = 1 + (e * 37 + int(rng.integers(0, 3))) % longest if longest > 64 else int(rng.integers(1, longest + 1))
        pat = letters(rng, m)
        kind = int(rng.integers(0, 8))
        if kind == 0:
            lay.add_no_hit(pat)
        elif kind == 1:
            lay.add(pat, edited(rng, pat, dels=k + 1 + int(rng.integers(0, 3))))
        elif kind == 2:
            lay.add(pat, edited(rng, pat, subs=min(m, 5), sigma=26))
        else:
            lay.add(pat, edited(rng, pat, subs=int(rng.integers(0, 2)), ins=int(rng.integers(0, 2)), dels=int(rng.integers(0, 2))))
    text = lay.text()
    return text, lay.patterns, lay.starts, lay.ends, k, al.align(text, lay.patterns, lay.starts, lay.ends, k)


@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
def test_counts_around_a_wave_with_lengths_1_to_512_mixed(count, ctx):
    text, patterns, starts, ends, k, want = mixed_case(count, 512, 0xC0 + count)
    check(ctx, text, patterns, starts, ends, k, want=want, pad=count % 8)


def test_5000_entries_and_one_context_over_growing_and_shrinking_calls(ctx):
    text, patterns, starts, ends, k, want = mixed_case(5000, 48, 0x5000)
    assert 400 < np.count_nonzero(want[0] == al.NONE) < 2500
    d_text = on_device(text, 5)
    for count in (1, 5000, 63, 257, 5000, 64):
        w = al.align(text, patterns[:count], starts[:count], ends[:count], k) if count != 5000 else want
        check(ctx, text, patterns[:count], starts[:count], ends[:count], k, want=w, ctx_text=d_text)
    assert ctx.last_align_launches() == 1 and ctx.last_align_ms() > 0
    # a long pattern after short ones and back: another instance, a larger workspace, the same context
    t2, p2, s2, e2, k2, w2 = mixed_case(65, 512, 0xC0 + 65)
    check(ctx, t2, p2, s2, e2, k2, want=w2)
    check(ctx, text, patterns[:300], starts[:300], ends[:300], k, ctx_text=d_text)


def test_pid_one_pattern_for_all_and_one_per_entry(ctx):
    rng = np.random.default_rng(0x91D)
    pats = [letters(rng, m) for m in (7, 30, 64, 65, 200)]
    lay, pid = Layout(rng), []
    for e in range(130):
        p = int(rng.integers(0, len(pats)))
        pid.append(p)
        lay.add(pats[p], edited(rng, pats[p], subs=e % 2, ins=e % 3 == 0, dels=e % 5 == 0))
    text = lay.text()
    check(ctx, text, pats, lay.starts, lay.ends, 3, pid=pid)  # pid given: 5 patterns, 130 entries
    check(ctx, text, lay.patterns, lay.starts, lay.ends, 3)  # pat_count == count
    check(ctx, text, lay.patterns, lay.starts, lay.ends, 3, pid=list(range(130)))  # ... and the same through pid
    one = [e for e in range(130) if pid[e] == 2]
    w = check(ctx, text, [pats[2]], [lay.starts[e] for e in one], [lay.ends[e] for e in one], 3)  # pat_count == 1
    assert len(one) > 5 and np.all(w[0] != al.NONE)
    check(ctx, text, [pats[2]], [lay.starts[one[0]]], [lay.ends[one[0]]], 3)  # a single entry: 1 == count


# ---- capacity, base offset ---------------------------------------------------------------------------------------------------

def test_capacity_zero_exact_and_one_below(ctx):
    text, patterns, starts, ends, k, want = mixed_case(257, 512, 0xC0 + 257)
    last = max(e for e in range(257) if want[1][e + 1] > want[1][e])  # (the last entry with a script)
    count = last + 1
    w = al.align(text, patterns[:count], starts[:count], ends[:count], k)
    exact = int(w[1][-1])
    d_text = on_device(text, 1)
    rc, total, dist, op_off, ops = raw_align(ctx, d_text, patterns[:count], starts[:count], ends[:count], k, capacity=0)
    assert rc == host.OK and total == exact and np.array_equal(op_off, w[1]) and np.array_equal(dist, w[0])
    rc, total, dist, op_off, ops = raw_align(ctx, d_text, patterns[:count], starts[:count], ends[:count], k, capacity=exact)
    assert rc == host.OK and np.array_equal(ops, w[2])
    rc, total, dist, op_off, ops = raw_align(ctx, d_text, patterns[:count], starts[:count], ends[:count], k, capacity=exact - 1)
    assert rc == host.ERR_CAPACITY and total == exact and np.array_equal(op_off, w[1]) and np.array_equal(dist, w[0])
    kept = int(w[1][last])  # every entry but the last is complete
    assert kept > 0 and np.array_equal(ops[:kept], w[2][:kept])
    rc, total, dist, op_off, ops = raw_align(ctx, d_text, patterns[:count], starts[:count], ends[:count], k, capacity=exact + 9)
    assert rc == host.OK and np.array_equal(ops[:exact], w[2]) and np.all(ops[exact:] == MARK32)


@pytest.mark.parametrize("base", [1, (1 << 40) + 3, (1 << 63) + 5])
def test_base_offset(base, ctx):
    text, patterns, starts, ends, k, want = mixed_case(65, 512, 0xC0 + 65)
    shift = lambda v: [x if x == NO_POS else x + base for x in v]
    check(ctx, text, patterns, shift(starts), shift(ends), k, base_offset=base, want=want)


# ---- bad entries on the device entry ----------------------------------------------------------------------------------------

def test_every_kind_of_bad_entry_returns_err_arg(ctx):
    text = b"xxabcdxxabxdxxacdxx"
    d_text = on_device(text, 3)
    pats = [b"abcd"] * 3
    good = dict(starts=[2, 8, 14], ends=[5, 11, 16])
    blob, off = host.pack_strings(pats)
    u64 = lambda *v: np.array(v, dtype=np.uint64)
    long_blob = np.full(521, 97, dtype=np.uint8)
    bad = {
        "pid >= pat_count": dict(good, pid=[0, 3, 1]),
        "offsets decrease": dict(good, patterns=(blob, u64(0, 8, 4, 12))),
        "offsets past the blob": dict(good, patterns=(blob, u64(0, 4, 8, 13))),
        "a pattern of 0 bytes": dict(good, patterns=(blob, u64(0, 4, 4, 12))),
        "a pattern of 513 bytes": dict(good, patterns=(long_blob, u64(0, 4, 517, 521))),
        "start below base_offset": dict(good, base_offset=3),
        "end at n": dict(starts=[2, 8, 14], ends=[5, 11, 19]),
        "end < start": dict(starts=[2, 8, 14], ends=[5, 7, 16]),
        "start NO_POS alone": dict(starts=[2, NO_POS, 14], ends=[5, 11, 16]),
        "end NO_POS alone": dict(starts=[2, 8, 14], ends=[5, NO_POS, 16]),
    }
    for what, kw in bad.items():
        kw = dict(dict(patterns=pats), **kw)
        rc = raw_align(ctx, d_text, kw.pop("patterns"), kw.pop("starts"), kw.pop("ends"), 1, capacity=16, **kw)[0]
        assert rc == host.ERR_ARG, what
        assert "bmx_align_device" in host.lib().bmx_last_error().decode(), what
    w = check(ctx, text, pats, good["starts"], good["ends"], 1, ctx_text=d_text)  # the context is fine afterwards
    assert host.cigar_strings(w[1], w[2]) == ["4=", "2=1X1=", "1=1I2="]


# ---- a caller's stream ------------------------------------------------------------------------------------------------------

def test_on_a_callers_non_blocking_stream_with_work_queued_before_and_behind(ctx):
    """The lists the entry reads hold a decoy; the real ones are copied over them on the caller's non-blocking stream
    behind a long delay, and the entry is called while that copy is outstanding.  Work of the library that is not ordered
    behind the caller's stream reads the decoy, whose answer differs.  Behind the call the stream copies the answer on."""
    import torch

    text, patterns, starts, ends, k, want = mixed_case(257, 512, 0xC0 + 257)
    d_text = on_device(text, 2)
    to_dev = lambda v: torch.from_numpy(np.asarray(v, dtype=np.uint64).view(np.int64).copy()).cuda()
    real_s, real_e = to_dev(starts), to_dev(ends)
    d_start, d_end = to_dev([NO_POS] * 257), to_dev([NO_POS] * 257)  # the decoy: no entry has an alignment
    blob, off = host.pack_strings(patterns)
    d_pats = (torch.from_numpy(blob.copy()).cuda(), torch.from_numpy(off.astype(np.int64)).cuda())
    got = ctx.align_device(d_text, d_pats, d_start, d_end, k)
    assert int(got[1][-1]) == 0 and bool((got[0] == al.NONE).all())
    s, keep = side_stream_with_delay()
    with torch.cuda.stream(s):
        d_start.copy_(real_s, non_blocking=True)
        d_end.copy_(real_e, non_blocking=True)
        pending = torch.cuda.Event()
        pending.record(s)
        assert not pending.query(), "delay too short: the producer had finished before the call"
        dist, op_off, ops = ctx.align_device(d_text, d_pats, d_start, d_end, k, stream=s)
        behind = [torch.empty_like(t) for t in (dist, op_off, ops)]
        for dst, src in zip(behind, (dist, op_off, ops)):
            dst.copy_(src, non_blocking=True)
    s.synchronize()
    assert np.array_equal(behind[0].cpu().numpy(), want[0])
    assert np.array_equal(behind[1].cpu().numpy().astype(np.uint64), want[1])
    assert np.array_equal(behind[2].cpu().numpy().view(np.uint32), want[2])
    del keep
    torch.cuda.empty_cache()


# ---- more entries than one launch's workspace holds -------------------------------------------------------------------------

def test_several_launches_give_the_same_lists(exp_ctx):
    text, patterns, starts, ends, k, want = mixed_case(5000, 48, 0x5000)
    d_text = on_device(text, 7)
    exp_ctx.set_knob("align_ws_kib", 3 * 1024)  # about 1 MiB of columns and slots per launch
    check(exp_ctx, text, patterns, starts, ends, k, want=want, ctx_text=d_text)
    several = exp_ctx.last_align_launches()
    assert 1 < several < 79, several
    exp_ctx.set_knob("align_ws_kib", 1)  # one wave per launch
    check(exp_ctx, text, patterns, starts, ends, k, want=want, ctx_text=d_text)
    assert exp_ctx.last_align_launches() == (5000 + 63) // 64
    rc, total, dist, op_off, ops = raw_align(exp_ctx, d_text, patterns, starts, ends, k, capacity=int(want[1][2000]) + 1)
    assert rc == host.ERR_CAPACITY and np.array_equal(op_off, want[1])
    assert np.array_equal(ops[:int(want[1][2000])], want[2][:int(want[1][2000])])
    t2, p2, s2, e2, k2, w2 = mixed_case(257, 512, 0xC0 + 257)  # 8 words per column: five waves, five launches
    check(exp_ctx, t2, p2, s2, e2, k2, want=w2)
    assert exp_ctx.last_align_launches() == 5
    exp_ctx.set_knob("align_ws_kib", 0)
    check(exp_ctx, text, patterns, starts, ends, k, want=want, ctx_text=d_text)
    assert exp_ctx.last_align_launches() == 1


# ---- end to end: spans, map, the CLI ------------------------------------------------------------------------------------------

EXAMPLE_TEXT, EXAMPLE_PAT = b"xxabcdxxabxdxxacdxx", b"abcd"


def test_spans_with_cigar_on_the_worked_example(ctx):
    plain = ctx.search_approx_spans(EXAMPLE_TEXT, EXAMPLE_PAT, 1)
    starts, ends, dist, scripts = ctx.search_approx_spans(EXAMPLE_TEXT, EXAMPLE_PAT, 1, best=True, cigar=True)
    assert len(plain) == 3 and all(np.array_equal(a, b) for a, b in zip(plain, (starts, ends, dist)))
    assert starts.tolist() == [2, 8, 14] and ends.tolist() == [5, 11, 16] and scripts == ["4=", "2=1X1=", "1=1I2="]
    every = ctx.search_approx_spans(EXAMPLE_TEXT, EXAMPLE_PAT, 1, best=False, cigar=True)
    assert every[3] == [al.cigar(al.script(EXAMPLE_PAT, EXAMPLE_TEXT[s:e + 1])[1]) for s, e in zip(every[0], every[1])]
    d, off, ops = ctx.align(EXAMPLE_TEXT, [EXAMPLE_PAT], starts, ends, 1)  # the host entry itself, and the module's
    assert d.tolist() == dist.tolist() and host.cigar_strings(off, ops) == scripts
    d, off, ops = ctx.align(EXAMPLE_TEXT, [EXAMPLE_PAT], starts + np.uint64(9), ends + np.uint64(9), 0, base_offset=9)
    assert d.tolist() == [0, al.NONE, al.NONE] and host.cigar_strings(off, ops) == ["4=", "", ""]


def test_spans_with_cigar_on_16_mib_with_planted_edited_copies(ctx):
    rng = np.random.default_rng(0x16)
    n, m, k, every = 16 << 20, 32, 3, 64 << 10
    text = (32 + rng.integers(0, 95, n)).astype(np.uint8)
    pat = bytes((32 + rng.integers(0, 95, m)).astype(np.uint8))
    planted = {}
    for c, at in enumerate(range(1000, n - 100, every)):
        copy = bytearray(pat)
        where, kind = 1 + c % (m - 2), c % 3
        if kind == 0:
            copy[where] = 32 + (copy[where] - 32 + 1) % 95
        elif kind == 1:
            del copy[where]
        else:
            copy.insert(where, 32 + (copy[where] - 32 + 1) % 95)
        text[at:at + len(copy)] = np.frombuffer(bytes(copy), np.uint8)
        planted[at] = bytes(copy)
    starts, ends, dist, scripts = ctx.search_approx_spans(text, pat, k, best=True, cigar=True)
    raw = text.tobytes()
    assert len(scripts) == starts.size >= len(planted) == 256
    for s, e, d, got in zip(starts.tolist(), ends.tolist(), dist.tolist(), scripts):
        want_d, runs = al.script(pat, raw[s:e + 1])
        # (a BEST span's distance is the smallest over all starts for its end, and its start attains it)
        assert (d, got) == (want_d, al.cigar(runs)), (s, e)
    found = dict(zip(starts.tolist(), zip(ends.tolist(), dist.tolist(), scripts)))
    hits = [at for at, copy in planted.items() if at in found and found[at][0] == at + len(copy) - 1 and found[at][1] == 1]
    assert len(hits) >= 250 and all(sum(c in "XID" for c in found[at][2]) == 1 for at in hits)
    assert {re.sub(r"\d+", "", found[at][2]) for at in hits} >= {"=X=", "=I=", "=D="}


def test_index_map_with_cigar_on_256_reads(ctx):
    rng = np.random.default_rng(0x256)
    text = letters(rng, 1 << 16)
    reads, edits = [], []
    for r in range(256):
        at = int(rng.integers(0, len(text) - 120))
        subs, ins, dels = r % 2, r % 3 == 0, r % 5 == 0
        reads.append(edited(rng, text[at:at + 100], subs=subs, ins=int(ins), dels=int(dels)))
        edits.append(subs + ins + dels)
    with ctx.index(on_device(text, 3)) as idx:
        plain = idx.map(reads, 12, 8, 4)
        bs, be, bd, scripts = idx.map(reads, 12, 8, 4, cigar=True)
        assert len(plain) == 3 and all(bool((a == b).all()) for a, b in zip(plain, (bs, be, bd)))
        full = idx.map(reads, 12, 8, 4, base_offset=77, candidates=True, cigar=True)
        assert len(full) == 8 and full[7] == scripts
    bs, be, bd = bs.cpu().numpy(), be.cpu().numpy(), bd.cpu().numpy()
    mapped = 0
    for r in range(256):
        if bd[r] == host.MAP_NO_HIT:
            assert scripts[r] == ""
            continue
        d, runs = al.script(reads[r], text[int(bs[r]):int(be[r]) + 1])
        assert (int(bd[r]), scripts[r]) == (d, al.cigar(runs)) and d <= edits[r]
        mapped += 1
    assert mapped >= 250 and {c for s in scripts for c in s if not c.isdigit()} == set("=XID")
    host_res = ctx.index_map(text, reads, 12, 8, 4, cigar=True)  # the host entries: bmx_index_map, then bmx_align
    assert len(host_res) == 4 and host_res[3] == scripts and np.array_equal(host_res[2], bd)
    assert len(ctx.index_map(text, reads, 12, 8, 4)) == 3


def run_cli(*args):
    r = subprocess.run([CLI, *args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


def test_cli_lines_with_and_without_cigar(ctx, tmp_path):
    tp, pp, rp = (str(tmp_path / f) for f in ("text.txt", "pat.txt", "reads.txt"))
    open(tp, "wb").write(EXAMPLE_TEXT)
    open(pp, "wb").write(EXAMPLE_PAT)
    base = ("--approx", "1", "--spans", "--best", "--text", tp, "--pattern", pp, "--iters", "1")
    plain, with_c = run_cli(*base), run_cli(*base, "--cigar")
    stable = lambda lines: [re.sub(r"\(.*? ms\)", "", x) for x in lines if "time" not in x.lower()]
    at = next(i for i, line in enumerate(plain) if line.startswith("match spans (best): 3"))
    # without the flag: the lines as they have always been, `start end dist`
    assert plain[at + 1:at + 4] == ["2 5 0", "8 11 1", "14 16 1"] and len(plain) == len(with_c) == at + 4
    assert with_c[at + 1:] == ["2 5 0 4=", "8 11 1 2=1X1=", "14 16 1 1=1I2="]
    assert stable(plain[:at + 1]) == stable(with_c[:at + 1])

    rng = np.random.default_rng(0xC11)
    text = letters(rng, 4000)
    reads = [edited(rng, text[at:at + 60], subs=r % 2, ins=int(r % 3 == 0), dels=int(r % 4 == 0)) for r, at in enumerate(range(50, 3800, 300))]
    reads.append(b"zzzzzzzzzzzzzzzzzzzzzzzz")
    open(tp, "wb").write(text)
    open(rp, "wb").write(b"\n".join(reads) + b"\n")
    base = ("--index-map", rp, "--text", tp, "--min-len", "10", "--max-occ", "4", "--approx", "3")
    plain, with_c = run_cli(*base), run_cli(*base, "--cigar")
    assert len(plain) == len(with_c) == len(reads) + 1 and plain[-1] == with_c[-1] and plain[-1].startswith("mapped ")
    assert plain[-2] == with_c[-2] == f"{len(reads) - 1} - - -"
    for r, (a, b) in enumerate(zip(plain[:-2], with_c[:-2])):
        assert re.fullmatch(r"\d+ \d+ \d+ \d+", a), a  # the format without the flag
        q, s, e, d = (int(x) for x in a.split())
        dist, runs = al.script(reads[q], text[s:e + 1])
        assert q == r and d == dist and b == f"{a} {al.cigar(runs)}", (a, b)
    bad = subprocess.run([CLI, "--cigar", "--text", tp, "--pattern", pp], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "--cigar" in bad.stderr
