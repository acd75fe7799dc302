"""GPU suite of the non-overlapping match selection, replace and extract (bmx_spans_select_device, bmx_replace_device,
bmx_extract_device, Context.sub_device / findall_device) against tests/subst_oracle.py: the selection at the edges of its
tiles (T from bmx_exp_last_launch, mostly 2^3 through the knob "select_tile_shift" so that lists of a few hundred entries
reach three levels), every list shape, input form and capacity rule; the regions of the union; replace and extract at every
alignment of text, span and replacement, at the edges of the copy's tiles, past 4 GiB; sub and findall for every kind of
search against the oracle fed with the host search's own lists and against Python's ``re``; the host-buffer forms; the three
entries on a caller's non-blocking stream behind a pending copy; the driver's --replace and --only-matching."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import rows_oracle as ro
import stream_cases as sc
import subst_oracle as so
from conftest import ROOT
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

pytestmark = pytest.mark.gpu

NONE = so.NONE
COPY_TILE = 16384  # output bytes of a tile of the copy kernel (csrc/bmx_subst_kernel.h)
SMALL_SHIFT = 3


@pytest.fixture(scope="module")
def exp(built):
    """A context of libbmx_exp.so for the module: the knob "select_tile_shift" and the session "select"."""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = host.Context(0, library=host.exp_lib())
    yield c
    c.set_knob("select_tile_shift", 0)
    c.close()


@pytest.fixture()
def small(exp):
    """The experiments context with T = 8."""
    exp.set_knob("select_tile_shift", SMALL_SHIFT)
    yield exp
    exp.set_knob("select_tile_shift", 0)


def dev(a):
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a.copy()).cuda()


def u64(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


def check_select(c, starts=None, ends=None, length=0, rows=None, merge=False):
    """The selection of the list on the device, with and without the indices, against the oracle."""
    as64 = lambda a: None if a is None else np.asarray(a).astype(np.uint64)
    starts, ends, rows = as64(starts), as64(ends), as64(rows)
    spans = so.spans_of(starts, ends, length, rows)
    want = so.merge(spans) if merge else so.select(spans)
    d = lambda a: None if a is None else dev(a)
    got = c.select_spans_device(d(starts), d(ends), length, rows=d(rows), merge=merge, index=True)
    for g, w, what in zip(got, want, ("starts", "ends", "indices")):
        assert np.array_equal(u64(g), w), (what, len(spans), merge)
    got2 = c.select_spans_device(d(starts), d(ends), length, rows=d(rows), merge=merge)
    assert len(got2) == 2 and np.array_equal(u64(got2[0]), want[0]) and np.array_equal(u64(got2[1]), want[1])
    return want


def ascending(rng, count, overlap=0.5, span=10, at=100):
    """`count` spans of `span` bytes with non-decreasing ends, about `overlap` of them overlapping their predecessor."""
    step = np.where(rng.random(count) < overlap, rng.integers(0, span, count), rng.integers(span, 3 * span, count))
    e = at + span + np.cumsum(step)
    return (e - (span - 1)).astype(np.uint64), e.astype(np.uint64)


def none_where(mask) -> np.ndarray:
    rows = np.zeros(mask.size, np.uint64)
    rows[mask] = NONE
    return rows


def sizes(T):
    return [1, 2, T - 1, T, T + 1, T * T - 1, T * T + 1, T * T + T + 1, T * T * T + 1]


# ---- select ----------------------------------------------------------------------------------------------------------------

def test_select_list_sizes_reach_three_levels(small):
    rng = np.random.default_rng(1)
    T = 1 << SMALL_SHIFT
    for count in sizes(T):
        s, e = ascending(rng, count)
        check_select(small, s, e)
        shift, levels, tiles = small.last_launch("select")
        assert (1 << shift) == T and tiles == -(-count // T)
        assert T ** levels < max(count, 2) <= T ** (levels + 1) or count == 1
    assert small.last_launch("select")[1] == 3
    starts, ends = small.select_spans_device(dev(np.zeros(0, np.uint64)), dev(np.zeros(0, np.uint64)))
    assert starts.numel() == 0 and ends.numel() == 0


def test_select_at_the_production_tile(exp):
    exp.set_knob("select_tile_shift", 0)
    rng = np.random.default_rng(2)
    check_select(exp, *ascending(rng, 5))
    T = 1 << exp.last_launch("select")[0]
    count = T * T + T + 1
    check_select(exp, *ascending(rng, count))
    assert exp.last_launch("select") == (8, 2, -(-count // T))
    check_select(exp, *ascending(rng, T + 1, overlap=0.9))
    assert exp.last_launch("select")[1] == 1


def test_select_list_shapes(small):
    rng = np.random.default_rng(3)
    T = 1 << SMALL_SHIFT
    n = T * T * T + 5 * T + 3
    i = np.arange(n, dtype=np.uint64)
    assert check_select(small, 20 * i, 20 * i + 9)[0].size == n  # all disjoint: the chain is the list
    assert check_select(small, np.zeros(n), 5 + i)[0].size == 1  # all overlapping the first: a chain of one
    check_select(small, 10 * i - (i % 2) * 5 + 5, 10 * i + 14)  # alternating
    s, e = ascending(rng, n, overlap=0.3)
    e2 = e.copy()
    for at, reach in ((T + 2, 3 * T + 1), (2 * T * T + 1, T * T + 5)):  # an end that skips three tiles, one that skips a super-tile
        e2[at:at + reach] = e2[at + reach]
        s[at + 1:at + reach] = np.minimum(s[at + 1:at + reach], e2[at] - 1)
    s[T + 2], s[2 * T * T + 1] = s[T + 2] - 3, s[2 * T * T + 1] - 3
    check_select(small, s, e2)
    check_select(small, np.sort(rng.integers(0, 4 * n, n)), None, 7)  # equal and repeated starts, one length
    e = np.sort(rng.integers(50, 2 * n, n))  # equal ends
    check_select(small, e - rng.integers(0, 9, n), e)
    # a start-sorted list with varying lengths (the dictionary search's order)
    s = np.sort(rng.integers(0, 6 * n, n))
    check_select(small, s, s + rng.integers(0, 12, n))
    # non-monotone starts under ascending ends (`abcd|c` shaped): a long match and a short one inside it
    e = 30 * np.arange(1, n + 1)
    check_select(small, np.where(np.arange(n) % 3 == 0, e - 40, e - 2), e)


def test_select_skipped_entries(small):
    rng = np.random.default_rng(4)
    T = 1 << SMALL_SHIFT
    n = T * T + 3 * T + 2
    for where in ([0, 1, 2], [T, 2 * T - 1, 3 * T], list(range(2 * T, 3 * T)), list(range(0, T * T)), list(range(n))):
        for kind in range(3):
            s, e = ascending(rng, n)
            rows = np.zeros(n, np.uint64)
            w = np.array(where)
            if kind == 0:
                s[w] = NONE
            elif kind == 1:
                e[w] = s[w] - 1
            else:
                rows[w] = NONE
            check_select(small, s, e, 0, rows)
    s, e, rows = None, None, None
    for by_start in (False, True):  # all three kinds anywhere
        e = np.sort(rng.integers(8, 4 * n, n)).astype(np.uint64)
        s = (e - rng.integers(0, 9, n).astype(np.uint64)).astype(np.uint64)
        if by_start:
            s = np.sort(rng.integers(0, 4 * n, n)).astype(np.uint64)
            e = s + rng.integers(0, 9, n).astype(np.uint64)
        kind = rng.integers(0, 8, n)
        rows = none_where(kind == 2)
        s[kind == 0] = NONE
        flip = kind == 1
        s[flip], e[flip] = e[flip] + 1, s[flip]
        check_select(small, s, e, 0, rows)


def test_select_input_forms_and_large_values(small):
    rng = np.random.default_rng(5)
    n = 300
    s, e = ascending(rng, n, span=6, at=(1 << 40) - 40 * n)
    a = check_select(small, s, e)
    b = check_select(small, s, None, 6)
    c = check_select(small, None, e, 6)
    assert all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(a, b, c)) and int(a[1][-1]) >= (1 << 40) - 40 * n
    # ends below len - 1 are skipped, not wrapped
    check_select(small, None, np.array([0, 2, 4, 5, 9, 11]), 5)


def test_select_errors_and_capacity(small):
    import torch

    rng = np.random.default_rng(6)
    s, e = ascending(rng, 200)
    bad_s, bad_e = s.copy(), e.copy()
    bad_s[150] = e[170] + 1  # an entry that starts behind the end of a later one
    bad_e[150] = bad_s[150] + 3
    with pytest.raises(host.BmxError) as err:
        small.select_spans_device(dev(bad_s), dev(bad_e))
    assert err.value.rc == host.ERR_ARG
    with pytest.raises(host.BmxError) as err:  # merge needs non-decreasing ends
        small.select_spans_device(dev(bad_s), dev(bad_e), merge=True)
    assert err.value.rc == host.ERR_ARG
    for merge in (False, True):
        want = (so.merge if merge else so.select)(so.spans_of(s, e))
        total = want[0].size
        out = tuple(torch.full((total - 1,), -7, dtype=torch.int64, device="cuda") for _ in range(3))
        n_out = C.c_uint64(0)
        d_s, d_e = dev(s), dev(e)
        args = (small._h, C.c_void_p(d_s.data_ptr()), C.c_void_p(d_e.data_ptr()), 0, 200, None, int(merge))
        rc = small._L.bmx_spans_select_device(*args, *(C.c_void_p(t.data_ptr()) for t in out), total - 1, C.byref(n_out), None)
        assert rc == host.ERR_CAPACITY and n_out.value == total  # one short: the lowest entries
        for g, w in zip(out, want):
            assert np.array_equal(u64(g), w[:total - 1])
        n_out.value = 0
        assert small._L.bmx_spans_select_device(*args, None, None, None, 0, C.byref(n_out), None) == host.OK  # counts only
        assert n_out.value == total


def test_merge(small):
    rng = np.random.default_rng(7)
    T = 1 << SMALL_SHIFT
    for count in sizes(T):
        check_select(small, *ascending(rng, count), merge=True)
        check_select(small, *ascending(rng, count, overlap=0.95), merge=True)  # regions across tiles and super-tiles
    n = T * T * T + 9
    s, e = ascending(rng, n, overlap=0.2)
    s[n - 5] = s[n // 2]  # a late span that reaches back over many earlier regions
    assert check_select(small, s, e, merge=True)[0].size < check_select(small, s[:n - 5], e[:n - 5], merge=True)[0].size
    i = np.arange(n, dtype=np.uint64)
    assert check_select(small, 4 * i, 4 * i + 3, merge=True)[0].size == n  # abutting spans stay apart
    assert check_select(small, 4 * i, 4 * i + 4, merge=True)[0].size == 1  # overlapping by one byte: one region
    rows = none_where(rng.random(n) < 0.2)
    s, e = ascending(rng, n, overlap=0.6)
    s[rng.random(n) < 0.1] = NONE
    check_select(small, s, e, 0, rows, merge=True)
    check_select(small, np.full(9, NONE), np.arange(9), merge=True)  # nothing but skipped entries
    check_select(small, np.full(9, NONE), np.arange(9))


# ---- replace and extract ---------------------------------------------------------------------------------------------------

def placed(t: np.ndarray, align: int, pad: int = 64):
    """The numpy text on the device with its first byte at `align` within a 16-byte line."""
    import torch

    buf = torch.zeros(t.size + pad, dtype=torch.uint8, device="cuda")
    skew = (align - buf.data_ptr()) % 16
    d = buf[skew:skew + t.size]
    d.copy_(torch.from_numpy(t))
    return d


def check_copy(c, t, starts, ends, repls=(b"",), align=0, out_align=None, base=0, length=0):
    """Replace (with every replacement) and extract of the spans on the device against the oracle; the output tensor sits
    between guard bytes that must survive."""
    import torch

    text = t.tobytes()
    d_text = placed(t, align)
    starts = None if starts is None else np.asarray(starts).astype(np.uint64)
    ends = None if ends is None else np.asarray(ends).astype(np.uint64)
    lst = starts if starts is not None else ends
    os_ = starts if starts is not None else ends - np.uint64(length - 1)
    oe = ends if ends is not None else starts + np.uint64(length - 1)
    d_s, d_e = (None if starts is None else dev(starts)), (None if ends is None else dev(ends))
    for repl in repls:
        want = so.replace(text, os_, oe, repl, base)
        if out_align is None:
            got, n_out = c.replace_device(d_text, d_s, d_e, repl, length, base_offset=base)
        else:
            guard = torch.full((len(want) + 96,), 0xA5, dtype=torch.uint8, device="cuda")
            skew = 32 + (out_align - (guard.data_ptr() + 32)) % 16
            got, n_out = c.replace_device(d_text, d_s, d_e, repl, length, base_offset=base, out=guard[skew:skew + len(want)])
            g = guard.cpu().numpy()
            assert np.all(g[:skew] == 0xA5) and np.all(g[skew + len(want):] == 0xA5), "bytes outside the output were written"
        assert n_out == len(want)
        assert got.cpu().numpy().tobytes() == want, (t.size, lst.size, len(repl), align, out_align)
    blob, off = c.extract_device(d_text, d_s, d_e, length, base_offset=base)
    want_blob, want_off = so.extract(text, os_, oe, base)
    assert np.array_equal(u64(off), want_off) and blob.cpu().numpy().tobytes() == want_blob


def random_disjoint(rng, n, count, longest=9):
    """`count` ascending, pairwise disjoint spans inside [0, n)."""
    cuts = np.sort(rng.choice(n, 2 * count, replace=False))
    s, e = cuts[0::2], np.minimum(cuts[1::2] - 1, cuts[0::2] + longest - 1)
    return s.astype(np.uint64), np.maximum(s, e).astype(np.uint64)


def test_copy_sizes_alignments_and_replacement_lengths(ctx):
    rng = np.random.default_rng(8)
    for n in (1, 15, 16, 17, 4097):
        t = rng.integers(0, 256, n).astype(np.uint8)
        s, e = random_disjoint(rng, n, max(1, min(n // 4, 40)), 5) if n > 1 else (np.array([0]), np.array([0]))
        check_copy(ctx, t, s, e, (b"", b"x", b"0123456789abcdefg"))
        check_copy(ctx, t, np.array([0]), np.array([n - 1]), (b"", b"whole"))  # one span that is the whole text
        check_copy(ctx, t, np.zeros(0), np.zeros(0), (b"zz",))  # no span: the text itself, the single offset 0
    t = rng.integers(0, 256, 4097).astype(np.uint8)
    s, e = random_disjoint(rng, 4097, 60, 40)
    for align in range(16):  # the text pointer at all 16 alignments, the output at all 16
        check_copy(ctx, t, s, e, (b"abc",), align=align, out_align=(5 * align + 3) % 16)
    for rl in (0, 1, 15, 16, 17, 4097, 65536):
        repl = rng.integers(0, 256, rl).astype(np.uint8).tobytes()
        check_copy(ctx, t, s[:7], e[:7], (repl,), out_align=rl % 16)
    d_text, d_s, d_e = dev(t), dev(s), dev(e)
    with pytest.raises(host.BmxError) as err:
        ctx.replace_device(d_text, d_s, d_e, bytes(65537))
    assert err.value.rc == host.ERR_ARG
    import torch

    empty = torch.empty(0, dtype=torch.uint8, device="cuda")  # n = 0
    out, n_out = ctx.replace_device(empty, dev(np.zeros(0, np.uint64)), dev(np.zeros(0, np.uint64)), b"q")
    assert n_out == 0 and out.numel() == 0


def test_copy_every_source_and_destination_alignment(ctx):
    rng = np.random.default_rng(9)
    t = rng.integers(0, 256, 2000).astype(np.uint8)
    for a in range(16):  # a span starting at source alignment a; the replacement lands at every destination alignment
        for rl in range(0, 16, 3):
            s = np.array([100 + a, 900 + a])
            check_copy(ctx, t, s, s + 4, (bytes(range(65, 65 + rl)),))
    # spans at the text's first and last byte, adjacent spans
    check_copy(ctx, t, np.array([0, 1, 2, 1990, 1995]), np.array([0, 1, 5, 1994, 1999]), (b"", b"#", b"long replacement string"))


def test_copy_piece_boundaries_at_tile_edges(ctx):
    rng = np.random.default_rng(10)
    n = 4 * COPY_TILE + 100
    t = rng.integers(0, 256, n).astype(np.uint8)
    for d in (-1, 0, 1):  # with an empty replacement of a 3-byte span at x, output byte x is a piece boundary
        s = np.array([k * COPY_TILE + d + 3 * (k - 1) for k in (1, 2, 3)])
        check_copy(ctx, t, s, s + 2, (b"", b"abc", b"abcdefgh"))
    # growing and shrinking outputs, dense input: every other byte a one-byte span
    s = np.arange(0, n, 2, dtype=np.uint64)
    check_copy(ctx, t, s, s, (b"", b"x", b"xyz"), align=3)
    s, e = random_disjoint(rng, n, 500, 30)
    check_copy(ctx, t, s, e, (b"", bytes(100)), align=7, out_align=9)
    check_copy(ctx, t, s, None, (b"-",), length=1)  # the one-list forms
    check_copy(ctx, t, None, s + 1, (b"-",), length=2)


def test_copy_limits_errors_and_capacity(ctx):
    import torch

    rng = np.random.default_rng(11)
    n = 5000
    t = rng.integers(0, 256, n).astype(np.uint8)
    base = (1 << 40) - n
    s, e = random_disjoint(rng, n, 80, 12)
    check_copy(ctx, t, s + np.uint64(base), e + np.uint64(base), (b"", b"R!"), base=base)
    d_text = dev(t)

    def rc_of(s, e, base=0):
        with pytest.raises(host.BmxError) as err:
            ctx.replace_device(d_text, dev(np.asarray(s).astype(np.uint64)), dev(np.asarray(e).astype(np.uint64)), b"x", base_offset=base)
        with pytest.raises(host.BmxError) as err2:
            ctx.extract_device(d_text, dev(np.asarray(s).astype(np.uint64)), dev(np.asarray(e).astype(np.uint64)), base_offset=base)
        return err.value.rc, err2.value.rc

    assert rc_of([10, 15], [16, 20]) == (host.ERR_ARG, host.ERR_ARG)  # overlapping
    assert rc_of([30, 10], [35, 12]) == (host.ERR_ARG, host.ERR_ARG)  # descending
    assert rc_of([10, 4990], [12, 5000]) == (host.ERR_ARG, host.ERR_ARG)  # past the view's end
    assert rc_of([10, 40], [12, 45], base=11) == (host.ERR_ARG, host.ERR_ARG)  # in front of the view
    assert rc_of([10, 40], [12, 39]) == (host.ERR_ARG, host.ERR_ARG)  # an end below its start
    with pytest.raises(host.BmxError) as err:  # the output overlaps the text
        ctx.replace_device(d_text[:4000], dev(s[:3]), dev(e[:3]), b"x", out=d_text[3990:])
    assert err.value.rc == host.ERR_ARG
    # capacity: one byte short stores the lowest bytes, 0 counts
    want = so.replace(t.tobytes(), s, e, b"[]")
    blob, off = so.extract(t.tobytes(), s, e)
    n_out = C.c_uint64(0)
    d_s, d_e, d_off = dev(s), dev(e), torch.empty(s.size + 1, dtype=torch.int64, device="cuda")
    p = lambda x: C.c_void_p(x.data_ptr())
    for cap in (len(want) - 1, 17, 1):
        out = torch.full((len(want) + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        rc = ctx._L.bmx_replace_device(ctx._h, p(d_text), n, 0, p(d_s), p(d_e), 0, s.size, b"[]", 2, p(out), cap, C.byref(n_out), None)
        assert rc == host.ERR_CAPACITY and n_out.value == len(want)
        g = out.cpu().numpy()
        assert g[:cap].tobytes() == want[:cap] and np.all(g[cap:] == 0xA5)
    assert ctx._L.bmx_replace_device(ctx._h, p(d_text), n, 0, p(d_s), p(d_e), 0, s.size, b"[]", 2, None, 0, C.byref(n_out), None) == host.OK
    assert n_out.value == len(want)
    out = torch.full((len(blob) + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    rc = ctx._L.bmx_extract_device(ctx._h, p(d_text), n, 0, p(d_s), p(d_e), 0, s.size, p(out), len(blob) - 1, p(d_off), C.byref(n_out), None)
    assert rc == host.ERR_CAPACITY and n_out.value == len(blob) and np.array_equal(u64(d_off), off)
    g = out.cpu().numpy()
    assert g[:len(blob) - 1].tobytes() == blob[:-1] and np.all(g[len(blob) - 1:] == 0xA5)
    assert ctx._L.bmx_extract_device(ctx._h, p(d_text), n, 0, p(d_s), p(d_e), 0, s.size, None, 0, p(d_off), C.byref(n_out), None) == host.OK
    assert n_out.value == len(blob)
    assert ctx.last_subst_ms() >= 0


def test_copy_past_4_gib(ctx):
    """2^32 + 4,097 bytes with spans that end at 2^32 - 1, begin at 2^32 and straddle it: positions do not wrap."""
    import torch

    n = (1 << 32) + 4097
    d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
    ctx.gen_text(d_text, 0, 0x5AB5, 0)
    lo = (1 << 32) - 5000
    tail = d_text[lo:].cpu().numpy()
    head = d_text[:4096].cpu().numpy()
    for s, e in (([100, (1 << 32) - 8], [107, (1 << 32) - 1]), ([100, 1 << 32], [107, (1 << 32) + 7]), ([100, (1 << 32) - 4], [107, (1 << 32) + 3])):
        s, e = np.array(s, np.uint64), np.array(e, np.uint64)
        out, n_out = ctx.replace_device(d_text, dev(s), dev(e), b"<4GiB>")
        assert n_out == n - 16 + 12
        want_head = so.replace(head.tobytes(), s[:1], e[:1], b"<4GiB>")
        assert out[:len(want_head)].cpu().numpy().tobytes() == want_head
        want_tail = so.replace(tail.tobytes(), s[1:] - np.uint64(lo), e[1:] - np.uint64(lo), b"<4GiB>")
        assert out[lo - 2:].cpu().numpy().tobytes() == want_tail
        blob, off = ctx.extract_device(d_text, dev(s), dev(e))
        assert u64(off).tolist() == [0, 8, 16]
        assert blob.cpu().numpy().tobytes() == head[100:108].tobytes() + tail[int(s[1]) - lo:int(e[1]) - lo + 1].tobytes()
        del out
    del d_text
    torch.cuda.empty_cache()


# ---- end to end ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def the_log():
    text, _ = ro.log_text(np.random.default_rng(2024), 20000, 90)
    t = np.frombuffer(text, np.uint8).copy()
    rng = np.random.default_rng(7)
    for p in rng.integers(0, t.size - 20, 3000):  # digits and overlapping occurrences
        t[p:p + 10] = np.frombuffer(b"ERROR: 123", np.uint8)
    for p in rng.integers(0, t.size - 20, 2000):
        t[p:p + 4] = np.frombuffer(b"aaaa", np.uint8)
    return t.tobytes()


def host_lists(ctx, text, kind, expr, k, longest=False):
    """(starts, ends) of every match from the HOST search of the kind and its starts pass."""
    if kind == "exact":
        s = ctx.search(text, expr)
        return s, s + np.uint64(len(expr) - 1)
    if kind == "classes":
        s = ctx.search_classes(text, expr)
        return s, s + np.uint64(host.compile_classes(expr).shape[0] - 1)
    if kind == "hamming":
        s = ctx.search_hamming(text, expr, k)[0]
        return s, s + np.uint64(len(expr) - 1)
    if kind == "gaps":
        return ctx.search_gaps_spans(text, expr, longest=longest)
    if kind == "regex":
        return ctx.search_regex_spans(text, expr, longest=longest)
    if kind == "regex_star":
        return ctx.search_regex_star_spans(text, expr, longest=longest)
    s, e, _ = ctx.search_approx_spans(text, expr, k, best=False)
    return s, e


KINDS = [("exact", b"aa", 0), ("classes", "ERR[A-Z]R: [0-9]", 0), ("hamming", b"ERROR: 123", 1), ("gaps", "ERROR.{0,4}[0-9]", 0),
         ("regex", "ERROR: [0-9]{3}", 0), ("regex_star", "[0-9]+", 0), ("approx", b"ERROR: 123", 1)]


@pytest.mark.parametrize("kind,expr,k", KINDS, ids=[k[0] for k in KINDS])
def test_sub_and_findall_for_every_kind(ctx, kind, expr, k):
    text = the_log()
    d_text = dev(np.frombuffer(text, np.uint8))
    s, e = host_lists(ctx, text, kind, expr, k)
    ws, we, _ = so.select(so.spans_of(s, e))
    assert ws.size > 100
    out, n_out = ctx.sub_device(d_text, expr, b"<>", kind=kind, k=k)
    assert out.cpu().numpy().tobytes() == so.replace(text, ws, we, b"<>")
    blob, off = ctx.findall_device(d_text, expr, kind=kind, k=k)
    want_blob, want_off = so.extract(text, ws, we)
    assert blob.cpu().numpy().tobytes() == want_blob and np.array_equal(u64(off), want_off)


def test_sub_and_findall_against_re(ctx):
    text = the_log()
    d_text = dev(np.frombuffer(text, np.uint8))
    for kind, expr, rx in (("regex", "ERROR: [0-9]{3}", rb"ERROR: [0-9]{3}"), ("classes", "[a-c][a-c]", rb"[a-c][a-c]"),
                           ("exact", b"aa", rb"aa")):
        out, _ = ctx.sub_device(d_text, expr, b"--", kind=kind)
        assert out.cpu().numpy().tobytes() == re.sub(rx, b"--", text)
        blob, off = ctx.findall_device(d_text, expr, kind=kind)
        blob, off = blob.cpu().numpy().tobytes(), u64(off)
        assert [blob[off[i]:off[i + 1]] for i in range(off.size - 1)] == re.findall(rx, text)
    out, _ = ctx.sub_device(d_text, "[0-9]+", b"N", kind="regex_star", merge=True)
    assert out.cpu().numpy().tobytes() == re.sub(rb"[0-9]+", b"N", text)
    assert host.sub(text[:5000], "[0-9]+", b"N", kind="regex_star", merge=True) == re.sub(rb"[0-9]+", b"N", text[:5000])
    assert host.findall(text[:5000], b"aa", kind="exact") == re.findall(rb"aa", text[:5000])


def test_sub_with_rows_leaves_matches_across_a_line_break(ctx):
    text = the_log()
    d_text = dev(np.frombuffer(text, np.uint8))
    rows = ctx.rows_split_device(d_text)
    # a line break can only be a match's first byte: such a match runs across two rows (a row ends with its delimiter)
    expr = "[^a-z][^a-z\\x0a]"
    out, _ = ctx.sub_device(d_text, expr, b"", kind="classes", rows=rows)
    got = out.cpu().numpy().tobytes()
    assert got.count(b"\n") == text.count(b"\n")
    s, e = host_lists(ctx, text, "classes", expr, 0)
    off = ro.split(np.frombuffer(text, np.uint8), 10)
    ws, we, _ = so.select(so.spans_of(s, e, 0, ro.row_of(off, s, e)))
    assert got == so.replace(text, ws, we, b"")
    assert ctx.sub_device(d_text, expr, b"", kind="classes")[0].cpu().numpy().tobytes().count(b"\n") < text.count(b"\n")


# ---- plumbing --------------------------------------------------------------------------------------------------------------

def test_host_buffer_forms(ctx):
    rng = np.random.default_rng(12)
    s, e = ascending(rng, 3000)
    rows = none_where(rng.random(3000) < 0.1)
    for merge in (False, True):
        want = (so.merge if merge else so.select)(so.spans_of(s, e, 0, rows))
        got = host.select_spans(s, e, rows=rows, merge=merge, index=True)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
    t = rng.integers(0, 256, 70001).astype(np.uint8)
    text = t.tobytes()
    s, e = random_disjoint(rng, t.size, 900, 20)
    want = so.replace(text, s, e, b"=+=")
    out, n_out = np.zeros(len(want) + 8, np.uint8), C.c_uint64(0)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    L = host.lib()
    assert L.bmx_replace(ctx._h, ptr(t), t.size, ptr(s), ptr(e), 0, s.size, b"=+=", 3, ptr(out), out.size, C.byref(n_out)) == host.OK
    assert n_out.value == len(want) and out[:len(want)].tobytes() == want
    assert L.bmx_replace(ctx._h, ptr(t), t.size, ptr(s), ptr(e), 0, s.size, b"=+=", 3, ptr(out), 100, C.byref(n_out)) == host.ERR_CAPACITY
    assert n_out.value == len(want)
    blob, off = so.extract(text, s, e)
    out, got_off = np.zeros(len(blob), np.uint8), np.zeros(s.size + 1, np.uint64)
    assert L.bmx_extract(ctx._h, ptr(t), t.size, ptr(s), ptr(e), 0, s.size, ptr(out), out.size, ptr(got_off), C.byref(n_out)) == host.OK
    assert n_out.value == len(blob) and out.tobytes() == blob and np.array_equal(got_off, off)


@functools.lru_cache(maxsize=None)
def delay_scratch():
    import torch

    return torch.zeros(2 * sc.DELAY_BYTES, dtype=torch.uint8, device="cuda")


def behind_a_pending_copy(buf, real, what):
    """On a fresh non-blocking stream: a long delay, then the copy of `real` over `buf` (which holds the decoy); returns
    the stream with the copy still outstanding (asserted)."""
    import torch

    s = torch.cuda.Stream()
    scratch = delay_scratch()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for i in range(sc.DELAY_COPIES):
            a, b = (0, sc.DELAY_BYTES) if i & 1 else (sc.DELAY_BYTES, 0)
            scratch[a:a + sc.DELAY_BYTES].copy_(scratch[b:b + sc.DELAY_BYTES], non_blocking=True)
        buf.copy_(real, non_blocking=True)
        pending = torch.cuda.Event()
        pending.record(s)
    assert not pending.query(), f"{what}: the producer had finished before the call"
    return s


def test_the_three_entries_on_a_callers_stream_behind_a_pending_copy(ctx):
    rng = np.random.default_rng(0x57A)
    s, e = ascending(rng, 70000)
    s2, e2 = ascending(rng, 70000)
    want = so.select(so.spans_of(s, e))
    assert not np.array_equal(want[0], so.select(so.spans_of(s, e2))[0][:want[0].size])
    d_s, d_e, d_real = dev(s), dev(e2), dev(e)
    st = behind_a_pending_copy(d_e, d_real, "select_spans_device")
    got = ctx.select_spans_device(d_s, d_e, stream=st)
    assert np.array_equal(u64(got[0]), want[0]) and np.array_equal(u64(got[1]), want[1])

    real = rng.integers(0, 256, 300001).astype(np.uint8)
    decoy = rng.integers(0, 256, 300001).astype(np.uint8)
    ws, we = random_disjoint(rng, real.size, 4000, 25)
    d_ws, d_we = dev(ws), dev(we)
    buf, d_real = dev(decoy), dev(real)
    st = behind_a_pending_copy(buf, d_real, "replace_device")
    out, _ = ctx.replace_device(buf, d_ws, d_we, b"stream", stream=st)
    assert out.cpu().numpy().tobytes() == so.replace(real.tobytes(), ws, we, b"stream")
    buf.copy_(dev(decoy))
    st = behind_a_pending_copy(buf, d_real, "extract_device")
    blob, off = ctx.extract_device(buf, d_ws, d_we, stream=st)
    want_blob, want_off = so.extract(real.tobytes(), ws, we)
    assert blob.cpu().numpy().tobytes() == want_blob and np.array_equal(u64(off), want_off)


def cli(path, args):
    exe = os.path.join(ROOT, host.__name__.split(".")[0], "bin", "bmx_cli")
    out = subprocess.run([exe, "--text", str(path)] + args, capture_output=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return out.stdout, out.stderr.decode()


def test_cli_replace_and_only_matching(tmp_path):
    text = the_log()[:60000]
    path, pat, dst = tmp_path / "log.txt", tmp_path / "pat.txt", tmp_path / "new.txt"
    path.write_bytes(text)
    pat.write_bytes(b"aa")
    out, err = cli(path, ["--regex", "ERROR: [0-9]{3}", "--replace", "<E>"])
    assert out == re.sub(rb"ERROR: [0-9]{3}", b"<E>", text) and err.splitlines()[-1].startswith("replaced ")
    out, err = cli(path, ["--pattern", str(pat), "--replace", "", "--out", str(dst)])
    assert out == b"" and dst.read_bytes() == text.replace(b"aa", b"")
    found = re.findall(rb"aa", text)
    out, err = cli(path, ["--pattern", str(pat), "--only-matching", "--max-print", "1000000"])
    assert out.split(b"\n")[:-1] == found and err.splitlines()[-1].startswith(f"matches: {len(found)} of ")
    out, err = cli(path, ["--pattern", str(pat), "--only-matching", "--max-print", "3"])
    assert out == b"aa\n" * 3 and err.splitlines()[-1].startswith(f"matches: {len(found)} of ")
    out, err = cli(path, ["--regex-star", "[0-9]+", "--merge", "--replace", "N"])
    assert out == re.sub(rb"[0-9]+", b"N", text)
    out, err = cli(path, ["--regex-star", "[0-9]+", "--merge", "--only-matching", "--max-print", "1000000"])
    assert out.split(b"\n")[:-1] == re.findall(rb"[0-9]+", text)
    # --lines: a match that begins with a line break crosses two lines and stays
    expr = "[^a-z][^a-z\\x0a]"
    out, err = cli(path, ["--classes", expr, "--replace", "", "--lines"])
    assert out.count(b"\n") == text.count(b"\n") and len(out) < len(text)
    out, err = cli(path, ["--classes", expr, "--replace", ""])
    assert out.count(b"\n") < text.count(b"\n")
