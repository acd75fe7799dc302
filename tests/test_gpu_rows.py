"""GPU suite of the row-wise results (bmx_rows_split_device, bmx_rows_of_device, bmx_rows_matching_device, Context.grep_device,
bmx_cli --lines) against tests/rows_oracle.py: the split at the edges of its geometry (the tile, a wave's piece and a
round of 1 KiB, the tile from bmx_exp_last_launch), every alignment, every capacity rule and past 4 GiB; the row of a match at
every kind of boundary; the matching rows with NONE entries anywhere; grep for every kind of search against the oracle fed
with the host search's own lists, and for the two regular-expression searches against Python's ``re`` per line; the three
entries on a caller's non-blocking stream behind a pending copy."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import rows_oracle as ro
import stream_cases as sc
from conftest import ROOT, golden_file_bytes
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

pytestmark = pytest.mark.gpu

NONE = int(ro.NONE)
ROUND = 1024  # a wave of the split reads its piece of the tile in rounds of 1 KiB (include/bmx_exp.h)


@pytest.fixture(scope="module")
def exp(built):
    """A context of libbmx_exp.so for the module: bmx_exp_last_launch knows the split's geometry."""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = host.Context(0, library=host.exp_lib())
    yield c
    c.close()


@pytest.fixture(scope="module")
def TILE(exp):
    """Bytes of a tile of the split, from the kernel's own constant (the same object file is in both libraries)."""
    tile = 1 << exp.last_launch("rows")[0]
    assert tile % (8 * ROUND) == 0
    return tile


def dev(a, dtype=None):
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    t = torch.from_numpy(a.copy()).cuda()
    return t if dtype is None else t.to(dtype)


def u64(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


def text_of(rng, n, d=10, p=0.05):
    t = rng.integers(0, 256, n).astype(np.uint8)
    t[t == d] = (d + 1) & 0xFF
    t[rng.random(n) < p] = d
    return t


def check_split(ctx, t, d=10, base=0, align=0):
    """Splits the numpy text on the device at the given alignment within a 16-byte line and compares with the oracle."""
    import torch

    buf = torch.empty(t.size + 32, dtype=torch.uint8, device="cuda")
    skew = (align - buf.data_ptr()) % 16
    d_text = buf[skew:skew + t.size]
    d_text.copy_(torch.from_numpy(t))
    assert t.size == 0 or d_text.data_ptr() % 16 == align
    rows = ctx.rows_split_device(d_text, d, base_offset=base)
    want = ro.split(t, d, base)
    assert rows.count == want.size - 1
    assert np.array_equal(u64(rows.offsets), want), (t.size, d, base, align)
    assert rows.longest == (int(np.diff(want).max()) if want.size > 1 else 0)
    return rows


# ---- split -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 4097])
@pytest.mark.parametrize("d", [0x00, 0x0A, 0xFF])
def test_split_small_sizes_and_delimiters(ctx, n, d):
    rng = np.random.default_rng(n * 256 + d)
    check_split(ctx, text_of(rng, n, d, 0.2), d)
    check_split(ctx, rng.integers(0, 256, n).astype(np.uint8), d)  # plain random bytes


def test_split_without_and_with_only_delimiters(ctx):
    n = 4097
    check_split(ctx, np.full(n, ord("a"), np.uint8))  # none: one unterminated row
    rows = check_split(ctx, np.full(n, 10, np.uint8))  # only: n rows of one byte
    assert rows.count == n and rows.longest == 1
    t = np.full(n, ord("a"), np.uint8)
    t[0] = t[n - 1] = 10
    rows = check_split(ctx, t)
    assert rows.count == 2 and rows.longest == n - 1


def test_split_one_delimiter_around_every_boundary(exp, TILE):
    """Three tiles (the last one short); one delimiter at boundary - 1, boundary and boundary + 1 of every round of 1 KiB,
    which covers every piece of a wave and every tile."""
    import torch

    ctx = exp
    n = 3 * TILE - 5
    d_text = torch.full((n,), ord("a"), dtype=torch.uint8, device="cuda")
    assert d_text.data_ptr() % 16 == 0
    out = torch.empty(8, dtype=torch.int64, device="cuda")
    got, want = [], []
    for b in range(0, n + ROUND, ROUND):
        for pos in (b - 1, b, b + 1):
            if not 0 <= pos < n:
                continue
            d_text[pos] = 10
            rows = ctx.rows_split_device(d_text, out=out)
            got.append(rows.offsets.clone())
            want.append([0, pos + 1] + ([n] if pos + 1 < n else []))
            d_text[pos] = ord("a")
    assert len(got) > 3 * (TILE // ROUND) * 3 - 6
    assert ctx.last_launch("rows")[2] == 3  # three tiles ran
    assert [g.cpu().tolist() for g in got] == want


@pytest.mark.parametrize("align", range(16))
def test_split_at_every_alignment(ctx, align):
    rng = np.random.default_rng(align)
    t = text_of(rng, 4097 + align, 10, 0.1)
    t[0] = 10  # the first byte of an unaligned text is a row of its own
    check_split(ctx, t, align=align)
    check_split(ctx, text_of(rng, 5, 10, 0.3), align=align)  # a text inside one line, or across two


def test_split_base_offset_at_the_top_of_the_range(ctx):
    rng = np.random.default_rng(40)
    t = text_of(rng, 70001, 10, 0.02)
    check_split(ctx, t, base=(1 << 40) - t.size)


def split_raw(ctx, d_text, n, d_off, capacity, want_longest=True):
    rows, longest = C.c_uint64(0), C.c_uint64(0)
    rc = ctx._L.bmx_rows_split_device(ctx._h, C.c_void_p(d_text.data_ptr()), n, 0, 10, C.c_void_p(d_off.data_ptr()) if d_off is not None else None,
                                      capacity, C.byref(rows), C.byref(longest) if want_longest else None, None)
    return rc, rows.value, longest.value


def test_split_capacity_rules(ctx, TILE):
    import torch

    rng = np.random.default_rng(7)
    t = text_of(rng, 3 * TILE + 17, 10, 0.01)
    want = ro.split(t, 10)
    rows = want.size - 1
    d_text = dev(t)
    out = torch.full((rows + 8,), -1, dtype=torch.int64, device="cuda")
    rc, got, longest = split_raw(ctx, d_text, t.size, out, rows)  # one short
    assert (rc, got, longest) == (host.ERR_CAPACITY, rows, int(np.diff(want).max()))
    assert np.array_equal(u64(out[:rows]), want[:rows]) and bool((out[rows:] == -1).all())
    out.fill_(-1)
    rc, got, longest = split_raw(ctx, d_text, t.size, out, 1)
    assert (rc, got, out[0].item()) == (host.ERR_CAPACITY, rows, 0) and bool((out[1:] == -1).all())
    rc, got, longest = split_raw(ctx, d_text, t.size, None, 0)  # counts only
    assert (rc, got, longest) == (host.OK, rows, int(np.diff(want).max()))
    rc, got, _ = split_raw(ctx, d_text, t.size, None, 0, want_longest=False)
    assert (rc, got) == (host.OK, rows)
    out.fill_(-1)
    rc, got, longest = split_raw(ctx, d_text, t.size, out, rows + 1)  # exact
    assert (rc, got) == (host.OK, rows) and np.array_equal(u64(out[:rows + 1]), want) and bool((out[rows + 1:] == -1).all())
    assert ctx.last_rows_ms() > 0


@pytest.mark.parametrize("where", ["first", "last", "tail"])
def test_split_longest_row(ctx, TILE, where):
    lens = [50, 60, 70, 40]
    if where == "first":
        lens[0] = 3 * TILE
    else:
        lens[-1] = 3 * TILE
    text = b"".join(b"x" * (ln - 1) + b"\n" for ln in lens)
    if where == "tail":
        text = text[:-1]
    rows = check_split(ctx, np.frombuffer(text, np.uint8))
    assert rows.count == 4 and rows.longest == 3 * TILE - (where == "tail")


def test_split_past_4_gib(ctx):
    import torch

    n = (1 << 32) + 4097
    d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
    ctx.gen_text(d_text, 0, 0x2095, 0)  # printable-95: no newline
    rng = np.random.default_rng(32)
    pos = np.unique(np.concatenate([rng.integers(0, n, 1000), [(1 << 32) - 1, 1 << 32, (1 << 32) + 1]])).astype(np.int64)
    d_text[torch.from_numpy(pos).cuda()] = 10
    rows = ctx.rows_split_device(d_text)
    want = np.concatenate([[0], pos + 1, [n]]).astype(np.uint64)
    got = u64(rows.offsets)
    longest = rows.longest
    del d_text, rows
    torch.cuda.empty_cache()
    assert np.array_equal(got, want) and longest == int(np.diff(want).max())


# ---- the row of every match ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def log():
    """A 20,000-line log with planted tokens, once for the module: (text bytes, offsets, lines)."""
    text, plants = ro.log_text(np.random.default_rng(20000), 20000, 100)
    assert len(plants) > 2000
    return text, ro.split(text, 10), text.split(b"\n")[:-1]


def random_spans(rng, off, count, max_len=40):
    lo, hi = int(off[0]), int(off[-1])
    s = rng.integers(max(lo - 50, 0), hi + 50, count).astype(np.uint64)
    e = s + rng.integers(0, max_len, count).astype(np.uint64)
    order = np.argsort(e, kind="stable")
    return s[order], e[order]


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 257])
def test_rows_of_counts(ctx, log, count):
    _, off, _ = log
    rows = ctx.rows(dev(off))
    s, e = random_spans(np.random.default_rng(count), off, count)
    got = rows.of(starts=dev(s), ends=dev(e))
    assert got.numel() == count and np.array_equal(u64(got), ro.row_of(off, s, e))


def test_rows_of_boundaries_and_empty_rows(ctx):
    off = np.array([100, 110, 110, 110, 125, 125, 140], np.uint64)  # rows 1, 2 and 4 are empty
    rows = ctx.rows(dev(off))
    assert rows.count == 6 and rows.longest == 15
    cases = [(100, 100, 0), (109, 109, 0), (100, 109, 0), (99, 100, NONE), (109, 110, NONE), (110, 110, 3), (110, 124, 3),
             (124, 125, NONE), (125, 139, 5), (139, 139, 5), (139, 140, NONE), (140, 141, NONE), (150, 160, NONE),
             (0, 5, NONE), (99, 99, NONE), (NONE, 120, NONE), (NONE, NONE, NONE), (120, 119, NONE), (100, 139, NONE)]
    s = np.array([c[0] for c in cases], np.uint64)
    e = np.array([c[1] for c in cases], np.uint64)
    want = np.array([c[2] for c in cases], np.uint64)
    assert np.array_equal(ro.row_of(off, s, e), want)
    got = u64(rows.of(starts=dev(s), ends=dev(e)))
    assert np.array_equal(got, want)
    assert not set(got.tolist()) & {1, 2, 4}  # the empty rows get nothing
    one = ctx.rows(dev(np.array([100, 140], np.uint64)))  # rows = 1
    assert u64(one.of(starts=dev(s), ends=dev(e))).tolist() == [0 if 100 <= a <= b < 140 else NONE for a, b, _ in cases]
    # ends with a length larger than the end: no start, no row
    ends = np.array([3, 5, 104, 109, 111], np.uint64)
    assert u64(rows.of(ends=dev(ends), length=5)).tolist() == [NONE, NONE, 0, 0, NONE]
    assert u64(ctx.rows(dev(np.array([0, 4, 8], np.uint64))).of(ends=dev(ends[:2]), length=5)).tolist() == [NONE, NONE]


def test_rows_of_many_rows_shuffled_and_three_forms(ctx):
    rng = np.random.default_rng(20)
    rows_n = (1 << 20) + 1
    off = np.concatenate([[7], 7 + np.cumsum(rng.integers(0, 60, rows_n))]).astype(np.uint64)
    rows = ctx.rows(dev(off))
    s, e = random_spans(rng, off, 100_000)
    want = ro.row_of(off, s, e)
    assert (want != ro.NONE).sum() > 10_000 and (want == ro.NONE).sum() > 10_000
    assert np.array_equal(u64(rows.of(starts=dev(s), ends=dev(e))), want)
    perm = rng.permutation(s.size)
    assert np.array_equal(u64(rows.of(starts=dev(s[perm]), ends=dev(e[perm]))), want[perm])
    m = 9
    e9 = s + np.uint64(m - 1)
    want9 = ro.row_of(off, s, e9)
    for kw in (dict(starts=dev(s), ends=dev(e9)), dict(starts=dev(s), length=m), dict(ends=dev(e9), length=m)):
        assert np.array_equal(u64(rows.of(**kw)), want9), list(kw)


# ---- the matching rows ---------------------------------------------------------------------------------------------------

def check_matching(ctx, ids, rows_n):
    rows = ctx.rows(dev(np.arange(rows_n + 1, dtype=np.uint64)))
    ids = np.asarray(ids, np.uint64)
    hit, cnt = ro.matching(ids, rows_n)
    got, got_cnt = rows.matching(dev(ids) if ids.size else dev(np.zeros(1, np.uint64))[:0])
    assert np.array_equal(u64(got), hit) and np.array_equal(u64(got_cnt), cnt)
    assert int(cnt.sum()) == int((ids != ro.NONE).sum())
    inv, none = rows.matching(dev(ids) if ids.size else dev(np.zeros(1, np.uint64))[:0], invert=True)
    assert none is None and np.array_equal(u64(inv), ro.matching(ids, rows_n, invert=True)[0])
    only, none = rows.matching(dev(ids) if ids.size else dev(np.zeros(1, np.uint64))[:0], counts=False)
    assert none is None and np.array_equal(u64(only), hit)


@pytest.mark.parametrize("name,ids,rows_n", [
    ("none at the front", [NONE, NONE, 2, 2, 5], 7),
    ("none at the back", [0, 3, 3, NONE, NONE], 7),
    ("none interleaved", [1, NONE, 1, NONE, NONE, 1, 4, NONE, 4, 6], 7),
    ("all none", [NONE] * 70, 7),
    ("only row 0", [0] * 130, 7),
    ("only the last row", [6, 6, 6], 7),
    ("every row", list(range(300)), 300),
    ("empty list", [], 5),
    ("no rows", [], 0),
    ("no rows, none only", [NONE, NONE], 0),
])
def test_matching_by_hand(ctx, name, ids, rows_n):
    check_matching(ctx, ids, rows_n)


def test_matching_random_lists(ctx):
    rng = np.random.default_rng(11)
    for count, rows_n in ((1000, 50), (70_000, 100_000), (70_000, 900)):
        ids = np.sort(rng.integers(0, rows_n, count)).astype(np.uint64)
        ids[rng.random(count) < 0.3] = ro.NONE
        check_matching(ctx, ids, rows_n)


def matching_raw(ctx, ids, rows_n, flags, capacity, counts=True):
    import torch

    d_ids = dev(np.asarray(ids, np.uint64))
    out = torch.full((capacity + 4,), -1, dtype=torch.int64, device="cuda")
    cnt = torch.full((capacity + 4,), -1, dtype=torch.int64, device="cuda") if counts else None
    total = C.c_uint64(0)
    rc = ctx._L.bmx_rows_matching_device(ctx._h, C.c_void_p(d_ids.data_ptr()), len(ids), rows_n, flags, C.c_void_p(out.data_ptr()),
                                         C.c_void_p(cnt.data_ptr()) if counts else None, capacity, C.byref(total), None)
    return rc, total.value, out.cpu().tolist(), cnt.cpu().tolist() if counts else None


def test_matching_capacity_and_bad_lists(ctx):
    ids = [0, 0, NONE, 2, 5, 5, 5, 6]
    rc, total, out, cnt = matching_raw(ctx, ids, 8, 0, 3)  # one short
    assert (rc, total) == (host.ERR_CAPACITY, 4) and out == [0, 2, 5, -1, -1, -1, -1] and cnt == [2, 1, 3, -1, -1, -1, -1]
    rc, total, out, _ = matching_raw(ctx, ids, 8, host.ROWS_INVERT, 3, counts=False)
    assert (rc, total) == (host.ERR_CAPACITY, 4) and out == [1, 3, 4, -1, -1, -1, -1]
    rc, total, out, cnt = matching_raw(ctx, ids, 8, 0, 4)
    assert (rc, total) == (host.OK, 4) and out[:4] == [0, 2, 5, 6] and cnt[:4] == [2, 1, 3, 1]
    total = C.c_uint64(0)
    d_ids = dev(np.asarray(ids, np.uint64))
    assert ctx._L.bmx_rows_matching_device(ctx._h, C.c_void_p(d_ids.data_ptr()), len(ids), 8, 0, None, None, 0, C.byref(total),
                                           None) == host.ERR_CAPACITY and total.value == 4  # counts only
    for bad in ([0, 3, NONE, 2, 5], [0, 1, 8], [9]):  # a list that decreases; an id equal to rows; one past it
        for flags in (0, host.ROWS_INVERT):
            rc, _, _, _ = matching_raw(ctx, bad, 8, flags, 8, counts=False)
            assert rc == host.ERR_ARG, (bad, flags)
            assert b"d_row" in ctx._L.bmx_last_error()


def test_empty_list_with_counts_through_the_c_entry(ctx):
    rc, total, out, cnt = matching_raw(ctx, [], 5, 0, 4)
    assert (rc, total) == (host.OK, 0) and out == [-1] * 8 and cnt == [-1] * 8


def test_host_buffer_forms(ctx):
    """bmx_rows_split, bmx_rows_of and bmx_rows_matching on host arrays (what the driver's --lines calls)."""
    rng = np.random.default_rng(5)
    t = text_of(rng, 70001, 10, 0.02)
    want = ro.split(t, 10)
    off, longest = host.rows_split(t)
    assert np.array_equal(off, want) and longest == int(np.diff(want).max())
    s, e = random_spans(rng, want, 3000, 30)
    ids = ro.row_of(want, s, e)
    row = np.full(s.size, 7, np.uint64)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    L = host.lib()
    assert L.bmx_rows_of(ctx._h, ptr(off), off.size - 1, ptr(s), ptr(e), 0, s.size, ptr(row)) == host.OK
    assert np.array_equal(row, ids)
    hit, cnt = ro.matching(ids, off.size - 1)
    out, counts, n_out = np.zeros(off.size, np.uint64), np.zeros(off.size, np.uint64), C.c_uint64(0)
    assert L.bmx_rows_matching(ctx._h, ptr(row), row.size, off.size - 1, 0, ptr(out), ptr(counts), out.size, C.byref(n_out)) == host.OK
    assert n_out.value == hit.size and np.array_equal(out[:hit.size], hit) and np.array_equal(counts[:hit.size], cnt)
    assert L.bmx_rows_matching(ctx._h, ptr(row), row.size, off.size - 1, host.ROWS_INVERT, ptr(out), None, out.size,
                               C.byref(n_out)) == host.OK
    inv = ro.matching(ids, off.size - 1, invert=True)[0]
    assert n_out.value == inv.size and np.array_equal(out[:inv.size], inv)
    assert L.bmx_rows_matching(ctx._h, ptr(row), row.size, off.size - 1, 0, ptr(out), ptr(counts), hit.size - 1,
                               C.byref(n_out)) == host.ERR_CAPACITY and n_out.value == hit.size


# ---- end to end ----------------------------------------------------------------------------------------------------------

STAR = "ERROR[^\n]*timeout"  # (a real newline inside the set: the grammar's own escape for it is \x0a)
KINDS = {
    "exact": dict(expr="ERROR: 123"),
    "classes": dict(expr="ERR[A-Z]R: [0-9]"),
    "hamming": dict(expr="ERROR: 123", k=2),
    "gaps": dict(expr="ERROR.{0,4}[0-9]"),
    "regex": dict(expr="(ERROR|FATAL): [0-9]{2,4}"),
    "regex_star": dict(expr=STAR),
    "approx": dict(expr="ERROR: 123", k=1),
}


def host_lists(ctx, kind, text, expr, k, window):
    """(starts, ends) of the host search of the same kind, the starts by its default rule."""
    if kind == "exact":
        s = ctx.search(text, expr)
        return s, s + np.uint64(len(expr) - 1)
    if kind == "classes":
        s = ctx.search_classes(text, expr)
        return s, s + np.uint64(host.compile_classes(expr).shape[0] - 1)
    if kind == "hamming":
        s, _ = ctx.search_hamming(text, expr, k)
        return s, s + np.uint64(len(expr) - 1)
    if kind == "gaps":
        return ctx.search_gaps_spans(text, expr)
    if kind == "regex":
        return ctx.search_regex_spans(text, expr)
    if kind == "regex_star":
        return ctx.search_regex_star_spans(text, expr, window=window)
    s, e, _ = ctx.search_approx_spans(text, expr, k, best=False)
    return s, e


@pytest.mark.parametrize("kind", list(KINDS))
def test_grep_every_kind_against_the_oracle(ctx, log, kind):
    text, off, lines = log
    expr, k = KINDS[kind]["expr"], KINDS[kind].get("k", 0)
    d_text = dev(np.frombuffer(text, np.uint8))
    got, cnt = ctx.grep_device(d_text, expr, kind=kind, k=k)
    s, e = host_lists(ctx, kind, text, expr, k, int(np.diff(off).max()))
    assert e.size > 100
    ids = ro.row_of(off, s, e)
    hit, want_cnt = ro.matching(ids, off.size - 1)
    assert hit.size > 100
    assert np.array_equal(u64(got), hit) and np.array_equal(u64(cnt), want_cnt)
    inv, none = ctx.grep_device(d_text, expr, kind=kind, k=k, invert=True)
    assert none is None and np.array_equal(u64(inv), ro.matching(ids, off.size - 1, invert=True)[0])
    if kind in ("regex", "regex_star"):  # the independent reference: re per line
        pat = re.compile(expr.encode())
        assert hit.tolist() == [i for i, ln in enumerate(lines) if pat.search(ln)]
    if kind == "exact":
        assert hit.tolist() == [i for i, ln in enumerate(lines) if expr.encode() in ln]
        assert want_cnt.tolist() == [ln.count(expr.encode()) for ln in lines if expr.encode() in ln]


def test_grep_drops_a_match_that_straddles_a_line_break(ctx):
    text = b"ab\ncd\nab.cd\nab"  # no trailing newline: four rows
    d_text = dev(np.frombuffer(text, np.uint8))
    rows, cnt = ctx.grep_device(d_text, "b.c", kind="regex")
    assert (rows.tolist(), cnt.tolist()) == ([2], [1])  # the end at "b\nc" belongs to no line
    assert ctx.search_regex(text, "b.c").tolist() == [3, 9]
    assert ctx.grep_device(d_text, "b.c", kind="regex", invert=True)[0].tolist() == [0, 1, 3]
    rows, cnt = ctx.grep_device(d_text, "ab", kind="exact")
    assert (rows.tolist(), cnt.tolist()) == ([0, 2, 3], [1, 1, 1])  # the unterminated tail is a row
    rows, cnt = ctx.grep_device(d_text, "b.", kind="regex")  # the newline as a match's last byte stays in its row
    assert (rows.tolist(), cnt.tolist()) == ([0, 2], [1, 1])
    r, c = host.grep(text, "[a-d]", kind="classes")
    assert (r.tolist(), c.tolist()) == ([0, 1, 2, 3], [2, 2, 4, 2])
    off, longest = host.rows_split(text)
    assert off.tolist() == [0, 3, 6, 12, 14] and longest == 6


# ---- streams ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def delay_scratch():
    import torch

    return torch.zeros(2 * sc.DELAY_BYTES, dtype=torch.uint8, device="cuda")


def behind_a_pending_copy(buf, real, what):
    """On a fresh non-blocking stream: a long delay, then the copy of `real` over `buf` (which holds the decoy); returns
    the stream with the copy still outstanding (asserted).  The caller keeps `real` alive until the stream is done: torch
    hands a freed block to the next allocation at once."""
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


def test_the_three_entries_on_a_callers_stream_behind_a_pending_copy(ctx, TILE):
    import torch

    rng = np.random.default_rng(0x57A)
    n = 3 * TILE + 9
    real, decoy = text_of(rng, n, 10, 0.01), text_of(rng, n, 10, 0.01)  # the decoy: the newlines elsewhere
    want = ro.split(real, 10)
    assert not np.array_equal(want, ro.split(decoy, 10))
    buf, d_real = dev(decoy), dev(real)
    s = behind_a_pending_copy(buf, d_real, "rows_split_device")
    rows = ctx.rows_split_device(buf, stream=s)
    assert np.array_equal(u64(rows.offsets), want) and rows.longest == int(np.diff(want).max())

    st, en = random_spans(rng, want, 5000, 30)
    st2, en2 = random_spans(rng, want, 5000, 30)
    ids, ids2 = ro.row_of(want, st, en), ro.row_of(want, st, en2)
    assert not np.array_equal(ids, ids2)
    d_st, d_en, d_real = dev(st), dev(en2), dev(en)
    s = behind_a_pending_copy(d_en, d_real, "Rows.of")
    got = rows.of(starts=d_st, ends=d_en, stream=s)
    assert np.array_equal(u64(got), ids)

    ids2 = ro.row_of(want, st2, en2)
    hit, want_cnt = ro.matching(ids, rows.count)
    assert not np.array_equal(hit, ro.matching(ids2, rows.count)[0])
    d_ids, d_real = dev(ids2), dev(ids)
    s = behind_a_pending_copy(d_ids, d_real, "Rows.matching")
    got, cnt = rows.matching(d_ids, stream=s)
    assert np.array_equal(u64(got), hit) and np.array_equal(u64(cnt), want_cnt)
    d_ids.copy_(dev(ids2))
    s = behind_a_pending_copy(d_ids, d_real, "Rows.matching inverted")
    got, _ = rows.matching(d_ids, invert=True, stream=s)
    assert np.array_equal(u64(got), ro.matching(ids, rows.count, invert=True)[0])
    torch.cuda.synchronize()


# ---- the driver ------------------------------------------------------------------------------------------------------------

def cli_lines(path, args):
    cli = os.path.join(ROOT, host.__name__.split(".")[0], "bin", "bmx_cli")
    out = subprocess.run([cli, "--text", str(path), "--lines", "--max-print", "1000000"] + args, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    body = [ln for ln in out.stdout.splitlines() if ln and ln[0].isdigit()]
    assert out.stdout.splitlines()[-1].startswith("lines with") and len(body) + 1 == len(out.stdout.splitlines())
    return [tuple(map(int, ln.split("\t"))) for ln in body]


def test_cli_lines(ctx, tmp_path):
    """bmx_cli --regex EXPR --lines [--invert] on the golden input5.txt (one unterminated line) and --regex-star on a log of
    300 lines, against the oracle fed with the host searches' spans."""
    log_bytes, _ = ro.log_text(np.random.default_rng(300), 300, 90, trailing_newline=False)
    for name, text, flag, expr in (("input5.txt", golden_file_bytes("input5.txt"), "--regex", "(Hello|Virus)"),
                                   ("log.txt", log_bytes, "--regex-star", "ERROR[^\\x0a]*timeout"),
                                   ("log.txt", log_bytes, "--regex", "(ERROR|FATAL): [0-9]{2,4}")):
        path = tmp_path / name
        path.write_bytes(text)
        off = ro.split(text, 10)
        rows_n = off.size - 1
        if flag == "--regex":
            s, e = ctx.search_regex_spans(text, expr)
        else:
            s, e = ctx.search_regex_star_spans(text, expr, window=int(np.diff(off).max()))
        ids = ro.row_of(off, s, e)
        hit, cnt = ro.matching(ids, rows_n)
        assert hit.size > 0
        assert cli_lines(path, [flag, expr]) == list(zip(hit.tolist(), cnt.tolist()))
        assert cli_lines(path, [flag, expr, "--invert"]) == [(r,) for r in ro.matching(ids, rows_n, invert=True)[0].tolist()]
