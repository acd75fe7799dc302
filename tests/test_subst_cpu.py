"""CPU suite of the non-overlapping match selection, replace and extract (bmx_spans_select*, bmx_replace*, bmx_extract*):
the oracle (tests/subst_oracle.py) against Python's ``re`` and ``bytes``, the prefix-maximum identity the kernels rest on
against the sequential loop, the tiled chain walk of csrc/bmx_subst_kernel.h restated in Python against the same loop, and
every argument error of the six C entries with ctx = NULL, which has to come back as BMX_ERR_ARG before any HIP call and
touch no output."""
import ctypes as C
import re

import numpy as np
import pytest

import subst_oracle as so
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

P = C.c_void_p(0x1000)  # a non-NULL pointer that no valid call dereferences before its checks fail
NONE = so.NONE


def two_letter(rng, n, letters=b"ab"):
    return bytes(rng.choice(list(letters), n).astype(np.uint8))


def every_occurrence(pattern: bytes, text: bytes):
    """(starts, ends) of every occurrence, overlapping ones included, ascending: what the searches report."""
    rx = re.compile(b"(?=(" + pattern + b"))", re.DOTALL)
    found = [(m.start(1), m.end(1) - 1) for m in rx.finditer(text)]
    return np.array([s for s, _ in found], dtype=np.uint64), np.array([e for _, e in found], dtype=np.uint64)


# ---- the oracle against re / bytes ---------------------------------------------------------------------------------

@pytest.mark.parametrize("pattern", [b"aa", b"aba", b"a", b"abab", b"[ab]b", b"a[ab]a", b"b.b"])
def test_select_oracle_is_finditer_for_fixed_length_patterns(pattern):
    rng = np.random.default_rng(len(pattern) * 7 + pattern[0])
    for n in (0, 1, 2, 4, 37, 400):
        text = two_letter(rng, n) if n != 4 else b"aaaa"
        starts, ends = every_occurrence(pattern, text)
        spans = so.spans_of(starts, ends)
        assert so.ordered(spans)
        s, e, idx = so.select(spans)
        want = [(m.start(), m.end() - 1) for m in re.finditer(pattern, text, re.DOTALL)]
        assert list(zip(s.tolist(), e.tolist())) == want
        assert np.array_equal(starts[idx.astype(np.int64)], s)
        assert so.replace(text, s, e, b"XY") == re.sub(pattern, b"XY", text, flags=re.DOTALL)
        assert so.replace(text, s, e, b"") == re.sub(pattern, b"", text, flags=re.DOTALL)
        blob, off = so.extract(text, s, e)
        assert [blob[off[i]:off[i + 1]] for i in range(off.size - 1)] == re.findall(pattern, text, re.DOTALL)
        # the one-list forms give the same selection
        m = int(e[0] - s[0] + 1) if s.size else 1
        if starts.size and all(int(b) - int(a) + 1 == m for a, b in zip(starts, ends)):
            assert np.array_equal(so.select(so.spans_of(starts, None, m))[0], s)
            assert np.array_equal(so.select(so.spans_of(None, ends, m))[0], s)


def test_select_oracle_counts_like_bytes_count_and_replaces_like_bytes_replace():
    assert so.select(so.spans_of(*every_occurrence(b"aa", b"aaaa")))[0].tolist() == [0, 2]
    rng = np.random.default_rng(3)
    for lit in (b"aa", b"ab", b"aab", b"bbbb"):
        text = two_letter(rng, 600)
        s, e, _ = so.select(so.spans_of(*every_occurrence(re.escape(lit), text)))
        assert s.size == text.count(lit)
        assert so.replace(text, s, e, b"-") == text.replace(lit, b"-")


@pytest.mark.parametrize("pattern,letters", [(b"[0-9]+", b"01x"), (b"(ab)+", b"ab"), (b"(ab)+", b"abx")])
def test_merge_oracle_is_the_mask_of_covered_bytes(pattern, letters):
    rng = np.random.default_rng(11)
    rx = re.compile(pattern)
    for n in (0, 1, 5, 60, 200):
        text = two_letter(rng, n, letters)
        covered = np.zeros(n + 1, dtype=bool)
        for s in range(n):  # every match from every start, through lookahead-free fullmatch on every window
            for e in range(s, n):
                if rx.fullmatch(text, s, e + 1):
                    covered[s:e + 1] = True
        edges = np.flatnonzero(np.diff(np.concatenate(([False], covered)).astype(np.int8)))
        want = list(zip(edges[0::2].tolist(), (edges[1::2] - 1).tolist()))
        starts, ends = so.all_matches(pattern, text, longest=True)
        ms, me, _ = so.merge(so.spans_of(starts, ends))
        got = list(zip(ms.tolist(), me.tolist()))
        if pattern == b"[0-9]+":
            assert got == want == [(m.start(), m.end() - 1) for m in rx.finditer(text)]
        else:  # abutting regions stay apart: the mask joins them
            joined = []
            for s, e in got:
                if joined and joined[-1][1] + 1 == s:
                    joined[-1] = (joined[-1][0], e)
                else:
                    joined.append((s, e))
            assert joined == want


def test_merge_oracle_keeps_abutting_spans_apart_and_merges_overlapping_ones():
    spans = so.spans_of(np.array([0, 3, 4, 9, 2]), np.array([2, 5, 6, 9, 12]))
    s, e, idx = so.merge(spans)
    assert (s.tolist(), e.tolist(), idx.tolist()) == ([0], [12], [0])
    spans = so.spans_of(np.array([0, 3, 4, 9]), np.array([2, 5, 6, 9]))
    s, e, idx = so.merge(spans)
    assert (s.tolist(), e.tolist(), idx.tolist()) == ([0, 3, 9], [2, 6, 9], [0, 1, 3])


# ---- the identity and the tiled chain ----------------------------------------------------------------------------------

def random_list(rng, count, by_start):
    """A list in order (non-decreasing ends, or non-decreasing starts with varying lengths) with skipped entries of all
    three kinds."""
    if by_start:
        s = np.sort(rng.integers(0, 4 * count + 8, count))
        # s[i] <= e[j] for i < j: every end reaches at least the largest start before it
        e = np.maximum(s + rng.integers(0, 9, count), np.maximum.accumulate(s))
    else:
        e = np.sort(rng.integers(8, 4 * count + 16, count))
        s = e - rng.integers(0, 9, count)
    s, e = s.astype(np.uint64), e.astype(np.uint64)
    rows = np.zeros(count, dtype=np.uint64)
    kind = rng.integers(0, 12, count)
    s[kind == 0] = NONE
    flip = kind == 1
    s[flip], e[flip] = e[flip] + 1, s[flip]
    rows[kind == 2] = NONE
    return s, e, rows


def tiled_chain(spans, shift):
    """csrc/bmx_subst_kernel.h in Python: next, X_1 .. X_L by `shift` rounds of pointer jumping inside blocks of T^l
    entries, the top walk, the descent; returns the taken flags and the most pointers any one walk followed."""
    count, T = len(spans), 1 << shift
    key = [0 if skip else s + 1 for s, e, skip in spans]
    pm, top = [], 0
    for v in key:
        top = max(top, v)
        pm.append(top)
    upper = lambda v: next((i for i, p in enumerate(pm) if p > v), count)
    x = [[max(upper(e + 1), j + 1) if not skip else j + 1 for j, (s, e, skip) in enumerate(spans)]]
    levels = 0
    while (count - 1) >> (shift * (levels + 1)):
        levels += 1
    for v in range(1, levels + 1):
        cur = list(x[v - 1])
        for _ in range(shift):
            end = [min(((j >> (shift * v)) + 1) << (shift * v), count) for j in range(count)]
            cur = [cur[c] if c < end[j] else c for j, c in enumerate(cur)]
        x.append(cur)
    taken = [0] * count
    entry = [dict() for _ in range(levels + 1)]
    longest = 0
    p, steps = upper(0), 0
    while p < count:
        if levels == 0:
            taken[p] = 1
        else:
            entry[levels][p >> (shift * levels)] = p
        p, steps = x[levels][p], steps + 1
    longest = steps
    for v in range(levels, 0, -1):
        for b, q in entry[v].items():
            end, steps = min((b + 1) << (shift * v), count), 0
            while q < end:
                if v == 1:
                    taken[q] = 1
                else:
                    entry[v - 1][q >> (shift * (v - 1))] = q
                q, steps = x[v - 1][q], steps + 1
            longest = max(longest, steps)
    assert longest <= T
    return taken, levels


@pytest.mark.parametrize("by_start", [False, True])
def test_prefix_maximum_identity_against_the_loop(by_start):
    rng = np.random.default_rng(29 + by_start)
    for trial in range(1500):
        count = int(rng.integers(0, 40)) if trial % 10 else int(rng.integers(40, 400))
        s, e, rows = random_list(rng, count, by_start)
        spans = so.spans_of(s, e, 0, rows)
        assert so.ordered(spans)
        a, b = so.select(spans), so.select_pm(spans)
        assert all(np.array_equal(u, v) for u, v in zip(a, b))
        # disjoint, and maximal: every entry left out overlaps an entry taken or is skipped
        assert np.all(a[0][1:] > a[1][:-1])


def test_order_condition_is_the_prefix_maximum_check():
    rng = np.random.default_rng(5)
    for _ in range(600):
        count = int(rng.integers(1, 30))
        s = rng.integers(0, 60, count)
        e = s + rng.integers(0, 6, count)
        spans = so.spans_of(s, e)
        top, by_pm = 0, True
        for ss, ee, _ in spans:
            by_pm &= top <= ee + 1
            top = max(top, ss + 1)
        assert by_pm == so.ordered(spans)


@pytest.mark.parametrize("shift,counts", [(3, [1, 2, 7, 8, 9, 63, 64, 65, 73, 511, 512, 513, 600]), (2, [15, 16, 17, 64, 65, 300])])
def test_tiled_chain_walk_takes_what_the_loop_takes(shift, counts):
    rng = np.random.default_rng(shift)
    for count in counts:
        for by_start in (False, True):
            s, e, rows = random_list(rng, count, by_start)
            spans = so.spans_of(s, e, 0, rows)
            taken, levels = tiled_chain(spans, shift)
            want_levels = 0
            while (1 << (shift * (want_levels + 1))) < count:
                want_levels += 1
            assert levels == want_levels
            assert np.flatnonzero(taken).tolist() == so.select(spans)[2].tolist()
    # one span over everything behind it, and all disjoint
    n = 600
    for s, e in ((np.arange(n), np.full(n, n)), (3 * np.arange(n), 3 * np.arange(n) + 1)):
        spans = so.spans_of(s, e)
        assert np.flatnonzero(tiled_chain(spans, 3)[0]).tolist() == so.select(spans)[2].tolist()


# ---- argument errors, ctx = NULL -------------------------------------------------------------------------------------------

def test_select_argument_errors(built):
    L = host.lib()
    n_out = C.c_uint64(77)
    tail = (C.byref(n_out), None)
    for fn, tail in ((L.bmx_spans_select_device, (C.byref(n_out), None)), (L.bmx_spans_select, (C.byref(n_out),))):
        assert fn(None, None, None, 4, 4, None, 0, P, P, None, 8, *tail) == host.ERR_ARG  # no list
        assert fn(None, P, P, 4, 4, None, 0, P, P, None, 8, *tail) == host.ERR_ARG  # both lists and a length
        assert fn(None, P, None, 0, 4, None, 0, P, P, None, 8, *tail) == host.ERR_ARG  # starts alone, no length
        assert fn(None, None, P, 0, 4, None, 0, P, P, None, 8, *tail) == host.ERR_ARG  # ends alone, no length
        assert fn(None, P, P, 0, 4, None, 2, P, P, None, 8, *tail) == host.ERR_ARG  # unknown flag
        assert fn(None, P, P, 0, 1 << 32, None, 0, P, P, None, 8, *tail) == host.ERR_ARG  # count too large
        assert fn(None, P, P, 0, 4, None, 0, None, P, None, 8, *tail) == host.ERR_ARG  # capacity without starts_out
        assert fn(None, P, P, 0, 4, None, 0, P, None, None, 8, *tail) == host.ERR_ARG  # capacity without ends_out
        assert n_out.value == 77
        assert fn(None, P, P, 0, 4, None, 0, P, P, None, 8, None, *tail[1:]) == host.ERR_ARG  # NULL n_out
        assert fn(None, None, None, 0, 0, None, host.SELECT_MERGE, None, None, None, 0, *tail) == host.OK  # count == 0: nothing to do
        assert n_out.value == 0
        n_out.value = 77
    for starts, ends, ln in ((P, P, 0), (P, None, 4), (None, P, 4)):  # the three valid forms, but no context
        assert L.bmx_spans_select_device(None, starts, ends, ln, 4, None, 0, P, P, P, 8, C.byref(n_out), None) == host.ERR_ARG
    assert n_out.value == 77
    assert L.bmx_last_subst_ms(None) < 0
    assert host.SELECT_MERGE == 1 and host.MAX_REPLACEMENT == 65536


def test_replace_and_extract_argument_errors(built):
    L = host.lib()
    n_out = C.c_uint64(77)
    far = C.c_void_p(0x100000)
    repl = b"xy"

    def replace(fn, text=P, n=64, starts=P, ends=P, ln=0, count=4, r=repl, rl=2, out=far, cap=64, no=C.byref(n_out)):
        dev = fn is L.bmx_replace_device
        args = [None, text, n] + ([0] if dev else []) + [starts, ends, ln, count, r, rl, out, cap, no] + ([None] if dev else [])
        return fn(*args)

    def extract(fn, text=P, n=64, starts=P, ends=P, ln=0, count=4, out=far, cap=64, off=P, no=C.byref(n_out)):
        dev = fn is L.bmx_extract_device
        args = [None, text, n] + ([0] if dev else []) + [starts, ends, ln, count, out, cap, off, no] + ([None] if dev else [])
        return fn(*args)

    for call, fns in ((replace, (L.bmx_replace_device, L.bmx_replace)), (extract, (L.bmx_extract_device, L.bmx_extract))):
        for fn in fns:
            assert call(fn, text=None) == host.ERR_ARG  # NULL text
            assert call(fn, n=1 << 40) == host.ERR_ARG  # n too large
            assert call(fn, count=1 << 32) == host.ERR_ARG  # count too large
            assert call(fn, starts=None, ends=None, ln=4) == host.ERR_ARG  # no list
            assert call(fn, ln=4) == host.ERR_ARG  # both lists and a length
            assert call(fn, ends=None) == host.ERR_ARG  # starts alone, no length
            assert call(fn, starts=None) == host.ERR_ARG  # ends alone, no length
            assert call(fn, out=None) == host.ERR_ARG  # capacity without a buffer
            assert call(fn, no=None) == host.ERR_ARG  # NULL n_out
            assert call(fn, out=C.c_void_p(0x1000 + 63), cap=8) == host.ERR_ARG  # the output overlaps the text's last byte
            assert call(fn, out=C.c_void_p(0x1000 - 7), cap=8) == host.ERR_ARG  # ... its first byte
    for fn in (L.bmx_replace_device, L.bmx_replace):
        assert replace(fn, r=None) == host.ERR_ARG  # NULL replacement with a length
        assert replace(fn, rl=host.MAX_REPLACEMENT + 1) == host.ERR_ARG  # replacement too long
    for fn in (L.bmx_extract_device, L.bmx_extract):
        assert extract(fn, off=None) == host.ERR_ARG  # NULL offsets
    for starts, ends, ln in ((P, P, 0), (P, None, 4), (None, P, 4)):  # the three valid forms, but no context
        assert replace(L.bmx_replace_device, starts=starts, ends=ends, ln=ln) == host.ERR_ARG
        assert extract(L.bmx_extract_device, starts=starts, ends=ends, ln=ln) == host.ERR_ARG
    assert replace(L.bmx_replace_device, r=None, rl=0, out=C.c_void_p(0x1000 + 64), cap=8) == host.ERR_ARG  # abutting is no overlap: the context is missing
    assert n_out.value == 77
    # no span and nothing to copy: answered without a device
    assert replace(L.bmx_replace_device, text=None, n=0, starts=None, ends=None, count=0, out=None, cap=0) == host.OK and n_out.value == 0
    assert replace(L.bmx_replace_device, starts=None, ends=None, count=0, out=None, cap=0) == host.OK and n_out.value == 64
    buf, out = C.create_string_buffer(b"abcdef"), C.create_string_buffer(8)
    assert L.bmx_replace(None, C.cast(buf, C.c_void_p), 6, None, None, 0, 0, None, 0, C.cast(out, C.c_void_p), 8, C.byref(n_out)) == host.OK
    assert (n_out.value, out.raw[:6]) == (6, b"abcdef")
    off = (C.c_uint64 * 1)(9)
    assert L.bmx_extract(None, C.cast(buf, C.c_void_p), 6, None, None, 0, 0, None, 0, off, C.byref(n_out)) == host.OK
    assert (n_out.value, off[0]) == (0, 0)
