"""Oracles of the non-overlapping match selection, replace and extract (bmx_spans_select*, bmx_replace*, bmx_extract*):
the sequential loop, the union of the spans, b"".join replace and extract, in plain Python / numpy."""
from __future__ import annotations

import numpy as np

NONE = 0xFFFFFFFFFFFFFFFF


def spans_of(starts=None, ends=None, length=0, rows=None):
    """The list as [(s, e, skipped)] from one of the three input forms; the skip rule of include/bmx.h."""
    lst = starts if starts is not None else ends
    out = []
    for j in range(len(lst)):
        if starts is not None and ends is not None:
            s, e = int(starts[j]), int(ends[j])
        elif starts is not None:
            s = int(starts[j])
            e = s + length - 1
        else:
            e = int(ends[j])
            s = e - (length - 1)
        skip = s < 0 or s >= NONE or e >= NONE or e < s or e < length - 1 or (rows is not None and int(rows[j]) in (NONE, -1))
        out.append((s, e, skip))
    return out


def ordered(spans):
    """s[i] <= e[j] for all non-skipped i < j."""
    top = -1
    for s, e, skip in spans:
        if skip:
            continue
        if top > e:
            return False
        top = max(top, s)
    return True


def select(spans):
    """The sequential loop: (starts, ends, indices) of the entries taken."""
    last = -1
    out = []
    for j, (s, e, skip) in enumerate(spans):
        if skip or s <= last:
            continue
        out.append((s, e, j))
        last = e
    return _columns(out)


def select_pm(spans):
    """The same set through the prefix-maximum identity: key = s + 1 (0: skipped), PM its prefix maximum,
    next[j] = the first i with PM[i] > e[j] + 1, the first entry taken = the first i with PM[i] > 0."""
    key = [0 if skip else s + 1 for s, e, skip in spans]
    pm, top = [], 0
    for v in key:
        top = max(top, v)
        pm.append(top)

    def upper(v):
        lo, hi = 0, len(pm)
        while lo < hi:
            mid = (lo + hi) // 2
            if pm[mid] > v:
                hi = mid
            else:
                lo = mid + 1
        return lo

    out = []
    j = upper(0)
    while j < len(spans):
        s, e, skip = spans[j]
        assert not skip and key[j] == pm[j]
        out.append((s, e, j))
        nxt = upper(e + 1)
        assert nxt > j
        j = nxt
    return _columns(out)


def merge(spans):
    """The connected regions of the union (non-decreasing ends): (starts, ends, index of each region's first entry)."""
    live = [(s, e, j) for j, (s, e, skip) in enumerate(spans) if not skip]
    out = []
    for pos, (s, e, j) in enumerate(live):
        smallest = min(x[0] for x in live[pos:])
        largest = max((x[1] for x in live[:pos]), default=-1)
        if smallest > largest:
            if out:
                out[-1][1] = largest
            out.append([smallest, None, j])
    if out:
        out[-1][1] = max(x[1] for x in live)
    return _columns([tuple(r) for r in out])


def _columns(rows):
    cols = [np.array([r[i] for r in rows], dtype=np.uint64) for i in range(3)]
    return cols[0], cols[1], cols[2]


def replace(text: bytes, starts, ends, repl: bytes, base_offset: int = 0) -> bytes:
    parts, at = [], 0
    for s, e in zip(starts, ends):
        s, e = int(s) - base_offset, int(e) - base_offset
        parts.append(text[at:s])
        parts.append(repl)
        at = e + 1
    parts.append(text[at:])
    return b"".join(parts)


def extract(text: bytes, starts, ends, base_offset: int = 0):
    pieces = [text[int(s) - base_offset:int(e) - base_offset + 1] for s, e in zip(starts, ends)]
    off = np.zeros(len(pieces) + 1, dtype=np.uint64)
    if pieces:
        off[1:] = np.cumsum([len(p) for p in pieces])
    return b"".join(pieces), off


def all_matches(pattern: bytes, text: bytes, longest: bool = False):
    """Every (start, end) with a match of `pattern` ending at `end`, one per end, sorted by end: the start is the largest
    one for that end (the shortest match), or the smallest with `longest`.  What the searches and their starts passes report."""
    import re

    rx = re.compile(pattern, re.DOTALL)
    best = {}
    for s in range(len(text)):
        for e in range(s, len(text)):
            if rx.fullmatch(text, s, e + 1):
                if e not in best or (s < best[e] if longest else s > best[e]):
                    best[e] = s
    ends = sorted(best)
    return np.array([best[e] for e in ends], dtype=np.uint64), np.array(ends, dtype=np.uint64)
