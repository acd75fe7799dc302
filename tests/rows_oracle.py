"""Test helper: the row-wise results (bmx_rows_*, include/bmx.h) restated in numpy alone.

    split(text, d)            offsets of the rows of a text split at the delimiter byte d (wc -l semantics)
    row_of(off, s, e)         the row of every match [s, e] (e the last byte), NONE where there is none
    matching(ids, rows, inv)  the distinct rows of a list of row ids with their counts, or the rows without an entry
    log_text(rng, n, max_len) a log of n lines with planted tokens, and where they were planted
"""
import numpy as np

NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def split(text, d: int, base_offset: int = 0) -> np.ndarray:
    """off[0] = base_offset, off[i] = base_offset + (position of the i-th d) + 1, off[rows] = base_offset + n; a text that
    ends with d has no extra empty row, an empty text has no row and the single entry off[0]."""
    t = np.frombuffer(bytes(text), np.uint8) if isinstance(text, (bytes, bytearray)) else np.asarray(text, np.uint8)
    cut = np.flatnonzero(t == d).astype(np.uint64) + np.uint64(1)
    off = np.concatenate([np.zeros(1, np.uint64), cut])
    if t.size and t[-1] != d:
        off = np.concatenate([off, np.array([t.size], np.uint64)])
    return off + np.uint64(base_offset)


def row_of(off, s, e) -> np.ndarray:
    """The r with off[r] <= s and e < off[r + 1] for every pair, else NONE.  A start of NONE and an end below its start
    have no row."""
    off = np.asarray(off, np.uint64)
    s = np.asarray(s, np.uint64)
    e = np.asarray(e, np.uint64)
    rows = off.size - 1
    r = np.searchsorted(off, e, side="right").astype(np.int64) - 1  # the largest r with off[r] <= e
    ok = (r >= 0) & (r < rows) & (s != NONE) & (e >= s)
    rc = np.clip(r, 0, max(rows - 1, 0))
    ok &= s >= off[rc]
    out = np.full(e.shape, NONE, np.uint64)
    out[ok] = r[ok].astype(np.uint64)
    return out


def matching(ids, rows: int, invert: bool = False):
    """(distinct rows ascending, counts) of the entries that are not NONE; inverted: (the rows of [0, rows) without an
    entry, None)."""
    ids = np.asarray(ids, np.uint64)
    hit, counts = np.unique(ids[ids != NONE], return_counts=True)
    if invert:
        return np.setdiff1d(np.arange(rows, dtype=np.uint64), hit), None
    return hit, counts.astype(np.uint64)


TOKENS = [b"ERROR: 123", b"FATAL: 42", b"ERROR: 7", b"PANIC: 99999", b"ERROR disk timeout", b"WARN: 12", b"timeout ERROR"]


def log_text(rng, n_lines: int, max_len: int, trailing_newline: bool = True):
    """(text bytes, plants): n_lines lines of 0..max_len printable-95 bytes, every fourth or so with one of TOKENS
    written over its head where it fits; plants = [(line, token)]."""
    lens = rng.integers(0, max_len + 1, n_lines)
    body = (rng.integers(0, 95, int(lens.sum())) + 32).astype(np.uint8)
    lines, plants, at = [], [], 0
    for i, ln in enumerate(lens.tolist()):
        line = body[at:at + ln].copy()
        at += ln
        if rng.integers(0, 4) == 0:
            tok = TOKENS[int(rng.integers(0, len(TOKENS)))]
            if len(tok) <= ln:
                p = int(rng.integers(0, ln - len(tok) + 1))
                line[p:p + len(tok)] = np.frombuffer(tok, np.uint8)
                plants.append((i, tok))
        lines.append(line.tobytes())
    text = b"\n".join(lines) + (b"\n" if trailing_newline and n_lines else b"")
    return text, plants
