"""Test helper for the match spans of the approximate search (bmx_approx_spans_device): the start of every match and the
BMX_SPANS_BEST selection in numpy, independent of Myers' bit-parallel form the library runs.

``span_starts`` fills the plain edit table of the REVERSED pattern against the text read backwards from each end, column
by column, for all ends at once: after L columns, row m holds ED(pat, text[j-L+1..j]).  The vertical dependency within a
column, e[i] = min(e[i], e[i-1] + 1), is a running minimum of e[i] - i (as tests/approx_oracle.py does along its rows).
A pattern is bytes / str, or ``member``: a boolean array [m, 256] (tests/classes_oracle.py).
"""
import numpy as np


def _member(pat_or_classes) -> np.ndarray:
    if isinstance(pat_or_classes, str):
        pat_or_classes = pat_or_classes.encode("latin-1")
    if isinstance(pat_or_classes, (bytes, bytearray)):
        member = np.zeros((len(pat_or_classes), 256), dtype=bool)
        member[np.arange(len(pat_or_classes)), np.frombuffer(bytes(pat_or_classes), np.uint8)] = True
        return member
    return np.asarray(pat_or_classes, dtype=bool).reshape(-1, 256)


def span_starts(text, pat_or_classes, k: int, ends):
    """(starts int64, distances int64) for ends j of text: d = min over L of ED(pat, text[j-L+1..j]) over
    L = 1..min(j + 1, m + k), and start = j - L + 1 for the SMALLEST such L (the largest start that attains d)."""
    t = np.frombuffer(bytes(text), np.uint8) if isinstance(text, (bytes, bytearray)) else np.asarray(text, np.uint8)
    member = _member(pat_or_classes)
    m = member.shape[0]
    ends = np.asarray(ends, dtype=np.int64)
    E = ends.size
    rev_miss = ~member[::-1]  # [m, 256]: row i = "the byte does not belong to position m - 1 - i"
    rows = np.arange(m + 1, dtype=np.int32)
    col = np.broadcast_to(rows, (E, m + 1)).copy()  # column 0: D[i][0] = i
    best = np.full(E, 1 << 20, dtype=np.int32)
    best_len = np.zeros(E, dtype=np.int64)
    for L in range(1, m + k + 1):
        at = ends - (L - 1)
        live = at >= 0  # the window is clipped at text[0]
        if not live.any():
            break
        byte = t[np.where(live, at, 0)]
        e = np.empty_like(col)
        e[:, 0] = L
        e[:, 1:] = np.minimum(col[:, :-1] + rev_miss[:, byte].T, col[:, 1:] + 1)  # diagonal / horizontal
        col = np.minimum.accumulate(e - rows, axis=1) + rows  # vertical = running min
        better = live & (col[:, m] < best)
        best = np.where(better, col[:, m], best)
        best_len = np.where(better, L, best_len)
    return ends - best_len + 1, best.astype(np.int64)


def select_best(ends, dist, k: int) -> np.ndarray:
    """Indices kept by BMX_SPANS_BEST: entry i iff dist[i] <= dprev and dist[i] < dnext, where a list neighbour counts
    only if its end is adjacent (else k + 1)."""
    ends = np.asarray(ends, dtype=np.int64)
    dist = np.asarray(dist, dtype=np.int64)
    if ends.size == 0:
        return np.zeros(0, np.int64)
    dprev = np.full(ends.size, k + 1, np.int64)
    dnext = np.full(ends.size, k + 1, np.int64)
    adj = ends[1:] == ends[:-1] + 1  # entry i + 1 directly follows entry i
    dprev[1:][adj] = dist[:-1][adj]
    dnext[:-1][adj] = dist[1:][adj]
    return np.nonzero((dist <= dprev) & (dist < dnext))[0].astype(np.int64)
