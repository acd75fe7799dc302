"""Test helper: the approximate-search answer by Sellers' dynamic programme, row by row in numpy.

Independent of Myers' bit-parallel form the library runs: row i of the edit table over the whole text at once, with
a free start (row 0 is all zeros).  The horizontal dependency within a row, e[j] = min(e[j], e[j-1] + 1), is a running
minimum of e[j] - j.  About 6 s for 16 MiB at m = 16: fully checked texts stay at that size or below.
"""
import numpy as np


def approx_ends(text: bytes, pat: bytes, k: int):
    """(ends int64, distances int64): every end j with min over s of ED(pat, text[s..j]) <= k, ascending."""
    t = np.frombuffer(bytes(text), np.uint8)
    p = np.frombuffer(bytes(pat), np.uint8)
    idx = np.arange(t.size + 1, dtype=np.int64)
    prev = np.zeros(t.size + 1, np.int64)  # row 0: free start
    for i in range(1, p.size + 1):
        e = np.empty(t.size + 1, np.int64)
        e[0] = i
        e[1:] = np.minimum(prev[:-1] + (t != p[i - 1]), prev[1:] + 1)  # diagonal / vertical
        prev = np.minimum.accumulate(e - idx) + idx  # horizontal = running min
    d = prev[1:]
    ends = np.nonzero(d <= k)[0]
    return ends, d[ends]


def edit_distance(a: bytes, b: bytes) -> int:
    """Plain Levenshtein distance (two rows), for the brute-force check of approx_ends."""
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j - 1] + (a[i - 1] != b[j - 1]), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return prev[len(b)]


def approx_ends_brute(text: bytes, pat: bytes, k: int):
    """The definition itself: for every end j the minimum over all starts s <= j + 1 of ED(pat, text[s..j])."""
    ends, dists = [], []
    for j in range(len(text)):
        best = min(edit_distance(pat, text[s:j + 1]) for s in range(j + 2))
        if best <= k:
            ends.append(j)
            dists.append(best)
    return np.array(ends, np.int64), np.array(dists, np.int64)
