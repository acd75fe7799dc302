"""Test helper for the k-mismatch search: the answers in numpy, independent of Shift-Add.

A pattern is ``member`` as in tests/classes_oracle.py: a boolean array [m, 256], member[i][b] = "byte value b belongs to
class i".  ``must`` is a mask: bit i set = position i may not mismatch.
"""
import numpy as np


def must_mask(positions) -> int:
    mask = 0
    for i in positions:
        mask |= 1 << int(i)
    return mask


def hamming_starts(text: bytes, member, k: int, must: int = 0, n_own=None):
    """(starts int64, distances int64): every start p < n_own with p + m <= n whose window has at most k positions outside
    their class and none of them in ``must``, ascending.  Membership per position, mismatches summed over m shifted slices
    of the text."""
    t = np.frombuffer(bytes(text), np.uint8)
    member = np.asarray(member, dtype=bool)
    m = member.shape[0]
    if t.size < m:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    windows = t.size - m + 1
    d = np.zeros(windows, np.int64)
    ok = np.ones(windows, dtype=bool)
    for i in range(m):
        miss = ~member[i][t[i:i + windows]]
        d += miss
        if (must >> i) & 1:
            ok &= ~miss
    ok &= d <= k
    if n_own is not None:
        ok[min(n_own, windows):] = False
    starts = np.nonzero(ok)[0].astype(np.int64)
    return starts, d[starts]


def hamming_starts_brute(text: bytes, member, k: int, must: int = 0, n_own=None):
    """The definition itself, window by window."""
    m = len(member)
    starts, dists = [], []
    for p in range(len(text) - m + 1):
        if n_own is not None and p >= n_own:
            break
        miss = [i for i in range(m) if not member[i][text[p + i]]]
        if len(miss) <= k and not any((must >> i) & 1 for i in miss):
            starts.append(p)
            dists.append(len(miss))
    return np.array(starts, np.int64), np.array(dists, np.int64)
