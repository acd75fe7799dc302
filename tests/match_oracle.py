"""Test helper: matching statistics and seeds of the text index (bmx_index_match*, bmx_index_seeds*) in plain Python and
numpy, no GPU.

For position i of a query of m bytes, len[i] is the largest l <= m - i such that query[i : i + l] occurs in the text
(bytes.find: plain byte equality, p + l <= n); (lo[i], cnt[i]) is the interval of the index's array whose suffixes begin
with query[i : i + len[i]] (index_oracle.sa_range over model_order), (0, 0) where len[i] == 0.  Position i is a seed for
(min_len, max_occ) iff len[i] >= min_len, i == 0 or len[i - 1] <= len[i], and max_occ == 0 or cnt[i] <= max_occ."""
from typing import List, Sequence, Tuple

import numpy as np

import index_oracle as io


def longest_match_at(text: bytes, rest: bytes) -> int:
    """The largest l such that rest[:l] occurs in text, one length after the other from 1 (no shortcut)."""
    l = 0
    while l < len(rest) and text.find(rest[:l + 1]) >= 0:
        l += 1
    return l


def matching_statistics(text, query) -> np.ndarray:
    """len[i] for every position of the query, by bytes.find.  A match that starts at i and has l bytes leaves one of
    l - 1 bytes at i + 1, so the search at i + 1 starts from there (test_index_match_cpu.py holds this to
    longest_match_at)."""
    t, q = io.as_bytes(text), io.as_bytes(query)
    out, l = np.zeros(len(q), np.int64), 0
    for i in range(len(q)):
        l = max(l - 1, 0)
        while i + l < len(q) and t.find(q[i:i + l + 1]) >= 0:
            l += 1
        out[i] = l
    return out


def intervals(text, sa: Sequence[int], query, lens: Sequence[int], keys=None) -> Tuple[np.ndarray, np.ndarray]:
    """(lo, cnt) of query[i : i + lens[i]] for every position, (0, 0) where lens[i] == 0."""
    t, q = io.as_bytes(text), io.as_bytes(query)
    if keys is None:
        keys = io.suffix_keys(t, sa)
    lo, cnt = np.zeros(len(q), np.int64), np.zeros(len(q), np.int64)
    for i, l in enumerate(lens):
        if l > 0:
            lo[i], cnt[i] = io.sa_range(t, sa, q[i:i + int(l)], keys)
    return lo, cnt


def seed_positions(lens: Sequence[int], cnts: Sequence[int], min_len: int, max_occ: int = 0) -> List[int]:
    """The seeds of ONE query from its matching statistics, by the definition."""
    assert min_len >= 1
    return [i for i in range(len(lens))
            if lens[i] >= min_len and (i == 0 or lens[i - 1] <= lens[i]) and (max_occ == 0 or cnts[i] <= max_occ)]


def seeds(text, sa: Sequence[int], queries: Sequence[bytes], min_len: int, max_occ: int = 0, keys=None):
    """(seed_off, qpos, len, lo, cnt) of a column of queries, in order of (query, position)."""
    t = io.as_bytes(text)
    if keys is None:
        keys = io.suffix_keys(t, sa)
    seed_off, rows = [0], []
    for q in queries:
        lens = matching_statistics(t, q)
        lo, cnt = intervals(t, sa, q, lens, keys)
        for i in seed_positions(lens, cnt, min_len, max_occ):
            rows.append((i, int(lens[i]), int(lo[i]), int(cnt[i])))
        seed_off.append(len(rows))
    cols = np.array(rows, np.int64).reshape(-1, 4)
    return np.array(seed_off, np.int64), cols[:, 0], cols[:, 1], cols[:, 2], cols[:, 3]


def seeds_from_arrays(off: Sequence[int], lens: np.ndarray, lo: np.ndarray, cnt: np.ndarray, min_len: int, max_occ: int = 0):
    """The same from per-blob-byte arrays that are already known to be right (off: the count + 1 query offsets)."""
    seed_off, rows = [0], []
    for a, b in zip(off[:-1], off[1:]):
        a, b = int(a), int(b)
        for i in seed_positions(lens[a:b], cnt[a:b], min_len, max_occ):
            rows.append((i, int(lens[a + i]), int(lo[a + i]), int(cnt[a + i])))
        seed_off.append(len(rows))
    cols = np.array(rows, np.int64).reshape(-1, 4)
    return np.array(seed_off, np.int64), cols[:, 0], cols[:, 1], cols[:, 2], cols[:, 3]
