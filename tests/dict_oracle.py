"""Test helper: the dictionary-search answer without Boyer-Moore and without the library's filters.

The patterns are grouped by length.  For each length L every window of the text is keyed on its first min(L, 8)
bytes (a sliding integer in numpy) and looked up among the keys of that length's patterns; a pattern longer than 8
bytes is then compared in full in a Python ``dict``.  The pairs are sorted by (position, pattern index).
"""
from collections import defaultdict

import numpy as np


def _keys(t: np.ndarray, q: int, nw: int) -> np.ndarray:
    key = np.zeros(nw, np.uint64)
    for j in range(q):
        key |= t[j:j + nw].astype(np.uint64) << np.uint64(8 * j)
    return key


def dict_matches(text, patterns, n_own=None):
    """(positions int64, pattern indices int64): every (p, i) with text[p:p + len(patterns[i])] == patterns[i] and
    p < n_own (default: all), ordered by p, then i."""
    t = np.frombuffer(bytes(text), np.uint8)
    n = t.size
    own = n if n_own is None else min(n_own, n)
    by_len = defaultdict(list)
    for i, p in enumerate(patterns):
        p = p.encode("latin-1") if isinstance(p, str) else bytes(p)
        by_len[len(p)].append((p, i))
    out_p, out_i = [], []
    for L, items in by_len.items():
        nw = min(n - L + 1, own)
        if nw <= 0:
            continue
        q = min(L, 8)
        key = _keys(t, q, nw)
        groups = defaultdict(list)  # prefix key -> [(pattern, id)], ids ascending
        for p, i in items:
            groups[int.from_bytes(p[:q], "little")].append((p, i))
        pk = np.array(sorted(groups), dtype=np.uint64)
        hit = np.nonzero(np.isin(key, pk))[0]
        if hit.size == 0:
            continue
        if L <= 8:  # the key is the whole pattern: expand every hit by its group's ids, vectorised
            lists = [np.array([i for _, i in groups[int(k)]], np.int64) for k in pk]
            cnt = np.array([a.size for a in lists], np.int64)
            start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
            flat = np.concatenate(lists)
            g = np.searchsorted(pk, key[hit])
            reps = cnt[g]
            pos = np.repeat(hit.astype(np.int64), reps)
            within = np.arange(pos.size, dtype=np.int64) - np.repeat(np.cumsum(reps) - reps, reps)
            out_p.append(pos)
            out_i.append(flat[np.repeat(start[g], reps) + within])
        else:
            tb = bytes(text)
            full = {}
            for p, i in items:
                full.setdefault(p, []).append(i)
            ps, ids = [], []
            for h in hit.tolist():
                for i in full.get(tb[h:h + L], ()):
                    ps.append(h)
                    ids.append(i)
            out_p.append(np.array(ps, np.int64))
            out_i.append(np.array(ids, np.int64))
    if not out_p:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    pos = np.concatenate(out_p)
    ids = np.concatenate(out_i)
    order = np.lexsort((ids, pos))
    return pos[order], ids[order]


def dict_matches_brute(text, patterns):
    """The definition itself, for small cases."""
    tb = bytes(text)
    pats = [p.encode("latin-1") if isinstance(p, str) else bytes(p) for p in patterns]
    ps, ids = [], []
    for s in range(len(tb)):
        for i, p in enumerate(pats):
            if tb[s:s + len(p)] == p:
                ps.append(s)
                ids.append(i)
    return np.array(ps, np.int64), np.array(ids, np.int64)


class DictIndex:
    """The dictionary as a Python ``dict`` (pattern bytes -> ids), built once: matches(s) answers for many short texts."""

    def __init__(self, patterns):
        self.ids = {}
        for i, p in enumerate(patterns):
            self.ids.setdefault(bytes(p), []).append(i)
        self.lengths = sorted({len(p) for p in self.ids})

    def matches(self, s: bytes):
        ps, ids = [], []
        for a in range(len(s)):
            for L in self.lengths:
                if a + L > len(s):
                    break
                for i in self.ids.get(s[a:a + L], ()):
                    ps.append(a)
                    ids.append(i)
        pos = np.array(ps, np.int64)
        idx = np.array(ids, np.int64)
        order = np.lexsort((idx, pos))
        return pos[order], idx[order]
