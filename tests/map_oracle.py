"""Test helper: read mapping over the text index (bmx_index_map*) in numpy and plain Python, no GPU.

Built from helpers that exist: match_oracle's matching statistics and seed rule give the seeds (their occurrences by
bytes.find, ordered as the index's array orders them; test_index_map_cpu.py holds that to match_oracle.seeds), approx_oracle.approx_ends the distance at every end of
a candidate's window, spans_oracle.span_starts the start.  For a seed (q, i, len, lo, cnt) and t in [0, cnt): the
occurrence is p = sa[lo + t], the diagonal d = p - i, the window [w0, w1) = [max(0, d - k), min(n, d + m + k)).  On the
view text[w0:w1]: dist = the minimum over ends j of D(j) = min over s of ED(query, view[s..j]), end = the largest j that
attains it, start = the largest s with ED(query, view[s..end]) == dist.  A candidate is a hit iff dist <= k.  Per query the
hit with the smallest (dist, end) is the answer.  Candidates are in order of (query, seed, t) and not de-duplicated."""
import numpy as np

import approx_oracle as ao
import index_oracle as io
import match_oracle as mo
import spans_oracle as so

NO_HIT = 255
NO_POS = 0xFFFFFFFFFFFFFFFF


def window(n: int, m: int, i: int, p: int, k: int):
    d = p - i
    return max(0, d - k), min(n, d + m + k)


_VIEWS = {}


def in_view(view: bytes, query: bytes, k: int):
    """(start, end, dist) inside the view, or None if the best distance is above k.  The answer depends on the window's
    bytes only, so equal windows (two seeds on one diagonal, the same read under another max_occ) are computed once."""
    key = (view, query, k)
    if key not in _VIEWS:
        ends, dists = ao.approx_ends(view, query, len(query))  # k = m: every end of the view (D(j) <= m always)
        assert ends.size == len(view)
        dist = int(dists.min())
        if dist > k:
            _VIEWS[key] = None
        else:
            end = int(ends[np.flatnonzero(dists == dist)[-1]])
            starts, d2 = so.span_starts(view, query, k, [end])
            assert int(d2[0]) == dist, "the start pass and the search disagree"
            _VIEWS[key] = (int(starts[0]), end, dist)
    return _VIEWS[key]


def candidate(text: bytes, query: bytes, i: int, p: int, k: int):
    """(start, end, dist) of one candidate in text coordinates, or None if its best distance is above k."""
    w0, w1 = window(len(text), len(query), i, p, k)
    r = in_view(text[w0:w1], query, k)
    return None if r is None else (w0 + r[0], w0 + r[1], r[2])


def seed_occurrences(text: bytes, rank, query: bytes, min_len: int, max_occ: int):
    """[(i, occurrences in the order of the index's array)] for the seeds of one query.  The interval of a match is exactly
    its set of occurrences (test_index_match_cpu.py), so sa[lo : lo + cnt] is that set ordered by rank = the inverse of
    sa; no suffix keys are needed, which keeps long texts cheap."""
    lens = mo.matching_statistics(text, query)
    out = []
    for i in range(len(query)):
        if lens[i] < min_len or (i > 0 and lens[i - 1] > lens[i]):
            continue
        occ = io.occurrences(text, query[i:i + int(lens[i])])
        if occ.size <= max_occ:
            out.append((i, occ[np.argsort(rank[occ], kind="stable")]))
    return out


def index_map(text, sa, queries, min_len: int, max_occ: int, k: int, base_offset: int = 0):
    """(best_start, best_end uint64, best_dist int64, cand_off int64, cand_start, cand_end uint64, cand_dist int64)."""
    assert min_len >= 1 and max_occ >= 1 and k >= 0
    t = io.as_bytes(text)
    rank = np.empty(len(t), np.int64)
    rank[np.asarray(sa, np.int64)] = np.arange(len(t))
    best, cands, cand_off, memo = [], [], [0], {}
    for query in queries:
        query = io.as_bytes(query)
        if query not in memo:
            memo[query] = [candidate(t, query, i, int(p), k) for i, occ in seed_occurrences(t, rank, query, min_len, max_occ)
                           for p in occ]
        mine = memo[query]
        hits = [c for c in mine if c is not None]
        best.append(min(hits, key=lambda c: (c[2], c[1])) if hits else None)
        cands += mine
        cand_off.append(len(cands))

    def columns(rows):
        st = np.array([NO_POS if r is None else base_offset + r[0] for r in rows], np.uint64)
        en = np.array([NO_POS if r is None else base_offset + r[1] for r in rows], np.uint64)
        di = np.array([NO_HIT if r is None else r[2] for r in rows], np.int64)
        return st, en, di

    return columns(best) + (np.array(cand_off, np.int64),) + columns(cands)


def edit_reads(rng, text: bytes, count: int, m: int, max_edits: int, letters: bytes, at_ends: int = 0):
    """`count` reads of about m bytes cut from the text, each with 0..max_edits random substitutions, insertions or
    deletions; the first `at_ends` reads alternate between the text's first and last m bytes.  Returns (reads, planted
    starts, edits made)."""
    reads, starts, edits = [], [], []
    for r in range(count):
        p = int(rng.integers(0, len(text) - m + 1))
        if r < at_ends:
            p = 0 if r % 2 == 0 else len(text) - m
        read = bytearray(text[p:p + m])
        e = int(rng.integers(0, max_edits + 1))
        for _ in range(e):
            kind, at = int(rng.integers(0, 3)), int(rng.integers(0, len(read)))
            c = letters[int(rng.integers(0, len(letters)))]
            if kind == 0:
                read[at] = c
            elif kind == 1:
                read.insert(at, c)
            elif len(read) > 1:
                del read[at]
        reads.append(bytes(read))
        starts.append(p)
        edits.append(e)
    return reads, starts, edits


def lower_case_order(text: bytes, prefix: int = 96) -> np.ndarray:
    """index_oracle.model_order for a text of lower-case letters whose suffixes differ within `prefix` bytes (asserted):
    every byte is above the virtual symbol, so the builder's order is the plain one, and a bounded key keeps 10^4..10^5
    bytes cheap.  A suffix shorter than the key is a proper prefix of nothing it ties with, so it sorts below its
    extensions as "nothing" does."""
    assert min(text) >= 97
    keys = [text[i:i + prefix] for i in range(len(text))]
    assert len(set(keys)) == len(keys), "two suffixes agree on their first `prefix` bytes"
    return np.array(sorted(range(len(text)), key=keys.__getitem__), dtype=np.int32)
