"""Test helper: staircase texts c_1^{r_1} c_2^{r_2} .. c_R^{r_R} (lower-case letters, strictly increasing) and the closed
forms of everything the text index and the LCP array compute on them, in numpy and plain Python.  The text is held as a run
list and never materialised here, so a text of 2^31 - 1 bytes costs what a text of 50 bytes costs; tests/test_stair_cases_cpu.py
holds every function to index_oracle, match_oracle, map_oracle and lcp_oracle on small staircases written out as bytes.

For lower-case text the builder's order is the plain one (a suffix that is a prefix of another comes first), so:

  suffix array   The runs appear in order: array indices [start_g, start_g + r_g) hold the suffixes that start in run g.  In
                 a run g < R two suffixes c^a d.. and c^b d.. with a > b differ at byte b, c against the larger d: the one
                 with more c's is smaller, so positions ASCEND.  In the last run c^a is a proper prefix of c^b for a < b: the
                 shorter one is smaller, so positions DESCEND.  Hence sa[j] = j below the last run and sa[j] = n - 1 - (j -
                 start_R) inside it.
  LCP            The first entry of every run is 0 (the letters differ, and lcp[0] = 0).  In a run g < R of length r the
                 neighbours at t - 1 and t share the r - t letters c of the later one: r - 1, r - 2, .., 1.  In the last run
                 the neighbours have t and t + 1 bytes: 1, 2, .., r - 1.
  occurrences    A query of one run c^l occurs at every start of the text's run of c that leaves l letters: one range of
                 positions.  A query of k >= 2 runs needs its first run to END a text run, its middle runs to EQUAL the text
                 runs behind it and its last run to BEGIN the next one: at most one position.  Either way the occurrences
                 are one range [first, first + count) of positions inside one run, which is what occurrence_range returns.

The device builders (device_text, device_sa, device_sa_chunk, device_lcp_chunk) use slice fills and torch.arange only: no
tensor wider than int32 of n elements and no host copy of n bytes."""
import bisect
from typing import List, Sequence, Tuple

import numpy as np

import index_oracle as io
import map_oracle as mp
import match_oracle as mo

KEY_BYTES = 513  # one more than the longest query: a suffix cut here compares with every query as the whole one does


def runs_of(q: bytes) -> List[Tuple[int, int]]:
    """[(byte, length)] of the maximal runs of q."""
    out = []
    for b in q:
        if out and out[-1][0] == b:
            out[-1][1] += 1
        else:
            out.append([b, 1])
    return [(b, l) for b, l in out]


class Staircase:
    def __init__(self, runs: Sequence[Tuple[int, int]], last_ascending: bool = False):
        """runs: (letter, length) pairs, letters lower-case and strictly increasing, lengths >= 1.  last_ascending: the
        WRONG closed form with the last run ascending, for the test that shows the checks reject it."""
        code = lambda c: c[0] if isinstance(c, bytes) else ord(c) if isinstance(c, str) else int(c)
        self.runs = [(code(c), int(r)) for c, r in runs]
        assert self.runs and all(97 <= c <= 122 and r >= 1 for c, r in self.runs)
        assert all(a[0] < b[0] for a, b in zip(self.runs, self.runs[1:])), "letters must increase strictly"
        self.R = len(self.runs)
        self.start = [0]
        for _, r in self.runs:
            self.start.append(self.start[-1] + r)
        self.n = self.start[-1]
        self.letter_run = {c: g for g, (c, _) in enumerate(self.runs)}
        self.last_ascending = last_ascending
        self._keys = {}  # suffix_key's, by position
        self._matches = {}  # match's, by query

    # ---- the text -------------------------------------------------------------------------------------------------------
    def run_at(self, p: int) -> int:
        assert 0 <= p < self.n
        return bisect.bisect_right(self.start, p) - 1

    def slice(self, lo: int, hi: int) -> bytes:
        lo, hi = max(0, lo), min(self.n, hi)
        if lo >= hi:
            return b""
        out = []
        for g in range(self.run_at(lo), self.R):
            a, b = max(lo, self.start[g]), min(hi, self.start[g + 1])
            if a >= b:
                break
            out.append(bytes([self.runs[g][0]]) * (b - a))
        return b"".join(out)

    def text(self) -> bytes:
        return self.slice(0, self.n)

    # ---- suffix array and LCP -------------------------------------------------------------------------------------------
    def _pieces(self, lo: int, hi: int):
        """(g, a, b): the parts [a, b) of the array indices [lo, hi) that lie in run g."""
        assert 0 <= lo <= hi <= self.n
        if lo < hi:
            for g in range(self.run_at(lo), self.R):
                a, b = max(lo, self.start[g]), min(hi, self.start[g + 1])
                if a >= b:
                    break
                yield g, a, b

    def _descends(self, g: int) -> bool:
        return g == self.R - 1 and not self.last_ascending

    def sa_chunk(self, lo: int, hi: int) -> np.ndarray:
        out = np.empty(hi - lo, np.int64)
        for g, a, b in self._pieces(lo, hi):
            j = np.arange(a, b, dtype=np.int64)
            out[a - lo:b - lo] = self.n - 1 - (j - self.start[g]) if self._descends(g) else j
        return out

    def sa_at(self, j: int) -> int:
        g = self.run_at(j)
        return self.n - 1 - (j - self.start[g]) if self._descends(g) else j

    def rank(self, p):
        """The array index of the suffix that starts at p (the inverse of the suffix array); p: an int or an array."""
        s = self.start[self.R - 1]
        if isinstance(p, np.ndarray):
            p = p.astype(np.int64)
            return np.where(p >= s, s + (self.n - 1 - p), p)
        return s + (self.n - 1 - p) if p >= s else p

    def lcp_chunk(self, lo: int, hi: int) -> np.ndarray:
        out = np.empty(hi - lo, np.int64)
        for g, a, b in self._pieces(lo, hi):
            t = np.arange(a, b, dtype=np.int64) - self.start[g]
            out[a - lo:b - lo] = t if g == self.R - 1 else np.where(t == 0, 0, self.runs[g][1] - t)
        return out

    def stats(self, min_len: int) -> Tuple[int, int, int, int]:
        """(max of lcp, the smallest j that attains it, sum of lcp, number of j with lcp[j] >= min_len), by arithmetic: a run
        of r holds 0 and 1 .. r - 1, the largest at its second entry (at its last entry in the last run)."""
        best, at, total, count = 0, 0, 0, 0
        for g, (_, r) in enumerate(self.runs):
            if r - 1 > best:
                best, at = r - 1, self.start[g] + (r - 1 if g == self.R - 1 else 1)
            total += r * (r - 1) // 2
            count += r if min_len <= 0 else max(0, r - min_len)
        return best, at, total, count

    # ---- queries --------------------------------------------------------------------------------------------------------
    def range_of_runs(self, qr: Sequence[Tuple[int, int]]) -> Tuple[int, int]:
        """(first, count): the occurrences of the query with the run list qr are the positions [first, first + count)."""
        g = self.letter_run.get(qr[0][0])
        if g is None:
            return 0, 0
        r = self.runs[g][1]
        if len(qr) == 1:
            return (self.start[g], r - qr[0][1] + 1) if qr[0][1] <= r else (0, 0)
        k = len(qr)
        if g + k > self.R or qr[0][1] > r:
            return 0, 0
        if any(tuple(qr[j]) != self.runs[g + j] for j in range(1, k - 1)):
            return 0, 0
        c, l = qr[-1]
        if self.runs[g + k - 1][0] != c or l > self.runs[g + k - 1][1]:
            return 0, 0
        return self.start[g + 1] - qr[0][1], 1

    def occurrence_range(self, q: bytes) -> Tuple[int, int]:
        q = io.as_bytes(q)
        return self.range_of_runs(runs_of(q)) if q else (0, 0)

    def occurrences(self, q) -> np.ndarray:
        """Every position at which q occurs, ascending (small counts only: the list is written out)."""
        first, count = self.occurrence_range(q)
        return np.arange(first, first + count, dtype=np.int64)

    def suffix_key(self, p: int):
        """index_oracle.model_key of suffix p, cut behind KEY_BYTES bytes (a cut key is longer than every query, so it
        compares as the whole one does; the virtual symbol only follows a suffix that is there to its end).  This repeats
        two rules of index_oracle.model_key and has to follow it if they change: a byte's key is index_oracle._signed2 of
        it (2 * b here: the text is lower case), and ONE virtual symbol ends the suffixes with n - 1 - p even.
        tests/test_stair_cases_cpu.py holds the keys to model_key through sa_range."""
        if p not in self._keys:
            tail = (io.VIRTUAL,) if p + KEY_BYTES >= self.n and (self.n - 1 - p) % 2 == 0 else ()
            self._keys[p] = tuple(2 * b for b in self.slice(p, p + KEY_BYTES)) + tail
        return self._keys[p]

    def is_insertion_point(self, q: bytes, lo: int) -> bool:
        """Suffix sa[lo - 1] is below q and suffix sa[lo] is not, under index_oracle's comparator."""
        pk = tuple(io._signed2(b) for b in io.as_bytes(q))
        if not 0 <= lo <= self.n:
            return False
        return (lo == 0 or self.suffix_key(self.sa_at(lo - 1)) < pk) and (lo == self.n or self.suffix_key(self.sa_at(lo)) >= pk)

    def interval_of_range(self, first: int, count: int) -> Tuple[int, int]:
        """The occurrences are positions of one run: their ranks are a range too, in the last run mirrored."""
        return min(self.rank(first), self.rank(first + count - 1)), count

    def interval(self, q) -> Tuple[int, int]:
        """(lo, cnt) of the array: from occurrences and rank; for a query that does not occur, the insertion point by
        bisection over the closed-form array with the comparator's keys."""
        q = io.as_bytes(q)
        first, count = self.occurrence_range(q)
        if count:
            return self.interval_of_range(first, count)
        pk = tuple(io._signed2(b) for b in q)
        x, y = 0, self.n
        while x < y:
            mid = (x + y) // 2
            if self.suffix_key(self.sa_at(mid)) < pk:
                x = mid + 1
            else:
                y = mid
        return x, 0

    def match(self, q) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(len, lo, cnt) for every position of q (match_oracle's definitions): l is extended while the occurrences are not
        empty; a match of l bytes at i leaves one of l - 1 at i + 1."""
        q = io.as_bytes(q)
        if q not in self._matches:
            self._matches[q] = self._match(q)
        return self._matches[q]

    def _match(self, q: bytes):
        qr = runs_of(q)
        ends = np.cumsum([l for _, l in qr]).tolist()  # run j covers [ends[j] - l_j, ends[j])

        def sub(i, j):  # the run list of q[i:j]
            a = bisect.bisect_right(ends, i)
            out, at = [], i
            while at < j:
                e = min(ends[a], j)
                out.append((qr[a][0], e - at))
                at, a = e, a + 1
            return out

        lens, los, cnts = np.zeros(len(q), np.int64), np.zeros(len(q), np.int64), np.zeros(len(q), np.int64)
        l = 0
        for i in range(len(q)):
            l = max(l - 1, 0)
            while i + l < len(q) and self.range_of_runs(sub(i, i + l + 1))[1]:
                l += 1
            lens[i] = l
            if l:
                los[i], cnts[i] = self.interval_of_range(*self.range_of_runs(sub(i, i + l)))
        return lens, los, cnts

    def matching_statistics(self, q) -> np.ndarray:
        return self.match(q)[0]

    def seeds(self, queries, min_len: int, max_occ: int = 0):
        """(seed_off, qpos, len, lo, cnt) as match_oracle.seeds gives them."""
        blob = b"".join(io.as_bytes(q) for q in queries)
        off = np.concatenate([[0], np.cumsum([len(q) for q in queries])]).astype(np.int64)
        cols = [self.match(q) for q in queries]
        cat = lambda j: np.concatenate([c[j] for c in cols]) if blob else np.zeros(0, np.int64)
        return mo.seeds_from_arrays(off, cat(0), cat(1), cat(2), min_len, max_occ)

    def index_map(self, queries, min_len: int, max_occ: int, k: int, base_offset: int = 0):
        """The outputs of map_oracle.index_map: seeds and their occurrences from the functions above, in order of rank
        (ascending array index), every candidate's (start, end, dist) by map_oracle.in_view on the window's bytes."""
        assert min_len >= 1 and max_occ >= 1 and k >= 0
        best, cands, cand_off, memo = [], [], [0], {}
        for query in queries:
            query = io.as_bytes(query)
            if query not in memo:
                lens, los, cnts = self.match(query)
                mine = []
                for i in mo.seed_positions(lens, cnts, min_len, max_occ):
                    for t in range(int(cnts[i])):
                        w0, w1 = mp.window(self.n, len(query), i, self.sa_at(int(los[i]) + t), k)
                        r = mp.in_view(self.slice(w0, w1), query, k)
                        mine.append(None if r is None else (w0 + r[0], w0 + r[1], r[2]))
                memo[query] = mine
            mine = memo[query]
            hits = [c for c in mine if c is not None]
            best.append(min(hits, key=lambda c: (c[2], c[1])) if hits else None)
            cands += mine
            cand_off.append(len(cands))

        def columns(rows):
            st = np.array([mp.NO_POS if r is None else base_offset + r[0] for r in rows], np.uint64)
            en = np.array([mp.NO_POS if r is None else base_offset + r[1] for r in rows], np.uint64)
            di = np.array([mp.NO_HIT if r is None else r[2] for r in rows], np.int64)
            return st, en, di

        return columns(best) + (np.array(cand_off, np.int64),) + columns(cands)

    # ---- on the device ----------------------------------------------------------------------------------------------------
    def device_text(self):
        import torch

        t = torch.empty(self.n, dtype=torch.uint8, device="cuda")
        for g, (c, _) in enumerate(self.runs):
            t[self.start[g]:self.start[g + 1]] = c
        return t

    def device_sa(self):
        import torch

        s = self.start[self.R - 1]
        sa = torch.arange(self.n, dtype=torch.int32, device="cuda")
        if not self.last_ascending:
            sa[s:] = torch.arange(self.n - 1, s - 1, -1, dtype=torch.int32, device="cuda")
        return sa

    def device_sa_chunk(self, lo: int, hi: int):
        """sa_chunk as an int32 device tensor."""
        import torch

        out = torch.empty(hi - lo, dtype=torch.int32, device="cuda")
        for g, a, b in self._pieces(lo, hi):
            if self._descends(g):
                first = self.n - 1 - (a - self.start[g])
                out[a - lo:b - lo] = torch.arange(first, first - (b - a), -1, dtype=torch.int32, device="cuda")
            else:
                out[a - lo:b - lo] = torch.arange(a, b, dtype=torch.int32, device="cuda")
        return out

    def device_lcp_chunk(self, lo: int, hi: int):
        """lcp_chunk as an int32 device tensor."""
        import torch

        out = torch.empty(hi - lo, dtype=torch.int32, device="cuda")
        for g, a, b in self._pieces(lo, hi):
            s, r = self.start[g], self.runs[g][1]
            if g == self.R - 1:
                out[a - lo:b - lo] = torch.arange(a - s, b - s, dtype=torch.int32, device="cuda")
            else:
                out[a - lo:b - lo] = torch.arange(r - (a - s), r - (b - s), -1, dtype=torch.int32, device="cuda")
                if a == s:
                    out[a - lo] = 0
        return out


def letters(word: str) -> List[Tuple[int, int]]:
    """Runs from a compact spelling: 'a:5 b:1 c:2'."""
    return [(ord(part.split(":")[0]), int(part.split(":")[1])) for part in word.split()]


def random_staircase(rng, max_runs: int = 6, max_len: int = 9) -> Staircase:
    R = int(rng.integers(1, max_runs + 1))
    cs = np.sort(rng.choice(np.arange(97, 123), size=R, replace=False))
    return Staircase([(int(c), int(rng.integers(1, max_len + 1))) for c in cs])


def big_runs():
    """The staircase of tests/test_gpu_index_limits.py: 2^31 - 1 bytes, array indices and positions on both sides of 2^30,
    intervals of more than 2^30 entries, runs of 1, 2 and 3, and a short descending last run that ends at n - 1."""
    fixed = [("a", (1 << 30) + 5), ("b", 1), ("c", 2), ("d", 3), ("e", (1 << 29) + 77), ("f", 600), ("h", 300)]
    rest = (1 << 31) - 1 - sum(r for _, r in fixed)
    return fixed[:6] + [("g", rest)] + fixed[6:]
