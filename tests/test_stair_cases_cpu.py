"""tests/stair_cases.py against the oracles it stands in for (no GPU): on random staircases of 1 to 6 runs of 1 to 9 letters
and on the boundary forms, every closed form equals index_oracle, match_oracle, map_oracle and lcp_oracle on the text written
out as bytes, for every query test_index_match_cpu.queries_for makes and every string of up to 4 letters over the staircase's
letters and one absent letter.  tests/test_gpu_index_limits.py takes all its expected values at n = 2^31 - 1 from these
functions."""
import numpy as np
import pytest

import index_oracle as io
import lcp_oracle as lo
import map_oracle as mp
import match_oracle as mo
import sa_checks
import stair_cases as sc
from test_index_match_cpu import queries_for

BOUNDARY_FORMS = ["a:1", "k:9", "a:1 b:1", "a:1 b:1 c:1 d:1", "a:5 z:1", "c:1 d:7 e:1", "b:9 c:1 d:1", "a:3 b:1 c:2 d:3 e:4 f:1"]


def staircases():
    rng = np.random.default_rng(0x57A1)
    out = [sc.random_staircase(rng) for _ in range(200)]
    assert {s.R for s in out} == set(range(1, 7)) and {r for s in out for _, r in s.runs} == set(range(1, 10))
    return out + [sc.Staircase(sc.letters(w)) for w in BOUNDARY_FORMS]


def queries(rng, s, text):
    absent = next(c for c in range(97, 123) if c not in s.letter_run)
    short = io.all_queries(bytes(c for c, _ in s.runs) + bytes([absent]), 4)
    whole = [text, text + bytes([absent]), text[1:], text[:-1] or text, text + text[-1:]]
    return short + queries_for(rng, "printable", text, k=8) + [q for q in whole if q]


def check_arrays(s, text):
    n = len(text)
    assert s.n == n and s.slice(0, n) == text
    want = io.model_order(text)
    assert np.array_equal(s.sa_chunk(0, n), want) and [s.sa_at(j) for j in range(n)] == want.tolist()
    assert np.array_equal(s.rank(np.arange(n)), np.argsort(want)) and all(s.rank(int(p)) == j for j, p in enumerate(want))
    lcp = lo.brute(text, want)
    assert np.array_equal(s.lcp_chunk(0, n), lcp)
    for a, b in ((0, 0), (1, n), (n // 2, n), (n // 3, (2 * n) // 3 + 1), (n - 1, n)):  # slices of all three
        a = min(a, b)
        assert np.array_equal(s.sa_chunk(a, b), want[a:b]) and np.array_equal(s.lcp_chunk(a, b), lcp[a:b])
        assert s.slice(a, b) == text[a:b]
    assert s.slice(-3, n + 5) == text
    for min_len in (0, 1, 2, 5, 9, 10):
        m = int(lcp.max())
        assert s.stats(min_len) == (m, int(np.flatnonzero(lcp == m)[0]), int(lcp.sum()), int((lcp >= min_len).sum()))
    return want


@pytest.mark.parametrize("part", range(4))
def test_closed_forms_equal_the_oracles(part):
    rng = np.random.default_rng(0x57A2 + part)
    n_queries = 0
    for s in staircases()[part::4]:
        text = s.text()
        sa = check_arrays(s, text)
        keys = io.suffix_keys(text, sa)
        qs = queries(rng, s, text)
        n_queries += len(qs)
        arrays = []
        for q in qs:
            occ = io.occurrences(text, q)
            assert np.array_equal(s.occurrences(q), occ), (s.runs, q)
            want = io.sa_range(text, sa, q, keys)
            assert s.interval(q) == want, (s.runs, q)
            assert s.is_insertion_point(q, want[0])
            if want[1] == 0:  # ... and nothing else is one
                assert not s.is_insertion_point(q, want[0] + 1) and not s.is_insertion_point(q, want[0] - 1), (s.runs, q)
            lens = mo.matching_statistics(text, q)
            got = s.match(q)
            assert np.array_equal(got[0], lens), (s.runs, q)
            wlo, wcnt = mo.intervals(text, sa, q, lens, keys)
            assert np.array_equal(got[1], wlo) and np.array_equal(got[2], wcnt), (s.runs, q)
            arrays.append((lens, wlo, wcnt))
        assert np.array_equal(s.matching_statistics(qs[-1]), mo.matching_statistics(text, qs[-1]))
        # seeds of EVERY query under two settings: match_oracle's rule over the oracle's own per-byte arrays (what
        # match_oracle.seeds does, without computing them once more); match_oracle.seeds itself under all four settings
        # on a slice of the queries
        off = np.concatenate([[0], np.cumsum([len(q) for q in qs])])
        cols = [np.concatenate([a[j] for a in arrays]) for j in range(3)]
        some = qs[-13:] + qs[:40:3]
        for min_len, max_occ in ((1, 0), (2, 2)):
            for g, w in zip(s.seeds(qs, min_len, max_occ), mo.seeds_from_arrays(off, *cols, min_len, max_occ)):
                assert np.array_equal(g, w), (s.runs, min_len, max_occ)
        for min_len, max_occ in ((1, 0), (2, 0), (2, 2), (1, 1)):
            for g, w in zip(s.seeds(some, min_len, max_occ), mo.seeds(text, sa, some, min_len, max_occ, keys)):
                assert np.array_equal(g, w), (s.runs, min_len, max_occ)
    assert n_queries > 10_000


SETTINGS = ((1, 4, 0), (2, 8, 2), (1, 1, 1), (3, 64, 4))  # (min_len, max_occ, k)


def check_map(s, text, sa, reads, settings):
    for min_len, max_occ, k in settings:
        got = s.index_map(reads, min_len, max_occ, k, base_offset=(1 << 40) + 3)
        want = mp.index_map(text, sa, reads, min_len, max_occ, k, base_offset=(1 << 40) + 3)
        for g, w, name in zip(got, want, ("best_start", "best_end", "best_dist", "cand_off", "cand_start", "cand_end", "cand_dist")):
            assert g.dtype == w.dtype and np.array_equal(g, w), (s.runs, name, min_len, max_occ, k)


@pytest.mark.parametrize("part", range(4))
def test_map_oracle_on_staircases(part):
    """Staircase.index_map against map_oracle.index_map on EVERY staircase under four settings, for the queries_for
    queries, the whole text and its neighbours, the text with a foreign letter in its middle, and every string of up to 2
    letters over the staircase's letters and one absent letter.  Every window is aligned twice by approx_oracle and
    spans_oracle, and the strings of 3 and 4 letters cost up to two seconds per staircase, so they run on a stated subset:
    all the boundary forms and every 40th random staircase (13 in all), under the first two settings."""
    rng = np.random.default_rng(0x57A3 + part)
    longer = 0
    for j, s in list(enumerate(staircases()))[part::4]:
        text = s.text()
        sa = io.model_order(text)
        reads = queries(rng, s, text) + [text[:len(text) // 2] + b"z" + text[len(text) // 2:]]
        check_map(s, text, sa, reads[:short_count(s, 2)] + reads[short_count(s, 4):], SETTINGS)
        if j >= 200 or j % 40 == 13 * part:
            check_map(s, text, sa, reads[short_count(s, 2):short_count(s, 4)], SETTINGS[:2])
            longer += 1
    assert longer >= 3


def short_count(s, max_len):
    """The number of strings of 1 .. max_len letters over the staircase's letters and one absent letter: `queries` lists
    them first, shortest first."""
    return sum((s.R + 1) ** m for m in range(1, max_len + 1))


def test_a_wrong_closed_form_is_rejected():
    """The check is sensitive: the same staircase with its last run ascending is a permutation, and not sorted."""
    for word in ("a:4 b:1 c:5", "k:9", "a:1 b:2"):
        runs = sc.letters(word)
        good, wrong = sc.Staircase(runs), sc.Staircase(runs, last_ascending=True)
        x = np.frombuffer(good.text(), np.uint8)
        assert sa_checks.is_permutation(good.sa_chunk(0, good.n), good.n) and sa_checks.is_sorted(x, good.sa_chunk(0, good.n))
        assert sa_checks.is_permutation(wrong.sa_chunk(0, good.n), good.n)
        assert not sa_checks.is_sorted(x, wrong.sa_chunk(0, good.n))
        assert not np.array_equal(wrong.sa_chunk(0, good.n), io.model_order(good.text()))


def test_the_big_staircase_by_arithmetic():
    """The staircase of the GPU suite: its size, a few entries of both arrays on both sides of 2^30, and the statistics, all
    without writing it out."""
    s = sc.Staircase(sc.big_runs())
    n = (1 << 31) - 1
    assert s.n == n and s.R == 8 and [r for _, r in s.runs][1:4] == [1, 2, 3] and s.runs[-1] == (ord("h"), 300)
    assert s.sa_at(0) == 0 and s.sa_at((1 << 30) + 4) == (1 << 30) + 4 and s.sa_at(n - 300) == n - 1 and s.sa_at(n - 1) == n - 300
    assert s.rank(n - 1) == n - 300 and s.rank(n - 300) == n - 1 and s.rank(12345) == 12345
    assert s.lcp_chunk(0, 3).tolist() == [0, (1 << 30) + 4, (1 << 30) + 3] and s.lcp_chunk(n - 3, n).tolist() == [297, 298, 299]
    assert s.lcp_chunk((1 << 30) + 4, (1 << 30) + 12).tolist() == [1, 0, 0, 1, 0, 2, 1, 0]
    assert s.slice((1 << 30) + 3, (1 << 30) + 13) == b"aabccddde" + b"e" and s.slice(n - 302, n + 9) == b"gg" + b"h" * 300
    assert s.stats((1 << 30) + 4) == ((1 << 30) + 4, 1, sum(r * (r - 1) // 2 for _, r in s.runs), 1)
    assert s.stats((1 << 30) + 5)[3] == 0 and s.stats(0)[3] == n and s.stats(1)[3] == n - 8
    assert s.occurrence_range(b"aabccddde") == ((1 << 30) + 3, 1) and s.occurrence_range(b"abcddde") == (0, 0)
    assert s.interval(b"a") == (0, (1 << 30) + 5) and s.interval(b"hh") == (n - 299, 299) and s.interval(b"h" * 301)[1] == 0
    assert s.is_insertion_point(b"h" * 301, n) and s.is_insertion_point(b"A", 0) and s.is_insertion_point(b"ba", (1 << 30) + 5)
    assert not s.is_insertion_point(b"ba", (1 << 30) + 6) and s.interval(b"ba") == ((1 << 30) + 5, 0)
