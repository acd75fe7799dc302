"""Test helper: the LCP array (bmx_lcp_*) in numpy and plain Python, no GPU.

lcp[0] = 0 and lcp[j] = the number of leading bytes the suffixes sa[j - 1] and sa[j] share, as plain bytes and with
nothing past the end of the text (include/bmx.h, the LCP section).  That is defined for any permutation `sa`; `brute` is
the definition, the other functions are faster references for the texts they are made for.
"""
from typing import Tuple

import numpy as np

from index_oracle import as_bytes


def common_prefix(t: bytes, a: int, b: int) -> int:
    """Leading bytes t[a:] and t[b:] share: equal blocks are skipped whole, the block that differs is walked byte by byte."""
    lim = len(t) - max(a, b)
    h = 0
    while h < lim and t[a + h:a + h + 64] == t[b + h:b + h + 64]:
        h += 64
    while h < lim and t[a + h] == t[b + h]:
        h += 1
    return min(h, lim)


def brute(text, sa) -> np.ndarray:
    """The definition, pair by pair, for any permutation `sa`."""
    t = as_bytes(text)
    sa = [int(v) for v in sa]
    out = np.zeros(len(sa), dtype=np.int32)
    for j in range(1, len(sa)):
        out[j] = common_prefix(t, sa[j - 1], sa[j])
    return out


def kasai(text, sa) -> np.ndarray:
    """Kasai, Lee, Arimura, Arikawa and Park's linear-time loop.  Valid for LEXICOGRAPHIC arrays only: the step "the next
    suffix shares at least h - 1 bytes with its predecessor" needs the order of the suffixes, not just a permutation.  (The
    array bmx_suffix_array builds is lexicographic on lower-case text.)"""
    t = as_bytes(text)
    n = len(t)
    sa = np.asarray(sa, dtype=np.int64)
    rank = np.empty(n, dtype=np.int64)
    rank[sa] = np.arange(n)
    sa_l, rank_l = sa.tolist(), rank.tolist()
    out = [0] * n
    h = 0
    for i in range(n):
        r = rank_l[i]
        if r == 0:
            h = 0
            continue
        j = sa_l[r - 1]
        while i + h < n and j + h < n and t[i + h] == t[j + h]:
            h += 1
        out[r] = h
        if h:
            h -= 1
    return np.array(out, dtype=np.int32)


def wrong_entries(text, sa, lcp) -> np.ndarray:
    """The positions j at which lcp[j] is not the common prefix of the suffixes sa[j - 1] and sa[j], for any permutation
    `sa` and any text, in a few vector operations: the byte behind the prefix differs or is past the end (exact), and the
    prefixes have the same polynomial hash modulo 2^64 (a wrong value passes with probability about 2^-60).  For texts on
    which pair-by-pair comparison is quadratic and no closed form holds."""
    x = np.frombuffer(as_bytes(text), np.uint8)
    n = x.size
    sa = np.asarray(sa, dtype=np.int64)
    h = np.asarray(lcp, dtype=np.int64)
    bad = np.zeros(n, dtype=bool)
    bad[0] = h[0] != 0
    if n > 1:
        a, b, h1 = np.minimum(sa[:-1], sa[1:]), np.maximum(sa[:-1], sa[1:]), h[1:]
        fits = (h1 >= 0) & (b + h1 <= n)
        hc = np.where(fits, h1, 0)
        with np.errstate(over="ignore"):
            pw = np.full(n + 1, 0x9E3779B97F4A7C15, dtype=np.uint64)
            pw[0] = 1
            pw = np.cumprod(pw)
            pre = np.zeros(n + 1, dtype=np.uint64)
            pre[1:] = np.cumsum(x.astype(np.uint64) * pw[:n])
            same = (pre[a + hc] - pre[a]) * pw[b - a] == pre[b + hc] - pre[b]
        ends = b + hc == n
        differs = ends | (x[np.minimum(a + hc, n - 1)] != x[np.minimum(b + hc, n - 1)])
        bad[1:] = ~(fits & same & differs)
    return np.nonzero(bad)[0]


def primitive_period(para: np.ndarray) -> int:
    """The smallest q that divides len(para) with para = tile(para[:q])."""
    p = para.size
    for q in range(1, p + 1):
        if p % q == 0 and np.array_equal(np.tile(para[:q], p // q), para):
            return q
    return p


def periodic_pairs(x: np.ndarray, q: int, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Common prefix of the suffixes a[k] and b[k] (a != b) of x = tile(a paragraph of primitive period q)[:n]: n - max(a, b)
    where a and b are congruent modulo q; otherwise the common prefix of the first 2 q bytes, clipped at the end of the
    text -- two suffixes of different residues that agreed on 2 q bytes would give the paragraph a shorter period (Fine and
    Wilf), so that prefix is below 2 q."""
    n = x.size
    a = np.asarray(a, dtype=np.int64)
    b = np.asarray(b, dtype=np.int64)
    lim = n - np.maximum(a, b)
    out = lim.copy()
    other = np.nonzero((a - b) % q != 0)[0]
    ao, bo, lo = a[other], b[other], lim[other]
    h = np.zeros(other.size, dtype=np.int64)
    alive = np.ones(other.size, dtype=bool)
    for k in range(2 * q):
        alive &= k < lo
        alive[alive] = x[ao[alive] + k] == x[bo[alive] + k]
        h += alive
    out[other] = h
    return out.astype(np.int32)


def periodic(x: np.ndarray, p: int, sa) -> np.ndarray:
    """The LCP array of x = tile(paragraph of p bytes)[:n] over any permutation `sa`, by the rule of periodic_pairs."""
    x = np.asarray(x, dtype=np.uint8)
    sa = np.asarray(sa, dtype=np.int64)
    out = np.zeros(sa.size, dtype=np.int32)
    if sa.size > 1:
        out[1:] = periodic_pairs(x, primitive_period(x[:p]) if x.size >= p else x.size + p, sa[:-1], sa[1:])
    return out


def embedded_pair(L: int, pad: int) -> Tuple[bytes, int, int]:
    """(text, p, q): text = pad + w + 'x' + w + 'y' with w of L random letters a..w and a pad of `pad` distinct capitals.
    The two copies of w, at p and q, are the only suffixes that begin with w: they are neighbours in the suffix array and
    share exactly L bytes, and no other pair shares more (tests/test_lcp_cpu.py checks that for every L it is used with)."""
    rng = np.random.default_rng(0xE3B * 4096 + 8 * L + pad)
    w = bytes((rng.integers(0, 23, L) + 97).astype(np.uint8))
    head = b"ABCDEFGH"[:pad]
    return head + w + b"x" + w + b"y", pad, pad + L + 1
