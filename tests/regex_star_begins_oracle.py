"""Test helper for the begins search and the ends pass of expressions with ``*``, ``+`` and ``{a,}``
(bmx_search_regex_star_begins*, bmx_regex_star_ends_device) and for leftmost-longest matching with them, written from the
descriptions in include/bmx.h and DESIGN.md s31: the definition by brute force over Python's ``re``, the automaton's answer
through the reversed automaton on the reversed text, the windowed ends with the clipped count, the sequential definition of
the POSIX matches with a window and a per-row limit, the downward slow path (bounds, columns, sweep, walk from the swept
states) restated on Python ints, and a model of the first launch on the tile frame's geometry.

It imports the existing oracles and changes none.
"""
import numpy as np

import regex_star_oracle as so
from regex_oracle import bits

NONE = 0xFFFFFFFFFFFFFFFF


def begins_brute(text, expr, flags: int = 0):
    """The definition: for every start s, every end e, re.fullmatch of the substring.  Returns (starts, shortest ends,
    longest ends) as lists.  Independent of the automaton; for texts of at most 64 bytes."""
    text = bytes(text)
    assert len(text) <= 64
    rx = so.to_re(expr, flags)
    starts, short, long_ = [], [], []
    for s in range(len(text)):
        ok = [e for e in range(s, len(text)) if rx.fullmatch(text, s, e + 1)]
        if ok:
            starts.append(s)
            short.append(ok[0])
            long_.append(ok[-1])
    return starts, short, long_


def begins_numpy(text, rx: so.StarRx) -> np.ndarray:
    """Every start, ascending (int64): text[s..e] matches rx iff the mirrored substring matches reverse(rx), so the ends of
    reverse(rx) on the reversed text are the starts."""
    t = bytes(text)[::-1]
    return (len(t) - 1 - so.ends_numpy(t, so.reverse(rx)))[::-1].astype(np.int64)


def ends_numpy(text, rx: so.StarRx, starts, window: int, limit=None, longest: bool = False):
    """(ends uint64, clipped): for every start the end of the shortest match of at most ``window`` bytes that begins there
    (``longest``: of the longest such) and uses no byte past limit[i] (if given) or past the text; NONE where there is
    none.  An entry is clipped when the anchored run over the useful positions holds a position with a successor after
    ``window`` bytes and neither its limit nor the text's end would have stopped it there."""
    t = bytes(text)
    k = so.masked(rx)
    out = np.full(len(starts), NONE, np.uint64)
    clipped = 0
    for i, s in enumerate(int(x) for x in starts):
        room = len(t) - s
        if limit is not None:
            room = min(room, int(limit[i]) - s + 1) if int(limit[i]) >= s else 0
        steps = min(room, window)
        D, seed = 0, True
        for L in range(1, steps + 1):
            D = k.step(D, t[s + L - 1], seed)
            seed = False
            if D == 0:
                break
            if D & k.last and (longest or out[i] == NONE):
                out[i] = s + L - 1
        else:
            if steps == window and room > window and k.follow_of(D) != 0:
                clipped += 1
    return out, clipped


def posix_matches(text, rx: so.StarRx, window=None, limit_of=None):
    """The sequential definition of leftmost-longest: at position p take the smallest start s >= p from which a match of at
    most ``window`` bytes begins that stays inside limit_of(s) (the last byte of the row of s), take its longest such end,
    continue at e + 1.  Returns [(s, e)]."""
    t = bytes(text)
    n = len(t)
    k = so.masked(rx)
    out, p = [], 0
    while p < n:
        found = None
        for s in range(p, n):
            top = n - 1 if limit_of is None else min(n - 1, limit_of(s))
            if window is not None:
                top = min(top, s + window - 1)
            D, seed, best = 0, True, None
            for j in range(s, top + 1):
                D = k.step(D, t[j], seed)
                seed = False
                if D == 0:
                    break
                if D & k.last:
                    best = j
            if best is not None:
                found = (s, best)
                break
        if found is None:
            break
        out.append(found)
        p = found[1] + 1
    return out


def posix_brute(text, expr, flags: int = 0):
    """The same through ``re`` alone (no window, no limit), for tiny texts."""
    rx = so.to_re(expr, flags)
    t = bytes(text)
    out, p = [], 0
    while p < len(t):
        found = None
        for s in range(p, len(t)):
            ok = [e for e in range(s, len(t)) if rx.fullmatch(t, s, e + 1)]
            if ok:
                found = (s, ok[-1])
                break
        if found is None:
            break
        out.append(found)
        p = found[1] + 1
    return out


# ---- the kernels' geometry: aligned coordinates, view byte i = aligned byte i + first, the view ends at n + first --------

def reversed_masked(rx: so.StarRx) -> so.StarRx:
    """What the host hands the kernels: the useful positions only, mirrored; ``all`` is where the upper bound starts."""
    k = so.masked(rx)
    r = so.reverse(k)
    r.all = sum(1 << (rx.m - 1 - i) for i in bits(k.all))
    return r


def run_down(t: bytes, k: so.StarRx, first: int, a: int, b: int, entry: int, seed: bool) -> int:
    """The state below aligned byte a after the aligned bytes b - 1, ..., a, entered with ``entry``; a byte past the view
    is stepped with an empty class word, the bytes in front of the view are left out (nothing depends on them)."""
    D = entry
    for i in range(b - 1, max(a, first) - 1, -1):
        D = k.step(D, t[i - first], seed) if i < len(t) + first else 0
    return D


def lanes(n: int, first: int, tail: int, ps: int):
    """(tile, lane, lo, hi) of every lane that owns starts: the frame's cut of [first, n - tail + first)."""
    return so.tile_lanes(n - tail, first, 0, ps)


def _walk_down(t, k, first, top, D, lo, hi, out):
    got = []
    for i in range(min(top, len(t) + first) - 1, lo - 1, -1):
        D = k.step(D, t[i - first])
        if i < hi and D & k.last:
            got.append(i - first)
    out.extend(got[::-1])


class FastTaintDown:
    """``lanes``: the (tile, lane) pairs whose two bounds did not meet, with the bounds; ``waves``: the number of (tile, 64
    consecutive lanes) that hold one (regex_star_begins_last()["tainted"]); ``starts``: the list the launch reports."""

    def __init__(self, lanes, waves, starts):
        self.lanes, self.waves, self.starts = lanes, waves, starts


def fast_taint_down(text, rx: so.StarRx, first: int, tail: int, ps: int, warm: int) -> FastTaintDown:
    """RegexStarBeginsPolicy<.., ENTRY = false>::walk: a lane with the starts [lo, hi) runs e (from the empty set) and f
    (from every useful position) over the aligned bytes [top16, top16 + warm) downwards, top16 = roundup16(hi); a warm-up
    that would begin at or past the view's end (top16 + warm >= n + first) begins on the view's last byte with e = f = 0.
    Tainted where e != f; either way the lane reports the starts of the walk from e."""
    t = bytes(text)
    k = reversed_masked(rx)
    view_hi = len(t) + first
    bad, waves, starts = [], set(), []
    for tile, lane, lo, hi in lanes(len(t), first, tail, ps):
        top16 = (hi + 15) & ~15
        if top16 + warm >= view_hi:
            e = f = run_down(t, k, first, top16, view_hi, 0, True)
        else:
            e = run_down(t, k, first, top16, top16 + warm, 0, True)
            f = run_down(t, k, first, top16, top16 + warm, k.all, True)
        if e != f:
            bad.append((tile, lane, e, f))
            waves.add((tile, lane >> 6))
        _walk_down(t, k, first, top16, e, lo, hi, starts)
    return FastTaintDown(bad, len(waves), np.array(starts, np.int64))


def slow_begins(text, rx: so.StarRx, first: int, tail: int, ps: int, use_columns: bool = True) -> np.ndarray:
    """The slow path's list: pieces of 1 << ps aligned bytes numbered from the TOP of the view (piece l = aligned piece
    p_top - l), the pair bounds of every piece's entry state (the state above its top byte; piece 0 enters with 0 and piece
    1 has f = 0), the columns, regex_star_oracle's sweep unchanged, then every lane's walk from the swept state of the piece
    that holds its last start."""
    t = bytes(text)
    k = reversed_masked(rx)
    piece = 1 << ps
    p_top = (len(t) + first - 1) >> ps
    span = lambda l: ((p_top - l) * piece, (p_top - l + 1) * piece)
    e, u = [0], [0]
    for l in range(1, p_top + 1):
        a, b = span(l - 1)
        lo = run_down(t, k, first, a, b, 0, True)
        hi = run_down(t, k, first, a, b, 0 if l == 1 else k.all, True)
        e.append(lo), u.append(hi & ~lo)
    base = [run_down(t, k, first, *span(l), e[l], True) for l in range(p_top + 1)]
    cols = [[run_down(t, k, first, *span(l), 1 << p, False) for p in bits(u[l])] for l in range(p_top + 1)]
    entry = so.sweep(e, u, base, cols, use_columns)
    starts = []
    for _, _, lo, hi in lanes(len(t), first, tail, ps):
        p = (hi - 1) >> ps
        _walk_down(t, k, first, (p + 1) << ps, entry[p_top - p], lo, hi, starts)
    return np.array(starts, np.int64)
