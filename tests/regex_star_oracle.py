"""Test helper for the regular-expression search with unbounded repetition, written from the description of
bmx_compile_regex_star and of the bmx_search_regex_star* entries in include/bmx.h, not from the C code: regex_oracle's
grammar with the three quantifiers ``*``, ``+`` and ``{a,}``, the Glushkov sets with cycles, a matcher that carries position
sets, the answers for larger texts, a translation to Python's ``re`` with a brute force over it, a generator of random
expressions, the identity the slow path of csrc/bmx_regex_star_kernel.h rests on, restated on Python ints, and a model of
the first launch on the tile frame's geometry (``fast_taint``: which lanes end their pair warm-up with two different
bounds, how many waves hold one, and the lower-bound list such a launch reports).

An automaton is a ``StarRx``: regex_oracle's ``Rx`` whose ``follow`` may point anywhere; ``max_len`` is UNBOUNDED where a
cycle lies among the positions a match can use.
"""
import re

import numpy as np

import classes_oracle as co
import regex_oracle as ro
from classes_oracle import ExprError
from regex_oracle import bits

UNBOUNDED = -1
NO_START = (1 << 64) - 1


def useful(m, first, last, follow):
    """The positions reachable from ``first`` from which ``last`` can be reached."""
    fwd, bwd = first, last
    grown = True
    while grown:
        grown = False
        for i in range(m):
            if (fwd >> i) & 1 and follow[i] & ~fwd:
                fwd |= follow[i]
                grown = True
            if not (bwd >> i) & 1 and follow[i] & bwd:
                bwd |= 1 << i
                grown = True
    return fwd & bwd


def lengths(m, first, last, follow):
    """(shortest, longest) match in bytes; longest is UNBOUNDED where a cycle lies among the useful positions, and both
    are 0 where nothing can match."""
    use = useful(m, first, last, follow)
    if not use:
        return 0, 0
    # shortest: breadth first
    dist, frontier, d = {}, first & use, 1
    while frontier:
        for i in bits(frontier):
            dist[i] = d
        nxt = 0
        for i in bits(frontier):
            nxt |= follow[i] & use
        frontier = nxt & ~sum(1 << i for i in dist)
        d += 1
    lo = min(dist[i] for i in bits(last & use))
    # a cycle: depth-first colouring
    colour = {}

    def cyclic(i):
        colour[i] = 1
        for j in bits(follow[i] & use):
            if colour.get(j) == 1 or (j not in colour and cyclic(j)):
                return True
        colour[i] = 2
        return False

    if any(i not in colour and cyclic(i) for i in bits(use)):
        return lo, UNBOUNDED
    longest = {}

    def deep(i):
        if i not in longest:
            longest[i] = 1 + max([deep(j) for j in bits(follow[i] & use)] + ([0] if (last >> i) & 1 else []))
        return longest[i]

    return lo, max(deep(i) for i in bits(first & use))


class StarRx:
    def __init__(self, member, first, last, follow):
        self.member = np.asarray(member, bool).reshape(-1, 256)
        self.m = len(self.member)
        self.first, self.last, self.follow = int(first), int(last), [int(f) for f in follow]
        self.min_len, self.max_len = lengths(self.m, self.first, self.last, self.follow)
        self.B = [sum(1 << i for i in range(self.m) if self.member[i][c]) for c in range(256)]
        self._memo = {}

    def follow_of(self, D):
        """The OR of follow[i] over the positions of D."""
        f = self._memo.get(D)
        if f is None:
            f = 0
            for i in bits(D):
                f |= self.follow[i]
            self._memo[D] = f
        return f

    def step(self, D, c, seed=True):
        return ((self.first if seed else 0) | self.follow_of(D)) & self.B[c]


# ---- the grammar ----------------------------------------------------------------------------------------------------
# regex_oracle's tree, with ("rep", node, a, None) for a repeat without an upper count.

def _repeat(toks, at, flags, depth):
    if ro._op(toks, at, b"?{*+"):
        raise ExprError("a quantifier with nothing in front of it")
    if ro._op(toks, at, b"("):
        if depth + 1 > ro.MAX_DEPTH:
            raise ExprError("nesting deeper than 32")
        node, at = _alt(toks, at + 1, flags, depth + 1)
        if not ro._op(toks, at, b")"):
            raise ExprError("unbalanced (")
        at += 1
    else:
        row, at = ro._element(toks, at, flags)
        node = ("elem", row)
    a = b = 1
    if ro._op(toks, at, b"?"):
        a, at = 0, at + 1
    elif ro._op(toks, at, b"*"):
        a, b, at = 0, None, at + 1
    elif ro._op(toks, at, b"+"):
        a, b, at = 1, None, at + 1
    elif ro._op(toks, at, b"{"):
        a, at = ro._number(toks, at + 1)
        b = a
        if ro._op(toks, at, b","):
            if ro._op(toks, at + 1, b"}"):
                b, at = None, at + 1
            else:
                b, at = ro._number(toks, at + 1)
        if not ro._op(toks, at, b"}"):
            raise ExprError("unterminated {...}")
        at += 1
        if b is not None and (b < 1 or a > b):
            raise ExprError("b == 0 or a > b")
    else:
        return node, at
    if ro._op(toks, at, b"?{*+"):
        raise ExprError("a quantifier right after another quantifier")
    return ("rep", node, a, b), at


def _alt(toks, at, flags, depth):
    alts = []
    while True:
        cat = []
        while at < len(toks) and not ro._op(toks, at, b"|)"):
            node, at = _repeat(toks, at, flags, depth)
            cat.append(node)
        alts.append(("cat", cat))
        if not ro._op(toks, at, b"|"):
            return ("alt", alts), at
        at += 1


def tree(expr, flags: int = 0):
    e = expr.encode("latin-1") if isinstance(expr, str) else bytes(expr)
    if flags & ~(ro.ICASE | ro.IUPAC):
        raise ExprError("an unknown flag bit")
    toks = co._tokens(e)
    node, at = _alt(toks, 0, flags, 0)
    if at < len(toks):
        raise ExprError("unbalanced )")
    return node


class _Glushkov(ro._Glushkov):
    """regex_oracle's recursion and the one rule more: X+ links every last position of X to the first positions of X.
    X{a,} is a - 1 copies of X followed by X+; a == 0 makes it X*, which is (X+)?."""

    def walk(self, node):
        if node[0] != "rep" or node[3] is not None or not ro._has_element(node):
            return super().walk(node)
        _, sub, a, _ = node
        f = (True, 0, 0)
        copies = max(a, 1)
        for i in range(copies):
            g = self.walk(sub)
            if i == copies - 1:
                for l in bits(g[2]):
                    self.follow[l] |= g[1]
                g = (g[0] or a == 0, g[1], g[2])
            f = self.cat(f, g)
        return f


def parse(expr, flags: int = 0) -> StarRx:
    """The grammar of bmx_compile_regex_star -> StarRx; raises ExprError where the library returns BMX_ERR_ARG."""
    g = _Glushkov()
    nullable, first, last = g.walk(tree(expr, flags))
    if not g.rows:
        raise ExprError("zero positions")
    if nullable:
        raise ExprError("matches the empty string")
    return StarRx(np.array(g.rows), first, last, g.follow)


# ---- Python's re, and the definition by brute force -----------------------------------------------------------------

def _re_text(node) -> bytes:
    kind = node[0]
    if kind == "elem":
        vals = np.nonzero(node[1])[0]
        return b"[" + b"".join(b"\\x%02x" % v for v in vals) + b"]" if vals.size else b"(?:(?!))"
    if kind == "cat":
        return b"".join(_re_text(k) for k in node[1])
    if kind == "alt":
        return b"(?:" + b"|".join(_re_text(k) for k in node[1]) + b")"
    _, sub, a, b = node
    if not ro._has_element(sub):
        return b""  # (the empty string, whatever its counts)
    return b"(?:" + _re_text(sub) + (b"){%d,}" % a if b is None else b"){%d,%d}" % (a, b))


def to_re(expr, flags: int = 0):
    """The expression in Python's syntax: bytes, DOTALL, every group non-capturing, every class spelt out."""
    return re.compile(_re_text(tree(expr, flags)), re.DOTALL)


def ends_brute(text, expr, flags: int = 0, window=None):
    """The definition: for every end j, every start s (within ``window`` bytes of j if given), re.fullmatch of the
    substring.  Returns (ends, shortest-match starts, longest-match starts) as lists.  For tiny inputs."""
    rx = to_re(expr, flags)
    text = bytes(text)
    ends, short, long_ = [], [], []
    for j in range(len(text)):
        s0 = 0 if window is None else max(0, j + 1 - window)
        ok = [s for s in range(s0, j + 1) if rx.fullmatch(text[s:j + 1])]
        if ok:
            ends.append(j)
            short.append(ok[-1])
            long_.append(ok[0])
    return ends, short, long_


# ---- the automaton's answers ----------------------------------------------------------------------------------------

def states(text, rx: StarRx, entry: int = 0, seed: bool = True):
    """The state behind every byte of ``text`` entered with the set ``entry`` (a list of ints)."""
    D, out = entry, []
    for c in bytes(text):
        D = rx.step(D, c, seed)
        out.append(D)
    return out


def ends_numpy(text, rx: StarRx) -> np.ndarray:
    """Every end, ascending (int64): the set-carrying matcher, one int per byte."""
    last = rx.last
    return np.array([j for j, D in enumerate(states(text, rx)) if D & last], np.int64)


def reverse(rx: StarRx) -> StarRx:
    return StarRx(rx.member[::-1], *_flipped(rx))


def _flipped(rx):
    m = rx.m

    def flip(s):
        return sum(1 << (m - 1 - i) for i in bits(s))

    follow = [0] * m
    for i in range(m):
        for j in bits(rx.follow[i]):
            follow[m - 1 - j] |= 1 << (m - 1 - i)
    return flip(rx.last), flip(rx.first), follow


def starts_numpy(text, rx: StarRx, ends, window: int, longest: bool = False) -> np.ndarray:
    """For every end of ``ends`` the start of the shortest match of at most ``window`` bytes that ends there (``longest``:
    of the longest such), NO_START where there is none (uint64): the reversed automaton, anchored at the end, walked back."""
    t = bytes(text)
    rv = reverse(rx)
    out = np.full(len(ends), NO_START, np.uint64)
    for k, j in enumerate(int(e) for e in ends):
        D, seed = 0, True
        for L in range(1, min(window, j + 1) + 1):
            D = rv.step(D, t[j - L + 1], seed)
            seed = False
            if D == 0:
                break
            if D & rv.last:
                out[k] = j - L + 1
                if not longest:
                    break
    return out


def plant_path(rng, text, rx: StarRx, at, stop=0.3):
    """Overwrite text (uint8 array) from ``at`` on with an instance of a random path from ``first`` to ``last`` over the
    useful positions with a non-empty class; at a position of ``last`` the path ends with probability ``stop`` (or where
    nothing follows).  Returns the index behind the copy."""
    alive = [i for i in range(rx.m) if rx.member[i].any()]
    follow = [f if i in alive else 0 for i, f in enumerate(rx.follow)]
    mask = sum(1 << i for i in alive)
    use = useful(rx.m, rx.first & mask, rx.last & mask, [f & mask for f in follow])
    here = list(bits(rx.first & use))
    while here and at < text.size:
        i = int(rng.choice(here))
        text[at] = rng.choice(np.nonzero(rx.member[i])[0])
        at += 1
        here = list(bits(follow[i] & use))
        if (rx.last >> i) & 1 and (not here or rng.random() < stop):
            break
    return at


# ---- random expressions ---------------------------------------------------------------------------------------------

def _rand_quant(rng):
    r = int(rng.integers(0, 14))
    if r < 5:
        return ""
    if r < 7:
        return "?"
    if r == 7:
        return "{%d}" % int(rng.integers(1, 4))
    if r == 8:
        a = int(rng.integers(0, 3))
        return "{%d,%d}" % (a, max(1, a + int(rng.integers(0, 3))))
    if r < 11:
        return "+"
    if r < 13:
        return "*"
    return "{%d,}" % int(rng.integers(0, 4))


def _rand_concat(rng, symbols, depth):
    parts = []
    for _ in range(int(rng.integers(1, 4))):
        if depth < 3 and rng.integers(0, 3) == 0:
            alts = [_rand_concat(rng, symbols, depth + 1) for _ in range(int(rng.integers(1, 4)))]
            if rng.integers(0, 6) == 0:
                alts.insert(int(rng.integers(0, len(alts) + 1)), "")  # an empty alternative
            atom = "(" + "|".join(alts) + ")"
        else:
            atom = ro._rand_element(rng, symbols)
        parts.append(atom + _rand_quant(rng))
    return "".join(parts)


def random_regex(rng, symbols, max_m=8, cyclic=None):
    """(expression str, StarRx) over the byte values ``symbols``: regex_oracle's generator with * + {a,} on elements and on
    groups.  Nullable expressions and those over max_m positions are drawn again; ``cyclic`` True / False asks for an
    automaton with / without a cycle."""
    symbols = np.asarray(symbols)
    while True:
        alts = [_rand_concat(rng, symbols, 0) for _ in range(1 if rng.integers(0, 4) else 2)]
        expr = "|".join(alts)
        try:
            rx = parse(expr)
        except ExprError:
            continue
        if rx.m <= max_m and rx.max_len != 0 and (cyclic is None or cyclic == (rx.max_len == UNBOUNDED)):
            return expr, rx


# ---- the identity behind the slow path ------------------------------------------------------------------------------
# Follow is built from OR and AND, so the state after a stretch of text entered with the set X is
#     c | OR over u in X of col[u]
# with c the run from the empty set (``first`` seeding every step) and col[u] the run from {u} alone without seeding.

def run(text, rx: StarRx, entry: int, seed: bool) -> int:
    D = entry
    for c in bytes(text):
        D = rx.step(D, c, seed)
    return D


# The kernels cut pieces and tiles in ALIGNED coordinates: view byte i is aligned byte i + first, first = pointer mod 16,
# and the ``first`` bytes in front of the view are stepped with an empty class word, which leaves the empty state.

def run_aligned(text: bytes, rx: StarRx, first: int, a: int, b: int, entry: int, seed: bool) -> int:
    """The state behind the aligned bytes [a, b) (clipped to the text's end) entered with ``entry``."""
    D = entry
    for i in range(a, min(b, len(text) + first)):
        D = rx.step(D, text[i - first], seed) if i >= first else 0
    return D


def pair_bounds(text, rx: StarRx, piece: int, first: int = 0):
    """(e, u) per piece of ``piece`` aligned bytes: e_l the state in front of piece l from the pair walk's lower bound (over
    piece l - 1 from the empty set; piece 0 and piece 1 are exact), u_l = f_l & ~e_l with f_l the upper bound (from every
    position)."""
    t = bytes(text)
    full = getattr(rx, "all", (1 << rx.m) - 1)  # (masked(): the useful positions)
    n_pieces = (len(t) + first + piece - 1) // piece
    e, u = [], []
    for l in range(n_pieces):
        if l == 0:
            e.append(0), u.append(0)
            continue
        lo = run_aligned(t, rx, first, (l - 1) * piece, l * piece, 0, True)
        hi = run_aligned(t, rx, first, (l - 1) * piece, l * piece, 0 if l == 1 else full, True)
        e.append(lo), u.append(hi & ~lo)
    return e, u


def columns(text, rx: StarRx, piece: int, e, u, first: int = 0):
    """(base, cols) per piece: base_l the state behind piece l entered with e_l, cols_l[r] the unseeded run of the piece
    from the r-th position of u_l."""
    t = bytes(text)
    base, cols = [], []
    for l in range(len(e)):
        base.append(run_aligned(t, rx, first, l * piece, (l + 1) * piece, e[l], True))
        cols.append([run_aligned(t, rx, first, l * piece, (l + 1) * piece, 1 << p, False) for p in bits(u[l])])
    return base, cols


def sweep(e, u, base, cols, use_columns: bool = True):
    """The true state in front of every piece: a piece with u == 0 knows it (e), the others get it from the piece before:
    truth(l + 1) = base_l | OR over the positions of truth(l) & u_l of their column.  ``use_columns`` False leaves the
    column term out (what a sweep that carried ``base`` alone would give: a lower bound again)."""
    entry = [0] * len(e)
    for l in range(len(e)):
        if u[l] == 0:
            entry[l] = e[l]
        else:
            k = l - 1
            nxt = base[k]
            if use_columns:
                rank = {p: r for r, p in enumerate(bits(u[k]))}
                for p in bits(entry[k] & u[k]):
                    nxt |= cols[k][rank[p]]
            entry[l] = nxt
    return entry


# ---- the tile frame's geometry and a model of the first launch ---------------------------------------------------------

def masked(rx: StarRx) -> StarRx:
    """The automaton the host hands the kernels: only the positions a match can use (the others are taken out of the
    classes, of first, last and follow[]); its ``all`` is where the upper bound starts."""
    use = useful(rx.m, rx.first, rx.last, rx.follow)
    member = rx.member.copy()
    for i in range(rx.m):
        if not (use >> i) & 1:
            member[i] = False
    k = StarRx(member, rx.first & use, rx.last & use, [f & use if (use >> i) & 1 else 0 for i, f in enumerate(rx.follow)])
    k.all = use
    return k


def tile_lanes(n: int, first: int, lead: int, ps: int):
    """(tile, lane, lo, hi) for every lane that owns ends, in aligned coordinates, as bmx_tile_frame.h cuts them: tiles of
    256 << ps ends counted from aligned byte 0, lane l of a tile the 1 << ps ends from tile0 + (l << ps), both clipped to
    [lead + first, n + first)."""
    own_lo, own_hi = lead + first, n + first
    shift = ps + 8
    for tile in range(own_lo >> shift, (own_hi + (1 << shift) - 1) >> shift):
        tile0 = tile << shift
        for lane in range(256):
            lo, hi = max(tile0 + (lane << ps), own_lo), min(tile0 + ((lane + 1) << ps), own_hi)
            if lo < hi:
                yield tile, lane, lo, hi


class FastTaint:
    """What fast_taint returns: ``lanes`` the (tile, lane) pairs whose two bounds did not meet, ``waves`` the number of
    (tile, 64 consecutive lanes) that hold one (regex_star_last()["tainted"]), ``ends`` the list the launch reports (every
    lane walked from its lower bound; view coordinates, ascending, int64)."""

    def __init__(self, lanes, waves, ends):
        self.lanes, self.waves, self.ends = lanes, waves, ends


def fast_taint(text, rx: StarRx, first: int, lead: int, ps: int, warm: int, walk: bool = True) -> FastTaint:
    """RegexStarPolicy<.., ENTRY = false>::walk on the tile frame's geometry: a lane with the owned ends [lo, hi) runs the
    lower state e (from the empty set) and the upper state f (from every useful position) over the aligned bytes
    [start16 - warm, start16), start16 = lo & ~15; a warm-up that would begin at or in front of aligned byte 0
    (start16 <= warm) begins there with e = f = 0.  The lane is tainted where e != f; either way it reports the ends of
    the walk from e.  ``walk`` False: the warm-ups alone (``ends`` stays empty)."""
    t = bytes(text)
    k = masked(rx)
    last = k.last
    lanes, waves, ends = [], set(), []
    for tile, lane, lo, hi in tile_lanes(len(t), first, lead, ps):
        start16 = lo & ~15
        e, f, a = (0, 0, 0) if start16 <= warm else (0, k.all, start16 - warm)
        for i in range(a, start16):
            if i < first:
                e = f = 0
            elif e == f:  # (met: they stay equal)
                e = f = k.step(e, t[i - first])
            else:
                e, f = k.step(e, t[i - first]), k.step(f, t[i - first])
        if e != f:
            lanes.append((tile, lane))
            waves.add((tile, lane >> 6))
        D = e
        for i in range(start16, hi if walk else start16):
            D = k.step(D, t[i - first]) if i >= first else 0
            if i >= lo and D & last:
                ends.append(i - first)
    return FastTaint(lanes, len(waves), np.array(ends, np.int64))


def entry_ends(text, rx: StarRx, first: int, lead: int, ps: int, entry) -> np.ndarray:
    """RegexStarPolicy<.., ENTRY = true>::walk: every lane starts at the first byte of the aligned piece that holds its
    first owned end, in the state ``entry`` gives for that piece."""
    t = bytes(text)
    ends = []
    for _, _, lo, hi in tile_lanes(len(t), first, lead, ps):
        piece = lo >> ps
        D = entry[piece]
        for i in range(piece << ps, hi):
            D = rx.step(D, t[i - first]) if i >= first else 0
            if i >= lo and D & rx.last:
                ends.append(i - first)
    return np.array(ends, np.int64)


def slow_ends(text, rx: StarRx, first: int, lead: int, ps: int, use_columns: bool = True) -> np.ndarray:
    """The slow path's list: pair bounds, columns and sweep over the aligned pieces from piece 0 (what lies in front of
    ``lead`` counts), then the walk from the swept states."""
    k = masked(rx)
    e, u = pair_bounds(text, k, 1 << ps, first)
    base, cols = columns(text, k, 1 << ps, e, u, first)
    return entry_ends(text, k, first, lead, ps, sweep(e, u, base, cols, use_columns))
