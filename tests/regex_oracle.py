"""Test helper for the regular-expression search, written from the description of bmx_compile_regex and struct bmx_regex
in include/bmx.h, not from the C code: the grammar restated in Python, the Glushkov sets, a matcher that carries position
sets, the answers in numpy for large texts, a translation to Python's ``re`` and a brute force over it that is independent
of all of these, the fixed-length variants of an expression, and the word-level recurrence of csrc/bmx_regex_kernel.h.

An automaton is an ``Rx``: ``member`` is a boolean array [m, 256] (member[i][b] = "byte value b belongs to the class of
position i"; classes_oracle.pack / unpack go to and from the library's layout), ``first`` and ``last`` are ints used as bit
sets, ``follow`` is a list of m such ints, ``min_len`` / ``max_len`` are the shortest and the longest match.
"""
import re

import numpy as np

import classes_oracle as co
from classes_oracle import ExprError

ICASE, IUPAC = 1, 2
MAX_M = 64
MAX_DEPTH = 32


class Rx:
    def __init__(self, member, first, last, follow):
        self.member = np.asarray(member, bool).reshape(-1, 256)
        self.m = len(self.member)
        self.first, self.last, self.follow = int(first), int(last), [int(f) for f in follow]
        self.min_len, self.max_len = lengths(self.m, self.first, self.last, self.follow)


def bits(x):
    """The set bits of x, ascending."""
    i = 0
    while x:
        if x & 1:
            yield i
        x >>= 1
        i += 1


def lengths(m, first, last, follow):
    """(shortest, longest) path from ``first`` to ``last`` in positions; (0, 0) where there is none."""
    lo, hi = [0] * m, [0] * m
    for i in range(m):
        if (first >> i) & 1:
            lo[i], hi[i] = 1, max(hi[i], 1)
        if hi[i]:
            for j in bits(follow[i]):
                lo[j] = lo[i] + 1 if lo[j] == 0 else min(lo[j], lo[i] + 1)
                hi[j] = max(hi[j], hi[i] + 1)
    ends = [i for i in bits(last) if hi[i]]
    return (min(lo[i] for i in ends), max(hi[i] for i in ends)) if ends else (0, 0)


# ---- the grammar ----------------------------------------------------------------------------------------------------
# A tree node is ("elem", row), ("cat", [nodes]), ("alt", [nodes]) or ("rep", node, a, b).

def _number(toks, at):
    j = at
    while j < len(toks) and not toks[j][1] and 48 <= toks[j][0] <= 57:
        j += 1
    if j == at:
        raise ExprError("a number is due")
    return int(bytes(v for v, _ in toks[at:j])), j


def _op(toks, at, chars):
    return at < len(toks) and not toks[at][1] and toks[at][0] in chars


def _element(toks, at, flags):
    """One element of the class grammar at toks[at] -> (row, next index)."""
    v, lit = toks[at]
    at += 1
    negated = False
    row = np.zeros(256, dtype=bool)
    if not lit and v == ord("."):
        row[:] = True
    elif not lit and v == ord("["):
        if _op(toks, at, b"^"):
            negated = True
            at += 1
        close = next((j for j in range(at + 1, len(toks)) if toks[j] == (ord("]"), False)), None)
        if close is None:
            raise ExprError("unterminated set")
        row = co._set_row(toks[at:close])
        at = close + 1
    elif not lit and flags & IUPAC and chr(v) in co.IUPAC_SETS:
        row[[ord(b) for b in co.IUPAC_SETS[chr(v)]]] = True
    else:
        row[v] = True
    if flags & ICASE:
        for lo in range(97, 123):
            row[lo] = row[lo - 32] = row[lo] or row[lo - 32]
    return (~row if negated else row), at


def _repeat(toks, at, flags, depth):
    if _op(toks, at, b"*+"):
        raise ExprError("unbounded repetition is out of scope")
    if _op(toks, at, b"?{"):
        raise ExprError("a quantifier with nothing in front of it")
    if _op(toks, at, b"("):
        if depth + 1 > MAX_DEPTH:
            raise ExprError("nesting deeper than 32")
        node, at = _alt(toks, at + 1, flags, depth + 1)
        if not _op(toks, at, b")"):
            raise ExprError("unbalanced (")
        at += 1
    else:
        row, at = _element(toks, at, flags)
        node = ("elem", row)
    a = b = 1
    if _op(toks, at, b"?"):
        a, at = 0, at + 1
    elif _op(toks, at, b"{"):
        a, at = _number(toks, at + 1)
        b = a
        if _op(toks, at, b","):
            if _op(toks, at + 1, b"}"):
                raise ExprError("{a,}: unbounded repetition is out of scope")
            b, at = _number(toks, at + 1)
        if not _op(toks, at, b"}"):
            raise ExprError("unterminated {...}")
        at += 1
        if b < 1 or a > b:
            raise ExprError("b == 0 or a > b")
    else:
        if _op(toks, at, b"*+"):
            raise ExprError("unbounded repetition is out of scope")
        return node, at
    if _op(toks, at, b"?{*+"):
        raise ExprError("a quantifier right after another quantifier")
    return ("rep", node, a, b), at


def _alt(toks, at, flags, depth):
    alts = []
    while True:
        cat = []
        while at < len(toks) and not _op(toks, at, b"|)"):
            node, at = _repeat(toks, at, flags, depth)
            cat.append(node)
        alts.append(("cat", cat))
        if not _op(toks, at, b"|"):
            return ("alt", alts), at
        at += 1


def tree(expr, flags: int = 0):
    e = expr.encode("latin-1") if isinstance(expr, str) else bytes(expr)
    if flags & ~(ICASE | IUPAC):
        raise ExprError("an unknown flag bit")
    toks = co._tokens(e)
    node, at = _alt(toks, 0, flags, 0)
    if at < len(toks):
        raise ExprError("unbalanced )")
    return node


def _has_element(node):
    if node[0] == "elem":
        return True
    if node[0] == "rep":
        return _has_element(node[1])
    return any(_has_element(k) for k in node[1])


class _Glushkov:
    """The standard recursion: (nullable, first, last) of every subtree, follow as a side effect."""

    def __init__(self):
        self.rows, self.follow = [], []

    def cat(self, f, g):
        for i in bits(f[2]):
            self.follow[i] |= g[1]
        return (f[0] and g[0], f[1] | (g[1] if f[0] else 0), g[2] | (f[2] if g[0] else 0))

    def walk(self, node):
        if not _has_element(node):
            return (True, 0, 0)  # the empty string, whatever its counts
        kind = node[0]
        if kind == "elem":
            if len(self.rows) >= MAX_M:
                raise ExprError("more than 64 positions")
            self.rows.append(node[1])
            self.follow.append(0)
            bit = 1 << (len(self.rows) - 1)
            return (False, bit, bit)
        if kind == "cat":
            f = (True, 0, 0)
            for k in node[1]:
                f = self.cat(f, self.walk(k))
            return f
        if kind == "alt":
            parts = [self.walk(k) for k in node[1]]
            return (any(p[0] for p in parts), sum(p[1] for p in parts), sum(p[2] for p in parts))
        _, sub, a, b = node
        f = (True, 0, 0)
        for i in range(b):
            g = self.walk(sub)
            f = self.cat(f, (g[0] or i >= a, g[1], g[2]))
        return f


def parse(expr, flags: int = 0) -> Rx:
    """The grammar of bmx_compile_regex -> Rx; raises ExprError where the library returns BMX_ERR_ARG."""
    g = _Glushkov()
    nullable, first, last = g.walk(tree(expr, flags))
    if not g.rows:
        raise ExprError("zero positions")
    if nullable:
        raise ExprError("matches the empty string")
    return Rx(np.array(g.rows), first, last, g.follow)


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
    if not _has_element(sub):
        return b""  # (re refuses to repeat what cannot consume a byte; it is the empty string)
    return b"(?:" + _re_text(sub) + b"){%d,%d}" % (a, b)


def to_re(expr, flags: int = 0):
    """The expression in Python's syntax: bytes, DOTALL, every group non-capturing, every class spelt out."""
    return re.compile(_re_text(tree(expr, flags)), re.DOTALL)


def ends_brute(text, expr, flags: int = 0):
    """The definition: for every end j, every start s, re.fullmatch of the substring.  Returns (ends, shortest-match
    starts, longest-match starts) as lists.  For tiny inputs."""
    rx = to_re(expr, flags)
    text = bytes(text)
    ends, short, long_ = [], [], []
    for j in range(len(text)):
        ok = [s for s in range(j + 1) if rx.fullmatch(text[s:j + 1])]
        if ok:
            ends.append(j)
            short.append(ok[-1])
            long_.append(ok[0])
    return ends, short, long_


# ---- the automaton's answers ----------------------------------------------------------------------------------------

def match_ends(text, rx: Rx):
    """The matcher that carries position sets: per byte the positions that have just consumed it on some path from
    ``first``.  Returns (ends, shortest-match starts, longest-match starts) as lists."""
    short_len, long_len = {}, {}  # position -> shortest / longest path that ends in it on the current byte
    ends, short, long_ = [], [], []
    for j, c in enumerate(bytes(text)):
        ns, nl = {}, {}
        for i in range(rx.m):
            if not rx.member[i][c]:
                continue
            cand_s = [1] if (rx.first >> i) & 1 else []
            cand_l = list(cand_s)
            for p in short_len:
                if (rx.follow[p] >> i) & 1:
                    cand_s.append(short_len[p] + 1)
                    cand_l.append(long_len[p] + 1)
            if cand_s:
                ns[i], nl[i] = min(cand_s), max(cand_l)
        short_len, long_len = ns, nl
        fin = [i for i in short_len if (rx.last >> i) & 1]
        if fin:
            ends.append(j)
            short.append(j - min(short_len[i] for i in fin) + 1)
            long_.append(j - max(long_len[i] for i in fin) + 1)
    return ends, short, long_


def _preds(rx: Rx):
    return [[p for p in range(i) if (rx.follow[p] >> i) & 1] for i in range(rx.m)]


def ends_numpy(text, rx: Rx) -> np.ndarray:
    """Every end, ascending (int64), for texts of MiB size: one boolean array per position ("position i consumed byte j
    on some path"), filled in ascending position order from the shifted arrays of its predecessors."""
    t = np.frombuffer(bytes(text), np.uint8)
    act = []
    hit = np.zeros(t.size, bool)
    for i, preds in enumerate(_preds(rx)):
        reach = np.full(t.size, bool((rx.first >> i) & 1))
        for p in preds:
            reach[1:] |= act[p][:-1]
        act.append(reach & rx.member[i][t])
        if (rx.last >> i) & 1:
            hit |= act[i]
    return np.nonzero(hit)[0].astype(np.int64)


def starts_numpy(text, rx: Rx, longest: bool = False):
    """(ends, starts): for every end the largest start (the shortest match), or with ``longest`` the smallest one.  One
    array of path lengths per position, 0 = not active."""
    t = np.frombuffer(bytes(text), np.uint8)
    pick = np.maximum if longest else (lambda a, b: np.where(a == 0, b, np.where(b == 0, a, np.minimum(a, b))))
    lens = []
    best = np.zeros(t.size, np.int32)
    for i, preds in enumerate(_preds(rx)):
        cur = np.full(t.size, 1 if (rx.first >> i) & 1 else 0, np.int32)
        for p in preds:
            step = np.zeros(t.size, np.int32)
            step[1:] = np.where(lens[p][:-1] > 0, lens[p][:-1] + 1, 0)
            cur = pick(cur, step)
        cur[~rx.member[i][t]] = 0
        lens.append(cur)
        if (rx.last >> i) & 1:
            best = pick(best, cur)
    ends = np.nonzero(best)[0].astype(np.int64)
    return ends, ends - best[ends] + 1


def paths(rx: Rx, limit: int = 64):
    """Every path from ``first`` to ``last`` as a list of positions; ValueError beyond ``limit`` of them."""
    out = []

    def go(path):
        if (rx.last >> path[-1]) & 1:
            out.append(list(path))
            if len(out) > limit:
                raise ValueError("too many paths")
        for j in bits(rx.follow[path[-1]]):
            go(path + [j])

    for i in bits(rx.first):
        go([i])
    return out


def variants(rx: Rx, limit: int = 64):
    """Every path as a fixed-length class pattern, each once (a list of member arrays)."""
    seen, out = set(), []
    for p in paths(rx, limit):
        v = rx.member[p]
        key = (len(p), v.tobytes())
        if key not in seen:
            seen.add(key)
            out.append(v)
    return out


def variant_ends(text, rx: Rx) -> np.ndarray:
    """The union of starts + length - 1 over the variants."""
    lists = [co.class_starts(text, v) + (len(v) - 1) for v in variants(rx)]
    return np.unique(np.concatenate(lists)) if lists else np.zeros(0, np.int64)


def plant(rng, text, variant, at):
    """Overwrite text (uint8 array) from ``at`` on with an instance of a variant; a position with an empty class ends the
    copy.  Returns the index behind the copy."""
    for row in variant:
        vals = np.nonzero(row)[0]
        if vals.size == 0 or at >= text.size:
            break
        text[at] = rng.choice(vals)
        at += 1
    return at


def plant_path(rng, text, rx: Rx, at):
    """Overwrite text from ``at`` on with an instance of a random path from ``first`` to ``last`` (for automata with more
    paths than variants() lists).  Returns the index behind the copy."""
    alive = [i for i in range(rx.m) if rx.member[i].any()]
    can_end = set()
    for i in reversed(alive):  # positions from which `last` can be reached over non-empty classes
        if (rx.last >> i) & 1 or any(j in can_end for j in bits(rx.follow[i])):
            can_end.add(i)
    here = [i for i in bits(rx.first) if i in can_end]
    while here and at < text.size:
        i = int(rng.choice(here))
        text[at] = rng.choice(np.nonzero(rx.member[i])[0])
        at += 1
        here = [j for j in bits(rx.follow[i]) if j in can_end]
        if (rx.last >> i) & 1 and (not here or rng.integers(0, 2)):
            break
    return at


# ---- random expressions ---------------------------------------------------------------------------------------------

def _rand_element(rng, symbols):
    r = int(rng.integers(0, 10))
    if r == 0:
        return "."
    if r < 4 and len(symbols) > 1:
        pick = sorted(set(int(x) for x in rng.choice(symbols, int(rng.integers(1, 4)))))
        body = "".join("\\x%02x" % v for v in pick)
        return ("[^" if r == 1 else "[") + body + "]"
    return "\\x%02x" % int(rng.choice(symbols))


def _rand_quant(rng):
    r = int(rng.integers(0, 10))
    if r < 5:
        return ""
    if r < 7:
        return "?"
    if r == 7:
        return "{%d}" % int(rng.integers(1, 4))
    a = int(rng.integers(0, 3))
    return "{%d,%d}" % (a, max(1, a + int(rng.integers(0, 3))))


def _rand_concat(rng, symbols, depth):
    parts = []
    for _ in range(int(rng.integers(1, 4))):
        if depth < 3 and rng.integers(0, 3) == 0:
            alts = [_rand_concat(rng, symbols, depth + 1) for _ in range(int(rng.integers(1, 4)))]
            if rng.integers(0, 6) == 0:
                alts.insert(int(rng.integers(0, len(alts) + 1)), "")  # an empty alternative
            atom = "(" + "|".join(alts) + ")"
        else:
            atom = _rand_element(rng, symbols)
        parts.append(atom + _rand_quant(rng))
    return "".join(parts)


def random_regex(rng, symbols, max_m=8):
    """(expression str, Rx) over the byte values ``symbols``: elements, sets, groups, alternation (now and then with an
    empty alternative), ? {a} {a,b} on elements and on groups.  Nullable expressions and those over max_m positions are
    rejected and drawn again."""
    symbols = np.asarray(symbols)
    while True:
        alts = [_rand_concat(rng, symbols, 0) for _ in range(1 if rng.integers(0, 4) else 2)]
        expr = "|".join(alts)
        try:
            rx = parse(expr)
        except ExprError:
            continue
        if rx.m <= max_m:
            return expr, rx


# ---- the recurrence of csrc/bmx_regex_kernel.h, word by word -------------------------------------------------------

def split(rx: Rx):
    """(lin, nl): the positions i with follow[i] == {i + 1}, and the other positions with a successor."""
    lin = sum(1 << i for i in range(rx.m) if rx.follow[i] == 1 << (i + 1))
    nl = sum(1 << i for i in range(rx.m) if rx.follow[i] and rx.follow[i] != 1 << (i + 1))
    return lin, nl


def tables(rx: Rx, nbytes: int):
    """T_b[v] for b in range(nbytes): the OR of follow[8b + t] over the bits t of v."""
    f = rx.follow + [0] * (8 * nbytes - rx.m)
    T = []
    for b in range(nbytes):
        row = []
        for v in range(256):
            x = 0
            for t in bits(v):
                x |= f[8 * b + t]
            row.append(x)
        T.append(row)
    return T


def word_ends(text, rx: Rx, width: int):
    """D = (first | Follow(D)) & B[c], Follow(D) = ((D & lin) << 1) | OR_b T_b[byte b of (D & nl)], in a word of ``width``
    bits (32: m <= 32; 64), as the kernel runs it: bit i = position i, a hit iff (D & last) != 0."""
    assert rx.m <= width
    full = (1 << width) - 1
    lin, nl = split(rx)
    T = tables(rx, width // 8)
    active = [b for b in range(width // 8) if (nl >> (8 * b)) & 0xFF]
    B = [sum(1 << i for i in range(rx.m) if rx.member[i][c]) for c in range(256)]
    D, ends = 0, []
    for j, c in enumerate(bytes(text)):
        F = ((D & lin) << 1) & full
        x = D & nl
        for b in active:
            F |= T[b][(x >> (8 * b)) & 0xFF]
        D = (rx.first | F) & B[c]
        if D & rx.last:
            ends.append(j)
    return np.array(ends, np.int64)


def reverse(rx: Rx) -> Rx:
    """The reversed automaton: position i becomes m - 1 - i, first and last swap, follow is transposed."""
    m = rx.m

    def flip(s):
        return sum(1 << (m - 1 - i) for i in bits(s))

    follow = [0] * m
    for i in range(m):
        for j in bits(rx.follow[i]):
            follow[m - 1 - j] |= 1 << (m - 1 - i)
    return Rx(rx.member[::-1], flip(rx.last), flip(rx.first), follow)
