"""Test helper for the anchored regular-expression search (bmx_compile_regex_anchored, bmx_search_regex_anchored*), written
from the model in include/bmx.h, not from the C code.  Two checkers that share nothing:

1. the automaton's answer: a ``Rx`` of regex_oracle plus one boolean row ``before[i]`` / ``after[i]`` per position and the two
   neighbour bytes of the view, in numpy (one array per position, as regex_oracle.ends_numpy) -- forward and, through the
   reversed automaton on the reversed text, the begins side;
2. Python's ``re`` on bytes with re.MULTILINE: for end j the expression followed by a look-ahead that pins the end, matched
   from every start with ``pos`` so that the context on both sides stays visible.
"""
import re

import numpy as np

import classes_oracle as co
import regex_oracle as ro

WORD, LINE = 4, 8
NL = 10
W = np.zeros(256, bool)
W[[c for c in range(256) if chr(c).isascii() and (chr(c).isalnum() or c == 95)]] = True


class Anchored:
    """rx: regex_oracle.Rx; before, after: bool [m, 256] (read where the position is in first / last)."""

    def __init__(self, rx, before, after):
        self.rx = rx
        self.before = np.asarray(before, bool).reshape(-1, 256)[: rx.m]
        self.after = np.asarray(after, bool).reshape(-1, 256)[: rx.m]


def from_lib(re_, an) -> Anchored:
    """The library's two structs (host.Regex, host.RegexAnchors) as an Anchored."""
    m = re_.m
    rx = ro.Rx(co.unpack(re_.class_array()), re_.first, re_.last, list(re_.follow)[:m])
    return Anchored(rx, co.unpack(an.before_array()[:m]), co.unpack(an.after_array()[:m]))


def full(rx) -> Anchored:
    return Anchored(rx, np.ones((rx.m, 256), bool), np.ones((rx.m, 256), bool))


def reverse(a: Anchored) -> Anchored:
    """The mirror image: the reversed automaton, before and after swapped and mirrored."""
    return Anchored(ro.reverse(a.rx), a.after[::-1], a.before[::-1])


def spans_numpy(text, a: Anchored, left: int = NL, right: int = NL, longest: bool = False):
    """(ends, starts) int64: every end of an anchored match of the view ``text`` with the neighbour bytes left / right, and
    for each the largest start, or with ``longest`` the smallest.  One array of path lengths per position (0 = inactive)."""
    rx = a.rx
    t = np.frombuffer(bytes(text), np.uint8)
    n = t.size
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    prev = np.concatenate(([left], t[:-1])).astype(np.uint8)
    nxt = np.concatenate((t[1:], [right])).astype(np.uint8)
    pick = np.maximum if longest else (lambda x, y: np.where(x == 0, y, np.where(y == 0, x, np.minimum(x, y))))
    lens = []
    best = np.zeros(n, np.int32)
    preds = [[p for p in range(i) if (rx.follow[p] >> i) & 1] for i in range(rx.m)]
    for i in range(rx.m):
        cur = np.zeros(n, np.int32)
        if (rx.first >> i) & 1:
            cur = a.before[i][prev].astype(np.int32)
        for p in preds[i]:
            step = np.zeros(n, np.int32)
            step[1:] = np.where(lens[p][:-1] > 0, lens[p][:-1] + 1, 0)
            cur = pick(cur, step)
        cur = np.where(rx.member[i][t], cur, 0).astype(np.int32)
        lens.append(cur)
        if (rx.last >> i) & 1:
            best = pick(best, np.where(a.after[i][nxt], cur, 0).astype(np.int32))
    ends = np.nonzero(best)[0].astype(np.int64)
    return ends, ends - best[ends] + 1


def begins_numpy(text, a: Anchored, left: int = NL, right: int = NL, longest: bool = False):
    """(starts, ends) int64: every start of an anchored match, ascending, and for each the smallest end, or with
    ``longest`` the largest."""
    t = bytes(text)[::-1]
    n = len(t)
    e, s = spans_numpy(t, reverse(a), right, left, longest)
    return (n - 1 - e)[::-1].astype(np.int64), (n - 1 - s)[::-1].astype(np.int64)


def simulate(text, a: Anchored, left: int = NL, right: int = NL):
    """The definition, position sets with their starts carried along: {(s, j)} of every anchored match.  Tiny inputs."""
    rx = a.rx
    t = bytes(text)
    out = set()
    active = {}  # position -> set of starts, after the current byte
    for j, c in enumerate(t):
        p_byte = t[j - 1] if j else left
        n_byte = t[j + 1] if j + 1 < len(t) else right
        new = {}
        for i in range(rx.m):
            if not rx.member[i][c]:
                continue
            starts = set()
            if (rx.first >> i) & 1 and a.before[i][p_byte]:
                starts.add(j)
            for p, ss in active.items():
                if (rx.follow[p] >> i) & 1:
                    starts |= ss
            if starts:
                new[i] = starts
        active = new
        for i, ss in active.items():
            if (rx.last >> i) & 1 and a.after[i][n_byte]:
                out |= {(s, j) for s in ss}
    return out


# ---- Python's re ----------------------------------------------------------------------------------------------------

def to_python(expr) -> bytes:
    """The expression in Python's syntax: \\< and \\> spelt with \\b and a look-around, everything else as it stands (sets and
    escapes are copied unread)."""
    e = expr.encode("latin-1") if isinstance(expr, str) else bytes(expr)
    out = bytearray()
    i = 0
    while i < len(e):
        c = e[i:i + 1]
        if c == b"\\":
            two = e[i:i + 2]
            if two == b"\\<":
                out += b"\\b(?=\\w)"
            elif two == b"\\>":
                out += b"\\b(?<=\\w)"
            elif two == b"\\x":
                out += e[i:i + 4]
                i += 2
            else:
                out += two
            i += 2
        elif c == b"[":
            j = i + 1
            if e[j:j + 1] == b"^":
                j += 1
            j += 1  # (the first member may be ])
            while e[j:j + 1] != b"]":
                j += 2 if e[j:j + 1] == b"\\" else 1
            out += e[i:j + 1]
            i = j + 1
        else:
            out += c
            i += 1
    return bytes(out)


def matches_re(text, expr, flags: int = 0, left: int = NL, right: int = NL):
    """{(s, j)} of every anchored match by Python's re: the view between its two neighbour bytes, for every end j the
    expression with a look-ahead that leaves exactly the bytes behind j, from every start with ``pos``.  flags: WORD / LINE
    as grep -w / -x (a look-behind and a look-ahead around the expression)."""
    body = b"(?:" + to_python(expr) + b")"
    if flags & WORD:
        body = b"(?<!\\w)" + body + b"(?!\\w)"
    if flags & LINE:
        body = b"(?<=\\n)" + body + b"(?=\\n)"
    t = bytes(text)
    whole = bytes([left]) + t + bytes([right])
    out = set()
    for j in range(len(t)):
        rest = len(t) - 1 - j + 1  # the bytes of `whole` behind j
        pat = re.compile(body + b"(?=(?s:.{%d})\\Z)" % rest, re.MULTILINE | re.DOTALL)
        for s in range(j + 1):
            if pat.match(whole, s + 1):
                out.add((s, j))
    return out


def lists_of(matches):
    """{(s, j)} -> (ends, largest start of each, smallest start of each, starts, smallest end of each, largest end of each)."""
    by_end, by_start = {}, {}
    for s, j in matches:
        by_end.setdefault(j, []).append(s)
        by_start.setdefault(s, []).append(j)
    ends = sorted(by_end)
    starts = sorted(by_start)
    return (ends, [max(by_end[j]) for j in ends], [min(by_end[j]) for j in ends],
            starts, [min(by_start[s]) for s in starts], [max(by_start[s]) for s in starts])
