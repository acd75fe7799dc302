"""Test helper: the capture model of bmx_compile_regex_groups restated in Python from its description in include/bmx.h
(the expression tree, the expansion of counted repeats into copies, the depth-first order over the epsilon moves, the
tags, the walker).  Nothing here calls the library; the tests compare the two.

    tables(expr)            -> (n_groups, pref [65][64], open [65][65], close [65][65]) as numpy arrays, or raises Refused
    walk(model, text, s, e) -> ((begin, end), ...) for groups 0..n_groups of the span text[s..e], None where it is no match
                               (model: Model.from_library(re, gr))
    py_regs(expr, text, s, e) -> what Python's re returns as fullmatch(text, s, e + 1).regs (bytes, DOTALL), or None
"""
from __future__ import annotations

import re as pyre

import numpy as np

START = END = 64
MAX_GROUPS = 16


# 64 positions and 16 groups: 16 groups of four positions each, alternatives and optional parts among them ...
WIDE = "".join("(a[bc]?c|.)" if i % 2 else "([ab](?:c|a)a?)" for i in range(16))
WIDE_PIECES = (["ac", "ba", "aca", "baa", "bc", "aa"], ["ac", "abc", "acc", "x", "a", "c"])  # ... what the even and the odd ones match


def wide_text(rng) -> bytes:
    """A text that WIDE matches as a whole, 16..42 bytes."""
    return "".join(WIDE_PIECES[i % 2][int(rng.integers(0, 6))] for i in range(16)).encode()


class Refused(ValueError):
    pass


# ---- the tree ----
# ("elem",) | ("cat", [kids]) | ("alt", [kids]) | ("rep", a, b, kid) | ("group", g, kid)

def _skip_escape(e: bytes, p: int) -> int:
    if p >= len(e):
        raise Refused("a dangling backslash")
    if e[p] != ord("x"):
        return p + 1
    if len(e) - (p + 1) < 2:
        raise Refused("bad hex")
    return p + 3


def _element_end(e: bytes, at: int) -> int:
    c = e[at]
    if c == ord("\\"):
        return _skip_escape(e, at + 1)
    if c != ord("["):
        return at + 1
    p = at + 1
    if p < len(e) and e[p] == ord("^"):
        p += 1
    first = True
    while p < len(e):
        x = e[p]
        p += 1
        if x == ord("]") and not first:
            return p
        first = False
        if x == ord("\\"):
            p = _skip_escape(e, p)
        if p + 1 < len(e) and e[p] == ord("-") and e[p + 1] != ord("]"):
            p += 1
            x = e[p]
            p += 1
            if x == ord("\\"):
                p = _skip_escape(e, p)
    raise Refused("an unterminated set")


class _Parser:
    def __init__(self, expr: bytes):
        self.e = expr
        self.at = 0
        self.n_groups = 0

    def number(self):
        p = self.at
        while self.at < len(self.e) and chr(self.e[self.at]).isdigit():
            self.at += 1
        if p == self.at:
            raise Refused("a malformed {...}")
        return int(self.e[p:self.at])

    def repeat(self):
        e = self.e
        c = chr(e[self.at])
        if c in "?{*+":
            raise Refused("a quantifier with nothing in front of it, or unbounded repetition")
        if c == "(":
            self.at += 1
            g = 0
            if self.at < len(e) and e[self.at] == ord("?"):
                if e[self.at + 1:self.at + 2] != b":":
                    raise Refused("(? followed by anything but :")
                self.at += 2
            else:
                if self.n_groups == MAX_GROUPS:
                    raise Refused("more than 16 capturing groups")
                self.n_groups += 1
                g = self.n_groups
            atom = self.alt()
            if self.at >= len(e) or e[self.at] != ord(")"):
                raise Refused("an unbalanced (")
            self.at += 1
            if g:
                atom = ("group", g, atom)
        else:
            self.at = _element_end(e, self.at)
            atom = ("elem",)
        if self.at >= len(e):
            return atom
        c = chr(e[self.at])
        if c == "?":
            a, b = 0, 1
            self.at += 1
        elif c == "{":
            self.at += 1
            a = b = self.number()
            if self.at < len(e) and e[self.at] == ord(","):
                self.at += 1
                b = self.number()
            if self.at >= len(e) or e[self.at] != ord("}"):
                raise Refused("a malformed {...}")
            self.at += 1
            if b < 1 or a > b:
                raise Refused("{a,b} needs 0 <= a <= b and b >= 1")
        elif c in "*+":
            raise Refused("unbounded repetition")
        else:
            return atom
        if self.at < len(e) and chr(e[self.at]) in "?{*+":
            raise Refused("a quantifier right after another quantifier")
        return ("rep", a, b, atom)

    def alt(self):
        alts = []
        while True:
            cat = []
            while self.at < len(self.e) and chr(self.e[self.at]) not in "|)":
                cat.append(self.repeat())
            alts.append(("cat", cat))
            if self.at >= len(self.e) or self.e[self.at] != ord("|"):
                break
            self.at += 1
        return ("alt", alts)


def parse(expr) -> tuple:
    """(tree, n_groups) of an expression in bmx_compile_regex_groups' grammar."""
    e = expr.encode("latin-1") if isinstance(expr, str) else bytes(expr)
    p = _Parser(e)
    tree = p.alt()
    if p.at < len(e):
        raise Refused("an unbalanced )")
    return tree, p.n_groups


def _empty(t) -> bool:  # can the subtree match the empty string?
    k = t[0]
    if k == "elem":
        return False
    if k == "cat":
        return all(_empty(x) for x in t[1])
    if k == "alt":
        return any(_empty(x) for x in t[1])
    if k == "rep":
        return t[1] == 0 or _empty(t[3])
    return _empty(t[2])


def _has(t, what) -> bool:
    k = t[0]
    if k == what:
        return True
    if k in ("cat", "alt"):
        return any(_has(x, what) for x in t[1])
    if k == "rep":
        return _has(t[3], what)
    if k == "group":
        return _has(t[2], what)
    return False


def _check_repeats(t):
    k = t[0]
    if k == "rep":
        if t[2] >= 2 and _empty(t[3]) and _has(t[3], "group"):
            raise Refused("a repeat of two or more whose body can match the empty string and holds a capturing group")
        _check_repeats(t[3])
    elif k in ("cat", "alt"):
        for x in t[1]:
            _check_repeats(x)
    elif k == "group":
        _check_repeats(t[2])


# ---- the expanded tree as states with ordered epsilon moves ----

class _Nfa:
    def __init__(self):
        self.pos = []    # state -> position it consumes, or -1
        self.next = []   # ... and the state behind it
        self.moves = []  # state -> [(to, open, close)] in the order a backtracking matcher tries them
        self.n_pos = 0

    def state(self):
        self.pos.append(-1)
        self.next.append(-1)
        self.moves.append([])
        return len(self.pos) - 1

    def thread(self, t, cur):
        k = t[0]
        if not _has(t, "elem") and not _has(t, "group"):
            return cur
        if k == "elem":
            c, out = self.state(), self.state()
            self.pos[c], self.next[c] = self.n_pos, out
            self.n_pos += 1
            self.moves[cur].append((c, 0, 0))
            return out
        if k == "group":
            bit = 1 << (t[1] - 1)
            kin = self.state()
            self.moves[cur].append((kin, bit, 0))
            kout = self.thread(t[2], kin)
            out = self.state()
            self.moves[kout].append((out, 0, bit))
            return out
        if k == "cat":
            for x in t[1]:
                cur = self.thread(x, cur)
            return cur
        if k == "alt":
            out = self.state()
            for x in t[1]:
                kin = self.state()
                self.moves[cur].append((kin, 0, 0))
                self.moves[self.thread(x, kin)].append((out, 0, 0))
            return out
        _, a, b, kid = t
        copies = b if _has(kid, "elem") else 1
        for i in range(copies):
            if i < a:
                cur = self.thread(kid, cur)
                continue
            kin, after = self.state(), self.state()
            self.moves[cur].append((kin, 0, 0))  # the optional copy before its skip
            self.moves[self.thread(kid, kin)].append((after, 0, 0))
            self.moves[cur].append((after, 0, 0))
            cur = after
        return cur


def tables(expr):
    """(n_groups, pref, open, close) of the expression, by the header's rules; Refused where the library must refuse for a
    reason of the capture model (syntax errors of the elements are the class compiler's and are not restated here)."""
    tree, n_groups = parse(expr)
    _check_repeats(tree)
    nfa = _Nfa()
    start = nfa.state()
    final = nfa.thread(tree, start)
    if nfa.n_pos > 64:
        raise Refused("more than 64 positions")
    if nfa.n_pos == 0 or _empty(tree):
        raise Refused("matches the empty string")
    pref = np.full((65, 64), 0xFF, dtype=np.uint8)
    op = np.zeros((65, 65), dtype=np.uint16)
    cl = np.zeros((65, 65), dtype=np.uint16)
    behind = {START: start}
    for s, p in enumerate(nfa.pos):
        if p >= 0:
            behind[p] = nfa.next[s]
    for row, s0 in behind.items():
        seen = set()
        rank = 0
        stack = [(s0, 0, 0)]
        while stack:  # depth first, the moves of a state in their order
            s, o, c = stack.pop()
            if s in seen:
                continue
            seen.add(s)
            q = nfa.pos[s] if nfa.pos[s] >= 0 else END if s == final else -1
            if q >= 0:
                if q != END:
                    pref[row, rank] = q
                    rank += 1
                op[row, q], cl[row, q] = o, c
                continue
            for to, mo, mc in reversed(nfa.moves[s]):
                stack.append((to, o | mo, c | mc))
    return n_groups, pref, op, cl


# ---- the walker ----

class Model:
    """What the walker reads: the automaton (first, last, follow, class membership) and the three tables."""

    def __init__(self, m, first, last, follow, member, n_groups, pref, op, cl):
        self.m, self.first, self.last, self.follow, self.member = m, first, last, follow, member
        self.n_groups, self.pref, self.open, self.close = n_groups, pref, op, cl

    @classmethod
    def from_library(cls, re_, gr):
        classes = np.frombuffer(bytes(re_.classes), dtype=np.uint8).reshape(64, 32)
        member = [[bool((classes[q, c >> 3] >> (c & 7)) & 1) for c in range(256)] for q in range(re_.m)]
        return cls(re_.m, int(re_.first), int(re_.last), [int(re_.follow[i]) for i in range(re_.m)], member, gr.n_groups,
                   gr.pref_array(), gr.open_array(), gr.close_array())


def walk(model: Model, text: bytes, s: int, e: int):
    L = e - s + 1
    m = model.m
    B = [0] * L  # B[t]: the positions that consume text[s + t] and can still reach `last` at e
    for t in range(L - 1, -1, -1):
        c = text[s + t]
        for q in range(m):
            if model.member[q][c] and ((model.last >> q) & 1 if t == L - 1 else model.follow[q] & B[t + 1]):
                B[t] |= 1 << q
    if not (B[0] & model.first):
        return None
    begin = [-1] * (model.n_groups + 1)
    end = [-1] * (model.n_groups + 1)
    begin[0], end[0] = s, e + 1
    cur = START
    for t in range(L + 1):
        nxt = END
        if t < L:
            nxt = next(int(q) for q in model.pref[cur] if q != 0xFF and (B[t] >> int(q)) & 1)
        o, c = int(model.open[cur, nxt]), int(model.close[cur, nxt])
        for g in range(1, model.n_groups + 1):
            if (o >> (g - 1)) & 1:
                begin[g] = s + t
            if (c >> (g - 1)) & 1:
                end[g] = s + t
        cur = nxt
    return tuple((b, x) if b >= 0 and x >= 0 else (-1, -1) for b, x in zip(begin, end))


def py_regs(expr, text: bytes, s: int, e: int):
    e_ = expr.encode("latin-1") if isinstance(expr, str) else bytes(expr)
    mt = pyre.compile(e_, pyre.DOTALL).fullmatch(text, s, e + 1)
    return None if mt is None else tuple(mt.regs)


# ---- random expressions over {a, b, c} ----

def random_expr(rng, depth: int = 0) -> str:
    """alternation, ?, {a,b}, nesting, capturing and non-capturing groups; may be one the library refuses."""
    def atom(d):
        r = rng.random()
        if d >= 3 or r < 0.45:
            return ["a", "b", "c", "[ab]", "[bc]", "."][int(rng.integers(0, 6))]
        inner = alt(d + 1)
        return ("(" if rng.random() < 0.7 else "(?:") + inner + ")"

    def rep(d):
        x = atom(d)
        r = rng.random()
        if r < 0.25:
            return x + "?"
        if r < 0.40:
            a = int(rng.integers(0, 3))
            b = a + int(rng.integers(0, 3))
            if b == 0:
                b = 1
            return x + ("{%d}" % a if a == b else "{%d,%d}" % (a, b))
        return x

    def cat(d):
        return "".join(rep(d) for _ in range(int(rng.integers(1 if d else 1, 4))))

    def alt(d):
        parts = [cat(d) for _ in range(1 + (rng.random() < 0.35) + (rng.random() < 0.1))]
        if d and rng.random() < 0.08:
            parts.append("")
        return "|".join(parts)

    return alt(depth)
