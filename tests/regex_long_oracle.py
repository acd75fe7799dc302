"""Test helper for the regular-expression search of up to 128 positions (bmx_compile_regex_long, bmx_search_regex_long*),
written from the description of struct bmx_regex_long in include/bmx.h, not from the C code.  The grammar, the tree, the
matcher that carries position sets, the numpy answers, the translation to Python's ``re`` and the brute force are
regex_oracle's: they work on Python integers of any width.  This module lifts that module's limit of 64 positions without
touching its globals (a subclass of its Glushkov walker) and adds the word-level recurrence of
csrc/bmx_regex_long_kernel.h: a state of four dwords, the shift carried from dword to dword, the follow tables compacted.
"""
import numpy as np

import regex_oracle as ro
from regex_oracle import ExprError, Rx  # noqa: F401

MAX_M = 128
MASK32 = 0xFFFFFFFF


class _Glushkov128(ro._Glushkov):
    """regex_oracle's recursion with the limit at 128 positions."""

    def walk(self, node):
        if node[0] == "elem":
            if len(self.rows) >= MAX_M:
                raise ExprError("more than 128 positions")
            self.rows.append(node[1])
            self.follow.append(0)
            bit = 1 << (len(self.rows) - 1)
            return (False, bit, bit)
        return super().walk(node)


def parse(expr, flags: int = 0) -> Rx:
    """The grammar of bmx_compile_regex_long -> Rx; raises ExprError where the library returns BMX_ERR_ARG."""
    g = _Glushkov128()
    nullable, first, last = g.walk(ro.tree(expr, flags))
    if not g.rows:
        raise ExprError("zero positions")
    if nullable:
        raise ExprError("matches the empty string")
    return Rx(np.array(g.rows), first, last, g.follow)


def positions(expr, flags: int = 0) -> int:
    """The positions the expression expands to, without a limit (0 where it has none or does not parse)."""
    def count(node):
        if node[0] == "elem":
            return 1
        if node[0] == "rep":
            return node[3] * count(node[1]) if ro._has_element(node[1]) else 0
        return sum(count(k) for k in node[1])

    try:
        return count(ro.tree(expr, flags))
    except ExprError:
        return 0


def random_regex(rng, symbols, min_m: int, max_m: int = MAX_M, bar: float = 1 / 6):
    """(expression str, Rx) with min_m..max_m positions: regex_oracle's random pieces, concatenated or (with probability
    ``bar``) joined by | until the expression is long enough; counted repeats of a piece now and then.  A high ``bar``
    keeps the shortest match short, so that a tiny text has matches."""
    symbols = np.asarray(symbols)
    while True:
        target = int(rng.integers(min_m, max_m + 1))
        expr, m = "", 0
        while m < target:
            piece = ro._rand_concat(rng, symbols, 0)
            r = int(rng.integers(0, 8))
            if r == 0:
                piece = "(" + piece + "){%d,%d}" % (int(rng.integers(0, 3)), int(rng.integers(2, 6)))
            elif r == 1:
                piece = ro._rand_element(rng, symbols) + "{%d,%d}" % (int(rng.integers(0, 4)), int(rng.integers(4, 24)))
            cand = piece if not expr else expr + ("|" if rng.random() < bar else "") + piece
            cm = positions(cand)
            if cm == 0 or cm > max_m:
                break
            expr, m = cand, cm
        if not (min_m <= m <= max_m):
            continue
        try:
            rx = parse(expr)
        except ExprError:
            continue
        if min_m <= rx.m <= max_m:
            return expr, rx


# ---- struct bmx_regex_long <-> Rx ------------------------------------------------------------------------------------

def words(s: int):
    """A set as the struct's two words."""
    return [s & (2**64 - 1), s >> 64]


def dwords(s: int):
    return [(s >> (32 * q)) & MASK32 for q in range(4)]


# ---- the recurrence of csrc/bmx_regex_long_kernel.h, dword by dword --------------------------------------------------

def _shift1(d):
    """(d << 1) over four dwords: every dword takes the top bit of the one below it."""
    return [(d[0] << 1) & MASK32] + [((d[q] << 1) | (d[q - 1] >> 31)) & MASK32 for q in (1, 2, 3)]


def word_ends(text, rx: Rx):
    """D = (first | Follow(D)) & B[c], Follow(D) = ((D & lin) << 1 over 128 bits) | OR_b T_b[byte b of (D & nl)] on four
    dwords, the tables in slots popcount(nl_bytes below b); a hit iff (D & last) != 0.  Returns (ends, table slots)."""
    assert rx.m <= MAX_M
    lin, nl = ro.split(rx)
    nl_bytes = sum(1 << b for b in range(16) if (nl >> (8 * b)) & 0xFF)
    T = ro.tables(rx, 16)
    slots = [dwt for b, dwt in enumerate(T) if (nl_bytes >> b) & 1]  # compacted
    slot_of = {b: bin(nl_bytes & ((1 << b) - 1)).count("1") for b in range(16) if (nl_bytes >> b) & 1}
    B = [dwords(sum(1 << i for i in range(rx.m) if rx.member[i][c])) for c in range(256)]
    first, last, lin4, nl4 = dwords(rx.first), dwords(rx.last), dwords(lin), dwords(nl)
    D, ends = [0, 0, 0, 0], []
    for j, c in enumerate(bytes(text)):
        F = _shift1([D[q] & lin4[q] for q in range(4)])
        x = [D[q] & nl4[q] for q in range(4)]
        if any(x):
            for b, slot in slot_of.items():
                w = dwords(slots[slot][(x[b >> 2] >> (8 * (b & 3))) & 0xFF])
                F = [F[q] | w[q] for q in range(4)]
        D = [(first[q] | F[q]) & B[c][q] for q in range(4)]
        if any(D[q] & last[q] for q in range(4)):
            ends.append(j)
    return np.array(ends, np.int64), len(slots)
