"""Test helper for the gapped pattern search: the grammar of bmx_compile_gaps restated in Python from its description in
include/bmx.h (both syntaxes), the answers in numpy without Shift-And, a brute force over a regular expression that is
independent of both, the fixed-length variants of a pattern, and the recurrence of csrc/bmx_gaps_kernel.h word by word.

A pattern is (``member``, ``optional``): member is a boolean array [M, 256], member[i][b] = "byte value b belongs to
class i" (classes_oracle.pack / unpack go to and from the library's layout), and bit i of the int ``optional`` says that
position i may be skipped.
"""
import itertools
import re

import numpy as np

import classes_oracle as co
from classes_oracle import ExprError

ICASE, IUPAC, PROSITE = 1, 2, 4
MAX_M = 64


def _fold(row):
    for lo in range(97, 123):
        row[lo] = row[lo - 32] = row[lo] or row[lo - 32]


def _digits(toks, at):
    """Unescaped decimal digits from toks[at] on -> (value, next index); at least one."""
    j = at
    while j < len(toks) and not toks[j][1] and 48 <= toks[j][0] <= 57:
        j += 1
    if j == at:
        raise ExprError("a number is due")
    return int(bytes(v for v, _ in toks[at:j])), j


def _counts(toks, at, close):
    """Behind the opening bracket: n or a,b and the closing byte -> (a, b, next index)."""
    a, at = _digits(toks, at)
    b = a
    if at < len(toks) and toks[at] == (ord(","), False):
        b, at = _digits(toks, at + 1)
    if at >= len(toks) or toks[at] != (close, False):
        raise ExprError("unterminated repetition")
    if b < 1 or a > b:
        raise ExprError("b == 0 or a > b")
    return a, b, at + 1


def _finish(rows, opts):
    if not rows or len(rows) > MAX_M:
        raise ExprError("zero positions or more than 64")
    if all(opts):
        raise ExprError("no mandatory position")
    return np.array(rows), sum(1 << i for i, o in enumerate(opts) if o)


def _parse_default(e: bytes, flags: int):
    toks = co._tokens(e)
    rows, opts = [], []
    at = 0
    while at < len(toks):
        v, lit = toks[at]
        if not lit and v in b"?{*+":
            raise ExprError("a quantifier without an element, or unbounded repetition")
        at += 1
        negated = False
        row = np.zeros(256, dtype=bool)
        if not lit and v == ord("."):
            row[:] = True
        elif not lit and v == ord("["):
            if at < len(toks) and toks[at] == (ord("^"), False):
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
            _fold(row)
        if negated:
            row = ~row
        a = b = 1
        if at < len(toks) and toks[at] == (ord("?"), False):
            a, at = 0, at + 1
        elif at < len(toks) and toks[at] == (ord("{"), False):
            a, b, at = _counts(toks, at + 1, ord("}"))
        if len(rows) + b > MAX_M:
            raise ExprError("more than 64 positions")
        rows += [row] * b
        opts += [False] * a + [True] * (b - a)
    return _finish(rows, opts)


def _parse_prosite(e: bytes, flags: int):
    if flags & IUPAC:
        raise ExprError("PROSITE with IUPAC")
    if e.endswith(b"."):
        e = e[:-1]
    toks = [(v, False) for v in e]  # no escapes in this syntax
    rows, opts = [], []
    at = 0
    while True:
        if at >= len(e):
            raise ExprError("an element is due")
        c = e[at]
        at += 1
        row = np.zeros(256, dtype=bool)
        if c == ord("x"):
            row[:] = True
        elif c in b"[{":
            close = e.find(b"]" if c == ord("[") else b"}", at)
            if close < 0 or close == at:
                raise ExprError("unterminated or empty set")
            body = e[at:close]
            if b"<" in body or b">" in body:
                raise ExprError("anchor")
            row[list(body)] = True
            if flags & ICASE:
                _fold(row)
            if c == ord("{"):
                row = ~row
            at = close + 1
        elif c in b"-]}()<>.,":
            raise ExprError("a syntax byte where an element is due")
        else:
            row[c] = True
        if c not in b"[{" and flags & ICASE:
            _fold(row)
        a = b = 1
        if at < len(e) and e[at] == ord("("):
            a, b, at = _counts(toks, at + 1, ord(")"))
        if len(rows) + b > MAX_M:
            raise ExprError("more than 64 positions")
        rows += [row] * b
        opts += [False] * a + [True] * (b - a)
        if at == len(e):
            return _finish(rows, opts)
        if e[at] != ord("-"):
            raise ExprError("a separator is due")
        at += 1


def parse(expr, flags: int = 0):
    """The grammar of bmx_compile_gaps -> (member [M, 256], optional); raises ExprError where the library returns
    BMX_ERR_ARG."""
    e = expr.encode("latin-1") if isinstance(expr, str) else bytes(expr)
    if flags & ~(ICASE | IUPAC | PROSITE):
        raise ExprError("an unknown flag bit")
    return _parse_prosite(e, flags) if flags & PROSITE else _parse_default(e, flags)


def _opt_list(member, optional):
    return [bool((optional >> i) & 1) for i in range(len(member))]


def _reach(text, member, optional, pick, none):
    """The programme behind the three answers.  State of row i at prefix length p: the best length (by ``pick``) of a
    text[s:p] that is spelt by a choice of positions from 0..i holding every mandatory one of them, or ``none``."""
    t = np.frombuffer(bytes(text), np.uint8)
    prev = np.zeros(t.size + 1, np.int64)  # no position yet: the empty string, anywhere
    for i, opt in enumerate(_opt_list(member, optional)):
        cur = np.full(t.size + 1, none, np.int64)
        take = member[i][t] & (prev[:-1] != none)
        cur[1:][take] = prev[:-1][take] + 1
        if opt:
            skip = prev != none
            both = skip & (cur != none)
            cur[skip & ~both] = prev[skip & ~both]
            cur[both] = pick(cur[both], prev[both])
        prev = cur
    return prev[1:]  # by end index j


def gap_ends(text, member, optional) -> np.ndarray:
    """Every end j at which some text[s..j] matches, ascending (int64): closed position sets carried along, O(M n)."""
    return np.nonzero(_reach(text, np.asarray(member, bool), optional, np.minimum, -1) != -1)[0].astype(np.int64)


def gap_starts(text, member, optional, longest: bool = False):
    """(ends, starts): for every end the largest start (the shortest match), or with ``longest`` the smallest one."""
    best = _reach(text, np.asarray(member, bool), optional, np.maximum if longest else np.minimum, -1)
    ends = np.nonzero(best != -1)[0].astype(np.int64)
    return ends, ends - best[ends] + 1


def _regex(member, optional):
    parts = []
    for row, opt in zip(np.asarray(member, bool), _opt_list(member, optional)):
        vals = np.nonzero(row)[0]
        cls = b"[" + b"".join(b"\\x%02x" % v for v in vals) + b"]" if vals.size else b"(?:(?!))"
        parts.append(cls + (b"?" if opt else b""))
    return re.compile(b"".join(parts) + b"\\Z", re.S)


def gap_ends_brute(text, member, optional):
    """The definition: for every end j, every start s, a regular expression anchored at both sides.  Returns (ends,
    shortest starts, longest starts) as lists."""
    rx = _regex(member, optional)
    text = bytes(text)
    ends, short, long_ = [], [], []
    for j in range(len(text)):
        ok = [s for s in range(j + 1) if rx.match(text[s:j + 1])]
        if ok:
            ends.append(j)
            short.append(ok[-1])
            long_.append(ok[0])
    return ends, short, long_


def variants(member, optional):
    """The fixed-length class patterns that the choices of optional positions give, each once (a list of member arrays)."""
    member = np.asarray(member, bool)
    opts = [i for i, o in enumerate(_opt_list(member, optional)) if o]
    seen, out = set(), []
    for keep in itertools.product((False, True), repeat=len(opts)):
        dropped = {i for i, k in zip(opts, keep) if not k}
        v = member[[i for i in range(len(member)) if i not in dropped]]
        key = v.tobytes()
        if key not in seen:
            seen.add(key)
            out.append(v)
    return out


def variant_ends(text, member, optional) -> np.ndarray:
    """The second identity of include/bmx.h: the union of starts + length - 1 over the variants."""
    lists = [co.class_starts(text, v) + (len(v) - 1) for v in variants(member, optional)]
    return np.unique(np.concatenate(lists)) if lists else np.zeros(0, np.int64)


def random_pattern(rng, symbols, max_m=7):
    """(member, optional) over the byte values ``symbols``: wildcards, small sets, now and then an empty class, runs of
    optional positions anywhere (the first and the last position included), at least one mandatory."""
    m = int(rng.integers(1, max_m + 1))
    member = np.zeros((m, 256), dtype=bool)
    for i in range(m):
        r = int(rng.integers(0, 16))
        if r == 0 and m > 1:
            continue  # an empty class
        if r < 5:
            member[i][symbols] = True
        else:
            member[i][rng.choice(symbols, int(rng.integers(1, 3)))] = True
    optional = 0
    for i in range(m):
        if rng.integers(0, 5) < 2:
            optional |= 1 << i
    if optional == (1 << m) - 1:
        optional &= ~(1 << int(rng.integers(0, m)))
    return member, optional


def plant(rng, text, member, optional, at, keep=None):
    """Overwrite text from ``at`` on with an instance of the pattern: every mandatory position, an optional one where
    ``keep`` (a set of positions; None: a coin per position) holds it.  A position with an empty class ends the copy.
    Returns the index behind the copy."""
    for i in range(len(member)):
        if (optional >> i) & 1 and (rng.integers(0, 2) if keep is None else i not in keep):
            continue
        vals = np.nonzero(member[i])[0]
        if vals.size == 0 or at >= text.size:
            break
        text[at] = rng.choice(vals)
        at += 1
    return at


def masks(optional: int, m: int, bits: int):
    """O, I, F, S of the recurrence as csrc/bmx_gaps_kernel.h defines them, shifted up so that bit m - 1 is the top bit
    of a word of ``bits`` bits."""
    opt = [bool((optional >> i) & 1) for i in range(m)]
    O = I = F = 0
    for i in range(m):
        if not opt[i]:
            continue
        O |= 1 << i
        if i == 0 or not opt[i - 1]:
            I |= 1 << max(i - 1, 0)
        if i == m - 1 or not opt[i + 1]:
            F |= 1 << i
    b = opt.index(False)
    S = (1 << (b + 1)) - 1
    up = bits - m
    return O << up, I << up, F << up, S << up


def word_ends(text, member, optional, bits: int):
    """The recurrence word by word, in a word of ``bits`` bits (32: M <= 32; 64), as the kernel runs it."""
    member = np.asarray(member, bool)
    m = len(member)
    assert m <= bits
    up, full = bits - m, (1 << bits) - 1
    O, I, F, S = masks(optional, m, bits)
    B = [sum(1 << (i + up) for i in range(m) if member[i][c]) for c in range(256)]
    D, ends = 0, []
    for j, c in enumerate(bytes(text)):
        D = (((D << 1) | S) & B[c]) & full
        Df = D | F
        D |= O & ~(((Df - I) & full) ^ Df) & full
        if D >> (bits - 1):
            ends.append(j)
    return np.array(ends, np.int64)
