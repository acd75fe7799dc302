"""Test helper for the class-pattern search: the answers in numpy, independent of Shift-And, and the expression grammar
restated in Python from its description in include/bmx.h.

A pattern is ``member``: a boolean array [m, 256], member[i][b] = "byte value b belongs to class i".  ``pack`` / ``unpack``
go to and from the library's layout (uint8 [m, 32]: bit (b & 7) of byte (b >> 3)).
"""
import numpy as np

ICASE, IUPAC = 1, 2
IUPAC_SETS = {"R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC", "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG",
              "N": "ACGT"}


def pack(member) -> np.ndarray:
    member = np.asarray(member, dtype=bool).reshape(-1, 256)
    return np.packbits(member, axis=1, bitorder="little")


def unpack(classes) -> np.ndarray:
    return np.unpackbits(np.asarray(classes, dtype=np.uint8).reshape(-1, 32), axis=1, bitorder="little").astype(bool)


def singletons(pat: bytes) -> np.ndarray:
    member = np.zeros((len(pat), 256), dtype=bool)
    member[np.arange(len(pat)), np.frombuffer(bytes(pat), np.uint8)] = True
    return member


def class_starts(text: bytes, member) -> np.ndarray:
    """Every start p with text[p + i] in class i for all i, ascending (int64)."""
    t = np.frombuffer(bytes(text), np.uint8)
    member = np.asarray(member, dtype=bool)
    m = member.shape[0]
    if t.size < m:
        return np.zeros(0, np.int64)
    ok = np.ones(t.size - m + 1, dtype=bool)
    for i in range(m):
        ok &= member[i][t[i:t.size - m + 1 + i]]
    return np.nonzero(ok)[0].astype(np.int64)


def class_approx_ends(text: bytes, member, k: int):
    """(ends int64, distances int64): Sellers' programme row by row (as tests/approx_oracle.py), a mismatch being "the
    text byte is not in class i"."""
    t = np.frombuffer(bytes(text), np.uint8)
    member = np.asarray(member, dtype=bool)
    idx = np.arange(t.size + 1, dtype=np.int64)
    prev = np.zeros(t.size + 1, np.int64)  # row 0: free start
    for i in range(1, member.shape[0] + 1):
        e = np.empty(t.size + 1, np.int64)
        e[0] = i
        e[1:] = np.minimum(prev[:-1] + ~member[i - 1][t], prev[1:] + 1)  # diagonal / vertical
        prev = np.minimum.accumulate(e - idx) + idx  # horizontal = running min
    d = prev[1:]
    ends = np.nonzero(d <= k)[0]
    return ends, d[ends]


def class_starts_brute(text: bytes, member) -> list:
    m = len(member)
    return [p for p in range(len(text) - m + 1) if all(member[i][text[p + i]] for i in range(m))]


def class_edit_distance(member, s: bytes) -> int:
    """Levenshtein distance between the class pattern and the string s (a substitution is free where the byte belongs)."""
    prev = list(range(len(s) + 1))
    for i in range(1, len(member) + 1):
        cur = [i] + [0] * len(s)
        for j in range(1, len(s) + 1):
            cur[j] = min(prev[j - 1] + (not member[i - 1][s[j - 1]]), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return prev[len(s)]


def class_approx_ends_brute(text: bytes, member, k: int):
    """The definition itself: for every end j the minimum over all starts s <= j + 1."""
    ends, dists = [], []
    for j in range(len(text)):
        best = min(class_edit_distance(member, text[s:j + 1]) for s in range(j + 2))
        if best <= k:
            ends.append(j)
            dists.append(best)
    return np.array(ends, np.int64), np.array(dists, np.int64)


class ExprError(ValueError):
    pass


def _tokens(e: bytes):
    """Pass 1: escapes resolved.  A token is (byte value, literal?): an escaped byte is a literal everywhere, an unescaped
    one may be an operator (. [ ] ^ -) or, outside sets, an IUPAC letter."""
    toks = []
    it = iter(range(len(e)))
    for i in it:
        if e[i] != 0x5C:
            toks.append((e[i], False))
            continue
        if i + 1 >= len(e):
            raise ExprError("dangling backslash")
        if e[i + 1] != ord("x"):
            toks.append((e[i + 1], True))
            next(it)
            continue
        try:
            digits = e[i + 2:i + 4].decode("ascii")
        except UnicodeDecodeError:
            raise ExprError("bad hex")
        if len(digits) != 2 or not all(d in "0123456789abcdefABCDEF" for d in digits):
            raise ExprError("bad hex")
        toks.append((int(digits, 16), True))
        for _ in range(3):
            next(it)
    return toks


def _set_row(body):
    """The tokens between [ and ] (negation stripped): items, and ranges item - item where a - has an item on both sides."""
    row = np.zeros(256, dtype=bool)
    values = [v for v, _ in body]
    dash = [(v == ord("-") and not lit) for v, lit in body]
    used = [False] * len(body)
    for j in range(1, len(body) - 1):  # left to right: a - between two unused items makes a range
        if dash[j] and not used[j - 1] and not used[j] and not used[j + 1]:
            if values[j + 1] < values[j - 1]:
                raise ExprError("reversed range")
            row[values[j - 1]:values[j + 1] + 1] = True
            used[j - 1] = used[j] = used[j + 1] = True
    for j, v in enumerate(values):
        if not used[j]:
            row[v] = True
    return row


def parse(expr, flags: int = 0) -> np.ndarray:
    """The grammar of bmx_compile_classes -> member [m, 256]; raises ExprError where the library returns BMX_ERR_ARG."""
    e = expr.encode("latin-1") if isinstance(expr, str) else bytes(expr)
    toks = _tokens(e)
    rows = []
    at = 0
    while at < len(toks):
        v, lit = toks[at]
        at += 1
        negated = False
        row = np.zeros(256, dtype=bool)
        if not lit and v == ord("."):
            row[:] = True
        elif not lit and v == ord("["):
            if at < len(toks) and toks[at] == (ord("^"), False):
                negated = True
                at += 1
            # the closing bracket: the first unescaped ] that is not directly behind [ or [^
            close = next((j for j in range(at + 1, len(toks)) if toks[j] == (ord("]"), False)), None)
            if close is None:
                raise ExprError("unterminated set")
            row = _set_row(toks[at:close])
            at = close + 1
        elif not lit and flags & IUPAC and chr(v) in IUPAC_SETS:
            row[[ord(b) for b in IUPAC_SETS[chr(v)]]] = True
        else:
            row[v] = True
        if flags & ICASE:
            for lo in range(97, 123):
                row[lo] = row[lo - 32] = row[lo] or row[lo - 32]
        rows.append(~row if negated else row)
    if not rows or len(rows) > 64:
        raise ExprError("zero elements or more than 64")
    return np.array(rows)
