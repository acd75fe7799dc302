"""Test helper: the text index (bmx_index_*) in numpy and plain Python, no GPU.

The suffix array the library builds keeps the reference's "past the end ranks as character 96" rule (oracle/sa_oracle.c),
so it is not the memcmp order outside lower-case text.  For a text that does not end in two or more bytes 96 it is the
sorted order of these strings, one per suffix i (include/bmx.h, the text-index section):

    text[i..n) compared as signed char,
    then, if n - 1 - i is even, ONE virtual symbol strictly between byte 95 and byte 96,
    then "nothing", which is below everything.

model_key writes that string as a tuple of integers: a byte is twice its signed value, the virtual symbol is the odd
number between twice 95 and twice 96, and "nothing" is the end of the tuple (a proper prefix is below every extension).
"""
import bisect
from typing import List, Sequence, Tuple

import numpy as np

VIRTUAL = 2 * 95 + 1
ABOVE_ALL = 1 << 20

# the alphabets of the issue: lower case, the neighbours of byte 96, bytes >= 0x80 and capitals, printable
ALPHABETS = {
    "ab": b"ab",
    "_`aA": b"_`aA",
    "a`\\x80Z": b"a`\x80Z",
    "printable": bytes(range(32, 127)),
}


def _signed2(b: int) -> int:
    return 2 * (b - 256 if b >= 128 else b)


def as_bytes(text) -> bytes:
    if isinstance(text, str):
        return text.encode("latin-1")
    if isinstance(text, np.ndarray):
        return text.astype(np.uint8).tobytes()
    return bytes(text)


def model_key(text: bytes, i: int) -> Tuple[int, ...]:
    n = len(text)
    tail = (VIRTUAL,) if (n - 1 - i) % 2 == 0 else ()
    return tuple(_signed2(b) for b in text[i:]) + tail


def model_order(text) -> np.ndarray:
    """The suffix array by the comparator above (for texts that do not end in two or more bytes 96)."""
    t = as_bytes(text)
    return np.array(sorted(range(len(t)), key=lambda i: model_key(t, i)), dtype=np.int32)


def occurrences(text, pat) -> np.ndarray:
    """Every p with p + m <= n and text[p..p+m) == pat, ascending, by brute force."""
    t, p = as_bytes(text), as_bytes(pat)
    out, at = [], t.find(p)
    while at >= 0 and p:
        out.append(at)
        at = t.find(p, at + 1)
    return np.array(out, dtype=np.int64)


def suffix_keys(text, sa: Sequence[int]) -> List[Tuple[int, ...]]:
    """The comparator's string of every suffix, in the order of `sa` (sa_range takes them, for many queries on one text)."""
    t = as_bytes(text)
    return [model_key(t, int(i)) for i in sa]


def sa_range(text, sa: Sequence[int], pat, keys=None) -> Tuple[int, int]:
    """(lo, cnt): binary search of pat over the array `sa` of `text` with the comparator above.  sa[lo : lo + cnt] are the
    suffixes that begin with pat; with cnt == 0, lo is the insertion point."""
    p = as_bytes(pat)
    if keys is None:
        keys = suffix_keys(text, sa)
    pk = tuple(_signed2(b) for b in p)
    lo = bisect.bisect_left(keys, pk)
    hi = bisect.bisect_left(keys, pk + (ABOVE_ALL,))  # above every suffix that begins with pat, below every larger one
    return lo, hi - lo


def random_text(rng, n: int, alphabet: bytes) -> bytes:
    """n random bytes over the alphabet; a text that would end in two bytes 96 gets another last byte (no case is skipped)."""
    t = bytearray(alphabet[int(j)] for j in rng.integers(0, len(alphabet), n))
    if n >= 2 and t[-1] == 96 and t[-2] == 96:
        t[-1] = next(b for b in alphabet if b != 96)
    return bytes(t)


def all_queries(alphabet: bytes, max_len: int) -> List[bytes]:
    """Every string of 1..max_len bytes over the alphabet's bytes below 0x80."""
    letters = [bytes([b]) for b in alphabet if b < 0x80]
    out, level = [], [b""]
    for _ in range(max_len):
        level = [x + c for x in level for c in letters]
        out += level
    return out
