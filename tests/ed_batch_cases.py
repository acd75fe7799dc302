"""Case generators for the batched edit distance (bmx_edit_distance_batch*), shared by tests/test_ed_batch_cpu.py (the
cases and their expected values, without a GPU) and tests/test_gpu_ed_batch.py (the kernels against them).  Expected
values come from the oracle's port, pair by pair; nothing here calls the library under test."""
from typing import List, Optional, Sequence, Tuple

import numpy as np

ALPHABETS = (2, 4, 95, 256)
BATCH_WORD = 64  # a pair with BOTH sides longer than this takes the pair-by-pair path
MAX_FALLBACK_PAIRS = 64  # every such pair costs a launch: no case holds more of them than this

GRID_LA = (0, 1, 31, 32, 33, 63, 64, 65)
GRID_LB = (0, 1, 2, 31, 32, 33, 63, 64, 65, 200, 5000)
QUERY_LENGTHS = (0, 1, 32, 33, 64, 65, 300)
LIMITS = (0, 1, 3, 1000, None)  # None = ED_NO_LIMIT


def rand_string(rng, n: int, alpha: int) -> bytes:
    """n bytes over `alpha` symbols: 0/1.., ACGT, printable-95 or every byte value."""
    v = rng.integers(0, alpha, n)
    if alpha == 4:
        return np.frombuffer(b"ACGT", np.uint8)[v].tobytes()
    if alpha == 95:
        return (v + 0x20).astype(np.uint8).tobytes()
    return v.astype(np.uint8).tobytes()


def edited(rng, s: bytes, k: int, alpha: int, max_len: int) -> bytes:
    """s after k random substitutions, insertions and deletions, never longer than max_len."""
    t = bytearray(s)
    for _ in range(k):
        op = int(rng.integers(0, 3))
        if op == 1 and len(t) >= max_len:
            op = 2
        if op != 1 and not t:
            op = 1 if max_len > 0 else -1
        if op == 0:
            t[int(rng.integers(0, len(t)))] = rand_string(rng, 1, alpha)[0]
        elif op == 1:
            t.insert(int(rng.integers(0, len(t) + 1)), rand_string(rng, 1, alpha)[0])
        elif op == 2:
            del t[int(rng.integers(0, len(t)))]
    return bytes(t)


def random_pairs(n: int = 20000, seed: int = 0xED8A, max_len: int = 80) -> Tuple[List[bytes], List[bytes]]:
    """n pairs, lengths 0..max_len per side, the four alphabets in turn; every second group of four has b = a after 0..8
    edits.  Only the first MAX_FALLBACK_PAIRS pairs that come out with both sides over BATCH_WORD stay so; a later one has
    one side (a and b in turn) cut to 0..BATCH_WORD bytes: the cap on such pairs is a condition of these tests."""
    rng = np.random.default_rng(seed)
    a, b = [], []
    long_left = MAX_FALLBACK_PAIRS
    for i in range(n):
        alpha = ALPHABETS[i % 4]
        x = rand_string(rng, int(rng.integers(0, max_len + 1)), alpha)
        if (i // 4) % 2 == 0:
            y = edited(rng, x, int(rng.integers(0, 9)), alpha, max_len)
        else:
            y = rand_string(rng, int(rng.integers(0, max_len + 1)), alpha)
        if min(len(x), len(y)) > BATCH_WORD:
            if long_left > 0:
                long_left -= 1
            elif i % 2 == 0:
                x = x[:int(rng.integers(0, BATCH_WORD + 1))]
            else:
                y = y[:int(rng.integers(0, BATCH_WORD + 1))]
        a.append(x)
        b.append(y)
    return a, b


def grid_pairs(seed: int = 0x6A1D) -> Tuple[List[bytes], List[bytes]]:
    """The full grid GRID_LA x GRID_LB three times: unrelated ACGT strings, strings with no common byte, and b = a's
    prefix or a extended (identical where the lengths agree).  9 of the pairs have both sides over BATCH_WORD."""
    rng = np.random.default_rng(seed)
    a, b = [], []
    for la in GRID_LA:
        for lb in GRID_LB:
            a.append(rand_string(rng, la, 4))
            b.append(rand_string(rng, lb, 4))
            a.append(rand_string(rng, la, 2))  # bytes 0 and 1
            b.append(rand_string(rng, lb, 95))  # bytes 0x20..0x7e
            x = rand_string(rng, max(la, lb), 256)
            a.append(x[:la])
            b.append(x[:lb])
    return a, b


def one_vs_many(qlen: int, n: int = 10000, seed: int = 0x0111) -> Tuple[bytes, List[bytes]]:
    """A query of qlen bytes and n candidates of 0..80 bytes, printable-95; every second candidate is a piece of the query
    after 0..8 edits.  With a query over BATCH_WORD bytes a candidate over BATCH_WORD bytes is a pair-by-pair pair, so
    there only the first MAX_FALLBACK_PAIRS // 2 candidates with an odd index may be that long (the others stop at
    BATCH_WORD): the cap on such pairs is a condition of these tests."""
    rng = np.random.default_rng(seed + qlen)
    q = rand_string(rng, qlen, 95)
    out = []
    long_left = MAX_FALLBACK_PAIRS // 2
    for i in range(n):
        top = 80
        if qlen > BATCH_WORD:
            if i % 2 == 1 and long_left > 0:
                long_left -= 1
                out.append(rand_string(rng, int(rng.integers(BATCH_WORD + 1, 81)), 95))
                continue
            top = BATCH_WORD
        if i % 2 == 0:
            lo = int(rng.integers(0, qlen + 1))
            piece = q[lo:lo + int(rng.integers(0, top + 1))]
            out.append(edited(rng, piece, int(rng.integers(0, 9)), 95, top))
        else:
            out.append(rand_string(rng, int(rng.integers(0, top + 1)), 95))
    return q, out


def long_pairs(seed: int = 0x10F6) -> Tuple[List[bytes], List[bytes]]:
    """A few pairs for the pair-by-pair path and the long-walk bound: both sides long and related (a few edits apart), a
    short side against 65,536 and against 65,537 bytes, mixed with ordinary short pairs."""
    rng = np.random.default_rng(seed)
    a, b = [], []
    for la, k in ((65, 3), (100, 0), (700, 9), (5000, 20), (65536, 12)):
        x = rand_string(rng, la, 4)
        a.append(x)
        b.append(edited(rng, x, k, 4, la + k))
        a.append(rand_string(rng, 10, 4))
        b.append(rand_string(rng, 12, 4))
    x = rand_string(rng, 65537, 95)
    a += [x[100:140], x[:65536], x[200:264]]
    b += [x[:65536], x[300:333], x]  # the last one: a longer side over the bound
    return a, b


def n_fallback(a: Sequence[bytes], b: Sequence[bytes], long_bound: Optional[int] = None) -> int:
    """Pairs with both sides over BATCH_WORD (and, with long_bound, those whose longer side exceeds it) that need their
    bytes at all."""
    n = 0
    for x, y in zip(a, b):
        lo, hi = min(len(x), len(y)), max(len(x), len(y))
        if lo > BATCH_WORD or (long_bound is not None and lo > 0 and hi > long_bound):
            n += 1
    return n


def expected(port, a: Sequence[bytes], b: Sequence[bytes]) -> np.ndarray:
    """port.edit_distance per pair; for long related strings port.edit_distance_within (same value, a band of cells)."""
    out = np.empty(len(b), dtype=np.uint32)
    for i, y in enumerate(b):
        x = a[i] if len(a) == len(b) else a[0]
        d = None
        if min(len(x), len(y)) > 2000:
            d = port.edit_distance_within(x, y, 64 + abs(len(x) - len(y)))
        out[i] = port.edit_distance(x, y) if d is None else d
    return out


def clamp(d: np.ndarray, limit: Optional[int]) -> np.ndarray:
    """What a call with `limit` returns: min(distance, limit + 1)."""
    return d if limit is None else np.minimum(d, np.uint32(limit + 1))
