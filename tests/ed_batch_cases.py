"""Case generators for the batched edit distance (bmx_edit_distance_batch*), shared by tests/test_ed_batch_cpu.py (the
cases and their expected values, without a GPU) and tests/test_gpu_ed_batch.py (the kernels against them).  Expected
values come from the oracle's port, pair by pair; nothing here calls the library under test.  kernel_paths is a model
of the kernel's dispatch (which pair takes which path, on which word, with which pattern load), written from the header:
the CPU suite applies it to the generators that aim at one path each, so that a generator that misses its target fails
there and not as silence on the GPU."""
from typing import List, Optional, Sequence, Tuple

import numpy as np

ALPHABETS = (2, 4, 95, 256)
BATCH_WORD = 64  # a pair with BOTH sides longer than this takes the pair-by-pair path
BATCH_LONG = 65536  # a pairwise pair with a longer side over this takes it too
MAX_FALLBACK_PAIRS = 64  # every such pair costs a launch: no case holds more of them than this (but growth_pairs)
WAVE = 64  # consecutive pairs that share the choice of the word
# kernel_paths: what the kernel does with a pair
OFFSETS, LISTED = "answered from offsets", "listed"
PAIR32, PAIR64, SHARED32, SHARED64 = "pairwise 32", "pairwise 64", "shared 32", "shared 64"

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


def kernel_paths(la: Sequence[int], lb: Sequence[int], one: bool = False, limit: Optional[int] = None,
                 a_bytes: Optional[int] = None, b_bytes: Optional[int] = None) -> List[Tuple[str, bool]]:
    """What bmx_edit_distance_batch_device does with every pair of a call, written from csrc/bmx_ed_batch_kernel.h and
    DESIGN.md s12 and not by calling the library: per pair (path, byte_path), path one of OFFSETS, LISTED, PAIR32, PAIR64,
    SHARED32, SHARED64, and byte_path whether ed_batch_load_pattern takes the pattern's last chunk byte by byte.

    la, lb: the lengths of the strings, which lie back to back from byte 0 of their blobs (host.pack_strings); with
    `one` la holds the query's length alone.  a_bytes, b_bytes: the blob sizes the call states (the packed size if None).
    The rules: lane i owns pair i and a wave is 64 consecutive pairs; a pair with a length difference over the limit or
    an empty side is answered from its offsets; one against many with a query of 1..BATCH_WORD bytes walks every other
    pair against the shared Peq; a pair with both sides over BATCH_WORD bytes or a longer side over BATCH_LONG is listed;
    every other pair walks with its shorter string (a on a tie) as the bit vector.  A wave runs the 64-bit word if any
    of its walking lanes has a bit vector of more than 32 bytes.  Chunk c of a pattern of m bytes at P is read if
    16c < m, and byte by byte if P + 16c + 16 > the end of its blob."""
    count = len(lb)
    one = one and count != 1  # (the host: a single pair is the same either way)
    la = [int(la[0])] * count if one else [int(x) for x in la]
    assert len(la) == count
    lb = [int(y) for y in lb]
    a_off = [0] * (count + 1) if one else np.concatenate(([0], np.cumsum(la, dtype=np.int64))).tolist()
    b_off = np.concatenate(([0], np.cumsum(lb, dtype=np.int64))).tolist()
    a_bytes = (la[0] if one and count else a_off[-1]) if a_bytes is None else a_bytes
    b_bytes = b_off[-1] if b_bytes is None else b_bytes
    assert a_bytes >= (la[0] if one and count else a_off[-1]) and b_bytes >= b_off[-1]
    shared = one and 1 <= la[0] <= BATCH_WORD
    kind, lane = [], []  # lane: None, or (m, distance from the pattern's start to its blob's end; None with the Peq)
    for i in range(count):
        lo, hi = min(la[i], lb[i]), max(la[i], lb[i])
        assert hi < 1 << 31
        if (limit is not None and hi - lo > limit) or lo == 0:
            kind.append(OFFSETS), lane.append(None)
        elif shared:
            kind.append("shared"), lane.append((la[i], None))
        elif lo > BATCH_WORD or hi > BATCH_LONG:
            kind.append(LISTED), lane.append(None)
        else:
            to_end = a_bytes - a_off[i] if la[i] <= lb[i] else b_bytes - b_off[i]
            kind.append("pairwise"), lane.append((lo, to_end))
    out = []
    for w in range(0, count, WAVE):
        wide = any(l is not None and l[0] > 32 for l in lane[w:w + WAVE])
        for k, l in zip(kind[w:w + WAVE], lane[w:w + WAVE]):
            if l is None:
                out.append((k, False))
            elif l[1] is None:
                out.append((SHARED64 if wide else SHARED32, False))
            else:
                m, to_end = l
                chunks = 4 if wide else 2
                by_byte = [c for c in range(chunks) if 16 * c < m and 16 * c + 16 > to_end]
                assert all(c == (m - 1) // 16 for c in by_byte)  # only a pattern's last chunk can come byte by byte
                out.append((PAIR64 if wide else PAIR32, bool(by_byte)))
    return out


def lengths(strings: Sequence[bytes]) -> List[int]:
    return [len(s) for s in strings]


def _relative(rng, p: bytes, n: int, alpha: int) -> bytes:
    """A string of exactly n >= 1 bytes: p after 0..8 edits, cut or filled up with random symbols."""
    t = edited(rng, p, int(rng.integers(0, 9)), alpha, n)
    return t[:n] + rand_string(rng, n - min(n, len(t)), alpha)


def word_column(seed: int = 0x30C1) -> Tuple[List[bytes], List[bytes]]:
    """Pairs for the two words of the pairwise kernel, a as the bit vector (the shorter string) in the first half of every
    (alphabet, m) group and b in the second.  Pairs [0, 1024): every m in 1..32, all four alphabets, and no longer bit
    vector, so all 16 waves stay 32-bit.  Pairs [1024, 3072): every m in 1..64 in the order 1, 33, 2, 34, ..., so that
    every wave of 64 holds bit vectors over 32 bytes and runs the 64-bit word, those of 1..32 bytes included.  Four
    pairs per (alphabet, side, m): the walked string is the pattern after substitutions (n = m), the pattern 0..8 edits
    apart and m + k bytes long (k running through 0..15 over the groups: every n mod 16, and n < 16 for small m), and
    two unrelated strings of m + k and of m + 16 + (0..99) bytes.  No side is empty and none is over 64 bytes on both
    sides or over 200 bytes at all: no pair is listed."""
    rng = np.random.default_rng(seed)
    a, b = [], []
    order64 = [m for pair in zip(range(1, 33), range(33, 65)) for m in pair]
    for ms in (list(range(1, 33)), order64):
        for ai, alpha in enumerate(ALPHABETS):
            for side in range(2):
                for m in ms:
                    p = rand_string(rng, m, alpha)
                    k = (m + 5 * ai + 3 * side) % 16
                    same_len = bytearray(p)
                    for _ in range(int(rng.integers(0, 4))):
                        same_len[int(rng.integers(0, m))] = rand_string(rng, 1, alpha)[0]
                    walked = [bytes(same_len), _relative(rng, p, m + k, alpha), rand_string(rng, m + (k + 7) % 16, alpha),
                              rand_string(rng, m + 16 + int(rng.integers(0, 100)), alpha)]
                    for t in walked:
                        if side == 1 and len(t) == m:
                            t += rand_string(rng, 16, alpha)  # b is the bit vector only if it is strictly shorter
                        a.append(p if side == 0 else t)
                        b.append(t if side == 0 else p)
    return a, b


def blob_end_slacks(m: int) -> List[int]:
    """Bytes between a pattern's end and the stated end of its blob that decide its last chunk's load: with
    r = (16 - m % 16) % 16 bytes missing to a full chunk, 0 (byte by byte whenever r > 0), r - 1 (the last slack still
    byte by byte) and r (the first with every chunk in one load)."""
    r = (16 - m % 16) % 16
    return sorted({0, max(r - 1, 0), r})


def blob_end_calls(seed: int = 0xB10B):
    """One column per word: {"word", "pat", "txt", "calls"}.  `pat` holds patterns of 64, 1, 2, ..., 63 bytes (word 64: the
    first lane keeps the one wave 64-bit for every count) or of 32, 1, ..., 31 bytes (word 32), over 256 symbols, and one
    more string of 16 bytes that no call compares: it is the memory behind the last pattern.  `txt` holds a strictly
    longer string per pattern (so the pattern is the bit vector on whichever side it is passed), related to it in every
    second pair.  `calls` is a list of (count, slack): the call compares the first `count` pairs and states
    off[count] + slack bytes as the pattern blob's size, so that pair count - 1 is the pattern at the blob's end.  Per m
    the slacks of blob_end_slacks: 180 calls for word 64, 90 for word 32, each to be made with the patterns as a and as b."""
    rng = np.random.default_rng(seed)
    cols = []
    for word in (64, 32):
        ms = [word] + list(range(1, word))
        pat = [rand_string(rng, m, 256) for m in ms]
        txt = []
        for i, p in enumerate(pat):
            n = len(p) + 1 + int(rng.integers(0, 40))
            txt.append(_relative(rng, p, n, 256) if i % 2 == 0 else rand_string(rng, n, 256))
        calls = [(i + 1, s) for i, m in enumerate(ms) for s in blob_end_slacks(m)]
        cols.append({"word": word, "pat": pat + [rand_string(rng, 16, 256)], "txt": txt, "calls": calls})
    return cols


SHARED_CANDIDATES = 260  # more than one workgroup of 256 lanes: two workgroups build the table
SHARED_LIMIT_LENGTHS = (1, 7, 64)  # run again with limit = 3


def shared_calls(seed: int = 0x5A4E):
    """For every query length 1..64: (query, candidates).  The query is over 256 symbols with at least one byte >= 0x80
    (and, from two bytes on, at least one below); SHARED_CANDIDATES candidates of 0..80 bytes, every second one a piece of
    the query after 0..8 edits, the others unrelated over 256 symbols; one is empty and one has 80 bytes."""
    rng = np.random.default_rng(seed)
    out = []
    for qlen in range(1, BATCH_WORD + 1):
        q = bytearray(rand_string(rng, qlen, 256))
        q[int(rng.integers(0, qlen))] |= 0x80
        if qlen > 1 and min(q) >= 0x80:
            q[q.index(min(q))] &= 0x7F
        q = bytes(q)
        cand = []
        for i in range(SHARED_CANDIDATES):
            if i % 2 == 0:
                lo = int(rng.integers(0, qlen + 1))
                piece = q[lo:lo + int(rng.integers(0, 81))]
                cand.append(edited(rng, piece, int(rng.integers(0, 9)), 256, 80))
            else:
                cand.append(rand_string(rng, int(rng.integers(0, 81)), 256))
        cand[1], cand[3] = b"", rand_string(rng, 80, 256)  # both ends of the range, whatever the draws
        out.append((q, cand))
    return out


LONG_SHARED = (65536, 65537, 200000)  # candidates at and over BATCH_LONG: kernel 2 walks them whatever their length


def long_shared(seed: int = 0x1056):
    """For queries of 7 and 64 bytes over 256 symbols: (query, 300 candidates).  Candidates 5, 70 and 290 (three waves,
    two workgroups) have LONG_SHARED bytes: unrelated, unrelated, and the 64-byte query repeated with 40 edits; the others
    are short, as in shared_calls.  One against many lists none of them; as the pairwise call with the query repeated the
    two over BATCH_LONG are listed."""
    rng = np.random.default_rng(seed)
    q64 = rand_string(rng, 64, 256)
    out = []
    for q in (q64[20:27], q64):
        cand = []
        for i in range(300):
            if i % 2 == 0:
                lo = int(rng.integers(0, len(q) + 1))
                cand.append(edited(rng, q[lo:lo + int(rng.integers(0, 81))], int(rng.integers(0, 9)), 256, 80))
            else:
                cand.append(rand_string(rng, int(rng.integers(0, 81)), 256))
        cand[5] = rand_string(rng, LONG_SHARED[0], 256)
        cand[70] = rand_string(rng, LONG_SHARED[1], 4)
        rep = bytearray(q64 * (LONG_SHARED[2] // 64))
        for at in rng.integers(0, len(rep), 40).tolist():  # substitutions keep the length
            rep[at] ^= 0x55
        cand[290] = bytes(rep)
        out.append((q, cand))
    return out


GROWTH_LISTED = (4097, 6000, 10)  # pairs for the pair-by-pair path in the three calls: past the list's first 4,096 entries,
# past what the first growth left, and a few
GROWTH_SHORT = 2000  # short pairs mixed among them
MAX_GROWTH_LISTED = 12000  # the one case past MAX_FALLBACK_PAIRS: listed pairs per TEST, under a second at 66-71 us each
# the calls of the two growth tests, (column, limit), in order on one context
GROWTH_SEQUENCES = {"grow": ((0, None), (1, None), (2, None)), "repeat": ((0, None), (0, 2))}


def growth_pairs(seed: int = 0x6207) -> List[Tuple[List[bytes], List[bytes]]]:
    """Three columns (a, b) with GROWTH_LISTED pairs of 65..70 bytes on both sides (every second one a few edits apart)
    at random places among GROWTH_SHORT pairs of 0..40 bytes."""
    rng = np.random.default_rng(seed)
    cols = []
    for n_listed in GROWTH_LISTED:
        is_long = np.zeros(n_listed + GROWTH_SHORT, dtype=bool)
        is_long[rng.choice(is_long.size, n_listed, replace=False)] = True
        a, b = [], []
        for i, lng in enumerate(is_long.tolist()):
            alpha = ALPHABETS[i % 4]
            lo, hi = (65, 70) if lng else (0, 40)
            x = rand_string(rng, int(rng.integers(lo, hi + 1)), alpha)
            n = int(rng.integers(lo, hi + 1))
            y = _relative(rng, x, n, alpha) if i % 2 == 0 and n > 0 else rand_string(rng, n, alpha)
            a.append(x)
            b.append(y)
        cols.append((a, b))
    return cols


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
