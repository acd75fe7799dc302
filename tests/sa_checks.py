"""CPU-side checks of a suffix array that do not need a suffix array construction (numpy only), for texts too long for the
prefix-doubling oracle.  For LOWERCASE text only: in its first sort the reference ranks the position behind the text as
character 96 ('`'), which is below every lowercase letter but not below every byte, so only on lowercase text is its order the
ordinary one (a suffix that is a prefix of another comes first) -- here: the text padded with 0.

  is_permutation(sa, n)                 every start 0 .. n-1 exactly once
  is_sorted(x, sa)                      adjacent suffixes strictly ascending, compared to their ends
  periodic_is_sorted(x, p, sa)          the same for x = tile(paragraph of p letters)[:n], from the first 2 p bytes only
  periodic_suffix_array(x, p)           that rule as one np.lexsort: the array itself (small n)

A permutation whose adjacent pairs all ascend strictly is the suffix array, nothing else.  The walks go through the array in
chunks, so 2^25 entries need the text, eight bytes per character of packed words and one chunk's temporaries.

Why 2 p bytes are enough for a periodic text (q = its primitive period; q divides p): let two suffixes i and j both have
2 p bytes and agree on them, and d = (j - i) mod q.  If d != 0 the window of 2 p >= q + d bytes has the periods q and d, so
(Fine and Wilf) gcd(q, d) < q as well, and as it holds a whole period of the text, so has the text: q was not primitive.  So
d = 0, the later suffix is a prefix of the earlier one and comes first.  A suffix shorter than 2 p bytes meets the padding, which
is below every letter, where the other still has a letter -- unless both have the same length, i.e. are the same suffix."""
import numpy as np

CHUNK = 1 << 20


def is_permutation(sa, n) -> bool:
    sa = np.asarray(sa)
    if sa.size != n:
        return False
    if n == 0:
        return True
    if int(sa.min()) < 0 or int(sa.max()) >= n:
        return False
    seen = np.zeros(n, dtype=bool)
    seen[sa] = True
    return bool(seen.all())


def _packed_words(x):
    """w[i] = bytes i .. i+7 of the text padded with 0, most significant first; w[n] = 0 stands for every start past the end."""
    x = np.ascontiguousarray(x, dtype=np.uint8)
    n = x.size
    pad = np.zeros(n + 8, dtype=np.uint8)
    pad[:n] = x
    w = np.zeros(n + 1, dtype=np.uint64)
    for k in range(8):
        w[:n] |= pad[k:k + n].astype(np.uint64) << np.uint64(8 * (7 - k))
    return w


def _adjacent_compare(w, n, sa, limit=None, chunk=CHUNK):
    """For every adjacent pair of `sa`: -1 / 0 / +1 as suffix sa[j] is below / equal to / above suffix sa[j + 1] on their first
    `limit` bytes (None: to their ends), 0-padded.  Yields (first pair of the chunk, int8 array)."""
    m = len(sa) - 1
    for lo in range(0, m, chunk):
        hi = min(m, lo + chunk)
        ia = np.asarray(sa[lo:hi], dtype=np.int64)
        ib = np.asarray(sa[lo + 1:hi + 1], dtype=np.int64)
        out = np.zeros(hi - lo, dtype=np.int8)
        act = np.arange(hi - lo)
        off = 0
        while act.size and (limit is None or off < limit):
            pa = np.minimum(ia[act] + off, n)
            pb = np.minimum(ib[act] + off, n)
            both_ended = (pa == n) & (pb == n)  # (the same suffix twice: never in a permutation)
            wa, wb = w[pa], w[pb]
            if limit is not None and limit - off < 8:
                mask = np.uint64((0xFFFFFFFFFFFFFFFF << (8 * (8 - (limit - off)))) & 0xFFFFFFFFFFFFFFFF)
                wa, wb = wa & mask, wb & mask
            lt, gt = wa < wb, wa > wb
            out[act[lt]] = -1
            out[act[gt]] = 1
            act = act[~(lt | gt | both_ended)]
            off += 8
        yield lo, out


def is_sorted(x, sa, chunk=CHUNK) -> bool:
    """Adjacent suffixes strictly ascending (lowercase text).  Each pair is compared eight bytes at a time until it differs.
    An entry that occurs twice in a row compares as equal and fails here; other damage to the SET of entries does not show
    in adjacent pairs, so callers assert is_permutation as well: both together admit only the suffix array."""
    x = np.ascontiguousarray(x, dtype=np.uint8)
    w = _packed_words(x)
    return all(bool((c < 0).all()) for _, c in _adjacent_compare(w, x.size, sa, None, chunk))


def periodic_is_sorted(x, p, sa, chunk=CHUNK) -> bool:
    """x = tile(paragraph of p lowercase letters)[:n].  Adjacent suffixes compare by their first 2 p bytes padded with 0; if
    those are equal the shorter one (the later start) comes first.  Like is_sorted, to be used beside is_permutation."""
    x = np.ascontiguousarray(x, dtype=np.uint8)
    w = _packed_words(x)
    sa = np.asarray(sa)
    for lo, c in _adjacent_compare(w, x.size, sa, 2 * p, chunk):
        a, b = sa[lo:lo + c.size], sa[lo + 1:lo + 1 + c.size]
        if not bool(((c < 0) | ((c == 0) & (a > b))).all()):
            return False
    return True


def periodic_suffix_array(x, p) -> np.ndarray:
    """The suffix array of a periodic lowercase text by the same rule, as one lexsort over 2 p key bytes (small n only)."""
    x = np.ascontiguousarray(x, dtype=np.uint8)
    n = x.size
    pad = np.concatenate([x, np.zeros(2 * p, dtype=np.uint8)])
    idx = np.arange(n)
    keys = [-idx] + [pad[k:k + n] for k in range(2 * p - 1, -1, -1)]  # (lexsort: the last key is the primary one)
    return np.lexsort(keys).astype(np.int32)
