"""Test helper for the begins search and the ends pass (bmx_search_regex_begins*, bmx_regex_ends_device) and for
leftmost-longest matching: the definition by brute force over Python's ``re``, the automaton's answer through the reversed
automaton on the reversed text (regex_oracle's numpy matchers), and the sequential definition of the POSIX matches."""
import numpy as np

import regex_oracle as ro

NONE = 0xFFFFFFFFFFFFFFFF


def begins_brute(text, expr, flags: int = 0):
    """The definition: for every start s, every end e, re.fullmatch of the substring.  Returns (starts, shortest ends,
    longest ends) as lists.  Independent of the automaton; for tiny inputs."""
    rx = ro.to_re(expr, flags)
    text = bytes(text)
    starts, short, long_ = [], [], []
    for s in range(len(text)):
        ok = [e for e in range(s, len(text)) if rx.fullmatch(text, s, e + 1)]
        if ok:
            starts.append(s)
            short.append(ok[0])
            long_.append(ok[-1])
    return starts, short, long_


def begins_numpy(text, rx: ro.Rx):
    """The automaton's answer: (starts, shortest ends, longest ends) as int64 arrays, starts ascending.  text[s..e] matches
    rx iff the mirrored substring matches reverse(rx), so the ends of reverse(rx) on the reversed text are the starts, and
    its starts there the ends."""
    t = bytes(text)[::-1]
    n = len(t)
    rev = ro.reverse(rx)
    e_short, s_short = ro.starts_numpy(t, rev, longest=False)
    e_long, s_long = ro.starts_numpy(t, rev, longest=True)
    assert np.array_equal(e_short, e_long) and np.array_equal(e_short, ro.ends_numpy(t, rev))
    starts = (n - 1 - e_short)[::-1]
    # the reversed text's LARGEST start of an end is the original's smallest end of that start
    return starts.astype(np.int64), (n - 1 - s_short)[::-1].astype(np.int64), (n - 1 - s_long)[::-1].astype(np.int64)


def posix_matches(text, expr, limit_of=None, flags: int = 0):
    """The sequential definition of leftmost-longest: at position p take the smallest start s >= p from which a match
    begins, take its longest end (with ``limit_of``: no match may use a byte past limit_of(s), the last byte of the row of
    s; a start without a match inside its row is no start), continue at e + 1.  Returns [(s, e)]."""
    rx = ro.to_re(expr, flags)
    text = bytes(text)
    n = len(text)
    out = []
    p = 0
    while p < n:
        found = None
        for s in range(p, n):
            top = n - 1 if limit_of is None else min(n - 1, limit_of(s))
            ok = [e for e in range(s, top + 1) if rx.fullmatch(text, s, e + 1)]
            if ok:
                found = (s, ok[-1])
                break
        if found is None:
            break
        out.append(found)
        p = found[1] + 1
    return out


def row_end(text, delim: int = 10):
    """limit_of for the lines of ``text`` split at ``delim``: s -> the last byte of its row (the delimiter itself, or the
    text's last byte)."""
    t = np.frombuffer(bytes(text), np.uint8)
    cuts = np.nonzero(t == delim)[0]

    def limit_of(s):
        i = int(np.searchsorted(cuts, s))
        return int(cuts[i]) if i < cuts.size else t.size - 1

    return limit_of


def posix_replace(text, expr, repl: bytes, limit_of=None) -> bytes:
    text = bytes(text)
    parts, at = [], 0
    for s, e in posix_matches(text, expr, limit_of):
        parts.append(text[at:s])
        parts.append(repl)
        at = e + 1
    parts.append(text[at:])
    return b"".join(parts)


def struct_of(rx: ro.Rx):
    """An oracle automaton as the library's plain data (struct bmx_regex), with its length fields."""
    import ctypes as C

    import classes_oracle as co
    from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

    r = host.Regex()
    r.m, r.first, r.last, r.min_len, r.max_len = rx.m, rx.first, rx.last, rx.min_len, rx.max_len
    for i, f in enumerate(rx.follow):
        r.follow[i] = f
    packed = co.pack(rx.member).tobytes()
    C.memmove(r.classes, packed, len(packed))
    return r
