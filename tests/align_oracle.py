"""Oracle of the alignments (bmx_align*, include/bmx.h): the plain unit-cost table D[i][t] = ED(pat[:i], span[:t]) and
the canonical walk from (m, L) back to (0, 0) that takes at each cell the first step that keeps the value -- diagonal
('=' or 'X'), up ('I'), left ('D') -- written from the start of the span to its end with equal neighbours merged into
runs.  Rows are filled with numpy (the left neighbour by a running minimum), the walk is plain Python."""
import numpy as np

INS, DEL, EQ, X = 1, 2, 7, 8
NONE = 255
NO_POS = (1 << 64) - 1
CHARS = "MIDNSHP=X"


def table(pat: bytes, span: bytes) -> np.ndarray:
    m, L = len(pat), len(span)
    s = np.frombuffer(span, dtype=np.uint8)
    ramp = np.arange(L + 1, dtype=np.int64)
    D = np.empty((m + 1, L + 1), dtype=np.int64)
    D[0] = ramp
    for i in range(1, m + 1):
        row = np.empty(L + 1, dtype=np.int64)
        row[0] = i
        row[1:] = np.minimum(D[i - 1, :-1] + (s != pat[i - 1]), D[i - 1, 1:] + 1)
        D[i] = np.minimum.accumulate(row - ramp) + ramp  # D[i][t] = min over u <= t of row[u] + (t - u)
    return D


def script(pat: bytes, span: bytes):
    """(dist, runs): runs = [(length, code), ...] from the start of the span to its end."""
    D = table(pat, span)
    i, t = len(pat), len(span)
    steps = []
    while i > 0 or t > 0:
        v = D[i, t]
        if i > 0 and t > 0 and D[i - 1, t - 1] + (pat[i - 1] != span[t - 1]) == v:
            steps.append(EQ if pat[i - 1] == span[t - 1] else X)
            i, t = i - 1, t - 1
        elif i > 0 and D[i - 1, t] + 1 == v:
            steps.append(INS)
            i -= 1
        else:
            assert t > 0 and D[i, t - 1] + 1 == v
            steps.append(DEL)
            t -= 1
    runs = []
    for c in reversed(steps):
        if runs and runs[-1][1] == c:
            runs[-1] = (runs[-1][0] + 1, c)
        else:
            runs.append((1, c))
    return int(D[len(pat), len(span)]), runs


def cigar(runs) -> str:
    return "".join(f"{n}{CHARS[c]}" for n, c in runs)


def words(runs) -> list:
    return [(n << 4) | c for n, c in runs]


def apply(pat: bytes, span: bytes, runs) -> bytes:
    """The span rebuilt from the pattern by the script ('=' must copy equal bytes, 'X' must change one)."""
    out = bytearray()
    i = t = 0
    for n, c in runs:
        for _ in range(n):
            if c == EQ:
                assert pat[i] == span[t]
                out.append(pat[i])
                i, t = i + 1, t + 1
            elif c == X:
                assert pat[i] != span[t]
                out.append(span[t])
                i, t = i + 1, t + 1
            elif c == INS:
                i += 1
            else:
                assert c == DEL
                out.append(span[t])
                t += 1
    assert i == len(pat)
    return bytes(out)


def align(text: bytes, patterns, starts, ends, k: int, pid=None, base_offset: int = 0):
    """(dist uint8, op_off uint64, ops uint32) as bmx_align defines them; bad entries are the caller's to avoid."""
    count = len(starts)
    dist = np.full(count, NONE, dtype=np.uint8)
    op_off = np.zeros(count + 1, dtype=np.uint64)
    ops = []
    for e in range(count):
        s, j = int(starts[e]), int(ends[e])
        if not (s == NO_POS and j == NO_POS):
            pat = patterns[int(pid[e]) if pid is not None else (0 if len(patterns) == 1 else e)]
            span = text[s - base_offset:j - base_offset + 1]
            if abs(len(span) - len(pat)) <= k:
                d, runs = script(pat, span)
                if d <= k:
                    dist[e] = d
                    ops += words(runs)
        op_off[e + 1] = len(ops)
    return dist, op_off, np.asarray(ops, dtype=np.uint32)
