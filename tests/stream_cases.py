"""Test helper: one input per device entry point for the stream-ordering tests (tests/test_gpu_streams.py), built in
numpy alone.  A case is a REAL input, a DECOY of the same shape and the oracle's answer for either.  The GPU tests leave
the decoy in the device buffer, enqueue a long delay and then the copy of the real input on the caller's stream, and call
the entry point while that copy is still outstanding: a kernel, a copy or a memset of the library that is not ordered
behind the caller's stream reads the decoy.  tests/test_stream_cases_cpu.py proves, with the oracles alone, that the
decoy's answer differs from the real one's for every case -- without that a stale read would pass unnoticed.

Sizes (those the oracles already handle in the GPU suite; ordering bugs need a pending producer, not a large text):

    scan        4 MiB + 37 printable-95, m = 16, 300 plants                    port.search
    scan_dense  1 MiB + 7 of one byte, pattern of two: n - 1 hits (fill pass)  port.search
    scan_gen    2 MiB + 37 of the synthetic corpus (bmx_gen_text_device, then bmx_plant_device)
    multi       2 MiB + 11 printable-95, 5 patterns of 2..40 bytes             port.search per pattern
    approx32    1 MiB + 3 printable-95, m = 16, k = 3 (32-bit words)           approx_oracle.approx_ends
    approx64    512 KiB + 5 printable-95, m = 40, k = 2 (64-bit words)         approx_oracle.approx_ends
    approx_big  17 MiB + 5 background, "ab" within 1 edit: 1,089 tiles of 16 KiB where eight workgroups per CU are
                resident -- more than the 1,024 status words a context starts with, so they are re-allocated and
                cleared in mid-life; oracle on the windows around the plants (limit_cases.plan_plants)
    dict        1 MiB + 9 printable-95, 48 patterns of 2..24 bytes             dict_oracle.dict_matches
    dict_big    17 MiB + 1 background, 6 patterns: 2,177 tiles of 8 KiB (status words re-allocated for any occupancy);
                oracle on the plants (reach 0)
    ed          9,000 x 7,000 and 3,000 x 2,500 over four letters              port.edit_distance
    sa          300,000 and 100,000 over a..d                                  port.suffix_array
    regex_star  256 KiB + 9 of ACGT, N[ACGT]*G: one text that taints the call (slow path) and one that does not, each the
                other's decoy                                                  regex_star_oracle.ends_numpy
"""
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

import limit_cases as lc
import regex_star_oracle as so
from approx_oracle import approx_ends
from dict_oracle import DictIndex, dict_matches
from parallel_implementation_of_string_matching_algorithms_opencl_amd import corpus

# ---- the numbers the issue leaves to the measurement on the MI355X ------------------------------------------------------
# delay(stream): DELAY_COPIES device-to-device copies of DELAY_BYTES each, enqueued back to back.
# Measured on the MI355X (tests/test_gpu_streams.py prints both, pytest -s shows them):
#   host gap, pending.record() -> the assertion in front of the host.py call, worst of the 16 call sites of one run:
#     0.093 ms (a fresh context is created inside it; 0.006 ms where only the event is queried); host.py's own
#     marshalling in front of the C call, a dozen ctypes conversions, is of the same order
#   the delay alone, from a pair of events around it: 34.6 ms = 370 x the worst gap (20 x is asked for)
# The condition the tests hold is `not pending.query()` right before every call; these numbers are only how it is met.
DELAY_BYTES = 256 << 20
DELAY_COPIES = 96
HOST_GAP_MEASURED_MS = 0.093
DELAY_MEASURED_MS = 34.6
# Join timeout of the two host threads: 20 x the single-thread wall time of SEQUENCE on one context, measured on the
# MI355X in a process of its own (first use of every kernel and workspace included): 17.0 ms.
SEQUENCE_MEASURED_S = 0.0170
JOIN_TIMEOUT_S = 20 * SEQUENCE_MEASURED_S


@dataclass
class StreamCase:
    name: str
    kind: str                                   # scan | multi | approx | dict | ed | sa
    real: Tuple[np.ndarray, ...]                # the operands (one text; edit distance: a and b)
    decoy: Tuple[np.ndarray, ...]               # same shapes
    pat: bytes = b""
    k: int = 0
    patterns: List[bytes] = field(default_factory=list)
    expr: str = ""                              # regex_star: the expression
    windows: Optional[Tuple[list, list]] = None  # (real, decoy): (start, length) windows that hold every hit
    _want: dict = field(default_factory=dict)

    def operands(self, which: str) -> Tuple[np.ndarray, ...]:
        return self.real if which == "real" else self.decoy

    def want(self, port, which: str = "real") -> List[np.ndarray]:
        """The oracle's answer as a list of int64 arrays: scan [positions]; multi one list per pattern; approx
        [ends, distances]; dict [positions, pattern ids]; ed [[distance]]; sa [suffix array]."""
        if which not in self._want:
            self._want[which] = [np.asarray(a, np.int64) for a in self._answer(port, self.operands(which), which)]
        return self._want[which]

    def _answer(self, port, ops, which):
        if self.kind == "scan":
            return [port.search(ops[0], self.pat)]
        if self.kind == "multi":
            return [port.search(ops[0], p) for p in self.patterns]
        if self.kind == "ed":
            return [[port.edit_distance(ops[0], ops[1])]]
        if self.kind == "sa":
            return [port.suffix_array(ops[0])]
        if self.kind == "regex_star":
            return [so.ends_numpy(ops[0].tobytes(), so.parse(self.expr))]
        text = ops[0].tobytes()
        wins = None if self.windows is None else self.windows[0 if which == "real" else 1]
        if self.kind == "approx":
            if wins is None:
                return list(approx_ends(text, self.pat, self.k))
            parts = [approx_ends(text[lo:lo + ln], self.pat, self.k) for lo, ln in wins]
            return [np.concatenate([e + lo for (e, _), (lo, _) in zip(parts, wins)]), np.concatenate([d for _, d in parts])]
        assert self.kind == "dict"
        if wins is None:
            return list(dict_matches(text, self.patterns))
        index = DictIndex(self.patterns)
        parts = [index.matches(text[lo:lo + ln]) for lo, ln in wins]
        return [np.concatenate([p + lo for (p, _), (lo, _) in zip(parts, wins)]), np.concatenate([i for _, i in parts])]


def same(a: Sequence[np.ndarray], b: Sequence[np.ndarray]) -> bool:
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def _printable(rng, n: int) -> np.ndarray:
    return (rng.integers(0, 95, n) + 32).astype(np.uint8)


def _with_plants(text: np.ndarray, rng, plants: Sequence[bytes], count: int) -> np.ndarray:
    """`count` plants, cycling through `plants`, at random offsets (the last one flush with the end of the text)."""
    room = max(len(p) for p in plants)
    offs = sorted(rng.integers(0, text.size - room, count - 1).tolist()) + [None]
    for j, off in enumerate(offs):
        p = np.frombuffer(plants[j % len(plants)], np.uint8)
        off = text.size - p.size if off is None else off
        text[off:off + p.size] = p
    return text


def _edited(pat: bytes, rng, k: int) -> List[bytes]:
    """The pattern, and copies with 1..k edits (a substitution, a deletion, an insertion in turn)."""
    out = [pat]
    for e in range(1, k + 1):
        s = bytearray(pat)
        for j in range(e):
            at = int(rng.integers(1, len(s) - 1))
            if j % 3 == 0:
                s[at] = 0x7E if s[at] != 0x7E else 0x7D
            elif j % 3 == 1:
                del s[at]
            else:
                s.insert(at, 0x7E)
        out.append(bytes(s))
    return out


def _pair(make, seed: int):
    """(real, decoy): the same recipe from two seeds."""
    return make(np.random.default_rng(seed)), make(np.random.default_rng(seed ^ 0xDEC0))


def scan_case(seed: int, n: int = (4 << 20) + 37) -> StreamCase:
    pat = b"stream-ordering!"
    real, decoy = _pair(lambda rng: _with_plants(_printable(rng, n), rng, [pat], 300), seed)
    return StreamCase(f"scan n={n}", "scan", (real,), (decoy,), pat=pat)


def scan_dense_case(seed: int, n: int = (1 << 20) + 7) -> StreamCase:
    """One byte all through: n - 1 hits, the result takes the fill pass (per-tile count arrays of the context).  The
    decoy has another byte in every 4,096th place."""
    real = np.full(n, ord("a"), np.uint8)
    decoy = real.copy()
    decoy[(seed % 4096)::4096] = ord("b")
    return StreamCase(f"scan dense n={n}", "scan", (real,), (decoy,), pat=b"aa")


def multi_case(seed: int, n: int = (2 << 20) + 11) -> StreamCase:
    pats = [b"ab", b"Multi", b"pattern-pass", b"a table blob per call..", b"0123456789" * 4]
    real, decoy = _pair(lambda rng: _with_plants(_printable(rng, n), rng, pats[1:], 400), seed)
    return StreamCase(f"multi n={n}", "multi", (real,), (decoy,), patterns=pats)


def approx_case(seed: int, wide: bool) -> StreamCase:
    n, pat, k = ((512 << 10) + 5, b"sixty-four-bit words: forty bytes long!!", 2) if wide else ((1 << 20) + 3, b"approximate-sear", 3)
    assert len(pat) == (40 if wide else 16)

    def make(rng):
        return _with_plants(_printable(rng, n), rng, _edited(pat, rng, k), 200)

    real, decoy = _pair(make, seed)
    return StreamCase(f"approx m={len(pat)} k={k} n={n}", "approx", (real,), (decoy,), pat=pat, k=k)


def _planted_pair(n: int, seed: int, plants: Sequence[bytes], count: int, reach: int):
    out, wins = [], []
    for s in (seed, seed ^ 0xDEC0):
        rng = np.random.default_rng(s)
        offs = lc.spread_offsets(0, n - 64, count, 64, rng)
        plan = lc.plan_plants(n, [(o, plants[j % len(plants)]) for j, o in enumerate(offs)] + [(n - len(plants[0]), plants[0])], reach)
        out.append(np.frombuffer(lc.host_planted_text(plan, s & 0xFFFF), np.uint8))
        wins.append(plan.windows)
    return out[0], out[1], (wins[0], wins[1])


def approx_big_case(seed: int, n: int = (17 << 20) + 5) -> StreamCase:
    real, decoy, wins = _planted_pair(n, seed, [b"ab", b"a", b"b", b"xab"], 500, 3)
    return StreamCase(f"approx big n={n}", "approx", (real,), (decoy,), pat=b"ab", k=1, windows=wins)


def dict_case(seed: int, n: int = (1 << 20) + 9) -> StreamCase:
    words = np.random.default_rng(0xD1C7)  # the dictionary is the same for every seed
    pats = [bytes(_printable(words, int(words.integers(2, 25)))) for _ in range(46)] + [b"dictionary", b"dict"]
    real, decoy = _pair(lambda rng: _with_plants(_printable(rng, n), rng, pats[8:], 500), seed)
    return StreamCase(f"dict n={n}", "dict", (real,), (decoy,), patterns=pats)


def dict_big_case(seed: int, n: int = (17 << 20) + 1) -> StreamCase:
    pats = [b"lazy dog", b"q", b"fox", b"hi", b"lazy", b"a longer pattern of the dictionary"]
    real, decoy, wins = _planted_pair(n, seed, pats + [b"qq", b"hifox"], 600, 0)
    return StreamCase(f"dict big n={n}", "dict", (real,), (decoy,), patterns=pats, windows=wins)


def ed_case(seed: int, la: int = 9000, lb: int = 7000) -> StreamCase:
    """Real: two unrelated strings (a distance near 0.5 la).  Decoy: b is a copy of a's head with a few hundred edits (a
    small distance).  The CPU test also asserts that ONE stale operand changes the distance."""
    rng = np.random.default_rng(seed)
    a = (rng.integers(0, 4, la) + 65).astype(np.uint8)
    b = (rng.integers(0, 4, lb) + 65).astype(np.uint8)
    a2 = (rng.integers(0, 4, la) + 65).astype(np.uint8)
    b2 = np.resize(a2, lb).copy()
    at = rng.integers(0, lb, 300)
    b2[at] = (b2[at] - 65 + 1) % 4 + 65
    return StreamCase(f"ed {la}x{lb}", "ed", (a, b), (a2, b2))


def sa_case(seed: int, n: int = 300_000) -> StreamCase:
    real, decoy = _pair(lambda rng: (rng.integers(0, 4, n) + 97).astype(np.uint8), seed)
    return StreamCase(f"sa n={n}", "sa", (real,), (decoy,))


# ---- the star search: a tainted and an untainted text under one expression ------------------------------------------------

STAR_EXPR = "N[ACGT]*G"
STAR_N = (256 << 10) + 9  # five tiles of 64 KiB at the rule's piece (2^8 ends, a warm-up of 64 bytes)


def regex_star_cases(seed: int = 0x57A) -> List[StreamCase]:
    """[real tainted / decoy untainted, the other way round] for bmx_search_regex_star_device.  Tainted: ACGT with one N
    near the front -- the loop lives through every warm-up in the upper bound and in no lower one, so the call takes the
    slow path (memset, three kernels, a scan, a copy and four events on the caller's stream), and every G behind the N is
    a hit.  Untainted: the same kind of text with a '-' in every 32nd place, which ends the loop in both bounds, and an N
    in every 100th; the call is the first launch alone.  tests/test_stream_cases_cpu.py proves both predictions with
    so.fast_taint and that the two answers differ."""
    rng = np.random.default_rng(seed)
    tainted = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, STAR_N)].copy()
    tainted[7] = ord("N")
    clean = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, STAR_N)].copy()
    clean[50::100] = ord("N")
    clean[31::32] = ord("-")
    return [StreamCase("star: real tainted, decoy untainted", "regex_star", (tainted,), (clean,), expr=STAR_EXPR),
            StreamCase("star: real untainted, decoy tainted", "regex_star", (clean,), (tainted,), expr=STAR_EXPR)]


# ---- the synthetic corpus produced on the stream (bmx_gen_text_device + bmx_plant_device) ------------------------------

GEN_SPEC = corpus.CorpusSpec("streams", (2 << 20) + 37, 16, 0, 0x5EED0051, 1 << 14, 1 << 18, -1)
GEN_SHORT = b"e "  # two bytes: a few hundred natural occurrences in 2 MiB of printable-95 text, before anything is planted


def gen_case() -> Tuple[StreamCase, StreamCase]:
    """(unplanted, planted).  bmx_gen_text_device only launches; bmx_plant_device synchronises its stream (it frees its
    staging buffers), so only the generator can still be outstanding when the search is called: the first case searches
    the two-byte GEN_SHORT in the generated text before anything is planted, the second the planted 16-byte pattern."""
    s = GEN_SPEC
    decoy = _printable(np.random.default_rng(0x6E6), s.n)
    raw = corpus.stream_bytes(0, s.n, s.seed, s.kind).copy()
    return (StreamCase("scan of generated text", "scan", (raw,), (decoy,), pat=GEN_SHORT),
            StreamCase("scan of generated and planted text", "scan", (s.host_text(),), (raw,), pat=s.pattern()))


# ---- the case lists ----------------------------------------------------------------------------------------------------

def entry_point_cases(seed: int = 0x57A) -> List[StreamCase]:
    """One case per entry point, for "input still being produced" and "null stream busy, fresh context"."""
    return [scan_case(seed), multi_case(seed), approx_case(seed, wide=False), approx_case(seed, wide=True), dict_case(seed),
            ed_case(seed), sa_case(seed)]


# (case key, stream): A and B are the caller's two non-blocking streams, 0 the null stream
SEQUENCE = [("scan", "A"), ("multi", "B"), ("approx32", "0"), ("dict", "A"), ("ed_small", "B"), ("sa_small", "0"),
            ("scan_dense", "A"), ("approx64", "B"), ("ed", "0"), ("sa", "A"), ("dict_big", "B"), ("approx_big", "0"),
            ("ed_small", "A"), ("multi", "0"), ("dict", "B"), ("approx32", "A"), ("sa_small", "B"), ("scan", "B")]


def sequence_cases(seed: int) -> dict:
    """The cases of SEQUENCE: every algorithm, shapes that grow (the workspace is re-allocated), shrink and repeat (it is
    reused), each algorithm on more than one stream."""
    return {"scan": scan_case(seed), "scan_dense": scan_dense_case(seed), "multi": multi_case(seed),
            "approx32": approx_case(seed, wide=False), "approx64": approx_case(seed, wide=True),
            "approx_big": approx_big_case(seed), "dict": dict_case(seed), "dict_big": dict_big_case(seed),
            "ed_small": ed_case(seed, 3000, 2500), "ed": ed_case(seed), "sa_small": sa_case(seed, 100_000), "sa": sa_case(seed)}
