"""Test helper: inputs for the thresholds of the approximate and the dictionary search (tests/test_gpu_search_limits.py),
built in numpy alone.  tests/test_limit_cases_cpu.py proves every per-tile count claimed here with the oracles, so the GPU
tests may rely on "this tile holds 2049 hits" without a GPU having said so.

Both kernels order their output tile by tile.  A tile parks its hits in an LDS pool of 2048 entries (TILE_STAGE,
DICT_STAGE) and walks itself a second time when it has more.  Tiles are counted from the text pointer rounded down to
16 bytes: view byte i has the aligned coordinate i + first, first = pointer mod 16.  For a text of 1 MiB or less

* an approximate-search tile is 256 << ps ends with ps = max(6, ceil_log2(4 (m + k))) (bmx_internal_approx_piece_shift:
  the other term, n over the resident lanes, stays at or below 64 for any occupancy of a 256-CU device);
* a dictionary tile is one round of 8 KiB of match starts (rounds_shift = 0).

Texts are background bytes in 0x80..0xFF, which no pattern here contains, with `units` planted in them: short byte
strings whose hits are known from the oracle run on the unit alone.  Two units are at least `gap` background bytes
apart, so no alignment (approximate: at most m + k bytes long, with at least one pattern byte matched) and no pattern
occurrence touches two of them, and the text's hits are the units' hits.
"""
from dataclasses import dataclass, field
from typing import List, Sequence, Tuple

import numpy as np

from approx_oracle import approx_ends
from dict_oracle import dict_matches

STAGE = 2048            # TILE_STAGE == DICT_STAGE: hits a tile parks
DICT_TILE = 8192        # dictionary tile of a text <= 1 MiB
MAX_TILE_TEXT = 1 << 20  # the tile sizes above hold up to here
OFFSETS = (0, 1, 15)    # pointer offsets (mod 16) every tile case is rebuilt for

EDGE = list(range(2040, 2057))                 # every count around the pool size
SEQUENCE = [3, 2049, 5, 2048, 2049, 0, 2047]   # sparse / dense / sparse / full / dense / empty / one below
COUNT_LISTS = (EDGE[:9] + [0, 1, 4096], EDGE[9:] + SEQUENCE)  # <= 16 tiles each: 1 MiB at the largest tile (64 KiB)


def ceil_log2(x: int) -> int:
    s = 0
    while (1 << s) < x:
        s += 1
    return s


def approx_tile_bytes(m: int, k: int) -> int:
    """Ends per tile of the approximate search on a text of at most MAX_TILE_TEXT bytes."""
    return 256 << max(6, ceil_log2(4 * (m + k)))


def background(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0x80, 0x100, n, dtype=np.uint8)


def bin_by_tile(positions, tile: int, first: int, n_tiles: int) -> List[int]:
    """Hits per tile for positions in view coordinates."""
    return np.bincount((np.asarray(positions, np.int64) + first) // tile, minlength=n_tiles).tolist()


@dataclass
class Unit:
    data: bytes
    rel: np.ndarray  # hit positions relative to the unit's first byte, one entry per hit, ascending

    @property
    def count(self) -> int:
        return int(self.rel.size)


@dataclass
class TileCase:
    name: str
    text: bytes
    tile: int
    first: int
    counts: List[int]
    pat: bytes = b""                 # approximate search
    k: int = 0
    patterns: List[bytes] = field(default_factory=list)  # dictionary search

    def prefix(self, t: int) -> int:
        return int(sum(self.counts[:t]))


def _lay_out(units: Sequence[Unit], counts: Sequence[int], tile: int, first: int, gap: int, seed: int) -> bytes:
    """A text of len(counts) tiles (aligned coordinates; the view starts at `first`) in which tile t holds exactly
    counts[t] hits, all from `units`.  In a tile the first unit sits as far left and the last as far right as the tile
    allows (hits at both edges), the others evenly between."""
    n = len(counts) * tile - first
    assert 0 < n <= MAX_TILE_TEXT, n
    text = background(n, seed)
    by_count = {}
    for u in units:
        if u.count:
            by_count.setdefault(u.count, []).append(u)
    sizes = sorted(by_count, reverse=True)
    turn = 0
    cursor = 0
    for t, need in enumerate(counts):
        lo, hi = max(t * tile - first, 0), (t + 1) * tile - first
        chosen = []
        while need:
            c = next((c for c in sizes if c <= need), None)
            assert c is not None, f"no unit with at most {need} hits"
            chosen.append(by_count[c][turn % len(by_count[c])])
            turn += 1
            need -= c
        if not chosen:
            continue
        starts = [max(cursor, lo - int(chosen[0].rel[0]))]
        for u in chosen[:-1]:
            starts.append(starts[-1] + len(u.data) + gap)
        slack = min(hi - 1 - (starts[-1] + int(chosen[-1].rel[-1])), n - (starts[-1] + len(chosen[-1].data)))
        assert slack >= 0, f"tile {t} cannot hold {counts[t]} hits"
        for i, u in enumerate(chosen):
            shift = slack * i // (len(chosen) - 1) if len(chosen) > 1 else (slack if t % 2 else 0)
            s = starts[i] + shift
            assert s + len(u.data) <= n
            text[s:s + len(u.data)] = np.frombuffer(u.data, np.uint8)
            cursor = s + len(u.data) + gap
    return text.tobytes()


# ---- approximate search -----------------------------------------------------------------------------------------------

def approx_unit(data: bytes, pat: bytes, k: int) -> Unit:
    """The unit's qualifying ends, from the oracle on the unit between m + k background bytes on either side."""
    pad = len(pat) + k
    bg = background(2 * pad, 0xB6).tobytes()
    e, _ = approx_ends(bg[:pad] + data + bg[pad:], pat, k)
    return Unit(data, e - pad)


def edited_copies(pat: bytes, k: int) -> List[bytes]:
    """The pattern and copies of it with 1..k bytes replaced by a background byte (from byte 0 on, evenly spread): a copy
    with j substitutions qualifies at fewer ends around it, the one with k at a single end."""
    out = [pat]
    for j in range(1, k + 1):
        s = bytearray(pat)
        for i in range(j):
            s[i * len(pat) // j] = 0x80 + i
        out.append(bytes(s))
    return out


def runs(byte: int, m: int, counts: Sequence[int]) -> List[bytes]:
    """Runs of one byte: a run of m - 1 + c holds c exact occurrences of byte * m, at adjacent ends."""
    return [bytes([byte]) * (m - 1 + c) for c in counts]


def approx_tile_case(hits_per_tile: Sequence[int], m: int, k: int, first: int = 0, pat: bytes = None,
                     plants: Sequence[bytes] = None, name: str = "") -> TileCase:
    """Tile t (aligned coordinates) holds exactly hits_per_tile[t] qualifying ends.  `pat`: m bytes below 0x80 (default:
    m distinct ones); `plants`: the byte strings to plant (default: edited_copies)."""
    pat = bytes(range(0x30, 0x30 + m)) if pat is None else pat
    assert len(pat) == m and max(pat) < 0x80 and 0 <= k < m
    units = [approx_unit(p, pat, k) for p in (plants if plants is not None else edited_copies(pat, k))]
    tile = approx_tile_bytes(m, k)
    gap = m + k if k else 1
    text = _lay_out(units, hits_per_tile, tile, first, gap, seed=1000 * m + 10 * k + first)
    return TileCase(name or f"approx m={m} k={k}", text, tile, first, list(hits_per_tile), pat=pat, k=k)


# (name, m, k, pattern, plants, count lists)
_DISTINCT33 = bytes(range(0x30, 0x30 + 33))
APPROX_TILE_SETS = [
    # one byte: a hit is a byte; runs put hits at adjacent ends of one lane, single bytes spread them over the lanes
    ("m1_k0", 1, 0, b"q", runs(0x71, 1, [1, 5, 64, 700]), COUNT_LISTS),
    # two bytes, one edit: "ab" qualifies at three ends, "a" at two, "b" at one (hits cluster, distances 0 and 1)
    ("m2_k1", 2, 1, b"ab", [b"ab", b"a", b"b"], COUNT_LISTS),
    # the 64-bit word, exact: runs of "a" against "a" * 33
    ("m33_k0_runs", 33, 0, b"a" * 33, runs(0x61, 33, [1, 3, 50, 600]), COUNT_LISTS),
    # the 64-bit word, one edit: a copy qualifies at three ends, a copy with one substitution at one; a 64 KiB tile holds
    # at most 2900 such hits, so 2600 stands in for 4096
    ("m33_k1", 33, 1, _DISTINCT33, None, (EDGE[:9] + [0, 1, 2600], EDGE[9:] + SEQUENCE)),
]


def approx_tile_cases(only: str = None):
    """Every TileCase the GPU tests run (or those of one set): each set, each count list, rebuilt for each pointer
    offset so that the counts hold in aligned coordinates."""
    for name, m, k, pat, plants, lists in APPROX_TILE_SETS:
        if only is not None and name != only:
            continue
        for li, counts in enumerate(lists):
            for first in OFFSETS:
                yield approx_tile_case(counts, m, k, first, pat, plants, name=f"{name} list {li} offset {first}")


# ---- dictionary search ------------------------------------------------------------------------------------------------

DUP_GROUPS = ((b"dupA", 2047), (b"dupB", 2048), (b"dupC", 2049), (b"dupD", 4200))  # 4200 > 65,535 / 16


def dict_variant(variant: str) -> Tuple[List[bytes], List[bytes]]:
    """(patterns, plants) of a variant: "one" -- one pair per position; "two" -- two patterns at each planted position;
    "dup" -- one position carries 2047, 2048, 2049 or 4200 pairs through that many copies of one pattern, their ids mixed
    among the others'."""
    if variant == "one":
        return [b"lazy dog", b"q", b"fox", b"hi"], [b"q" * 64, b"q" * 8, b"lazy dog", b"fox", b"q", b"hi"]
    if variant == "two":
        return [b"wx", b"q", b"lazy dog", b"w"], [b"wx", b"q"]
    assert variant == "dup"
    pats = [b"q"] + [p for p, c in DUP_GROUPS for _ in range(c)]
    order = np.random.default_rng(0xD0B).permutation(len(pats))
    return [pats[i] for i in order], [b"q"] + [p for p, _ in DUP_GROUPS]


def dict_unit(data: bytes, patterns: Sequence[bytes]) -> Unit:
    p, _ = dict_matches(data, patterns)
    return Unit(data, p)


def dict_tile_case(pairs_per_tile: Sequence[int], variant: str, first: int = 0, name: str = "") -> TileCase:
    """Tile t (8 KiB of aligned match starts) holds exactly pairs_per_tile[t] pairs."""
    patterns, plants = dict_variant(variant)
    units = [dict_unit(p, patterns) for p in plants]
    text = _lay_out(units, pairs_per_tile, DICT_TILE, first, 1, seed=77 + first + len(patterns))
    return TileCase(name or f"dict {variant}", text, DICT_TILE, first, list(pairs_per_tile), patterns=patterns)


DICT_VARIANTS = ("one", "two", "dup")
# the two heavy positions in an otherwise sparse text: 2049 pairs at one position, 4200 at another
DUP_SPARSE = [1, 2049, 0, 2, 4200, 1, 0, 2048, 3, 2047, 1]


def dict_count_lists(variant: str):
    return COUNT_LISTS + ((DUP_SPARSE,) if variant == "dup" else ())


def dict_tile_cases(only: str = None):
    for variant in DICT_VARIANTS:
        if only is not None and variant != only:
            continue
        for li, counts in enumerate(dict_count_lists(variant)):
            for first in OFFSETS:
                yield dict_tile_case(counts, variant, first, name=f"{variant} list {li} offset {first}")


# ---- planted texts for the large runs ---------------------------------------------------------------------------------

@dataclass
class PlantPlan:
    n: int
    idx: np.ndarray     # text indices to overwrite, ascending
    val: np.ndarray     # their bytes
    windows: List[Tuple[int, int]]  # (start, length), ascending and disjoint: every hit lies in one of them


def plan_plants(n: int, plants: Sequence[Tuple[int, bytes]], reach: int) -> PlantPlan:
    """A text of n background bytes (0x80..0xFF, the caller's) with `plants` (offset, bytes below 0x80) copied in; the
    plants must not overlap.  windows: each plant with `reach` bytes on either side, clipped to the text, overlapping
    or adjoining ones merged.  Outside the plants every byte is background, which no pattern contains.  A dictionary
    occurrence therefore lies inside a run of plant bytes (reach 0); an alignment of cost <= k matches at least one
    pattern byte and spans at most m + k bytes, so with reach = m + k it lies inside a window, and the oracle on the
    window, whose first `reach` bytes are background, sees the same table columns as on the whole text."""
    plants = sorted(plants, key=lambda p: p[0])
    idx, val, windows = [], [], []
    end = 0
    for off, data in plants:
        assert off >= end and off + len(data) <= n and max(data) < 0x80, (off, end)
        end = off + len(data)
        idx.append(np.arange(off, end, dtype=np.int64))
        val.append(np.frombuffer(data, np.uint8))
        lo, hi = max(off - reach, 0), min(end + reach, n)
        if windows and lo <= windows[-1][0] + windows[-1][1]:
            windows[-1] = (windows[-1][0], hi - windows[-1][0])
        else:
            windows.append((lo, hi - lo))
    return PlantPlan(n, np.concatenate(idx), np.concatenate(val), windows)


def spread_offsets(lo: int, hi: int, count: int, room: int, rng, keep_clear: Sequence[Tuple[int, int]] = ()) -> List[int]:
    """About `count` offsets in [lo, hi), one in the first half of each (hi - lo) // count stretch, each with `room`
    free bytes behind it; those within `room` of a (from, to) range of keep_clear are left out."""
    spacing = (hi - lo) // count
    assert spacing > 4 * room
    out = []
    for j in range(count):
        p = lo + j * spacing + int(rng.integers(room, spacing // 2))
        if p + room <= hi and not any(a - room < p < b + room for a, b in keep_clear):
            out.append(p)
    return out


def host_planted_text(plan: PlantPlan, seed: int) -> bytes:
    """The planted text on the host (small n only)."""
    t = background(plan.n, seed)
    t[plan.idx] = plan.val
    return t.tobytes()
