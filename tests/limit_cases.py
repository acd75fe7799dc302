"""Test helper: inputs for the thresholds of the approximate and the dictionary search (tests/test_gpu_search_limits.py)
and for every search over the tile frame at a chosen piece size and grid (tests/test_gpu_tile_geometry.py; below, from
`Search` on), built in numpy alone.  tests/test_limit_cases_cpu.py proves every per-tile count claimed here with the oracles, so the GPU
tests may rely on "this tile holds 2049 hits" without a GPU having said so.

The star search (bmx_search_regex_star_device) has its searches (STAR_SEARCHES: a family that never taints a call and one
that always does), its warm-up edge cases and its 4 GiB patterns here too, for tests/test_gpu_regex_star_limits.py.

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

import zlib

import numpy as np

import classes_oracle as co
import gaps_oracle as go
import hamming_oracle as ho
import regex_oracle as ro
import regex_star_oracle as so
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
    search: object = None            # a Search (tile frame at a chosen piece size)
    ps: int = 0                      # ... and its piece shift: tile == 256 << ps

    def prefix(self, t: int) -> int:
        return int(sum(self.counts[:t]))


def _lay_out(units: Sequence[Unit], counts: Sequence[int], tile: int, first: int, gap: int, seed: int, keep: int = 0) -> bytes:
    """A text of len(counts) tiles (aligned coordinates; the view starts at `first`) in which tile t holds exactly
    counts[t] hits, all from `units`.  In a tile the first unit sits as far left and the last as far right as the tile
    allows (hits at both edges), the others evenly between.  The first `keep` bytes of the view stay free (background)."""
    n = len(counts) * tile - first
    assert 0 < n <= MAX_TILE_TEXT, n
    text = background(n, seed)
    by_count = {}
    for u in units:
        if u.count:
            by_count.setdefault(u.count, []).append(u)
    sizes = sorted(by_count, reverse=True)
    turn = 0
    cursor = keep
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


# ---- the searches over the tile frame at a chosen piece size and grid ---------------------------------------------------
#
# tests/test_gpu_tile_geometry.py forces the geometry of a launch through libbmx_exp.so's knobs "tile_piece_shift" and
# "tile_max_grid": a tile is 256 << ps ends for a ps the production rule can give the pattern (Search.floor .. Search.cap),
# and `grid` workgroups share the tiles.  A hit is counted in the tile of its END, whatever the search reports: the class
# and the k-mismatch search report the start, end - (m - 1).

@dataclass
class Search:
    """One search over the tile frame with its oracle.  kind: "classes", "approx_classes", "hamming", "gaps", "regex",
    "regex_star", "approx" or "approx_long"; letters: the bytes a run is made of."""
    kind: str
    name: str
    member: np.ndarray = None    # classes [m, 256] (classes, approx_classes, hamming, gaps)
    k: int = 0                   # edits / mismatches
    must: int = 0                # hamming
    optional: int = 0            # gaps
    rx: object = None            # regex: regex_oracle.Rx; regex_star: regex_star_oracle.StarRx
    pat: bytes = b""             # approx, approx_long
    letters: bytes = b"ab"
    prefix: bytes = b""          # regex_star, natural taint: what the text begins with (and every hit's match)

    @property
    def m(self) -> int:
        return self.rx.m if self.kind in ("regex", "regex_star") else len(self.pat) if self.pat else len(self.member)

    @property
    def reach(self) -> int:
        """No match is longer; two plants this far apart share no match, and the rule's floor is ceil_log2(4 reach).  The
        star search has no longest match: a background byte between two plants empties the state of a pattern none of
        whose classes holds one (test_limit_cases_cpu.py), and behind `prefix` it leaves the state the prefix alone
        leaves, so 1."""
        if self.kind == "regex_star":
            return 1
        if self.kind == "regex":
            return self.rx.max_len
        return self.m + (self.k if self.kind in ("approx", "approx_long", "approx_classes") else 0)

    @property
    def min_len(self) -> int:
        """The shortest run of `letters` that holds a hit (behind `prefix`: every letter is one)."""
        if self.kind == "regex_star" and self.prefix:
            return 1
        if self.kind in ("regex", "regex_star"):
            return self.rx.min_len
        if self.kind == "gaps":
            return self.m - bin(self.optional).count("1")
        return self.m - self.k

    @property
    def floor(self) -> int:
        """The smallest piece shift the production rule gives this pattern (bmx_internal_*_piece_shift)."""
        if self.kind == "regex_star":
            return 8  # (MIN_PIECE_SHIFT of bmx_regex_star.hip: the pattern has no say)
        return max(6, min(ceil_log2(4 * self.reach), self.cap))

    @property
    def cap(self) -> int:
        return 12 if self.kind in ("approx_long", "regex_star") else 11

    @property
    def report(self) -> int:
        """reported position = end - report"""
        return self.m - 1 if self.kind in ("classes", "hamming") else 0

    def ends(self, text: bytes):
        """(ends int64 ascending, distances int64 or None) by the search's own oracle."""
        if self.kind == "classes":
            return co.class_starts(text, self.member) + (self.m - 1), None
        if self.kind == "approx_classes":
            return co.class_approx_ends(text, self.member, self.k)
        if self.kind == "hamming":
            p, d = ho.hamming_starts(text, self.member, self.k, self.must)
            return p + (self.m - 1), d
        if self.kind == "gaps":
            return go.gap_ends(text, self.member, self.optional), None
        if self.kind == "regex":
            return ro.ends_numpy(text, self.rx), None
        if self.kind == "regex_star":
            return so.ends_numpy(text, self.rx), None
        return approx_ends(text, self.pat, self.k)

    def ends_behind_prefix(self, stretch: bytes):
        """The hits of a stretch of text that lies somewhere behind `prefix` (relative to the stretch): the oracle on
        the prefix and the stretch.  Without a prefix: ends()."""
        e, d = self.ends(self.prefix + stretch)
        return e - len(self.prefix), d

    def run(self, length: int) -> bytes:
        """`length` bytes of the search's letters (random among them, the same for every call)."""
        rng = np.random.default_rng(zlib.crc32(self.name.encode()) + length)
        return np.frombuffer(self.letters, np.uint8)[rng.integers(0, len(self.letters), length)].tobytes()

    def unit(self, data: bytes) -> Unit:
        """The hits of `data` between `reach` background bytes on either side, as ends relative to its first byte."""
        pad = self.reach
        bg = background(2 * pad, 0xB6).tobytes()
        e, _ = self.ends_behind_prefix(bg[:pad] + data + bg[pad:])
        return Unit(data, e - pad)

    def run_unit(self, hits: int) -> Unit:
        """A run that holds `hits` hits at adjacent ends, or a few more where edits reach past its last byte."""
        u = self.unit(self.run(self.min_len - 1 + hits))
        assert hits <= u.count <= hits + self.k and np.all(np.diff(u.rel) == 1), (self.name, hits, u.count)
        return u


def _gaps(name, expr):
    member, optional = go.parse(expr)
    return Search("gaps", name, member=member, optional=optional)


# Every kernel slot of the frame.  The Shift-And family matches runs of the letters a and b (the k-mismatch search: of
# a alone, with position 0 in `must`, so that a run of L bytes holds L - (m - k) + 1 hits and its last k have the
# distances 1..k); a run one byte longer holds one hit more, so a unit has any wanted count and a dense tile hits at
# adjacent ends.  The gapped and the regex patterns have 1 to 3 ends per shortest plant.
SEARCHES = {x.name: x for x in (
    Search("approx", "approx32", pat=b"ab", k=1),
    Search("approx", "approx64", pat=_DISTINCT33, k=1),
    Search("approx_long", "approx_long2", pat=bytes(range(0x30, 0x30 + 65)), k=1),
    Search("classes", "classes32", member=co.parse("[ab]" * 5)),
    Search("classes", "classes64", member=co.parse("[ab]" * 64)),
    Search("approx_classes", "approx_classes", member=co.parse("[aA][bB][cC][dD][eE][fF]"), k=1),
    _gaps("gaps32", "[ab][cd]?[ab]{1,3}"),
    _gaps("gaps64", "[ab]{30}[cd]?[ab]{1,3}"),
    Search("hamming", "hamming32x2", member=co.singletons(b"a" * 8), k=2, must=1, letters=b"a"),
    Search("hamming", "hamming32x4", member=co.singletons(b"a" * 12), k=6, must=1, letters=b"a"),
    Search("hamming", "hamming64x2", member=co.singletons(b"a" * 40), k=3, must=1, letters=b"a"),
    Search("hamming", "hamming64x4", member=co.singletons(b"a" * 40), k=9, must=1, letters=b"a"),
    Search("regex", "regex32", rx=ro.parse("[ab][ab][ab]?")),
    Search("regex", "regex64", rx=ro.parse("[ab]{33}[ab]?")),
    Search("regex", "regex32nl", rx=ro.parse("([ab]|c[ab])[ab]{1,2}")),
    Search("regex", "regex64nl", rx=ro.parse("([ab]|c[ab])[ab]{30}[ab]{1,2}")),
)}
# the long approximate search and the run search at k = 1 for the large pieces: runs of one letter
SEARCHES["approx_run"] = Search("approx", "approx_run", pat=b"a" * 40, k=2, letters=b"a")
SEARCHES["approx_long_run"] = Search("approx_long", "approx_long_run", pat=b"a" * 65, k=1, letters=b"a")

# The star search (bmx_search_regex_star_device; tests/test_gpu_regex_star_limits.py), every kernel slot of its two
# launches.  First family: no lane's pair warm-up ends with two different bounds (a letter or two, or one background
# byte, and they meet), so the call is the first launch alone unless the slow path is forced: a cycle at 32 and at 64
# bits (a self-loop is an irregular position), and the star-free automata of regex32, regex64 and regex32nl through the
# star entry (the slots without irregular positions, and the acyclic irregular one).  Second family, NATURAL TAINT:
# c.*[ab] on a text whose byte 0 is the only c.  The upper bound holds the `.` for ever and the lower bound never has it,
# so every lane whose warm-up does not begin at view byte 0 is tainted, the first launch reports (nearly) nothing and the
# slow path's columns carry the `.` from piece to piece; the hits are the letters, as for [ab]+.
STAR_SEARCHES = {x.name: x for x in (
    Search("regex_star", "star32", rx=so.parse("[ab]+")),
    Search("regex_star", "star64", rx=so.parse("(q{33})?[ab]+")),
    Search("regex_star", "star_regex32", rx=so.parse("[ab][ab][ab]?")),
    Search("regex_star", "star_regex64", rx=so.parse("[ab]{33}[ab]?")),
    Search("regex_star", "star_regex32nl", rx=so.parse("([ab]|c[ab])[ab]{1,2}")),
    Search("regex_star", "taint32", rx=so.parse("c.*[ab]"), prefix=b"c"),
    Search("regex_star", "taint64", rx=so.parse("(q{33})?c.*[ab]"), prefix=b"c"),
)}
STAR_FAST = [n for n, s in STAR_SEARCHES.items() if not s.prefix]
STAR_TAINT = [n for n, s in STAR_SEARCHES.items() if s.prefix]
STAR_COUNT_OFFSET = 15  # the pointer offset of the count-list cases (the geometry cases run at all of OFFSETS)


def search_named(name: str) -> Search:
    return SEARCHES[name] if name in SEARCHES else STAR_SEARCHES[name]


def star_warm(ps: int) -> int:
    """bmx_internal_regex_star_warm: a sixteenth of the piece, at least 64 bytes."""
    return max(64, (1 << ps) >> 4)


GRIDS = (1, 2, 3)
SEQUENCE_BOTH_WAYS = SEQUENCE + SEQUENCE[::-1]  # 14 tiles: dense then sparse and sparse then dense in every workgroup


def tiles_per_workgroup_at_least(n_tiles: int, grid: int) -> int:
    """Tiles go to the workgroups one ticket at a time, so how they spread is the scheduler's; but `grid` workgroups
    that take n_tiles tiles between them leave one with at least the mean, rounded up."""
    assert n_tiles >= 1 and grid >= 1
    return -(-n_tiles // grid)


def search_units(s: Search) -> List[Unit]:
    """The units of a search's tile cases: for the distinct-byte approximate patterns the edited copies (1 or 3 ends
    each), else runs of 1, 2, 3, 64 and 700 hits."""
    if s.kind in ("approx", "approx_long", "approx_classes") and len(set(s.pat or b"abcdef")) > 2:
        pat = s.pat or b"abcdef"
        return [s.unit(p) for p in edited_copies(pat, s.k)]
    if s.name == "approx32":
        return [s.unit(p) for p in (b"ab", b"a", b"b")]
    return [s.run_unit(c) for c in (1, 2, 3, 64, 700)]


def geometry_counts(s: Search) -> List[int]:
    """The run sparse / dense / sparse / full / dense / empty / one below, then backwards: 14 tiles, or as many of them
    as 1 MiB holds at the search's floor (the long approximate search: 8 tiles of 128 KiB)."""
    return SEQUENCE_BOTH_WAYS[:min(len(SEQUENCE_BOTH_WAYS), MAX_TILE_TEXT // (256 << s.floor))]


def search_tile_case(s: Search, hits_per_tile: Sequence[int], ps: int, first: int = 0) -> TileCase:
    """Tile t of 256 << ps ends (aligned coordinates) holds exactly hits_per_tile[t] hits of the search."""
    assert s.floor <= ps <= s.cap, (s.name, ps)
    units = search_units(s)
    assert any(u.count == 1 for u in units), s.name
    tile = 256 << ps
    text = _lay_out(units, hits_per_tile, tile, first, s.reach, seed=zlib.crc32(s.name.encode()) % 100000 + first, keep=len(s.prefix))
    text = s.prefix + text[len(s.prefix):]
    return TileCase(f"{s.name} ps={ps} offset {first}", text, tile, first, list(hits_per_tile), search=s, ps=ps)


def geometry_cases(only: str = None):
    """Every TileCase of the several-tiles-per-workgroup tests: each search at its floor, rebuilt for each pointer
    offset."""
    for name, s in SEARCHES.items():
        if name.endswith("_run") or (only is not None and name != only):
            continue
        for first in OFFSETS:
            yield search_tile_case(s, geometry_counts(s), s.floor, first)


def star_geometry_cases(name: str):
    """The same fourteen tiles of 64 KiB (the star search's smallest piece) for a star search, at each pointer offset."""
    s = STAR_SEARCHES[name]
    for first in OFFSETS:
        yield search_tile_case(s, SEQUENCE_BOTH_WAYS, s.floor, first)


def star_count_case(name: str, which: int) -> TileCase:
    """COUNT_LISTS[which] (every per-tile count 2040..2056 around the pool, 0, 1, 4096) in tiles of 64 KiB."""
    s = STAR_SEARCHES[name]
    return search_tile_case(s, COUNT_LISTS[which], s.floor, STAR_COUNT_OFFSET)


def dict_geometry_case(first: int) -> TileCase:
    """The dictionary search's: two patterns at each planted position, 14 tiles of 8 KiB."""
    return dict_tile_case(SEQUENCE_BOTH_WAYS, "two", first, name=f"dict two both ways offset {first}")


def capacity_inside_second_dense(case: TileCase) -> int:
    """A capacity that ends in the middle of the second tile with more hits than the pool."""
    dense = [t for t, c in enumerate(case.counts) if c > STAGE]
    assert len(dense) >= 2
    return case.prefix(dense[1]) + case.counts[dense[1]] // 2


# ---- large pieces: hits on tile and lane boundaries, a full lane, a dense tile beside an empty one ---------------------------

BOUNDARY_OFFSET = 11
# (search, piece shift): each of the four Shift-And searches at 9, 10 and 11, its kernel slots taking turns (only the
# 32-bit k-mismatch slots run at all three or at two of them: an oracle run per case is the cost), m = 64 also at its floor
# 8; the two approximate searches at their caps
BOUNDARY_CASES = (
    ("classes64", 8), ("classes64", 9), ("classes32", 10), ("classes64", 11),
    ("gaps32", 9), ("gaps64", 10), ("gaps32", 11),
    ("hamming64x4", 9), ("hamming32x2", 9), ("hamming32x2", 10), ("hamming32x4", 10), ("hamming64x2", 11), ("hamming32x4", 11),
    ("regex32nl", 9), ("regex64", 10), ("regex32", 11), ("regex64nl", 11),
    ("approx_run", 11), ("approx_long_run", 12),
)
# the star search at 9..12, its slots taking turns: first family (run on the fast path and with the slow path forced),
# then natural taint
STAR_BOUNDARY_CASES = (
    ("star32", 9), ("star_regex64", 9), ("star64", 10), ("star_regex32nl", 10), ("star_regex32", 11), ("star64", 11),
    ("star32", 12), ("star_regex64", 12), ("star_regex32nl", 12),
)
STAR_TAINT_BOUNDARY_CASES = (("taint32", 9), ("taint64", 10), ("taint64", 11), ("taint32", 12))
BOUNDARY_LANES = (37, 101, 255)
FULL_LANE = 100    # of tile 1, which is walked twice: its hits are written by the second walk
PARKED_LANE = 150  # of tile 0, which stays below the pool: its hits go through the parked words, ordinal and all


def parked_lane_hits(ps: int) -> int:
    """Hits of the parked lane: the whole lane, or as many as leave tile 0 (with its boundary hits) inside the pool."""
    return min(1 << ps, STAGE - 48)


@dataclass
class BoundaryCase:
    name: str
    search: Search
    ps: int
    first: int
    text: bytes
    spans: List[Tuple[int, int]]  # (start, length) of every plant, ascending

    @property
    def tile(self) -> int:
        return 256 << self.ps

    def windows(self) -> List[Tuple[int, int]]:
        """The plants with `reach` bytes on either side, merged: every hit lies in one (plan_plants' argument)."""
        out = []
        for a, ln in self.spans:
            lo, hi = max(a - self.search.reach, 0), min(a + ln + self.search.reach, len(self.text))
            if out and lo <= out[-1][0] + out[-1][1]:
                out[-1] = (out[-1][0], max(hi, out[-1][0] + out[-1][1]) - out[-1][0])
            else:
                out.append((lo, hi - lo))
        return out

    def ends_by_windows(self):
        """The oracle on every window; the same lists as on the whole text (test_limit_cases_cpu.py), at a cost that
        goes with the plants."""
        es, ds = [], []
        for lo, ln in self.windows():
            stretch = self.text[lo:lo + ln]
            e, d = self.search.ends(stretch) if lo == 0 else self.search.ends_behind_prefix(stretch)
            es.append(e + lo)
            ds.append(d)
        return np.concatenate(es), (None if ds[0] is None else np.concatenate(ds))


def boundary_case(name: str, ps: int, first: int = BOUNDARY_OFFSET) -> BoundaryCase:
    """Three tiles of 256 << ps ends and 5 bytes.  In aligned coordinates, with T the tile and P = 1 << ps the piece:
    hits on both sides of the lane boundaries 37 P, 101 P and 255 P of tile 0 and of the tile boundary T; in lane 150 of
    tile 0 a hit at each of the first min(P, 2000) ends, in a tile of 2048 hits or fewer, so that ordinals up to that
    number less one are parked (and read back beside the distance, of which the run's last k hits have their own); in tile 1 nine
    hits in the middle of every lane (more than the pool in all: the tile is walked twice) and every end of lane 100, with
    the last end of lane 99 and the first of lane 101; the last ends of tile 1 up to 2 T - 1; tile 2 empty; the first end of
    tile 3 and every one up to the text's last byte."""
    s = search_named(name)
    assert s.floor <= ps <= s.cap, (name, ps)
    T, P = 256 << ps, 1 << ps
    n = 3 * T + 5
    text = background(n, zlib.crc32(name.encode()) % 100000 + ps)
    spans = []

    def put(u: Unit, which: int, aligned_end: int):
        """Unit u with its hit number `which` at the aligned end."""
        at = aligned_end - first - int(u.rel[which])
        assert at >= 0 and at + len(u.data) <= n and (not spans or at >= spans[-1][0] + spans[-1][1] + 1), (name, aligned_end)
        text[at:at + len(u.data)] = np.frombuffer(u.data, np.uint8)
        spans.append((at, len(u.data)))

    three, nine, full = s.run_unit(3), s.run_unit(9), s.run_unit(P + 2)
    for lane in BOUNDARY_LANES[:2]:
        put(three, 1, lane * P)
    put(s.run_unit(parked_lane_hits(ps) - s.k), 0, PARKED_LANE * P)  # (edits reach up to k ends past a run)
    put(three, 1, BOUNDARY_LANES[2] * P)
    put(three, 1, T)
    for lane in range(2, 254):
        if lane == FULL_LANE:
            put(full, 0, T + lane * P - 1)
        elif abs(lane - FULL_LANE) > 1:
            put(nine, 0, T + lane * P + P // 2 - 4)
    put(three, -1, 2 * T - 1)
    # 5 + first hits, from the aligned end 3 T to the text's last byte (a k-mismatch window has to lie inside the text)
    tail = s.run((s.m if s.kind == "hamming" else s.min_len) - 1 + 5 + first)
    text[n - len(tail):] = np.frombuffer(tail, np.uint8)
    spans.append((n - len(tail), len(tail)))
    assert spans[0][0] > len(s.prefix)
    text[:len(s.prefix)] = np.frombuffer(s.prefix, np.uint8)  # (the star search's natural taint: the one c, at view byte 0)
    return BoundaryCase(f"{name} ps={ps}", s, ps, first, text.tobytes(), spans)


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


# ---- the star search: the edge of the pair warm-up -------------------------------------------------------------------------
#
# c[ab]*d on background with ONE run c, letters, d.  The loop keeps the upper bound alive on the letters and the lower
# bound has it only behind the c, so the lane that owns the d is exact if and only if its warm-up holds the c -- or begins
# at view byte 0 by rule.  Every other lane's warm-up ends on a background byte or holds the c too.

STAR_EDGE = Search("regex_star", "edge", rx=so.parse("c[ab]*d"))


@dataclass
class WarmEdgeCase:
    name: str
    text: bytes
    first: int
    ps: int
    warm: int
    lead: int
    tainted_waves: int  # what the first launch must count (so.fast_taint agrees: test_limit_cases_cpu.py)
    d_at: int           # the one hit (view coordinates)


def _edge_text(n: int, first: int, c_aligned: int, d_aligned: int, seed: int) -> bytes:
    text = background(n, seed)
    c, d = c_aligned - first, d_aligned - first
    assert 0 <= c < d < n
    rng = np.random.default_rng(seed + 1)
    text[c + 1:d] = np.frombuffer(b"ab", np.uint8)[rng.integers(0, 2, d - c - 1)]
    text[c], text[d] = ord("c"), ord("d")
    return text.tobytes()


def warm_edge_cases(ps: int, first: int, warm: int = None):
    """Pieces of 2^ps ends, the view `first` bytes into its 16-byte line, a warm-up of `warm` bytes (default: the rule's).
    First the lane at the aligned boundary S (lane 3 of tile 1 at ps 8, of tile 0 above) with its d at S + 7 and the c
    at S - dist: inside the warm-up by one chunk (warm - 16), on its first chunk (its last and its first byte: warm - 15 + 14
    = warm - 1, warm), in the chunk in front (warm + 1, warm + 16).  Then a lead that puts the first lane's start16 at
    warm - 16, warm (both begin at view byte 0 by rule: exact whatever lies there) and warm + 16 (the warm-up begins at
    chunk 1), with the c at view byte 0."""
    warm = star_warm(ps) if warm is None else warm
    S = ((256 + 3) << ps) if ps == 8 else (3 << ps)
    seed = 7000 + 100 * ps + first
    for dist in (warm - 16, warm - 1, warm, warm + 1, warm + 16):
        if dist >= 1:
            text = _edge_text(S + (2 << ps) - first, first, S - dist, S + 7, seed + dist)
            yield WarmEdgeCase(f"ps={ps} offset {first} warm {warm}: c {dist} in front of start16", text, first, ps, warm, 0,
                               int(dist > warm), S + 7 - first)
    for start16 in (warm - 16, warm, warm + 16):
        if start16 >= 16:
            lo = start16 + 3
            text = _edge_text(max(2 << ps, start16 + (1 << ps)) - first, first, first, lo + 4, seed + 50 + start16)
            yield WarmEdgeCase(f"ps={ps} offset {first} warm {warm}: first lane's start16 {start16}, c at view byte 0", text, first,
                               ps, warm, lo - first, int(start16 > warm), lo + 4 - first)


# ---- the star search past 2^32: plants on ACGT -----------------------------------------------------------------------------

STAR_BIG = so.parse("(wx|y)z+[ef]")   # plant letters only: the bounds meet at the first ACGT byte
STAR_BIG_TAINT = so.parse("q.*[ef]")  # one q in front: no lane's bounds meet, one chain of pieces spans the text
STAR_BIG_REACH = 16


def star_big_instance(rng) -> bytes:
    """A string STAR_BIG matches, of at most 32 bytes (a path cut short there matches nothing; it is a plant all the same)."""
    buf = np.full(32, ord("z"), np.uint8)
    end = so.plant_path(rng, buf, STAR_BIG, 0)
    return buf[:end].tobytes()


def row_of_windows(text_of, windows):
    """(row, row_at, text_at): the windows laid end to end (text_of(lo, length) -> bytes), where window i begins in the
    row, and where in the text."""
    row = b"".join(text_of(lo, ln) for lo, ln in windows)
    return row, np.cumsum([0] + [ln for _, ln in windows]), np.array([lo for lo, _ in windows], np.int64)


def row_to_text(row_pos, row_at, text_at):
    row_pos = np.asarray(row_pos, np.int64)
    w = np.searchsorted(row_at, row_pos, side="right") - 1
    return row_pos - row_at[w] + text_at[w]
