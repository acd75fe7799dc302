"""GPU suite of the anchored regular-expression search (bmx_search_regex_anchored_device, its starts pass, the begins search
and its ends pass, kind="regex_anchored" of grep / sub / findall, the host-buffer forms, the CLI) against
regex_anchored_oracle.py: spans_numpy / begins_numpy everywhere (the CPU suite ties them to Python's re), matches_re itself
where the text is small.

The geometry case forces lanes of 64 ends / 16 starts and two workgroups through libbmx_exp.so ("tile_piece_shift",
"regex_begins_piece_shift", "tile_max_grid"): the delayed hit and the extra warm-up byte at the smallest shape at which they
can go wrong."""
import os
import re
import subprocess

import numpy as np
import pytest

import regex_anchored_oracle as ao
import regex_oracle as ro
from conftest import ROOT
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

pytestmark = pytest.mark.gpu

LOG = "^(ERROR|FATAL|PANIC): [0-9]{2,4}$"
NL, WORDB, OTHER = 10, ord("a"), ord(" ")


def _dev(data, first: int = 0, before: bytes = b"", behind: bytes = b""):
    """A view at alignment ``first`` (mod 16) of a device buffer that holds ``before`` in front of it and ``behind`` after."""
    import torch

    data = bytes(data)
    pad = (first - len(before)) % 16
    buf = torch.from_numpy(np.frombuffer(b"\x00" * pad + before + data + behind + b"\x00" * 16, np.uint8).copy()).cuda()
    view = buf[pad + len(before):pad + len(before) + len(data)]
    assert len(data) == 0 or view.data_ptr() % 16 == first % 16
    return view


def _t(values):
    import torch

    return torch.from_numpy(np.asarray(values, np.int64)).cuda()


def _check(ctx, text, pair, a=None, first=0, left=NL, right=NL, before=b"", behind=b"", what=None, passes=True):
    """All four entries on one view against the oracle.  Returns the number of matches' ends."""
    text = bytes(text)
    a = a or ao.from_lib(*pair)
    d_text = _dev(text, first, before, behind)
    kw = dict(left=left, right=right)
    cap = max(len(text), 1)
    want_e, want_s = ao.spans_numpy(text, a, left, right)
    got, total = ctx.search_regex_anchored_device(d_text, pair, capacity=cap, **kw)
    assert total == want_e.size and np.array_equal(got.cpu().numpy(), want_e), (what, "ends", total, want_e.size)
    want_b, want_be = ao.begins_numpy(text, a, left, right)
    gotb, totalb = ctx.search_regex_anchored_begins_device(d_text, pair, capacity=cap, **kw)
    assert totalb == want_b.size and np.array_equal(gotb.cpu().numpy(), want_b), (what, "begins", totalb, want_b.size)
    if passes and total:
        assert np.array_equal(ctx.regex_anchored_starts_device(d_text, pair, _t(want_e), **kw).cpu().numpy(), want_s), (what, "starts")
        long_s = ao.spans_numpy(text, a, left, right, longest=True)[1]
        assert np.array_equal(ctx.regex_anchored_starts_device(d_text, pair, _t(want_e), longest=True, **kw).cpu().numpy(), long_s), what
        assert np.array_equal(ctx.regex_anchored_ends_device(d_text, pair, _t(want_b), **kw).cpu().numpy(), want_be), (what, "ends pass")
        long_e = ao.begins_numpy(text, a, left, right, longest=True)[1]
        assert np.array_equal(ctx.regex_anchored_ends_device(d_text, pair, _t(want_b), longest=True, **kw).cpu().numpy(), long_e), what
    return int(total)


EXPRS = ["^a?b", "^a|b$", r"\bab\b", r"\<[ab]{1,3}\>", r"a\Bb", r"\b[a-z.]b", r"[a-z.]{1,3}\b", "^.", "b$"]


@pytest.mark.parametrize("n", [1, 15, 16, 17, 31, 32, 33, 4097])
def test_view_sizes(ctx, n):
    rng = np.random.default_rng(n)
    alphabet = np.frombuffer(b"ab. \n", np.uint8)
    hits = 0
    for expr in EXPRS:
        pair = host.compile_regex_anchored(expr)
        text = rng.choice(alphabet, n).tobytes()
        hits += _check(ctx, text, pair, what=(n, expr))
        if n <= 33:
            assert {j for _, j in ao.matches_re(text, expr)} == set(ao.spans_numpy(text, ao.from_lib(*pair))[0].tolist()), (n, expr)
    assert hits > 0


def test_every_alignment_and_every_length_mod_16(ctx):
    """16 alignments x 16 lengths mod 16, each view cut out of one text whose real neighbours are passed as left / right, and
    once more with a line break and a word edge on view byte 0 and n - 1."""
    rng = np.random.default_rng(0xA116)
    back = bytearray(rng.choice(np.frombuffer(b"ab. \n", np.uint8), 400).tobytes())
    pairs = [(e, host.compile_regex_anchored(e)) for e in ("^a?b", r"\bab?\b", r"[a-z.]{1,3}\b", "^.|.$")]
    oracles = [ao.from_lib(*p) for _, p in pairs]
    hits = 0
    for first in range(16):
        for r in range(16):
            n = 32 + r + 16 * (first % 3)
            lo = 100 + first
            for edge in (None, b"\n", b"a") if r % 4 == first % 4 else (None,):
                text = bytearray(back[lo:lo + n])
                if edge:
                    text[0:1] = edge
                    text[-1:] = edge
                for (expr, pair), a in zip(pairs, oracles):
                    hits += _check(ctx, text, pair, a, first=first, left=back[lo - 1], right=back[lo + n], before=bytes(back[lo - 8:lo]),
                                   behind=bytes(back[lo + n:lo + n + 8]), what=(first, n, expr, edge), passes=(r % 4 == 0))
    assert hits > 2000


def test_left_and_right_change_exactly_the_expected_entries(ctx):
    text = b"ab cat\nab"
    # (expression, the ends by `left` with right = \n, the ends by `right` with left = \n)
    cases = [("^ab", {NL: [1, 8], WORDB: [8], OTHER: [8]}, None),
             ("ab$", None, {NL: [8], WORDB: [], OTHER: []}),
             (r"\bab\b", {NL: [1, 8], WORDB: [8], OTHER: [1, 8]}, {NL: [1, 8], WORDB: [1], OTHER: [1, 8]})]
    for first in (0, 5):
        d_text = _dev(text, first, before=b"zz", behind=b"zz")
        for expr, by_left, by_right in cases:
            pair = host.compile_regex_anchored(expr)
            base = ctx.search_regex_anchored_device(d_text, pair)[0].cpu().tolist()
            for v, want in (by_left or {}).items():
                got = ctx.search_regex_anchored_device(d_text, pair, left=v)[0].cpu().tolist()
                assert got == want and (v != NL or got == base), (expr, "left", v)
                assert ctx.search_regex_anchored_begins_device(d_text, pair, left=v)[0].cpu().tolist() == [e - 1 for e in want]
            for v, want in (by_right or {}).items():
                got = ctx.search_regex_anchored_device(d_text, pair, right=v)[0].cpu().tolist()
                assert got == want, (expr, "right", v)
                assert ctx.search_regex_anchored_begins_device(d_text, pair, right=v)[0].cpu().tolist() == [e - 1 for e in want]
                if want:
                    assert ctx.regex_anchored_starts_device(d_text, pair, _t(want), right=v).cpu().tolist() == [e - 1 for e in want]
                    assert ctx.regex_anchored_ends_device(d_text, pair, _t([e - 1 for e in want]), right=v).cpu().tolist() == want


def _planted(rng, n, alphabet, plants, count):
    text = rng.choice(np.frombuffer(alphabet, np.uint8), n).astype(np.uint8)
    for at in rng.integers(1, n - 80, count):
        p = plants[int(rng.integers(0, len(plants)))]
        text[at:at + len(p)] = np.frombuffer(p, np.uint8)
    p = plants[0].lstrip(b"\n")
    text[:len(p)] = np.frombuffer(p, np.uint8)
    return text


KERNELS = [
    (r"\bneedle in the hay\b", b"nedl ithay.", [b" needle in the hay ", b"xneedle in the hay."], False, False),
    (LOG, b"EROFATL: 0123\n ", [b"\nERROR: 123\n", b"\nFATAL: 12\n", b" PANIC: 1234\n", b"\nERROR: 12 "], False, True),
    (r"^GATTACAGATTACAGATTACATG([ACGT]{3}){2,4}(TAA|TAG|TGA)\>", b"ACGT\n ", [b"\nGATTACAGATTACAGATTACATGAAACCCTAA ",
                                                                                 b"\nGATTACAGATTACAGATTACATGAAACCCGGGTAG\n"], True, True),
    (r"\<" + "[AC][CG][GT][AT]" * 10 + "$", b"ACGT\n ", [b" " + b"ACGA" * 10 + b"\n", b"\n" + b"CGTT" * 10 + b"\n"], True, False),
    (r"\b[a-z.]{2}(x|yz)\b", b"axyz._ \n", [b" .ax ", b" abyz\n", b".axx"], False, True),  # the split makes it irregular
]


@pytest.mark.parametrize("case", range(len(KERNELS)), ids=["m<=32 regular", "m<=32 irregular", "m>32 irregular", "m>32 regular", "split"])
def test_the_kernel_shapes_forward_and_begins(ctx, case):
    expr, alphabet, plants, wide, irregular = KERNELS[case]
    pair = host.compile_regex_anchored(expr)
    a = ao.from_lib(*pair)
    assert (a.rx.m > 32) == wide and (ro.split(a.rx)[1] != 0) == irregular
    assert (ro.split(ro.reverse(a.rx))[1] != 0) == irregular  # which begins kernel the host picks
    rng = np.random.default_rng(a.rx.m)
    text = _planted(rng, 20011, alphabet, plants, 200)
    for first in (0, 9):
        assert _check(ctx, text.tobytes(), pair, a, first=first, what=expr) >= 30


def test_lane_tile_and_ownership_boundaries(exp_ctx):
    """Lanes of 64 ends (forward) and 16 starts (begins), two workgroups over several tiles: a line break and a planted match
    at every residue around a lane edge, a tile edge and the end of the ownership."""
    expr = r"^(k|lm)n{3}o\b"
    pair = host.compile_regex_anchored(expr)
    a = ao.from_lib(*pair)
    L = a.rx.max_len
    first = 5
    T = 64 * 256  # the forward tile
    n = 2 * T + 300
    text = np.full(n, ord("z"), np.uint8)
    edges = [64 * 3 - first, 16 * 21 - first, T - first, 2 * T - first, 4096 - first]  # of a lane, of a tile, on either walk
    variants = []
    for edge in edges:
        for r in range(-L - 2, 4):  # the line break, the match's first and its last byte on every residue around the edge
            t = text.copy()
            at = edge + r
            t[at - 1] = 10
            t[at:at + 6] = np.frombuffer(b"lmnnno", np.uint8)
            t[at + 6] = ord(".")
            t[at + 20] = 10  # a second one that begins with the alternative
            t[at + 21:at + 26] = np.frombuffer(b"knnno", np.uint8)
            t[at + 26] = 10
            variants.append((at, t))
    exp_ctx.set_knob("tile_piece_shift", 6)
    exp_ctx.set_knob("regex_begins_piece_shift", 4)
    exp_ctx.search_regex_anchored_device(_dev(b"x", 0), pair)  # (the shared knobs reach a session that exists)
    exp_ctx.search_regex_anchored_begins_device(_dev(b"x", 0), pair)
    exp_ctx.set_knob("tile_piece_shift", 6)
    exp_ctx.set_knob("tile_max_grid", 2)
    for at, t in variants:
        d_text = _dev(t.tobytes(), first)
        got, total = exp_ctx.search_regex_anchored_device(d_text, pair, capacity=64)
        assert got.cpu().tolist() == [at + 5, at + 25], at
        shift, grid, tiles = exp_ctx.last_launch("regex_anchored")
        assert (shift, grid) == (6, 2) and tiles == 3
        gotb, totalb = exp_ctx.search_regex_anchored_begins_device(d_text, pair, capacity=64)
        assert gotb.cpu().tolist() == [at, at + 21], at
        shift, grid, tiles = exp_ctx.last_launch("regex_anchored_begins")
        assert (shift, grid) == (4, 2) and tiles > 2 * grid - 1
        # the condition fails one byte off: a word byte behind the match, no line break in front of it
        t2 = t.copy()
        t2[at + 6] = ord("o")
        t2[at + 20] = ord("z")
        d_text = _dev(t2.tobytes(), first)
        assert exp_ctx.search_regex_anchored_device(d_text, pair, capacity=64)[1] == 0
        assert exp_ctx.search_regex_anchored_begins_device(d_text, pair, capacity=64)[1] == 0
    # ownership: a lead / tail that cuts between the two matches
    at, t = variants[7]
    d_text = _dev(t.tobytes(), first)
    assert exp_ctx.search_regex_anchored_device(d_text, pair, lead=at + 6)[0].cpu().tolist() == [at + 25]
    assert exp_ctx.search_regex_anchored_device(d_text, pair, lead=at + 5)[0].cpu().tolist() == [at + 5, at + 25]
    assert exp_ctx.search_regex_anchored_begins_device(d_text, pair, tail=n - at - 21)[0].cpu().tolist() == [at]
    assert exp_ctx.search_regex_anchored_begins_device(d_text, pair, tail=n - at - 22)[0].cpu().tolist() == [at, at + 21]


@pytest.fixture(scope="module")
def dense():
    rng = np.random.default_rng(0xDE25E)
    n = 1 << 16
    lines = rng.choice(np.frombuffer(b"ab\n", np.uint8), n, p=[0.4, 0.3, 0.3]).astype(np.uint8)
    words = rng.choice(np.frombuffer(b"ab ", np.uint8), n, p=[0.3, 0.3, 0.4]).astype(np.uint8)
    return lines, words


def test_dense_tiles_on_both_walks(ctx, dense):
    lines, words = dense
    for text, expr in ((lines, "^."), (words, r"\b[a-z]"), (lines, "[ab]{1,2}$")):
        pair = host.compile_regex_anchored(expr)
        for first in (0, 3):
            assert _check(ctx, text.tobytes(), pair, first=first, what=expr, passes=(first == 0)) > 10000


def test_capacity(ctx, dense):
    import ctypes as C
    import torch

    lines, _ = dense
    pair = host.compile_regex_anchored("^.")
    a = ao.from_lib(*pair)
    want = ao.spans_numpy(lines.tobytes(), a)[0]
    d_text = _dev(lines.tobytes(), 2)
    total = C.c_uint64(0)
    out = torch.full((want.size + 8,), -1, dtype=torch.int64, device="cuda")
    for fn in (ctx._L.bmx_search_regex_anchored_device, ctx._L.bmx_search_regex_anchored_begins_device):  # (^. : one-byte matches)
        def raw(cap, with_out=True):
            rc = fn(ctx._h, C.c_void_p(d_text.data_ptr()), d_text.numel(), 0, 0, C.byref(pair[0]), C.byref(pair[1]), 10, 10,
                    C.c_void_p(out.data_ptr()) if with_out else None, cap, C.byref(total), None)
            return rc, int(total.value)

        assert raw(0, False) == (host.ERR_CAPACITY, want.size)  # count only
        out.fill_(-1)
        assert raw(want.size) == (host.OK, want.size)  # exact
        assert np.array_equal(out[:want.size].cpu().numpy(), want) and bool((out[want.size:] == -1).all())
        for cap in (want.size - 1, 1, 2049):
            out.fill_(-1)
            assert raw(cap) == (host.ERR_CAPACITY, want.size), cap
            assert np.array_equal(out[:cap].cpu().numpy(), want[:cap]) and bool((out[cap:] == -1).all()), cap  # the lowest


@pytest.mark.parametrize("shards", [3, 7])
def test_shards_concatenate_with_real_neighbour_bytes(ctx, shards):
    pair = host.compile_regex_anchored(LOG)
    a = ao.from_lib(*pair)
    rng = np.random.default_rng(shards)
    n = 70001
    text = _planted(rng, n, KERNELS[1][1], KERNELS[1][2], 2500)
    raw = text.tobytes()
    want_e = ao.spans_numpy(raw, a)[0]
    want_b = ao.begins_numpy(raw, a)[0]
    assert want_e.size > 200
    d_text = _dev(raw, 6)
    halo = a.rx.max_len - 1
    cuts = [n * i // shards for i in range(shards + 1)]
    for base in (0, (1 << 40) - n):
        ends, begins = [], []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            lead = min(halo, lo)
            got, total = ctx.search_regex_anchored_device(d_text[lo - lead:hi], pair, lead=lead, base_offset=base + lo - lead, capacity=hi - lo,
                                                          left=raw[lo - lead - 1] if lo - lead else NL, right=raw[hi] if hi < n else NL)
            assert total == got.numel()
            ends.append(got.cpu().numpy())
            tail = min(halo, n - hi)
            got, total = ctx.search_regex_anchored_begins_device(d_text[lo:hi + tail], pair, tail=tail, base_offset=base + lo, capacity=hi - lo,
                                                                 left=raw[lo - 1] if lo else NL, right=raw[hi + tail] if hi + tail < n else NL)
            assert total == got.numel()
            begins.append(got.cpu().numpy())
        assert np.array_equal(np.concatenate(ends), want_e + base), base
        assert np.array_equal(np.concatenate(begins), want_b + base), base


def test_both_identities(ctx):
    """Full classes give the unanchored lists of all four entries; the begins list is the set of starts of every match."""
    import torch

    rng = np.random.default_rng(0x1DE2)
    some = 0
    for case in range(10):
        symbols = np.arange(97, 99 + case % 3)
        expr, rx = ro.random_regex(rng, symbols, 12 if case % 2 else 40)
        text = rng.choice(symbols, 5000).astype(np.uint8)
        re_ = host.compile_regex(expr)
        pair = (re_, host.RegexAnchors.full())
        d_text = torch.from_numpy(text).cuda()
        n = text.size
        ends, total = ctx.search_regex_device(d_text, re_, capacity=n)
        got, t2 = ctx.search_regex_anchored_device(d_text, pair, capacity=n, left=case, right=255 - case)
        assert t2 == total and torch.equal(got, ends), expr
        begins, tb = ctx.search_regex_begins_device(d_text, re_, capacity=n)
        gotb, t3 = ctx.search_regex_anchored_begins_device(d_text, pair, capacity=n, left=case, right=255 - case)
        assert t3 == tb and torch.equal(gotb, begins), expr
        if total:
            for longest in (False, True):
                assert torch.equal(ctx.regex_anchored_starts_device(d_text, pair, ends, longest=longest),
                                   ctx.regex_starts_device(d_text, re_, ends, longest=longest)), expr
                assert torch.equal(ctx.regex_anchored_ends_device(d_text, pair, begins, longest=longest),
                                   ctx.regex_ends_device(d_text, re_, begins, longest=longest)), expr
        some += total
    assert some > 5000
    for expr in (r"\bab?\b", "^a|b$", r"[a-z.]{1,3}\b"):  # begins == the starts of the brute oracle
        text = rng.choice(np.frombuffer(b"ab. \n", np.uint8), 60).tobytes()
        want = sorted({s for s, _ in ao.matches_re(text, expr)})
        assert ctx.search_regex_anchored_begins_device(_dev(text, 3), expr)[0].cpu().tolist() == want, expr


def _random_anchored_pairs(count, seed):
    from test_regex_anchored_cpu import _random_anchored

    rng = np.random.default_rng(seed)
    symbols = np.frombuffer(b"ab_ .\n", np.uint8)
    for _ in range(count):
        expr, _ = _random_anchored(rng, symbols)
        yield expr, rng.choice(symbols, int(rng.integers(1, 60))).tobytes()


def test_passes_on_random_pairs_limits_and_foreign_lists(ctx):
    import torch

    seen = 0
    for i, (expr, text) in enumerate(_random_anchored_pairs(80, 0xE2D6)):
        pair = host.compile_regex_anchored(expr)
        seen += _check(ctx, text, pair, first=i % 16, left=text[0], right=text[-1], before=text, behind=text, what=(expr, text))
    assert seen > 100
    pair = host.compile_regex_anchored(r"\ba.{0,3}b\b")
    text = b"a1b3b ab+a"
    d_text = _dev(text, 3, behind=b"bbbb")
    assert ctx.regex_anchored_ends_device(d_text, pair, _t([0, 6])).cpu().tolist() == [4, 7]  # a1b: a word byte follows
    assert ctx.regex_anchored_ends_device(d_text, pair, _t([0, 6]), longest=True).cpu().tolist() == [4, 7]
    assert ctx.regex_anchored_ends_device(d_text, pair, _t([0, 0, 6, 6]), limit=_t([4, 3, 7, 6]), longest=True).cpu().tolist() == [4, -1, 7, -1]
    assert ctx.regex_anchored_starts_device(d_text, pair, _t([4, 7])).cpu().tolist() == [0, 6]
    assert ctx.regex_anchored_starts_device(d_text, pair, _t([])).numel() == 0 and ctx.regex_anchored_ends_device(d_text, pair, _t([])).numel() == 0
    for bad in ([0, len(text)], [-1, 0], [1 << 40], [2], [9]):  # outside the view; an end of the unanchored expression only; none
        for fn in (ctx.regex_anchored_starts_device, ctx.regex_anchored_ends_device):
            with pytest.raises(host.BmxError) as e:
                fn(d_text, pair, _t(bad))
            assert e.value.rc == host.ERR_ARG
    assert ctx.regex_starts_device(d_text, pair[0], _t([2])).cpu().tolist() == [0]  # (unanchored, a1b is a match)


def _log(lines=1500):
    rng = np.random.default_rng(2100)
    words = [b"ERROR: ", b"FATAL: ", b"INFO: ", b" ERROR: ", b"cat ", b"concat ", b"ERROR: 12 cat"]
    out = []
    for _ in range(lines):
        w = words[int(rng.integers(0, len(words)))]
        out.append(w + bytes(rng.integers(48, 58, int(rng.integers(0, 6))).astype(np.uint8)) +
                   (b"" if rng.integers(0, 2) else b" cat" + bytes(rng.integers(97, 100, int(rng.integers(0, 2))).astype(np.uint8))))
    return b"\n".join(out) + b"\n"


def test_grep_sub_findall(ctx):
    import torch

    text = _log()
    d_text = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
    lines = text.split(b"\n")[:-1]
    for expr, py in ((LOG, rb"^(?:ERROR|FATAL|PANIC): [0-9]{2,4}$"), (r"\bcat\b", rb"\bcat\b")):
        rx = re.compile(py, re.MULTILINE)
        want_rows = [i for i, ln in enumerate(lines) if rx.search(ln)]
        assert len(want_rows) > 50
        rows, counts = ctx.grep_device(d_text, expr, kind="regex_anchored")
        assert rows.cpu().tolist() == want_rows and counts.cpu().tolist() == [len(rx.findall(lines[i])) for i in want_rows]
        inv, none = ctx.grep_device(d_text, expr, kind="regex_anchored", invert=True)
        assert none is None and inv.cpu().tolist() == [i for i in range(len(lines)) if i not in set(want_rows)]
        # these matches cannot overlap and have one length per start: every selection coincides with re's
        for kw in ({}, {"posix": True}, {"rows": True}, {"posix": True, "rows": True}):
            assert host.findall(text, expr, kind="regex_anchored", **kw) == rx.findall(text), (expr, kw)
            assert host.sub(text, expr, b"<>", kind="regex_anchored", **kw) == rx.sub(b"<>", text), (expr, kw)
    g_rows, _ = host.grep(text, "cat", kind="regex_anchored", flags=host.REGEX_WORD)  # grep -w
    assert g_rows.tolist() == [i for i, ln in enumerate(lines) if re.search(rb"(?<!\w)cat(?!\w)", ln)]
    g_rows, _ = host.grep(text, "ERROR: [0-9]{2}", kind="regex_anchored", flags=host.REGEX_LINE)  # grep -x
    assert g_rows.tolist() == [i for i, ln in enumerate(lines) if re.fullmatch(rb"ERROR: [0-9]{2}", ln)] and g_rows.size > 5
    assert host.findall(b"ab abc\nabcd", r"\<[a-z]{1,3}", kind="regex_anchored", posix=True) == [b"ab", b"abc", b"abc"]
    assert host.findall(b"ab abc\nabcd", r"\<[a-z]{1,3}", kind="regex_anchored") == [b"a", b"a", b"a"]  # leftmost-shortest
    with pytest.raises(ValueError):
        host.sub(text, "a", b"", kind="regex_anchored", posix=True, merge=True)


def test_host_buffer_forms(ctx):
    text = _log(200)
    a = ao.from_lib(*host.compile_regex_anchored(r"\bcat\b|^ERROR: [0-9]{1,3}"))
    expr = r"\bcat\b|^ERROR: [0-9]{1,3}"
    e, s = ao.spans_numpy(text, a)
    assert e.size > 50
    assert np.array_equal(host.search_regex_anchored(text, expr).astype(np.int64), e)
    gs, ge = host.search_regex_anchored(text, expr, spans=True)
    assert np.array_equal(ge.astype(np.int64), e) and np.array_equal(gs.astype(np.int64), s)
    gs, ge = host.search_regex_anchored(text, expr, spans=True, longest=True)
    assert np.array_equal(gs.astype(np.int64), ao.spans_numpy(text, a, longest=True)[1])
    b, be = ao.begins_numpy(text, a, longest=True)
    assert np.array_equal(host.search_regex_anchored(text, expr, begins=True).astype(np.int64), b)
    gs, ge = host.search_regex_anchored(text, expr, begins=True, spans=True, longest=True)
    assert np.array_equal(gs.astype(np.int64), b) and np.array_equal(ge.astype(np.int64), be)
    assert np.array_equal(host.search_regex_anchored(b"cat concat\ncat", "cat", flags=host.REGEX_WORD), [2, 13])
    with pytest.raises(host.BmxError) as err:
        ctx.search_regex_anchored(text, expr, capacity=3)
    assert err.value.rc == host.ERR_CAPACITY
    ctx.search_regex_anchored_device(_dev(text, 1), expr)
    ctx.search_regex_anchored_begins_device(_dev(text, 1), expr)
    assert ctx.last_regex_anchored_ms() > 0 and ctx.last_regex_anchored_begins_ms() > 0


def test_on_a_callers_stream_behind_a_pending_copy(ctx):
    """As test_gpu_regex_begins.py: the view holds a decoy while the copy of the real text is outstanding on a non-blocking
    stream; the gate tables travel on the same stream in front of the launch."""
    import torch

    pair = host.compile_regex_anchored(LOG)
    a = ao.from_lib(*pair)
    rng = np.random.default_rng(78)
    real = _planted(rng, 1 << 20, KERNELS[1][1], KERNELS[1][2], 20000)
    decoy = _planted(rng, 1 << 20, KERNELS[1][1], KERNELS[1][2], 15000)
    want_e, want_s = ao.spans_numpy(real.tobytes(), a)
    want_b, want_be = ao.begins_numpy(real.tobytes(), a)
    assert want_e.size > 500 and not np.array_equal(want_e, ao.spans_numpy(decoy.tobytes(), a)[0])
    buf = torch.from_numpy(decoy.copy()).cuda()
    d_real = torch.from_numpy(real.copy()).cuda()
    out = torch.full((want_e.size + 64,), -1, dtype=torch.int64, device="cuda")
    outb = torch.full((want_e.size + 64,), -1, dtype=torch.int64, device="cuda")
    scratch = torch.zeros(2 << 28, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for i in range(64):
            x, y = (0, 1 << 28) if i & 1 else (1 << 28, 0)
            scratch[x:x + (1 << 28)].copy_(scratch[y:y + (1 << 28)], non_blocking=True)
        buf.copy_(d_real, non_blocking=True)
        pending = torch.cuda.Event()
        pending.record(s)
        assert not pending.query(), "the delay is too short: the producer had finished before the call"
        ends, total = ctx.search_regex_anchored_device(buf, pair, out=out, stream=s)
        starts = ctx.regex_anchored_starts_device(buf, pair, ends, stream=s)
        begins, totalb = ctx.search_regex_anchored_begins_device(buf, pair, out=outb, stream=s)
        bends = ctx.regex_anchored_ends_device(buf, pair, begins, stream=s)
    assert total == want_e.size and np.array_equal(ends.cpu().numpy(), want_e) and bool((out[total:] == -1).all())
    assert np.array_equal(starts.cpu().numpy(), want_s)
    assert totalb == want_b.size and np.array_equal(begins.cpu().numpy(), want_b) and np.array_equal(bends.cpu().numpy(), want_be)


def _cli(path, args, ok=True):
    exe = os.path.join(ROOT, host.__name__.split(".")[0], "bin", "bmx_cli")
    out = subprocess.run([exe, "--text", str(path)] + args, capture_output=True, timeout=120)
    assert (out.returncode == 0) == ok, out.stderr
    return out.stdout, out.stderr.decode()


def test_cli(tmp_path):
    text = b"cat concat\nERROR: 12\n ERROR: 34\nthe cat sat\nERROR: 567 cat\n"
    path = tmp_path / "t.txt"
    path.write_bytes(text)
    ends = [m.end() - 1 for m in re.finditer(rb"\bcat\b", text)]
    out, _ = _cli(path, ["--regex-anchored", r"\bcat\b", "--positions", "--iters", "1"])
    assert [int(l.split(b":")[1]) for l in out.split(b"\n") if l.startswith(b"End at")] == ends
    assert f"regex matches: {len(ends)}".encode() in out
    out, _ = _cli(path, ["--regex-anchored", "cat", "--word", "--starts", "--positions", "--iters", "0"])
    assert [tuple(map(int, l.split(b":")[1].split())) for l in out.split(b"\n") if l.startswith(b"Match at")] == [(e - 2, e) for e in ends]
    out, _ = _cli(path, ["--regex-anchored", "^ERROR: [0-9]{2,3}", "--begins", "--spans", "--longest", "--positions"])
    assert [tuple(map(int, l.split(b":")[1].split())) for l in out.split(b"\n") if l.startswith(b"Match at")] == [(11, 19), (44, 53)]
    out, _ = _cli(path, ["--regex-anchored", "ERROR: [0-9]{2}", "--line", "--only-matching"])
    assert out == b"ERROR: 12\n"
    out, _ = _cli(path, ["--regex-anchored", "^ERROR: [0-9]{1,3}", "--only-matching", "--posix", "--lines"])
    assert out == b"ERROR: 12\nERROR: 567\n"
    out, _ = _cli(path, ["--regex-anchored", r"\<cat\>", "--replace", "dog", "--posix"])
    assert out == re.sub(rb"\bcat\b", b"dog", text)
    _, err = _cli(path, ["--regex-anchored", r"a\bb"], ok=False)
    assert "bmx_compile_regex_anchored" in err
    _cli(path, ["--regex", "cat", "--word"], ok=False)
