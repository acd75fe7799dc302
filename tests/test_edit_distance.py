"""Edit distance (the reference's second algorithm, SURVEY.md s8 f1 / BASELINE config 5).

CPU part: the two-row oracle (oracle/ed_oracle.c) against golden distances produced by
the reference's own editDistDP (tests/golden/edit_distance.json) and against the
reference build.  GPU part: bmx_edit_distance through the C ABI against the same
fixtures, the oracle on seeded inputs around the tile edges, and size-independent
properties at 64k x 64k."""
import numpy as np
import pytest

from conftest import golden_file_bytes, load_golden
from golden import reference_runs


def _case_strings(case):
    if "a_file" in case:
        return golden_file_bytes(case["a_file"]), golden_file_bytes(case["b_file"])
    return case["a"].encode("latin-1"), case["b"].encode("latin-1")


# ------------------------------------------------------------------ CPU (oracle)
def test_oracle_matches_reference_editDistDP_golden(port):
    for case in load_golden("edit_distance.json"):
        a, b = _case_strings(case)
        assert port.edit_distance(a, b) == case["distance"], case.get("name", (case.get("a"), case.get("b")))


def test_survey_known_answers(port):
    cases = {c["name"]: c for c in load_golden("edit_distance.json") if "name" in c}
    assert cases["ED-1"]["distance"] == 522 and cases["ED-2"]["distance"] == 1044
    assert cases["ED-1"]["prefix_bytes"] == 3000 and cases["ED-2"]["prefix_bytes"] == 6000


def test_oracle_equals_reference_build_random(port, reference):
    """Against the reference build when it is present, and against its recorded answers (tests/golden/reference_runs.py)."""
    for (x, y), want in zip(reference_runs.edit_distance_pairs(), reference_runs.load("edit_distance"), strict=True):
        d = port.edit_distance(x, y)
        if reference is not None:
            assert d == reference.edit_distance(x, y)
        assert d == want


def test_oracle_metric_properties(port):
    rng = np.random.default_rng(1)
    for _ in range(30):
        x = (rng.integers(0, 4, int(rng.integers(1, 300))) + 65).astype(np.uint8)
        y = (rng.integers(0, 4, int(rng.integers(1, 300))) + 65).astype(np.uint8)
        d = port.edit_distance(x, y)
        assert d == port.edit_distance(y, x)
        assert abs(len(x) - len(y)) <= d <= max(len(x), len(y))
        assert port.edit_distance(x, x) == 0


def test_thresholded_oracle_agrees_with_the_full_oracle(port):
    """oracle.Port.edit_distance_within (the diagonal band -t <= c - r <= t + (la - lb), Ukkonen's cut-off) against the full
    two-row oracle: unrelated and related pairs up to 2,000 characters, either string the longer one, t below, at and above
    the distance.  It must say "more than t" (None) exactly when the distance is more than t."""
    rng = np.random.default_rng(41)
    pairs = []
    for it in range(240):
        la = int(rng.choice([1, 2, 3, 17, 64, 65, 300, 999, 2000])) if it % 3 else int(rng.integers(1, 2001))
        al = int(rng.integers(1, 5))
        x = (rng.integers(0, al, la) + 97).astype(np.uint8)
        kind = it % 4
        if kind == 0:  # unrelated, any two lengths
            y = (rng.integers(0, al, int(rng.integers(1, 2001))) + 97).astype(np.uint8)
        else:  # related: substitutions, deletions, inserted runs; kind 3 also cuts a piece out of the copy
            y = x.copy()
            y[rng.integers(0, la, int(rng.integers(0, la // 8 + 2)))] = ord("z")
            y = np.delete(y, rng.integers(0, y.size, int(rng.integers(0, la // 10 + 1))))
            for _ in range(int(rng.integers(0, 4))):
                at = int(rng.integers(0, y.size + 1))
                y = np.concatenate([y[:at], np.full(int(rng.integers(1, 40)), ord("y"), dtype=np.uint8), y[at:]])
            if kind == 3 and y.size > 4:
                lo = int(rng.integers(0, y.size // 2))
                y = y[lo:lo + int(rng.integers(1, y.size - lo + 1))]
            if y.size == 0:
                y = x[:1].copy()
        pairs.append((x, y))
    pairs += [(np.frombuffer(b"kitten", np.uint8), np.frombuffer(b"sitting", np.uint8)),
              (np.full(500, 97, np.uint8), np.full(500, 97, np.uint8)), (np.full(300, 97, np.uint8), np.full(200, 98, np.uint8))]
    n_within = n_more = 0
    for it, (x, y) in enumerate(pairs):
        d = port.edit_distance(x, y)
        for t in sorted({0, d // 2, max(d - 1, 0), d, d + 1, 2 * d + 3} | ({5000} if it % 8 == 0 else set())):  # (t = 5000: the whole table)
            for a, b in ((x, y), (y, x)):
                got = port.edit_distance_within(a, b, t)
                assert got == (d if d <= t else None), (x.size, y.size, d, t, got)
            n_within += d <= t
            n_more += d > t
    assert n_within > 500 and n_more > 300  # (both answers are exercised)


# ------------------------------------------------------------------ GPU
def _ctx_for(v, ctx, exp_ctx):
    """The product library builds schedule 13, 0 as its alias and their tiles (+16 / +32); every schedule that lost is
    libbmx_exp.so's alone (test_product_library_accepts_only_its_ed_schedules)."""
    return ctx if (v & ~48) in (0, 13) else exp_ctx


@pytest.mark.gpu
def test_gpu_golden(ctx):
    for case in load_golden("edit_distance.json"):
        a, b = _case_strings(case)
        assert ctx.edit_distance(a, b) == case["distance"], case.get("name", (case.get("a"), case.get("b")))


@pytest.mark.gpu
def test_gpu_vs_oracle_around_tile_edges_all_tile_shapes(ctx, exp_ctx, port):
    """Lengths straddling the tile width/height (64*C columns, R rows) of every tile shape,
    unequal lengths included (the reference itself is only right for equal lengths)."""
    rng = np.random.default_rng(7)
    lens = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1000, 1025]
    try:
        # 0: the library's own choice; 1..7: columns per lane (band pipeline, one launch); 8 / 9 / 10: the bit-parallel band (2048
        # columns per wave) with one / two / four rows per step; +32: tiles filled from both corners at once where there are three tile diagonals or more; +16:
        # tiles from the top-left corner only
        for v in [0, 8, 9, 10, 11, 12, 13, 2, 4, 7, 5, 32, 33, 34, 35, 16, 17, 18, 20]:
            c = _ctx_for(v, ctx, exp_ctx)
            c.set_ed_variant(v)
            for it in range(14 if v not in (8, 9, 10, 11, 12, 13) else 40):
                ls = lens if v not in (8, 9, 10, 11, 12, 13) else lens + [3, 4, 5, 31, 32, 33, 2016, 2047, 2048, 2049, 2080, 4095, 4097, 6200]
                la, lb = int(rng.choice(ls)), int(rng.choice(ls))
                al = int(rng.integers(2, 5))
                x = (rng.integers(0, al, la) + 97).astype(np.uint8)
                y = (rng.integers(0, al, lb) + 97).astype(np.uint8)
                assert c.edit_distance(x, y) == port.edit_distance(x, y), (v, la, lb)
    finally:
        ctx.set_ed_variant(0)


@pytest.mark.gpu
def test_gpu_two_ended_schedule_on_every_grid_shape(exp_ctx, port):
    """The forward and the mirrored half meet on a staircase of tile edges: grids of 1..9 x
    1..9 tiles (128 x 256 tiles, variant 1: a tile shape of libbmx_exp.so), full and ragged last tiles, strings that are
    related (long shared runs: the optimal path hugs the diagonal) and unrelated."""
    rng = np.random.default_rng(11)
    ctx = exp_ctx
    ctx.set_ed_variant(33)
    try:
        for tr in (1, 2, 3, 5, 9):
            for tc in (1, 2, 3, 4, 7):
                for ragged in (False, True):
                    lb = tr * 128 - (int(rng.integers(1, 128)) if ragged else 0)
                    la = tc * 256 - (int(rng.integers(1, 256)) if ragged else 0)
                    x = (rng.integers(0, 3, la) + 97).astype(np.uint8)
                    if rng.integers(0, 2):  # related: y is an edited copy of x, cut or padded to lb
                        y = x.copy()
                        y[rng.integers(0, la, la // 9 + 1)] = ord("z")
                        y = np.delete(y, rng.integers(0, la, la // 17 + 1))
                        y = np.resize(y, lb) if y.size >= lb else np.concatenate(
                            [y, (rng.integers(0, 3, lb - y.size) + 97).astype(np.uint8)])
                    else:
                        y = (rng.integers(0, 3, lb) + 97).astype(np.uint8)
                    want = port.edit_distance(x, y)
                    assert ctx.edit_distance(x, y) == want, (tr, tc, la, lb)
                    assert ctx.edit_distance(y, x) == want, (tc, tr, lb, la)
    finally:
        ctx.set_ed_variant(0)


@pytest.mark.gpu
def test_gpu_band_pipeline_cut_shapes(exp_ctx, port):
    """The band pipeline's two directions meet on a staircase whose step is set by the assumed
    lag between neighbouring bands: tiny lag = one flat cut row, huge lag = one direction does
    whole bands alone (cut clipped to 0 / lb), in between = a real staircase."""
    rng = np.random.default_rng(13)
    shapes = [(1, 1), (70, 300), (300, 70), (257, 256), (256, 257), (1000, 1500), (1500, 1000), (3000, 513),
              (513, 3000), (2048, 2048)]
    shapes = shapes + [(5000, 900), (900, 5000), (4096, 4096), (6500, 2049)]  # (several bands of the bit-parallel kernel: 2048 columns each)
    for lag, variant in [(l, v) for v in (0, 4, 8, 9, 10, 11, 12, 13) for l in ("0", "3", "64", "200", "700", "100000")]:
        exp_ctx.set_knob("ed_lag", int(lag))  # (a switch of libbmx_exp.so: the product library assumes its measured lag)
        exp_ctx.set_ed_variant(variant)       # (0: the library's choice; 4: bands of 384 columns; 8 / 9 / 10: bit-parallel bands, 1 / 2 / 4 rows per step)
        ctx = exp_ctx
        for grp in ((32, 16) if variant >= 11 else (32,)):  # (the other hand-over group: another kernel instance of these)
            exp_ctx.set_knob("ed_group", grp)
            for la, lb in shapes:
                x = (rng.integers(0, 3, la) + 97).astype(np.uint8)
                y = (rng.integers(0, 3, lb) + 97).astype(np.uint8)
                if la == lb:
                    y = x.copy()
                    y[rng.integers(0, la, la // 7 + 1)] = ord("q")
                assert ctx.edit_distance(x, y) == port.edit_distance(x, y), (lag, variant, grp, la, lb)
        exp_ctx.set_knob("ed_group", 32)


@pytest.mark.gpu
def test_gpu_degenerate(ctx):
    assert ctx.edit_distance(b"", b"") == 0
    assert ctx.edit_distance(b"", b"abc") == 3
    assert ctx.edit_distance(b"abcd", b"") == 4
    assert ctx.edit_distance(b"kitten", b"sitting") == 3
    assert ctx.edit_distance(b"a" * 3000, b"a" * 3000) == 0
    assert ctx.edit_distance(b"a" * 3000, b"b" * 2000) == 3000


@pytest.mark.gpu
def test_gpu_every_byte_value_on_the_bit_parallel_bands(ctx, exp_ctx, port):
    """The bit-parallel bands index their Eq table by the character: all 256 byte values, NUL and 0xff included, on shapes with a
    narrow last band, fewer rows than a group, rows that are not whole steps, and a band whose lanes have not all started when the
    rows end (schedules 13 = the default, 11, 9)."""
    rng = np.random.default_rng(29)
    shapes = [(2048, 2048), (2049, 5), (4096 + 33, 127), (300, 4097), (6145, 2047), (70, 70), (2047, 129), (5000, 63)]
    try:
        for v in (13, 11, 9, 0):
            c = _ctx_for(v, ctx, exp_ctx)
            c.set_ed_variant(v)
            for la, lb in shapes:
                x = rng.integers(0, 256, la).astype(np.uint8)
                y = rng.integers(0, 256, lb).astype(np.uint8)
                k = min(la, lb)
                y[: k // 2] = x[: k // 2]  # (a long common prefix: the distance is not just max(la, lb))
                x[la // 3] = 0
                y[lb // 2] = 0
                x[-1] = 255
                assert c.edit_distance(x, y) == port.edit_distance(x, y), (v, la, lb)
    finally:
        ctx.set_ed_variant(0)


@pytest.mark.gpu
def test_gpu_mid_size_vs_oracle(ctx, port):
    rng = np.random.default_rng(3)
    x = (rng.integers(0, 4, 9000) + 65).astype(np.uint8)
    y = x.copy()
    y[rng.integers(0, 9000, 700)] = ord("N")       # substitutions
    y = np.delete(y, rng.integers(0, 9000, 200))   # deletions
    assert ctx.edit_distance(x, y) == port.edit_distance(x, y)
    z = (rng.integers(0, 4, 7777) + 65).astype(np.uint8)
    assert ctx.edit_distance(x, z) == port.edit_distance(x, z)


@pytest.mark.gpu
def test_gpu_config5_64k_properties(ctx, exp_ctx, port):
    """BASELINE config 5: 64k x 64k.  Known-by-construction answers plus one full
    comparison with the two-row oracle (13 s of CPU)."""
    import torch

    n = 65536
    rng = np.random.default_rng(5)
    x = (rng.integers(0, 4, n) + 65).astype(np.uint8)
    dx = torch.from_numpy(x).cuda()
    assert ctx.edit_distance_device(dx, dx) == 0
    # k substitutions at distinct positions with a fifth symbol: distance is exactly k
    y = x.copy()
    pos = rng.choice(n, 1000, replace=False)
    y[pos] = ord("N")
    assert ctx.edit_distance_device(dx, torch.from_numpy(y).cuda()) == 1000
    # symmetry on unrelated strings, then the oracle
    z = (rng.integers(0, 4, n) + 65).astype(np.uint8)
    dz = torch.from_numpy(z).cuda()
    d1 = ctx.edit_distance_device(dx, dz)
    assert d1 == ctx.edit_distance_device(dz, dx)
    try:
        for v in (16, 32, 4, 8, 9, 10, 11, 12, 13):  # tiles from one corner (the first schedule) / from both corners; value bands; bit-parallel bands
            c = _ctx_for(v, ctx, exp_ctx)
            c.set_ed_variant(v)
            assert d1 == c.edit_distance_device(dx, dz)
    finally:
        ctx.set_ed_variant(0)
    assert d1 == port.edit_distance(x, z)


@pytest.mark.gpu
def test_product_library_accepts_only_its_ed_schedules(ctx, exp_ctx):
    """bmx_set_ed_variant follows the scan kernels' rule (test_gpu_parity.py::test_product_library_accepts_only_its_variants):
    libbmx.so builds schedule 13, slot 0 as its alias and their tiles behind +16 / +32, and refuses every other slot with
    BMX_ERR_ARG; libbmx_exp.so accepts all fourteen.  No kernel runs."""
    from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

    def refused(c, v):
        with pytest.raises(host.BmxError) as e:
            c.set_ed_variant(v)
        return e.value.rc == host.ERR_ARG

    try:
        for base in range(14):
            for flags in (0, 16, 32, 48):
                if base in (0, 13):
                    ctx.set_ed_variant(base + flags)
                else:
                    assert refused(ctx, base + flags), (base, flags)
                exp_ctx.set_ed_variant(base + flags)
        for v in [b + f for b in (14, 20) for f in (0, 16, 32, 48)] + [14, 27, -1]:
            assert refused(ctx, v), v
    finally:
        ctx.set_ed_variant(0)


@pytest.mark.gpu
def test_edit_distance_leaves_the_scan_history_alone(built, port):
    """The edit distance times itself with events of its own.  It used to re-record the scan history's next ring slot,
    which -- once 64 scans had been timed -- is the history's oldest entry: [63] then read the edit distance's time.
    Elapsed times of recorded events do not change, so all 64 floats are bit-equal before and after."""
    from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

    rng = np.random.default_rng(43)
    text = (rng.integers(0, 26, 64 * 1024) + 97).astype(np.uint8)
    with host.Context(0) as c:
        for _ in range(70):  # (the ring of 64 has wrapped)
            c.search(text, b"abcd")
        before = np.asarray(c.scan_ms_history(64), dtype=np.float32)
        last = c.last_scan_ms()
        assert before.size == 64
        try:
            for v, la, lb in ((0, 300, 70), (0, 3000, 3000), (32, 600, 600)):  # band path twice, then the tile path
                c.set_ed_variant(v)
                x = (rng.integers(0, 4, la) + 97).astype(np.uint8)
                y = (rng.integers(0, 4, lb) + 97).astype(np.uint8)
                assert c.edit_distance(x, y) == port.edit_distance(x, y), (v, la, lb)
        finally:
            c.set_ed_variant(0)
        after = np.asarray(c.scan_ms_history(64), dtype=np.float32)
        assert before.tobytes() == after.tobytes(), np.flatnonzero(before != after)
        assert c.last_scan_ms() == last
