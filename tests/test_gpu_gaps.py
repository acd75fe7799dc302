"""GPU suite for the gapped pattern search (bmx_search_gaps_device / bmx_search_gaps / bmx_gaps_starts_device /
bmx_cli --gaps): full lists compared with the numpy matcher (tests/gaps_oracle.py), with the class search where no
position is optional, and with the merged lists of the class search over every fixed-length variant of a pattern."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import classes_oracle as co
import gaps_oracle as go
from conftest import ROOT, golden_file_bytes
from parallel_implementation_of_string_matching_algorithms_opencl_amd import corpus, host

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "parallel_implementation_of_string_matching_algorithms_opencl_amd", "bin", "bmx_cli")
ZINC = "C-x(2,4)-C-x(3)-[LIVMFYWC]-x(8)-H-x(3,5)-H"


def piece(m: int) -> int:
    """The host's piece rule for a text far smaller than the resident lanes: 2^ps ends per lane with
    ps = max(6, ceil(log2(4 m))); a tile is 256 pieces."""
    return max(64, 1 << (4 * m - 1).bit_length())


def _dev(ctx, data, offset: int = 0):
    """data on the device, starting `offset` bytes into a buffer (any alignment)."""
    import torch

    data = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data
    buf = torch.zeros(data.size + offset + 16, dtype=torch.uint8, device=f"cuda:{ctx.device}")
    if data.size:
        buf[offset:offset + data.size] = torch.from_numpy(data.copy()).to(buf.device)
    return buf[offset:offset + data.size]


def _gpu(ctx, d_text, member, optional, **kw):
    n = kw.get("n", d_text.numel())
    cap = kw.pop("capacity", max(n, 1))
    ends, total = ctx.search_gaps_device(d_text, (co.pack(member), optional), capacity=cap, **kw)
    return ends.cpu().numpy().astype(np.int64), total


def _check(ctx, text, member, optional, offset: int = 0, starts: bool = False):
    text = bytes(text)
    want = go.gap_ends(text, member, optional)
    d_text = _dev(ctx, text, offset)
    got, total = _gpu(ctx, d_text, member, optional)
    assert total == want.size, (len(text), len(member), bin(optional), offset, total, want.size)
    assert np.array_equal(got, want), (len(text), len(member), bin(optional), offset)
    if starts and want.size:
        import torch

        d_ends = torch.from_numpy(want).to(d_text.device)
        for longest in (False, True):
            s = ctx.gaps_starts_device(d_text, (co.pack(member), optional), d_ends, longest=longest)
            assert np.array_equal(s.cpu().numpy(), go.gap_starts(text, member, optional, longest)[1]), (len(member), bin(optional), longest)
    return want


def _bits(*positions):
    return sum(1 << i for i in positions)


def test_random_cases_against_oracle(ctx):
    """300 patterns over 2, 4 and 95 symbols at the sixteen alignments of the view: the ends, and for every end the
    shortest and the longest match."""
    rng = np.random.default_rng(0x6A9500)
    hits = 0
    for case in range(300):
        sigma = (2, 4, 95)[case % 3]
        n = int(rng.integers(0, 5001)) if case % 10 else int(rng.integers(0, 70))  # every tenth: n around or below M
        base = 0x20 if sigma == 95 else 0x61
        symbols = np.arange(base, base + sigma)
        member, optional = go.random_pattern(rng, symbols, max_m=(8, 32, 64)[case % 7 % 3])
        text = (rng.integers(0, sigma, n) + base).astype(np.uint8)
        for _ in range(int(rng.integers(0, 4))):
            if n:
                go.plant(rng, text, member, optional, int(rng.integers(0, n)))
        hits += _check(ctx, text, member, optional, offset=case % 16, starts=True).size
    assert hits > 10000


def _random_bytes_member(rng, m):
    member = np.zeros((m, 256), dtype=bool)
    for i in range(m):
        member[i][rng.integers(0x80, 0x100, 3)] = True  # bytes >= 0x80 in every class
        member[i][rng.integers(0, 0x100, int(rng.integers(0, 120)))] = True
    return member


def test_word_switch_and_any_byte_values(ctx):
    rng = np.random.default_rng(72)
    for m in (1, 2, 31, 32, 33, 63, 64):
        text = rng.integers(0, 256, 6000).astype(np.uint8)
        member = _random_bytes_member(rng, m)
        optional = int(rng.integers(0, 1 << 62)) & ((1 << m) - 1) & ~(1 << (m // 3))
        for at in (0, 100, 3000, 5900):
            go.plant(rng, text, member, optional, at)
        want = _check(ctx, text, member, optional, offset=m % 16, starts=True)
        assert want.size >= 4
        if m > 1:
            empty = member.copy()
            empty[m // 2] = False  # an empty class: only matches that skip it are left
            _check(ctx, text, empty, optional | (1 << (m // 2)), offset=1, starts=True)
            _check(ctx, text, empty, optional & ~(1 << (m // 2)), offset=2)


@pytest.mark.parametrize("m", range(33, 65))
def test_block_across_the_half_word_boundary(ctx, m):
    """Shifted up by 64 - M, positions M - 33 and M - 32 sit in bits 31 and 32 of the word: an optional block over both
    makes the borrow of Df - I cross from the low half into the high half."""
    rng = np.random.default_rng(m)
    symbols = np.arange(0x61, 0x64)
    member = np.zeros((m, 256), dtype=bool)
    for i in range(m):
        member[i][rng.choice(symbols, int(rng.integers(1, 3)))] = True
    lo, hi = max(m - 34, 0), min(m - 31, m - 1)
    block = [i for i in range(lo, hi + 1)]
    if len(block) == m:
        block = block[1:]
    optional = _bits(*block)
    assert optional & (1 << (m - 33)) and optional & (1 << (m - 32))
    text = (rng.integers(0, 3, 8000) + 0x61).astype(np.uint8)
    at = 3
    for keep in range(1 << len(block)):  # every choice of the block's positions, planted once
        kept = {p for b, p in enumerate(block) if (keep >> b) & 1}
        at = go.plant(rng, text, member, optional, at, keep=kept) + int(rng.integers(0, 9))
    want = _check(ctx, text, member, optional, offset=m % 16, starts=True)
    assert want.size >= 1 << len(block)  # the copies are disjoint: each has an end of its own


@pytest.mark.parametrize("m", [3, 5, 32, 33, 64])
def test_block_shapes(ctx, m):
    """A block at position 0, a block that ends at position M - 1, two blocks with one mandatory position between them,
    and M - 1 optional positions around one mandatory."""
    rng = np.random.default_rng(100 + m)
    symbols = np.arange(0x61, 0x63)
    shapes = [_bits(0, 1), _bits(m - 2, m - 1), _bits(0, 2) if m == 3 else _bits(1, 2, 4, 5) & ((1 << m) - 1),
              ((1 << m) - 1) & ~(1 << (m // 2)), ((1 << m) - 1) & ~1, ((1 << m) - 1) & ~(1 << (m - 1))]
    for optional in shapes:
        member = np.zeros((m, 256), dtype=bool)
        for i in range(m):
            member[i][rng.choice(symbols, int(rng.integers(1, 3)))] = True
        text = (rng.integers(0, 2, 3000) + 0x61).astype(np.uint8)
        for at in range(5, 2900, 211):
            go.plant(rng, text, member, optional, at)
        want = _check(ctx, text, member, optional, offset=(m + 3) % 16, starts=True)
        assert want.size > 10, (m, bin(optional))


@pytest.mark.parametrize("m", [8, 16, 64])
def test_lengths_at_piece_and_tile_edges(ctx, m):
    p = piece(m)
    assert p == {8: 64, 16: 64, 64: 256}[m]
    rng = np.random.default_rng(m)
    symbols = np.arange(0x61, 0x65)
    member, optional = go.random_pattern(rng, symbols, max_m=m)
    while len(member) != m or not optional:
        member, optional = go.random_pattern(rng, symbols, max_m=m)
    member[~member.any(axis=1)] = True  # (no empty class here: the planted copies are whole)
    shortest = m - bin(optional).count("1")
    big = (rng.integers(0, 4, 3 * 256 * p + 5) + 0x61).astype(np.uint8)
    for at in range(0, big.size - m, 997):
        go.plant(rng, big, member, optional, at)
    for n in (0, 1, shortest - 1, shortest):  # views shorter than the shortest match, and one that holds exactly one
        got, total = _gpu(ctx, _dev(ctx, big[:n], 5), member, optional)
        want = go.gap_ends(big[:n].tobytes(), member, optional)
        assert total == want.size and np.array_equal(got, want) and (n >= shortest or total == 0)
    for n in (p - 1, p, p + 1, 256 * p - 1, 256 * p, 256 * p + 1, 3 * 256 * p + 5):
        for off in (0, 9):
            assert _check(ctx, big[:n], member, optional, offset=off).size > 0


def test_every_end_is_a_hit(ctx):
    """All wildcards, three of eight positions optional: every end from the fifth byte on.  Three tiles plus 5, each with
    eight times as many hits as the pool parks, so every tile walks twice.  The view begins 7 bytes into a 16-byte line:
    the bytes in front of it belong to a wildcard too, and no match may begin there (ends 0..3 are no hits)."""
    m = 8
    n = 3 * 256 * piece(m) + 5
    rng = np.random.default_rng(9)
    text = rng.integers(0, 256, n).astype(np.uint8)
    for optional in (_bits(5, 6, 7), _bits(0, 1, 2), _bits(1, 3, 6)):
        got, total = _gpu(ctx, _dev(ctx, text, 7), np.ones((m, 256), dtype=bool), optional)
        assert total == n - 4 and np.array_equal(got, np.arange(4, n))
    _, total = _gpu(ctx, _dev(ctx, text, 7), np.ones((m, 256), dtype=bool), _bits(5, 6, 7), capacity=0)
    assert total == n - 4


def test_dense_and_sparse_neighbour_tiles(ctx):
    rng = np.random.default_rng(6)
    n = corpus.MiB
    text = (rng.integers(0, 95, n) + 0x20).astype(np.uint8)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    for blk in range(0, n, 3 * 40000):  # dense stretches of ACGT that cut across tile boundaries
        text[blk:blk + 40000] = acgt[rng.integers(0, 4, min(40000, n - blk))]
    member, optional = go.parse("AN{3,6}", go.IUPAC)
    want = _check(ctx, text, member, optional, offset=4, starts=True)
    assert want.size > n // 12


def test_capacity_keeps_the_lowest_ends(ctx):
    import torch

    spec = corpus.CorpusSpec("gaps_cap", 2 * corpus.MiB, 12, 1, seed=0x5EED6A00, plant_period=1 << 12)
    text = spec.host_text().tobytes()
    member, optional = go.parse("ACN{1,3}GT", go.IUPAC)
    want = go.gap_ends(text, member, optional)
    total = want.size
    assert total > 5000  # more than a tile parks
    d_text = spec.device_text(ctx)
    cls = co.pack(member)
    for cap in (0, 1, total - 1, total // 2):
        out = torch.full((max(cap, 1),), -1, dtype=torch.int64, device=d_text.device)
        n_matches = C.c_uint64(0)
        rc = ctx._L.bmx_search_gaps_device(ctx._h, C.c_void_p(d_text.data_ptr()), d_text.numel(), 0, 0,
                                           C.c_void_p(cls.ctypes.data), len(member), optional, C.c_void_p(out.data_ptr()), cap,
                                           C.byref(n_matches), None)
        assert rc == host.ERR_CAPACITY and n_matches.value == total, (cap, rc, n_matches.value)
        if cap:
            assert np.array_equal(out.cpu().numpy(), want[:cap]), cap
        else:
            assert int(out[0].item()) == -1
    got, t = _gpu(ctx, d_text, member, optional, capacity=total)
    assert t == total and np.array_equal(got, want)
    with pytest.raises(host.BmxError):
        ctx.search_gaps(text, (cls, optional), capacity=3)


def test_lead_and_base_offset(ctx):
    rng = np.random.default_rng(4)
    text = (rng.integers(0, 2, 4000) + 0x61).astype(np.uint8).tobytes()
    member, optional = go.parse("a[ab]?b.{0,2}a")
    want = go.gap_ends(text, member, optional)
    assert want.size > 500
    d_text = _dev(ctx, text, 3)
    base = 10 ** 12 + 7
    for n, lead in ((4000, 0), (4000, 1), (4000, 5), (4000, 1234), (4000, 3999), (4000, 4000), (2000, 1990), (6, 2), (0, 0)):
        got, total = _gpu(ctx, d_text, member, optional, n=n, lead=lead, base_offset=base)
        w = want[(want >= lead) & (want < n)] + base  # matches may begin in front of lead, never end behind n
        assert total == w.size and np.array_equal(got, w), (n, lead)


def test_shards_concatenate_to_the_whole_list(ctx):
    spec = corpus.CorpusSpec("gaps_shards", 16 * corpus.MiB, 16, 1, seed=0x5EED6A01, plant_period=1 << 13,
                             boundary_period=1 << 20)
    d_text = spec.device_text(ctx)
    pat = spec.pattern().decode("latin-1")
    expr = pat[:3] + "N{0,2}" + pat[3:9] + ".?" + pat[10:]
    member, optional = go.parse(expr, go.IUPAC)
    m = len(member)
    n = d_text.numel()
    whole, whole_t = _gpu(ctx, d_text, member, optional)
    assert whole_t > 1000 and whole.size == whole_t
    cuts = [0, 3 * corpus.MiB + 3, 5 * corpus.MiB, 5 * corpus.MiB + 1, 11 * corpus.MiB + 12345, n]
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        begin = max(a - (m - 1), 0)  # the shard and its halo in front
        got, t = _gpu(ctx, d_text[begin:b], member, optional, lead=a - begin, base_offset=begin)
        parts.append(got)
    assert np.array_equal(np.concatenate(parts), whole)
    head = spec.host_text()[:corpus.MiB].tobytes()  # and the whole against the matcher on the first MiB
    assert np.array_equal(whole[whole < corpus.MiB], go.gap_ends(head, member, optional))


@pytest.mark.parametrize("kind", [0, 1])
def test_no_optional_position_is_the_class_search(ctx, kind):
    import torch

    for m in (1, 16, 32, 33, 64):
        spec = corpus.CorpusSpec(f"gaps_exact_{kind}_{m}", 16 * corpus.MiB + 5, m, kind, seed=0x5EED6A10 + m,
                                 plant_period=1 << 14, boundary_period=1 << 20)
        d_text = spec.device_text(ctx)
        member = co.singletons(spec.pattern())
        member[m // 2] = True  # one wildcard
        out = torch.empty(d_text.numel(), dtype=torch.int64, device=d_text.device)
        starts, total = ctx.search_classes_device(d_text, co.pack(member), out=out)
        ends, total_g = ctx.search_gaps_device(d_text, (co.pack(member), 0), capacity=max(total, 1))
        assert total_g == total >= 1000 and torch.equal(ends, starts + (m - 1)), (kind, m)


@pytest.mark.parametrize("expr,flags,count", [(ZINC, host.GAPS_PROSITE, 9), ("AC.{0,3}GT[AC].{0,3}TTG", 0, 16)])
def test_list_is_the_union_over_the_variants(ctx, expr, flags, count):
    """The second identity of include/bmx.h on a 16 MiB corpus with copies of every variant planted: one pass of the gaps
    kernel against one class-search pass per variant, merged."""
    import torch

    kind = 0 if flags else 1
    spec = corpus.CorpusSpec(f"gaps_union_{kind}", 16 * corpus.MiB, 16, kind, seed=0x5EED6A20 + kind, plant_period=1 << 14)
    classes, optional = host.compile_gaps(expr, flags)
    member = co.unpack(classes)
    vs = go.variants(member, optional)
    assert len(vs) == count
    text = spec.host_text().copy()
    rng = np.random.default_rng(17)
    opts = [i for i in range(len(member)) if (optional >> i) & 1]
    at = 1000
    for rep in range(40):
        for keep in range(1 << len(opts)):
            at = go.plant(rng, text, member, optional, at, keep={p for b, p in enumerate(opts) if (keep >> b) & 1}) + 4099
    assert at < text.size
    d_text = torch.from_numpy(text).to(f"cuda:{ctx.device}")
    lists = []
    for v in vs:
        starts, total = ctx.search_classes_device(d_text, co.pack(v), capacity=1 << 20)
        assert total == starts.numel()
        lists.append(starts + (len(v) - 1))
    want = torch.unique(torch.cat(lists))  # sorted, each end once
    ends, total = ctx.search_gaps_device(d_text, (classes, optional), capacity=1 << 20)
    assert total == want.numel() >= 40 * count and torch.equal(ends, want)
    s_short = ctx.gaps_starts_device(d_text, (classes, optional), ends)
    s_long = ctx.gaps_starts_device(d_text, (classes, optional), ends, longest=True)
    lens = {len(v) for v in vs}
    assert set((ends - s_short + 1).unique().tolist()) <= lens and set((ends - s_long + 1).unique().tolist()) <= lens
    assert bool((s_long <= s_short).all())


def test_starts_errors(ctx):
    import torch

    text = golden_file_bytes("input5L.txt.gz")
    d_text = _dev(ctx, text, 5)
    pair = host.compile_gaps("occur{1,2}ences?")
    ends, total = ctx.search_gaps_device(d_text, pair, capacity=len(text), base_offset=100)
    assert total > 100
    s = ctx.gaps_starts_device(d_text, pair, ends, base_offset=100)
    want_e, want_s = go.gap_starts(text, co.unpack(pair[0]), pair[1])
    assert np.array_equal(ends.cpu().numpy(), want_e + 100) and np.array_equal(s.cpu().numpy(), want_s + 100)
    for bad in (99, 100 + len(text)):  # an end outside [base_offset, base_offset + n)
        broken = ends.clone()
        broken[total // 2] = bad
        with pytest.raises(host.BmxError) as e:
            ctx.gaps_starts_device(d_text, pair, broken, base_offset=100)
        assert e.value.rc == host.ERR_ARG and "outside the view" in str(e.value)
    with pytest.raises(host.BmxError) as e:  # the list of another pattern
        ctx.gaps_starts_device(d_text, host.compile_gaps("zq?zzz"), ends, base_offset=100)
    assert e.value.rc == host.ERR_ARG and "no match" in str(e.value)
    assert ctx.gaps_starts_device(d_text, pair, ends[:0]).numel() == 0  # count == 0: no launch
    again = ctx.gaps_starts_device(d_text, pair, ends, base_offset=100)  # and the status word is clean again
    assert torch.equal(again, s)


def test_entry_points_and_the_cli(ctx, tmp_path):
    text = golden_file_bytes("input5L.txt.gz")
    path = tmp_path / "input5L.txt"
    path.write_bytes(text)
    cases = [("occur{1,2}ences?", 0, []), ("occurrences?", host.CLASS_ICASE, ["--icase"]), ("[Tt]he.{0,2}e", 0, []),
             ("t-x(1,3)-e-{a}", host.GAPS_PROSITE, ["--prosite"]), ("T-[Hh]-x(0,2)-e", host.GAPS_PROSITE | host.CLASS_ICASE, ["--prosite", "--icase"])]
    for expr, flags, opts in cases:
        member, optional = go.parse(expr, flags)
        want_e, want_s = go.gap_starts(text, member, optional)
        _, want_l = go.gap_starts(text, member, optional, longest=True)
        assert want_e.size > 50, expr
        assert np.array_equal(ctx.search_gaps(text, expr, flags).astype(np.int64), want_e)  # host entry point, expression
        assert np.array_equal(ctx.search_gaps(text, host.compile_gaps(expr, flags)).astype(np.int64), want_e)  # a pair
        assert np.array_equal(host.search_gaps(text, expr, flags).astype(np.int64), want_e)  # module level
        s, e = host.search_gaps(text, expr, flags, spans=True)
        assert np.array_equal(e.astype(np.int64), want_e) and np.array_equal(s.astype(np.int64), want_s)
        s, e = ctx.search_gaps_spans(text, expr, flags, longest=True)
        assert np.array_equal(e.astype(np.int64), want_e) and np.array_equal(s.astype(np.int64), want_l)
        ends, total = ctx.search_gaps_device(_dev(ctx, text, 5), expr, flags=flags, capacity=len(text))
        assert total == want_e.size and np.array_equal(ends.cpu().numpy().astype(np.int64), want_e)
        args = [CLI, "--gaps", expr, "--text", str(path), "--iters", "2", "--positions", "--max-print", "3"] + opts
        r = subprocess.run(args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert f"gapped matches: {want_e.size}" in r.stdout
        assert f"first end: {want_e[0]}\n" in r.stdout and f"last end: {want_e[-1]}\n" in r.stdout
        assert [int(x) for x in re.findall(r"End at : (\d+)", r.stdout)] == want_e[:3].tolist()
        assert "Average time" in r.stdout
        with_starts = ((["--starts"], want_s), (["--starts", "--longest"], want_l))
        for more, starts in with_starts if expr in (cases[0][0], cases[3][0]) else with_starts[:0]:
            r = subprocess.run(args + more, capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stderr
            got = [(int(a), int(b)) for a, b in re.findall(r"Match at : (\d+) (\d+)", r.stdout)]
            assert got == list(zip(starts[:3].tolist(), want_e[:3].tolist())), (expr, more)
    r = subprocess.run([CLI, "--gaps", "a*", "--text", str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "bad gapped pattern" in r.stderr


def test_on_a_callers_non_blocking_stream(ctx):
    """The rig of tests/test_gpu_streams.py: the buffers hold DECOYS (a text whose end list differs; for the starts pass a
    text and a list of ends whose starts differ), the caller's non-blocking stream holds a long delay and then the copies
    of the real inputs, and each entry is called while those copies are still outstanding.  A kernel, a clear of the
    look-back words or the ticket, or the starts pass's clear and copy of its status word that went to another stream
    would read the decoy."""
    import torch

    from test_gpu_streams import Pending, delay, side_stream

    text = golden_file_bytes("input5L.txt.gz")
    decoy = text.replace(b"he", b"eh")  # the same length, other ends
    pair = host.compile_gaps("[Tt]he.{0,2}e")
    member, optional = co.unpack(pair[0]), pair[1]
    want_e, want_s = go.gap_starts(text, member, optional)
    _, want_l = go.gap_starts(text, member, optional, longest=True)
    assert len(decoy) == len(text) and not np.array_equal(go.gap_ends(decoy, member, optional), want_e)
    assert want_e.size > 1000 and not np.array_equal(want_s[::-1], want_s)
    real_text = _dev(ctx, text, 0)
    real_ends = torch.from_numpy(want_e).to(real_text.device)
    out = torch.full((len(text),), -1, dtype=torch.int64, device=real_text.device)

    # the search, on a context of its own: its first call allocates and clears the look-back words and the ticket
    with host.Context(0) as fresh:
        for c, what in ((fresh, "search_gaps_device, first call of a context"), (ctx, "search_gaps_device")):
            d_text = _dev(ctx, decoy, 2)
            s = side_stream()
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                delay(s)
                d_text.copy_(real_text, non_blocking=True)
                pending = Pending(s)
                pending.assert_outstanding(what)
                ends, total = c.search_gaps_device(d_text, pair, out=out)
                taken = ends.clone()  # consumed on the stream
            assert total == want_e.size and np.array_equal(taken.cpu().numpy(), want_e), what

    # the starts: the text is a decoy and the list is the real one turned round (every entry a true end, other starts)
    for longest, want in ((False, want_s), (True, want_l)):
        d_text = _dev(ctx, decoy, 2)
        d_ends = real_ends.flip(0).contiguous()
        s = side_stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            delay(s)
            d_text.copy_(real_text, non_blocking=True)
            d_ends.copy_(real_ends, non_blocking=True)
            pending = Pending(s)
            pending.assert_outstanding("gaps_starts_device")
            got = ctx.gaps_starts_device(d_text, pair, d_ends, longest=longest)
        assert np.array_equal(got.cpu().numpy(), want), longest
    side = side_stream()  # and the stream as an argument, torch's current one being the null stream
    torch.cuda.synchronize()
    ends, total = ctx.search_gaps_device(real_text, pair, out=out, stream=side)
    got = ctx.gaps_starts_device(real_text, pair, ends, stream=side)
    assert total == want_e.size and np.array_equal(ends.cpu().numpy(), want_e) and np.array_equal(got.cpu().numpy(), want_s)


def test_repeat_calls_interleaved_with_the_other_searches(ctx):
    """The gaps, the class and the approximate search share the look-back code, not their state."""
    text = golden_file_bytes("input5L.txt.gz")
    d_text = _dev(ctx, text, 11)
    pair = host.compile_gaps("occur{1,2}ences?", host.CLASS_ICASE)
    member = co.parse("occurrences", co.ICASE)
    want = go.gap_ends(text, co.unpack(pair[0]), pair[1])
    want_c = co.class_starts(text, member)
    want_a, _ = co.class_approx_ends(text, member, 1)
    want_s, _ = co.class_approx_ends(text, co.singletons(b"occurrences"), 1)
    for _ in range(3):
        ends, t = ctx.search_gaps_device(d_text, pair, capacity=len(text))
        assert t == want.size and np.array_equal(ends.cpu().numpy(), want)
        assert ctx.last_gaps_ms() >= 0
        pos, t = ctx.search_classes_device(d_text, co.pack(member), capacity=len(text))
        assert t == want_c.size and np.array_equal(pos.cpu().numpy(), want_c)
        e, _, t = ctx.search_approx_classes_device(d_text, co.pack(member), 1, capacity=len(text))
        assert t == want_a.size and np.array_equal(e.cpu().numpy(), want_a)
        e, _, t = ctx.search_approx_device(d_text, b"occurrences", 1, capacity=len(text))
        assert t == want_s.size > 100 and np.array_equal(e.cpu().numpy(), want_s)
    assert set((want_c + 10).tolist()) <= set(want.tolist())
