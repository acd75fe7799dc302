"""GPU suite for the class-pattern search (bmx_search_classes_device / bmx_search_classes / bmx_cli --classes) and the
approximate search with classes (bmx_search_approx_classes_device): full lists compared with the numpy oracle
(tests/classes_oracle.py), with the exact search for singleton classes and with the approximate search for strings."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import classes_oracle as co
from conftest import ROOT, golden_file_bytes
from parallel_implementation_of_string_matching_algorithms_opencl_amd import corpus, host

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "parallel_implementation_of_string_matching_algorithms_opencl_amd", "bin", "bmx_cli")
PRIMER = "GTGYCAGCMGCCGCGGTAA"


def piece(m: int) -> int:
    """The host's piece rule (bmx_internal_classes_piece_shift) for a text far smaller than the resident lanes: 2^ps ends
    per lane with ps = max(6, ceil(log2(4 m))); a tile is 256 pieces."""
    return max(64, 1 << (4 * m - 1).bit_length())


def _dev(ctx, data: bytes, offset: int = 0):
    """data on the device, starting `offset` bytes into a buffer (any alignment)."""
    import torch

    buf = torch.zeros(len(data) + offset + 16, dtype=torch.uint8, device=f"cuda:{ctx.device}")
    if data:
        buf[offset:offset + len(data)] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(buf.device)
    return buf[offset:offset + len(data)] if data else buf[offset:offset]


def _gpu(ctx, d_text, member, **kw):
    n = kw.get("n", d_text.numel())
    cap = kw.pop("capacity", max(n, 1))
    pos, total = ctx.search_classes_device(d_text, co.pack(member), capacity=cap, **kw)
    return pos.cpu().numpy().astype(np.int64), total


def _check(ctx, text: bytes, member, offset: int = 0):
    want = co.class_starts(text, member)
    got, total = _gpu(ctx, _dev(ctx, text, offset), member)
    assert total == want.size, (len(text), len(member), offset, total, want.size)
    assert np.array_equal(got, want), (len(text), len(member), offset)


def _random_member(rng, m, symbols):
    """Per position a random singleton, a 2-4 member set, any, or a negated singleton."""
    member = np.zeros((m, 256), dtype=bool)
    for i in range(m):
        kind = int(rng.integers(0, 4))
        if kind == 0:
            member[i][rng.choice(symbols)] = True
        elif kind == 1:
            member[i][rng.choice(symbols, int(rng.integers(2, 5)))] = True
        elif kind == 2:
            member[i] = True
        else:
            member[i] = True
            member[i][rng.choice(symbols)] = False
    return member


def _plant(rng, text, member, at):
    """Overwrite text[at : at + m) with a member of every class."""
    for i in range(member.shape[0]):
        text[at + i] = rng.choice(np.nonzero(member[i])[0])


def test_random_cases_against_oracle(ctx):
    rng = np.random.default_rng(0xC1A5500)
    for case in range(300):
        sigma = (2, 4, 95)[case % 3]
        n = int(rng.integers(0, 5001)) if case % 10 else int(rng.integers(0, 70))  # every tenth: n around or below m
        m = int(rng.integers(1, 65))
        base = 0x20 if sigma == 95 else 0x61
        symbols = np.arange(base, base + sigma)
        text = (rng.integers(0, sigma, n) + base).astype(np.uint8)
        member = _random_member(rng, m, symbols)
        if n > m and rng.integers(0, 2):
            _plant(rng, text, member, int(rng.integers(0, n - m + 1)))
        _check(ctx, text.tobytes(), member, offset=case % 16)


def test_word_switch_and_any_byte_values(ctx):
    rng = np.random.default_rng(71)
    text = rng.integers(0, 256, 6000).astype(np.uint8)
    for m in (1, 2, 31, 32, 33, 63, 64):
        member = np.zeros((m, 256), dtype=bool)
        for i in range(m):
            member[i][rng.integers(0x80, 0x100, 3)] = True  # bytes >= 0x80 in every class
            member[i][rng.integers(0, 0x100, int(rng.integers(0, 120)))] = True
        for at in (0, 100, 3000, 6000 - m):
            _plant(rng, text, member, at)
        want = co.class_starts(text.tobytes(), member)
        assert {0, 100, 3000, 6000 - m} <= set(want.tolist())
        _check(ctx, text.tobytes(), member, offset=m % 16)
        empty = member.copy()
        empty[m // 2] = False  # an empty class matches nothing
        _check(ctx, text.tobytes(), empty, offset=1)


@pytest.mark.parametrize("kind", [0, 1])
def test_singletons_equal_exact_search(ctx, port, kind):
    import torch

    for m in (1, 8, 16, 32, 33, 64):
        spec = corpus.CorpusSpec(f"classes_exact_{kind}_{m}", 16 * corpus.MiB + 5, m, kind, seed=0x5EEDC000 + m,
                                 plant_period=1 << 14, boundary_period=1 << 20)
        d_text = spec.device_text(ctx)
        pat = spec.pattern()
        want = port.search(spec.host_text(), pat).astype(np.int64)
        pos, total = ctx.search_device(d_text, pat, capacity=d_text.numel())
        assert total == want.size and np.array_equal(pos.cpu().numpy().astype(np.int64), want)
        out = torch.empty(max(want.size, 1), dtype=torch.int64, device=d_text.device)
        got, total = ctx.search_classes_device(d_text, co.pack(co.singletons(pat)), out=out)
        assert total == want.size, (kind, m)
        assert np.array_equal(got.cpu().numpy().astype(np.int64), want), (kind, m)


def test_dense_tiles_walk_twice(ctx):
    m = 8
    n = 3 * 256 * piece(m) + 5  # three tiles plus 5
    rng = np.random.default_rng(8)
    text = rng.integers(0, 256, n).astype(np.uint8).tobytes()
    got, total = _gpu(ctx, _dev(ctx, text, 7), np.ones((m, 256), dtype=bool))
    assert total == n - m + 1 and np.array_equal(got, np.arange(n - m + 1))


def test_dense_and_sparse_neighbour_tiles(ctx):
    rng = np.random.default_rng(5)
    n = 3 * corpus.MiB
    text = (rng.integers(0, 95, n) + 0x20).astype(np.uint8)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    for blk in range(0, n, 3 * 40000):  # dense stretches of ACGT that cut across tile boundaries
        text[blk:blk + 40000] = acgt[rng.integers(0, 4, min(40000, n - blk))]
    member = co.parse("NNNNNNNN", co.IUPAC)  # every window inside a stretch is a hit
    assert co.class_starts(text.tobytes(), member).size > n // 4
    _check(ctx, text.tobytes(), member, offset=4)


@pytest.mark.parametrize("m", [8, 16, 64])
def test_lengths_at_piece_and_tile_edges(ctx, m):
    p = piece(m)
    assert p == {8: 64, 16: 64, 64: 256}[m]
    rng = np.random.default_rng(m)
    member = _random_member(rng, m, np.arange(0x61, 0x65))
    big = (rng.integers(0, 4, 256 * p + 64) + 0x61).astype(np.uint8)
    for at in range(0, big.size - m, 997):
        _plant(rng, big, member, at)
    for n in (p - 1, p, p + 1, 256 * p - 1, 256 * p, 256 * p + 1, 256 * p + m - 1, 256 * p + m):
        for off in (0, 9):
            _check(ctx, big[:n].tobytes(), member, offset=off)


def test_small_and_shifted_views(ctx):
    rng = np.random.default_rng(3)
    text = (rng.integers(0, 2, 4000) + 0x61).astype(np.uint8).tobytes()
    member = co.parse("a[ab]b.a")
    m = 5
    want = co.class_starts(text, member)
    assert want.size > 100
    d_text = _dev(ctx, text, 3)
    for n in (0, 1, m - 1):  # n < m: nothing fits
        got, total = _gpu(ctx, d_text, member, n=n)
        assert total == 0 and got.size == 0
    got, total = _gpu(ctx, d_text, member, n=m)  # n == m: one window
    assert got.tolist() == want[want < 1].tolist() and total == got.size
    for n, n_own in ((4000, 0), (4000, 1), (4000, 1234), (4000, 3996), (4000, 3997), (4000, 4000), (2000, 1990), (2000, 5000)):
        got, total = _gpu(ctx, d_text, member, n=n, n_own=n_own, base_offset=10 ** 12 + 7)
        w = want[(want < n_own) & (want + m <= n)] + 10 ** 12 + 7
        assert total == w.size and np.array_equal(got, w), (n, n_own)


def test_capacity_keeps_the_lowest_starts(ctx):
    import torch

    spec = corpus.CorpusSpec("classes_cap", 2 * corpus.MiB, 12, 1, seed=0x5EEDC200, plant_period=1 << 12)
    text = spec.host_text().tobytes()
    member = co.parse("ACNNGT", co.IUPAC)
    want = co.class_starts(text, member)
    total = want.size
    assert total > 5000  # more than a tile parks
    d_text = spec.device_text(ctx)
    cls = co.pack(member)
    for cap in (0, 1, total - 1, total // 2):
        out = torch.full((max(cap, 1),), -1, dtype=torch.int64, device=d_text.device)
        n_matches = C.c_uint64(0)
        rc = ctx._L.bmx_search_classes_device(ctx._h, C.c_void_p(d_text.data_ptr()), d_text.numel(), d_text.numel(), 0,
                                              C.c_void_p(cls.ctypes.data), 6, C.c_void_p(out.data_ptr()), cap,
                                              C.byref(n_matches), None)
        assert rc == host.ERR_CAPACITY and n_matches.value == total, (cap, rc, n_matches.value)
        if cap:
            assert np.array_equal(out.cpu().numpy(), want[:cap]), cap
        else:
            assert int(out[0].item()) == -1
    got, t = _gpu(ctx, d_text, member, capacity=total)
    assert t == total and np.array_equal(got, want)


def test_shards_concatenate_to_the_whole_list(ctx):
    spec = corpus.CorpusSpec("classes_shards", 16 * corpus.MiB, 16, 1, seed=0x5EEDC300, plant_period=1 << 13,
                             boundary_period=1 << 20)
    d_text = spec.device_text(ctx)
    pat = spec.pattern().decode("latin-1")
    expr = pat[:3] + "N" + pat[4:9] + "." + pat[10:]
    member = co.parse(expr, co.IUPAC)
    m = 16
    n = d_text.numel()
    whole, whole_t = _gpu(ctx, d_text, member)
    assert whole_t > 1000 and np.array_equal(whole, co.class_starts(spec.host_text().tobytes(), member))
    cuts = [0, 3 * corpus.MiB + 3, 5 * corpus.MiB, 5 * corpus.MiB + 1, 11 * corpus.MiB + 12345, n]
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        view = d_text[a:min(b + m - 1, n)]  # the shard and its halo
        got, t = _gpu(ctx, view, member, n_own=b - a, base_offset=a)
        parts.append(got)
    assert np.array_equal(np.concatenate(parts), whole)


def test_entry_points_and_the_cli(ctx, tmp_path):
    text = golden_file_bytes("input5L.txt.gz")
    cases = [("occurrences", 0), ("occurrences", host.CLASS_ICASE), ("[Tt]he", 0), ("t.e", host.CLASS_ICASE)]
    (tmp_path / "input5L.txt").write_bytes(text)
    for expr, flags in cases:
        want = co.class_starts(text, co.parse(expr, flags))
        assert want.size > 100
        assert np.array_equal(ctx.search_classes(text, expr, flags).astype(np.int64), want)  # host entry point, expression
        assert np.array_equal(ctx.search_classes(text, host.compile_classes(expr, flags)).astype(np.int64), want)  # classes
        assert np.array_equal(host.search_classes(text, expr, flags).astype(np.int64), want)  # module level
        pos, total = ctx.search_classes_device(_dev(ctx, text, 5), expr, flags=flags, capacity=len(text))
        assert total == want.size and np.array_equal(pos.cpu().numpy().astype(np.int64), want)
        args = [CLI, "--classes", expr, "--text", str(tmp_path / "input5L.txt"), "--iters", "2", "--positions", "--max-print", "3"]
        r = subprocess.run(args + (["--icase"] if flags else []), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert f"class matches: {want.size}" in r.stdout
        assert f"first start: {want[0]}\n" in r.stdout and f"last start: {want[-1]}\n" in r.stdout
        assert [int(x) for x in re.findall(r"Start at : (\d+)", r.stdout)] == want[:3].tolist()
        assert "Average time" in r.stdout
    with pytest.raises(host.BmxError):
        ctx.search_classes(text, "occurrences", capacity=3)
    # the CLI's approximate search with classes prints what --approx prints
    ends, dists = co.class_approx_ends(text, co.parse("occurrences", co.ICASE), 1)
    r = subprocess.run([CLI, "--classes", "occurrences", "--icase", "--approx", "1", "--text", str(tmp_path / "input5L.txt"),
                        "--iters", "1", "--positions", "--max-print", "3"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert f"approximate matches (k = 1): {ends.size}" in r.stdout
    assert f"first end: {ends[0]} (distance {dists[0]})" in r.stdout and f"last end: {ends[-1]} (distance {dists[-1]})" in r.stdout
    got = [(int(a), int(b)) for a, b in re.findall(r"End at : (\d+) \(distance (\d+)\)", r.stdout)]
    assert got == list(zip(ends[:3].tolist(), dists[:3].tolist()))


def test_on_a_callers_non_blocking_stream(ctx):
    import torch

    text = golden_file_bytes("input5L.txt.gz")
    want = co.class_starts(text, co.parse("[Tt]he"))
    d_text = _dev(ctx, text, 2)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    pos, total = ctx.search_classes_device(d_text, "[Tt]he", capacity=len(text), stream=side)
    assert total == want.size and np.array_equal(pos.cpu().numpy().astype(np.int64), want)
    with torch.cuda.stream(side):  # and as torch's current stream
        pos, total = ctx.search_classes_device(d_text, "[Tt]he", capacity=len(text))
    assert total == want.size and np.array_equal(pos.cpu().numpy().astype(np.int64), want)
    member = co.parse("occurrences", co.ICASE)  # the approximate search with classes on the same stream
    want_e, want_d = co.class_approx_ends(text, member, 1)
    e, d, total = ctx.search_approx_classes_device(d_text, co.pack(member), 1, capacity=len(text), stream=side)
    assert total == want_e.size and np.array_equal(e.cpu().numpy().astype(np.int64), want_e)
    assert np.array_equal(d.cpu().numpy().astype(np.int64), want_d)
    e2, d2 = _approx_host(ctx, text, member, 1)  # and the host-buffer entry point
    assert np.array_equal(e2, want_e) and np.array_equal(d2, want_d)


def test_repeat_calls(ctx):
    text = golden_file_bytes("input5L.txt.gz")
    d_text = _dev(ctx, text, 11)
    member = co.parse("occurrences", co.ICASE)
    first, t1 = _gpu(ctx, d_text, member)
    for _ in range(3):
        again, t2 = _gpu(ctx, d_text, member)
        assert t1 == t2 and np.array_equal(first, again)
        assert ctx.last_classes_ms() >= 0
    assert np.array_equal(first, co.class_starts(text, member))


# ---- approximate search with classes ----------------------------------------------------------------------------------

def _approx(ctx, d_text, member, k):
    n = max(d_text.numel(), 1)
    e, d, total = ctx.search_approx_classes_device(d_text, co.pack(member), k, capacity=n)
    return e.cpu().numpy().astype(np.int64), d.cpu().numpy().astype(np.int64), total


def _approx_host(ctx, text, member, k):
    """bmx_search_approx_classes: host buffers in and out."""
    cls = co.pack(member)
    ends = np.empty(max(len(text), 1), np.uint64)
    dist = np.empty(max(len(text), 1), np.uint8)
    total = C.c_uint64(0)
    rc = ctx._L.bmx_search_approx_classes(ctx._h, text, len(text), C.c_void_p(cls.ctypes.data), cls.shape[0], k,
                                          C.c_void_p(ends.ctypes.data), C.c_void_p(dist.ctypes.data), ends.size, C.byref(total))
    assert rc == host.OK
    return ends[:total.value].astype(np.int64), dist[:total.value].astype(np.int64)


def test_approx_random_cases_against_oracle(ctx):
    rng = np.random.default_rng(0xC1A5501)
    for case in range(100):
        sigma = (2, 4, 95)[case % 3]
        n = int(rng.integers(0, 3001)) if case % 10 else int(rng.integers(0, 70))
        m = int(rng.integers(1, 65))
        k = int(rng.integers(0, m))
        base = 0x20 if sigma == 95 else 0x61
        symbols = np.arange(base, base + sigma)
        text = (rng.integers(0, sigma, n) + base).astype(np.uint8)
        member = _random_member(rng, m, symbols)
        if n > m and rng.integers(0, 2):
            _plant(rng, text, member, int(rng.integers(0, n - m + 1)))
        want_e, want_d = co.class_approx_ends(text.tobytes(), member, k)
        e, d, total = _approx(ctx, _dev(ctx, text.tobytes(), case % 16), member, k)
        assert total == want_e.size and np.array_equal(e, want_e) and np.array_equal(d, want_d), (case, n, m, k)
        if k == 0 or case % 5 == 0:  # k = 0: the class starts + m - 1
            e0, d0, _ = _approx(ctx, _dev(ctx, text.tobytes(), 3), member, 0)
            assert np.array_equal(e0, co.class_starts(text.tobytes(), member) + m - 1) and not d0.any()
            got, _ = _gpu(ctx, _dev(ctx, text.tobytes(), 3), member)
            assert np.array_equal(e0, got + m - 1)


def test_approx_singletons_equal_the_string_entry_point(ctx):
    rng = np.random.default_rng(12)
    text = (rng.integers(0, 4, 200000) + 0x61).astype(np.uint8)
    d_text = _dev(ctx, text.tobytes(), 6)
    for m, k in ((1, 0), (8, 2), (32, 5), (33, 5), (64, 20)):
        pat = text[7000:7000 + m].tobytes()
        e1, d1, t1 = ctx.search_approx_device(d_text, pat, k, capacity=text.size)
        e2, d2, t2 = _approx(ctx, d_text, co.singletons(pat), k)
        assert t1 == t2 > 0 and np.array_equal(e1.cpu().numpy(), e2) and np.array_equal(d1.cpu().numpy(), d2), (m, k)


def test_approx_degenerate_primer_with_planted_substitutions(ctx):
    rng = np.random.default_rng(16)
    member = co.parse(PRIMER, co.IUPAC)
    m, k = len(PRIMER), 2
    n = 1 << 20
    text = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].copy()
    planted = []
    for j, at in enumerate(range(1000, n - 1000, 4099)):
        _plant(rng, text, member, at)
        subs = j % (k + 2)  # 0 .. k + 1 substitutions, each to a base outside the class
        for i in rng.choice(m, subs, replace=False):
            text[at + i] = rng.choice([b for b in b"ACGT" if not member[i][b]])
        planted.append((at, subs))
    want_e, want_d = co.class_approx_ends(text.tobytes(), member, k)
    by_end = dict(zip(want_e.tolist(), want_d.tolist()))
    for at, subs in planted:  # a copy is reported at its end with exactly its substitutions, or not at all beyond k
        assert by_end.get(at + m - 1, k + 1) == min(subs, k + 1), (at, subs)
    e, d, total = _approx(ctx, _dev(ctx, text.tobytes(), 13), member, k)
    assert total == want_e.size and np.array_equal(e, want_e) and np.array_equal(d, want_d)
    got, t = _gpu(ctx, _dev(ctx, text.tobytes(), 13), member)  # and the class search finds exactly the clean copies
    assert np.array_equal(got, co.class_starts(text.tobytes(), member)) and t >= sum(1 for _, s in planted if s == 0)
