"""GPU suite for the k-mismatch search (bmx_search_hamming[_classes]_device / bmx_search_hamming[_classes] /
bmx_cli --hamming): starts and distances compared in full with the numpy oracle (tests/hamming_oracle.py), with the class
search at k = 0 and with the approximate search's ends at the same k (the superset rule)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import classes_oracle as co
import hamming_oracle as ho
from conftest import ROOT, golden_file_bytes
from parallel_implementation_of_string_matching_algorithms_opencl_amd import corpus, host

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "parallel_implementation_of_string_matching_algorithms_opencl_amd", "bin", "bmx_cli")
ACGT = np.frombuffer(b"ACGT", np.uint8)
GUIDE = "GACGTTACCGGATCAAGCTT"  # 20 bases, then the PAM: any base and two G that must match


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


def _gpu(ctx, d_text, member, k, must=0, **kw):
    import torch

    cap = max(kw.get("n", d_text.numel()), 1)
    out = torch.full((cap,), -1, dtype=torch.int64, device=d_text.device)
    dist = torch.full((cap,), 255, dtype=torch.uint8, device=d_text.device)
    s, d, total = ctx.search_hamming_device(d_text, co.pack(member), k, must=must, out=out, dist_out=dist, **kw)
    return s.cpu().numpy().astype(np.int64), d.cpu().numpy().astype(np.int64), total


def _check(ctx, text: bytes, member, k, must=0, offset: int = 0):
    want_s, want_d = ho.hamming_starts(text, member, k, must)
    s, d, total = _gpu(ctx, _dev(ctx, text, offset), member, k, must)
    where = (len(text), len(member), k, hex(must), offset)
    assert total == want_s.size, where + (total, want_s.size)
    assert np.array_equal(s, want_s), where
    assert np.array_equal(d, want_d), where
    return want_s, want_d


def _random_member(rng, m, symbols):
    """Per position a random singleton, a 2-4 member set, any, a negated singleton or (rarely) the empty class."""
    member = np.zeros((m, 256), dtype=bool)
    for i in range(m):
        kind = int(rng.integers(0, 9))
        if kind < 3:
            member[i][rng.choice(symbols)] = True
        elif kind < 5:
            member[i][rng.choice(symbols, int(rng.integers(2, 5)))] = True
        elif kind < 6:
            member[i] = True
        elif kind < 8:
            member[i] = True
            member[i][rng.choice(symbols)] = False
    return member


def _plant(rng, text, member, at, subs=0, symbols=None):
    """Overwrite text[at : at + m) with a member of every class (where there is one), then put a byte from outside the
    class at `subs` random positions (where there is one among `symbols`)."""
    m = member.shape[0]
    for i in range(m):
        inside = np.nonzero(member[i])[0]
        if inside.size:
            text[at + i] = rng.choice(inside)
    for i in rng.choice(m, min(subs, m), replace=False):
        outside = [b for b in (symbols if symbols is not None else range(256)) if not member[i][b]]
        if outside:
            text[at + i] = rng.choice(outside)


def test_random_cases_against_oracle(ctx):
    rng = np.random.default_rng(0x4A3300)
    seen_k, hits, with_must = set(), 0, 0
    for case in range(300):
        sigma = (2, 4, 95)[case % 3]
        n = int(rng.integers(0, 5001)) if case % 10 else int(rng.integers(0, 70))  # every tenth: n around or below m
        m = int(rng.integers(1, 65))
        k = case % 16 if case % 16 < m else int(rng.integers(0, min(m, 16)))
        base = 0x20 if sigma == 95 else 0x61
        symbols = np.arange(base, base + sigma)
        text = (rng.integers(0, sigma, n) + base).astype(np.uint8)
        member = _random_member(rng, m, symbols)
        for _ in range(int(rng.integers(0, 6))):
            if n > m:
                _plant(rng, text, member, int(rng.integers(0, n - m + 1)), int(rng.integers(0, k + 3)), symbols)
        must = 0
        if case % 2:
            must = int(rng.integers(0, 1 << 63)) & ((1 << m) - 1)
            if case % 4 == 1:
                must &= int(rng.integers(0, 1 << 63))  # sparser
        want_s, _ = _check(ctx, text.tobytes(), member, k, must, offset=case % 16)
        seen_k.add(k)
        hits += want_s.size
        with_must += bool(must) and want_s.size > 0
    assert seen_k == set(range(16)) and hits > 10000 and with_must > 20


def test_word_and_slice_switches_on_any_byte_values(ctx):
    rng = np.random.default_rng(72)
    text = rng.integers(0, 256, 6000).astype(np.uint8)
    for m in (1, 2, 31, 32, 33, 63, 64):
        member = np.zeros((m, 256), dtype=bool)
        for i in range(m):
            member[i][rng.integers(0x80, 0x100, 3)] = True  # bytes >= 0x80 in every class
            member[i][rng.integers(0, 0x100, int(rng.integers(0, 120)))] = True
        for k in (0, 1, 3, 4, 7, 8, 15):
            if k >= m:
                continue
            for j, at in enumerate((0, 100, 900, 1700, 2500, 3000, 4100, 6000 - m)):
                _plant(rng, text, member, at, (0, k, k + 1, 1, k, max(k - 1, 0), k + 2, k)[j])
            want_s, want_d = _check(ctx, text.tobytes(), member, k, offset=(m + k) % 16)
            assert {0, 100, 6000 - m} <= set(want_s.tolist()) and (k == 0 or want_d.max() == min(k, m))
            _check(ctx, text.tobytes(), member, k, must=(1 << (m - 1)) | 1, offset=1)


@pytest.mark.parametrize("m", [20, 64])
def test_saturation_at_the_wrap_points_of_the_counters(ctx, m):
    rng = np.random.default_rng(m)
    member = co.singletons(b"A" * m)
    blocks = []
    counts = list(range(m + 1)) + [4, 5, 16, 17, 32, 64, m, 0, m, 15, 16]
    for c in counts:  # a window with exactly c mismatches; its neighbours overlap two of them
        c = min(c, m)
        blk = np.full(m, ord("A"), np.uint8)
        blk[rng.choice(m, c, replace=False)] = rng.integers(ord("B"), ord("Z"), c)
        blocks.append(blk)
    text = np.concatenate(blocks)
    full = ho.hamming_starts(text.tobytes(), member, m - 1)[1]  # (at k = m - 1 every window but an all-wrong one is listed)
    assert {0, 4, 5, 16, 17}.issubset(full.tolist()) and (m < 64 or {32, 63}.issubset(full.tolist()))
    d_text = _dev(ctx, text.tobytes(), 5)
    for k in range(1, 16):
        want_s, want_d = ho.hamming_starts(text.tobytes(), member, k)
        s, d, total = _gpu(ctx, d_text, member, k)
        assert total == want_s.size and np.array_equal(s, want_s) and np.array_equal(d, want_d), (m, k)
        assert want_d.max() == k and 0 in want_s.tolist()
    nothing = rng.integers(ord("B"), ord("Z"), 5000).astype(np.uint8).tobytes()  # no A at all: every window is all wrong
    d_nothing = _dev(ctx, nothing, 3)
    for k in range(1, 16):
        s, d, total = _gpu(ctx, d_nothing, member, k)
        assert total == 0 and s.size == 0, (m, k)


def test_guide_with_a_pam_that_must_match(ctx):
    rng = np.random.default_rng(23)
    member = co.parse(GUIDE + "NGG", co.IUPAC)
    m = 23
    must = ho.must_mask([21, 22])
    n = 1 << 19
    for k in (1, 3, 4):
        text = ACGT[rng.integers(0, 4, n)].copy()
        planted = []
        for j, at in enumerate(range(500, n - 500, 1031)):
            subs = j % (k + 2)  # 0 .. k + 1 substitutions in the guide
            pam = (j // (k + 2)) % 3  # none, or one in either G of the PAM
            text[at:at + m] = np.frombuffer((GUIDE + "AGG").encode(), np.uint8)
            for i in rng.choice(20, subs, replace=False):
                text[at + i] = rng.choice([b for b in b"ACGT" if b != text[at + i]])
            if pam:
                text[at + 20 + pam] = rng.choice(list(b"ACT"))
            planted.append((at, subs, pam))
        want_s, want_d = _check(ctx, text.tobytes(), member, k, must, offset=13)
        by_start = dict(zip(want_s.tolist(), want_d.tolist()))
        for at, subs, pam in planted:  # listed with its substitutions iff the PAM is whole and the guide within k
            assert by_start.get(at) == (subs if subs <= k and not pam else None), (k, at, subs, pam)
        plain_s, plain_d = _check(ctx, text.tobytes(), member, k, 0, offset=13)  # must = 0: the plain count
        assert plain_s.size > want_s.size
        assert any(pam and subs < k and at in plain_s for at, subs, pam in planted)
        s, d, total = _gpu(ctx, _dev(ctx, text.tobytes(), 2), member, k, (1 << m) - 1)  # must = all: the class search
        exact, exact_total = ctx.search_classes_device(_dev(ctx, text.tobytes(), 2), co.pack(member), capacity=n)
        assert total == exact_total > 0 and np.array_equal(s, exact.cpu().numpy()) and not d.any()


def test_k0_is_the_class_search(ctx):
    rng = np.random.default_rng(40)
    for m in (1, 5, 32, 33, 64):
        text = (rng.integers(0, 4, 50000) + 0x61).astype(np.uint8)
        member = _random_member(rng, m, np.arange(0x61, 0x65))
        member[member.sum(axis=1) == 0, 0x61] = True  # no empty class here: there shall be hits
        for at in range(0, text.size - m, 611):
            _plant(rng, text, member, at)
        d_text = _dev(ctx, text.tobytes(), 9)
        exact, exact_total = ctx.search_classes_device(d_text, co.pack(member), capacity=text.size)
        assert exact_total > 50
        for must in (0, (1 << m) - 1, int(rng.integers(0, 1 << 62)) & ((1 << m) - 1)):
            s, d, total = _gpu(ctx, d_text, member, 0, must)
            assert total == exact_total and np.array_equal(s, exact.cpu().numpy()) and not d.any(), (m, must)


def test_every_hit_is_among_the_approximate_ends(ctx):
    rng = np.random.default_rng(41)
    for m, k in ((8, 2), (20, 3), (32, 6), (33, 4), (64, 15)):
        text = (rng.integers(0, 4, 200000) + 0x61).astype(np.uint8)
        member = _random_member(rng, m, np.arange(0x61, 0x65))
        member[member.sum(axis=1) == 0] = True  # no empty class here: a planted copy has its substitutions and no more
        for j, at in enumerate(range(100, text.size - m, 1777)):
            _plant(rng, text, member, at, j % (k + 2), np.arange(0x61, 0x65))
        d_text = _dev(ctx, text.tobytes(), 6)
        s, d, total = _gpu(ctx, d_text, member, k)
        e, ed, e_total = ctx.search_approx_classes_device(d_text, co.pack(member), k, capacity=text.size)
        assert total > 50 and e_total >= total
        ends, edit = e.cpu().numpy().astype(np.int64), ed.cpu().numpy().astype(np.int64)
        at = np.searchsorted(ends, s + m - 1)
        assert (at < ends.size).all() and np.array_equal(ends[at], s + m - 1), (m, k)
        assert (edit[at] <= d).all(), (m, k)


@pytest.mark.parametrize("m,k", [(16, 2), (16, 5), (64, 3), (64, 9)])
def test_lengths_at_piece_and_tile_edges(ctx, m, k):
    p = piece(m)
    assert 256 * p == {16: 16 << 10, 64: 64 << 10}[m]
    rng = np.random.default_rng(m + k)
    symbols = np.arange(0x61, 0x65)
    member = _random_member(rng, m, symbols)
    member[member.sum(axis=1) == 0] = True  # no empty class here: the planted copies shall be hits
    big = (rng.integers(0, 4, 256 * p + 64) + 0x61).astype(np.uint8)
    for j, at in enumerate(range(0, big.size - m, 499)):
        _plant(rng, big, member, at, j % (k + 2), symbols)
    for at in (p - m, 256 * p - m, 256 * p - m + 1, 256 * p - 1, 256 * p):  # windows that end at and straddle the edges
        _plant(rng, big, member, at, k, symbols)
    must = 1 << (m // 2)
    for n in (p - 1, p, p + 1, 256 * p - 1, 256 * p, 256 * p + 1, 256 * p + m - 1, 256 * p + m):
        for off in (0, 9):
            _check(ctx, big[:n].tobytes(), member, k, must if off else 0, offset=off)


def test_small_and_shifted_views(ctx):
    rng = np.random.default_rng(3)
    text = (rng.integers(0, 2, 4000) + 0x61).astype(np.uint8).tobytes()
    member = co.parse("a[ab]b.aab")
    m, k, must = 7, 1, 0b0000100
    want, want_d = ho.hamming_starts(text, member, k, must)
    assert want.size > 100 and want_d.max() == 1
    d_text = _dev(ctx, text, 3)
    for n in (0, 1, m - 1):  # n < m: nothing fits
        s, d, total = _gpu(ctx, d_text, member, k, must, n=n)
        assert total == 0 and s.size == 0
    s, d, total = _gpu(ctx, d_text, member, k, must, n=m)  # n == m: one window
    assert s.tolist() == want[want < 1].tolist() and total == s.size
    for n, n_own in ((4000, 0), (4000, 1), (4000, 1234), (4000, 3994), (4000, 3995), (4000, 4000), (2000, 1990), (2000, 5000)):
        s, d, total = _gpu(ctx, d_text, member, k, must, n=n, n_own=n_own, base_offset=10 ** 12 + 7)
        keep = (want < n_own) & (want + m <= n)
        assert total == keep.sum() and np.array_equal(s, want[keep] + 10 ** 12 + 7) and np.array_equal(d, want_d[keep]), (n, n_own)
        ws, wd = ho.hamming_starts(text[:n], member, k, must, n_own)  # and the oracle's own ownership rule
        assert np.array_equal(ws, want[keep]) and np.array_equal(wd, want_d[keep])


def test_dense_tiles_walk_twice(ctx):
    m = 8
    n = 3 * 256 * piece(m) + 5  # three tiles plus 5
    rng = np.random.default_rng(8)
    text = rng.integers(0, 256, n).astype(np.uint8).tobytes()
    for k in (2, 7):  # every start a hit, distance 0
        s, d, total = _gpu(ctx, _dev(ctx, text, 7), np.ones((m, 256), dtype=bool), k)
        assert total == n - m + 1 and np.array_equal(s, np.arange(n - m + 1)) and not d.any()


def test_dense_and_sparse_neighbour_tiles(ctx):
    rng = np.random.default_rng(5)
    n = 3 * corpus.MiB
    text = (rng.integers(0, 95, n) + 0x20).astype(np.uint8)
    for blk in range(0, n, 3 * 40000):  # dense stretches of ACGT that cut across tile boundaries, a stray byte now and then
        text[blk:blk + 40000] = ACGT[rng.integers(0, 4, min(40000, n - blk))]
        text[blk + 7:blk + 40000:53] = ord("x")
    member = co.parse("NNNNNNNNNN", co.IUPAC)
    for k, must in ((1, 0), (4, 0b11)):
        want_s, want_d = _check(ctx, text.tobytes(), member, k, must, offset=4)
        assert want_s.size > n // 4 and set(want_d.tolist()) >= {0, 1}


def test_capacity_keeps_the_lowest_starts(ctx):
    import torch

    spec = corpus.CorpusSpec("hamming_cap", 2 * corpus.MiB, 12, 1, seed=0x5EED4A00, plant_period=1 << 12)
    text = spec.host_text().tobytes()
    member = co.parse("ACNNGTAC", co.IUPAC)
    k = 1
    want, want_d = ho.hamming_starts(text, member, k)
    total = want.size
    assert total > 5000  # more than a tile parks
    d_text = spec.device_text(ctx)
    cls = co.pack(member)
    for cap in (0, 1, total - 1, total // 2):
        out = torch.full((max(cap, 1),), -1, dtype=torch.int64, device=d_text.device)
        n_matches = C.c_uint64(0)
        rc = ctx._L.bmx_search_hamming_classes_device(ctx._h, C.c_void_p(d_text.data_ptr()), d_text.numel(), d_text.numel(), 0,
                                                      C.c_void_p(cls.ctypes.data), 8, k, 0, C.c_void_p(out.data_ptr()), None, cap,
                                                      C.byref(n_matches), None)  # d_dist = NULL
        assert rc == host.ERR_CAPACITY and n_matches.value == total, (cap, rc, n_matches.value)
        if cap:
            assert np.array_equal(out.cpu().numpy(), want[:cap]), cap
        else:
            assert int(out[0].item()) == -1
    s, d, t = _gpu(ctx, d_text, member, k)
    assert t == total and np.array_equal(s, want) and np.array_equal(d, want_d)


def test_shards_concatenate_to_the_whole_list(ctx):
    rng = np.random.default_rng(77)
    n = corpus.MiB
    text = ACGT[rng.integers(0, 4, n)].copy()
    for m, k, must in ((12, 2, 0b11), (40, 6, 1 << 39)):
        member = co.singletons(text[5000:5000 + m].tobytes())
        for j, at in enumerate(range(0, n - m, 2003)):
            _plant(rng, text, member, at, j % (k + 2), ACGT)
        d_text = _dev(ctx, text.tobytes())
        whole_s, whole_d = _check(ctx, text.tobytes(), member, k, must)
        assert whole_s.size > 300
        cuts = [0, 200003, 200004, 524288, 524288 + m - 1, n]  # five unequal shards
        parts_s, parts_d = [], []
        for a, b in zip(cuts[:-1], cuts[1:]):
            view = d_text[a:min(b + m - 1, n)]  # the shard and its halo
            s, d, t = _gpu(ctx, view, member, k, must, n_own=b - a, base_offset=a)
            assert t == s.size
            parts_s.append(s)
            parts_d.append(d)
        assert np.array_equal(np.concatenate(parts_s), whole_s) and np.array_equal(np.concatenate(parts_d), whole_d)


def test_entry_points_and_the_cli(ctx, tmp_path):
    text = golden_file_bytes("input5L.txt.gz")
    (tmp_path / "input5L.txt").write_bytes(text)
    (tmp_path / "pattern.txt").write_bytes(b"occurrences")
    base = [CLI, "--text", str(tmp_path / "input5L.txt"), "--iters", "2", "--positions", "--max-print", "3"]

    def cli(args, k, want_s, want_d):
        r = subprocess.run(base + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert f"k-mismatch matches (k = {k}): {want_s.size}\n" in r.stdout
        assert f"first start: {want_s[0]} (distance {want_d[0]})\n" in r.stdout
        assert f"last start: {want_s[-1]} (distance {want_d[-1]})\n" in r.stdout
        got = [(int(a), int(b)) for a, b in re.findall(r"Start at : (\d+) \(distance (\d+)\)", r.stdout)]
        assert got == list(zip(want_s[:3].tolist(), want_d[:3].tolist()))
        assert "Average time" in r.stdout

    # a string, with and without `must`
    for k, must in ((2, None), (3, [0, 1, 2]), (2, 0b11000000000)):
        mask = host._must_mask(must)
        want_s, want_d = ho.hamming_starts(text, co.singletons(b"occurrences"), k, mask)
        assert want_s.size > 100
        s, d = ctx.search_hamming(text, "occurrences", k, must)  # host entry point through the Context
        assert s.dtype == np.uint64 and d.dtype == np.uint8
        assert np.array_equal(s.astype(np.int64), want_s) and np.array_equal(d.astype(np.int64), want_d)
        s, d = host.search_hamming(text, b"occurrences", k, must)  # module level
        assert np.array_equal(s.astype(np.int64), want_s) and np.array_equal(d.astype(np.int64), want_d)
        s, d, total = ctx.search_hamming_device(_dev(ctx, text, 5), "occurrences", k, must=must)  # the string's device entry
        assert total == want_s.size and np.array_equal(s.cpu().numpy(), want_s) and np.array_equal(d.cpu().numpy(), want_d)
    want_s, want_d = ho.hamming_starts(text, co.singletons(b"occurrences"), 2)
    cli(["--hamming", "2", "--pattern", str(tmp_path / "pattern.txt")], 2, want_s, want_d)
    want_s, want_d = ho.hamming_starts(text, co.singletons(b"occurrences"), 3, 0b10000000111)
    cli(["--hamming", "3", "--must", "0-2,10", "--pattern", str(tmp_path / "pattern.txt")], 3, want_s, want_d)
    # classes: an expression with flags, a compiled array
    member = co.parse("occurrences", co.ICASE)
    want_s, want_d = ho.hamming_starts(text, member, 1)
    s, d = ctx.search_hamming(text, "occurrences", 1, flags=host.CLASS_ICASE)
    assert np.array_equal(s.astype(np.int64), want_s) and np.array_equal(d.astype(np.int64), want_d)
    s, d = ctx.search_hamming(text, host.compile_classes("occurrences", host.CLASS_ICASE), 1)
    assert np.array_equal(s.astype(np.int64), want_s) and np.array_equal(d.astype(np.int64), want_d)
    cli(["--hamming", "1", "--classes", "occurrences", "--icase"], 1, want_s, want_d)
    with pytest.raises(host.BmxError):
        ctx.search_hamming(text, "occurrences", 2, capacity=3)
    # --classes --iupac on a DNA text, with a PAM that must match
    rng = np.random.default_rng(99)
    dna = ACGT[rng.integers(0, 4, 300000)].copy()
    guide = np.frombuffer((GUIDE + "TGG").encode(), np.uint8)
    for j, at in enumerate(range(100, dna.size - 100, 997)):
        dna[at:at + 23] = guide
        dna[at + rng.choice(23, j % 5, replace=False)] = ord("A")
    (tmp_path / "input5L.txt").write_bytes(dna.tobytes())
    member = co.parse(GUIDE + "NGG", co.IUPAC)
    want_s, want_d = ho.hamming_starts(dna.tobytes(), member, 3, ho.must_mask([21, 22]))
    assert want_s.size > 100 and want_d.max() == 3
    cli(["--hamming", "3", "--classes", GUIDE + "NGG", "--iupac", "--must", "21-22"], 3, want_s, want_d)
    s, d = ctx.search_hamming(dna.tobytes(), GUIDE + "NGG", 3, must=[21, 22], flags=host.CLASS_IUPAC)
    assert np.array_equal(s.astype(np.int64), want_s) and np.array_equal(d.astype(np.int64), want_d)
    for bad in (["--hamming", "3", "--must", "5-2"], ["--must", "1"], ["--hamming", "1", "--approx", "1"],
                ["--hamming", "1", "--must", "64"]):
        r = subprocess.run(base + bad + ["--classes", GUIDE], capture_output=True, text=True, timeout=120)
        assert r.returncode == 2, bad


def test_on_a_callers_non_blocking_stream(ctx):
    import torch

    text = golden_file_bytes("input5L.txt.gz")
    member = co.singletons(b"occurrences")
    want_s, want_d = ho.hamming_starts(text, member, 2, 1)
    d_text = _dev(ctx, text, 2)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    s, d, total = ctx.search_hamming_device(d_text, "occurrences", 2, must=1, stream=side)
    assert total == want_s.size and np.array_equal(s.cpu().numpy(), want_s) and np.array_equal(d.cpu().numpy(), want_d)
    with torch.cuda.stream(side):  # and as torch's current stream
        s, d, total = ctx.search_hamming_device(d_text, co.pack(member), 2, must=[0])
    assert total == want_s.size and np.array_equal(s.cpu().numpy(), want_s) and np.array_equal(d.cpu().numpy(), want_d)


def test_repeat_calls_interleaved_with_other_searches(ctx):
    text = golden_file_bytes("input5L.txt.gz")
    d_text = _dev(ctx, text, 11)
    shapes = [(co.parse("occurrences", co.ICASE), 2, 0), (co.singletons(b"the "), 1, 0b1000),
              (co.parse("." * 30 + "occurrences"), 5, 0), (co.singletons(text[1000:1042]), 9, 1)]
    want = [ho.hamming_starts(text, member, k, must) for member, k, must in shapes]
    assert all(w[0].size > 0 for w in want)
    exact = co.class_starts(text, shapes[0][0])
    ends, dists = co.class_approx_ends(text, shapes[0][0], 1)
    for rep in range(20):
        member, k, must = shapes[rep % 4]
        s, d, total = _gpu(ctx, d_text, member, k, must)
        assert total == want[rep % 4][0].size and np.array_equal(s, want[rep % 4][0]) and np.array_equal(d, want[rep % 4][1]), rep
        assert ctx.last_hamming_ms() >= 0
        pos, t = ctx.search_classes_device(d_text, co.pack(shapes[0][0]), capacity=len(text))
        assert t == exact.size and np.array_equal(pos.cpu().numpy(), exact)
        e, ed, t = ctx.search_approx_classes_device(d_text, co.pack(shapes[0][0]), 1, capacity=len(text))
        assert t == ends.size and np.array_equal(e.cpu().numpy(), ends) and np.array_equal(ed.cpu().numpy().astype(np.int64), dists)
