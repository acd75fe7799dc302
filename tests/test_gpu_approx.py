"""GPU suite for the approximate search (bmx_search_approx_device / bmx_search_approx / bmx_cli --approx): ends and
distances compared in full with the Sellers oracle (tests/approx_oracle.py) or, for k = 0, with the exact search."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from approx_oracle import approx_ends
from conftest import ROOT, golden_file_bytes
from test_approx_cpu import KNOWN, known_text
from parallel_implementation_of_string_matching_algorithms_opencl_amd import corpus, host

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "parallel_implementation_of_string_matching_algorithms_opencl_amd", "bin", "bmx_cli")


def _dev(ctx, data: bytes, offset: int = 0):
    """data on the device, starting `offset` bytes into a buffer (any alignment)."""
    import torch

    buf = torch.zeros(len(data) + offset + 16, dtype=torch.uint8, device=f"cuda:{ctx.device}")
    if data:
        buf[offset:offset + len(data)] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(buf.device)
    return buf[offset:offset + len(data)] if data else buf[offset:offset]


def _gpu(ctx, d_text, pat, k, **kw):
    cap = kw.pop("capacity", None)
    n = kw.get("n", d_text.numel())
    ends, dists, total = ctx.search_approx_device(d_text, pat, k, capacity=cap if cap is not None else max(n, 1), **kw)
    return ends.cpu().numpy().astype(np.int64), dists.cpu().numpy().astype(np.int64), total


def _check(ctx, text: bytes, pat: bytes, k: int, offset: int = 0):
    want_e, want_d = approx_ends(text, pat, k)
    e, d, total = _gpu(ctx, _dev(ctx, text, offset), pat, k)
    assert total == want_e.size, (len(text), pat, k, offset, total, want_e.size)
    assert np.array_equal(e, want_e), (len(text), pat, k, offset)
    assert np.array_equal(d, want_d), (len(text), pat, k, offset)


def test_random_cases_against_oracle(ctx):
    rng = np.random.default_rng(0xA77A0)
    for case in range(300):
        sigma = (2, 4, 95)[case % 3]
        n = int(rng.integers(0, 5001)) if case % 10 else int(rng.integers(0, 70))  # every tenth: n around or below m
        m = int(rng.integers(1, 65))
        k = int(rng.integers(0, m))
        base = 0x20 if sigma == 95 else 0x61
        text = (rng.integers(0, sigma, n) + base).astype(np.uint8)
        pat = (rng.integers(0, sigma, m) + base).astype(np.uint8)
        if n > m and rng.integers(0, 2):  # a copy of the pattern with a few edits
            at = int(rng.integers(0, n - m + 1))
            text[at:at + m] = pat
            for _ in range(int(rng.integers(0, k + 1))):
                text[int(rng.integers(at, at + m))] = base + int(rng.integers(0, sigma))
        _check(ctx, text.tobytes(), pat.tobytes(), k, offset=case % 16)


def test_every_k_and_any_bytes(ctx):
    rng = np.random.default_rng(7)
    text = rng.integers(0, 256, 3000).astype(np.uint8)
    for m in (1, 2, 7, 31, 32, 33, 63, 64):
        pat = rng.integers(0, 256, m).astype(np.uint8)
        text[100:100 + m] = pat
        text[2000:2000 + m] = pat[::-1]
        for k in range(m):
            if m > 8 and k not in (0, 1, m // 2, m - 2, m - 1):
                continue
            _check(ctx, text.tobytes(), pat.tobytes(), k, offset=m % 16)


def test_known_answers_both_entry_points(ctx):
    for name, pat, k, hits, first, last, per_dist in KNOWN:
        text = known_text(name)
        want_e, want_d = approx_ends(text, pat, k)
        e, d, total = _gpu(ctx, _dev(ctx, text, 3), pat, k)
        assert total == hits and np.array_equal(e, want_e) and np.array_equal(d, want_d), (name, pat, k)
        assert [(int(x), int(y)) for x, y in zip(e[:len(first)], d[:len(first)])] == first and int(e[-1]) == last
        assert np.bincount(d, minlength=k + 1).tolist() == per_dist
        e2, d2 = ctx.search_approx(text, pat, k)
        assert np.array_equal(e2.astype(np.int64), want_e) and np.array_equal(d2.astype(np.int64), want_d)
        assert ctx.last_approx_ms() >= 0
    e3, d3 = host.search_approx(b"xxabcdxxabxdxxacdxx", "abcd", 1)  # the module-level entry point
    assert e3.tolist() == [4, 5, 6, 11, 16] and d3.tolist() == [1, 0, 1, 1, 1]


def test_known_answers_through_the_cli(ctx, tmp_path):
    (tmp_path / "input5L.txt").write_bytes(golden_file_bytes("input5L.txt.gz"))
    for name, pat, k, hits, first, last, per_dist in KNOWN[1:]:
        (tmp_path / "pat.txt").write_bytes(pat)
        r = subprocess.run([CLI, "--approx", str(k), "--text", str(tmp_path / "input5L.txt"), "--pattern",
                            str(tmp_path / "pat.txt"), "--iters", "2", "--positions", "--max-print", "3"],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        out = r.stdout
        assert f"approximate matches (k = {k}): {hits}" in out
        assert f"first end: {first[0][0]} (distance {first[0][1]})" in out
        assert re.search(rf"last end: {last} \(distance \d\)", out)
        got = [(int(a), int(b)) for a, b in re.findall(r"End at : (\d+) \(distance (\d+)\)", out)]
        assert got == first
        assert "Average time" in out


@pytest.mark.parametrize("kind", [0, 1])
def test_k0_equals_exact_search(ctx, port, kind):
    import torch

    for m in (1, 8, 16, 32, 33, 64):
        spec = corpus.CorpusSpec(f"approx_k0_{kind}_{m}", 16 * corpus.MiB + 5, m, kind, seed=0x5EEDA000 + m,
                                 plant_period=1 << 14, boundary_period=1 << 20)
        d_text = spec.device_text(ctx)
        pat = spec.pattern()
        want = port.search(spec.host_text(), pat).astype(np.int64)
        pos, total = ctx.search_device(d_text, pat, capacity=d_text.numel())
        assert total == want.size and np.array_equal(pos.cpu().numpy().astype(np.int64), want)
        out = torch.empty(max(want.size, 1), dtype=torch.int64, device=d_text.device)
        e, d, total = ctx.search_approx_device(d_text, pat, 0, out=out)
        assert total == want.size, (kind, m)
        assert np.array_equal(e.cpu().numpy().astype(np.int64) - (m - 1), want), (kind, m)
        assert int(d.max().item() if d.numel() else 0) == 0


def test_word_switch_and_full_k(ctx):
    rng = np.random.default_rng(33)
    text = (rng.integers(0, 4, 20000) + 0x61).astype(np.uint8)
    for m in (32, 33):
        pat = text[5000:5000 + m].copy()
        for k in (0, 1, 5, m - 1):
            _check(ctx, text.tobytes(), pat.tobytes(), k, offset=5)
    pat = (rng.integers(0, 4, 64) + 0x61).astype(np.uint8)
    _check(ctx, text[:6000].tobytes(), pat.tobytes(), 63, offset=1)  # every end qualifies
    _check(ctx, text[:40].tobytes(), pat.tobytes(), 63)  # n < m


@pytest.mark.parametrize("m,k,piece", [(8, 2, 64), (16, 0, 64), (64, 63, 512)])
def test_lengths_at_piece_and_tile_edges(ctx, m, k, piece):
    """Lane pieces are 2^ps ends (64 .. 2048, at least 4 (m + k)), tiles 256 pieces: lengths at both, +- 1."""
    rng = np.random.default_rng(m * 100 + k)
    pat = (rng.integers(0, 4, m) + 0x61).astype(np.uint8)
    big = (rng.integers(0, 4, 256 * piece + 64) + 0x61).astype(np.uint8)
    for at in range(0, big.size - m, 997):
        big[at:at + m] = pat
    for n in (piece - 1, piece, piece + 1, 256 * piece - 1, 256 * piece, 256 * piece + 1):
        for off in (0, 9):
            _check(ctx, big[:n].tobytes(), pat.tobytes(), k, offset=off)


def test_dense_tiles_walk_twice(ctx):
    spec = corpus.CorpusSpec("approx_dense", 8 * corpus.MiB, 8, 1, seed=0x5EEDA100, plant_period=0, boundary_period=0)
    text = spec.host_text().tobytes()
    pat = b"ACGTTGCA"
    want_e, want_d = approx_ends(text, pat, 3)
    assert want_e.size > len(text) // 16  # far more than a tile can park
    e, d, total = _gpu(ctx, spec.device_text(ctx), pat, 3)
    assert total == want_e.size and np.array_equal(e, want_e) and np.array_equal(d, want_d)


def test_dense_and_sparse_neighbour_tiles(ctx):
    rng = np.random.default_rng(5)
    n = 3 * corpus.MiB
    text = (rng.integers(0, 95, n) + 0x20).astype(np.uint8)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    for blk in range(0, n, 3 * 40000):  # dense stretches of ACGT that cut across tile boundaries
        text[blk:blk + 40000] = acgt[rng.integers(0, 4, min(40000, n - blk))]
    _check(ctx, text.tobytes(), b"ACGTTGCA", 3, offset=4)


def test_capacity_keeps_the_lowest_ends(ctx):
    import torch

    spec = corpus.CorpusSpec("approx_cap", 2 * corpus.MiB, 12, 1, seed=0x5EEDA200, plant_period=1 << 12)
    text = spec.host_text().tobytes()
    pat = spec.pattern()
    want_e, want_d = approx_ends(text, pat, 2)
    total = want_e.size
    assert total > 100
    d_text = spec.device_text(ctx)
    for cap in (0, 1, total - 1, total // 2):
        out = torch.full((max(cap, 1),), -1, dtype=torch.int64, device=d_text.device)
        dist = torch.full((max(cap, 1),), 255, dtype=torch.uint8, device=d_text.device)
        n_matches = C.c_uint64(0)
        rc = ctx._L.bmx_search_approx_device(ctx._h, C.c_void_p(d_text.data_ptr()), d_text.numel(), 0, 0, pat, len(pat),
                                             2, C.c_void_p(out.data_ptr()), C.c_void_p(dist.data_ptr()), cap,
                                             C.byref(n_matches), None)
        assert rc == host.ERR_CAPACITY and n_matches.value == total, (cap, rc, n_matches.value)
        if cap:
            assert np.array_equal(out.cpu().numpy(), want_e[:cap]), cap
            assert np.array_equal(dist.cpu().numpy().astype(np.int64), want_d[:cap]), cap
    e, d, t = _gpu(ctx, d_text, pat, 2, capacity=total)
    assert t == total and np.array_equal(e, want_e)


def test_shards_concatenate_to_the_whole_list(ctx):
    spec = corpus.CorpusSpec("approx_shards", 64 * corpus.MiB, 16, 0, seed=0x5EEDA300, plant_period=1 << 15,
                             boundary_period=1 << 22)
    d_text = spec.device_text(ctx)
    pat = bytearray(spec.pattern())
    pat[5] = 0x7E  # one substitution against the plants: every plant is a hit at distance 1
    pat = bytes(pat)
    k = 2
    n = d_text.numel()
    whole_e, whole_d, whole_t = _gpu(ctx, d_text, pat, k)
    assert whole_t > 1000 and int(whole_d.min()) >= 1
    cuts = [0, 7 * corpus.MiB + 3, 20 * corpus.MiB, 20 * corpus.MiB + 1, 41 * corpus.MiB + 12345, n]
    es, ds = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        lead = min(a, len(pat) + k - 1)
        view = d_text[a - lead:b]
        e, d, t = _gpu(ctx, view, pat, k, lead=lead, base_offset=a - lead)
        es.append(e)
        ds.append(d)
    assert np.array_equal(np.concatenate(es), whole_e) and np.array_equal(np.concatenate(ds), whole_d)


def _edit(rng, pat: bytes, edits: int) -> bytes:
    s = bytearray(pat)
    for _ in range(edits):
        op = int(rng.integers(0, 3))
        i = int(rng.integers(0, len(s)))
        c = int(rng.integers(0x20, 0x7F))
        if op == 0:
            s[i] = c
        elif op == 1:
            s.insert(i, c)
        elif len(s) > 1:
            del s[i]
    return bytes(s)


def test_one_gib_with_planted_edits(ctx):
    import torch

    n = 1 << 30
    m, k = 16, 3
    pat = b"approximate-sear"
    gen = torch.Generator(device="cuda").manual_seed(0xA77)
    d_text = torch.randint(0x80, 0x100, (n,), dtype=torch.uint8, device="cuda", generator=gen)  # never in the pattern
    rng = np.random.default_rng(0xA771)
    spacing = 1 << 18  # >> 2 (m + k)
    starts = np.arange(64, n - spacing, spacing, dtype=np.int64) + rng.integers(0, spacing // 2, (n - spacing) // spacing)
    starts = starts[:4000]
    idx, val, windows = [], [], []
    for p in starts.tolist():
        copy = _edit(rng, pat, int(rng.integers(0, k + 2)))  # some with k + 1 edits: maybe no hit at all
        idx.append(np.arange(p, p + len(copy), dtype=np.int64))
        val.append(np.frombuffer(copy, np.uint8))
        windows.append((p - (m + k), len(copy) + 2 * (m + k)))  # every alignment of cost <= k that touches the copy
    d_text[torch.from_numpy(np.concatenate(idx)).cuda()] = torch.from_numpy(np.concatenate(val)).cuda()
    exp_e, exp_d = [], []
    for lo, length in windows:
        w = d_text[lo:lo + length].cpu().numpy().tobytes()
        e, d = approx_ends(w, pat, k)
        exp_e.append(e + lo)
        exp_d.append(d)
    exp_e = np.concatenate(exp_e)
    exp_d = np.concatenate(exp_d)
    assert exp_e.size > 1000
    out = torch.empty(exp_e.size + 1024, dtype=torch.int64, device="cuda")
    e, d, total = ctx.search_approx_device(d_text, pat, k, out=out)
    assert total == exp_e.size
    assert np.array_equal(e.cpu().numpy().astype(np.int64), exp_e)
    assert np.array_equal(d.cpu().numpy().astype(np.int64), exp_d)
    del d_text, out
    torch.cuda.empty_cache()


def test_repeat_calls_and_no_distances(ctx):
    import torch

    text = golden_file_bytes("input5L.txt.gz")
    d_text = _dev(ctx, text, 11)
    e1, d1, t1 = _gpu(ctx, d_text, b"occurrences", 2)
    e2, d2, t2 = _gpu(ctx, d_text, b"occurrences", 2)
    assert t1 == t2 == 6275 and np.array_equal(e1, e2) and np.array_equal(d1, d2)
    out = torch.empty(t1, dtype=torch.int64, device=d_text.device)
    total = C.c_uint64(0)
    rc = ctx._L.bmx_search_approx_device(ctx._h, C.c_void_p(d_text.data_ptr()), d_text.numel(), 0, 0, b"occurrences", 11, 2,
                                         C.c_void_p(out.data_ptr()), None, t1, C.byref(total), None)
    assert rc == host.OK and total.value == t1
    assert np.array_equal(out.cpu().numpy(), e1)
    e3, d3 = ctx.search_approx(text, b"occurrences", 2, capacity=t1)
    assert np.array_equal(e3.astype(np.int64), e1)
