"""GPU suite for the dictionary search (bmx_dict_search_device / bmx_dict_search / bmx_cli --dict): positions and pattern
indices compared in full with the oracle of tests/dict_oracle.py, with the exact scan, and with recorded answers."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden_file_bytes
from dict_oracle import DictIndex, dict_matches
from parallel_implementation_of_string_matching_algorithms_opencl_amd import corpus, host

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "parallel_implementation_of_string_matching_algorithms_opencl_amd", "bin", "bmx_cli")


def _dev(ctx, data: bytes, offset: int = 0):
    """data on the device, starting `offset` bytes into a buffer (any alignment)."""
    import torch

    buf = torch.zeros(len(data) + offset + 16, dtype=torch.uint8, device=f"cuda:{ctx.device}")
    if data:
        buf[offset:offset + len(data)] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(buf.device)
    return buf[offset:offset + len(data)]


def _gpu(d, d_text, capacity=None, **kw):
    n = kw.get("n", d_text.numel())
    cap = capacity if capacity is not None else max(2 * n, 1)
    pos, pid, total = d.search_device(d_text, capacity=cap, **kw)
    return pos.cpu().numpy().astype(np.int64), pid.cpu().numpy().astype(np.int64), total


def _check(ctx, text: bytes, pats, offset: int = 0, d=None):
    want_p, want_i = dict_matches(text, pats)
    own = d is None
    if own:
        d = ctx.dictionary(pats)
    p, i, total = _gpu(d, _dev(ctx, text, offset), capacity=max(want_p.size, 1))
    if own:
        d.close()
    assert total == want_p.size, (len(text), len(pats), offset, total, want_p.size)
    assert np.array_equal(p, want_p), (len(text), len(pats), offset)
    assert np.array_equal(i, want_i), (len(text), len(pats), offset)
    return total


def _random_dict(rng, sigma: int, base: int, K: int, text: np.ndarray, max_m: int):
    """K patterns over the alphabet: pieces of the text (they occur), random ones, duplicates, prefixes and suffixes
    of one another; lengths 1 .. max_m, mostly short."""
    pats = []
    n = text.size
    for _ in range(K):
        r = int(rng.integers(0, 10))
        m = int(min(max_m, rng.choice([1, 2, 3, 4, 5, 8, 16, 31, 64, 200, 512]) if r < 2 else rng.integers(1, 13)))
        if r < 5 and n > m:
            a = int(rng.integers(0, n - m + 1))
            pats.append(text[a:a + m].tobytes())
        elif r < 7 and pats:
            q = pats[int(rng.integers(0, len(pats)))]
            cut = int(rng.integers(1, len(q) + 1))
            pats.append(q[:cut] if r == 5 else q[-cut:])  # a prefix or a suffix of another pattern
        elif r == 7 and pats:
            pats.append(pats[int(rng.integers(0, len(pats)))])  # a duplicate under another index
        else:
            pats.append((rng.integers(0, sigma, m) + base).astype(np.uint8).tobytes())
    return pats


@pytest.mark.parametrize("sigma", [2, 4, 26, 95])
def test_random_dictionaries_against_oracle(ctx, sigma):
    rng = np.random.default_rng(0xD1C70 + sigma)
    base = 0x20 if sigma == 95 else 0x61
    for case in range(24):
        n = int(rng.integers(0, 40000)) if case % 6 else int(rng.integers(0, 40))
        text = (rng.integers(0, sigma, n) + base).astype(np.uint8)
        K = int(rng.choice([1, 2, 7, 33, 300, 4096])) if case % 8 else 4096
        pats = _random_dict(rng, sigma, base, K, text, 512)
        _check(ctx, text.tobytes(), pats, offset=case % 16)
    # texts shorter than the longest pattern, and n = 0
    pats = [b"a" * 40, b"ab", b"a", b"b" * 3, b"abab"]
    for n in (0, 1, 2, 3, 4, 5, 39, 40, 41):
        _check(ctx, (b"ab" * 30)[:n], pats, offset=n % 16)


@pytest.mark.parametrize("kind", [0, 1])
def test_agrees_with_search_device_and_multi(ctx, kind):
    import torch

    spec = corpus.CorpusSpec(f"dict_scan_{kind}", 8 * corpus.MiB + 11, 16, kind, seed=0x5EEDD100 + kind,
                             plant_period=1 << 13, boundary_period=1 << 19)
    d_text = spec.device_text(ctx)
    pat = spec.pattern()
    pos, total = ctx.search_device(d_text, pat, capacity=d_text.numel())
    with ctx.dictionary([pat]) as d:
        p, i, t = _gpu(d, d_text, capacity=total + 8)
    assert t == total and np.array_equal(p, pos.cpu().numpy().astype(np.int64)) and (i == 0).all()
    h = spec.host_text()
    pats = [pat, pat[:8], pat[3:9], h[100:104].tobytes(), pat[:1] if kind == 1 else pat[:3], h[5000:5031].tobytes(),
            pat, pat[:2]]
    for K in (2, 5, 8):
        out = torch.empty(d_text.numel() * 3, dtype=torch.int64, device=d_text.device)
        lists = ctx.search_device_multi(d_text, pats[:K], out=out)
        want_p = np.concatenate([x.cpu().numpy().astype(np.int64) for x in lists])
        want_i = np.concatenate([np.full(x.numel(), k, np.int64) for k, x in enumerate(lists)])
        order = np.lexsort((want_i, want_p))
        with ctx.dictionary(pats[:K]) as d:
            p, i, t = _gpu(d, d_text, capacity=want_p.size + 8)
        assert t == want_p.size and np.array_equal(p, want_p[order]) and np.array_equal(i, want_i[order]), K


def test_corpora_files_against_recorded_answers(ctx):
    with open(os.path.join(GOLDEN, "corpora.json")) as f:
        cases = json.load(f)["cases"]
    by_file = {}
    for c in cases:
        by_file.setdefault(c["file"], []).append(c)
    for name, cs in by_file.items():
        text = golden_file_bytes(name)
        pats = [c["pattern"].encode("latin-1") for c in cs]
        pos, pid = ctx.search_dict(text, pats)
        for i, c in enumerate(cs):
            mine = pos[pid == i].astype(np.int64)
            assert mine.size == c["count"], (name, c["pattern"])
            if c["count"]:
                assert int(mine[0]) == c["first"] and int(mine[-1]) == c["last"], (name, c["pattern"])
            if c["positions"] is not None:
                assert mine.tolist() == c["positions"], (name, c["pattern"])
        assert np.all(np.diff(pos.astype(np.int64)) >= 0)


def test_english_words(ctx):
    text = golden_file_bytes("input5L.txt.gz")
    # its distinct words (219: the file repeats its paragraphs) and its distinct runs of 2..4 words as they stand
    spans = [(w.start(), w.end()) for w in re.finditer(rb"[A-Za-z]+", text)]
    words = sorted({text[spans[i][0]:spans[i + k - 1][1]] for k in range(1, 5) for i in range(len(spans) - k + 1)})
    assert len(words) > 1000 and min(len(w) for w in words) == 1
    rng = np.random.default_rng(1)
    words = [words[j] for j in rng.permutation(len(words))]  # ids in no particular order
    total = _check(ctx, text, words, offset=7)
    assert total > len(text) // 8
    d = ctx.dictionary(words)
    pos, pid = d.search(text)
    want_p, want_i = dict_matches(text, words)
    assert np.array_equal(pos.astype(np.int64), want_p) and np.array_equal(pid.astype(np.int64), want_i)
    assert ctx.last_dict_ms() > 0 and ctx.last_dict_candidates() >= np.unique(want_p).size
    d.close()


def test_dense_output(ctx):
    spec = corpus.CorpusSpec("dict_dense", 8 * corpus.MiB, 8, 1, seed=0x5EEDD200, plant_period=0, boundary_period=0)
    text = spec.host_text().tobytes()
    acgt = b"ACGT"
    pats = [bytes([a, b, c, e]) for a in acgt for b in acgt for c in acgt for e in acgt] + [bytes([x]) for x in acgt]
    assert len(pats) == 260
    total = _check(ctx, text, pats, offset=3)
    assert total == 2 * len(text) - 3  # two pairs at every position but the last three


def test_dense_stretches_and_one_large_bucket(ctx):
    rng = np.random.default_rng(5)
    n = 3 * corpus.MiB
    text = (rng.integers(0, 95, n) + 0x20).astype(np.uint8)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    for blk in range(0, n, 3 * 40000):  # dense stretches of ACGT that cut across tile boundaries
        text[blk:blk + 40000] = acgt[rng.integers(0, 4, min(40000, n - blk))]
    pats = [b"ACG", b"A", b"CGTA", b"GT", b"TTTT", text[777:790].tobytes()]
    _check(ctx, text.tobytes(), pats, offset=4)
    # one bucket of 10,000 patterns sharing the 4-byte prefix "pref", planted in a sparse text
    suffixes = rng.integers(0x61, 0x7B, (10000, 6)).astype(np.uint8)
    bucket = [b"pref" + s.tobytes() for s in suffixes] + [b"pref", b"pre"]
    small = (rng.integers(0, 95, 1 << 20) + 0x20).astype(np.uint8)
    for j, at in enumerate(range(1000, small.size - 20, 5003)):
        w = bucket[(j * 37) % len(bucket)]
        small[at:at + len(w)] = np.frombuffer(w, np.uint8)
    _check(ctx, small.tobytes(), bucket, offset=9)


def test_capacity_keeps_the_lowest_pairs(ctx):
    import torch

    text = golden_file_bytes("input5L.txt.gz")
    pats = [b"the", b"e", b"occurrences", b"th", b"is", b"string matching"]
    want_p, want_i = dict_matches(text, pats)
    total = want_p.size
    d_text = _dev(ctx, text, 5)
    with ctx.dictionary(pats) as d:
        for cap in (0, 1, total - 1, total // 2):
            out = torch.full((max(cap, 1),), -1, dtype=torch.int64, device=d_text.device)
            pid = torch.full((max(cap, 1),), -1, dtype=torch.int32, device=d_text.device)
            n_matches = C.c_uint64(0)
            rc = ctx._L.bmx_dict_search_device(ctx._h, d._h, C.c_void_p(d_text.data_ptr()), d_text.numel(), d_text.numel(), 0,
                                               C.c_void_p(out.data_ptr()), C.c_void_p(pid.data_ptr()), cap,
                                               C.byref(n_matches), None)
            assert rc == host.ERR_CAPACITY and n_matches.value == total, (cap, rc, n_matches.value)
            if cap:
                assert np.array_equal(out.cpu().numpy(), want_p[:cap]), cap
                assert np.array_equal(pid.cpu().numpy().astype(np.int64), want_i[:cap]), cap
            else:
                assert int(out[0]) == -1
        p, i, t = d.search_device(d_text, capacity=total, pid_out=False)  # d_pid = NULL
        assert t == total and i is None and np.array_equal(p.cpu().numpy(), want_p)
        with pytest.raises(host.BmxError):
            ctx.search_dict(text, pats, capacity=total - 1)


def test_shards_concatenate_to_the_whole_list(ctx):
    spec = corpus.CorpusSpec("dict_shards", 32 * corpus.MiB + 77, 16, 0, seed=0x5EEDD300, plant_period=1 << 14,
                             boundary_period=1 << 21)
    d_text = spec.device_text(ctx)
    h = spec.host_text()
    pat = spec.pattern()
    pats = [pat, pat[:5], pat[4:], h[123456:123456 + 200].tobytes(), b"~", pat[-3:], h[9_000_000:9_000_004].tobytes()]
    halo = max(len(p) for p in pats) - 1
    n = d_text.numel()
    with ctx.dictionary(pats) as d:
        whole_p, whole_i, whole_t = _gpu(d, d_text, capacity=1 << 22)
        assert whole_t > 1000
        cuts = [0, 3 * corpus.MiB + 3, 11 * corpus.MiB, 11 * corpus.MiB + 1, 20 * corpus.MiB + 12345, n]
        ps, ids = [], []
        for a, b in zip(cuts[:-1], cuts[1:]):
            view = d_text[a:min(b + halo, n)]
            p, i, t = _gpu(d, view, capacity=1 << 22, n_own=b - a, base_offset=a)
            ps.append(p)
            ids.append(i)
    assert np.array_equal(np.concatenate(ps), whole_p) and np.array_equal(np.concatenate(ids), whole_i)
    want_p, want_i = dict_matches(h.tobytes(), pats)
    assert np.array_equal(whole_p, want_p) and np.array_equal(whole_i, want_i)


def test_one_gib_with_planted_dictionary(ctx):
    import torch

    n = 1 << 30
    rng = np.random.default_rng(0xD1C7B16)
    K = 65536
    lens = rng.integers(4, 33, K)  # m uniform in 4..32, a few short and a few long ones
    lens[:64] = rng.integers(100, 513, 64)
    lens[64:96] = rng.integers(1, 4, 32)
    pats = [(rng.integers(0x20, 0x7F, int(m))).astype(np.uint8).tobytes() for m in lens]
    gen = torch.Generator(device="cuda").manual_seed(0xD1C7)
    d_text = torch.randint(0x80, 0x100, (n,), dtype=torch.uint8, device="cuda", generator=gen)  # in no pattern
    spacing = n // 100000
    starts = np.arange(100000, dtype=np.int64) * spacing + rng.integers(0, spacing - 520, 100000)
    which = rng.integers(0, K, 100000)
    idx = np.concatenate([np.arange(s, s + len(pats[w]), dtype=np.int64) for s, w in zip(starts.tolist(), which.tolist())])
    val = np.concatenate([np.frombuffer(pats[w], np.uint8) for w in which.tolist()])
    d_text[torch.from_numpy(idx).cuda()] = torch.from_numpy(val).cuda()
    index = DictIndex(pats)
    memo = {}
    exp_p, exp_i = [], []
    for s, w in zip(starts.tolist(), which.tolist()):  # each plant is bounded by background bytes on both sides
        if w not in memo:
            memo[w] = index.matches(pats[w])
        p, i = memo[w]
        exp_p.append(p + s)
        exp_i.append(i)
    exp_p = np.concatenate(exp_p)
    exp_i = np.concatenate(exp_i)
    assert exp_p.size >= 100000
    with ctx.dictionary(pats) as d:
        out = torch.empty(exp_p.size + 1024, dtype=torch.int64, device="cuda")
        p, i, total = d.search_device(d_text, out=out)
        assert total == exp_p.size
        assert np.array_equal(p.cpu().numpy().astype(np.int64), exp_p)
        assert np.array_equal(i.cpu().numpy().astype(np.int64), exp_i)
    del d_text, out
    torch.cuda.empty_cache()


def test_reuse_across_texts_and_two_dictionaries(ctx):
    text = golden_file_bytes("input5L.txt.gz")
    a = ctx.dictionary([b"occurrences", b"the", b"a"])
    b = ctx.dictionary([b"is", b"occurrences starting fro", b"xyzzy"])
    for j, off in enumerate((0, 1, 13)):
        piece = text[j * 100000:(j + 3) * 100000]
        for d, pats in ((a, [b"occurrences", b"the", b"a"]), (b, [b"is", b"occurrences starting fro", b"xyzzy"])):
            _check(ctx, piece, pats, offset=off, d=d)
            _check(ctx, piece, pats, offset=off, d=d)  # a repeated call
    p, i = a.search(text)
    assert int((i == 0).sum()) == 1098
    other = host.Context(0)
    try:
        total = C.c_uint64(0)
        d_text = _dev(other, text[:1000])
        rc = other._L.bmx_dict_search_device(other._h, a._h, C.c_void_p(d_text.data_ptr()), 1000, 1000, 0, None, None, 0,
                                             C.byref(total), None)
        assert rc == host.ERR_ARG  # a dictionary of another context
    finally:
        other.close()
    a.close()
    b.close()
    pos, pid = host.search_dict(b"abcabc", ["abc", "c", "bc"])  # the module-level entry point
    assert pos.tolist() == [0, 1, 2, 3, 4, 5] and pid.tolist() == [0, 2, 1, 0, 2, 1]


def test_cli_dict(tmp_path):
    text = golden_file_bytes("input5L.txt.gz")
    (tmp_path / "input5L.txt").write_bytes(text)
    pats = [b"occurrences", b"string matching", b"occurrences starting fro"]
    (tmp_path / "words.txt").write_bytes(b"\n".join(pats) + b"\n")
    want_p, want_i = dict_matches(text, pats)
    r = subprocess.run([CLI, "--dict", str(tmp_path / "words.txt"), "--text", str(tmp_path / "input5L.txt"), "--iters",
                        "2", "--positions", "--max-print", "4"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = r.stdout
    assert "dictionary " in out and ": 3 patterns" in out
    assert f"dictionary matches: {want_p.size}" in out
    assert f"first match: {want_p[0]} (pattern {want_i[0]})" in out
    assert f"last match: {want_p[-1]} (pattern {want_i[-1]})" in out
    got = [(int(a), int(b)) for a, b in re.findall(r"Match at : (\d+) \(pattern (\d+)\)", out)]
    assert got == list(zip(want_p[:4].tolist(), want_i[:4].tolist()))
    assert "Average time" in out
