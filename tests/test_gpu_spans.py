"""GPU suite for the match spans of the approximate search (bmx_approx_spans[_classes]_device, bmx_search_approx_spans,
bmx_cli --approx K --spans): the ends come from the search itself, every start, kept entry and distance is compared in full
with tests/spans_oracle.py."""
import os
import subprocess

import numpy as np
import pytest

import classes_oracle as co
from conftest import ROOT
from spans_oracle import select_best, span_starts
from test_spans_cpu import EXAMPLE_ALL, EXAMPLE_BEST, EXAMPLE_K, EXAMPLE_PAT, EXAMPLE_TEXT
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "parallel_implementation_of_string_matching_algorithms_opencl_amd", "bin", "bmx_cli")


def _dev(ctx, data, offset: int = 0):
    """data on the device, starting `offset` bytes into a buffer (any alignment)."""
    import torch

    data = bytes(data)
    buf = torch.zeros(len(data) + offset + 16, dtype=torch.uint8, device=f"cuda:{ctx.device}")
    if data:
        buf[offset:offset + len(data)] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(buf.device)
    return buf[offset:offset + len(data)]


def _np(t):
    return t.cpu().numpy().astype(np.int64)


def _search(ctx, d_text, pat, k, base_offset=0):
    """The list of ends as the search returns it: CUDA tensors.  pat: bytes, or member [m, 256] for classes."""
    cap = max(d_text.numel(), 1)
    if isinstance(pat, (bytes, bytearray)):
        e, d, total = ctx.search_approx_device(d_text, pat, k, capacity=cap, base_offset=base_offset)
    else:
        e, d, total = ctx.search_approx_classes_device(d_text, co.pack(pat), k, capacity=cap, base_offset=base_offset)
    assert total == e.numel()
    return e, d


def _check_list(ctx, d_text, text, pat, k, e, d, base_offset=0):
    """Both flag values on the list (e, d) against the oracle, in full."""
    arg = pat if isinstance(pat, (bytes, bytearray)) else co.pack(pat)
    ends, dist = _np(e) - base_offset, _np(d)
    want_s, want_d = span_starts(text, pat, k, ends)
    assert np.array_equal(want_d, dist)  # the search's own distances
    s0, e0, d0, t0 = ctx.approx_spans_device(d_text, arg, k, e, d, base_offset=base_offset)
    assert t0 == ends.size
    assert np.array_equal(_np(s0) - base_offset, want_s), (len(text), k)
    assert np.array_equal(_np(e0) - base_offset, ends) and np.array_equal(_np(d0), dist)
    keep = select_best(ends, dist, k)
    s1, e1, d1, t1 = ctx.approx_spans_device(d_text, arg, k, e, d, best=True, base_offset=base_offset)
    assert t1 == keep.size, (len(text), k, t1, keep.size)
    assert np.array_equal(_np(e1) - base_offset, ends[keep]), (len(text), k)
    assert np.array_equal(_np(d1), dist[keep])
    assert np.array_equal(_np(s1) - base_offset, want_s[keep]), (len(text), k)
    assert np.all(want_s <= ends) and np.all(ends - want_s + 1 >= len(pat) - dist) and np.all(ends - want_s + 1 <= len(pat) + dist)
    return want_s, keep


def _check(ctx, text, pat, k, offset=0, base_offset=0):
    d_text = _dev(ctx, text, offset)
    e, d = _search(ctx, d_text, pat, k, base_offset)
    return _check_list(ctx, d_text, text, pat, k, e, d, base_offset)


@pytest.mark.parametrize("chunk", range(10))
def test_random_cases_against_oracle(ctx, chunk):
    """300 cases in ten parts: n in 0..5000, m in 1..64, k < m, sigma in {2, 4, 95}, planted edited copies, device offset
    case % 16, both flag values."""
    rng = np.random.default_rng(0x5BA50 + chunk)
    for case in range(30 * chunk, 30 * chunk + 30):
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


@pytest.mark.parametrize("m", [1, 2, 31, 32, 33, 63, 64])
def test_word_boundaries_on_any_bytes(ctx, m):
    rng = np.random.default_rng(700 + m)
    text = rng.integers(0, 256, 3000).astype(np.uint8)
    pat = rng.integers(0, 256, m).astype(np.uint8)
    text[100:100 + m] = pat
    text[1000:1000 + m] = pat
    text[1000 + m // 2] ^= 0x55  # one substitution
    text[2000:2000 + m] = pat[::-1]
    text[2990:3000] = np.resize(pat, 10)  # a prefix at the very end
    for k in sorted({0, 1, m // 2, m - 1}):
        if k < m:
            _check(ctx, text.tobytes(), pat.tobytes(), k, offset=m % 16)


@pytest.mark.parametrize("offset", [0, 1, 15])
def test_clipped_windows_at_the_start_of_the_text(ctx, offset):
    """The pattern, and a copy missing its first two bytes, at offset 0 of the view: the window of the reported ends is
    clipped to j + 1 < m + k bytes, and nothing below text[0] may count (the bytes in front of the view ARE the pattern's
    first bytes, to make a read below text[0] show)."""
    import torch

    pat = b"clipped-windows!"
    m, k = len(pat), 6
    filler = b"\x00" * 40
    for head in (pat, pat[2:]):
        text = head + filler + pat + filler
        buf = torch.zeros(offset + len(text) + 16, dtype=torch.uint8, device="cuda")
        lead = (pat[:2] * 8)[-offset:] if offset else b""  # what a walk past text[0] would read
        buf[:offset + len(text)] = torch.from_numpy(np.frombuffer(lead + text, np.uint8).copy()).cuda()
        d_text = buf[offset:offset + len(text)]
        e, d = _search(ctx, d_text, pat, k)
        ends = _np(e)
        assert np.count_nonzero(ends + 1 < m + k) >= 5  # clipped windows are among the reported ends
        want_s, _ = _check_list(ctx, d_text, text, pat, k, e, d)
        assert want_s[0] == 0 and int(want_s.min()) == 0


def _dense_list(ctx):
    """ACGT, m = 8, k = 4 over 1 MiB: most positions are ends, in long runs.  (d_text, text, pat, k, ends, dist), made once."""
    if not hasattr(_dense_list, "made"):
        import torch

        n = 1 << 20
        d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
        ctx.gen_text(d_text, 0, 0x5BA4D, 1)
        text = d_text.cpu().numpy().tobytes()
        pat, k = b"ACGTTGCA", 4
        e, d = _search(ctx, d_text, pat, k)
        assert e.numel() > n // 2
        _dense_list.made = (d_text, text, pat, k, e, d)
    return _dense_list.made


def test_dense_list_selects_entry_for_entry(ctx):
    d_text, text, pat, k, e, d = _dense_list(ctx)
    _, keep = _check_list(ctx, d_text, text, pat, k, e, d)
    assert 0 < keep.size < e.numel() // 2
    assert ctx.last_spans_ms() >= 0


@pytest.mark.parametrize("length", [0, 1, host.SPANS_BLOCK - 1, host.SPANS_BLOCK, host.SPANS_BLOCK + 1, 3 * host.SPANS_BLOCK - 1,
                                    3 * host.SPANS_BLOCK, 3 * host.SPANS_BLOCK + 1, host.SPANS_TILE - 1, host.SPANS_TILE,
                                    host.SPANS_TILE + 1, 3 * host.SPANS_TILE - 1, 3 * host.SPANS_TILE, 3 * host.SPANS_TILE + 1])
def test_list_lengths_at_workgroup_edges(ctx, length):
    """A prefix of the dense list is a list too (the rule takes list neighbours literally): lengths 0, 1, and one and three
    workgroups' entries +- 1, for the starts kernel's workgroup and for the selection's."""
    d_text, text, pat, k, e, d = _dense_list(ctx)
    _check_list(ctx, d_text, text, pat, k, e[:length], d[:length])


def test_all_wildcards_keep_one_span(ctx):
    n = 100000
    rng = np.random.default_rng(8)
    text = rng.integers(0, 256, n).astype(np.uint8).tobytes()
    member = np.ones((8, 256), dtype=bool)
    d_text = _dev(ctx, text, 3)
    e, d = _search(ctx, d_text, member, 0)
    assert e.numel() == 99993
    s1, e1, d1, t1 = ctx.approx_spans_device(d_text, co.pack(member), 0, e, d, best=True)
    assert t1 == 1 and (int(s1[0]), int(e1[0]), int(d1[0])) == (n - 8, n - 1, 0)
    s0, e0, d0, t0 = ctx.approx_spans_device(d_text, co.pack(member), 0, e, d)
    assert t0 == 99993 and np.array_equal(_np(s0), _np(e) - 7)


@pytest.mark.parametrize("slot", ["first", "last"])
def test_survivor_at_a_workgroup_boundary(ctx, slot):
    """By construction: an exact occurrence gives three adjacent ends (1, 0, 1) of which the middle one is kept, one with a
    substitution gives a single end.  With one single in front the kept end of occurrence 682 is list entry 2048, the first
    slot of the selection's second workgroup; with none it is entry 2047, the last slot of the first.  Either reads its
    neighbour across the boundary."""
    pat, k = b"abcd", 1
    pieces = ([b"abxd"] if slot == "first" else []) + [b"abcd"] * 1400
    text = b"xxxxxx" + b"xxxxxx".join(pieces) + b"xxxxxx"
    d_text = _dev(ctx, text, 5)
    e, d = _search(ctx, d_text, pat, k)
    ends, dist = _np(e), _np(d)
    at = host.SPANS_TILE if slot == "first" else host.SPANS_TILE - 1
    assert dist[at] == 0 and dist[at - 1] == 1 and dist[at + 1] == 1 and ends[at + 1] - ends[at - 1] == 2
    want_s, keep = _check_list(ctx, d_text, text, pat, k, e, d)
    assert at in keep.tolist() and at - 1 not in keep.tolist() and at + 1 not in keep.tolist()
    assert keep.size == len(pieces)


def test_classes_singletons_and_an_iupac_primer(ctx):
    rng = np.random.default_rng(21)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    text = acgt[rng.integers(0, 4, 20000)].copy()
    primer = "GTGYCAGCMGCCGCGGTAA"
    member = co.parse(primer, co.IUPAC)
    for at, inst in ((500, b"GTGCCAGCAGCCGCGGTAA"), (5000, b"GTGTCAGCCGCCGCGGTAA"), (9000, b"GTGTCAGCCGCGCGGTAA"),
                     (15000, b"GTGACAGCAGCCGCGGTAA")):
        text[at:at + len(inst)] = np.frombuffer(inst, np.uint8)
    text = text.tobytes()
    k = 2
    d_text = _dev(ctx, text, 7)
    e, d = _search(ctx, d_text, member, k)
    assert e.numel() >= 8
    _check_list(ctx, d_text, text, member, k, e, d)
    # the library's own compiler gives the same classes, and so the same spans
    s_a, e_a, d_a, t_a = ctx.approx_spans_device(d_text, host.compile_classes(primer, host.CLASS_IUPAC), k, e, d, best=True)
    s_b, e_b, d_b, t_b = ctx.approx_spans_device(d_text, co.pack(member), k, e, d, best=True)
    assert t_a == t_b and np.array_equal(_np(s_a), _np(s_b)) and np.array_equal(_np(e_a), _np(e_b))
    # singleton classes: the string form's result
    pat = b"GTGTCAGCCGCCGCGGTAA"
    e2, d2 = _search(ctx, d_text, pat, k)
    e3, d3 = _search(ctx, d_text, co.singletons(pat), k)
    assert np.array_equal(_np(e2), _np(e3)) and np.array_equal(_np(d2), _np(d3))
    for best in (False, True):
        got_s = ctx.approx_spans_device(d_text, pat, k, e2, d2, best=best)
        got_c = ctx.approx_spans_device(d_text, co.pack(co.singletons(pat)), k, e2, d2, best=best)
        assert got_s[3] == got_c[3] and all(np.array_equal(_np(x), _np(y)) for x, y in zip(got_s[:3], got_c[:3]))
    _check_list(ctx, d_text, text, pat, k, e2, d2)


def test_permuted_list_and_no_distances(ctx):
    import torch

    rng = np.random.default_rng(31)
    text = (rng.integers(0, 2, 6000) + 0x61).astype(np.uint8)
    pat = text[3000:3020].copy().tobytes()
    text = text.tobytes()
    k = 5
    d_text = _dev(ctx, text, 9)
    e, d = _search(ctx, d_text, pat, k)
    assert e.numel() > 20
    want_s, _ = span_starts(text, pat, k, _np(e))
    perm = torch.from_numpy(rng.permutation(e.numel())).cuda()
    s_p, e_p, d_p, t_p = ctx.approx_spans_device(d_text, pat, k, e[perm].contiguous(), d[perm].contiguous())
    assert t_p == e.numel() and np.array_equal(_np(s_p), want_s[perm.cpu().numpy()])
    s_n, e_n, d_n, t_n = ctx.approx_spans_device(d_text, pat, k, e, None)
    assert t_n == e.numel() and d_n is None and np.array_equal(_np(s_n), want_s)


def test_base_offset_shifts_starts_and_ends(ctx):
    base = (1 << 33) + 7
    text = b"zz" + EXAMPLE_TEXT * 40
    want_s, keep = _check(ctx, text, EXAMPLE_PAT, EXAMPLE_K, offset=2, base_offset=base)
    assert keep.size == 3 * 40


def test_ends_around_4_gib(ctx):
    """A view of 4 GiB + 64 KiB: the pattern ends at 2^32 - 1 and again at 2^32 + m + 1; a hand-built list of the ends
    2^32 - 1, 2^32 and 2^32 + m + 1.  The oracle runs on the window around them only."""
    import torch

    n = (1 << 32) + (1 << 16)
    pat, k = b"four-gib-pattern", 2
    m = len(pat)
    d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
    ctx.gen_text(d_text, 0, 0x5BA46, 1)  # ACGT: no byte of the pattern
    ctx.plant(d_text, 0, pat, [(1 << 32) - m, (1 << 32) + 2])
    lo = (1 << 32) - 64
    window = d_text[lo:lo + 160].cpu().numpy().tobytes()
    ends = np.array([(1 << 32) - 1, 1 << 32, (1 << 32) + m + 1], dtype=np.int64)
    want_s, want_d = span_starts(window, pat, k, ends - lo)
    assert want_d.tolist() == [0, 1, 0] and (want_s + lo).tolist() == [(1 << 32) - m, (1 << 32) - m, (1 << 32) + 2]
    e = torch.from_numpy(ends).cuda()
    d = torch.from_numpy(want_d.astype(np.uint8)).cuda()
    s0, e0, d0, t0 = ctx.approx_spans_device(d_text, pat, k, e, d)
    assert t0 == 3 and np.array_equal(_np(s0), want_s + lo)
    s1, e1, d1, t1 = ctx.approx_spans_device(d_text, pat, k, e, d, best=True)
    assert list(zip(_np(s1).tolist(), _np(e1).tolist(), _np(d1).tolist())) == [((1 << 32) - m, (1 << 32) - 1, 0),
                                                                             ((1 << 32) + 2, (1 << 32) + m + 1, 0)]
    del d_text
    torch.cuda.empty_cache()


def test_errors_on_the_device_and_recovery(ctx):
    import torch

    text = b"zz" + EXAMPLE_TEXT * 10
    d_text = _dev(ctx, text, 4)
    e, d = _search(ctx, d_text, EXAMPLE_PAT, EXAMPLE_K)
    bad = e.clone()
    bad[3] = len(text)  # an end >= n: the kernel reads nothing for it
    with pytest.raises(host.BmxError) as err:
        ctx.approx_spans_device(d_text, EXAMPLE_PAT, EXAMPLE_K, bad, d)
    assert err.value.rc == host.ERR_ARG
    bad[3] = -5  # ... and one far outside (2^64 - 5)
    with pytest.raises(host.BmxError) as err:
        ctx.approx_spans_device(d_text, EXAMPLE_PAT, EXAMPLE_K, bad, None)
    assert err.value.rc == host.ERR_ARG
    with pytest.raises(host.BmxError) as err:  # a list that belongs to another pattern
        ctx.approx_spans_device(d_text, b"xdxx", EXAMPLE_K, e, d)
    assert err.value.rc == host.ERR_ARG
    with pytest.raises(host.BmxError) as err:  # the right ends with another list's distances
        ctx.approx_spans_device(d_text, EXAMPLE_PAT, EXAMPLE_K, e, torch.zeros_like(d), best=True)
    assert err.value.rc == host.ERR_ARG
    s, e2, d2, t = ctx.approx_spans_device(d_text, EXAMPLE_PAT, EXAMPLE_K, e, d, best=True)  # the status word is reset
    assert t == 30 and _np(s)[:3].tolist() == [4, 10, 16]


def test_call_on_a_non_blocking_stream(ctx):
    import torch

    text = (b"zz" + EXAMPLE_TEXT) * 3000
    d_text = _dev(ctx, text, 1)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        e, d = _search(ctx, d_text, EXAMPLE_PAT, EXAMPLE_K)
    s1, e1, d1, t1 = ctx.approx_spans_device(d_text, EXAMPLE_PAT, EXAMPLE_K, e, d, best=True, stream=side)
    got = (_np(s1), _np(e1), _np(d1))  # valid after return: no further synchronisation here
    want_s, _ = span_starts(text, EXAMPLE_PAT, EXAMPLE_K, _np(e))
    keep = select_best(_np(e), _np(d), EXAMPLE_K)
    assert t1 == keep.size == 9000
    assert np.array_equal(got[0], want_s[keep]) and np.array_equal(got[1], _np(e)[keep]) and np.array_equal(got[2], _np(d)[keep])
    assert ctx.last_spans_ms() >= 0


def test_host_entry_points_on_the_worked_example(ctx):
    for best, want in ((False, EXAMPLE_ALL), (True, EXAMPLE_BEST)):
        s, e, d = ctx.search_approx_spans(EXAMPLE_TEXT, EXAMPLE_PAT, EXAMPLE_K, best=best)
        assert list(zip(s.tolist(), e.tolist(), d.tolist())) == want
        s, e, d = ctx.search_approx_spans_classes(EXAMPLE_TEXT, "ab[c]d", EXAMPLE_K, best=best)
        assert list(zip(s.tolist(), e.tolist(), d.tolist())) == want
    s, e, d = host.search_approx_spans(EXAMPLE_TEXT, "abcd", 1)  # the module-level entry point: best by default
    assert list(zip(s.tolist(), e.tolist(), d.tolist())) == EXAMPLE_BEST
    s, e, d = ctx.search_approx_spans_classes(EXAMPLE_TEXT, "AB.D", 0, flags=host.CLASS_ICASE)
    assert list(zip(s.tolist(), e.tolist(), d.tolist())) == [(2, 5, 0), (8, 11, 0)]
    s, e, d = ctx.search_approx_spans(b"", EXAMPLE_PAT, 1)
    assert s.size == e.size == d.size == 0
    s, e, d = ctx.search_approx_spans(b"no hit in here", b"qqqq", 1)
    assert s.size == 0
    assert ctx.last_spans_ms() >= 0


def test_host_entry_capacity(ctx):
    import ctypes as C

    starts = np.zeros(8, np.uint64)
    ends = np.zeros(8, np.uint64)
    dist = np.zeros(8, np.uint8)
    total = C.c_uint64(0)

    def call(flags, cap):
        return ctx._L.bmx_search_approx_spans(ctx._h, EXAMPLE_TEXT, len(EXAMPLE_TEXT), EXAMPLE_PAT, 4, 1, flags,
                                              C.c_void_p(starts.ctypes.data), C.c_void_p(ends.ctypes.data),
                                              C.c_void_p(dist.ctypes.data), cap, C.byref(total))

    assert call(1, 0) == host.ERR_CAPACITY and total.value == 3  # counting only
    assert call(1, 2) == host.ERR_CAPACITY and total.value == 3  # the lowest two, after a search that had to run twice
    assert list(zip(starts[:2].tolist(), ends[:2].tolist(), dist[:2].tolist())) == EXAMPLE_BEST[:2]
    assert call(1, 3) == host.OK and total.value == 3
    assert list(zip(starts[:3].tolist(), ends[:3].tolist(), dist[:3].tolist())) == EXAMPLE_BEST
    assert call(0, 4) == host.ERR_CAPACITY and total.value == 5
    assert list(zip(starts[:4].tolist(), ends[:4].tolist(), dist[:4].tolist())) == EXAMPLE_ALL[:4]
    assert call(0, 8) == host.OK and total.value == 5


def test_spans_through_the_cli(ctx, tmp_path):
    (tmp_path / "text.txt").write_bytes(EXAMPLE_TEXT)
    (tmp_path / "pat.txt").write_bytes(EXAMPLE_PAT)
    base = [CLI, "--approx", "1", "--text", str(tmp_path / "text.txt"), "--iters", "1"]

    def spans_of(out):
        lines = out.splitlines()
        at = next(i for i, line in enumerate(lines) if line.startswith("match spans"))
        return lines[at], [tuple(int(x) for x in line.split()) for line in lines[at + 1:] if line[:1].isdigit()]

    plain = subprocess.run(base + ["--pattern", str(tmp_path / "pat.txt")], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and "match spans" not in plain.stdout
    r = subprocess.run(base + ["--pattern", str(tmp_path / "pat.txt"), "--spans"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "approximate matches (k = 1): 5" in r.stdout  # what --approx prints stays
    head, got = spans_of(r.stdout)
    assert head.startswith("match spans: 5") and got == EXAMPLE_ALL
    r = subprocess.run(base + ["--pattern", str(tmp_path / "pat.txt"), "--spans", "--best"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    head, got = spans_of(r.stdout)
    assert head.startswith("match spans (best): 3") and got == EXAMPLE_BEST
    r = subprocess.run(base + ["--classes", "AB[cx]D", "--icase", "--spans", "--best", "--max-print", "2"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    head, got = spans_of(r.stdout)
    assert head.startswith("match spans (best): 3") and got == [(2, 5, 0), (8, 11, 0)] and "... 1 more" in r.stdout
    for bad in (["--spans"], ["--approx", "1", "--best"]):  # --spans needs --approx, --best needs --spans
        r = subprocess.run([CLI, "--text", str(tmp_path / "text.txt"), "--pattern", str(tmp_path / "pat.txt")] + bad,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 2
