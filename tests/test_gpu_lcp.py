"""GPU suite for the LCP array (bmx_lcp_*): the kernels of csrc/bmx_lcp_kernel.h against the references of
tests/lcp_oracle.py -- small texts over five alphabets, arbitrary permutations, both sides of the one-lane budget, long
pairs and reducible chains across tiles, a text longer than one grid, unaligned views, arrays that are no permutation,
the statistics, a caller's non-blocking stream and workspace reuse."""
import numpy as np
import pytest

import index_oracle as io
import lcp_oracle as lo
from conftest import golden_file_bytes
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 7, 8, 9, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 70001)
ALPHABETS = {"ab": b"ab", "26 letters": bytes(range(97, 123)), "_`aA": b"_`aA", "a`\\x80Z": b"a`\x80Z",
             "printable": bytes(range(32, 127))}


def dev(x):
    import torch

    return torch.from_numpy(np.frombuffer(io.as_bytes(x), np.uint8).copy()).to("cuda:0")


def device_lcp(ctx, text):
    """(sa, lcp) as numpy through the two device entries."""
    d_text = dev(text)
    d_sa = ctx.suffix_array_device(d_text)
    return d_sa.cpu().numpy(), ctx.lcp_array_device(d_text, d_sa).cpu().numpy()


def check_stats(ctx, d_lcp, lcp: np.ndarray):
    mx = int(lcp.max())
    for min_len in (0, 1, mx, mx + 1):
        got = ctx.lcp_stats_device(d_lcp, min_len)
        want = {"max": mx, "argmax": int(lcp.argmax()), "sum": int(lcp.astype(np.int64).sum()), "count": int((lcp >= min_len).sum())}
        assert got == want, (min_len, got, want)


@pytest.mark.parametrize("name", list(ALPHABETS))
def test_small_texts(name, ctx):
    import torch

    rng = np.random.default_rng(0x1C9 + len(name))
    for n in SIZES:
        t = io.random_text(rng, n, ALPHABETS[name])
        sa, lcp = ctx.lcp_array(t)
        want = lo.brute(t, sa)
        assert np.array_equal(lcp, want), (name, n, np.nonzero(lcp != want)[0][:8].tolist())
        assert ctx.last_lcp_ms() > 0
        sa_d, lcp_d = device_lcp(ctx, t)
        assert np.array_equal(sa_d, sa) and np.array_equal(lcp_d, lcp), (name, n)
        check_stats(ctx, torch.from_numpy(lcp).to("cuda:0"), lcp)


def test_arbitrary_permutation(ctx):
    import torch

    rng = np.random.default_rng(0xA2B)
    t = io.random_text(rng, 4097, b"ab")
    perm = rng.permutation(4097).astype(np.int32)
    got = ctx.lcp_array_device(dev(t), torch.from_numpy(perm).to("cuda:0")).cpu().numpy()
    assert np.array_equal(got, lo.brute(t, perm))


@pytest.mark.parametrize("delta", (-9, -8, -1, 0, 1, 7, 8, 9))
def test_both_sides_of_the_lane_budget(delta, ctx):
    L = host.LCP_LANE_BYTES + delta
    for pad in range(8):  # both alignments of both streams
        t, p, q = lo.embedded_pair(L, pad)
        sa, lcp = device_lcp(ctx, t)
        assert np.array_equal(lcp, lo.brute(t, sa)), (L, pad)
        assert int(lcp.max()) == L
        long_pairs = ctx.last_lcp_long_pairs()
        assert long_pairs == 0 if L <= host.LCP_LANE_BYTES else long_pairs >= 1, (L, pad, long_pairs)


def test_one_letter_is_one_long_pair(ctx):
    n = 70001
    sa, lcp = device_lcp(ctx, b"a" * n)
    assert np.array_equal(sa, np.arange(n - 1, -1, -1)) and np.array_equal(lcp, np.arange(n))
    assert ctx.last_lcp_long_pairs() == 1


def test_two_letters_repeated(ctx):
    n = 70001
    x = np.tile(np.frombuffer(b"ab", np.uint8), n // 2 + 1)[:n].copy()
    sa, lcp = device_lcp(ctx, x)
    assert np.array_equal(lcp, lo.periodic(x, 2, sa))


@pytest.mark.parametrize("period", (61, 8))
def test_periodic_text(period, ctx):
    rng = np.random.default_rng(period)
    n = 150_000
    para = (rng.integers(0, 26, period) + 97).astype(np.uint8)
    x = np.tile(para, n // period + 1)[:n].copy()
    sa, lcp = device_lcp(ctx, x)
    assert np.array_equal(lcp, lo.periodic(x, period, sa))
    assert ctx.last_lcp_long_pairs() >= 1


def test_fibonacci_word(ctx):
    a, b = b"a", b"ab"
    while len(b) < 28_000:
        a, b = b, b + a
    sa, lcp = device_lcp(ctx, b)  # (lower case: the array is lexicographic)
    assert np.array_equal(lcp, lo.kasai(b, sa))


def test_the_reference_corpus(ctx):
    """The corpus holds capitals and punctuation, so the builder's order is not lexicographic on it and kasai does not
    apply; it is not exactly periodic either.  Every entry is checked by lcp_oracle.wrong_entries instead."""
    raw = golden_file_bytes("input5L.txt.gz")
    sa, lcp = device_lcp(ctx, raw)
    assert lo.wrong_entries(raw, sa, lcp).size == 0
    assert int(lcp.max()) > len(raw) // 2 and ctx.last_lcp_long_pairs() >= 1


def test_longer_than_one_grid(ctx):
    """All 'a', n = 65,536 x 256 + 4,097, the array given as n-1 .. 0: one pair of n - 1 bytes, everything else reducible."""
    import torch

    n = 65536 * 256 + 4097
    d_text = torch.full((n,), ord("a"), dtype=torch.uint8, device="cuda:0")
    d_sa = torch.arange(n - 1, -1, -1, dtype=torch.int32, device="cuda:0")
    d_lcp = ctx.lcp_array_device(d_text, d_sa)
    assert bool(torch.equal(d_lcp, torch.arange(n, dtype=torch.int32, device="cuda:0")))
    assert ctx.last_lcp_long_pairs() == 1
    assert ctx.lcp_stats_device(d_lcp, n - 1) == {"max": n - 1, "argmax": n - 1, "sum": n * (n - 1) // 2, "count": 1}


@pytest.mark.parametrize("offset", (1, 3, 7))
def test_nothing_past_n_at_any_alignment(offset, ctx):
    import torch

    n = 4097
    buf = torch.full((n + 64,), ord("a"), dtype=torch.uint8, device="cuda:0")
    view = buf[offset:offset + n]
    d_sa = torch.arange(n - 1, -1, -1, dtype=torch.int32, device="cuda:0")
    got = ctx.lcp_array_device(view, d_sa)
    assert bool(torch.equal(got, torch.arange(n, dtype=torch.int32, device="cuda:0")))  # bytes past the view would give more
    built = ctx.suffix_array_device(view.clone())
    assert bool(torch.equal(built, d_sa))


@pytest.mark.parametrize("kind", ("entry equal to n", "entry of -1", "entry duplicated"))
def test_bad_arrays(kind, ctx):
    import torch

    n = 257
    rng = np.random.default_rng(n)
    t = io.random_text(rng, n, b"ab")
    d_text = dev(t)
    good = ctx.suffix_array_device(d_text)
    want = lo.brute(t, good.cpu().numpy())
    bad = good.clone()
    if kind == "entry equal to n":
        bad[100] = n
    elif kind == "entry of -1":
        bad[0] = -1
    else:
        bad[200] = bad[31]
    with pytest.raises(host.BmxError) as e:
        ctx.lcp_array_device(d_text, bad)
    assert e.value.rc == host.ERR_ARG
    assert np.array_equal(ctx.lcp_array_device(d_text, good).cpu().numpy(), want)  # the context is as good as before


def test_index_repeat_statistics(ctx):
    rng = np.random.default_rng(40)
    for name in ("ab", "_`aA", "printable"):
        for n in (1, 2, 5, 17, 40):
            t = io.random_text(rng, n, ALPHABETS[name])
            subs = {}
            for i in range(n):
                for m in range(1, n - i + 1):
                    subs.setdefault(t[i:i + m], []).append(i)
            longest = max((len(s) for s, at in subs.items() if len(at) >= 2), default=0)
            with ctx.index(dev(t)) as ix:
                assert ix.distinct_substrings() == len(subs), (name, t)
                length, p, q = ix.longest_repeat()
                assert length == longest, (name, t)
                if longest:
                    assert p != q and t[p:p + length] == t[q:q + length]
                else:
                    assert p is None and q is None
    assert host.longest_repeat(b"abracadabra") == (4, 7, 0) and host.longest_repeat(b"abc") == (0, None, None)
    sa, lcp = host.lcp_array(b"banana")
    assert sa.tolist() == [5, 3, 1, 0, 4, 2] and lcp.tolist() == [0, 1, 3, 0, 0, 2]


def test_index_keeps_its_lcp_and_its_answers(ctx):
    rng = np.random.default_rng(41)
    t = io.random_text(rng, 5000, b"abc")
    pats = [b"a", b"abc", b"cab", b"bbbbbbbbbbbbbb", b"ca"]
    with ctx.index(dev(t)) as ix:
        lo0, cnt0 = (v.clone() for v in ix.count(pats))
        off0, pos0, total0 = ix.locate(pats)
        first = ix.lcp()
        assert ix.lcp() is first
        assert np.array_equal(first.cpu().numpy(), lo.kasai(t, ix.sa.cpu().numpy()))
        lo1, cnt1 = ix.count(pats)
        off1, pos1, total1 = ix.locate(pats)
        assert bool((lo0 == lo1).all()) and bool((cnt0 == cnt1).all())
        assert total0 == total1 and bool((off0 == off1).all()) and bool((pos0 == pos1).all())
    assert ix._lcp is None


def test_on_a_callers_non_blocking_stream(ctx, port):
    """Text and array are still being produced on the stream when the two entries are called, and the output is consumed
    on it right after: a kernel, a memset or a copy of the library off that stream would read the decoy."""
    import torch
    from test_gpu_streams import Pending, delay, side_stream

    n = 100_000
    rng = np.random.default_rng(0x57A)
    real, decoy = ((rng.integers(0, 4, n) + 97).astype(np.uint8) for _ in range(2))
    sa_real, sa_decoy = port.suffix_array(real), port.suffix_array(decoy)
    want = lo.kasai(real.tobytes(), sa_real)
    assert not np.array_equal(want, lo.kasai(decoy.tobytes(), sa_decoy))
    d_real, d_sa_real = dev(real), torch.from_numpy(sa_real.astype(np.int32)).to("cuda:0")
    buf, sa_buf = dev(decoy), torch.from_numpy(sa_decoy.astype(np.int32)).to("cuda:0")
    out = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    s = side_stream()
    with torch.cuda.stream(s):
        delay(s)
        buf.copy_(d_real, non_blocking=True)
        sa_buf.copy_(d_sa_real, non_blocking=True)
        pending = Pending(s)
        pending.assert_outstanding("lcp_array_device")
        lcp = ctx.lcp_array_device(buf, sa_buf, out=out)
        total = lcp.to(torch.int64).sum()  # consumed on the stream
        stats = ctx.lcp_stats_device(lcp, 3)
    s.synchronize()
    got = lcp.cpu().numpy()
    assert np.array_equal(got, want)
    assert int(total) == int(want.astype(np.int64).sum()) == stats["sum"]
    assert stats["max"] == int(want.max()) and stats["argmax"] == int(want.argmax()) and stats["count"] == int((want >= 3).sum())


def test_repeated_calls_reuse_the_workspace(ctx):
    rng = np.random.default_rng(0xBEE)
    big, small = io.random_text(rng, 70001, b"abcd"), io.random_text(rng, 257, b"ab")
    first = device_lcp(ctx, big)
    assert np.array_equal(first[1], lo.kasai(big, first[0]))
    mid = device_lcp(ctx, small)
    assert np.array_equal(mid[1], lo.brute(small, mid[0]))
    again = device_lcp(ctx, big)
    assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1])
