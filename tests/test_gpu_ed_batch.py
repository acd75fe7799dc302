"""GPU suite for the batched edit distance (bmx_edit_distance_batch*): every distance of every case of
tests/ed_batch_cases.py against the oracle's port -- random pairs in both argument orders, the length grid around the
32- and 64-byte words, limits, one against many, the pair-by-pair path and the long-walk bound, blobs past 4 GiB, bad
offsets caught on the device, streams, repeated calls, the host entry and bmx_cli.  Nothing compares the feature with
itself except where a second route to the same answer is the point (pairwise against one-against-many, stream against
stream), and there the oracle has checked one of the two.

The cases aimed at one path of the kernel each (cases.kernel_paths is the model of its dispatch, and
tests/test_ed_batch_cpu.py asserts that every generator reaches what it claims): word_column, every bit-vector length on
the 32-bit and on the 64-bit pairwise instantiation; blob_end_calls, the pattern at the stated end of its blob on either
side of the byte-by-byte threshold; shared_calls and long_shared, one Peq in LDS for queries of every length 1..64 with
bytes >= 0x80 and candidates of up to 200,000 bytes; growth_pairs, a list of pairs for the pair-by-pair path that
outgrows its first 4,096 entries twice; spans of 2^31 - 1 and 2^31 bytes on the blobs of the 4 GiB test, none of them
walked; and limit = 2^32 - 2."""
import os
import subprocess

import numpy as np
import pytest

import ed_batch_cases as cases
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

pytestmark = pytest.mark.gpu


def to_device(strings):
    """(blob uint8, offsets int64) CUDA tensors of a string column."""
    import torch

    blob, off = host.pack_strings(strings)
    return torch.from_numpy(blob.copy()).cuda(), torch.from_numpy(off.view(np.int64).copy()).cuda()


def run_device(ctx, a, b, limit=None, one=False):
    da, dao = to_device([a] if one else a)
    db, dbo = to_device(b)
    out = ctx.edit_distance_batch_device(da, dao, db, dbo, len(b), a_count=1 if one else len(b), limit=limit)
    return out.cpu().numpy().view(np.uint32)


def assert_same(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} differ, first at {bad[:5]}: got {got[bad[:5]]}, want {want[bad[:5]]}"


@pytest.fixture(scope="module")
def random_case(port):
    a, b = cases.random_pairs()
    return a, b, cases.expected(port, a, b)


def test_random_pairs_both_orders(ctx, random_case):
    a, b, want = random_case
    assert len(b) >= 20000
    assert_same(run_device(ctx, a, b), want, "a against b")
    assert ctx.last_ed_batch_fallbacks() == cases.n_fallback(a, b)
    assert ctx.last_ed_batch_ms() > 0
    assert_same(run_device(ctx, b, a), want, "b against a")


def test_length_grid_and_fallback_count(ctx, port):
    a, b = cases.grid_pairs()
    want = cases.expected(port, a, b)
    assert_same(run_device(ctx, a, b), want, "grid")
    both_long = sum(1 for x, y in zip(a, b) if len(x) > 64 and len(y) > 64)  # counted here, not by the library
    assert both_long == 9
    assert ctx.last_ed_batch_fallbacks() == both_long
    assert_same(run_device(ctx, b, a), want, "grid, sides swapped")
    assert ctx.last_ed_batch_fallbacks() == both_long


def test_long_pairs_and_long_walk_bound(ctx, port):
    a, b = cases.long_pairs()
    want = cases.expected(port, a, b)
    assert_same(run_device(ctx, a, b), want, "long pairs")
    n_fb = cases.n_fallback(a, b, host.ED_BATCH_LONG)
    assert 0 < n_fb <= cases.MAX_FALLBACK_PAIRS
    assert ctx.last_ed_batch_fallbacks() == n_fb
    assert_same(run_device(ctx, a, b, limit=5), cases.clamp(want, 5), "long pairs, limit 5")
    assert ctx.last_ed_batch_fallbacks() <= n_fb  # a length difference above the limit needs no bytes


@pytest.mark.parametrize("limit", cases.LIMITS)
def test_limit(ctx, random_case, limit):
    a, b, want = random_case
    if limit is None:
        da, dao = to_device(a)
        db, dbo = to_device(b)
        got = ctx.edit_distance_batch_device(da, dao, db, dbo, len(b), limit=host.ED_NO_LIMIT).cpu().numpy().view(np.uint32)
    else:
        got = run_device(ctx, a, b, limit=limit)
    assert_same(got, cases.clamp(want, limit), f"limit {limit}")


@pytest.mark.parametrize("qlen", cases.QUERY_LENGTHS)
def test_one_against_many(ctx, port, qlen):
    q, cand = cases.one_vs_many(qlen)
    assert len(cand) == 10000
    want = cases.expected(port, [q], cand)
    got = run_device(ctx, q, cand, one=True)
    assert_same(got, want, f"query of {qlen} bytes")
    n_fb = cases.n_fallback([q] * len(cand), cand)
    assert ctx.last_ed_batch_fallbacks() == n_fb <= cases.MAX_FALLBACK_PAIRS
    pairwise = run_device(ctx, [q] * len(cand), cand)
    assert_same(pairwise, want, f"query of {qlen} bytes, repeated")
    assert ctx.last_ed_batch_fallbacks() == n_fb
    assert_same(run_device(ctx, q, cand, limit=3, one=True), cases.clamp(want, 3), f"query of {qlen} bytes, limit 3")


def test_limit_just_below_no_limit(ctx, random_case):
    """limit = 2^32 - 2, the largest that is a limit: limit + 1 must not wrap in the kernel's clamp, in its length test
    or in the host's clamp of the listed pairs, so the distances come back unclamped."""
    a, b, want = random_case
    a, b, want = a[:2000], b[:2000], want[:2000]
    assert cases.n_fallback(a, b) > 0  # listed pairs among them: the host's clamp runs too
    assert_same(run_device(ctx, a, b, limit=2**32 - 2), want, "limit 2^32 - 2")
    assert ctx.last_ed_batch_fallbacks() == cases.n_fallback(a, b)


def listed(paths):
    return sum(1 for p, _ in paths if p == cases.LISTED)


def test_word_column_both_orders(ctx, port):
    """Every bit-vector length on the 32-bit and on the 64-bit pairwise instantiation, four alphabets, either side as the
    bit vector (tests/test_ed_batch_cpu.py asserts that the column reaches them)."""
    a, b = cases.word_column()
    want = cases.expected(port, a, b)
    assert_same(run_device(ctx, a, b), want, "word column")
    assert ctx.last_ed_batch_fallbacks() == 0
    assert_same(run_device(ctx, b, a), want, "word column, sides swapped")
    assert ctx.last_ed_batch_fallbacks() == 0


def test_blob_end_calls(ctx, port):
    """The pattern at the stated end of its blob: every m on both words, with the slack that still takes the last chunk
    byte by byte and the first that does not, the patterns as a and as b.  One upload per column; a call compares the
    first `count` pairs and states off[count] + slack bytes.  The bytes behind the stated end are the next pattern's, so a
    load that ran past it would go unnoticed here: tests/ed_batch_check.hip is what catches that.  This pins the
    distances of the compiled kernel on either side of the threshold."""
    import torch

    n_calls = 0
    for col in cases.blob_end_calls():
        pat, txt = col["pat"], col["txt"]
        want = cases.expected(port, pat[:-1], txt)
        d_pat, d_pat_off = to_device(pat)
        d_txt, d_txt_off = to_device(txt)
        off = d_pat_off.cpu().numpy()
        out = torch.empty(len(txt), dtype=torch.int32, device="cuda")
        for count, slack in col["calls"]:
            end = int(off[count]) + slack
            for pattern_first in (True, False):
                if pattern_first:
                    got = ctx.edit_distance_batch_device(d_pat[:end], d_pat_off, d_txt, d_txt_off, count, out=out)
                else:
                    got = ctx.edit_distance_batch_device(d_txt, d_txt_off, d_pat[:end], d_pat_off, count, out=out)
                assert_same(got.cpu().numpy().view(np.uint32), want[:count],
                            f"word {col['word']}, count {count}, slack {slack}, pattern {'a' if pattern_first else 'b'}")
                assert ctx.last_ed_batch_fallbacks() == 0
                n_calls += 1
    assert n_calls == 540


def shared_and_pairwise(ctx, port, q, cand, limits=()):
    """One against many (the Peq in LDS), then the pairwise call with the query repeated (the bit vector in registers):
    both Eq sources answer the same pairs, each against the oracle.  Returns the two fallback counts."""
    want = cases.expected(port, [q], cand)
    dq, dqo = to_device([q])
    dr, dro = to_device([q] * len(cand))
    db, dbo = to_device(cand)
    what = f"query of {len(q)} bytes"
    got = ctx.edit_distance_batch_device(dq, dqo, db, dbo, len(cand), a_count=1)
    assert_same(got.cpu().numpy().view(np.uint32), want, what)
    fb_shared = ctx.last_ed_batch_fallbacks()
    got = ctx.edit_distance_batch_device(dr, dro, db, dbo, len(cand))
    assert_same(got.cpu().numpy().view(np.uint32), want, what + ", repeated")
    fb_pairwise = ctx.last_ed_batch_fallbacks()
    for limit in limits:
        got = ctx.edit_distance_batch_device(dq, dqo, db, dbo, len(cand), a_count=1, limit=limit)
        assert_same(got.cpu().numpy().view(np.uint32), cases.clamp(want, limit), what + f", limit {limit}")
        got = ctx.edit_distance_batch_device(dr, dro, db, dbo, len(cand), limit=limit)
        assert_same(got.cpu().numpy().view(np.uint32), cases.clamp(want, limit), what + f", repeated, limit {limit}")
    return fb_shared, fb_pairwise


def test_shared_calls_every_query_length(ctx, port):
    """Queries of 1..64 bytes over 256 symbols, bytes >= 0x80 indexing the Peq, two workgroups building it."""
    for q, cand in cases.shared_calls():
        limits = (3,) if len(q) in cases.SHARED_LIMIT_LENGTHS else ()
        assert shared_and_pairwise(ctx, port, q, cand, limits) == (0, 0)


def test_long_shared_candidates(ctx, port):
    """Kernel 2 walks a candidate whatever its length: 65,536, 65,537 and 200,000 bytes among short ones, none listed.
    As the pairwise call the two over BMX_ED_BATCH_LONG go through the list."""
    for q, cand in cases.long_shared():
        lc = cases.lengths(cand)
        assert listed(cases.kernel_paths([len(q)], lc, one=True)) == 0
        assert shared_and_pairwise(ctx, port, q, cand) == (0, listed(cases.kernel_paths([len(q)] * len(cand), lc)))


@pytest.fixture(scope="module")
def growth(port, built):
    """A context of its own, so that the list of pairs for the pair-by-pair path starts at its first 4,096 entries
    whatever ran before, the three columns on the device and their expected values."""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = host.Context(0)
    cols = []
    for a, b in cases.growth_pairs():
        cols.append((to_device(a), to_device(b), cases.expected(port, a, b), cases.kernel_paths(cases.lengths(a), cases.lengths(b)),
                     cases.kernel_paths(cases.lengths(a), cases.lengths(b), limit=2)))
    yield c, cols
    c.close()


def growth_call(c, col, limit, what):
    import torch

    (da, dao), (db, dbo), want, paths, paths_2 = col
    out = torch.full((want.size + 7,), -1, dtype=torch.int32, device="cuda")  # guard entries behind count
    got = c.edit_distance_batch_device(da, dao, db, dbo, want.size, limit=limit, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert_same(got.cpu().numpy().view(np.uint32), cases.clamp(want, limit), what)
    assert bool((out[want.size:] == -1).all()), what
    assert c.last_ed_batch_fallbacks() == listed(paths if limit is None else paths_2), what


def test_list_growth_three_calls(growth):
    """4,097 listed pairs (the list's first 4,096 entries do not hold them: a second kernel pass, a new list, the answers
    behind the NEW capacity, a scatter kernel of 17 workgroups), then 6,000 (it grows again), then 10 (the large list
    stays), in order on one context."""
    c, cols = growth
    assert [listed(col[3]) for col in cols] == list(cases.GROWTH_LISTED)
    for (k, limit) in cases.GROWTH_SEQUENCES["grow"]:
        growth_call(c, cols[k], limit, f"growth call {k}")


def test_list_growth_first_column_again_and_limit(growth):
    """After test_list_growth_three_calls on the same context: the first column again, now into a list of 6,000 entries
    (more capacity than pairs: the answers lie behind the capacity, not behind the pairs), and with limit = 2, where the
    host clamps the listed answers and the kernel answers some of the long pairs from their offsets.  Split from the
    three calls to keep the listed pairs of one test under cases.MAX_GROWTH_LISTED; run alone it still checks every
    distance, on a list that grows in its first call."""
    c, cols = growth
    for (k, limit) in cases.GROWTH_SEQUENCES["repeat"]:
        growth_call(c, cols[k], limit, f"first column again, limit {limit}")


def test_blobs_past_4_gib(ctx, port):
    """Both blobs generated in HBM, b = a with 0..3 bytes per string replaced at known places, the offsets built on the
    device; every result against what the plants allow, 20,000 pairs against the oracle."""
    import torch

    n_bytes = (4 << 30) + (1 << 20) + 123
    period = 23
    lens = np.array([20 + (7 * j) % period for j in range(period)], dtype=np.int64)  # 20 .. 42 bytes
    prefix = torch.from_numpy(np.concatenate(([0], np.cumsum(lens)))).cuda()
    per = int(lens.sum())
    count = (n_bytes // per) * period
    i = torch.arange(count + 1, dtype=torch.int64, device="cuda")
    off = (i // period) * per + prefix[i % period]
    del i
    assert int(off[-1]) > 1 << 32 and int(off[-1]) <= n_bytes
    a = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    ctx.gen_text(a, 0, 0xED4B16, 0)
    b = a.clone()
    k = torch.arange(count, dtype=torch.int64, device="cuda") % 4  # replaced bytes of pair i
    for j in range(3):
        at = off[:-1][k > j] + (3 + 5 * j)
        b[at] = b[at] ^ 1  # a printable byte with its lowest bit flipped is another byte
        del at
    d = ctx.edit_distance_batch_device(a, off, b, off, count)
    assert ctx.last_ed_batch_fallbacks() == 0
    # equal lengths and k replaced bytes: 0 < d <= k, and 0 only where nothing was replaced
    assert bool(((d <= k) & ((d == 0) == (k == 0))).all())
    del k
    rng = np.random.default_rng(0x46B)
    inner = np.unique(rng.integers(1000, count - 1000, 19000))
    rng.shuffle(inner)
    pick = np.sort(np.concatenate((np.arange(1000), inner[:18000], np.arange(count - 1000, count))))
    assert pick.size == 20000 and pick[999] == 999 and pick[-1000] == count - 1000
    pick_d = torch.from_numpy(pick).cuda()
    start = off[pick_d]
    length = (off[pick_d + 1] - start).cpu().numpy()
    span = (start[:, None] + torch.arange(int(lens.max()), device="cuda")[None, :]).clamp_(max=n_bytes - 1)
    rows_a, rows_b = a[span].cpu().numpy(), b[span].cpu().numpy()
    got = d[pick_d].cpu().numpy()
    assert int(start.max()) > 1 << 32
    for r in range(pick.size):
        x, y = rows_a[r, :length[r]].tobytes(), rows_b[r, :length[r]].tobytes()
        assert got[r] == port.edit_distance(x, y), (r, int(pick[r]))
    spans_at_the_2_31_bound(ctx, a, b, off, d)


def spans_at_the_2_31_bound(ctx, a, b, off, d):
    """On the two blobs of test_blobs_past_4_gib (they are the only ones large enough; not allocated a second time), one
    pair per call.  No call here lets a lane or the single-pair path walk a string of 2 GiB, which would hold the GPU for
    minutes: every pair is one the kernel rejects or answers from its offsets alone, the model says so before the call is
    made, and the rejected ones carry limit = 0, under which a kernel that failed to reject them would answer them from
    their offsets too (and fail the test by not raising)."""
    import torch

    top = 1 << 31
    dev = lambda *v: torch.tensor(v, dtype=torch.int64, device="cuda")
    assert a.numel() > top and b.numel() > top
    for ao, bo in ((dev(0, top), dev(0, 5)), (dev(0, 5), dev(0, top)), (dev(7, top + 7), dev(2, 7))):
        with pytest.raises(host.BmxError) as e:  # a span of exactly 2^31 bytes
            ctx.edit_distance_batch_device(a, ao, b, bo, 1, limit=0)
        assert e.value.rc == host.ERR_ARG
    for la, lb, limit, want in ((top - 1, 5, 10, 11), (5, top - 1, 10, 11), (top - 1, 0, None, top - 1), (0, top - 1, None, top - 1)):
        assert cases.kernel_paths([la], [lb], limit=limit) == [(cases.OFFSETS, False)]
        got = ctx.edit_distance_batch_device(a, dev(3, 3 + la), b, dev(1, 1 + lb), 1, limit=limit)
        assert got.tolist() == [want], (la, lb, limit)
        assert ctx.last_ed_batch_fallbacks() == 0
    again = ctx.edit_distance_batch_device(a, off, b, off, 1000)  # and an ordinary call afterwards
    assert torch.equal(again, d[:1000]) and ctx.last_ed_batch_fallbacks() == 0


def test_bad_offsets_on_the_device(ctx):
    """Offsets that decrease, or end past the blob size passed in, come back as BMX_ERR_ARG.  What keeps this test from
    reading outside memory is the kernel's own check, which reads no string byte of a pair with bad offsets.  The arena
    adds a second guard for two readings only: every offset lies inside the blob and the blob is the start of a 1 MiB
    allocation, so a length taken as signed (-24: nothing to read) stays inside, and so does the string that ends past the
    stated 1,000 bytes.  A kernel that took the decreasing pair's length as unsigned would not be held by the arena."""
    import torch

    arena = torch.full((1 << 20,), 65, dtype=torch.uint8, device="cuda")
    blob = arena[:4096]
    good = torch.arange(0, 65 * 16, 16, dtype=torch.int64, device="cuda")  # 64 strings of 16 bytes
    for at in (2, 33, 64):
        bad = good.clone()
        bad[at] = bad[at - 1] - 8  # off[at] < off[at - 1]
        for ao, bo in ((bad, good), (good, bad)):
            with pytest.raises(host.BmxError) as e:
                ctx.edit_distance_batch_device(blob, ao, blob, bo, 64)
            assert e.value.rc == host.ERR_ARG
    with pytest.raises(host.BmxError) as e:  # the last offset past the size the caller states
        ctx.edit_distance_batch_device(blob[:1000], good, blob, good, 64)
    assert e.value.rc == host.ERR_ARG
    with pytest.raises(host.BmxError) as e:  # one against many: the query's two offsets
        ctx.edit_distance_batch_device(blob, torch.tensor([32, 16], device="cuda"), blob, good, 64, a_count=1)
    assert e.value.rc == host.ERR_ARG
    out = ctx.edit_distance_batch_device(blob, good, blob, good, 64)  # and the context is as good as before
    assert not out.any()


def test_null_stream_and_callers_stream(ctx, random_case):
    """The same call on the null stream and on a caller's non-blocking stream, with the caller's own work queued on that
    stream in front of the call (the blobs are produced there) and behind it (the result is consumed there)."""
    import torch

    a, b, want = random_case
    da, dao = to_device(a)
    db, dbo = to_device(b)
    on_null = ctx.edit_distance_batch_device(da, dao, db, dbo, len(b)).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        junk = torch.zeros(64 << 20, dtype=torch.uint8, device="cuda")
        for _ in range(8):
            junk += 1  # the caller's work in front
        da2, db2 = da ^ (junk[:da.numel()] - 8), db ^ (junk[:db.numel()] - 8)  # == da, db once the additions are done
        out = torch.full((len(b),), -1, dtype=torch.int32, device="cuda")
        got = ctx.edit_distance_batch_device(da2, dao, db2, dbo, len(b), out=out)
        after = got + junk[:len(b)].to(torch.int32)  # the caller's work behind
    side.synchronize()
    assert torch.equal(got, on_null)
    assert torch.equal(after, on_null + 8)
    assert_same(on_null.cpu().numpy().view(np.uint32), want, "null stream")


def test_repeated_calls_host_entry_and_cli(ctx, random_case, tmp_path):
    import torch

    a, b, want = random_case
    da, dao = to_device(a)
    db, dbo = to_device(b)
    out = torch.full((len(b) + 7,), -1, dtype=torch.int32, device="cuda")
    for count in (1, 300, 5000, len(b), 257, 0, 64, len(b)):  # growing and shrinking on one context
        got = ctx.edit_distance_batch_device(da, dao, db, dbo, count, out=out)
        assert got.numel() == count and (count == 0 or got.data_ptr() == out.data_ptr())
        assert_same(got.cpu().numpy().view(np.uint32), want[:count], f"count {count}")
        assert bool((out[len(b):] == -1).all())
    # the host entry, lists and (blob, offsets) pairs, and the module-level function
    assert_same(ctx.edit_distance_batch(a[:3000], b[:3000]), want[:3000], "host entry")
    assert_same(ctx.edit_distance_batch(host.pack_strings(a), host.pack_strings(b), limit=2), cases.clamp(want, 2), "host, packed")
    assert ctx.edit_distance_batch([], []).size == 0
    assert ctx.edit_distance_batch("kitten", ["sitting", b"kitten", ""]).tolist() == [3, 0, 6]
    assert host.edit_distance_batch(["flaw"], ["lawn"]).tolist() == [2]
    # bmx_cli on files: the printable pairs, line by line, and one line against many
    printable = lambda s: len(s) > 0 and min(s) >= 0x20 and max(s) < 0x7f
    keep = [i for i, (x, y) in enumerate(zip(a, b)) if printable(x) and printable(y)][:2000]
    assert len(keep) == 2000
    fa, fb, fq = tmp_path / "a.txt", tmp_path / "b.txt", tmp_path / "q.txt"
    fa.write_bytes(b"".join(a[i] + b"\n" for i in keep))
    fb.write_bytes(b"\n".join(b[i] for i in keep))  # a last line needs no newline
    fq.write_bytes(a[keep[0]] + b"\n")
    cli = os.path.join(os.path.dirname(host.LIB_PATH), "..", "bin", "bmx_cli")
    r = subprocess.run([cli, "--edit-distance-batch", str(fa), str(fb), "--iters", "2"], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert [int(t) for t in r.stdout.split()] == want[keep].tolist()
    assert b"kernel" in r.stderr and b"pairs" in r.stderr
    r = subprocess.run([cli, "--edit-distance-batch", str(fq), str(fb), "--limit", "4"], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    q_want = cases.clamp(np.array([_d(a[keep[0]], b[i]) for i in keep], np.uint32), 4)
    assert [int(t) for t in r.stdout.split()] == q_want.tolist()


def _d(x, y):
    import oracle

    return oracle.port().edit_distance(x, y)
