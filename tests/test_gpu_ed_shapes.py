"""GPU suite: the edit distance beyond the benchmark's shapes (bmx_edit_distance_device, `ed_band_run` in csrc/bmx_ed.hip).

tests/test_edit_distance.py stops at 65,536 x 65,536: 32 column bands of 2,048, 64 workgroups.  The default kernel
(csrc/bmx_ed_bits3_kernel.h) is a pipeline in which band b spins on band b - 1, launched as 2 x bands workgroups of
ed_bits3_lds(32, 2) = 142,000 bytes of LDS each: one workgroup per CU (160 KiB), 256 resident on the card's 256 CUs.  Here:
more workgroups than that, the workspace rules of the host side (kept up to 1 GiB, reused without clearing for the same shape,
cleared for another), every band schedule at shapes that favoured different band widths, and the argument limits.  The product
library builds the default schedule alone; the ones that lost run on a context of libbmx_exp.so.

References: the two-row oracle (port.edit_distance) and, for long related strings, its diagonal-band version
(port.edit_distance_within: exact whenever it answers at all; "more than t" fails the test).  Nothing is compared with the
library alone: where several schedules run, each must equal the oracle's answer."""
import ctypes as C

import numpy as np
import pytest

from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

pytestmark = pytest.mark.gpu

# The band schedules of g_ed_variants (csrc/bmx_ed.hip): every slot but 5, which has tiles only.  0 (= 13) and 13 are the
# product library's; the others exist in libbmx_exp.so alone.
BAND_SCHEDULES = [0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13]


def _dev(ctx, x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x)).to(f"cuda:{ctx.device}")


def _gpu(ctx, x, y):
    return ctx.edit_distance_device(_dev(ctx, x), _dev(ctx, y))


def _acgt(rng, n):
    return (rng.integers(0, 4, n) + 65).astype(np.uint8)


def _edited(rng, x, k, d, runs, run_len=(1, 6)):
    """x with k substitutions by a fifth letter at distinct positions, d deletions and `runs` inserted runs of a sixth letter.
    Returns (y, number of single-character edits made): the distance is at most that number."""
    y = x.copy()
    y[rng.choice(x.size, k, replace=False)] = ord("N")
    y = np.delete(y, rng.choice(y.size, d, replace=False))
    edits = k + d
    for at in sorted(rng.integers(0, y.size, runs).tolist(), reverse=True):
        ln = int(rng.integers(run_len[0], run_len[1]))
        y = np.concatenate([y[:at], np.full(ln, ord("Z"), dtype=np.uint8), y[at:]])
        edits += ln
    return y, edits


# la, the lb values, and the lb values that also get the related strings (an edited copy cut to lb at the start, middle, end of a).
# bands = ceil(la / 2048) = 147 / 513 / 2048, launched as 294 / 1,026 / 4,096 workgroups: all three exceed the 256 resident ones.
# lb shrinks with la so that the CPU oracle stays at 0.6 - 1.2 G cells per la (3.5 ns per cell).
FEW_ROWS = [(300_000, (1, 31, 500), (31, 500)), ((1 << 20) + 5, (1, 31, 200), (200,)), ((1 << 22) - 2047, (1, 31, 64), (64,))]


@pytest.mark.parametrize("la,lbs,related", FEW_ROWS)
def test_more_bands_than_resident_workgroups_few_rows(ctx, exp_ctx, port, la, lbs, related):
    """Unrelated strings over 4 letters and related ones, both argument orders, schedule 0, against the full oracle.  The
    largest la also on schedules 11 (one-wave bit-parallel bands) and 4 (value bands of 384 columns: 10,918 bands), which are
    libbmx_exp.so's."""
    rng = np.random.default_rng(la % 9973)
    a = _acgt(rng, la)
    da = _dev(ctx, a)
    cases = [("unrelated", lb, _acgt(rng, lb)) for lb in lbs]
    for lb in related:
        for where, at in (("start", 0), ("middle", la // 2 - 7), ("end", la - lb - lb // 8 - 3)):
            piece, _ = _edited(rng, a[at:at + lb + lb // 8 + 2], lb // 10, lb // 16, 1 if lb > 40 else 0)
            cases.append((where, lb, piece[:lb].copy()))
    for name, lb, b in cases:
        assert b.size == lb
        want = port.edit_distance(a, b)
        assert la - lb <= want <= la
        db = _dev(ctx, b)
        assert ctx.edit_distance_device(da, db) == want, (name, la, lb)
        assert ctx.edit_distance_device(db, da) == want, (name, lb, la)
        if la > 4_000_000 and lb == lbs[-1]:
            for v in (11, 4):
                exp_ctx.set_ed_variant(v)
                assert exp_ctx.edit_distance_device(da, db) == want, (v, name, la, lb)


def test_many_bands_many_rows_and_the_workspace_that_is_not_kept(built, port):
    """b = a with substitutions by a fifth letter, deletions and inserted runs of a sixth letter; reference: the thresholded
    oracle with t = 2 x (number of edits), which must answer (None = "more than t" fails).

    400,000 x ~400,000: 196 bands, 392 workgroups; 16 B x 197 x 400,001 = 1.26 GB of band workspace, above the 1 GiB that a
    context keeps: allocated and freed per call.  1,048,576 x ~1,048,576: 512 bands, 1,024 workgroups, 8.6 GB.  (A string of
    1,048,576 against one of 140,000 would need the band |la - lb| = 908,576 wide: 1.3 x 10^11 cells for either oracle, minutes
    of CPU; the related string of the same length keeps the band count and has more rows.)  In the same context a 3,000 x
    3,000 call against the full oracle follows (allocates the kept workspace), then the large shape again (not kept again)."""
    import torch

    assert torch.cuda.is_available()
    c = host.Context(0)
    try:
        for la, k, d, runs in ((400_000, 500, 300, 60), (1 << 20, 250, 150, 30)):
            rng = np.random.default_rng(la % 7919)
            a = _acgt(rng, la)
            b, edits = _edited(rng, a, k, d, runs)
            want = port.edit_distance_within(a, b, 2 * edits)
            assert want is not None and abs(la - b.size) <= want <= edits, (la, b.size, edits, want)
            da, db = _dev(c, a), _dev(c, b)
            assert c.edit_distance_device(da, db) == want, (la, b.size)
            x, y = _acgt(rng, 3000), _acgt(rng, 3000)
            assert _gpu(c, x, y) == port.edit_distance(x, y)
            assert c.edit_distance_device(db, da) == want, (b.size, la)
            assert c.edit_distance_device(da, db) == want, (la, b.size, "again")
    finally:
        c.close()


def test_workspace_reuse_sequence(built, port):
    """One context, a fixed sequence of shapes that all fit the workspace of the first call: same shape (reused without
    clearing: only this call's tag makes entries valid), other contents, other shapes (cleared), back again; then the same on
    schedule 4, whose band width lays the same storage out differently.  Each call against the full oracle.  Schedule 4 is
    libbmx_exp.so's, so the whole sequence runs on a context of that library; its schedule-0 part runs on the product
    library too, on the same strings."""
    import torch

    assert torch.cuda.is_available()
    shapes = [(4096, 4096), (4096, 4096), (2048, 8000), (8000, 2048), (4096, 4096), (100, 100), (6200, 5), (4096, 4096)]
    for library, schedules in ((None, (0,)), (host.exp_lib(), (0, 4))):
        rng = np.random.default_rng(808)
        c = host.Context(0, library=library)
        try:
            for v in schedules:
                c.set_ed_variant(v)
                for step, (la, lb) in enumerate(shapes):
                    x = _acgt(rng, la)
                    if la == lb:  # related: the answer is far from max(la, lb), stale entries would show
                        y = x.copy()
                        y[rng.integers(0, la, la // 9 + 1)] = ord("N")
                        y = np.resize(np.delete(y, rng.integers(0, la, la // 40 + 1)), lb)
                    else:
                        y = _acgt(rng, lb)
                    assert _gpu(c, x, y) == port.edit_distance(x, y), (library is not None, v, step, la, lb)
        finally:
            c.close()


PICK_SHAPES = [(8 * 1024, 128 * 1024), (20_000, 20_000), (300, 70_000)]


def test_every_band_schedule_equals_the_oracle_at_three_shapes(ctx, exp_ctx, port):
    """Three shapes at which the step model that once chose among the value bands preferred different widths (C = 3 at
    8k x 128k, C = 6 at 64k x 64k), 8k x 128k among them.  Schedule 0 is schedule 13 at every shape now, and
    the library does not report a pick: the test asserts that schedule 0 equals the oracle and that every explicit band
    schedule does too, in both argument orders."""
    rng = np.random.default_rng(1313)
    try:
        for lb, la in PICK_SHAPES:
            x = _acgt(rng, la)
            if la == lb:
                y, edits = _edited(rng, x, 200, 100, 20)
                want = port.edit_distance_within(x, y, 2 * edits)
                assert want is not None
            else:
                y = _acgt(rng, lb)
                want = port.edit_distance(x, y)
            dx, dy = _dev(ctx, x), _dev(ctx, y)
            for v in BAND_SCHEDULES:
                c = ctx if v in (0, 13) else exp_ctx
                c.set_ed_variant(v)
                assert c.edit_distance_device(dx, dy) == want, (v, la, y.size)
                assert c.edit_distance_device(dy, dx) == want, (v, y.size, la)
    finally:
        ctx.set_ed_variant(0)


def test_argument_limits(ctx):
    """A length of 2^31 is refused with BMX_ERR_ARG before anything is read or written (the pointer is a valid one-byte
    allocation, the distance word keeps its value); la = 0 returns lb without a kernel."""
    import torch

    L = ctx._L
    one = torch.zeros(1, dtype=torch.uint8, device=f"cuda:{ctx.device}")
    p = C.c_void_p(one.data_ptr())
    for la, lb in ((1 << 31, 1), (1, 1 << 31), (1 << 31, 1 << 31), (1 << 40, 1)):
        d = C.c_uint64(0xDEADBEEF)
        assert L.bmx_edit_distance_device(ctx._h, p, la, p, lb, C.byref(d), None) == host.ERR_ARG, (la, lb)
        assert d.value == 0xDEADBEEF
    torch.cuda.synchronize()
    assert int(one.cpu()[0]) == 0
    d = C.c_uint64(0)
    assert L.bmx_edit_distance_device(ctx._h, None, 0, p, (1 << 31) - 1, C.byref(d), None) == host.OK
    assert d.value == (1 << 31) - 1
    big = torch.zeros(3_000_000, dtype=torch.uint8, device=one.device)
    assert ctx.edit_distance_device(big[:100], big[:300]) == 200 and ctx.last_edit_distance_ms() > 0.0
    assert ctx.edit_distance_device(big[:0], big) == 3_000_000
    assert ctx.last_edit_distance_ms() == -1.0  # (no kernel ran: the time of the call before is gone)
    assert ctx.edit_distance_device(big, big[:0]) == 3_000_000
