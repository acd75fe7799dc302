"""GPU suite: the suffix array beyond the benchmark's shapes (bmx_suffix_array[_device], csrc/bmx_sa.hip).

tests/test_suffix_array.py stops at 2 MiB, where every helper kernel's grid-stride loop (at most 65,536 x 256 threads) goes
round once, and runs the host loop's default branches only.  Here: the fallback branches of the host loop (the `sa_flags`
switch of libbmx_exp.so), texts longer than one grid, the workspace and the pinned counters kept in a context across sizes,
and the device entry point on an unaligned view.  References: the prefix-doubling oracle (port.suffix_array) where it is
affordable, the order checks of tests/sa_checks.py (numpy; tested on the CPU in tests/test_suffix_array.py) beyond that, and
n-1 .. 0 for a text of one letter.  Nothing is compared with another run of the library."""
import numpy as np
import pytest

import sa_checks
from conftest import golden_file_bytes

pytestmark = pytest.mark.gpu

GRID = 65_536 * 256  # threads of the helper kernels' largest grid: texts beyond it take a second turn of every loop


def _lds_window_texts():
    """The texts of test_gpu_groups_around_the_lds_window (same seed, same order), and the reference's corpus."""
    rng = np.random.default_rng(77)
    out = []
    for n, period in ((150_000, 50), (150_000, 37), (150_000, 29), (150_000, 18), (150_000, 17), (8192 * 9, 23), (8192 * 9, 9),
                      (3072 * 20, 11), (200_003, 41), (65_536, 8), (100_000, 1), (100_000, 2)):
        para = (rng.integers(0, 26, period) + 97).astype(np.uint8)
        out.append((f"period {period} x {n}", np.tile(para, n // period + 1)[:n].copy()))
    out.append(("random", (rng.integers(0, 4, 300_000) + 97).astype(np.uint8)))
    out.append(("input5L", np.frombuffer(golden_file_bytes("input5L.txt.gz"), np.uint8).copy()))
    return out


def test_host_loop_branches_by_sa_flags(exp_ctx, port):
    """sa_flags 0: LDS rounds queued back to back (the default); 1: library sort only; 2: LDS rounds with a host wait per
    round; 3: both switches (library only).  Every text of the LDS-window test and the 500,007-byte corpus, each against
    the oracle; flag 1 runs no LDS round, flags 0 and 2 at least one on the random text, and the number of doubling rounds
    is the same under all four (a round does the same work whichever way it runs)."""
    texts = _lds_window_texts()
    want = [port.suffix_array(x) for _, x in texts]
    rounds = {}
    try:
        for flags in (0, 1, 2, 3):
            exp_ctx.set_knob("sa_flags", flags)
            for (name, x), w in zip(texts, want):
                sa = exp_ctx.suffix_array(x)
                r, l = exp_ctx.last_suffix_array_rounds(), exp_ctx.last_suffix_array_lds_rounds()
                assert np.array_equal(sa, w), (flags, name, r, l)
                rounds[(flags, name)] = (r, l)
                assert 0 <= l <= r, (flags, name, r, l)
                if flags & 1:
                    assert l == 0, (flags, name, r, l)
                elif name == "random":
                    assert l >= 1, (flags, name, r, l)
    finally:
        exp_ctx.set_knob("sa_flags", 0)
    for name, _ in texts:
        assert len({rounds[(f, name)][0] for f in (0, 1, 2, 3)}) == 1, (name, [rounds[(f, name)] for f in (0, 1, 2, 3)])


@pytest.mark.parametrize("n", [GRID + 4_097, (1 << 25) - 1])
def test_one_letter_longer_than_one_grid(ctx, n):
    """All 'a': suffix i is a prefix of suffix i - 1, so the answer is n-1 .. 0.  Groups stay far above the LDS window for
    most rounds: those go through the library sort with 2 x 25-bit keys, and every helper kernel's loop goes round twice."""
    import torch

    d = torch.full((n,), 97, dtype=torch.uint8, device=f"cuda:{ctx.device}")
    sa = ctx.suffix_array_device(d)
    torch.cuda.synchronize()
    assert ctx.last_suffix_array_rounds() > ctx.last_suffix_array_lds_rounds()
    want = torch.arange(n - 1, -1, -1, dtype=torch.int32, device=d.device)
    assert bool(torch.equal(sa, want)), int((sa != want).sum())


@pytest.mark.parametrize("period", [61, 8])
def test_periodic_longer_than_one_grid(ctx, period):
    """n = 2^24 + 4,097, a paragraph of 61 / 8 lowercase letters repeated: groups of n / period entries stay far above the LDS
    window until the last rounds, so library rounds and the crossing into LDS rounds both run at this size.  Reference: a
    permutation whose adjacent suffixes ascend by the periodic rule of tests/sa_checks.py."""
    n = GRID + 4_097
    rng = np.random.default_rng(period)
    para = (rng.integers(0, 26, period) + 97).astype(np.uint8)
    x = np.tile(para, n // period + 1)[:n].copy()
    sa = ctx.suffix_array(x)
    r, l = ctx.last_suffix_array_rounds(), ctx.last_suffix_array_lds_rounds()
    assert r - l >= 1, (r, l)
    assert sa_checks.is_permutation(sa, n)
    assert sa_checks.periodic_is_sorted(x, period, sa)


@pytest.mark.parametrize("n,letters", [(GRID + 4_097, 26), (GRID + 4_097, 2), ((1 << 25) - 1, 26), ((1 << 25) - 1, 2), (GRID, 26),
                                       (GRID + 1, 26)])
def test_random_longer_than_one_grid(ctx, n, letters):
    """Random lowercase text over 26 and over 2 letters, and the sizes at which the helper kernels' grids are exactly full
    and one entry over.  Reference: a permutation, adjacent suffixes strictly ascending (tests/sa_checks.py)."""
    rng = np.random.default_rng(n % 1000 + letters)
    x = (rng.integers(0, letters, n) + 97).astype(np.uint8)
    sa = ctx.suffix_array(x)
    assert ctx.last_suffix_array_lds_rounds() >= 1
    assert sa_checks.is_permutation(sa, n)
    assert sa_checks.is_sorted(x, sa)


def test_workspace_and_pinned_counters_across_sizes(built, port):
    """One context, four sizes in a row: the workspace grows once and is then reused for smaller texts (other offsets of the
    same arrays in it), the pinned block of the queued rounds stays.  Each against the oracle."""
    import torch
    from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

    assert torch.cuda.is_available()
    rng = np.random.default_rng(404)
    c = host.Context(0)
    try:
        para = (rng.integers(0, 26, 7) + 97).astype(np.uint8)
        for name, x in (("2^22 random", (rng.integers(0, 26, 1 << 22) + 97).astype(np.uint8)),
                        ("1,000 periodic", np.tile(para, 143)[:1000].copy()),
                        ("2^22 random, other contents", (rng.integers(0, 26, 1 << 22) + 97).astype(np.uint8)),
                        ("70,000 over 2 letters", (rng.integers(0, 2, 70_000) + 97).astype(np.uint8))):
            assert np.array_equal(c.suffix_array(x), port.suffix_array(x)), name
    finally:
        c.close()


def test_device_entry_on_an_odd_offset_view(ctx, port):
    """bmx_suffix_array_device on a view that starts 3 bytes into a larger tensor (no alignment of d_text), n = 300,001."""
    import torch

    rng = np.random.default_rng(303)
    n = 300_001
    big = (rng.integers(0, 4, n + 64) + 97).astype(np.uint8)
    d = torch.from_numpy(big).to(f"cuda:{ctx.device}")
    view = d[3:3 + n]
    assert view.data_ptr() % 2 == 1
    sa = ctx.suffix_array_device(view)
    torch.cuda.synchronize()
    assert np.array_equal(sa.cpu().numpy(), port.suffix_array(big[3:3 + n]))
