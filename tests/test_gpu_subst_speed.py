"""The selection and the replace against the route a caller took before them, measured in the same run, best of 3 after a
warm-up; no absolute times.

Selection: 2^22 ascending 10-byte spans, about half of them overlapping their predecessor, through select_spans_device
into tensors the caller holds, against the FIRST STEP ALONE of the only route there was: ``starts.cpu()`` and
``ends.cpu()``.  The host loop over the 2^22 entries and the upload of its result are not charged.  Both sides by the host's
clock around calls that return when their work is done.
Replace: 1 GiB of bmx_gen_text_device text with ``ERROR: 123`` planted 2^16 times, every plant deleted (repl_len = 0),
against ``d_text[mask]`` with the mask built outside the timed region, the torch route for a deletion; each side between one
pair of events.

Each may take at most (1 + SPREAD) times the old route, SPREAD being the 4 % box-to-box spread the README states for one
kernel: not being slower is the condition.  The third test asserts nothing about time: it prints what DESIGN.md s29 records
(replace against ``d_text.clone()``, the floor of one read and one write, for replacements of 0, 10 and 40 bytes; the dense
case, 1 GiB of ACGT with every A replaced; a selection that takes every span against one that takes one; extract of 2^16
and of 2^22 spans).

Measured on the MI355X (three runs): the selection takes 0.614-0.678 ms (kernels 0.56 ms, 2,577,943 of 2^22 taken) against
4.217-5.681 ms for the two downloads, ratio 0.115-0.153.  The deletion takes 1.371-1.389 ms (kernels 1.32-1.34 ms) against
9.365-9.388 ms for ``d_text[mask]``, ratio 0.146-0.148.  Recorded, no condition: replace with repl_len 0 / 10 / 40 takes
1.43 / 1.36 / 1.46 ms against 0.388 ms for ``d_text.clone()``, ratio 3.7 / 3.5 / 3.8; the dense case (268,440,646 one-byte
spans in 1 GiB of ACGT) 13.5 ms; a selection that takes every one of 2^22 spans 0.59 ms, one that takes one span 0.31 ms;
extract of the 2^16 spans 0.135 ms, of 2^22 spans 0.83 ms."""
import time

import numpy as np
import pytest

from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

pytestmark = pytest.mark.gpu

SPREAD = 0.04
N = 1 << 30
PLANT = b"ERROR: 123"


@pytest.fixture(scope="module")
def big(ctx):
    """(text, ascending starts of the plants), once for the module."""
    import torch

    d_text = torch.empty(N, dtype=torch.uint8, device="cuda")
    ctx.gen_text(d_text, 0, 0x29B5, 0)
    rng = np.random.default_rng(0x29B5)
    at = np.sort(rng.choice(N // 16 - 1, 1 << 16, replace=False).astype(np.uint64)) * np.uint64(16)
    ctx.plant(d_text, 0, PLANT, at)
    yield d_text, torch.from_numpy(at.view(np.int64)).cuda()
    del d_text
    torch.cuda.empty_cache()


def half_overlapping(count, seed):
    import torch

    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    step = torch.where(torch.rand(count, generator=g, device="cuda") < 0.5, torch.randint(1, 10, (count,), generator=g, device="cuda"),
                       torch.randint(10, 30, (count,), generator=g, device="cuda"))
    ends = 100 + torch.cumsum(step, 0)
    return ends - 9, ends


def best_ms(fn, events):
    import torch

    times = []
    for _ in range(3):
        events[0].record()
        res = fn()
        events[1].record()
        torch.cuda.synchronize()
        times.append(events[0].elapsed_time(events[1]))
    return min(times), res


def test_selection_is_not_slower_than_downloading_the_lists(ctx):
    import torch

    count = 1 << 22
    starts, ends = half_overlapping(count, 29)
    out = tuple(torch.empty(count, dtype=torch.int64, device="cuda") for _ in range(2))
    ctx.select_spans_device(starts, ends, out=out), starts.cpu(), ends.cpu()  # warm-up
    torch.cuda.synchronize()
    t_new, t_old = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        s, e = ctx.select_spans_device(starts, ends, out=out)
        t1 = time.perf_counter()
        hs, he = starts.cpu(), ends.cpu()
        t2 = time.perf_counter()
        t_new.append((t1 - t0) * 1e3)
        t_old.append((t2 - t1) * 1e3)
    hs, he = hs.numpy(), he.numpy()
    last, taken = -1, []
    for j in range(1 << 16):  # the host loop on the head of the list: the same entries
        if hs[j] > last:
            taken.append(j)
            last = he[j]
    assert s[:len(taken)].cpu().numpy().tolist() == hs[taken].tolist() and (1 << 21) < s.numel() < count
    assert bool((s[1:] > e[:-1]).all())
    a, b = min(t_new), min(t_old)
    print(f"SUBST select of {count} spans {a:.3f} ms (kernels {ctx.last_subst_ms():.3f} ms, {s.numel()} taken), starts.cpu() + ends.cpu() "
          f"{b:.3f} ms, ratio {a / b:.3f}")
    assert a <= (1.0 + SPREAD) * b, (a, b)


def test_replace_is_not_slower_than_the_mask_route(ctx, big):
    import torch

    d_text, at = big
    mask = torch.ones(N, dtype=torch.bool, device="cuda")
    mask[(at[:, None] + torch.arange(len(PLANT), device="cuda")[None, :]).reshape(-1)] = False
    out = torch.empty(N, dtype=torch.uint8, device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ctx.replace_device(d_text, at, None, b"", len(PLANT), out=out), d_text[mask]  # warm-up
    a, (got, n_out) = best_ms(lambda: ctx.replace_device(d_text, at, None, b"", len(PLANT), out=out), ev)
    kernel = ctx.last_subst_ms()
    b, want = best_ms(lambda: d_text[mask], ev)
    assert n_out == N - len(PLANT) * at.numel() == want.numel() and torch.equal(got, want)
    print(f"SUBST replace of {at.numel()} spans in 1 GiB by nothing {a:.3f} ms (kernels {kernel:.3f} ms), d_text[mask] {b:.3f} ms, ratio {a / b:.3f}")
    assert a <= (1.0 + SPREAD) * b, (a, b)


def test_recorded_figures(ctx, big):
    """No condition on time: the figures of DESIGN.md s29."""
    import torch

    d_text, at = big
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = torch.empty(N + 40 * at.numel(), dtype=torch.uint8, device="cuda")
    d_text.clone()
    floor, _ = best_ms(lambda: d_text.clone(), ev)
    for rl in (0, 10, 40):
        ctx.replace_device(d_text, at, None, b"#" * rl, len(PLANT), out=out)
        t, _ = best_ms(lambda: ctx.replace_device(d_text, at, None, b"#" * rl, len(PLANT), out=out), ev)
        print(f"SUBST replace repl_len {rl}: {t:.3f} ms (kernels {ctx.last_subst_ms():.3f} ms), clone {floor:.3f} ms, ratio {t / floor:.3f}")
    for count in (1 << 16, 1 << 22):
        s = at if count == at.numel() else torch.arange(count, device="cuda") * 250
        ctx.extract_device(d_text, s, None, len(PLANT), out=out)
        t, (blob, off) = best_ms(lambda: ctx.extract_device(d_text, s, None, len(PLANT), out=out), ev)
        assert blob.numel() == count * len(PLANT) and (count != at.numel() or bytes(blob[:10].cpu().numpy()) == PLANT)
        print(f"SUBST extract of {count} spans: {t:.3f} ms (kernels {ctx.last_subst_ms():.3f} ms)")
    count = 1 << 22
    i = torch.arange(count, device="cuda")
    for name, (s, e) in (("every span taken", (20 * i, 20 * i + 9)), ("one span taken", (torch.zeros_like(i), 5 + i))):
        sel = tuple(torch.empty(count, dtype=torch.int64, device="cuda") for _ in range(2))
        ctx.select_spans_device(s, e, out=sel)
        t, (ts, _) = best_ms(lambda: ctx.select_spans_device(s, e, out=sel), ev)
        assert ts.numel() == (count if name.startswith("every") else 1)
        print(f"SUBST select, {name}: {t:.3f} ms (kernels {ctx.last_subst_ms():.3f} ms)")
    del out
    acgt = torch.empty(N, dtype=torch.uint8, device="cuda")
    ctx.gen_text(acgt, 0, 0x29B6, 1)
    a_at = torch.nonzero(acgt == ord("A")).reshape(-1)
    out = torch.empty(N, dtype=torch.uint8, device="cuda")
    ctx.replace_device(acgt, a_at, None, b"N", 1, out=out)
    t, (got, n_out) = best_ms(lambda: ctx.replace_device(acgt, a_at, None, b"N", 1, out=out), ev)
    assert n_out == N and torch.equal(got, torch.where(acgt == ord("A"), torch.full_like(acgt, ord("N")), acgt))
    print(f"SUBST dense: {a_at.numel()} one-byte spans of 1 GiB ACGT replaced in {t:.3f} ms (kernels {ctx.last_subst_ms():.3f} ms)")
