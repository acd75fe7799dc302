"""The batched edit distance against what it replaces: for 2^20 pairs of 32 x 32 bytes in one pairwise call, the per-pair
time (HIP events around the batch kernel, best of 3 after a warm-up) has to be at least 20 times below the per-pair time
of the single-pair entry point looped by the caller over a 4,096-pair sample of the same data, measured in the same run.
The margin is loose on purpose: the loop pays a launch and a host wait per pair (tens of microseconds), the batch
kernel's arithmetic per pair is nanoseconds, and a batch call that cannot clear one order of magnitude has no reason to
exist.  tools/ed_batch_rate.py measures the same ratio for every shape."""
import time

import pytest

pytestmark = pytest.mark.gpu

MIN_SPEEDUP = 20


def test_batch_beats_the_callers_loop_at_32_bytes(ctx, port):
    import torch

    count, length, sample = 1 << 20, 32, 4096
    d_a = torch.empty(count * length, dtype=torch.uint8, device="cuda")
    d_b = torch.empty(count * length, dtype=torch.uint8, device="cuda")
    ctx.gen_text(d_a, 0, 0xEDBA7C00, 0)
    ctx.gen_text(d_b, 1 << 40, 0xEDBA7C00, 0)
    off = torch.arange(count + 1, dtype=torch.int64, device="cuda") * length
    out = torch.empty(count, dtype=torch.int32, device="cuda")
    ctx.edit_distance_batch_device(d_a, off, d_b, off, count, out=out)  # warm-up
    times = []
    for _ in range(3):
        ctx.edit_distance_batch_device(d_a, off, d_b, off, count, out=out)
        times.append(ctx.last_ed_batch_ms())
    assert ctx.last_ed_batch_fallbacks() == 0
    batch_s = min(times) * 1e-3 / count
    got = out[:sample].cpu().tolist()

    ctx.edit_distance_device(d_a[:length], d_b[:length])  # warm-up
    t0 = time.perf_counter()
    loop = [ctx.edit_distance_device(d_a[i * length:(i + 1) * length], d_b[i * length:(i + 1) * length]) for i in range(sample)]
    loop_s = (time.perf_counter() - t0) / sample

    h_a, h_b = d_a[:sample * length].cpu().numpy(), d_b[:sample * length].cpu().numpy()
    want = [port.edit_distance(h_a[i * length:(i + 1) * length], h_b[i * length:(i + 1) * length]) for i in range(sample)]
    assert got == want and loop == want
    print(f"batch {batch_s * 1e9:.3f} ns per pair, loop {loop_s * 1e6:.2f} us per pair, ratio {loop_s / batch_s:.0f}")
    assert loop_s >= MIN_SPEEDUP * batch_s, (batch_s, loop_s)
