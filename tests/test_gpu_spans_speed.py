"""The spans pass against what a caller had to do without it: gather the 2k + 1 candidate windows of every end (lengths
m - k .. m + k) into an Arrow column, run bmx_edit_distance_batch_device one against many over them and take an argmin per
end.  On at least 2^20 ends from one search of 256 MiB of ACGT text (m = 16, k = 3, the pattern planted every 1 KiB), the
spans kernel's time (bmx_last_spans_ms, flags == 0, best of 3 after a warm-up) has to be below the batch kernel's
(bmx_last_ed_batch_ms, the same; the gather is not charged) by more than the 4 % box-to-box spread the README states for one
kernel, and both must give the same starts.  tools/spans_rate.py measures the pass at 4 GiB.

Measured on an MI355X: 1,839,732 ends, spans pass 0.036 ms, batch kernel 0.176 ms, ratio 0.206."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SPREAD = 0.04


def test_spans_pass_beats_batch_edit_distance_over_candidate_windows(ctx):
    import torch

    n, m, k = 1 << 28, 16, 3
    d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
    ctx.gen_text(d_text, 0, 0x5BA45EED, 1)
    pat = d_text[987654321 % n:987654321 % n + m].cpu().numpy().tobytes()
    ctx.plant(d_text, 0, pat, np.arange(512, n - 64, 1024, dtype=np.uint64))
    out = torch.empty(1 << 22, dtype=torch.int64, device="cuda")
    dist = torch.empty(1 << 22, dtype=torch.uint8, device="cuda")
    ends, dists, total = ctx.search_approx_device(d_text, pat, k, out=out, dist_out=dist)
    assert total == ends.numel() and total >= 1 << 20, total
    sel = ends >= m + k  # (windows of every candidate length exist)
    ends, dists = ends[sel].contiguous(), dists[sel].contiguous()
    count = ends.numel()
    assert count >= 1 << 20

    ctx.approx_spans_device(d_text, pat, k, ends, dists)  # warm-up
    t_spans = []
    for _ in range(3):
        starts, _, _, got = ctx.approx_spans_device(d_text, pat, k, ends, dists)
        t_spans.append(ctx.last_spans_ms())
    assert got == count

    # the caller's alternative: one string per (length, end), lengths ascending
    lengths = list(range(m - k, m + k + 1))
    blob = torch.cat([d_text[(ends - (L - 1)).unsqueeze(1) + torch.arange(L, device="cuda")].reshape(-1) for L in lengths])
    off = torch.zeros(len(lengths) * count + 1, dtype=torch.int64, device="cuda")
    off[1:] = torch.cumsum(torch.tensor(lengths, device="cuda").repeat_interleave(count), 0)
    d_a = torch.from_numpy(np.frombuffer(pat, np.uint8).copy()).cuda()
    d_a_off = torch.tensor([0, m], dtype=torch.int64, device="cuda")
    ed = torch.empty(len(lengths) * count, dtype=torch.int32, device="cuda")
    ctx.edit_distance_batch_device(d_a, d_a_off, blob, off, len(lengths) * count, a_count=1, out=ed)  # warm-up
    t_batch = []
    for _ in range(3):
        ctx.edit_distance_batch_device(d_a, d_a_off, blob, off, len(lengths) * count, a_count=1, out=ed)
        t_batch.append(ctx.last_ed_batch_ms())
    assert ctx.last_ed_batch_fallbacks() == 0
    key = ed.reshape(len(lengths), count).to(torch.int64) * 256 + torch.tensor(lengths, device="cuda").unsqueeze(1)
    best = key.min(dim=0).values  # the smallest distance, then the shortest window
    assert torch.equal(best // 256, dists.to(torch.int64))
    assert torch.equal(ends - (best % 256) + 1, starts)

    s, b = min(t_spans), min(t_batch)
    print(f"{count} ends: spans pass {s:.3f} ms, batch edit distance over {len(lengths)} windows per end {b:.3f} ms, "
          f"ratio {s / b:.3f}")
    del d_text, blob, off, ed
    torch.cuda.empty_cache()
    assert s < (1.0 - SPREAD) * b, (s, b)
