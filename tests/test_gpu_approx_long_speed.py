"""The two-word kernel of the long approximate search against the one-word kernel it extends.  On 256 MiB of printable
text made on the device, best of five bmx_last_approx_ms after a warm-up, for
    bmx_search_approx_device       m = 64,  k = 4   (the one-word kernel: the yardstick)
    bmx_search_approx_long_device  m = 65,  k = 4   (two words, one bit of the second in use)
    bmx_search_approx_long_device  m = 128, k = 4   (two words, both full)
each new time has to be at most 2 x 1.5 x the old one: 2 for the two words; 1.5 for the carry hand-over between them (four
of about seventeen 64-bit operations per word), the wider LDS row, the larger warm-up share (m + k - 1 = 131 against 67
bytes per lane piece) and the 4 % run-to-run spread the README states.

Measured on an MI355X: m = 64 0.282 ms, m = 65 0.550 ms (1.95 x), m = 128 0.572 ms (2.03 x); the same shapes
from tools/approx_long_rate.py (profiles/r15_approx_long_rate.jsonl, best of 3): 0.268 / 0.525 / 0.551 ms."""
import pytest

pytestmark = pytest.mark.gpu

BAR = 2 * 1.5


def test_two_words_cost_at_most_three_times_one(ctx):
    import torch

    n, k = 1 << 28, 4
    d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
    ctx.gen_text(d_text, 0, 0xA7710EED, 0)
    source = d_text[123456789 % n:123456789 % n + 128].cpu().numpy().tobytes()
    out = torch.empty(1 << 16, dtype=torch.int64, device="cuda")
    dist = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    best = {}
    for m in (64, 65, 128):
        pat = source[:m]
        assert (m > 64) == (len(pat) > ctx_max_short())
        ends, dists, total = ctx.search_approx_device(d_text, pat, k, out=out, dist_out=dist)  # warm-up; m > 64: the long entry
        assert total >= 1 and 123456789 % n + m - 1 in ends.cpu().numpy().tolist()
        times = []
        for _ in range(5):
            ctx.search_approx_device(d_text, pat, k, out=out, dist_out=dist)
            times.append(ctx.last_approx_ms())
        best[m] = min(times)
    print(f"256 MiB, k = {k}: m = 64 (one word) {best[64]:.3f} ms, m = 65 {best[65]:.3f} ms ({best[65] / best[64]:.2f} x), "
          f"m = 128 {best[128]:.3f} ms ({best[128] / best[64]:.2f} x); bar {BAR:.1f} x")
    del d_text
    torch.cuda.empty_cache()
    assert best[65] <= BAR * best[64], best
    assert best[128] <= BAR * best[64], best


def ctx_max_short() -> int:
    from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

    return host.MAX_APPROX_PATTERN
