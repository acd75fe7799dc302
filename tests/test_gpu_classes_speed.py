"""The class-pattern search against what already answers the same question for literal patterns of up to 64 bytes: the
approximate search at k = 0.  On 1 GiB of printable-95 text and a 16-byte literal pattern copied from the text, the class
kernel's time (HIP events around the kernel, best of 3 after a warm-up) has to be below the approximate kernel's, measured
in the same run, by more than the 4 % box-to-box spread the README states for one kernel: a Shift-And kernel that cannot
beat Myers' recurrence at k = 0 has no reason to exist beside it.  tools/classes_rate.py measures both at 4 GiB for every
shape."""
import numpy as np
import pytest

import classes_oracle as co

pytestmark = pytest.mark.gpu

SPREAD = 0.04


def test_class_kernel_beats_the_approximate_kernel_at_k0(ctx):
    import torch

    n, m = 1 << 30, 16
    d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
    ctx.gen_text(d_text, 0, 0xC1A55E5, 0)
    pat = d_text[123456789:123456789 + m].cpu().numpy().tobytes()
    cls = co.pack(co.singletons(pat))
    out_c = torch.empty(1 << 16, dtype=torch.int64, device="cuda")
    out_a = torch.empty(1 << 16, dtype=torch.int64, device="cuda")
    dist = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    ctx.search_classes_device(d_text, cls, out=out_c)  # warm-up
    ctx.search_approx_device(d_text, pat, 0, out=out_a, dist_out=dist)
    t_classes, t_approx = [], []
    for _ in range(3):
        starts, total_c = ctx.search_classes_device(d_text, cls, out=out_c)
        t_classes.append(ctx.last_classes_ms())
        ends, _, total_a = ctx.search_approx_device(d_text, pat, 0, out=out_a, dist_out=dist)
        t_approx.append(ctx.last_approx_ms())
    assert total_c == total_a >= 1
    assert torch.equal(starts + (m - 1), ends) and 123456789 in starts.cpu().tolist()
    c, a = min(t_classes), min(t_approx)
    print(f"class kernel {c:.3f} ms, approximate kernel at k = 0 {a:.3f} ms, ratio {c / a:.3f}")
    del d_text
    torch.cuda.empty_cache()
    assert c < (1.0 - SPREAD) * a, (c, a)
