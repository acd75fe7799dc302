"""The gapped pattern search against what answers the same question without it: one class-search pass per fixed-length
variant of the pattern, merged by the caller.  On 1 GiB of printable-95 text and the PROSITE zinc-finger signature
C-x(2,4)-C-x(3)-[LIVMFYWC]-x(8)-H-x(3,5)-H (25 positions, 4 of them optional, 9 variants of 21..25 positions) with a few
planted copies, ONE pass of the gaps kernel (HIP events around the kernel, best of 3 after a warm-up) has to take less
than the SUM of the nine class-kernel passes, measured in the same run, by more than the 4 % box-to-box spread the README
states for one kernel; and the merged variant lists have to equal the gaps list.  tools/gaps_rate.py measures the kernel
at 4 GiB for more shapes."""
import numpy as np
import pytest

import classes_oracle as co
import gaps_oracle as go
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

pytestmark = pytest.mark.gpu

SPREAD = 0.04
ZINC = "C-x(2,4)-C-x(3)-[LIVMFYWC]-x(8)-H-x(3,5)-H"


def test_one_gaps_pass_beats_the_nine_class_passes(ctx):
    import torch

    n = 1 << 30
    classes, optional = host.compile_gaps(ZINC, host.GAPS_PROSITE)
    member = co.unpack(classes)
    variants = [co.pack(v) for v in go.variants(member, optional)]
    assert len(variants) == 9
    d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
    ctx.gen_text(d_text, 0, 0x6A955EED, 0)
    rng = np.random.default_rng(25)
    opts = [i for i in range(len(member)) if (optional >> i) & 1]
    planted = []
    for keep in range(1 << len(opts)):  # every choice of the optional positions, planted once
        copy = np.zeros(32, np.uint8)
        length = go.plant(rng, copy, member, optional, 0, keep={p for b, p in enumerate(opts) if (keep >> b) & 1})
        at = 1000 + keep * (n // 17)
        d_text[at:at + length] = torch.from_numpy(copy[:length]).cuda()
        planted.append(at + length - 1)
    out_g = torch.empty(1 << 16, dtype=torch.int64, device="cuda")
    out_c = torch.empty(1 << 16, dtype=torch.int64, device="cuda")
    ctx.search_gaps_device(d_text, (classes, optional), out=out_g)  # warm-up
    for v in variants:
        ctx.search_classes_device(d_text, v, out=out_c)
    t_gaps, t_classes = [], []
    for _ in range(3):
        ends, total = ctx.search_gaps_device(d_text, (classes, optional), out=out_g)
        t_gaps.append(ctx.last_gaps_ms())
        lists, ms = [], 0.0
        for v in variants:
            starts, t = ctx.search_classes_device(d_text, v, out=out_c)
            assert t == starts.numel()
            ms += ctx.last_classes_ms()
            lists.append(starts + (v.shape[0] - 1))
        t_classes.append(ms)
    merged = torch.unique(torch.cat(lists))
    assert total == merged.numel() >= len(planted) and torch.equal(ends, merged)
    assert set(planted) <= set(ends.cpu().tolist())
    g, c = min(t_gaps), min(t_classes)
    print(f"gaps kernel {g:.3f} ms, nine class-kernel passes {c:.3f} ms, ratio {g / c:.3f}")
    del d_text
    torch.cuda.empty_cache()
    assert g < (1.0 - SPREAD) * c, (g, c)
