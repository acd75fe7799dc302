"""The regular-expression search of up to 128 positions against what answers the same question without it: the 72-position
keyword expression split by hand into two alternations of at most 64 positions, one bmx_search_regex_device pass each,
merged by the caller.  On 1 GiB of printable-95 text with one copy of each of the expression's 30 fixed-length variants
planted, ONE pass of the long kernel (HIP events around the kernel, best of 3 after a warm-up) has to take less than the
SUM of the two 64-bit passes measured in the same run, and its list has to equal the merged lists.  The bound is derived,
not measured: the 128-bit step does at most twice the word work of the 64-bit step per byte, while the text, the frame and
the ordered output are paid once instead of twice; the merge is not charged to the old route, which is the margin.
tools/regex_long_rate.py measures the kernel at 4 GiB for more shapes."""
import numpy as np
import pytest

import regex_long_oracle as rl
import regex_oracle as ro
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

pytestmark = pytest.mark.gpu

HALVES = ["ERROR|FATAL|PANIC|WARNING|CRITICAL", "EXCEPTION|TIMEOUT|REFUSED|DENIED|ABORTED"]
TAIL = ": [0-9]{2,4}"
EXPR = "(" + "|".join(HALVES) + ")" + TAIL


def test_one_long_pass_beats_the_two_passes_of_the_split_expression(ctx):
    import torch

    n = 1 << 30
    long_ = host.compile_regex_long(EXPR)
    halves = [host.compile_regex("(" + h + ")" + TAIL) for h in HALVES]
    assert long_.m == 72 and [h.m for h in halves] == [36, 42]
    variants = ro.variants(rl.parse(EXPR))
    assert len(variants) == 30
    d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
    ctx.gen_text(d_text, 0, 0x331C5EED, 0)
    rng = np.random.default_rng(33)
    planted = []
    for i, v in enumerate(variants):  # every variant, planted once
        copy = np.zeros(32, np.uint8)
        length = ro.plant(rng, copy, v, 0)
        at = 1000 + i * (n // 31)
        d_text[at:at + length] = torch.from_numpy(copy[:length]).cuda()
        planted.append(at + length - 1)
    out_l = torch.empty(1 << 16, dtype=torch.int64, device="cuda")
    out_h = torch.empty(1 << 16, dtype=torch.int64, device="cuda")
    ctx.search_regex_long_device(d_text, long_, out=out_l)  # warm-up
    for h in halves:
        ctx.search_regex_device(d_text, h, out=out_h)
    t_long, t_split = [], []
    for _ in range(3):
        ends, total = ctx.search_regex_long_device(d_text, long_, out=out_l)
        t_long.append(ctx.last_regex_long_ms())
        lists, ms = [], 0.0
        for h in halves:
            part, t = ctx.search_regex_device(d_text, h, out=out_h)
            assert t == part.numel()
            ms += ctx.last_regex_ms()
            lists.append(part.clone())
        t_split.append(ms)
    merged = torch.unique(torch.cat(lists))
    assert total == merged.numel() >= len(planted) and torch.equal(ends, merged)
    assert set(planted) <= set(ends.cpu().tolist())
    one, two = min(t_long), min(t_split)
    print(f"long regex kernel {one:.3f} ms, the two 64-bit passes {two:.3f} ms, ratio {one / two:.3f}")
    del d_text
    torch.cuda.empty_cache()
    assert one < two, (one, two)
