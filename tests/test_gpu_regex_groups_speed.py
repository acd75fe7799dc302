"""The capture groups pass against the first step of the only route there was, measured in the same run, best of 3 after a
warm-up; no absolute times.

2^20 spans of ``([0-9]{4})-([0-9]{2})-([0-9]{2})`` planted in 256 MiB of bmx_gen_text_device text, their (starts, ends) on
the device as the search and the starts pass leave them.  regex_groups_device over the list -- the allocation of its output
and the wait for it included, by the host's clock around a call that returns when its work is done -- against
``starts.cpu()`` plus ``ends.cpu()``: the download that any host route (Python's ``re`` over the spans) must begin with, the
yardstick of tests/test_gpu_subst_speed.py.  The host's own matching and the upload of its result are not charged.

The groups pass must take less time than the downloads.

Measured on the MI355X (one run): the pass 0.173 ms (kernel 0.067 ms) against 0.987 ms for the two
downloads, ratio 0.175."""
import time

import numpy as np
import pytest

from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

pytestmark = pytest.mark.gpu

N = 1 << 28
COUNT = 1 << 20
EXPR = "([0-9]{4})-([0-9]{2})-([0-9]{2})"
PLANT = b"2026-10-21"


def test_groups_pass_is_not_slower_than_downloading_the_spans(ctx):
    import torch

    d_text = torch.empty(N, dtype=torch.uint8, device="cuda")
    ctx.gen_text(d_text, 0, 0x3434, 0)
    rng = np.random.default_rng(0x3434)
    at = np.sort(rng.choice(N // 16 - 1, COUNT, replace=False).astype(np.uint64)) * np.uint64(16)
    ctx.plant(d_text, 0, PLANT, at)
    starts = torch.from_numpy(at.view(np.int64)).cuda()
    ends = starts + (len(PLANT) - 1)
    pair = host.compile_regex_groups(EXPR)
    ctx.regex_groups_device(d_text, pair, starts, ends), starts.cpu(), ends.cpu()  # warm-up
    torch.cuda.synchronize()
    t_new, t_old = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        groups = ctx.regex_groups_device(d_text, pair, starts, ends)
        t1 = time.perf_counter()
        hs, he = starts.cpu(), ends.cpu()
        t2 = time.perf_counter()
        t_new.append((t1 - t0) * 1e3)
        t_old.append((t2 - t1) * 1e3)
    want = starts[:, None] + torch.tensor([[0, 10], [0, 4], [5, 7], [8, 10]], device="cuda").reshape(1, 8)
    assert tuple(groups.shape) == (COUNT, 4, 2) and torch.equal(groups.reshape(COUNT, 8), want)
    assert hs.numel() == he.numel() == COUNT
    a, b = min(t_new), min(t_old)
    print(f"GROUPS pass over {COUNT} spans {a:.3f} ms (kernel {ctx.last_regex_groups_ms():.3f} ms), starts.cpu() + ends.cpu() {b:.3f} ms, "
          f"ratio {a / b:.3f}")
    assert a < b, (a, b)
    del d_text
    torch.cuda.empty_cache()
