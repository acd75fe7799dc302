"""What the pair warm-up of the regex search with unbounded repetition costs beside the star-free kernel: on 1 GiB of
printable-95 text with a planted corpus, (ERROR|FATAL|PANIC): [0-9]+ through bmx_search_regex_star_device beside
(ERROR|FATAL|PANIC): [0-9]{1,8} through the unchanged bmx_search_regex_device, in the same process, the same hits checked
(HIP events around the kernels, best of 3 after a warm-up call).  The call has to end untainted, so the time is the one
launch.  Measured on an MI355X (tools/regex_star_rate.py, profiles/r19_regex_star_rate.jsonl): 0.4558 ms
against 0.4308 ms, ratio 1.058.  The bound is that ratio times 1.25: the 4 % box-to-box spread the README reports plus
run-to-run noise on a kernel of less than a millisecond."""
import pytest

from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

pytestmark = pytest.mark.gpu

STAR = "(ERROR|FATAL|PANIC): [0-9]+"
FREE = "(ERROR|FATAL|PANIC): [0-9]{1,8}"
PLANTS = [b"ERROR: 7", b"FATAL: 12345678", b"PANIC: 42", b"ERROR: 0001", b"FATAL: 9"]
MEASURED_RATIO = 1.058
MARGIN = 1.25


def test_pair_warm_up_costs_little_beside_the_star_free_kernel(exp_ctx):
    import torch

    n = 1 << 30
    d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
    exp_ctx.gen_text(d_text, 0, 0x57A25EED, 0)
    planted = []
    for i, p in enumerate(PLANTS):
        at = 1000 + i * (n // 7)
        d_text[at:at + len(p) + 1] = torch.frombuffer(bytearray(p + b" "), dtype=torch.uint8).cuda()
        planted.append(at + len(p) - 1)
    free, star = host.compile_regex(FREE), host.compile_regex_star(STAR)
    out_f = torch.empty(1 << 16, dtype=torch.int64, device="cuda")
    out_s = torch.empty(1 << 16, dtype=torch.int64, device="cuda")
    exp_ctx.search_regex_device(d_text, free, out=out_f)  # warm-up
    exp_ctx.search_regex_star_device(d_text, star, out=out_s)
    t_free, t_star = [], []
    for _ in range(3):
        ends_f, total_f = exp_ctx.search_regex_device(d_text, free, out=out_f)
        t_free.append(exp_ctx.last_regex_ms())
        ends_s, total_s = exp_ctx.search_regex_star_device(d_text, star, out=out_s)
        t_star.append(exp_ctx.last_regex_star_ms())
        last = exp_ctx.regex_star_last()
        assert last["tainted"] == 0 and last["slow"] == 0, last
    assert total_f == total_s >= len(planted) and torch.equal(ends_f, ends_s)
    assert set(planted) <= set(ends_s.cpu().tolist())
    f, s = min(t_free), min(t_star)
    print(f"star kernel {s:.4f} ms, star-free kernel {f:.4f} ms, ratio {s / f:.3f}")
    del d_text
    torch.cuda.empty_cache()
    assert s < MEASURED_RATIO * MARGIN * f, (s, f)
