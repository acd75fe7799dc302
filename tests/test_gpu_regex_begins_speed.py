"""What the begins search costs beside the route a caller had without it: on 1 GiB of printable-95 text with the five
plants of test_gpu_regex_star_speed.py, (ERROR|FATAL|PANIC): [0-9]{2,4} through bmx_search_regex_begins_device
(bmx_last_regex_begins_ms) beside torch.flip of the text followed by the unchanged bmx_search_regex_device with the reversed
automaton (HIP events around both), in one process, best of 3 after a warm-up call, the two lists equal after mapping.
The route holds the same recurrence over the same bytes plus one more read and one more write of the text, so the
condition is ratio < 1.0 with no margin.  Printed beside it, not asserted: the begins kernel beside the forward kernel on
the same text and expression, the ends pass on 2^20 starts, findall_device(posix=True) beside findall_device(merge=True).
Measured on an MI355X (tools/regex_begins_rate.py, profiles/r20_regex_begins_rate.jsonl): begins
0.655 ms, route 1.99 ms (flip alone 1.35 ms), ratio 0.33; forward kernel 0.407 ms on the expression and 0.622 ms on its
reversed automaton; ends pass on 2^20 starts 0.052 ms; findall posix 0.93 ms, merge 0.66 ms."""
import pytest

from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

pytestmark = pytest.mark.gpu

EXPR = "(ERROR|FATAL|PANIC): [0-9]{2,4}"
PLANTS = [b"ERROR: 7", b"FATAL: 12345678", b"PANIC: 42", b"ERROR: 0001", b"FATAL: 9"]
DENSE = "(e|th).{0,2}[a-z]"  # a few million starts: the ends pass takes the lowest 2^20


def measure(ctx, n, emit=print):
    """The measurements of this file and of tools/regex_begins_rate.py: a dict of times in ms, and whether the begins
    search's list equals the mapped list of the flip-and-search route."""
    import torch

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(call, repeats=3):
        call()  # warm-up
        best = None
        for _ in range(repeats):
            ev[0].record()
            res = call()
            ev[1].record()
            torch.cuda.synchronize()
            t = ev[0].elapsed_time(ev[1])
            best = t if best is None else min(best, t)
        return res, best

    d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
    ctx.gen_text(d_text, 0, 0x57A25EED, 0)
    planted = []
    for i, p in enumerate(PLANTS):
        at = 1000 + i * (n // 7)
        d_text[at:at + len(p) + 1] = torch.frombuffer(bytearray(p + b" "), dtype=torch.uint8).cuda()
        planted.append(at)
    re_ = host.compile_regex(EXPR)
    rev = host.reverse_regex(re_)
    out_b = torch.empty(1 << 16, dtype=torch.int64, device="cuda")
    out_f = torch.empty(1 << 16, dtype=torch.int64, device="cuda")

    ctx.search_regex_begins_device(d_text, re_, out=out_b)  # warm-up
    t_begins = []
    for _ in range(3):
        begins, total_b = ctx.search_regex_begins_device(d_text, re_, out=out_b)
        t_begins.append(ctx.last_regex_begins_ms())
    ctx.search_regex_device(d_text, re_, out=out_f)
    t_forward = []
    for _ in range(3):
        ctx.search_regex_device(d_text, re_, out=out_f)
        t_forward.append(ctx.last_regex_ms())

    ctx.search_regex_device(d_text, rev, out=out_f)  # the forward kernel with the reversed automaton, on the text as it is
    t_forward_rev = []
    for _ in range(3):
        ctx.search_regex_device(d_text, rev, out=out_f)
        t_forward_rev.append(ctx.last_regex_ms())

    def route():  # what a caller needs on the parent commit: unchanged code only
        flipped = torch.flip(d_text, [0])
        return ctx.search_regex_device(flipped, rev, out=out_f)

    (ends_r, total_r), t_route = timed(route)
    mapped = torch.flip((n - 1) - ends_r, [0])
    same = total_b == total_r and torch.equal(mapped, begins) and set(planted[1:4]) <= set(begins.cpu().tolist())  # (one digit is no match)
    _, t_flip = timed(lambda: torch.flip(d_text, [0]))
    torch.cuda.empty_cache()

    dense = host.compile_regex(DENSE)
    starts, total_d = ctx.search_regex_begins_device(d_text, dense, capacity=1 << 20)
    t_dense_begins = ctx.last_regex_begins_ms()
    _, t_ends = timed(lambda: ctx.regex_ends_device(d_text, dense, starts, longest=True))
    _, t_ends_short = timed(lambda: ctx.regex_ends_device(d_text, dense, starts))
    (blob_p, off_p), t_posix = timed(lambda: ctx.findall_device(d_text, EXPR, posix=True))
    (blob_m, off_m), t_merge = timed(lambda: ctx.findall_device(d_text, EXPR, merge=True))
    res = {"n": n, "expr": EXPR, "hits": int(total_b), "begins_ms": round(min(t_begins), 4), "forward_ms": round(min(t_forward), 4),
           "begins_over_forward": round(min(t_begins) / min(t_forward), 3),
           "forward_reversed_automaton_ms": round(min(t_forward_rev), 4), "route_ms": round(t_route, 4), "flip_ms": round(t_flip, 4),
           "begins_over_route": round(min(t_begins) / t_route, 3), "dense_expr": DENSE, "dense_hits": int(total_d),
           "dense_begins_ms": round(t_dense_begins, 4), "ends_list": int(starts.numel()), "ends_longest_ms": round(t_ends, 4),
           "ends_shortest_ms": round(t_ends_short, 4), "findall_posix_ms": round(t_posix, 4), "findall_merge_ms": round(t_merge, 4),
           "findall_matches": [int(off_p.numel() - 1), int(off_m.numel() - 1)]}
    emit(res)
    del d_text
    torch.cuda.empty_cache()
    return res, same


def test_begins_search_beats_flipping_the_text(ctx):
    res, same = measure(ctx, 1 << 30, emit=lambda r: print("\nBEGINS", r))
    assert same and res["begins_ms"] < res["route_ms"], res
