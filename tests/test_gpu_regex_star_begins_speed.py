"""What the pair warm-up costs the downward walk, and what the begins search for expressions with a cycle costs beside the
route a caller had without it: on 1 GiB of printable-95 text with five plants, (ERROR|FATAL|PANIC): [0-9]+ through
bmx_search_regex_star_begins_device (bmx_last_regex_star_begins_ms, untainted) beside
 (a) torch.flip of the text followed by the unchanged bmx_search_regex_star_device with the reversed automaton (HIP events
     around both), and
 (b) the star-free begins kernel on (ERROR|FATAL|PANIC): [0-9]{1,8} (bmx_last_regex_begins_ms),
in one process, best of 3 after a warm-up call, never against a stored time.  `measure` is also tools/regex_star_begins_rate.py's.
RECORDED holds the ratios of the run in profiles/r21_regex_star_begins_rate.jsonl; the test allows 1.25 times each, the margin
the project gives sub-millisecond kernels, and (a) below 1 in any case."""
import pytest

from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

pytestmark = pytest.mark.gpu

EXPR = "(ERROR|FATAL|PANIC): [0-9]+"
BOUNDED = "(ERROR|FATAL|PANIC): [0-9]{1,8}"
PLANTS = [b"ERROR: 7", b"FATAL: 12345678", b"PANIC: 42", b"ERROR: 0001", b"FATAL: 9"]
RECORDED = {"star_begins_over_route": 0.338, "star_begins_over_begins": 0.906}  # 0.7 ms beside 2.0732 ms and 0.7727 ms


def measure(ctx, n, emit=print):
    """A dict of times in ms and ratios, and whether the three lists agree."""
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
    for i, p in enumerate(PLANTS):
        at = 1000 + i * (n // 7)
        d_text[at:at + len(p) + 1] = torch.frombuffer(bytearray(p + b" "), dtype=torch.uint8).cuda()
    star = host.compile_regex_star(EXPR)
    rev = host.reverse_regex(star)
    bounded = host.compile_regex(BOUNDED)
    outs = [torch.empty(1 << 16, dtype=torch.int64, device="cuda") for _ in range(3)]

    def best_of(call, ms):
        call()
        times = []
        for _ in range(3):
            res = call()
            times.append(ms())
        return res, min(times)

    (s_star, total_star), t_star = best_of(lambda: ctx.search_regex_star_begins_device(d_text, star, out=outs[0]),
                                            ctx.last_regex_star_begins_ms)
    (s_b, total_b), t_begins = best_of(lambda: ctx.search_regex_begins_device(d_text, bounded, out=outs[1]), ctx.last_regex_begins_ms)

    def route():  # what a caller needs on the parent commit: unchanged code only
        return ctx.search_regex_star_device(torch.flip(d_text, [0]), rev, out=outs[2])

    (ends_r, total_r), t_route = timed(route)
    mapped = torch.flip((n - 1) - ends_r, [0])
    same = total_star == total_r == total_b and torch.equal(mapped, s_star) and torch.equal(s_b, s_star)
    _, t_flip = timed(lambda: torch.flip(d_text, [0]))
    res = {"n": n, "expr": EXPR, "hits": int(total_star), "star_begins_ms": round(t_star, 4), "begins_bounded_ms": round(t_begins, 4),
           "route_ms": round(t_route, 4), "flip_ms": round(t_flip, 4), "star_begins_over_route": round(t_star / t_route, 3),
           "star_begins_over_begins": round(t_star / t_begins, 3)}
    emit(res)
    del d_text
    torch.cuda.empty_cache()
    return res, same


def test_pair_warm_up_of_the_downward_walk(exp_ctx):
    res, same = measure(exp_ctx, 1 << 30, emit=lambda r: print("\nSTAR_BEGINS", r))
    last = exp_ctx.regex_star_begins_last()
    assert same, res
    assert res["star_begins_over_route"] < min(1.0, 1.25 * RECORDED["star_begins_over_route"]), res
    assert res["star_begins_over_begins"] < 1.25 * RECORDED["star_begins_over_begins"], res
    assert last["tainted"] == 0 and last["slow"] == 0, last
