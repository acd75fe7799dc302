"""What the anchored search costs beside the route a caller had without it: on 1 GiB of printable-95 text in which one
byte value has become the line break (lines of 95 bytes on average), ^(ERROR|FATAL|PANIC): [0-9]{2,4}$ planted at line
starts, in mid-line and in front of a byte that is no line break, through bmx_search_regex_anchored_device (HIP events
around the call) beside the unchanged route: bmx_search_regex_device on the expression without its anchors (its ends
have unique starts), bmx_regex_starts_device, bmx_rows_split_device and the torch comparisons of starts and ends against
the row offsets (events around all of it), in one process, best of 3 after a warm-up call, the two lists equal.  The route
runs the same recurrence over the same bytes and reads the text a second time for the split, so the condition is
ratio < 1.0 with no margin.  Printed beside it, not asserted: the anchored kernel beside the plain kernel on the unanchored
expression (the cost of the two extra gathers), \\b(ERROR|FATAL|PANIC)\\b, the begins side, both post-passes on 2^20 entries.
Measured on an MI355X (tools/regex_anchored_rate.py, profiles/r22_regex_anchored_rate.jsonl): anchored call
0.632 ms, route 1.03 ms, ratio 0.61; anchored kernel 0.593 ms beside 0.415 ms for the plain kernel on the unanchored
expression (0.588 ms with every class full: 1.42); \\b(ERROR|FATAL|PANIC)\\b 0.576 ms; anchored begins 0.632 ms (plain begins
0.638 ms); starts pass 0.058 ms and ends pass 0.063 ms on 2^20 entries."""
import pytest

from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

pytestmark = pytest.mark.gpu

PLAIN = "(ERROR|FATAL|PANIC): [0-9]{2,4}"
EXPR = "^" + PLAIN + "$"
WORDS = r"\b(ERROR|FATAL|PANIC)\b"
# at a line start and in front of a line break (a match); in mid-line; in front of a byte that is no line break
PLANTS = [b"\nERROR: 123\n", b"\nFATAL: 12\n", b" PANIC: 1234\n", b"\nERROR: 12 ", b"\nPANIC: 4321\n"]
DENSE = r"\<(e|th).{0,2}[a-z]"  # a few million matches: the post-passes take the lowest 2^20
BREAK_FROM = 0x7E  # the byte value of the generated text that becomes the line break


def measure(ctx, n, emit=print):
    """The measurements of this file and of tools/regex_anchored_rate.py: a dict of times in ms, and whether the anchored
    search's list equals the list of the route over unchanged code."""
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

    def kernel(call, last_ms, repeats=3):
        call()
        times = []
        for _ in range(repeats):
            res = call()
            times.append(last_ms())
        return res, min(times)

    d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
    ctx.gen_text(d_text, 0, 0x57A25EED, 0)
    d_text.masked_fill_(d_text == BREAK_FROM, 10)
    planted = []
    for i in range(40):
        p = PLANTS[i % len(PLANTS)]
        at = 1000 + i * (n // 41)
        d_text[at:at + len(p)] = torch.frombuffer(bytearray(p), dtype=torch.uint8).cuda()
        planted.append((at, p))
    plain = host.compile_regex(PLAIN)
    pair = host.compile_regex_anchored(EXPR)
    out_a = torch.empty(1 << 16, dtype=torch.int64, device="cuda")
    out_p = torch.empty(1 << 16, dtype=torch.int64, device="cuda")
    offsets = torch.empty(n // 64 + 2, dtype=torch.int64, device="cuda")

    (ends_a, total_a), t_anchored = timed(lambda: ctx.search_regex_anchored_device(d_text, pair, out=out_a))
    _, k_anchored = kernel(lambda: ctx.search_regex_anchored_device(d_text, pair, out=out_a), ctx.last_regex_anchored_ms)

    def route():  # what a caller needs on the parent commit: unchanged code only
        ends, _ = ctx.search_regex_device(d_text, plain, out=out_p)
        starts = ctx.regex_starts_device(d_text, plain, ends)
        off = ctx.rows_split_device(d_text, out=offsets).offsets.to(torch.int64)
        at_line_start = off[torch.searchsorted(off, starts).clamp(max=off.numel() - 1)] == starts
        after = ends + 2  # the row behind a match that a line break follows begins there
        at_line_end = (off[torch.searchsorted(off, after).clamp(max=off.numel() - 1)] == after) | (ends == n - 1)
        return ends[at_line_start & at_line_end]

    ends_r, t_route = timed(route)
    want = sorted(at + len(p) - 2 for at, p in planted if p[:1] == b"\n" and p[-1:] == b"\n")
    same = total_a == ends_r.numel() and torch.equal(ends_a, ends_r) and set(want) <= set(ends_a.cpu().tolist())
    _, k_plain = kernel(lambda: ctx.search_regex_device(d_text, plain, out=out_p), ctx.last_regex_ms)
    full = (plain, host.RegexAnchors.full())
    _, k_full = kernel(lambda: ctx.search_regex_anchored_device(d_text, full, out=out_a), ctx.last_regex_anchored_ms)
    words = host.compile_regex_anchored(WORDS)
    (_, total_w), k_words = kernel(lambda: ctx.search_regex_anchored_device(d_text, words, out=out_a), ctx.last_regex_anchored_ms)
    (begins, total_b), k_begins = kernel(lambda: ctx.search_regex_anchored_begins_device(d_text, pair, out=out_a),
                                         ctx.last_regex_anchored_begins_ms)
    _, k_begins_plain = kernel(lambda: ctx.search_regex_begins_device(d_text, plain, out=out_p), ctx.last_regex_begins_ms)
    same = same and total_b == total_a
    torch.cuda.empty_cache()

    dense = host.compile_regex_anchored(DENSE)
    d_ends, total_d = ctx.search_regex_anchored_device(d_text, dense, capacity=1 << 20)
    _, t_starts = timed(lambda: ctx.regex_anchored_starts_device(d_text, dense, d_ends, longest=True))
    d_begins, _ = ctx.search_regex_anchored_begins_device(d_text, dense, capacity=1 << 20)
    _, t_ends = timed(lambda: ctx.regex_anchored_ends_device(d_text, dense, d_begins, longest=True))
    res = {"n": n, "expr": EXPR, "hits": int(total_a), "anchored_ms": round(t_anchored, 4), "route_ms": round(t_route, 4),
           "anchored_over_route": round(t_anchored / t_route, 3), "anchored_kernel_ms": round(k_anchored, 4),
           "plain_kernel_ms": round(k_plain, 4), "anchored_full_classes_kernel_ms": round(k_full, 4),
           "full_over_plain": round(k_full / k_plain, 3), "words_expr": WORDS, "words_hits": int(total_w),
           "words_kernel_ms": round(k_words, 4), "begins_kernel_ms": round(k_begins, 4),
           "begins_plain_kernel_ms": round(k_begins_plain, 4), "dense_expr": DENSE, "dense_hits": int(total_d),
           "post_list": int(d_ends.numel()), "starts_longest_ms": round(t_starts, 4), "ends_longest_ms": round(t_ends, 4)}
    emit(res)
    del d_text
    torch.cuda.empty_cache()
    return res, same


def test_anchored_search_beats_the_route_over_unanchored_lists(ctx):
    res, same = measure(ctx, 1 << 30, emit=lambda r: print("\nANCHORED", r))
    assert same and res["anchored_ms"] / res["route_ms"] < 1.0, res
