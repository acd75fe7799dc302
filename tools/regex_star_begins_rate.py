"""Rate of the begins search for expressions with * + {a,} (bmx_search_regex_star_begins_device) on a synthetic text generated
in HBM (bmx_gen_text_device), printable-95 with the five plants of tests/test_gpu_regex_star_begins_speed.py -- the first
measurements are that file's `measure`, so the test and the profile cannot drift apart:

    star_begins_ms       the begins kernel on (ERROR|FATAL|PANIC): [0-9]+, untainted (HIP events around the kernel, best of 3)
    begins_bounded_ms    the star-free begins kernel on (ERROR|FATAL|PANIC): [0-9]{1,8}, same text
    route_ms, flip_ms    torch.flip of the text, then bmx_search_regex_star_device with the reversed automaton (events
                         around both); the flip alone
    forced_*             the same call with the slow path forced: phase times in microseconds
    tainted_*            [ab].*c on the text with every c turned into d and one c on its last byte: every lane tainted,
                         one chain as long as the text
    ends_*_ms            bmx_regex_star_ends_device over the lowest 2^20 starts of [a-z]+, window 4,096, longest, with and
                         without the early exit (events around the call)
    findall_*_ms         findall_device(posix=True, kind="regex_star") beside findall_device(merge=True, kind="regex_star")
                         on [0-9]+ (events around the call)

One JSON line per run.

    python tools/regex_star_begins_rate.py [--gib 1] [--out F]   (profiles/r21_regex_star_begins_rate.jsonl is one run's)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from parallel_implementation_of_string_matching_algorithms_opencl_amd import corpus, host  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    from test_gpu_regex_star_begins_speed import PLANTS, measure

    n = int(args.gib * corpus.GiB)
    ctx = host.Context(0, library=host.exp_lib())
    res, same = measure(ctx, n, emit=lambda r: None)
    res["lists_equal"] = bool(same)
    res["untainted"] = ctx.regex_star_begins_last()["tainted"] == 0

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(call, repeats=3):
        call()
        best = None
        for _ in range(repeats):
            ev[0].record()
            out = call()
            ev[1].record()
            torch.cuda.synchronize()
            t = ev[0].elapsed_time(ev[1])
            best = t if best is None else min(best, t)
        return out, best

    d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
    ctx.gen_text(d_text, 0, 0x57A25EED, 0)
    for i, p in enumerate(PLANTS):
        at = 1000 + i * (n // 7)
        d_text[at:at + len(p) + 1] = torch.frombuffer(bytearray(p + b" "), dtype=torch.uint8).cuda()
    out = torch.empty(1 << 16, dtype=torch.int64, device="cuda")
    phases = ("pieces", "columns", "first_us", "r1_us", "sweep_us", "r2_us")
    ctx.set_knob("regex_star_begins_force_slow", 1)
    for _ in range(2):
        ctx.search_regex_star_begins_device(d_text, res["expr"], out=out)
    last = ctx.regex_star_begins_last()
    res.update({"forced_" + k: last[k] for k in phases}, forced_ms=round(ctx.last_regex_star_begins_ms(), 4))
    ctx.set_knob("regex_star_begins_force_slow", 0)

    d_text[d_text == ord("c")] = ord("d")  # the one c is the text's last byte: no lower bound ever sees it
    d_text[n - 1] = ord("c")
    for _ in range(2):
        _, total = ctx.search_regex_star_begins_device(d_text, "[ab].*c", capacity=0)
    last = ctx.regex_star_begins_last()
    res.update({"tainted_" + k: last[k] for k in phases}, tainted_ms=round(ctx.last_regex_star_begins_ms(), 4),
               tainted_waves=last["tainted"], tainted_hits=int(total))

    starts, total = ctx.search_regex_star_begins_device(d_text, "[a-z]+", capacity=1 << 20)
    res.update(ends_expr="[a-z]+", ends_list=int(starts.numel()), ends_hits=int(total))
    (_, clipped), res["ends_longest_ms"] = timed(lambda: ctx.regex_star_ends_device(d_text, "[a-z]+", starts, window=4096, longest=True))
    ctx.set_knob("regex_star_ends_no_early_exit", 1)
    _, res["ends_longest_no_early_exit_ms"] = timed(lambda: ctx.regex_star_ends_device(d_text, "[a-z]+", starts, window=4096, longest=True), 1)
    ctx.set_knob("regex_star_ends_no_early_exit", 0)
    res["ends_clipped"] = clipped
    (_, off_p), res["findall_posix_ms"] = timed(lambda: ctx.findall_device(d_text, "[0-9]+", kind="regex_star", posix=True))
    (_, off_m), res["findall_merge_ms"] = timed(lambda: ctx.findall_device(d_text, "[0-9]+", kind="regex_star", merge=True))
    res["findall_matches"] = [int(off_p.numel() - 1), int(off_m.numel() - 1)]
    for k in ("ends_longest_ms", "ends_longest_no_early_exit_ms", "findall_posix_ms", "findall_merge_ms"):
        res[k] = round(res[k], 4)

    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(json.dumps(res) + "\n")
    ctx.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
