"""Rate of the capture groups pass (bmx_regex_groups_device) and of the copy with a template (bmx_expand_device) on a 1 GiB
printable-95 text generated in HBM (bmx_gen_text_device) with 2^20 dates planted, each next to the existing pass that does
the comparable work on the same list, in the same run:

    groups     ([0-9]{4})-([0-9]{2})-([0-9]{2}) searched (bmx_search_regex_device, the lowest 2^20 ends), the starts pass
               (bmx_regex_starts_device) and the groups pass over that list, device events around each call
    expand     bmx_expand_device with a template without a reference beside bmx_replace_device with the same literal, and
               with \\3.\\2.\\1, over the selection of that list; the extract form with \\1 beside bmx_extract_device

One JSON line each: ms (best of --iters after one warm-up call), the kernels' own time, and the ratio to the neighbour.

    python tools/regex_groups_rate.py [--gib 1] [--iters 3] [--out F]   (no --out: the lines go to stdout only;
                                                                        profiles/r23_regex_groups_rate.jsonl is one run's)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from parallel_implementation_of_string_matching_algorithms_opencl_amd import corpus, host  # noqa: E402

EXPR = "([0-9]{4})-([0-9]{2})-([0-9]{2})"
COUNT = 1 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    ctx = host.Context(0)
    n = int(args.gib * corpus.GiB)
    d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
    ctx.gen_text(d_text, 0, 0x3434, 0)
    rng = np.random.default_rng(0x3434)
    at = np.sort(rng.choice(n // 32 - 1, COUNT, replace=False).astype(np.uint64)) * np.uint64(32)
    ctx.plant(d_text, 0, b"2026-10-21", at)
    sink = open(args.out, "a") if args.out else None
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def emit(line):
        print(json.dumps(line), flush=True)
        if sink:
            sink.write(json.dumps(line) + "\n")
            sink.flush()

    def best(call):
        res = call()  # warm-up
        times = []
        for _ in range(args.iters):
            ev[0].record()
            res = call()
            ev[1].record()
            torch.cuda.synchronize()
            times.append(ev[0].elapsed_time(ev[1]))
        return round(min(times), 4), res

    pair = host.compile_regex_groups(EXPR)
    ends, total = ctx.search_regex_device(d_text, pair[0], capacity=COUNT, out=torch.empty(COUNT, dtype=torch.int64, device="cuda"))
    t_starts, starts = best(lambda: ctx.regex_starts_device(d_text, pair[0], ends))
    t_groups, groups = best(lambda: ctx.regex_groups_device(d_text, pair, starts, ends))
    assert bool((groups[:, 0, 0] == starts).all()) and bool((groups[:, 0, 1] == ends + 1).all())
    emit({"n": n, "pattern": "groups", "expr": EXPR, "m": pair[0].m, "hits": total, "list": int(ends.numel()), "starts_ms": t_starts,
          "groups_ms": t_groups, "groups_kernel_ms": round(ctx.last_regex_groups_ms(), 4), "ratio": round(t_groups / t_starts, 3)})

    s, e = ctx.select_spans_device(starts, ends)
    groups = ctx.regex_groups_device(d_text, pair, s, e)
    out = torch.empty(n + 16 * s.numel(), dtype=torch.uint8, device="cuda")
    lit = b"<redacted>"
    t_replace, (want, _) = best(lambda: ctx.replace_device(d_text, s, e, lit, out=out))
    k_replace = ctx.last_subst_ms()
    want = want.clone()
    t_expand, (got, _) = best(lambda: ctx.expand_device(d_text, groups, lit, out=out))
    assert torch.equal(got, want)
    emit({"n": n, "pattern": "expand_literal", "matches": int(s.numel()), "replace_ms": t_replace, "replace_kernels_ms": round(k_replace, 4),
          "expand_ms": t_expand, "expand_kernels_ms": round(ctx.last_subst_ms(), 4), "ratio": round(t_expand / t_replace, 3)})
    del want
    t_swap, (got, n_out) = best(lambda: ctx.expand_device(d_text, groups, "\\3.\\2.\\1", out=out))
    assert n_out == n
    emit({"n": n, "pattern": "expand_swap", "template": "\\3.\\2.\\1", "matches": int(s.numel()), "expand_ms": t_swap,
          "expand_kernels_ms": round(ctx.last_subst_ms(), 4), "ratio_to_replace": round(t_swap / t_replace, 3)})
    t_extract, (blob, _) = best(lambda: ctx.extract_device(d_text, groups[:, 1, 0].contiguous(), groups[:, 1, 1].contiguous() - 1, out=out))
    want = blob.clone()
    t_column, (got, _) = best(lambda: ctx.expand_device(d_text, groups, "\\1", extract=True, out=out))
    assert torch.equal(got, want)
    emit({"n": n, "pattern": "extract_group", "matches": int(s.numel()), "extract_ms": t_extract, "expand_ms": t_column,
          "ratio": round(t_column / t_extract, 3)})
    ctx.close()


if __name__ == "__main__":
    main()
