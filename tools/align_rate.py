"""Cost of the alignments (bmx_align_device) beside the starts pass that makes their input (bmx_approx_spans_device with
flags 0, bmx_approx_long_spans_device above 64 bytes), on the same list in the same process: the starts pass walks the
same columns once, with no stores and no traceback, so align / starts says what storing every column and walking back
costs.

Text: printable-95 generated in HBM (bmx_gen_text_device); the corpus pattern with its middle byte changed is planted
every KiB, so every occurrence has one substitution and the search for the unchanged pattern returns 2k - 1 ends around
each.  The first `entries` ends and their starts are the list; every entry aligns.

One JSON line per (m, k, entries): median and all times of --runs calls after --warmup calls of each pass (bmx_last_spans_ms,
bmx_last_align_ms: HIP events), the ratio of the medians, ns per entry, the alignment's launches, workspace bytes per entry
and the op words out.

    python tools/align_rate.py [--shapes 16:3,64:8,128:8,512:32] [--entries 65536,1048576] [--runs 20] [--warmup 5] [--out F]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from parallel_implementation_of_string_matching_algorithms_opencl_amd import corpus, host  # noqa: E402

PERIOD = 1024


def planted_list(ctx, m: int, k: int, entries: int, seed: int = 0x5EEDA119):
    """(d_text, pattern, ends, dist): a text with enough one-substitution copies of the pattern for `entries` ends."""
    import torch

    plants = -(-entries // (2 * k - 1)) + 2
    n = (plants + 2) * PERIOD
    d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
    ctx.gen_text(d_text, 0, seed, 0)
    pat = corpus.stream_bytes(corpus.PATTERN_STREAM_INDEX, m, seed, 0).tobytes()
    changed = bytearray(pat)
    changed[m // 2] = 32 + (changed[m // 2] - 32 + 1) % 95
    ctx.plant(d_text, 0, bytes(changed), np.arange(PERIOD // 2, n - 2 * PERIOD, PERIOD, dtype=np.uint64))
    torch.cuda.synchronize()
    room = (plants + 2) * (2 * k + 1)
    ends, dist, total = ctx.search_approx_device(d_text, pat, k, out=torch.empty(room, dtype=torch.int64, device="cuda"),
                                                 dist_out=torch.empty(room, dtype=torch.uint8, device="cuda"))
    assert entries <= total <= room, (total, entries, room)
    return d_text, pat, ends[:entries].contiguous(), dist[:entries].contiguous()


def workspace_bytes_per_entry(m: int, k: int) -> int:
    """The formula of include/bmx.h: columns x 2 planes x min(word bytes, band bytes), plus the slot and the run count."""
    word = 4 if m <= 32 else 8 * (1 if m <= 64 else 2 if m <= 128 else 4 if m <= 256 else 8)
    band = 4 * ((2 * k + 1 + 31) // 32)
    plane = band if m > 32 and k <= 63 and band < word else word
    return 8 * ((m + k + 7) // 8) * 2 * plane + 4 * (2 * k + 2)


def time_passes(ctx, d_text, pat, k, ends, dist, runs: int, warmup: int):
    """(starts ms, align ms, starts tensor, align result) -- all times of `runs` calls after `warmup` calls, each pass."""
    import torch

    count = ends.numel()
    t_starts, t_align = [], []
    for i in range(warmup + runs):
        starts, _, _, got = ctx.approx_spans_device(d_text, pat, k, ends, dist)
        assert got == count
        if i >= warmup:
            t_starts.append(ctx.last_spans_ms())
    out = (torch.empty(count, dtype=torch.uint8, device="cuda"), torch.empty(count + 1, dtype=torch.int64, device="cuda"),
           torch.empty(count * (2 * k + 1), dtype=torch.int32, device="cuda"))
    res = None
    for i in range(warmup + runs):
        res = ctx.align_device(d_text, [pat], starts, ends, k, out=out)
        if i >= warmup:
            t_align.append(ctx.last_align_ms())
    return t_starts, t_align, starts, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16:3,64:8,128:8,512:32")
    ap.add_argument("--entries", default="65536,1048576")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_align_rate.jsonl"))
    args = ap.parse_args()

    import torch

    ctx = host.Context(0)
    sink = open(args.out, "a") if args.out else None
    for shape in args.shapes.split(","):
        m, k = (int(x) for x in shape.split(":"))
        for entries in [int(x) for x in args.entries.split(",")]:
            d_text, pat, ends, dist = planted_list(ctx, m, k, entries)
            t_starts, t_align, starts, (adist, op_off, ops) = time_passes(ctx, d_text, pat, k, ends, dist, args.runs, args.warmup)
            assert bool((adist == dist).all()), "the global distance of a span is the distance of its end"
            s, a = statistics.median(t_starts), statistics.median(t_align)
            ws_bytes = workspace_bytes_per_entry(m, k)
            line = {"what": "align_over_starts", "m": m, "k": k, "entries": entries, "n": d_text.numel(),
                    "starts_ms": round(s, 4), "align_ms": round(a, 4), "align_over_starts": round(a / s, 3),
                    "align_ns_per_entry": round(a * 1e6 / entries, 2), "starts_ns_per_entry": round(s * 1e6 / entries, 2),
                    "launches": ctx.last_align_launches(), "workspace_bytes_per_entry": ws_bytes,
                    "ops": int(op_off[-1]), "runs": args.runs, "warmup": args.warmup,
                    "starts_ms_all": [round(t, 4) for t in t_starts], "align_ms_all": [round(t, 4) for t in t_align]}
            print(json.dumps(line), flush=True)
            if sink:
                sink.write(json.dumps(line) + "\n")
                sink.flush()
            del d_text, ends, dist, starts, adist, op_off, ops
            torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
