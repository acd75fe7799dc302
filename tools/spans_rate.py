"""Cost of the match spans (bmx_approx_spans_device) beside the approximate search that makes their input, on synthetic
texts generated in HBM (bmx_gen_text_device): printable-95 and ACGT, m in {16, 32, 64}, k in {1, 4, m / 4}, the corpus
pattern planted every --period bytes so that every shape has ends to work on.

One JSON line per (text kind, m, k): the search's kernel ms (bmx_last_approx_ms) and, on its list in the same run, the
spans time (bmx_last_spans_ms: HIP events around the spans kernels) with flags == 0 and with BMX_SPANS_BEST, each the best
of --iters after one warm-up call, the entries in and out, and ns per entry.  Then the dense list: ACGT, m = 8, k = 4 on
the first --dense-gib GiB, where most positions are ends, with and without BMX_SPANS_BEST.

    python tools/spans_rate.py [--gib 4] [--dense-gib 4] [--iters 3] [--kinds 0,1] [--ms 16,32,64] [--out F]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from parallel_implementation_of_string_matching_algorithms_opencl_amd import corpus, host  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--dense-gib", type=float, default=4.0)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--kinds", default="0,1")
    ap.add_argument("--ms", default="16,32,64")
    ap.add_argument("--period", type=int, default=1 << 16, help="the pattern is planted every so many bytes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_spans_rate.jsonl"))
    args = ap.parse_args()

    import torch

    ctx = host.Context(0)
    n = int(args.gib * corpus.GiB)
    d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
    sink = open(args.out, "a") if args.out else None

    def emit(line):
        print(json.dumps(line), flush=True)
        if sink:
            sink.write(json.dumps(line) + "\n")
            sink.flush()

    def spans(view, pat, k, ends, dist, best):
        kept = ctx.approx_spans_device(view, pat, k, ends, dist, best=best)[3]  # warm-up
        times = []
        for _ in range(args.iters):
            assert ctx.approx_spans_device(view, pat, k, ends, dist, best=best)[3] == kept
            times.append(ctx.last_spans_ms())
        return kept, min(times), times

    def measure(view, kind, pat, k, what):
        m = len(pat)
        total = ctx.search_approx_device(view, pat, k, capacity=0)[2]  # counting (and the warm-up)
        out = torch.empty(max(total, 1), dtype=torch.int64, device="cuda")
        dist = torch.empty(max(total, 1), dtype=torch.uint8, device="cuda")
        search = []
        for _ in range(args.iters):
            ends, dists, got = ctx.search_approx_device(view, pat, k, out=out, dist_out=dist)
            assert got == total
            search.append(ctx.last_approx_ms())
        line = {"what": what, "kind": ("printable95", "acgt")[kind], "n": view.numel(), "m": m, "k": k,
                "word": 32 if m <= 32 else 64, "ends": total, "approx_ms": round(min(search), 4)}
        if total:
            _, ms0, all0 = spans(view, pat, k, ends, dists, False)
            kept, ms1, all1 = spans(view, pat, k, ends, dists, True)
            line.update({"spans_ms": round(ms0, 4), "spans_ms_all": [round(t, 4) for t in all0],
                         "spans_ns_per_end": round(ms0 * 1e6 / total, 3), "spans_over_search": round(ms0 / min(search), 4),
                         "best_kept": kept, "best_ms": round(ms1, 4), "best_ms_all": [round(t, 4) for t in all1],
                         "best_over_search": round(ms1 / min(search), 4)})
        emit(line)
        del out, dist
        torch.cuda.empty_cache()

    for kind in [int(x) for x in args.kinds.split(",")]:
        seed = 0x5EED5A00 + kind
        for m in [int(x) for x in args.ms.split(",")]:
            ctx.gen_text(d_text, 0, seed, kind)  # afresh: the plants of the last m are gone
            pat = corpus.stream_bytes(corpus.PATTERN_STREAM_INDEX, m, seed, kind).tobytes()
            ctx.plant(d_text, 0, pat, np.arange(args.period // 2, n - 2 * m, args.period, dtype=np.uint64))
            torch.cuda.synchronize()
            for k in sorted({1, 4, m // 4}):
                measure(d_text, kind, pat, k, "planted")

    if args.dense_gib > 0:
        ctx.gen_text(d_text, 0, 0x5EED5A09, 1)
        torch.cuda.synchronize()
        measure(d_text[:int(min(args.dense_gib, args.gib) * corpus.GiB)], 1, b"ACGTTGCA", 4, "dense")
    ctx.close()


if __name__ == "__main__":
    main()
