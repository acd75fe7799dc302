"""Approximate-search rate (bmx_search_approx_device) on 4 GiB synthetic texts generated in HBM (bmx_gen_text_device):
printable-95 and ACGT, m in {8, 16, 32, 33, 64}, k in {0, 1, 2, 4, 8} (k < m).  One JSON line per (text kind, m, k):
kernel ms (HIP events, best of --iters after one warm-up call), GB/s of text, hits, and `frac` against the VALU bound

    bound_ms = n * ops_per_char / (256 CU * 128 lane-ops/clk * 2.4 GHz)

with ops_per_char the 32-bit lane operations of the recurrence per character for the word width:
20 for the 32-bit word (m <= 32), 35 for the 64-bit word.  The kernel is compute-bound, not HBM-bound.

    python tools/approx_rate.py [--gib 4] [--iters 3] [--kinds 0,1] [--ms 8,16,32,33,64] [--ks 0,1,2,4,8] [--out F]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from parallel_implementation_of_string_matching_algorithms_opencl_amd import corpus, host  # noqa: E402

OPS_PER_CHAR = {32: 20, 64: 35}
LANE_OPS_PER_S = 256 * 128 * 2.4e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--kinds", default="0,1")
    ap.add_argument("--ms", default="8,16,32,33,64")
    ap.add_argument("--ks", default="0,1,2,4,8")
    ap.add_argument("--capacity", type=int, default=1 << 24, help="ends stored per call (dense results count the rest)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    ctx = host.Context(0)
    n = int(args.gib * corpus.GiB)
    d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
    out = torch.empty(args.capacity, dtype=torch.int64, device="cuda")
    dist = torch.empty(args.capacity, dtype=torch.uint8, device="cuda")
    sink = open(args.out, "a") if args.out else None
    for kind in [int(x) for x in args.kinds.split(",")]:
        seed = 0x5EEDA400 + kind
        ctx.gen_text(d_text, 0, seed, kind)
        torch.cuda.synchronize()
        for m in [int(x) for x in args.ms.split(",")]:
            pat = corpus.stream_bytes(corpus.PATTERN_STREAM_INDEX, m, seed, kind).tobytes()
            for k in [int(x) for x in args.ks.split(",")]:
                if k >= m:
                    continue
                _, _, hits = ctx.search_approx_device(d_text, pat, k, out=out, dist_out=dist)  # warm-up
                times = []
                for _ in range(args.iters):
                    _, _, h = ctx.search_approx_device(d_text, pat, k, out=out, dist_out=dist)
                    assert h == hits, (h, hits)
                    times.append(ctx.last_approx_ms())
                ms = min(times)
                word = 32 if m <= 32 else 64
                bound_ms = n * OPS_PER_CHAR[word] / LANE_OPS_PER_S * 1e3
                line = {"kind": ("printable95", "acgt")[kind], "n": n, "m": m, "k": k, "word": word, "ms": round(ms, 4),
                        "ms_all": [round(t, 4) for t in times], "gbps": round(n / (ms * 1e-3) / 1e9, 1), "hits": hits,
                        "stored": min(hits, args.capacity), "ops_per_char": OPS_PER_CHAR[word],
                        "valu_bound_ms": round(bound_ms, 4), "frac": round(bound_ms / ms, 3)}
                print(json.dumps(line), flush=True)
                if sink:
                    sink.write(json.dumps(line) + "\n")
                    sink.flush()
    ctx.close()


if __name__ == "__main__":
    main()
