"""Rate of the text index's read mapping (bmx_index_map_device) on a random lower-case text made in HBM: n = 2^--log2n,
R reads of m bytes cut from the text with one byte replaced at a random place in every --every, for every combination of
--reads (log2 R), --lengths (m) and --edits (k).

One JSON line per combination, every number from the same run: the candidate count, the map call's ms (bmx_last_index_ms,
best of --iters after a warm-up) and, from that best call, its phases (bmx_last_index_map_phases): candidate expansion
(match kernel, scan, fill), verification with the 64-bit words of the instance that ran, start pass, per-query best; next
to them the seeds call's ms over the same reads, and how many reads mapped.

    python tools/index_map_rate.py [--log2n 25] [--reads 13,16] [--lengths 128,256] [--edits 4,8] [--iters 3] [--out F]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from parallel_implementation_of_string_matching_algorithms_opencl_amd import host  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=25)
    ap.add_argument("--reads", default="13,16")
    ap.add_argument("--lengths", default="128,256")
    ap.add_argument("--edits", default="4,8")
    ap.add_argument("--every", type=int, default=32)
    ap.add_argument("--min-len", type=int, default=16)
    ap.add_argument("--max-occ", type=int, default=8)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_index_map_rate.jsonl"))
    args = ap.parse_args()

    import torch

    ctx = host.Context(0)
    sink = open(args.out, "a") if args.out else None
    n = 1 << args.log2n
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0x5EED + args.log2n)
    d_text = torch.randint(97, 123, (n,), device="cuda", generator=gen).to(torch.uint8)
    idx = ctx.index(d_text)
    for lr in (int(x) for x in args.reads.split(",")):
        for m in (int(x) for x in args.lengths.split(",")):
            R = 1 << lr
            at = torch.randint(0, n - m, (R,), device="cuda", generator=gen)
            reads = d_text[at[:, None] + torch.arange(m, device="cuda")]
            rows = torch.arange(R, device="cuda")
            for lo in range(0, m, args.every):
                where = lo + torch.randint(0, min(args.every, m - lo), (R,), device="cuda", generator=gen)
                reads[rows, where] = torch.randint(97, 123, (R,), device="cuda", generator=gen).to(torch.uint8)
            q = (reads.reshape(-1), torch.arange(0, R * m + 1, m, dtype=torch.int64, device="cuda"))
            idx.seeds(q, args.min_len, args.max_occ, capacity=0)
            seeds_ms = []
            for _ in range(args.iters):
                n_seeds = int(idx.seeds(q, args.min_len, args.max_occ, capacity=0)[0][-1])
                seeds_ms.append(ctx.last_index_ms())
            for k in (int(x) for x in args.edits.split(",")):
                idx.map(q, args.min_len, args.max_occ, k)
                best_ms, phases, dist = None, None, None
                for _ in range(args.iters):
                    dist = idx.map(q, args.min_len, args.max_occ, k)[2]
                    if best_ms is None or ctx.last_index_ms() < best_ms:
                        best_ms, phases = ctx.last_index_ms(), ctx.last_index_map_phases()
                line = {"what": "map", "n": n, "reads": R, "m": m, "k": k, "every": args.every, "min_len": args.min_len,
                        "max_occ": args.max_occ, "seeds": n_seeds, "candidates": ctx.last_index_map_candidates(),
                        "mapped": int((dist != host.MAP_NO_HIT).sum()), "seeds_ms": round(min(seeds_ms), 4),
                        "map_ms": round(best_ms, 4), "words": phases["words"]}
                line.update({key: round(phases[key], 4) for key in ("expand_ms", "verify_ms", "start_ms", "best_ms")})
                print(json.dumps(line), flush=True)
                if sink:
                    sink.write(json.dumps(line) + "\n")
                    sink.flush()
    idx.close()
    ctx.close()


if __name__ == "__main__":
    main()
