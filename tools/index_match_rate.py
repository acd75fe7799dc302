"""Rate of the text index's matching statistics and seeds (bmx_index_match_device, bmx_index_seeds_device) on a random
lower-case text made in HBM: n = 2^k for the --log2n given, R reads of m bytes cut from the text with one byte replaced at a
random place in every --every, for the --shapes given as log2(R):m pairs.

One JSON line per shape: the match kernel's ms (bmx_last_index_ms, best of --iters after a warm-up) with the directory and
-- through the experiments build's switch "index_no_dir" -- without it, ns per position, the mean match length, the ms of
Index.count over the same reads as whole queries (one lane per read, for scale), and the seeds call's ms and seed count
for --min-len / --max-occ.

    python tools/index_match_rate.py [--log2n 25] [--shapes 13:128,16:128,13:512,17:32] [--every 32] [--iters 3] [--out F]
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
    ap.add_argument("--log2n", default="25", help="comma-separated; 25 is the largest size the builder is tested at")
    ap.add_argument("--shapes", default="13:128,16:128,13:512,17:32")
    ap.add_argument("--every", type=int, default=32)
    ap.add_argument("--min-len", type=int, default=16)
    ap.add_argument("--max-occ", type=int, default=0)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_index_match_rate.jsonl"))
    args = ap.parse_args()

    import torch

    ctx = host.Context(0, library=host.exp_lib())  # the same sources, with the switch
    sink = open(args.out, "a") if args.out else None

    def emit(line):
        print(json.dumps(line), flush=True)
        if sink:
            sink.write(json.dumps(line) + "\n")
            sink.flush()

    def best(call):
        call()
        times = []
        for _ in range(args.iters):
            call()
            times.append(ctx.last_index_ms())
        return min(times)

    for k in [int(x) for x in args.log2n.split(",")]:
        n = 1 << k
        gen = torch.Generator(device="cuda")
        gen.manual_seed(0x5EED + k)
        d_text = torch.randint(97, 123, (n,), device="cuda", generator=gen).to(torch.uint8)
        idx = ctx.index(d_text)
        for shape in args.shapes.split(","):
            lr, m = (int(x) for x in shape.split(":"))
            R = 1 << lr
            at = torch.randint(0, n - m, (R,), device="cuda", generator=gen)
            reads = d_text[at[:, None] + torch.arange(m, device="cuda")]
            rows = torch.arange(R, device="cuda")
            for lo in range(0, m, args.every):
                where = lo + torch.randint(0, min(args.every, m - lo), (R,), device="cuda", generator=gen)
                reads[rows, where] = torch.randint(97, 123, (R,), device="cuda", generator=gen).to(torch.uint8)
            q = (reads.reshape(-1), torch.arange(0, R * m + 1, m, dtype=torch.int64, device="cuda"))
            ctx.set_knob("index_no_dir", 0)
            with_dir = best(lambda: idx.match(q))
            mean_len = float(idx.match(q)[0].double().mean())
            ctx.set_knob("index_no_dir", 1)
            plain = best(lambda: idx.match(q))
            ctx.set_knob("index_no_dir", 0)
            count_ms = best(lambda: idx.count(q))
            seeds_ms = best(lambda: idx.seeds(q, args.min_len, args.max_occ, capacity=R * m))
            n_seeds = int(idx.seeds(q, args.min_len, args.max_occ, capacity=0)[0][-1])
            emit({"what": "match", "n": n, "reads": R, "m": m, "every": args.every, "positions": R * m,
                  "match_ms": round(with_dir, 4), "match_ms_no_directory": round(plain, 4),
                  "ns_per_position": round(with_dir * 1e6 / (R * m), 3), "mean_len": round(mean_len, 2),
                  "count_ms_whole_reads": round(count_ms, 4), "seeds_ms": round(seeds_ms, 4), "min_len": args.min_len,
                  "max_occ": args.max_occ, "seeds": n_seeds})
            del q, reads
            torch.cuda.empty_cache()
        idx.close()
        del d_text
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
