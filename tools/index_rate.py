"""Build time and query rate of the text index (bmx_index_*) on random lower-case texts made in HBM: n = 2^k for the --log2n
given, Q = 2^16 .. 2^24 queries of m = 8 / 32 / 256 bytes, half of them cut from the text and half random, counted with
the directory and -- through the experiments build's switch "index_no_dir" -- without it, plus one locate per shape where
the positions fit --locate-cap.

One JSON line per n with the build times (suffix array + directory, and the directory alone over a caller's array), then
one per (n, Q, m): the count kernel's ms (bmx_last_index_ms, best of --iters after a warm-up) with and without the
directory, queries per second, and the locate's ms and positions.

    python tools/index_rate.py [--log2n 25] [--log2q 16,20,24] [--ms 8,32,256] [--iters 3] [--out F]
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
    ap.add_argument("--log2q", default="16,20,24")
    ap.add_argument("--ms", default="8,32,256")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--locate-cap", type=int, default=1 << 28, help="a locate is measured where the positions are fewer")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_index_rate.jsonl"))
    args = ap.parse_args()

    import torch

    ctx = host.Context(0, library=host.exp_lib())  # the same sources, with the switch
    sink = open(args.out, "a") if args.out else None

    def emit(line):
        print(json.dumps(line), flush=True)
        if sink:
            sink.write(json.dumps(line) + "\n")
            sink.flush()

    def queries(d_text, Q, m, gen):
        """(blob, offsets) on the device: Q / 2 windows of the text, Q / 2 random strings, made in pieces of 2^20."""
        blob = torch.empty(Q * m, dtype=torch.uint8, device="cuda")
        view = blob.view(Q, m)
        step, ar = 1 << 20, torch.arange(m, device="cuda")
        for lo in range(0, Q // 2, step):
            hi = min(lo + step, Q // 2)
            at = torch.randint(0, d_text.numel() - m, (hi - lo,), device="cuda", generator=gen)
            view[lo:hi] = d_text[at[:, None] + ar]
            view[Q // 2 + lo:Q // 2 + hi] = torch.randint(97, 123, (hi - lo, m), device="cuda", generator=gen).to(torch.uint8)
        return blob, torch.arange(0, Q * m + 1, m, dtype=torch.int64, device="cuda")

    def best_count(idx, q):
        idx.count(q)
        times = []
        for _ in range(args.iters):
            idx.count(q)
            times.append(ctx.last_index_ms())
        return min(times)

    for k in [int(x) for x in args.log2n.split(",")]:
        n = 1 << k
        gen = torch.Generator(device="cuda")
        gen.manual_seed(0x1DE5 + k)
        d_text = torch.randint(97, 123, (n,), device="cuda", generator=gen).to(torch.uint8)
        idx = ctx.index(d_text)
        own = ctx.index(d_text, sa=idx.sa)
        emit({"what": "build", "n": n, "build_ms": round(idx.build_ms, 3), "suffix_array_ms": round(ctx.last_suffix_array_ms(), 3),
              "directory_ms": round(own.build_ms, 3)})
        own.close()
        for lq in [int(x) for x in args.log2q.split(",")]:
            for m in [int(x) for x in args.ms.split(",")]:
                Q = 1 << lq
                q = queries(d_text, Q, m, gen)
                ctx.set_knob("index_no_dir", 0)
                with_dir = best_count(idx, q)
                ctx.set_knob("index_no_dir", 1)
                plain = best_count(idx, q)
                ctx.set_knob("index_no_dir", 0)
                line = {"what": "count", "n": n, "Q": Q, "m": m, "count_ms": round(with_dir, 4),
                        "count_ms_no_directory": round(plain, 4), "queries_per_s": round(Q / (with_dir * 1e-3)),
                        "ns_per_query": round(with_dir * 1e6 / Q, 2)}
                total = idx.locate(q, capacity=0)[2]
                if 0 < total <= args.locate_cap:
                    times = []
                    for _ in range(args.iters):
                        assert idx.locate(q, capacity=total)[2] == total
                        times.append(ctx.last_index_ms())
                    line.update({"positions": total, "locate_ms": round(min(times), 4)})
                emit(line)
                del q
                torch.cuda.empty_cache()
        idx.close()
        del d_text
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
