"""Time of the LCP array (bmx_lcp_array_device) beside the suffix-array build it follows, on the three texts of
tests/test_gpu_lcp_speed.py -- random lower-case, 2^25 bytes; a 61-letter paragraph repeated, 2^24 + 4,097 bytes; all 'a',
2^25 - 1 bytes -- and on random ACGT text of 2^25 bytes.

One JSON line per text: lcp_ms = HIP events around the LCP kernels (bmx_last_lcp_ms), suffix_array_ms = the build beside
it (bmx_last_suffix_array_ms), each the best of --iters after a warm-up with the two alternating; their ratio; the pairs
that left the one-lane path; max and sum of the array.

    python tools/lcp_rate.py [--iters 5] [--out F]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from parallel_implementation_of_string_matching_algorithms_opencl_amd import host  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_lcp_rate.jsonl"))
    args = ap.parse_args()

    import torch

    ctx = host.Context(0)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0x1C9)
    para = (np.random.default_rng(61).integers(0, 26, 61) + 97).astype(np.uint8)
    n_per = (1 << 24) + 4097
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    texts = [
        ("random lower-case", torch.randint(97, 123, (1 << 25,), device="cuda", generator=gen).to(torch.uint8)),
        ("61-letter paragraph repeated", torch.from_numpy(np.tile(para, n_per // 61 + 1)[:n_per].copy()).to("cuda")),
        ("all 'a'", torch.full(((1 << 25) - 1,), ord("a"), dtype=torch.uint8, device="cuda")),
        ("random ACGT", acgt[torch.randint(0, 4, (1 << 25,), device="cuda", generator=gen)]),
    ]
    sink = open(args.out, "a") if args.out else None
    for name, d_text in texts:
        sa_ms, lcp_ms = [], []
        for it in range(args.iters + 1):  # the first round is the warm-up
            d_sa = ctx.suffix_array_device(d_text)
            sa_ms.append(ctx.last_suffix_array_ms())
            d_lcp = ctx.lcp_array_device(d_text, d_sa)
            lcp_ms.append(ctx.last_lcp_ms())
        stats = ctx.lcp_stats_device(d_lcp)
        line = {"what": "lcp", "text": name, "n": d_text.numel(), "lcp_ms": round(min(lcp_ms[1:]), 4),
                "suffix_array_ms": round(min(sa_ms[1:]), 4), "lcp_over_suffix_array": round(min(lcp_ms[1:]) / min(sa_ms[1:]), 4),
                "long_pairs": ctx.last_lcp_long_pairs(), "max": stats["max"], "sum": stats["sum"]}
        print(json.dumps(line), flush=True)
        if sink:
            sink.write(json.dumps(line) + "\n")
            sink.flush()
        del d_sa, d_lcp
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
