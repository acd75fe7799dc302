"""k-mismatch search rate (bmx_search_hamming_device) on 4 GiB synthetic texts generated in HBM (bmx_gen_text_device):
printable-95 and ACGT, m in {8, 16, 20, 32, 33, 64} and k in {1, 3, 4, 8, 15} (where k < m), the corpus pattern as a
string with must = 0, planted once.  k <= 3 runs the two-slice kernel, k >= 4 the four-slice one; m <= 32 the 32-bit word,
above it the 64-bit one.

One JSON line per (text kind, m, k): kernel ms (HIP events, best of --iters after one warm-up call), the whole call (host
clock), TB/s of text, hits; beside it the approximate search at the same pattern and k (bmx_search_approx_device) in the
same run, and the ratio of the two kernels.  Then per text kind one line for a 23-position guide + NGG class pattern
(20 bases, any base, G, G) at k = 3 with `must` on the two G, with must = 0, and the approximate search with the same
classes.

    python tools/hamming_rate.py [--gib 4] [--iters 3] [--kinds 0,1] [--ms 8,16,20,32,33,64] [--ks 1,3,4,8,15] [--out F] [--note TEXT]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from parallel_implementation_of_string_matching_algorithms_opencl_amd import corpus, host  # noqa: E402


def guide_classes(guide: bytes, kind: int) -> np.ndarray:
    """The guide as singletons, then N (the whole alphabet of the text) and two G."""
    alphabet = np.frombuffer(b"ACGT", np.uint8) if kind else np.arange(0x20, 0x7F, dtype=np.uint8)
    member = np.zeros((len(guide) + 3, 256), dtype=bool)
    member[np.arange(len(guide)), np.frombuffer(guide, np.uint8)] = True
    member[len(guide)][alphabet] = True
    member[len(guide) + 1:, ord("G")] = True
    return np.packbits(member, axis=1, bitorder="little")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--kinds", default="0,1")
    ap.add_argument("--ms", default="8,16,20,32,33,64")
    ap.add_argument("--ks", default="1,3,4,8,15")
    ap.add_argument("--capacity", type=int, default=1 << 24, help="entries stored per call")
    ap.add_argument("--out", default="")
    ap.add_argument("--note", default="", help="stored in every line (which build this is, when two are compared)")
    args = ap.parse_args()

    import torch

    ctx = host.Context(0)
    n = int(args.gib * corpus.GiB)
    d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
    out = torch.empty(args.capacity, dtype=torch.int64, device="cuda")
    dist = torch.empty(args.capacity, dtype=torch.uint8, device="cuda")
    sink = open(args.out, "a") if args.out else None

    def best(call, last_ms):
        hits = call()  # warm-up
        kernel, whole = [], []
        for _ in range(args.iters):
            t0 = time.perf_counter()
            h = call()
            whole.append((time.perf_counter() - t0) * 1e3)
            assert h == hits, (h, hits)
            kernel.append(last_ms())
        return hits, min(kernel), min(whole), kernel

    def emit(line):
        print(json.dumps(line), flush=True)
        if sink:
            sink.write(json.dumps(line) + "\n")
            sink.flush()

    def measure(kind, m, k, what, pattern, must, approx):
        hits, ms, call_ms, all_ms = best(
            lambda: ctx.search_hamming_device(d_text, pattern, k, must=must, out=out, dist_out=dist)[2], ctx.last_hamming_ms)
        a_hits, a_ms, a_call, a_all = best(approx, ctx.last_approx_ms)
        assert a_hits >= hits >= 1, (a_hits, hits)  # every hit's end is an approximate end
        emit({**({"note": args.note} if args.note else {}), "kind": ("printable95", "acgt")[kind], "n": n, "m": m, "k": k,
              "pattern": what, "must": must, "word": 32 if m <= 32 else 64, "slices": 2 if k <= 3 else 4, "ms": round(ms, 4),
              "ms_all": [round(t, 4) for t in all_ms], "call_ms": round(call_ms, 4), "tbps": round(n / (ms * 1e-3) / 1e12, 3),
              "hits": hits, "stored": min(hits, args.capacity), "approx_ms": round(a_ms, 4),
              "approx_ms_all": [round(t, 4) for t in a_all], "approx_call_ms": round(a_call, 4), "approx_hits": a_hits,
              "ratio": round(ms / a_ms, 3)})

    for kind in [int(x) for x in args.kinds.split(",")]:
        seed = 0x5EED4A00 + kind
        ctx.gen_text(d_text, 0, seed, kind)
        torch.cuda.synchronize()
        for m in [int(x) for x in args.ms.split(",")]:
            pat = corpus.stream_bytes(corpus.PATTERN_STREAM_INDEX, m, seed, kind).tobytes()
            ctx.plant(d_text, 0, pat, [n // 3])  # at least one hit of every pattern
            for k in [int(x) for x in args.ks.split(",")]:
                if k >= m:
                    continue
                measure(kind, m, k, "string", pat, 0,
                        lambda: ctx.search_approx_device(d_text, pat, k, out=out, dist_out=dist)[2])
        guide = corpus.stream_bytes(corpus.PATTERN_STREAM_INDEX, 20, seed, kind).tobytes()
        ctx.plant(d_text, 0, guide + b"AGG", [n // 5])
        cls = guide_classes(guide, kind)
        for must in ((1 << 21) | (1 << 22), 0):
            measure(kind, 23, 3, "guide+NGG", cls, must,
                    lambda: ctx.search_approx_classes_device(d_text, cls, 3, out=out, dist_out=dist)[2])
    ctx.close()


if __name__ == "__main__":
    main()
