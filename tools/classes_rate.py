"""Class-search rate (bmx_search_classes_device) on 4 GiB synthetic texts generated in HBM (bmx_gen_text_device):
printable-95 and ACGT, m in {8, 16, 32, 33, 64}, four patterns per m:

    literal    the corpus pattern as singleton classes
    wild4      the same with every fourth position a wildcard
    primer     the same with IUPAC-style degenerate positions: every third position a two-member class (the byte and
               its successor in the alphabet), every seventh the whole alphabet (ACGT: N; printable-95: all 95)
    all        every position a wildcard: every start is a hit, counted with capacity 0

One JSON line per (text kind, m, pattern): kernel ms (HIP events, best of --iters after one warm-up call), the whole
call (host clock), TB/s of text, hits.  Beside each literal line the approximate search at k = 0 on the same string
(bmx_search_approx_device), and the ratio of the two kernels.

    python tools/classes_rate.py [--gib 4] [--iters 3] [--kinds 0,1] [--ms 8,16,32,33,64] [--out F]
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


def pack(member):
    return np.packbits(member, axis=1, bitorder="little")


def patterns(pat: bytes, kind: int):
    m = len(pat)
    alphabet = np.frombuffer(b"ACGT", np.uint8) if kind else np.arange(0x20, 0x7F, dtype=np.uint8)
    literal = np.zeros((m, 256), dtype=bool)
    literal[np.arange(m), np.frombuffer(pat, np.uint8)] = True
    wild4 = literal.copy()
    wild4[3::4] = True
    primer = literal.copy()
    for i in range(2, m, 3):
        at = int(np.nonzero(alphabet == pat[i])[0][0])
        primer[i][alphabet[(at + 1) % alphabet.size]] = True
    for i in range(6, m, 7):
        primer[i][alphabet] = True
    return [("literal", literal), ("wild4", wild4), ("primer", primer), ("all", np.ones((m, 256), dtype=bool))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--kinds", default="0,1")
    ap.add_argument("--ms", default="8,16,32,33,64")
    ap.add_argument("--capacity", type=int, default=1 << 24, help="starts stored per call (`all` stores none)")
    ap.add_argument("--out", default="")
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

    for kind in [int(x) for x in args.kinds.split(",")]:
        seed = 0x5EEDC400 + kind
        ctx.gen_text(d_text, 0, seed, kind)
        torch.cuda.synchronize()
        for m in [int(x) for x in args.ms.split(",")]:
            pat = corpus.stream_bytes(corpus.PATTERN_STREAM_INDEX, m, seed, kind).tobytes()
            ctx.plant(d_text, 0, pat, [n // 3])  # at least one hit of every pattern
            for name, member in patterns(pat, kind):
                cls = pack(member)
                cap = 0 if name == "all" else args.capacity
                hits, ms, call_ms, all_ms = best(lambda: ctx.search_classes_device(d_text, cls, out=out, capacity=cap)[1],
                                                 ctx.last_classes_ms)
                line = {"kind": ("printable95", "acgt")[kind], "n": n, "m": m, "pattern": name, "word": 32 if m <= 32 else 64,
                        "ms": round(ms, 4), "ms_all": [round(t, 4) for t in all_ms], "call_ms": round(call_ms, 4),
                        "tbps": round(n / (ms * 1e-3) / 1e12, 3), "hits": hits, "stored": min(hits, cap)}
                if name == "literal":
                    a_hits, a_ms, a_call, _ = best(lambda: ctx.search_approx_device(d_text, pat, 0, out=out, dist_out=dist)[2],
                                                   ctx.last_approx_ms)
                    assert a_hits == hits, (a_hits, hits)
                    line.update({"approx_k0_ms": round(a_ms, 4), "approx_k0_call_ms": round(a_call, 4),
                                 "ratio": round(ms / a_ms, 3)})
                print(json.dumps(line), flush=True)
                if sink:
                    sink.write(json.dumps(line) + "\n")
                    sink.flush()
    ctx.close()


if __name__ == "__main__":
    main()
