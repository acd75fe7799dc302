"""Gapped-search rate (bmx_search_gaps_device) on 4 GiB synthetic texts generated in HBM (bmx_gen_text_device):
printable-95 and ACGT, the 32- and the 64-bit kernel, four patterns per word width:

    literal    the corpus pattern, no optional position (16 and 40 positions); beside it the class kernel on the same
               classes, in the same run, and the ratio of the two
    zinc       C-x(2,4)-C-x(3)-[LIVMFYWC]-x(8)-H-x(3,5)-H (25 positions); for the 64-bit word two of them with x(5,10)
               between (60 positions)
    gap16      the corpus pattern with one .{0,16} in the middle (8 + 16 + 8 = 32 and 24 + 16 + 24 = 64 positions)
    all        wildcards only, .{8,16} and .{20,40}: every end from the shortest length on is a hit, counted with
               capacity 0

One JSON line per (text kind, word, pattern): kernel ms (HIP events, best of --iters after one warm-up call), the whole
call (host clock), TB/s of text, hits.  A last line per text kind: the starts pass (bmx_gaps_starts_device, device
events around the call) over the lowest 2^20 ends of a pattern with a few million hits.

    python tools/gaps_rate.py [--gib 4] [--iters 3] [--kinds 0,1] [--out F]     (no --out: the lines go to stdout only;
                                                                                 profiles/r13_gaps_rate.jsonl is one run's)
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

ZINC = "C-x(2,4)-C-x(3)-[LIVMFYWC]-x(8)-H-x(3,5)-H"


def escaped(pat: bytes) -> str:
    return "".join("\\x%02x" % b for b in pat)


def patterns(pat: bytes):
    """(name, word, (classes, optional)) for a corpus pattern of 48 bytes."""
    c = host.compile_gaps
    return [
        ("literal", 32, c(escaped(pat[:16]))), ("literal", 64, c(escaped(pat[:40]))),
        ("zinc", 32, c(ZINC, host.GAPS_PROSITE)), ("zinc", 64, c(ZINC + "-x(5,10)-" + ZINC, host.GAPS_PROSITE)),
        ("gap16", 32, c(escaped(pat[:8]) + ".{0,16}" + escaped(pat[8:16]))),
        ("gap16", 64, c(escaped(pat[:24]) + ".{0,16}" + escaped(pat[24:48]))),
        ("all", 32, c(".{8,16}")), ("all", 64, c(".{20,40}")),
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--kinds", default="0,1")
    ap.add_argument("--capacity", type=int, default=1 << 24, help="ends stored per call (`all` stores none)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    ctx = host.Context(0)
    n = int(args.gib * corpus.GiB)
    d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
    out = torch.empty(args.capacity, dtype=torch.int64, device="cuda")
    sink = open(args.out, "a") if args.out else None

    def emit(line):
        print(json.dumps(line), flush=True)
        if sink:
            sink.write(json.dumps(line) + "\n")
            sink.flush()

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
        seed = 0x5EED6A00 + kind
        ctx.gen_text(d_text, 0, seed, kind)
        torch.cuda.synchronize()
        pat = corpus.stream_bytes(corpus.PATTERN_STREAM_INDEX, 48, seed, kind).tobytes()
        ctx.plant(d_text, 0, pat, [n // 3])  # at least one hit of the literal and gap16 patterns
        for name, word, pair in patterns(pat):
            m = pair[0].shape[0]
            cap = 0 if name == "all" else args.capacity
            hits, ms, call_ms, all_ms = best(lambda: ctx.search_gaps_device(d_text, pair, out=out, capacity=cap)[1],
                                             ctx.last_gaps_ms)
            line = {"kind": ("printable95", "acgt")[kind], "n": n, "pattern": name, "word": word, "m": m,
                    "optional": bin(pair[1]).count("1"), "ms": round(ms, 4), "ms_all": [round(t, 4) for t in all_ms],
                    "call_ms": round(call_ms, 4), "tbps": round(n / (ms * 1e-3) / 1e12, 3), "hits": hits, "stored": min(hits, cap)}
            if name == "literal":
                c_hits, c_ms, c_call, _ = best(lambda: ctx.search_classes_device(d_text, pair[0], out=out)[1], ctx.last_classes_ms)
                assert c_hits == hits, (c_hits, hits)
                line.update({"classes_ms": round(c_ms, 4), "classes_call_ms": round(c_call, 4), "ratio": round(ms / c_ms, 3)})
            emit(line)
        # the starts of about 10^6 ends
        pair = host.compile_gaps("ACG.{0,2}TAC" if kind else "e.{0,2}[a-z]")
        ends, total = ctx.search_gaps_device(d_text, pair, out=out, capacity=1 << 20)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = []
        for longest in (False, True):
            ctx.gaps_starts_device(d_text, pair, ends, longest=longest)  # warm-up
            t = []
            for _ in range(args.iters):
                ev0.record()
                starts = ctx.gaps_starts_device(d_text, pair, ends, longest=longest)
                ev1.record()
                torch.cuda.synchronize()
                t.append(ev0.elapsed_time(ev1))
            assert bool((starts <= ends).all()) and bool((ends - starts < pair[0].shape[0]).all())
            times.append(round(min(t), 4))
        emit({"kind": ("printable95", "acgt")[kind], "n": n, "pattern": "starts", "m": int(pair[0].shape[0]), "hits": total,
              "list": int(ends.numel()), "starts_ms": times[0], "starts_longest_ms": times[1]})
    ctx.close()


if __name__ == "__main__":
    main()
