"""Rate of the approximate search with patterns of up to 512 bytes (bmx_search_approx_long_device) and of the starts pass
on its lists (bmx_approx_long_spans_device), on printable-95 text generated in HBM (bmx_gen_text_device), the 512-byte
corpus pattern planted every --period bytes (its prefixes are the shorter patterns).

Per text size (--gibs, default 1 and 4 GiB, views of one buffer) one JSON line per (m, k): m = 64 through the old entry
(the one-word kernel: the yardstick) and m = 65, 128, 256, 512 through the new one, each at k = 4 and k = m / 8.  A line
holds the search's kernel ms (bmx_last_approx_ms, best of --iters after a warm-up call), the words per lane, the ratio to
the m = 64 line of the same k rule, the ends, and the spans pass on that list (bmx_last_spans_ms) with flags == 0 and with
BMX_SPANS_BEST.

Then the controls on the largest text: the three searches that share the tile frame, re-measured in the shapes of
tools/approx_rate.py, tools/classes_rate.py and tools/gaps_rate.py (profiles/r14_tile_frame_rate.jsonl has their
earlier times), and the three times of tests/test_gpu_approx_long_speed.py on 256 MiB.

    python tools/approx_long_rate.py [--gibs 1,4] [--iters 3] [--period 1048576] [--out F]     (no --out: the lines go to
                                                       stdout only; profiles/r15_approx_long_rate.jsonl is one run's)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from parallel_implementation_of_string_matching_algorithms_opencl_amd import corpus, host  # noqa: E402


def escaped(pat: bytes) -> str:
    return "".join("\\x%02x" % b for b in pat)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gibs", default="1,4")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--period", type=int, default=1 << 20, help="the pattern is planted every so many bytes")
    ap.add_argument("--out", default="", help="append the lines to this file too")
    args = ap.parse_args()

    import torch

    ctx = host.Context(0)
    gibs = [float(x) for x in args.gibs.split(",")]
    n_max = int(max(gibs) * corpus.GiB)
    d_text = torch.empty(n_max, dtype=torch.uint8, device="cuda")
    sink = open(args.out, "a") if args.out else None

    def emit(line):
        print(json.dumps(line), flush=True)
        if sink:
            sink.write(json.dumps(line) + "\n")
            sink.flush()

    def best_of(call, last_ms):
        first = call()  # warm-up
        times = []
        for _ in range(args.iters):
            assert call() == first
            times.append(last_ms())
        return first, min(times), [round(t, 4) for t in times]

    seed = 0x5EED7A00
    ctx.gen_text(d_text, 0, seed, 0)
    pat512 = corpus.stream_bytes(corpus.PATTERN_STREAM_INDEX, 512, seed, 0).tobytes()
    ctx.plant(d_text, 0, pat512, np.arange(args.period // 2, n_max - 1024, args.period, dtype=np.uint64))
    torch.cuda.synchronize()

    for gib in gibs:
        n = int(gib * corpus.GiB)
        view = d_text[:n]
        yard = {}
        for m in (64, 65, 128, 256, 512):
            pat = pat512[:m]
            for rule, k in (("4", 4), ("m/8", m // 8)):
                total = ctx.search_approx_device(view, pat, k, capacity=0)[2]  # counting
                out = torch.empty(max(total, 1), dtype=torch.int64, device="cuda")
                dist = torch.empty(max(total, 1), dtype=torch.uint8, device="cuda")
                got, ms, ms_all = best_of(lambda: ctx.search_approx_device(view, pat, k, out=out, dist_out=dist)[2],
                                          ctx.last_approx_ms)
                assert got == total
                if m == 64:
                    yard[rule] = ms
                line = {"tool": "tools/approx_long_rate.py", "what": "search", "kind": "printable95", "n": n, "m": m, "k": k,
                        "k_rule": rule, "entry": "bmx_search_approx_device" if m <= 64 else "bmx_search_approx_long_device",
                        "words": (m + 63) // 64, "kernel_words": 1 if m <= 64 else 2 if m <= 128 else 4 if m <= 256 else 8,
                        "ms": round(ms, 4), "ms_all": ms_all, "gbps": round(n / (ms * 1e-3) / 1e9, 1),
                        "over_m64": round(ms / yard[rule], 3), "ends": total}
                if total:
                    ends, dists = out[:total], dist[:total]
                    _, s_ms, s_all = best_of(lambda: ctx.approx_spans_device(view, pat, k, ends, dists)[3], ctx.last_spans_ms)
                    kept, b_ms, b_all = best_of(lambda: ctx.approx_spans_device(view, pat, k, ends, dists, best=True)[3],
                                                ctx.last_spans_ms)
                    line.update({"spans_ms": round(s_ms, 4), "spans_ms_all": s_all, "spans_ns_per_end": round(s_ms * 1e6 / total, 2),
                                 "best_kept": kept, "best_ms": round(b_ms, 4), "best_ms_all": b_all})
                emit(line)
                del out, dist
                torch.cuda.empty_cache()

    # ---- controls: the three one-word searches of the tile frame, in the shapes of their own rate tools ----
    n = n_max
    out = torch.empty(1 << 24, dtype=torch.int64, device="cuda")
    dist = torch.empty(1 << 24, dtype=torch.uint8, device="cuda")
    seed = 0x5EED6A00
    ctx.gen_text(d_text, 0, seed, 0)
    pat = corpus.stream_bytes(corpus.PATTERN_STREAM_INDEX, 48, seed, 0).tobytes()
    ctx.plant(d_text, 0, pat, [n // 3])
    torch.cuda.synchronize()
    for m, k in ((16, 2), (32, 4), (40, 4), (64, 4)):
        hits, ms, ms_all = best_of(lambda: ctx.search_approx_device(d_text, (pat + pat)[:m], k, out=out, dist_out=dist)[2],
                                   ctx.last_approx_ms)
        emit({"tool": "tools/approx_long_rate.py", "what": "control approx", "kind": "printable95", "n": n, "m": m, "k": k,
              "word": 32 if m <= 32 else 64, "ms": round(ms, 4), "ms_all": ms_all, "hits": hits})
    for m in (16, 40):
        pair = host.compile_gaps(escaped(pat[:m]))
        hits, ms, ms_all = best_of(lambda: ctx.search_gaps_device(d_text, pair, out=out)[1], ctx.last_gaps_ms)
        emit({"tool": "tools/approx_long_rate.py", "what": "control gaps literal", "kind": "printable95", "n": n, "m": m,
              "word": 32 if m <= 32 else 64, "ms": round(ms, 4), "ms_all": ms_all, "hits": hits})
        hits, ms, ms_all = best_of(lambda: ctx.search_classes_device(d_text, pair[0], out=out)[1], ctx.last_classes_ms)
        emit({"tool": "tools/approx_long_rate.py", "what": "control classes literal", "kind": "printable95", "n": n, "m": m,
              "word": 32 if m <= 32 else 64, "ms": round(ms, 4), "ms_all": ms_all, "hits": hits})

    # ---- the three times of tests/test_gpu_approx_long_speed.py ----
    n = 1 << 28
    view = d_text[:n]
    ctx.gen_text(view, 0, 0xA7710EED, 0)
    source = view[123456789 % n:123456789 % n + 128].cpu().numpy().tobytes()
    t = {}
    for m in (64, 65, 128):
        _, t[m], ms_all = best_of(lambda: ctx.search_approx_device(view, source[:m], 4, out=out, dist_out=dist)[2],
                                  ctx.last_approx_ms)
    emit({"tool": "tools/approx_long_rate.py", "what": "speed test shapes", "kind": "printable95", "n": n, "k": 4,
          "m64_ms": round(t[64], 4), "m65_ms": round(t[65], 4), "m128_ms": round(t[128], 4),
          "m65_over_m64": round(t[65] / t[64], 3), "m128_over_m64": round(t[128] / t[64], 3), "bar": 3.0})
    ctx.close()


if __name__ == "__main__":
    main()
