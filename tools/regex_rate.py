"""Regex-search rate (bmx_search_regex_device) on 4 GiB synthetic texts generated in HBM (bmx_gen_text_device):
printable-95 and ACGT, the 32- and the 64-bit kernel:

    literal    the corpus pattern as an expression without operators (16 and 40 positions, nl == 0); beside it the gapped
               and the class kernel on the same classes, in the same run, and the two ratios
    why        the four expressions of include/bmx.h's section: ATG([ACGT]{3}){2,4}(TAA|TAG|TGA),
               (ERROR|FATAL|PANIC): [0-9]{2,4}, ([0-9]{1,3}\\.){3}[0-9]{1,3}, (RGD|KGD)x{2,5}[ST]
    nlK        irregular positions in K = 1, 2, 4 and 8 bytes of the word (32 bits: 1, 2, 4): K groups (ab|a) with literal
               bytes between them, all spelt from the corpus pattern, so that the step reads K follow tables

One JSON line per (text kind, word, expression): kernel ms (HIP events, best of --iters after one warm-up call), the
whole call (host clock), TB/s of text, hits, the bytes of the word with an irregular position.  A last line per text
kind: the starts pass (bmx_regex_starts_device, device events around the call) over the lowest 2^20 ends of an
expression with a few million hits.

    python tools/regex_rate.py [--gib 4] [--iters 3] [--kinds 0,1] [--out F]    (no --out: the lines go to stdout only;
                                                                                 profiles/r18_regex_rate.jsonl is one run's)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from parallel_implementation_of_string_matching_algorithms_opencl_amd import corpus, host  # noqa: E402

WHY = ["ATG([ACGT]{3}){2,4}(TAA|TAG|TGA)", "(ERROR|FATAL|PANIC): [0-9]{2,4}", r"([0-9]{1,3}\.){3}[0-9]{1,3}", "(RGD|KGD)x{2,5}[ST]"]


def escaped(pat: bytes) -> str:
    return "".join("\\x%02x" % b for b in pat)


def nl_bytes(re_: host.Regex) -> int:
    """How many bytes of the word hold a position with a successor other than exactly the next one."""
    nl = sum(1 << i for i in range(re_.m) if re_.follow[i] and re_.follow[i] != 1 << (i + 1))
    return sum(1 for b in range(8) if (nl >> (8 * b)) & 0xFF)


def spread(pat: bytes, groups: int, positions: int) -> str:
    """`positions` positions that spell the pattern's own bytes: `groups` units of eight, (ab|a)cdefg over seven bytes
    each (the irregular positions of unit g lie in byte g of the word), then literal bytes."""
    out = []
    for g in range(groups):
        p = pat[7 * g:7 * g + 7]
        out.append("(" + escaped(p[0:2]) + "|" + escaped(p[0:1]) + ")" + escaped(p[2:7]))
    return "".join(out) + escaped(pat[7 * groups:7 * groups + positions - 8 * groups])


def expressions(pat: bytes):
    """(name, expression) for a corpus pattern of 64 bytes."""
    exprs = [("literal", escaped(pat[:16])), ("literal", escaped(pat[:40]))]
    exprs += [("why%d" % i, e) for i, e in enumerate(WHY)]
    exprs += [("nl%d" % k, spread(pat, k, 32)) for k in (1, 2, 4)]
    exprs += [("nl%d" % k, spread(pat, k, 64)) for k in (1, 2, 4, 8)]
    return exprs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--kinds", default="0,1")
    ap.add_argument("--capacity", type=int, default=1 << 24, help="ends stored per call")
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
        seed = 0x5EED2E00 + kind
        ctx.gen_text(d_text, 0, seed, kind)
        torch.cuda.synchronize()
        pat = corpus.stream_bytes(corpus.PATTERN_STREAM_INDEX, 64, seed, kind).tobytes()
        ctx.plant(d_text, 0, pat, [n // 3])  # at least one hit of the literal and the nlK expressions
        for name, expr in expressions(pat):
            re_ = host.compile_regex(expr)
            hits, ms, call_ms, all_ms = best(lambda: ctx.search_regex_device(d_text, re_, out=out)[1], ctx.last_regex_ms)
            line = {"kind": ("printable95", "acgt")[kind], "n": n, "pattern": name, "word": 64 if re_.m > 32 else 32, "m": re_.m,
                    "max_len": re_.max_len, "nl_bytes": nl_bytes(re_), "ms": round(ms, 4), "ms_all": [round(t, 4) for t in all_ms],
                    "call_ms": round(call_ms, 4), "tbps": round(n / (ms * 1e-3) / 1e12, 3), "hits": hits,
                    "stored": min(hits, args.capacity)}
            if name == "literal":
                classes = re_.class_array()
                g_hits, g_ms, _, _ = best(lambda: ctx.search_gaps_device(d_text, (classes, 0), out=out)[1], ctx.last_gaps_ms)
                c_hits, c_ms, _, _ = best(lambda: ctx.search_classes_device(d_text, classes, out=out)[1], ctx.last_classes_ms)
                assert g_hits == hits == c_hits, (g_hits, c_hits, hits)
                line.update({"gaps_ms": round(g_ms, 4), "classes_ms": round(c_ms, 4), "ratio_gaps": round(ms / g_ms, 3),
                             "ratio_classes": round(ms / c_ms, 3)})
            emit(line)
        # the starts of about 10^6 ends
        re_ = host.compile_regex("(ACG|TT).{0,2}TAC" if kind else "(e|th).{0,2}[a-z]")
        ends, total = ctx.search_regex_device(d_text, re_, out=out, capacity=1 << 20)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = []
        for longest in (False, True):
            ctx.regex_starts_device(d_text, re_, ends, longest=longest)  # warm-up
            t = []
            for _ in range(args.iters):
                ev0.record()
                starts = ctx.regex_starts_device(d_text, re_, ends, longest=longest)
                ev1.record()
                torch.cuda.synchronize()
                t.append(ev0.elapsed_time(ev1))
            assert bool((starts <= ends).all()) and bool((ends - starts < re_.max_len).all())
            times.append(round(min(t), 4))
        emit({"kind": ("printable95", "acgt")[kind], "n": n, "pattern": "starts", "m": re_.m, "hits": total,
              "list": int(ends.numel()), "starts_ms": times[0], "starts_longest_ms": times[1]})
    ctx.close()


if __name__ == "__main__":
    main()
