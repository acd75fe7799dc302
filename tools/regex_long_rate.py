"""Rate of the regex search for up to 128 positions (bmx_search_regex_long_device) on 4 GiB synthetic texts generated in HBM
(bmx_gen_text_device), printable-95 and ACGT, each expression next to the 64-bit kernel (bmx_search_regex_device) on the
nearest expression that fits it, in the same run:

    literal    the corpus pattern as an expression without operators at 65, 96 and 128 positions (no follow table);
               beside it the 64-position literal
    why        a.{0,100}b, ATG([ACGT]{3}){2,38}(TAA|TAG|TGA), C.{2,4}C.{20,40}[LIVMFYWC].{8,16}H.{3,5}H and the ten
               keywords in front of ": [0-9]{2,4}"; beside them a.{0,62}b, the same with {2,17}, with .{20,34}, and the first
               five keywords
    nlK        irregular positions in K = 1, 4 and 16 bytes of the word: K groups (ab|a) with literal bytes between them,
               all spelt from the corpus pattern, so that the step reads K follow tables (the kernels with 4, 4 and 16
               table slots); beside them K = 1, 4 and 8 at 64 positions

One JSON line per (text kind, expression): kernel ms (HIP events, best of --iters after one warm-up call), the whole call
(host clock), TB/s of text, hits, the follow tables, and the same of the 64-bit kernel with the ratio of the two.  A last
line per text kind: the starts pass (bmx_regex_long_starts_device, device events around the call) over the lowest 2^20
ends of an expression with a few million hits.

    python tools/regex_long_rate.py [--gib 4] [--iters 3] [--kinds 0,1] [--out F]   (no --out: the lines go to stdout only;
                                                                                  profiles/r20_regex_long_rate.jsonl is one run's)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from parallel_implementation_of_string_matching_algorithms_opencl_amd import corpus, host  # noqa: E402

WORDS = ["ERROR", "FATAL", "PANIC", "WARNING", "CRITICAL", "EXCEPTION", "TIMEOUT", "REFUSED", "DENIED", "ABORTED"]
WHY = [("a.{0,100}b", "a.{0,62}b"),
       ("ATG([ACGT]{3}){2,38}(TAA|TAG|TGA)", "ATG([ACGT]{3}){2,17}(TAA|TAG|TGA)"),
       ("C.{2,4}C.{20,40}[LIVMFYWC].{8,16}H.{3,5}H", "C.{2,4}C.{20,34}[LIVMFYWC].{8,16}H.{3,5}H"),
       ("(" + "|".join(WORDS) + "): [0-9]{2,4}", "(" + "|".join(WORDS[:5]) + "): [0-9]{2,4}")]


def escaped(pat: bytes) -> str:
    return "".join("\\x%02x" % b for b in pat)


def tables(re_) -> int:
    """How many bytes of the word hold a position with a successor other than exactly the next one."""
    wide = isinstance(re_, host.RegexLong)
    follow = [re_.follow_set(i) if wide else int(re_.follow[i]) for i in range(re_.m)]
    nl = sum(1 << i for i, f in enumerate(follow) if f and f != 1 << (i + 1))
    return sum(1 for b in range(16) if (nl >> (8 * b)) & 0xFF)


def spread(pat: bytes, groups: int, positions: int) -> str:
    """`positions` positions that spell the pattern's own bytes: `groups` units of eight, (ab|a)cdefg over seven bytes
    each (the irregular positions of unit g lie in byte g of the word), then literal bytes."""
    out = []
    for g in range(groups):
        p = pat[7 * g:7 * g + 7]
        out.append("(" + escaped(p[0:2]) + "|" + escaped(p[0:1]) + ")" + escaped(p[2:7]))
    return "".join(out) + escaped(pat[7 * groups:7 * groups + positions - 8 * groups])


def expressions(pat: bytes):
    """(name, expression for the long kernel, expression for the 64-bit kernel) for a corpus pattern of 128 bytes."""
    exprs = [("literal", escaped(pat[:m]), escaped(pat[:64])) for m in (65, 96, 128)]
    exprs += [("why%d" % i, a, b) for i, (a, b) in enumerate(WHY)]
    exprs += [("nl%d" % k, spread(pat, k, 128), spread(pat, min(k, 8), 64)) for k in (1, 4, 16)]
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
        seed = 0x5EED3300 + kind
        ctx.gen_text(d_text, 0, seed, kind)
        torch.cuda.synchronize()
        pat = corpus.stream_bytes(corpus.PATTERN_STREAM_INDEX, 128, seed, kind).tobytes()
        ctx.plant(d_text, 0, pat, [n // 3])  # at least one hit of the literal and the nlK expressions
        for name, expr, expr64 in expressions(pat):
            re_ = host.compile_regex_long(expr)
            hits, ms, call_ms, all_ms = best(lambda: ctx.search_regex_long_device(d_text, re_, out=out)[1], ctx.last_regex_long_ms)
            r64 = host.compile_regex(expr64)
            hits64, ms64, _, all64 = best(lambda: ctx.search_regex_device(d_text, r64, out=out)[1], ctx.last_regex_ms)
            emit({"kind": ("printable95", "acgt")[kind], "n": n, "pattern": name, "m": re_.m, "max_len": re_.max_len,
                  "tables": tables(re_), "ms": round(ms, 4), "ms_all": [round(t, 4) for t in all_ms], "call_ms": round(call_ms, 4),
                  "tbps": round(n / (ms * 1e-3) / 1e12, 3), "hits": hits, "stored": min(hits, args.capacity), "m64": r64.m,
                  "tables64": tables(r64), "ms64": round(ms64, 4), "ms64_all": [round(t, 4) for t in all64],
                  "tbps64": round(n / (ms64 * 1e-3) / 1e12, 3), "hits64": hits64, "ratio": round(ms / ms64, 3)})
        # the starts of about 10^6 ends
        re_ = host.compile_regex_long("(ACG|TT).{0,2}TAC[ACGT]{0,60}G" if kind else "(e|th).{0,2}[a-z][ -~]{0,60}s")
        ends, total = ctx.search_regex_long_device(d_text, re_, out=out, capacity=1 << 20)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = []
        for longest in (False, True):
            ctx.regex_long_starts_device(d_text, re_, ends, longest=longest)  # warm-up
            t = []
            for _ in range(args.iters):
                ev0.record()
                starts = ctx.regex_long_starts_device(d_text, re_, ends, longest=longest)
                ev1.record()
                torch.cuda.synchronize()
                t.append(ev0.elapsed_time(ev1))
            assert bool((starts <= ends).all()) and bool((ends - starts < re_.max_len).all())
            times.append(round(min(t), 4))
        emit({"kind": ("printable95", "acgt")[kind], "n": n, "pattern": "starts", "m": re_.m, "tables": tables(re_), "hits": total,
              "list": int(ends.numel()), "starts_ms": times[0], "starts_longest_ms": times[1]})
    ctx.close()


if __name__ == "__main__":
    main()
