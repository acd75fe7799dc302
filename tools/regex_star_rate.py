"""Rates of the regular-expression search with unbounded repetition (bmx_search_regex_star_device) on synthetic texts
generated in HBM (bmx_gen_text_device), through libbmx_exp.so for the phase times and the warm-up knob:

    pair      (ERROR|FATAL|PANIC): [0-9]+ on the new kernel beside (ERROR|FATAL|PANIC): [0-9]{1,8} on the star-free one, 1 GiB
              of printable-95 text with a planted corpus, the same hits: both kernel times and their ratio -- the cost of
              the pair warm-up, which tests/test_gpu_regex_star_speed.py bounds; and the same with the warm-up forced to
              64, 128, 256 and 512 bytes (the reason for the rule "a sixteenth of the piece")
    slow      ERROR.*timeout on 1 and 4 GiB of printable-95 text without ERROR: every lane tainted, one chain as long as the
              text; the first launch, R1, the sweep and R2 separately
    numbers   [0-9]+\\.[0-9]+ on 4 GiB of printable-95 and of ACGT text

One JSON line each: kernel ms (best of --iters after one warm-up call), what the call did.

    python tools/regex_star_rate.py [--iters 3] [--big-gib 4] [--out F]     (profiles/r19_regex_star_rate.jsonl is one run's)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from parallel_implementation_of_string_matching_algorithms_opencl_amd import corpus, host  # noqa: E402

STAR = "(ERROR|FATAL|PANIC): [0-9]+"
FREE = "(ERROR|FATAL|PANIC): [0-9]{1,8}"
PLANTS = [b"ERROR: 7", b"FATAL: 12345678", b"PANIC: 42", b"ERROR: 0001", b"FATAL: 9"]


def plant_corpus(ctx, d_text, n):
    import torch

    for i, p in enumerate(PLANTS):
        at = 1000 + i * (n // 7)
        d_text[at:at + len(p) + 1] = torch.frombuffer(bytearray(p + b" "), dtype=torch.uint8).to(d_text.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--big-gib", type=float, default=4.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    ctx = host.Context(0, library=host.exp_lib())
    sink = open(args.out, "a") if args.out else None

    def emit(line):
        print(json.dumps(line), flush=True)
        if sink:
            sink.write(json.dumps(line) + "\n")
            sink.flush()

    def best(call, last_ms):
        hits = call()  # warm-up
        ms = []
        for _ in range(args.iters):
            assert call() == hits
            ms.append(last_ms())
        return hits, min(ms), ms

    out = torch.empty(1 << 24, dtype=torch.int64, device="cuda")
    sizes = [corpus.GiB] + ([int(args.big_gib * corpus.GiB)] if args.big_gib > 1 else [])
    for n in sizes:
        d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
        ctx.gen_text(d_text, 0, 0x57A25EED, 0)
        slow = host.compile_regex_star("ERROR.*timeout")
        hits, ms, _ = best(lambda: ctx.search_regex_star_device(d_text, slow, out=out)[1], ctx.last_regex_star_ms)
        last = ctx.regex_star_last()
        emit({"what": "slow", "n": n, "expr": "ERROR.*timeout", "hits": hits, "ms": round(ms, 3), **last})
        if n == corpus.GiB:
            plant_corpus(ctx, d_text, n)
            free, star = host.compile_regex(FREE), host.compile_regex_star(STAR)
            h0, ms0, all0 = best(lambda: ctx.search_regex_device(d_text, free, out=out)[1], ctx.last_regex_ms)
            for warm in (0, 64, 128, 256, 512):
                ctx.set_knob("regex_star_warm", warm)
                h1, ms1, all1 = best(lambda: ctx.search_regex_star_device(d_text, star, out=out)[1], ctx.last_regex_star_ms)
                last = ctx.regex_star_last()
                assert h1 == h0 and last["tainted"] == 0 and last["slow"] == 0, (h0, h1, last)
                emit({"what": "pair", "n": n, "star": STAR, "free": FREE, "hits": h1, "warm_knob": warm, "warm": last["warm"],
                      "piece_shift": last["piece_shift"], "star_ms": round(ms1, 4), "free_ms": round(ms0, 4),
                      "ratio": round(ms1 / ms0, 3), "star_ms_all": [round(t, 4) for t in all1], "free_ms_all": [round(t, 4) for t in all0]})
            ctx.set_knob("regex_star_warm", 0)
        if n != corpus.GiB:
            for kind in (0, 1):
                if kind:
                    ctx.gen_text(d_text, 0, 0x57A25EED + kind, kind)
                num = host.compile_regex_star(r"[0-9]+\.[0-9]+")
                hits, ms, _ = best(lambda: ctx.search_regex_star_device(d_text, num, out=out)[1], ctx.last_regex_star_ms)
                last = ctx.regex_star_last()
                emit({"what": "numbers", "kind": ("printable95", "acgt")[kind], "n": n, "expr": r"[0-9]+\.[0-9]+", "hits": hits,
                      "ms": round(ms, 4), "tbps": round(n / (ms * 1e-3) / 1e12, 3), **last})
        del d_text
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
