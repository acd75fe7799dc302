"""Dictionary-search rate (bmx_dict_search_device) against the existing route (ceil(K / 8) calls of
bmx_search_device_multi), on 4 GiB of printable-95 text generated in HBM (bmx_gen_text_device) with 10,000 planted
dictionary words, and on 1 GiB of English-like text (the recipe of tools/english_like.py: Zipf words over English
letter frequencies; the dictionary's patterns are drawn from the same letters, so the filters see prose).

One JSON line per (text, m, K): the whole call (host wall clock around the C-ABI call, best of --iters after one
warm-up call), the kernel time (HIP events), TB/s of text, the fraction of the 7.05 TB/s read rate measured on this
part (profiles/r03_hbm_read_probe.jsonl), candidates per byte (positions that passed the LDS filters), the pairs, the
host build time of the dictionary, and the multi-pattern route: measured up to --multi-max patterns, extrapolated
above from its time per call at the largest measured K (marked "multi_extrapolated").

    python tools/dict_rate.py [--gib 4] [--english-gib 1] [--ks 1,8,64,1024,16384,65536] [--ms 8-32,4] [--iters 3]
                              [--multi-max 64] [--texts p95,english] [--out F]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from parallel_implementation_of_string_matching_algorithms_opencl_amd import corpus, host  # noqa: E402

READ_TBPS = 7.05
LETTERS = np.frombuffer(b"etaoinshrdlcumwfgypbvkjxqz", dtype=np.uint8)
FREQ = np.array([12.7, 9.1, 8.2, 7.5, 7.0, 6.7, 6.3, 6.1, 6.0, 4.3, 4.0, 2.8, 2.8, 2.4, 2.4, 2.2, 2.0, 2.0, 1.9, 1.5, 1.0,
                 0.8, 0.15, 0.15, 0.1, 0.07])
FREQ = FREQ / FREQ.sum()


def english_like(n: int, rng) -> np.ndarray:
    """tools/english_like.py's text: 4,096 words with Zipf frequencies, single spaces."""
    V, LMAX = 4096, 12
    lens = np.clip(rng.poisson(4.2, V) + 1, 1, LMAX)
    lens[:64] = np.clip(rng.integers(1, 5, 64), 1, 4)
    vocab = np.full((V, LMAX + 1), 32, dtype=np.uint8)
    for w in range(V):
        vocab[w, :lens[w]] = rng.choice(LETTERS, lens[w], p=FREQ)
    zipf = 1.0 / np.arange(1, V + 1) ** 1.05
    zipf /= zipf.sum()
    block = 64 << 20
    parts, have = [], 0
    while have < n:
        ids = rng.choice(V, size=block // 5, p=zipf)
        mask = np.arange(LMAX + 1)[None, :] < (lens[ids] + 1)[:, None]
        t = vocab[ids][mask][:block]
        parts.append(t)
        have += t.size
    return np.concatenate(parts)[:n]


def patterns(rng, K: int, mspec: str, text_kind: str):
    if "-" in mspec:
        lo, hi = (int(x) for x in mspec.split("-"))
        lens = rng.integers(lo, hi + 1, K)
    else:
        lens = np.full(K, int(mspec))
    if text_kind == "p95":
        return [(rng.integers(0x20, 0x7F, int(m))).astype(np.uint8).tobytes() for m in lens]
    return [rng.choice(LETTERS, int(m), p=FREQ).tobytes() for m in lens]


def plant(d_text, pats, count: int, rng):
    import torch

    n = d_text.numel()
    starts = np.sort(rng.choice(n // 64, count, replace=False).astype(np.int64) * 64)
    which = rng.integers(0, len(pats), count)
    idx = np.concatenate([np.arange(s, s + len(pats[w]), dtype=np.int64) for s, w in zip(starts.tolist(), which.tolist())])
    val = np.concatenate([np.frombuffer(pats[w], np.uint8) for w in which.tolist()])
    d_text[torch.from_numpy(idx).to(d_text.device)] = torch.from_numpy(val).to(d_text.device)


def best_of(fn, iters: int):
    fn()  # warm-up
    walls, kerns, res = [], [], None
    for _ in range(iters):
        t0 = time.perf_counter()
        res = fn()
        walls.append((time.perf_counter() - t0) * 1e3)
        kerns.append(res[1])
    return min(walls), min(kerns), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--english-gib", type=float, default=1.0)
    ap.add_argument("--ks", default="1,8,64,1024,16384,65536")
    ap.add_argument("--ms", default="8-32,4")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--multi-max", type=int, default=64)
    ap.add_argument("--plants", type=int, default=10000)
    ap.add_argument("--texts", default="p95,english")
    ap.add_argument("--capacity", type=int, default=1 << 25)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    ctx = host.Context(0)
    sink = open(args.out, "a") if args.out else None
    out = torch.empty(args.capacity, dtype=torch.int64, device="cuda")
    pid = torch.empty(args.capacity, dtype=torch.int32, device="cuda")
    for text_kind in args.texts.split(","):
        rng = np.random.default_rng(0xD1C7 + len(text_kind))
        if text_kind == "p95":
            n = int(args.gib * corpus.GiB)
            d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
            ctx.gen_text(d_text, 0, 0x5EEDD500, 0)
        else:
            n = int(args.english_gib * corpus.GiB)
            d_text = torch.from_numpy(english_like(n, rng)).cuda()
        torch.cuda.synchronize()
        for mspec in args.ms.split(","):
            multi_per_call = None
            for K in [int(x) for x in args.ks.split(",")]:
                pats = patterns(rng, K, mspec, text_kind)
                if text_kind == "p95":
                    ctx.gen_text(d_text, 0, 0x5EEDD500, 0)  # a fresh background, then this dictionary's plants
                    plant(d_text, pats, args.plants, rng)
                    torch.cuda.synchronize()
                t0 = time.perf_counter()
                d = ctx.dictionary(pats)
                build_ms = (time.perf_counter() - t0) * 1e3

                def one():
                    _, _, total = d.search_device(d_text, out=out, pid_out=pid)
                    return total, ctx.last_dict_ms()

                wall, kern, (pairs, _) = best_of(one, args.iters)
                cand = ctx.last_dict_candidates()
                d.close()
                line = {"text": text_kind, "n": n, "m": mspec, "K": K, "pairs": pairs, "call_ms": round(wall, 4),
                        "kernel_ms": round(kern, 4), "tbps": round(n / (kern * 1e-3) / 1e12, 3),
                        "frac_of_read": round(n / (kern * 1e-3) / 1e12 / READ_TBPS, 3),
                        "cand_per_byte": float(f"{cand / n:.3g}"), "candidates": cand, "build_ms": round(build_ms, 1)}
                calls = math.ceil(K / host.MAX_MULTI)
                if K <= args.multi_max:
                    def multi():
                        total = 0
                        for c in range(calls):
                            lists = ctx.search_device_multi(d_text, pats[c * 8:(c + 1) * 8], out=out)
                            total += sum(x.numel() for x in lists)
                        return total, 0.0

                    mwall, _, (mpairs, _) = best_of(multi, args.iters)
                    assert mpairs == pairs, (mpairs, pairs)
                    multi_per_call = mwall / calls
                    line["multi_ms"] = round(mwall, 3)
                elif multi_per_call is not None:
                    line["multi_ms"] = round(multi_per_call * calls, 1)
                    line["multi_extrapolated"] = True
                if "multi_ms" in line:
                    line["speedup_vs_multi"] = round(line["multi_ms"] / wall, 2)
                print(json.dumps(line), flush=True)
                if sink:
                    sink.write(json.dumps(line) + "\n")
                    sink.flush()
        del d_text
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
