"""Batched edit-distance rate (bmx_edit_distance_batch_device) on string columns generated in HBM (bmx_gen_text_device):
1 M and 16 M pairs of 16, 32, 64 bytes and 64 against 256, ACGT and printable-95, pairwise and one against many (the
query is a[0]).  One JSON line per shape: kernel ms (HIP events, best of --iters after one warm-up call), pairs/s,
GCUPS (cells = la x lb per pair), the bytes moved (both blobs, 16 B of offsets and 4 B of result per pair) over the time
against the 8 TB/s HBM peak, and `frac_valu` against the VALU bound of DESIGN.md s9's formula

    bound_ms = pairs x walked bytes x ops_per_char / (256 CU x 128 lane-ops/clk x 2.4 GHz)

with ops_per_char the VALU instructions per walked byte counted in the kernel's ISA: pairwise 56.5 with
the 32-bit word and 116.3 with the 64-bit word (Eq built from the pattern in registers), one against many 14.4 and 30.3
(Eq from the shared table).  Beside it, on a 4,096-pair sample of the same data: the per-pair time of the single-pair
entry point looped by the caller (edit_distance_device: one launch and one host wait per pair, what a caller had before)
and of the oracle's port on one CPU core, and `speedup_vs_loop` = looped per-pair time / batched per-pair time.
The tool exits with status 1 if a pairwise 32 x 32 line has a `speedup_vs_loop` below 20: a batch call that cannot clear
one order of magnitude over the caller's loop has no reason to exist.  `--no-compare` leaves the loop and the oracle
out (for a run under a profiler, where only the batch kernel is wanted).

    python tools/ed_batch_rate.py [--pairs 1,16] [--iters 3] [--sample 4096] [--texts acgt,printable95]
                                  [--shapes 16x16,32x32,64x64,64x256] [--modes pair,one] [--no-compare] [--out F]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import oracle  # noqa: E402
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host  # noqa: E402

OPS_PER_CHAR = {("pair", 32): 56.5, ("pair", 64): 116.3, ("one", 32): 14.4, ("one", 64): 30.3}
LANE_OPS_PER_S = 256 * 128 * 2.4e9
HBM_PEAK = 8.0e12
SHAPES = ((16, 16), (32, 32), (64, 64), (64, 256))
MIN_SPEEDUP_32 = 20  # pairwise 32 x 32: batched per-pair time at least this many times below the looped one


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="1,16", help="millions (2^20) of pairs")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--sample", type=int, default=4096)
    ap.add_argument("--texts", default="acgt,printable95")
    ap.add_argument("--shapes", default=",".join(f"{la}x{lb}" for la, lb in SHAPES))
    ap.add_argument("--modes", default="pair,one")
    ap.add_argument("--no-compare", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    ctx = host.Context(0)
    port = oracle.port()
    sink = open(args.out, "a") if args.out else None
    shapes = [tuple(int(x) for x in t.split("x")) for t in args.shapes.split(",")]
    too_slow = []
    for mpairs in [int(x) for x in args.pairs.split(",")]:
        count = mpairs << 20
        out = torch.empty(count, dtype=torch.int32, device="cuda")
        idx = torch.arange(count + 1, dtype=torch.int64, device="cuda")
        for kind, kind_name in ((1, "acgt"), (0, "printable95")):
            if kind_name not in args.texts.split(","):
                continue
            for la, lb in shapes:
                d_a = torch.empty(count * la, dtype=torch.uint8, device="cuda")
                d_b = torch.empty(count * lb, dtype=torch.uint8, device="cuda")
                ctx.gen_text(d_a, 0, 0xEDBA7C00 + kind, kind)
                ctx.gen_text(d_b, 1 << 40, 0xEDBA7C00 + kind, kind)
                a_off, b_off = idx * la, idx * lb
                torch.cuda.synchronize()
                n = min(args.sample, count)
                h_a, h_b = d_a[:n * la].cpu().numpy(), d_b[:n * lb].cpu().numpy()
                for mode in args.modes.split(","):
                    a_count = count if mode == "pair" else 1
                    call = lambda: ctx.edit_distance_batch_device(d_a, a_off, d_b, b_off, count, a_count=a_count, out=out)
                    call()  # warm-up
                    times = []
                    for _ in range(args.iters):
                        call()
                        times.append(ctx.last_ed_batch_ms())
                    ms = min(times)
                    t_loop = t_cpu = None
                    if not args.no_compare:
                        got = out[:n].cpu().numpy()
                        # the caller's loop over the single-pair entry point, and the oracle on one core, on the sample
                        ctx.edit_distance_device(d_a[:la], d_b[:lb])
                        t0 = time.perf_counter()
                        loop = [ctx.edit_distance_device(d_a[(0 if mode == "one" else i) * la:][:la], d_b[i * lb:(i + 1) * lb])
                                for i in range(n)]
                        t_loop = (time.perf_counter() - t0) / n
                        t0 = time.perf_counter()
                        cpu = [port.edit_distance(h_a[(0 if mode == "one" else i) * la:][:la], h_b[i * lb:(i + 1) * lb])
                               for i in range(n)]
                        t_cpu = (time.perf_counter() - t0) / n
                        assert got.tolist() == loop == cpu, "batch, looped single-pair path and oracle disagree"
                    # both blobs, 16 B of offsets and 4 B of result per pair (one against many: one query, 8 B of offsets)
                    moved = count * (la + lb + 20) if mode == "pair" else count * (lb + 12) + la + 16
                    bound_ms = count * lb * OPS_PER_CHAR[(mode, 32 if la <= 32 else 64)] / LANE_OPS_PER_S * 1e3
                    line = {
                        "tool": "ed_batch_rate", "mode": mode, "text": kind_name, "pairs": count, "la": la, "lb": lb,
                        "kernel_ms": round(ms, 4), "pairs_per_s": round(count / (ms * 1e-3)),
                        "gcups": round(count * la * lb / (ms * 1e-3) / 1e9, 1),
                        "bytes_moved": moved, "tb_per_s": round(moved / (ms * 1e-3) / 1e12, 3),
                        "frac_hbm": round(moved / (ms * 1e-3) / HBM_PEAK, 3),
                        "valu_bound_ms": round(bound_ms, 4), "frac_valu": round(bound_ms / ms, 3),
                        "batch_ns_per_pair": round(ms * 1e6 / count, 3), "fallbacks": ctx.last_ed_batch_fallbacks(),
                    }
                    if t_loop is not None:
                        speedup = t_loop / (ms * 1e-3 / count)
                        line.update({"loop_us_per_pair": round(t_loop * 1e6, 2), "cpu_us_per_pair": round(t_cpu * 1e6, 2),
                                     "speedup_vs_loop": round(speedup)})
                        if mode == "pair" and (la, lb) == (32, 32) and speedup < MIN_SPEEDUP_32:
                            too_slow.append(line)
                    text = json.dumps(line)
                    print(text, flush=True)
                    if sink:
                        sink.write(text + "\n")
                        sink.flush()
                del d_a, d_b
    ctx.close()
    if too_slow:
        sys.exit(f"pairwise 32 x 32: speedup_vs_loop below {MIN_SPEEDUP_32}: {too_slow}")


if __name__ == "__main__":
    main()
