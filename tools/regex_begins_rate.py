"""Rate of the regex begins search (bmx_search_regex_begins_device), of the ends pass (bmx_regex_ends_device) and of the
leftmost-longest findall on a synthetic text generated in HBM (bmx_gen_text_device), printable-95 with the five plants of
tests/test_gpu_regex_begins_speed.py -- the measurements are that file's `measure`, so the test and the profile cannot
drift apart:

    begins_ms            the begins kernel on (ERROR|FATAL|PANIC): [0-9]{2,4} (HIP events around the kernel, best of 3)
    forward_ms           bmx_search_regex_device's kernel on the same text and expression
    route_ms, flip_ms    torch.flip of the text, then the forward search with the reversed automaton (events around
                         both); the flip alone
    ends_*_ms            the ends pass over the lowest 2^20 starts of (e|th).{0,2}[a-z] (events around the call)
    findall_*_ms         the whole findall_device(posix=True) beside findall_device(merge=True) (events around the call)

One JSON line per run.

    python tools/regex_begins_rate.py [--gib 1] [--out F]    (no --out: stdout only; profiles/r20_regex_begins_rate.jsonl
                                                              is one run's)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from parallel_implementation_of_string_matching_algorithms_opencl_amd import corpus, host  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch  # noqa: F401  (before the library, as everywhere in tools/: both bring a HIP runtime)

    from test_gpu_regex_begins_speed import measure

    ctx = host.Context(0)
    res, same = measure(ctx, int(args.gib * corpus.GiB), emit=lambda r: None)
    res["lists_equal"] = bool(same)
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(json.dumps(res) + "\n")
    ctx.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
