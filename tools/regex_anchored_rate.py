"""Rate of the anchored regex search (bmx_search_regex_anchored_device), of its begins side and of both post-passes on a
synthetic text generated in HBM (bmx_gen_text_device), printable-95 with one byte value turned into the line break and the
plants of tests/test_gpu_regex_anchored_speed.py -- the measurements are that file's `measure`, so the test and the profile
cannot drift apart:

    anchored_ms, route_ms          ^(ERROR|FATAL|PANIC): [0-9]{2,4}$ through the anchored entry (HIP events around the call,
                                   best of 3) beside the unanchored search, its starts pass, the row split and the torch
                                   comparisons against the row offsets
    anchored_kernel_ms             the anchored kernel alone; plain_kernel_ms: bmx_search_regex_device's kernel on the
                                   expression without anchors; anchored_full_classes_kernel_ms: the anchored kernel on that
                                   automaton with every class full (the cost of the two extra gathers)
    words_kernel_ms                \\b(ERROR|FATAL|PANIC)\\b
    begins_kernel_ms               the anchored begins kernel beside the plain one (begins_plain_kernel_ms)
    starts_longest_ms, ends_longest_ms   both post-passes over the lowest 2^20 entries of \\<(e|th).{0,2}[a-z]

One JSON line per run.

    python tools/regex_anchored_rate.py [--gib 1] [--out F]    (no --out: stdout only; profiles/r22_regex_anchored_rate.jsonl
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

    from test_gpu_regex_anchored_speed import measure

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
