"""bench.py's other workloads, run the way the driver runs the headline one, so that a driver-side record of
them exists: the JSON line must parse, its parity flags must hold and its numbers must be sane (loose bounds far
below what profiles/ records -- a sanity check, not a performance gate).  Full BASELINE sizes (4 GiB)."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _line(*extra, cpu_baseline=False):
    """cpu_baseline: leave out --no-cpu-baseline, so that --full also runs the CPU legs and their parity checks."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "20", "--warmup", "3",
           *([] if cpu_baseline else ["--no-cpu-baseline"]), *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.parametrize("workload,alphabet,m", [("cfg3", "ACGT", 64), ("cfg3b", "printable-95", 64)])
def test_config3_line(ctx, workload, alphabet, m):
    """BASELINE config 3 (4 GiB, 64-byte pattern; ACGT: good-suffix-dominated for the reference's walker, the
    8-gram walker here) and its printable-95 twin, with --full: the whole GPU list against the CPU scan of the whole
    4 GiB text, and the host-buffer entry point's list against it."""
    line = _line("--workload", workload, "--full", cpu_baseline=True)
    assert line["parity"]["bit_exact_vs_cpu_baseline_full_text"] is True
    assert line["parity"]["host_entry_point_exact"] is True
    assert line["unit"] == "GB/s" and line["n_gpus"] == 1 and line["dtype"] == "u8"
    assert line["config"]["alphabet"] == alphabet and line["config"]["pattern_bytes"] == m
    assert line["config"]["text_bytes_total"] == 4 << 30
    assert line["parity"]["planted_offsets_exact"] is True and line["config"]["matches"] > 4000
    roof = line["roofline"]
    assert roof["bound"] == "hbm" and roof["algorithmic_bytes_per_launch"] == 4 << 30
    assert 0.2 < roof["kernel_ms"] < 3.0 and 0.3 < roof["frac"] < 1.0
    assert abs(roof["achieved"] - (4 << 30) / (roof["kernel_ms"] * 1e-3) / 1e9) < 2.0
    assert roof["kernel_ms"] <= line["ms_per_step"] * 1.05  # the kernel cannot take longer than the step around it
    print(json.dumps(line))


def test_edit_distance_line(ctx):
    """BASELINE config 5 (edit distance of two 64k ACGT strings) with --full: the distance equals the CPU oracle's."""
    line = _line("--workload", "ed64k", "--full", cpu_baseline=True)
    assert line["config"]["workload"] == "ed64k" and line["config"]["rows"] == line["config"]["cols"] == 1 << 16
    assert line["parity"]["distance_equals_cpu_oracle"] is True
    assert line["ms_per_step"] > 0
    print(json.dumps(line))


def test_dump_outputs_holds_the_last_steps_match_list(ctx, tmp_path):
    """--dump-outputs DIR: the match offsets of the last timed step as DIR/matches.npy (float64), the same from run to
    run; --steps sets the number of timed steps."""
    import numpy as np

    from parallel_implementation_of_string_matching_algorithms_opencl_amd import corpus

    outs = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        line = _line("--gib-per-gpu", "0.25", "--steps", "7", "--dump-outputs", str(d))
        assert line["steps"] == 7 and line["ms_per_step"] > 0
        outs.append(np.load(d / "matches.npy"))
    spec = corpus.scaled(corpus.CONFIGS["cfg2_4GiB_m16"], 1 << 28)
    assert outs[0].dtype == np.float64 and outs[0].size == line["config"]["matches"]
    assert np.array_equal(outs[0], spec.planted_offsets().astype(np.float64))
    assert np.array_equal(outs[0], outs[1])
