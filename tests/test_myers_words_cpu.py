"""The multi-word Myers column (csrc/bmx_myers_words.h) on the CPU: tests/myers_words_check.hip is compiled for the host
alone with the compiler the Makefile uses and run; it steps the column over random texts and compares the score with
the plain edit table after every column, in the search and in the global form, for 2, 4 and 8 words at every word
boundary.  No GPU and no device call."""
import os
import re
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "parallel_implementation_of_string_matching_algorithms_opencl_amd", "csrc")


def _hipcc() -> str:
    mk = open(os.path.join(CSRC, "Makefile")).read()
    return os.environ.get("HIPCC") or re.search(r"^HIPCC\s*\?=\s*(\S+)", mk, re.M).group(1)


def test_column_matches_the_edit_table(tmp_path):
    exe = str(tmp_path / "myers_words_check")
    build = subprocess.run([_hipcc(), "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", "-I", CSRC,
                            os.path.join(ROOT, "tests", "myers_words_check.hip"), "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "runs = 160" in run.stdout and "bad = 0" in run.stdout, run.stdout
