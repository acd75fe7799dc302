"""Seeded inputs of the tests that compare against the reference build, and what the reference build answered.

Those tests used to skip wherever oracle/_ref/libbmref.so had not been built (it needs the reference's sources).
Their inputs are generated here, once, for the tests and for the recording; the reference build's answers are kept
in reference_runs.json beside this file: distances as they are, offset lists, shift tables and suffix arrays as
"<size>:<first 16 hex digits of their SHA-256>".  The tests compare with the reference build when it is present
and with these recorded answers always.

Re-record (needs the reference build, see oracle/Makefile):

    python tests/golden/reference_runs.py
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PATH = os.path.join(HERE, "reference_runs.json")


def digest(*arrays) -> str:
    """Size and SHA-256 prefix of arrays as stored by the oracles (offsets uint64, tables / suffix arrays int32)."""
    h = hashlib.sha256()
    size = 0
    for a in arrays:
        a = np.ascontiguousarray(a)
        size += a.size
        h.update(a.tobytes())
    return f"{size}:{h.hexdigest()[:16]}"


def load(name: str):
    with open(PATH) as f:
        return json.load(f)[name]


# ---- inputs (the seeds and shapes the tests always used) ------------------------------------------------------
def table_patterns():
    """tests/test_abi_and_tables.py::test_build_tables_matches_reference_build"""
    rng = np.random.default_rng(100)
    for _ in range(2000):
        alpha = int(rng.integers(1, 4))
        m = int(rng.integers(1, 100))
        yield (rng.integers(0, alpha, m) + 97).astype(np.uint8).tobytes()


def search_cases():
    """tests/test_oracle_golden.py::test_port_equals_reference_build_random"""
    rng = np.random.default_rng(123)
    for _ in range(3000):
        alpha = int(rng.integers(1, 5))
        m = int(rng.integers(1, 13))
        n = int(rng.integers(1, 201))
        text = (rng.integers(0, alpha, n) + 97).astype(np.uint8)
        pat = (rng.integers(0, alpha, m) + 97).astype(np.uint8).tobytes()
        yield text, pat


def config_cases(n):
    """The reduced configs 2 and 3 at n bytes: (text, pattern)."""
    from parallel_implementation_of_string_matching_algorithms_opencl_amd import corpus

    for name in ("cfg2_4GiB_m16", "cfg3_4GiB_m64_acgt"):
        spec = corpus.scaled(corpus.CONFIGS[name], n)
        yield spec.host_text(), spec.pattern()


def edit_distance_pairs():
    """tests/test_edit_distance.py::test_oracle_equals_reference_build_random"""
    rng = np.random.default_rng(42)
    for _ in range(200):
        la, lb = int(rng.integers(0, 700)), int(rng.integers(0, 700))
        al = int(rng.integers(1, 6))
        x = (rng.integers(0, al, la) + 97).astype(np.uint8)
        y = (rng.integers(0, al, lb) + 97).astype(np.uint8)
        yield x, y


def suffix_array_texts():
    """tests/test_suffix_array.py::test_oracle_equals_reference_build_random"""
    rng = np.random.default_rng(21)
    for _ in range(200):
        n = int(rng.integers(1, 500))
        yield (rng.integers(0, int(rng.integers(1, 27)), n) + 97).astype(np.uint8)


def three_way_cases():
    """tests/test_gpu_parity.py::test_three_way_on_the_gpu_box_hip_port_and_reference_build (random part)"""
    rng = np.random.default_rng(4242)
    for _ in range(60):
        alpha = int(rng.choice([2, 4, 20, 95]))
        n = int(rng.integers(1, 400_000))
        m = int(rng.integers(1, 99))
        text = (rng.integers(0, alpha, n) + 32).astype(np.uint8)
        if n > m and rng.random() < 0.8:
            a = int(rng.integers(0, n - m))
            pat = text[a:a + m].copy()
            for p in rng.integers(0, n - m, 5):
                text[p:p + m] = pat
        else:
            pat = (rng.integers(0, alpha, m) + 32).astype(np.uint8)
        yield text, pat.tobytes()


# ---- recording ------------------------------------------------------------------------------------------------
def record(ref) -> dict:
    def tables(pat):
        bad, good = ref.tables(pat)
        return digest(bad, good[1:])  # good[0] is unset in the reference

    return {
        "source": "oracle/_ref/libbmref.so (the reference's own code), reference_runs.py",
        "tables": [tables(p) for p in table_patterns()],
        "search": [digest(ref.search(t, p)) + " " + tables(p) for t, p in search_cases()],
        "search_configs_5MiB": [digest(ref.search(t, p)) for t, p in config_cases(5 * (1 << 20) + 3)],
        "edit_distance": [ref.edit_distance(x, y) for x, y in edit_distance_pairs()],
        "suffix_array": [digest(ref.suffix_array(x)) for x in suffix_array_texts()],
        "three_way": [digest(ref.search(t, p)) for t, p in three_way_cases()],
        "three_way_configs_6MiB": [digest(ref.search(t, p)) for t, p in config_cases(6 * (1 << 20) + 13)],
    }


def main():
    sys.path.insert(0, ROOT)
    import oracle

    oracle.build(want_ref=True)
    ref = oracle.reference()
    assert ref is not None, "reference build missing (oracle/_ref/libbmref.so)"
    with open(PATH, "w") as f:
        json.dump(record(ref), f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
