"""CPU suite for the alignments (bmx_align*): the oracle (tests/align_oracle.py) on the examples of the definition and
on the properties of an edit script over 20,000 random pairs, cigar_strings, the header's constants, every argument
error that returns before any HIP call (ctx = NULL), every host-side entry check of bmx_align, count == 0, and the
kernel's pieces built for the host alone and run against a plain-table walk (tests/align_check.hip).  No device call is
made here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import align_oracle as al
from conftest import ROOT
from parallel_implementation_of_string_matching_algorithms_opencl_amd import host

CSRC = os.path.join(ROOT, "parallel_implementation_of_string_matching_algorithms_opencl_amd", "csrc")
NAMES = ("bmx_align_device", "bmx_align", "bmx_last_align_ms", "bmx_last_align_launches")
NO_POS = al.NO_POS


def test_examples_of_the_definition():
    for pat, span, want in ((b"abcd", b"abxd", "2=1X1="), (b"abcd", b"acd", "1=1I2="), (b"abcd", b"abccd", "2=1D2="),
                            (b"AAA", b"AA", "1I2="), (b"GATTACA", b"GCATGCA", "1=2X1=1X2=")):
        dist, runs = al.script(pat, span)
        assert al.cigar(runs) == want, (pat, span)
        assert dist == sum(n for n, c in runs if c != al.EQ)
    # the three BEST spans of the worked example of the spans' definition
    text, pat = b"xxabcdxxabxdxxacdxx", b"abcd"
    assert [al.cigar(al.script(pat, text[s:e + 1])[1]) for s, e in ((2, 5), (8, 11), (14, 16))] == ["4=", "2=1X1=", "1=1I2="]


def test_script_properties_on_random_pairs(port):
    rng = np.random.default_rng(0xA11C)
    n = 0
    for sigma in (2, 4, 95):
        for _ in range(6667):
            m, L = int(rng.integers(1, 17)), int(rng.integers(0, 17))
            pat = bytes((32 + rng.integers(0, sigma, m)).astype(np.uint8))
            if rng.integers(0, 2):  # a span made from the pattern by a few edits, or an unrelated one
                span = bytearray(pat)
                for _ in range(int(rng.integers(0, 4))):
                    at = int(rng.integers(0, len(span) + 1))
                    kind = int(rng.integers(0, 3))
                    if kind == 0 and at < len(span):
                        span[at] = 32 + int(rng.integers(0, sigma))
                    elif kind == 1 and at < len(span):
                        del span[at]
                    else:
                        span.insert(at, 32 + int(rng.integers(0, sigma)))
                span = bytes(span)
            else:
                span = bytes((32 + rng.integers(0, sigma, L)).astype(np.uint8))
            dist, runs = al.script(pat, span)
            assert sum(k for k, c in runs if c in (al.EQ, al.X, al.INS)) == len(pat)
            assert sum(k for k, c in runs if c in (al.EQ, al.X, al.DEL)) == len(span)
            assert sum(k for k, c in runs if c != al.EQ) == dist
            assert len(runs) <= 2 * dist + 1
            assert all(a[1] != b[1] for a, b in zip(runs, runs[1:])) and all(k >= 1 for k, _ in runs)
            assert al.apply(pat, span, runs) == span
            assert dist == port.edit_distance(pat, span), (pat, span)
            n += 1
    assert n >= 20000


def test_cigar_strings():
    op_off = np.array([0, 3, 3, 4, 6], dtype=np.uint64)
    ops = np.array([(2 << 4) | 7, (1 << 4) | 8, (1 << 4) | 7, (300 << 4) | 7, (1 << 4) | 1, (2 << 4) | 2], dtype=np.uint32)
    assert host.cigar_strings(op_off, ops) == ["2=1X1=", "", "300=", "1I2D"]
    assert host.cigar_strings(np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint32)) == []
    dist, off, words = al.align(b"xxabxdxx", [b"abcd"], [2], [5], 1)
    assert host.cigar_strings(off, words) == ["2=1X1="] and dist.tolist() == [1]


def test_header_constants_and_symbols(built):
    src = open(os.path.join(ROOT, "include", "bmx.h")).read()
    value = lambda name: int(re.search(rf"#define {name} \(?(\d+)", src).group(1))
    assert value("BMX_ALIGN_MAX_PATTERN") == host.ALIGN_MAX_PATTERN == 512
    assert value("BMX_ALIGN_MAX_K") == host.ALIGN_MAX_K == 254
    assert value("BMX_ALIGN_NONE") == host.ALIGN_NONE == host.MAP_NO_HIT == al.NONE
    assert (value("BMX_CIGAR_INS"), value("BMX_CIGAR_DEL"), value("BMX_CIGAR_EQ"), value("BMX_CIGAR_X")) == \
        (host.CIGAR_INS, host.CIGAR_DEL, host.CIGAR_EQ, host.CIGAR_X) == (al.INS, al.DEL, al.EQ, al.X) == (1, 2, 7, 8)
    assert re.search(r"#define BMX_ALIGN_WORKSPACE_BYTES \(1ull << 30\)", src) and host.ALIGN_WORKSPACE_BYTES == 1 << 30
    bound = {n for n, _, _ in host.SYMBOLS}
    L = C.CDLL(host.LIB_PATH)
    for name in NAMES:
        assert name in bound and hasattr(L, name), name
    assert host.lib().bmx_last_align_ms(None) < 0 and host.lib().bmx_last_align_launches(None) < 0


class Call:
    """The arguments of one bmx_align / bmx_align_device call over host arrays, every one replaceable."""

    def __init__(self, **kw):
        self.text = np.frombuffer(b"xxabcdxxabxdxxacdxx", dtype=np.uint8).copy()
        self.n = self.text.size
        self.base = 0
        self.blob = np.frombuffer(b"abcdabcdabcd", dtype=np.uint8).copy()
        self.pat_bytes = 12
        self.off = np.array([0, 4, 8, 12], dtype=np.uint64)
        self.pat_count = 3
        self.pid = None
        self.start = np.array([2, 8, 14], dtype=np.uint64)
        self.end = np.array([5, 11, 16], dtype=np.uint64)
        self.count = 3
        self.k = 1
        self.dist = np.zeros(3, dtype=np.uint8)
        self.op_off = np.zeros(4, dtype=np.uint64)
        self.ops = np.zeros(16, dtype=np.uint32)
        self.capacity = 16
        self.n_ops = C.c_uint64(77)
        for name, v in kw.items():
            assert hasattr(self, name)
            setattr(self, name, v)

    def args(self):
        p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
        return (p(self.text), self.n, self.base, p(self.blob), self.pat_bytes, p(self.off), self.pat_count, p(self.pid),
                p(self.start), p(self.end), self.count, self.k, p(self.dist), p(self.op_off), p(self.ops), self.capacity,
                C.byref(self.n_ops))

    def host(self):
        return host.lib().bmx_align(None, *self.args())

    def device(self):
        return host.lib().bmx_align_device(None, *self.args(), None)


def u64(*v):
    return np.array(v, dtype=np.uint64)


ARG_ERRORS = {
    "text NULL": dict(text=None), "patterns NULL": dict(blob=None), "offsets NULL": dict(off=None), "starts NULL": dict(start=None),
    "ends NULL": dict(end=None), "op_off NULL": dict(op_off=None), "ops NULL with room": dict(ops=None),
    "k < 0": dict(k=-1), "k > 254": dict(k=255), "n >= 2^40": dict(n=1 << 40),
    "pat_count neither 1 nor count": dict(pat_count=2),
}


def test_argument_errors_before_any_hip_call(built):
    for what, kw in ARG_ERRORS.items():
        assert Call(**kw).device() == host.ERR_ARG, what
        assert Call(**kw).host() == host.ERR_ARG, what
    # (with ctx = NULL the device entry has nothing to run on, and says so the same way)
    assert Call().device() == host.ERR_ARG
    # what the checks let through: NULL dist, NULL ops without room, a pid with any pat_count
    for kw in (dict(dist=None), dict(ops=None, capacity=0), dict(pid=np.zeros(3, dtype=np.uint32), pat_count=2)):
        c = Call(count=0, **kw)
        assert c.device() == host.OK and c.host() == host.OK, kw


def test_count_zero_launches_nothing(built):
    for entry in ("device", "host"):
        c = Call(count=0, text=None, blob=None, off=None, start=None, end=None, op_off=None, ops=None, dist=None)
        assert getattr(c, entry)() == host.OK and c.n_ops.value == 0, entry
        assert Call(count=0, k=255).device() == host.ERR_ARG  # (k is checked without an entry too)


ENTRY_ERRORS = {
    "pid >= pat_count": dict(pid=np.array([0, 3, 1], dtype=np.uint32)),
    "offsets decrease": dict(off=u64(0, 8, 4, 12)),
    "offsets past the blob": dict(off=u64(0, 4, 8, 13)),
    "a pattern of 0 bytes": dict(off=u64(0, 4, 4, 12)),
    "a pattern of 513 bytes": dict(blob=np.full(521, 97, dtype=np.uint8), pat_bytes=521, off=u64(0, 4, 517, 521)),
    "start below base_offset": dict(base=3),
    "end at n": dict(end=u64(5, 11, 19)),
    "end < start": dict(end=u64(5, 7, 16)),
    "start NO_POS alone": dict(start=u64(2, NO_POS, 14)),
    "end NO_POS alone": dict(end=u64(5, NO_POS, 16)),
}


def test_host_entry_checks_every_entry_on_the_host(built):
    for what, kw in ENTRY_ERRORS.items():
        assert Call(**kw).host() == host.ERR_ARG, what
    # the same call without the flaw gets past the checks (to the device, or to the lack of one), and so do a read
    # without a hit, a span too long for k and an unused pattern of any length beside a pid
    fine = (dict(), dict(start=u64(2, NO_POS, 14), end=u64(5, NO_POS, 16)), dict(end=u64(5, 18, 16)),
            dict(pid=np.zeros(3, dtype=np.uint32), off=u64(0, 4, 4, 12)))
    for kw in fine:
        assert Call(**kw).host() in (host.OK, host.ERR_NO_DEVICE), kw


def _hipcc() -> str:
    mk = open(os.path.join(CSRC, "Makefile")).read()
    return os.environ.get("HIPCC") or re.search(r"^HIPCC\s*\?=\s*(\S+)", mk, re.M).group(1)


def test_kernel_pieces_match_the_plain_table_walk(tmp_path):
    exe = str(tmp_path / "align_check")
    build = subprocess.run([_hipcc(), "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", "-I", CSRC,
                            os.path.join(ROOT, "tests", "align_check.hip"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "runs = 261" in run.stdout and "bad = 0" in run.stdout, run.stdout
