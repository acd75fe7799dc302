#!/usr/bin/env python3
"""Compare the GPU code objects of two builds of a library: `code_objects.py A.so B.so`.

The .hip_fatbin section of a HIP library is a row of offload bundles, one per translation unit, each with one code object
(an ELF file) per target.  Every code object of A is compared with its counterpart of B (the one with the same bytes, else
the one with the same kernel names, whatever the link order): byte for byte, and where the bytes differ section by section,
so that a difference in a note or a symbol name can be told from one in the code.  Prints one line per code object that
differs and exits 1 if any .text or .rodata section (code, kernel descriptors) does, 2 if it finds no code object in
either library (compressed bundles are not taken apart).  Needs llvm-objcopy
(ROCm's, $LLVM_OBJCOPY, or the one on PATH); runs without a GPU."""
import hashlib
import os
import shutil
import struct
import subprocess
import sys
import tempfile

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
CODE_SECTIONS = (".text", ".rodata")


def objcopy() -> str:
    for c in (os.environ.get("LLVM_OBJCOPY"), "/opt/rocm/llvm/bin/llvm-objcopy", shutil.which("llvm-objcopy")):
        if c and os.path.exists(c):
            return c
    sys.exit("llvm-objcopy not found")


def fatbin(path: str) -> bytes:
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "fatbin")
        subprocess.check_call([objcopy(), f"--dump-section=.hip_fatbin={out}", path, os.path.join(d, "copy")])
        with open(out, "rb") as f:
            return f.read()


def code_objects(blob: bytes):
    """[(bundle number, target triple, code object bytes)] of every device entry."""
    out = []
    at = blob.find(MAGIC)
    number = 0
    while at >= 0:
        (count,) = struct.unpack_from("<Q", blob, at + len(MAGIC))
        p = at + len(MAGIC) + 8
        for _ in range(count):
            off, size, tlen = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if not triple.startswith("host") and size:
                out.append((number, triple, blob[at + off:at + off + size]))
        number += 1
        at = blob.find(MAGIC, at + len(MAGIC))
    return out


def sections(elf: bytes):
    """{name: bytes} of a 64-bit little-endian ELF file."""
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", elf, 0x3A)
    heads = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    names = heads[shstrndx]
    strtab = elf[names[4]:names[4] + names[5]]
    out = {}
    for name, kind, _, _, off, size, *_ in heads:
        label = strtab[name:strtab.index(b"\0", name)].decode()
        out[label] = b"" if kind == 8 else elf[off:off + size]  # (SHT_NOBITS has no bytes)
    return out


def kernels(elf: bytes):
    """The names in the code object's dynamic string table: its kernels and their descriptors."""
    return frozenset(sections(elf).get(".dynstr", b"").split(b"\0")) - {b""}


def main(a_path: str, b_path: str) -> int:
    a, b = code_objects(fatbin(a_path)), code_objects(fatbin(b_path))
    if not a or not b:  # (e.g. compressed offload bundles, which this does not take apart: no verdict, not a pass)
        print(f"no code object found: {len(a)} in A, {len(b)} in B")
        return 2
    # a code object's counterpart: the one with the same bytes, else the one with the same kernels (the link order of
    # the translation units may differ between the builds)
    left = {}
    for _, triple, y in b:
        left.setdefault(hashlib.sha256(y).digest(), []).append((triple, y))
    rest, same = [], 0
    for n, triple, x in a:
        twins = left.get(hashlib.sha256(x).digest())
        if twins:
            twins.pop()
            same += 1
        else:
            rest.append((n, triple, x))
    others = [(t, y) for twins in left.values() for t, y in twins]
    bad = 0
    for n, triple, x in rest:
        names = kernels(x)
        match = next((i for i, (t, y) in enumerate(others) if t == triple and kernels(y) == names), None)
        if match is None:
            print(f"bundle {n} {triple}: no code object of B has the same {len(names)} names")
            bad += 1
            continue
        sx, sy = sections(x), sections(others.pop(match)[1])
        differ = sorted(s for s in set(sx) | set(sy) if sx.get(s) != sy.get(s))
        in_code = [s for s in differ if s.startswith(CODE_SECTIONS)]
        bad += bool(in_code)
        print(f"bundle {n} {triple}: sections that differ: {', '.join(differ) or 'none (layout only)'}"
              f"{'  <-- code' if in_code else ''}")
    for t, y in others:
        print(f"B has one more code object for {t} ({len(kernels(y))} names)")
        bad += 1
    digest = hashlib.sha256(b"".join(sorted(x for _, _, x in a))).hexdigest()[:16]
    print(f"{len(a)} code objects in A, {len(b)} in B, {same} byte for byte equal, {bad} with different code; "
          f"sha256 of A's, sorted: {digest}")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
