#!/usr/bin/env python3
"""Is the device code of two csrc directories the same, kernel by kernel?

    python tools/kernel_identity.py <csrc before> <csrc after> [-j JOBS]

The check behind "kernels instruction-identical" of a change that moves text
between translation units or touches host code only.  Cross-compiled, no GPU:
every .hip of either directory is compiled with its Makefile's own command
plus --cuda-device-only, and the gfx950 code objects are compared per symbol,
across all units of a side (a kernel may have moved to another unit):
  - the .text bytes of every function (kernels and what they call),
  - the 64-byte kernel descriptor outside bytes 16-23 (the entry offset, which
    depends on where the unit's other kernels lie),
  - the kernel's record in the amdhsa.kernels note: registers, LDS, scratch,
    arguments.
Prints the counts of identical, differing and missing symbols, the names of
the last two groups, and exits non-zero if either is not empty.
"""
import argparse
import glob
import os
import re
import shlex
import struct
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

LLVM = os.path.join(os.path.dirname(os.path.dirname(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))),
                    "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def run(cmd, **kw):
    out = subprocess.run(cmd, capture_output=True, text=True, **kw)
    if out.returncode:
        sys.exit(f"{' '.join(cmd)}\n{out.stdout[-2000:]}{out.stderr[-2000:]}")
    return out.stdout


def code_object(csrc, src, tmp):
    """Path of the gfx950 ELF of csrc/src."""
    stem = os.path.join(tmp, src[:-4])
    line = [l for l in run(["make", "-C", csrc, "-n", "-B", src[:-4] + ".o"]).splitlines()
            if f" -c {src} " in l][-1]
    cmd = shlex.split(line)
    # (-I tmp: the build_id.h that fft2.hip includes, where the tree has not been built)
    cmd[cmd.index("-o") + 1:] = [stem + ".out", "--cuda-device-only", "-I", tmp]
    run(cmd, cwd=csrc)
    run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
         f"--targets={TARGET}", f"--input={stem}.out", f"--output={stem}.elf"])
    return stem + ".elf"


def symbols(elf):
    """{name: (text bytes | None, masked descriptor | None, metadata record | None)}"""
    d = open(elf, "rb").read()
    shoff, = struct.unpack_from("<Q", d, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", d, 0x3A)
    sec = [struct.unpack_from("<IIQQQQIIQQ", d, shoff + i * shentsize) for i in range(shnum)]

    def cstr(table, off):
        base = sec[table][4] + off
        return d[base:d.index(b"\0", base)].decode()

    symtab = next(s for s in sec if cstr(shstrndx, s[0]) == ".symtab")
    funcs, descs = {}, {}
    for off in range(symtab[4], symtab[4] + symtab[5], 24):
        name, info, _, shndx, value, size = struct.unpack_from("<IBBHQQ", d, off)
        if not 0 < shndx < shnum or size == 0:
            continue
        name = cstr(symtab[6], name)
        at = sec[shndx][4] + value - sec[shndx][3]
        if info & 15 == 2:  # STT_FUNC
            funcs[name] = d[at:at + size]
        elif name.endswith(".kd") and size == 64:
            descs[name[:-3]] = d[at:at + 16] + d[at + 24:at + 64]
    # llvm-readelf prints the note as YAML: one "  - " item per kernel
    notes = run([os.path.join(LLVM, "llvm-readelf"), "--notes", elf])
    records = {}
    m = re.search(r"^amdhsa\.kernels:\s*\n((?:[ \t]+.*\n)*)", notes, re.M)
    for item in re.split(r"^  - ", m.group(1) if m else "", flags=re.M)[1:]:
        records[re.search(r"\.symbol:\s*'?([^'\s]+?)\.kd'?\s*$", item, re.M).group(1)] = item
    if not set(records) == set(descs) <= set(funcs):
        sys.exit(f"{elf}: descriptors, note and code name different kernels")
    return {n: (funcs.get(n), descs.get(n), records.get(n)) for n in set(funcs) | set(descs)}


def side(csrc, jobs, tmp):
    csrc = os.path.abspath(csrc)
    srcs = sorted(os.path.basename(f) for f in glob.glob(os.path.join(csrc, "*.hip")))
    os.makedirs(tmp)
    # fft2.hip includes it, host side only; the trees themselves are not written to
    with open(os.path.join(tmp, "build_id.h"), "w") as f:
        f.write('#define TIKE_BUILD_ID ""\n')
    with ThreadPoolExecutor(jobs) as pool:
        elfs = list(pool.map(lambda s: code_object(csrc, s, tmp), srcs))
    out = {}
    for src, elf in zip(srcs, elfs):
        for name, what in symbols(elf).items():
            # an inline function may be emitted by several units: then all copies must agree
            if out.setdefault(name, (src, what))[1] != what:
                sys.exit(f"{csrc}: {name} differs between {out[name][0]} and {src}")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("-j", type=int, default=4, help="compilations at a time")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        old = side(a.before, a.j, os.path.join(tmp, "a"))
        new = side(a.after, a.j, os.path.join(tmp, "b"))
    same = [n for n in old if n in new and old[n][1] == new[n][1]]
    differ = sorted(n for n in old if n in new and old[n][1] != new[n][1])
    missing = sorted(set(old) ^ set(new))
    kernels = sum(1 for n in old if old[n][1][1] is not None)
    print(f"{len(old)} symbols before ({kernels} kernels), {len(new)} after: "
          f"{len(same)} identical, {len(differ)} differing, {len(missing)} missing")
    moved = sorted({(old[n][0], new[n][0]) for n in same if old[n][0] != new[n][0]})
    for src, dst in moved:
        print(f"  {sum(1 for n in same if (old[n][0], new[n][0]) == (src, dst))} identical, "
              f"moved {src} -> {dst}")
    for n in differ:
        what = [w for w, x, y in zip(("text", "descriptor", "metadata"), old[n][1], new[n][1])
                if x != y]
        print(f"  DIFFERS ({', '.join(what)}): {n}  [{old[n][0]} / {new[n][0]}]")
    for n in missing:
        print(f"  MISSING {'after' if n in old else 'before'}: {n}  [{(old.get(n) or new[n])[0]}]")
    sys.exit(1 if differ or missing else 0)


if __name__ == "__main__":
    main()
