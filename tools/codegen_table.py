#!/usr/bin/env python3
"""Per-kernel code generation figures of the HIP sources, cross-compiled for gfx950 (no GPU needed).

    python tools/codegen_table.py [--csrc DIR] [--out FILE] [source.hip ...]

Compiles every source of etl_amd/build.py (or the ones named) to assembly with the product's flags and prints, for every kernel
(.amdhsa_kernel), what the compiler reports behind its body: VGPRs, AGPRs, SGPRs, scratch bytes, LDS bytes, code bytes, occupancy.
Two runs over two checkouts (--csrc) and a `diff` of the outputs show which kernels a change touched.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from etl_amd.build import DEFS, HIPCC, OPT, SOURCES  # noqa: E402

FIELDS = [("NumVgprs", "vgpr"), ("NumAgprs", "agpr"), ("TotalNumSgprs", "sgpr"), ("ScratchSize", "scratch"), ("LDSByteSize", "lds"),
          ("codeLenInByte", "code"), ("Occupancy", "occ")]


def kernels_of(asm):
    """name -> {field: int} for every kernel of one assembly file."""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    out = {}
    cur = None
    for line in asm.split("\n"):
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m:
            cur = m.group(1)
            continue
        m = re.match(r"^\s*;\s*(\w+):?\s*=?:?\s*(\d+)", line)
        if m and cur in names:
            for key, short in FIELDS:
                if m.group(1) == key:
                    out.setdefault(cur, {})[short] = int(m.group(2))
    return out


def demangle(names):
    try:
        res = subprocess.run(["c++filt"] + list(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, res))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", default=os.path.join(ROOT, "etl_amd", "csrc"))
    ap.add_argument("--out", default="")
    ap.add_argument("sources", nargs="*")
    a = ap.parse_args()
    srcs = a.sources or [s for s in SOURCES if s.endswith(".hip")]
    lines = ["%-12s %-72s %5s %5s %5s %8s %7s %8s %4s" % ("source", "kernel", "vgpr", "agpr", "sgpr", "scratch", "lds", "code", "occ")]
    with tempfile.TemporaryDirectory() as tmp:
        def asm_of(src):
            s = os.path.join(tmp, src + ".s")
            subprocess.check_call([HIPCC, "--offload-arch=gfx950", OPT.get(src, "-O3"), "-std=c++17", "-w", "--cuda-device-only", "-S"] +
                                  DEFS.get(src, []) + [os.path.join(a.csrc, src), "-o", s])
            return open(s).read()
        with ThreadPoolExecutor(8) as ex:
            asms = list(ex.map(asm_of, srcs))
        for src, asm in zip(srcs, asms):
            ks = kernels_of(asm)
            dm = demangle(sorted(ks))
            for n in sorted(ks, key=lambda n: dm[n]):
                k = ks[n]
                short = re.sub(r"\(.*", "", dm[n]).replace("etlg::", "").replace("void ", "")
                lines.append("%-12s %-72s %5d %5d %5d %8d %7d %8d %4d" % (src, short[:72], k.get("vgpr", -1), k.get("agpr", -1), k.get("sgpr", -1),
                                                                         k.get("scratch", -1), k.get("lds", -1), k.get("code", -1), k.get("occ", -1)))
    text = "\n".join(lines) + "\n"
    if a.out:
        open(a.out, "w").write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
