"""Builds the native pieces in-tree (no JIT cache): libetl_gfx950.so (HIP kernels
+ C ABI, cross-compiled for gfx950 with hipcc — works without a GPU) and
libetlg_synth.so (synthetic WAL generator, plain g++)."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libetl_gfx950.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# in the order they are started: the sources that take longest to compile first (the row formats and the Arrow columns instantiate
# json_display many times), so that a build takes about as long as its longest source
SOURCES = ["rowformats.hip", "rowformats_dl.hip", "columns.hip", "kernels.hip", "finish.hip", "host.cpp", "cells.hip", "fused.hip", "rows.hip", "plan.hip", "scan.hip",
           "copy.hip", "check.hip", "fingerprint.hip"]
# per-source optimisation level: k_fused is measurably faster built for size (88 vs 93 us on cfg2, tools/variants.sh);
# k_cells and the rest are not
# (round 6: so is k_copy_cells — cells.hip at -Os 468 / 304 us against 482-486 / 313-317 on the two table-copy workloads, same box;
# -O2, -fno-unroll-loops and the scheduler strategies move nothing on rows.hip / plan.hip: profiles/r06zv_compile_flag_sweep.txt)
OPT = {"fused.hip": "-Os", "cells.hip": "-Os"}
DEFS = {}   # no per-source feature flags: one code path per kernel
_INCLUDE = re.compile(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', re.M)


def headers_of(src):
    """The project headers a source includes, directly or through other headers (its .inc parts too): the #include "..." lines followed
    from the file that names them, as paths relative to csrc. No compiler runs; an include inside an #if counts whether it is taken or not."""
    seen, todo = [], [src]
    while todo:
        cur = todo.pop()
        for inc in _INCLUDE.findall(open(os.path.join(CSRC, cur)).read()):
            rel = os.path.normpath(os.path.join(os.path.dirname(cur), inc))
            if rel not in seen and rel != src:
                seen.append(rel)
                todo.append(rel)
    return sorted(seen)


# the library as a whole: every source and the union of their headers
DEPS = SOURCES + sorted({h for s in SOURCES for h in headers_of(s)}) + ["../build.py"]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build_native(force=False, verbose=False):
    deps = [os.path.join(CSRC, d) for d in DEPS]
    if not force and not _stale(LIB, deps):
        return LIB
    objs = [os.path.join(CSRC, os.path.splitext(src)[0] + ".o") for src in SOURCES]

    def compile_one(src):
        obj = os.path.join(CSRC, os.path.splitext(src)[0] + ".o")
        # an object is stale against its own source, the headers that source includes, and this file
        if force or _stale(obj, [os.path.join(CSRC, d) for d in [src] + headers_of(src) + ["../build.py"]]):
            cmd = [HIPCC, "--offload-arch=gfx950", OPT.get(src, "-O3"), "-std=c++17", "-fPIC", "-Wall",
                   "-Wno-unused-function"] + DEFS.get(src, []) + ["-c", os.path.join(CSRC, src), "-o", obj]
            if src.endswith(".cpp"):
                cmd[1:1] = ["-x", "hip"]
            if verbose:
                print(" ".join(cmd))
            subprocess.check_call(cmd)

    # the sources are independent translation units: compiled side by side in the order of SOURCES (longest first), so that the build
    # takes as long as its longest source instead of the sum of all
    jobs = max(1, min(len(SOURCES), int(os.environ.get("MAX_JOBS", "0") or 0) or (os.cpu_count() or 1), 16))
    with ThreadPoolExecutor(jobs) as ex:
        list(ex.map(compile_one, SOURCES))
    cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return LIB


def build_all(force=False, verbose=False):
    from . import synth
    build_native(force=force, verbose=verbose)
    synth.build(force=force)
    return LIB


if __name__ == "__main__":
    build_all(force="--force" in os.sys.argv, verbose=True)
