"""The shared kernel headers of etl_amd/csrc: one meaning per header in every translation unit, the layer cut between the value
codecs and the frame machinery, and build.py's dependency walk. Text only: no compiler, no GPU.

    python tests/test_kernel_headers.py --record    # rewrites tests/golden/kernel_headers_mm.json from the compiler's dependency lists (-MMD)
"""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from etl_amd import build  # noqa: E402

CSRC = os.path.join(ROOT, "etl_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "kernel_headers_mm.json")
FRAMES = "frames.hip.h"
HANDOFF_UNITS = ["columns.hip", "rowformats.hip", "rowformats_dl.hip", "finish.hip", "check.hip", "fingerprint.hip"]
HEADER_EXT = (".h", ".inc")


def macros_before_first_include(text):
    """Names a source #defines in front of its first #include "..." line."""
    m = re.search(r'^[ \t]*#[ \t]*include[ \t]+"', text, re.M)
    head = text[:m.start()] if m else text
    return re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)", head, re.M)


def leaked_switches(csrc, sources):
    """(source, macro, header) for every macro a source defines before its first project include and a header of `csrc` names."""
    headers = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith(HEADER_EXT)}
    out = []
    for src in sources:
        for name in macros_before_first_include(open(os.path.join(csrc, src)).read()):
            pat = re.compile(r"\b%s\b" % re.escape(name))
            out += [(src, name, h) for h, text in headers.items() if pat.search(text)]
    return out


def test_no_header_reads_a_switch_of_its_includer():
    """A header means the same in every unit: no macro that a source defines in front of its includes is named by a header. (On the
    commit before the split this reported ETLG_FLOAT_CALL, ETLG_DBG_WORD, ETLG_TSTAMP_WHO for rows.hip and cells.hip and
    ETLG_TEMPORAL_SWAR for rows.hip, in codec.hip.h / lookback.hip.h: seven hits.)"""
    assert leaked_switches(CSRC, build.SOURCES) == []


def test_handoff_units_do_not_see_the_frame_layer():
    assert os.path.exists(os.path.join(CSRC, FRAMES))
    for u in HANDOFF_UNITS:
        assert u in build.SOURCES
        assert FRAMES not in build.headers_of(u), u
    assert FRAMES in build.headers_of("kernels.hip") and FRAMES in build.headers_of("fused.hip")


def test_headers_of_matches_the_preprocessor():
    """headers_of() against what the preprocessor (-MMD) reported for every source (recorded: see the module docstring)."""
    want = json.load(open(GOLDEN))
    assert sorted(want) == sorted(build.SOURCES)
    for src in build.SOURCES:
        assert build.headers_of(src) == want[src], src
    assert set(build.DEPS) == set(build.SOURCES) | {h for v in want.values() for h in v} | {"../build.py"}


def test_codec_header_is_gone():
    assert not os.path.exists(os.path.join(CSRC, "codec.hip.h"))
    for top in ("etl_amd", "include", "tests", "tools"):
        for d, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith((".hip", ".cpp", ".h", ".inc")):
                    assert not re.search(r'#[ \t]*include[ \t]+"[^"]*codec\.hip\.h"', open(os.path.join(d, f), errors="replace").read()), f


def record():
    """The project headers (under the repository, outside the ROCm tree) in the preprocessor's dependency list of every source: the
    host pass of the HIP compile (the driver writes no dependency file for a device pass), asked of the compiler behind hipcc."""
    import tempfile
    clang = os.environ.get("CLANGXX", os.path.join(os.path.dirname(os.path.dirname(build.HIPCC)), "lib", "llvm", "bin", "clang++"))
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for src in build.SOURCES:
            dep = os.path.join(tmp, "d")
            subprocess.check_call([clang, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "--cuda-host-only", "-E", "-MMD", "-MF", dep,
                                   os.path.join(CSRC, src), "-o", os.devnull])
            deps = open(dep).read().replace("\\\n", " ").split(":", 1)[1].split()
            rel = {os.path.normpath(os.path.relpath(os.path.realpath(d), CSRC)) for d in deps if os.path.realpath(d).startswith(ROOT + os.sep)}
            out[src] = sorted(rel - {src})
    json.dump(out, open(GOLDEN, "w"), indent=1, sort_keys=True)
    open(GOLDEN, "a").write("\n")


if __name__ == "__main__":
    if "--record" in sys.argv:
        record()
