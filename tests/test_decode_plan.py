"""What the decode decides on the host alone (etl_amd/csrc/decode_plan.h): the fixed-width plan's launch geometry, the generic kernel
choice, k_rows' tile choice, the staging window of k_fused / k_cells / k_copy_cells, the side set's layout, the plan's summary, the chained
scan's bound and the output capacities — each against the expression it replaced, over a grid that crosses their thresholds, through a
stand-alone host program built with the address and undefined-behaviour sanitizers. And the shape of the decode's host files. No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "etl_amd", "csrc")
DECODE_FILES = ("host_decode.inc", "host_orchestrate.inc")


def test_decode_plan_holds_the_old_figures(tmp_path):
    exe = str(tmp_path / "decode_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", CSRC, os.path.join(ROOT, "tests", "native", "decode_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    assert "mismatches 0" in out.stdout


def test_decode_plan_header_stands_alone():
    """The header has no HIP include and names no context (the check above compiles it with g++ alone); the host reaches it through
    host_state.h, and etlg_decode with its chain lives in a file of its own that host.cpp includes in front of the batch calls, the
    hand-off files and the orchestration."""
    text = open(os.path.join(CSRC, "decode_plan.h")).read()
    assert "hip" not in [w for line in text.split("\n") if line.lstrip().startswith("#") for w in line.replace("/", " ").replace("<", " ").replace("_", " ").split()]
    code = "\n".join(line.split("//")[0] for line in text.split("\n"))
    assert "etlg_ctx" not in code and "etlg_batch" not in code
    assert '#include "decode_plan.h"' in open(os.path.join(CSRC, "host_state.h")).read()
    host = open(os.path.join(CSRC, "host.cpp")).read()
    assert host.index('#include "host_control.inc"') < host.index('#include "host_decode.inc"') < host.index('#include "host_handoff.inc"') < host.index('#include "host_orchestrate.inc"')
    for name in ("etlg_decode", "etlg_copy_decode", "flush_deferred", "choose_decode_stream", "take_ring_slot", "decode_tail"):
        assert f" {name}(etlg_ctx* c" in open(os.path.join(CSRC, "host_decode.inc")).read(), name


def test_decode_bodies_stay_short():
    """etlg_decode, decode_tail, build_side_inputs, enqueue_single and every step of theirs — every function of the decode's host files: at
    most 80 lines from the opening brace to the closing one, the limit the hand-off builders keep (tests/test_handoff_plan.py)."""
    seen = 0
    for name in DECODE_FILES:
        lines = open(os.path.join(CSRC, name)).read().split("\n")
        start = None
        for i, line in enumerate(lines):
            head = line.split("  //")[0].rstrip()   # (a step may carry a remark behind its opening brace)
            opens = head.endswith("{") and "(" in head and not line.lstrip().startswith(("//", "if", "for", "else", "struct", "namespace", "extern", "while", "switch"))
            if start is None and opens and len(line) - len(line.lstrip()) <= 2:
                start, indent = i, len(line) - len(line.lstrip())
            elif start is not None and line.startswith(" " * indent + "}") and len(line) - len(line.lstrip()) == indent:
                assert i - start + 1 <= 80, (name, lines[start].strip()[:60], i - start + 1)
                seen += 1
                start = None
    assert seen >= 60   # (the walk found the functions: the two files hold about a hundred)
