"""What the hand-off builders plan on the host alone (etl_amd/csrc/handoff_plan.h): the kinds of the columns, blocks A, B and C laid out as
the offset chains they replaced — every part at a multiple of 64, disjoint, inside the block — the lanes per row at the edges of their
thresholds, and the column words of the row formats — through a stand-alone host program built with the address and undefined-behaviour
sanitizers. No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "etl_amd", "csrc")


def test_handoff_plan_holds_the_layouts(tmp_path):
    exe = str(tmp_path / "handoff_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", CSRC, os.path.join(ROOT, "tests", "native", "handoff_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    assert "mismatches 0" in out.stdout


def test_handoff_plan_header_stands_alone():
    """The header has no HIP include and names no context (the check above compiles it with g++ alone); the host reaches it through
    host_state.h, and the two builders live in files of their own that host.cpp includes."""
    text = open(os.path.join(CSRC, "handoff_plan.h")).read()
    assert "hip" not in [w for line in text.split("\n") if line.lstrip().startswith("#") for w in line.replace("/", " ").replace("<", " ").replace("_", " ").split()]
    assert "etlg_ctx" not in "\n".join(line.split("//")[0] for line in text.split("\n"))
    assert '#include "handoff_plan.h"' in open(os.path.join(CSRC, "host_state.h")).read()
    host = open(os.path.join(CSRC, "host.cpp")).read()
    assert (host.index('#include "host_decode.inc"') < host.index('#include "host_handoff.inc"') < host.index('#include "host_handoff_columns.inc"')
            < host.index('#include "host_handoff_rows.inc"') < host.index('#include "host_orchestrate.inc"'))


def test_builder_bodies_stay_short():
    """build_columns, handoff_rows and every step of theirs: at most 80 lines from the opening brace to the closing one."""
    for name in ("host_handoff_columns.inc", "host_handoff_rows.inc"):
        lines = open(os.path.join(CSRC, name)).read().split("\n")
        start = None
        for i, line in enumerate(lines):
            opens = line.rstrip().endswith("{") and "(" in line and not line.lstrip().startswith(("//", "if", "for", "else", "struct", "namespace", "extern"))
            if start is None and opens and len(line) - len(line.lstrip()) <= 2:
                start, indent = i, len(line) - len(line.lstrip())
            elif start is not None and line.startswith(" " * indent + "}") and len(line) - len(line.lstrip()) == indent:
                assert i - start + 1 <= 80, (name, lines[start].strip()[:60], i - start + 1)
                start = None
