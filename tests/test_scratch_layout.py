"""The hand-off's scratch carve (etl_amd/csrc/scratch_layout.h): 64-byte aligned parts that never descend or overlap, and the blocks of
etlg_batch_cuts and etlg_batch_payload laid out as the offset chains they replaced — through a stand-alone host program built with
the address and undefined-behaviour sanitizers. No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scratch_layout_holds_the_layouts(tmp_path):
    exe = str(tmp_path / "scratch_layout_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "etl_amd", "csrc"), os.path.join(ROOT, "tests", "native", "scratch_layout_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    assert "mismatches 0" in out.stdout


def test_scratch_layout_header_stands_alone():
    """The header has no HIP include (the check above compiles it with g++ alone), and the host reaches it through host_state.h."""
    csrc = os.path.join(ROOT, "etl_amd", "csrc")
    text = open(os.path.join(csrc, "scratch_layout.h")).read()
    assert "hip" not in [w for line in text.split("\n") if line.lstrip().startswith("#") for w in line.replace("/", " ").replace("<", " ").replace("_", " ").split()]
    assert '#include "scratch_layout.h"' in open(os.path.join(csrc, "host_state.h")).read()
