"""The DuckLake plan kernels without a GPU: tests/test_gpu_ducklake_plan.py against the SIMT emulator build (tests/simt/build.py) — in
the default lane order, with the lanes of every workgroup shuffled between rendezvous (k_dlp_tiles hands wave sums and minima through LDS,
k_dlp_write carries a sum across the chunks of a loop: the file's tiles of 512 and 2 048 events have several), and with several
workgroups resident and interleaved in shuffled order (every k_dlp kernel reads what the launch before it left in global memory, and
k_dlp_members' lanes write the dense list and the groups' starts that the next launch's lanes read from other workgroups). No case of
the file may be skipped.
TEST INFRASTRUCTURE: the -m gpu run of the same file on an MI355X stays the gate."""
import subprocess
import sys

import pytest

from tests.test_simt_emulation import ROOT, _emu_env, simt_lib  # noqa: F401  (the emulator build, by import)


@pytest.mark.parametrize("order,grid", [(None, None), ("shuffle", None), (None, (3, "shuffle"))])
def test_ducklake_plan_kernels_on_the_emulator(simt_lib, order, grid):  # noqa: F811
    env = _emu_env(simt_lib, 900, order, grid=grid)
    env.pop("ETLG_DLP_TILE", None)
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_ducklake_plan.py"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-4000:], out.stderr[-2000:])
    assert " passed" in out.stdout and "skipped" not in out.stdout
