"""The BigQuery plan kernels without a GPU: tests/test_gpu_bigquery_plan.py against the SIMT emulator build (tests/simt/build.py) — in
the default lane order, with the lanes of every workgroup shuffled between rendezvous (k_bqp_tiles hands wave sums and minima through
LDS, k_bqp_write carries a sum across the chunks of a loop, k_bqp_pass sums its windows' bytes, rows and second rows: the file's tiles
of 2 048 events have several chunks), and with several workgroups resident and interleaved in shuffled order (every k_bqp kernel reads
what the launch before it left in global memory: the code bytes, the prefix, the windows' rows and offsets; k_bqp_copy reads nothing of
another workgroup). No case of the file may be skipped.
TEST INFRASTRUCTURE: the -m gpu run of the same file on an MI355X stays the gate."""
import subprocess
import sys

import pytest

from tests.test_simt_emulation import ROOT, _emu_env, simt_lib  # noqa: F401  (the emulator build, by import)


@pytest.mark.parametrize("order,grid", [(None, None), ("shuffle", None), (None, (3, "shuffle"))])
def test_bigquery_plan_kernels_on_the_emulator(simt_lib, order, grid):  # noqa: F811
    env = _emu_env(simt_lib, 900, order, grid=grid)
    env.pop("ETLG_BQP_TILE", None)
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_bigquery_plan.py"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-4000:], out.stderr[-2000:])
    assert " passed" in out.stdout and "skipped" not in out.stdout
