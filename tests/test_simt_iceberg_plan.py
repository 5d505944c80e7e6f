"""The Iceberg plan kernels without a GPU: tests/test_gpu_iceberg_plan.py against the SIMT emulator build (tests/simt/build.py) — in
the default lane order, with the lanes of every workgroup shuffled between rendezvous, and with several workgroups resident and
interleaved in shuffled order. No case of the file may be skipped.
Through LDS: k_icp_tiles hands its waves' sums of members, other-slot events and set bits and its two minima to the workgroup's first
lane; k_icp_scan and k_icp_write carry a sum across the chunks of a loop (the tile sums of all three scans; the two event prefixes and
the word prefix — the file's tiles of 2 048 events and 1 024 words, and of 256 events and 4 words, have several chunks or are cut
short); k_icp_pass sums its windows' rows and mixed windows. k_icp_mark, k_icp_windows and k_icp_emit use none.
Through global memory, each from the launch before it: k_icp_tiles leaves the code bytes and the three rows of tile sums (tsum, fsum,
bsum) and the two minima on the header; k_icp_scan turns the sums into carries and leaves the totals (pre / fpre / bpre's last entry)
and the two windows on the header; k_icp_write leaves pre, fpre and bpre; k_icp_pass reads pre and fpre and leaves the windows' rows,
other-slot events and 0 / 1 lengths, which etlg_k_scan_lens turns into spre; k_icp_windows and k_icp_emit read those, and k_icp_emit
reads bpre and the bitmaps' edge words for the slices. On a table-copy batch k_icp_emit reads bpre alone.
TEST INFRASTRUCTURE: the -m gpu run of the same file on an MI355X stays the gate."""
import subprocess
import sys

import pytest

from tests.test_simt_emulation import ROOT, _emu_env, simt_lib  # noqa: F401  (the emulator build, by import)


@pytest.mark.parametrize("order,grid", [(None, None), ("shuffle", None), (None, (3, "shuffle"))])
def test_iceberg_plan_kernels_on_the_emulator(simt_lib, order, grid):  # noqa: F811
    env = _emu_env(simt_lib, 900, order, grid=grid)
    env.pop("ETLG_ICP_TILE", None)
    env.pop("ETLG_ICP_WORDS", None)
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_iceberg_plan.py"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-4000:], out.stderr[-2000:])
    assert " passed" in out.stdout and "skipped" not in out.stdout
