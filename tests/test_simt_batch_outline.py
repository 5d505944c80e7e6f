"""The pass-plan kernels without a GPU: tests/test_gpu_batch_outline.py against the SIMT emulator build (tests/simt/build.py) — in the
default lane order and with the lanes of every workgroup shuffled between rendezvous (k_ol_tiles claims its LDS slot table from 256 lanes over
every chunk of the tile, fills it behind a barrier and hands wave totals through LDS; k_ol_write carries two sums across the chunks of a
loop — the file's tiles of 512 to 2 048 events have several — and folds the touched bits of neighbouring lanes with shuffles). No case of the file may be skipped.
TEST INFRASTRUCTURE: the -m gpu run of the same file on an MI355X stays the gate."""
import subprocess
import sys

import pytest

from tests.test_simt_emulation import ROOT, _emu_env, simt_lib  # noqa: F401  (the emulator build, by import)


@pytest.mark.parametrize("order", [None, "shuffle"])
def test_outline_kernels_on_the_emulator(simt_lib, order):  # noqa: F811
    env = _emu_env(simt_lib, 900, order)
    env.pop("ETLG_OL_TILE", None)
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_batch_outline.py"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-4000:], out.stderr[-2000:])
    assert " passed" in out.stdout and "skipped" not in out.stdout
