"""The table-copy hand-offs' kernels without a GPU: tests/test_gpu_copy_sinks.py against the SIMT emulator build (tests/simt/build.py) —
in the default lane order and with the lanes of every workgroup shuffled between rendezvous (k_rb_rows stages a workgroup's rows
through LDS with a row split over 1, 2 or 4 lanes; the columns' validity words are wave ballots). No case of the file may be skipped.
TEST INFRASTRUCTURE: the -m gpu run of the same file on an MI355X stays the gate."""
import subprocess
import sys

import pytest

from tests.test_simt_emulation import ROOT, _emu_env, simt_lib  # noqa: F401  (the emulator build, by import)


@pytest.mark.parametrize("order", [None, "shuffle"])
def test_copy_sink_kernels_on_the_emulator(simt_lib, order):  # noqa: F811
    env = _emu_env(simt_lib, 1500, order)
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_copy_sinks.py"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0, (out.stdout[-4000:], out.stderr[-2000:])
    assert " passed" in out.stdout and "skipped" not in out.stdout
