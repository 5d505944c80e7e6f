"""The shared prologue of the synchronous entry points without a GPU: tests/test_gpu_entry_prologue.py against the SIMT emulator build
(tests/simt/build.py), with immediate streams and with enqueued work running as late as the HIP ordering rules allow (a copy of the
input that the classify kernel is not ordered behind shows there). TEST INFRASTRUCTURE: the -m gpu run on an MI355X stays the gate."""
import subprocess
import sys

import pytest

from tests.test_simt_emulation import ROOT, _emu_env, simt_lib  # noqa: F401  (the emulator build, by import)


@pytest.mark.parametrize("streams", [None, "lazy"])
def test_entry_prologue_on_the_emulator(simt_lib, streams):  # noqa: F811
    env = _emu_env(simt_lib, 300, streams=streams)
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_entry_prologue.py"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-4000:], out.stderr[-2000:])
    assert " passed" in out.stdout and "skipped" not in out.stdout
