"""The batch-identity kernels without a GPU: tests/test_gpu_ducklake_identity.py against the SIMT emulator build (tests/simt/build.py) —
in the default lane order and with the lanes of every workgroup shuffled between rendezvous (k_fp_write's lanes write one event's bytes
side by side; k_fp_low, k_fp_affine and k_fp_fold hand LDS images from 256 lanes to one and back). No case of the file may be skipped.
TEST INFRASTRUCTURE: the -m gpu run of the same file on an MI355X stays the gate."""
import subprocess
import sys

import pytest

from tests.test_simt_emulation import ROOT, _emu_env, simt_lib  # noqa: F401  (the emulator build, by import)


@pytest.mark.parametrize("order", [None, "shuffle"])
def test_batch_identity_kernels_on_the_emulator(simt_lib, order):  # noqa: F811
    env = _emu_env(simt_lib, 900, order)
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_ducklake_identity.py"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-4000:], out.stderr[-2000:])
    assert " passed" in out.stdout and "skipped" not in out.stdout
