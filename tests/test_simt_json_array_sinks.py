"""The json[] literal walk of every hand-off without a GPU: tests/test_gpu_json_array_sinks.py against the SIMT emulator build
(tests/simt/build.py) — in the default lane order, with the lanes of every workgroup shuffled between rendezvous, and with the byte pass
forced to 1, 2 and 4 lanes per row (ETLG_RB_PARTS). TEST INFRASTRUCTURE: the -m gpu run of the same file on an MI355X stays the gate."""
import subprocess
import sys

import pytest

from tests.test_simt_emulation import ROOT, _emu_env, simt_lib  # noqa: F401  (the emulator build, by import)


@pytest.mark.parametrize("order,parts", [(None, None), ("shuffle", None), (None, "1"), (None, "2"), ("shuffle", "4")])
def test_json_array_sinks_on_the_emulator(simt_lib, order, parts):  # noqa: F811
    env = _emu_env(simt_lib, 900, order)
    env.pop("ETLG_RB_PARTS", None)
    if parts:
        env["ETLG_RB_PARTS"] = parts
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_json_array_sinks.py"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-4000:], out.stderr[-2000:])
    assert " passed" in out.stdout and "skipped" not in out.stdout
