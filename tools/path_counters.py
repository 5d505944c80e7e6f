"""Which path every batch took, for comparing two builds of the host layer: python tools/path_counters.py TOOL ROUNDS SEED [MODE]
Runs tools/TOOL.py (async_long_fuzz, copy_async_fuzz) with a clock that advances one second per look, so that the tool's "seconds"
argument is a round count and the same seed gives the same batches on any machine, and prints — summed over every Decoder the tool
closed — debug_paths(), debug_rows(), debug_copy() and the six words of etlg_ctx_debug_ring. The library is the one ETLG_LIB_PATH
names (the emulator build: ETLG_SIMT_RUN=1), else the product's. profiles/host_fold_paths.txt was made with it."""
import ctypes as C
import os
import runpy
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from etl_amd.decoder import Decoder  # noqa: E402

tool, rest = sys.argv[1], sys.argv[2:]
total = {}
ticks = [0.0]


def _tick():
    ticks[0] += 1.0
    return ticks[0]


def _closing(self, _close=Decoder.close):
    if getattr(self, "h", None):
        ring = (C.c_ulonglong * 8)()
        self.L.etlg_ctx_debug_ring(self.h, ring)
        for name, d in (("paths", self.debug_paths()), ("rows", self.debug_rows()), ("copy", self.debug_copy()),
                        ("ring", {"[%d]" % i: int(ring[i]) for i in range(6)})):
            for k, v in d.items():
                total[name + "." + k] = total.get(name + "." + k, 0) + v
    _close(self)


Decoder.close = _closing
time.time = _tick
sys.argv = [tool] + rest
try:
    runpy.run_path(os.path.join(ROOT, "tools", tool + ".py"), run_name="__main__")
except SystemExit as e:
    print("exit", e.code)
print("COUNTERS", tool, " ".join(rest), " ".join("%s=%d" % kv for kv in total.items()), flush=True)
