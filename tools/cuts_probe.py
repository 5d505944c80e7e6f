"""etlg_batch_cuts / etlg_cuts_locate on HBM-resident 64 MiB batches (cfg2, cfg3), warm, medians of 20 wall times after 3 warm calls:
  (a) etlg_batch_cuts, hints = NULL, device output, at the reference's default batch budget — BatchConfig::DEFAULT_MAX_BYTES = 8 MiB
      (crates/etl-config/src/shared/pipeline.rs:68; the runtime takes the smaller of it and the memory-ratio share, :42-49);
  (b) the same at a budget of 64 KiB; (c) the same at budget 1 (a cut behind every event);
      cfg3 holds partial Updates, whose hints are INCOMPLETE: with hints = NULL the walk ends at the first of them (stop_event is printed).
      The `completed` legs run (a)-(c) over a device copy of the hints with bit 63 cleared — the call's second form — to the last event;
  (d) etlg_cuts_locate for (a)'s and (b)'s cuts, in device memory, on the row_event of the batch's RowBinary object, device output;
  (e) what a caller does today on the same batch: etlg_batch_size_hints into HOST memory, then the rule as a one-thread loop over the
      array — the C below, compiled here with the system compiler into a temporary directory (bit 63 ignored: the walk to the last
      event, the twin of the `completed` legs, whose counts and carries it must equal);
  (f) the existing kernels of finish.hip: etlg_batch_size_hints to device memory on both batches, and etlg_batch_finish_cells on a freshly
      decoded type-matrix batch per call (the pass settles cells in place: a second call on the same batch has nothing to do).
`--tree DIR` imports the package from another checkout (built there): a tree without etlg_batch_cuts times (f) alone — run against the
parent commit's tree twice in the same job, the spread of its medians is the yardstick for this tree's. The output — this text as `#`
lines, then one JSON line per workload — is committed as it is printed (profiles/cuts_probe_mi355x.txt)."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

TREE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = TREE
if "--tree" in sys.argv:
    TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
sys.path.insert(0, TREE)
import etl_amd  # noqa: E402,F401
import numpy as np  # noqa: E402

EMU = os.environ.get("ETLG_SIMT_RUN") == "1"   # a rehearsal against the SIMT emulator build (tests/simt): device memory is host memory, times mean nothing
if not EMU:
    import torch  # noqa: E402

from etl_amd import abi, synth  # noqa: E402
from etl_amd.decoder import Batch, Decoder  # noqa: E402

DEFAULT_BUDGET = 8 * 1024 * 1024
HOST_C = r"""
#include <stdint.h>
/* EventBatch::push + the flush rule (apply.rs:656-657, :1932-1935) over [0, n): returns the cuts made, *carry the open batch's bytes */
uint64_t host_cuts(const uint64_t* hints, uint64_t n, uint64_t budget, uint64_t* cuts, uint64_t* carry) {
  uint64_t s = 0, k = 0;
  for (uint64_t i = 0; i < n; i++) {
    s += hints[i] & ~(1ull << 63);
    if (s >= budget) { cuts[k++] = i + 1; s = 0; }
  }
  *carry = s;
  return k;
}
"""


def build_host(tmp):
    src, lib = os.path.join(tmp, "host_cuts.c"), os.path.join(tmp, "host_cuts.so")
    open(src, "w").write(HOST_C)
    subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-shared", "-fPIC", src, "-o", lib])
    L = C.CDLL(lib)
    L.host_cuts.restype = C.c_uint64
    L.host_cuts.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    return L


def size_model():
    sys.path.insert(0, HERE)
    from oracle import size_hint as SH
    m = abi.SizeModel()
    for k, v in SH.MODEL.items():
        setattr(m, k, v)
    return m


def sync():
    if not EMU:
        torch.cuda.synchronize()


def dev_zeros(n):
    return np.zeros(n, dtype=np.int64) if EMU else torch.zeros(n, dtype=torch.int64, device="cuda")


def ptr(a):
    return a.ctypes.data if EMU else a.data_ptr()


def timed(call, reps, warm=3):
    ts, r = [], None
    for it in range(warm + reps):
        sync()
        t0 = time.perf_counter()
        r = call()
        sync()
        if it >= warm:
            ts.append(time.perf_counter() - t0)
    ts.sort()
    return {"ms_median": round(ts[len(ts) // 2] * 1e3, 4), "ms_min": round(ts[0] * 1e3, 4), "ms_max": round(ts[-1] * 1e3, 4)}, r


def hints_to_device(d, b, m, t):
    rc = d.L.etlg_batch_size_hints(d.h, b.h, C.byref(m), abi.F_OUTPUT_ON_DEVICE, C.c_void_p(ptr(t)))
    assert rc == abi.OK, rc


def wal(L, mk, reps, small):
    w = mk()
    buf, offs = w.fill((1 << 20) if small else (64 << 20))
    d = Decoder(0)
    w.register(d)
    b = d.decode(buf, offs, flags=abi.F_OUTPUT_ON_DEVICE | abi.F_NO_CONTROL)
    assert b.rc == 0, b.error
    ne, m = int(b.view().n_events), size_model()
    out = {"workload": w.name, "tree": TREE if "--tree" in sys.argv else ".", "batch_bytes": int(len(buf)), "events": ne}
    dev_hints = dev_zeros(ne + 1)
    out["f_size_hints_device"], _ = timed(lambda: hints_to_device(d, b, m, dev_hints), reps)
    if not hasattr(Batch, "cuts"):
        b.close(); d.close()
        return out
    done = dev_hints & 0x7FFFFFFFFFFFFFFF                                  # the completed copy: bit 63 cleared
    cuts_dev, rows_dev = dev_zeros(ne + 1), dev_zeros(ne + 1)
    sync()
    budgets = (("a_default_8MiB", DEFAULT_BUDGET), ("b_64KiB", 64 << 10), ("c_budget_1", 1))
    for tag, budget in budgets:
        t, r = timed(lambda: b.cuts(m, budget, cap=ne, on_device=ptr(cuts_dev)), reps)
        out[tag] = dict(t, n_cuts=int(r[1].n_cuts), stop_event=int(r[1].stop_event), carry_out=int(r[1].carry_out))
    nc = int(b.view().slots[0].n_cols)
    rb = b.rowbinary(0, [1] * nc + [0, 0], abi.CH_REPLACING_MERGE_TREE, on_device=True)
    for tag, budget in budgets:
        t, r = timed(lambda: b.cuts(None, budget, hints=ptr(done), cap=ne, on_device=ptr(cuts_dev)), reps)
        k = int(r[1].n_cuts)
        out[tag + "_completed"] = dict(t, n_cuts=k, stop_event=int(r[1].stop_event), carry_out=int(r[1].carry_out))
        if budget > 1:
            t, _ = timed(lambda: b.locate(ptr(cuts_dev), rb.view.row_event, rb.n_rows, n_cuts=k, out=ptr(rows_dev)), reps)
            out["d_locate_" + tag[2:]] = dict(t, n_cuts=k, rows=rb.n_rows)
    rb.close()
    # ---- (e) today: the hints come down, one thread adds them up
    t_down, host_hints = timed(lambda: b.size_hints(m), reps)
    host_cuts, carry = np.zeros(ne, dtype=np.uint64), C.c_uint64()
    out["e_size_hints_to_host"] = dict(t_down, bytes=8 * ne)
    for tag, budget in budgets:
        ts = []
        for it in range(2 + reps):
            t0 = time.perf_counter()
            k = L.host_cuts(host_hints.ctypes.data, ne, budget, host_cuts.ctypes.data, C.byref(carry))
            if it >= 2:
                ts.append(time.perf_counter() - t0)
        loop = round(sorted(ts)[len(ts) // 2] * 1e3, 4)
        dev = out[tag + "_completed"]
        out["e_" + tag[2:]] = {"host_loop_ms_median": loop, "download_plus_loop_ms": round(loop + t_down["ms_median"], 4),
                               "equals_device": (int(k), int(carry.value)) == (dev["n_cuts"], dev["carry_out"]),
                               "device_over_host": round(dev["ms_median"] / (loop + t_down["ms_median"]), 3)}
    b.close(); d.close()
    return out


def finish(reps, small):
    buf, offs = synth.type_matrix_stream(400 if small else 44000, mix=True)
    d = Decoder(0)
    synth.type_matrix_register(d)
    ts, st = [], None
    for it in range(3 + reps):
        b = d.decode(buf, offs, flags=abi.F_OUTPUT_ON_DEVICE | abi.F_NO_CONTROL)
        assert b.rc == 0, b.error
        sync()
        t0 = time.perf_counter()
        st = b.finish_cells()
        sync()
        if it >= 3:
            ts.append(time.perf_counter() - t0)
        b.close()
    d.close()
    ts.sort()
    return {"workload": "type_matrix", "tree": TREE if "--tree" in sys.argv else ".", "batch_bytes": int(len(buf)),
            "f_finish_cells": {"ms_median": round(ts[len(ts) // 2] * 1e3, 4), "ms_min": round(ts[0] * 1e3, 4), "ms_max": round(ts[-1] * 1e3, 4),
                               "arrays_typed": int(st.arrays_typed), "floats_settled": int(st.floats_settled)}}


def main():
    reps = int(os.environ.get("ETLG_PROBE_REPS", "20"))
    small = os.environ.get("ETLG_PROBE_SMALL") == "1"                       # a rehearsal size
    if "--tree" not in sys.argv:
        for line in __doc__.split("\n"):
            print(("# " + line).rstrip())
    with tempfile.TemporaryDirectory() as tmp:
        L = build_host(tmp)
        for mk in (synth.cfg2, synth.cfg3):
            print(json.dumps(wal(L, mk, reps, small)), flush=True)
    print(json.dumps(finish(reps, small)), flush=True)


if __name__ == "__main__":
    main()
