"""etlg_batch_iceberg beside etlg_batch_columns(INSERT | UPDATE) on HBM-resident 64 MiB batches (cfg2, cfg3), warm, device output,
alternating in one process: per call the median wall time of 20 calls (what a caller sees: both calls stop for the device equally
often) and the median time between two device events recorded on the context's stream around the call, rows, and for the changelog
call the bytes of the two CDC columns with the rate they imply for the difference between the two calls. The kernel split — k_col_cdc
alone — comes from a separate `rocprofv3 --kernel-trace --stats -- python tools/iceberg_probe.py` run.

`--tree DIR` imports the package from another checkout (built there): run against the parent commit's tree in the same job, the
medians of etlg_batch_columns there are the yardstick for the refactor of its body (a tree without etlg_batch_iceberg times that call
alone). One GPU job; every step of it under its own `timeout`."""
import json
import os
import sys
import time

TREE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--tree" in sys.argv:
    TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
sys.path.insert(0, TREE)
import etl_amd  # noqa: E402,F401
import torch  # noqa: E402

from etl_amd import abi, synth  # noqa: E402
from etl_amd.decoder import Batch, Decoder  # noqa: E402


def one(name, prime, buf, offs, reps=20, warm=3):
    st = torch.cuda.Stream()
    d = Decoder(0, stream=st.cuda_stream)              # the context's stream: the events below are recorded on it
    prime(d)
    b = d.decode(buf, offs, flags=abi.F_OUTPUT_ON_DEVICE | abi.F_NO_CONTROL)
    assert b.rc == 0, b.error
    out = {"workload": name, "batch_bytes": int(len(buf)), "tree": TREE if "--tree" in sys.argv else "."}
    calls = [("columns_iu", lambda: b.columns(0, kinds=("I", "U"), on_device=True))]
    if hasattr(Batch, "iceberg"):
        calls.append(("iceberg", lambda: b.iceberg(0, on_device=True)))
    for _, call in calls:
        for _ in range(warm):
            call().close()
    wall = {f: [] for f, _ in calls}
    dev = {f: [] for f, _ in calls}
    for _ in range(reps):
        for fmt, call in calls:
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            t0 = time.perf_counter()
            r = call()
            e1.record(st)
            torch.cuda.synchronize()
            wall[fmt].append(time.perf_counter() - t0)
            dev[fmt].append(e0.elapsed_time(e1))
            out[fmt] = {"rows": int(r.n_rows), "cols": int(r.view.n_cols)}
            if fmt == "iceberg":
                out[fmt]["host_rows"] = int(r.changelog.n_host_rows)
                out[fmt]["cdc_bytes_written"] = int(r.n_rows) * (6 + 33 + 16) + 16     # values + two offsets per row
                out[fmt]["cdc_bytes_read"] = int(r.n_rows) * (8 + 8 + 8 + 1)           # row_event, commit_lsn, tx_ordinal, kind
            r.close()
    for fmt, ts in wall.items():
        o = out[fmt]
        o["ms_median"] = round(sorted(ts)[len(ts) // 2] * 1e3, 3)
        o["ms_events_median"] = round(sorted(dev[fmt])[len(ts) // 2], 3)
        o["ms_min"] = round(min(ts) * 1e3, 3)
    if "iceberg" in out:
        diff = out["iceberg"]["ms_median"] - out["columns_iu"]["ms_median"]
        out["iceberg"]["ms_over_columns_iu"] = round(diff, 3)
        out["iceberg"]["ms_events_over_columns_iu"] = round(out["iceberg"]["ms_events_median"] - out["columns_iu"]["ms_events_median"], 3)
    b.close(); d.close()
    return out


def main():
    for mk in (synth.cfg2, synth.cfg3):
        w = mk()
        buf, offs = w.fill(64 << 20)
        print(json.dumps(one(w.name if hasattr(w, "name") else mk.__name__, w.register, buf, offs)), flush=True)


if __name__ == "__main__":
    main()
