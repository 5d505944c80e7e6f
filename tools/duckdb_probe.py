"""etlg_batch_duckdb on HBM-resident 64 MiB batches (cfg2, cfg3, the type-matrix table, and cfg3's table with every Update leaving
one TEXT column unchanged: the workload of ETLG_DL_UPDATES), warm, the three `what` values alternating with
etlg_batch_ndjson on the same batch in the same process (the yardstick: same kernels, similar bytes out): per call the median wall time
(device output; the call synchronises its stream three times inside — row count, sizes, end — so wall time is what a caller sees) and
the median time between two device events recorded on the CONTEXT'S stream around the call (the context is given a torch stream of
its own, so the events sit in the same queue as the call's kernels and copies; the host waits inside the call are part of that span
too), rows, output bytes per row, the write rate of the output against the HBM peak, and the ratio to NDJSON (of the wall medians). The kernel split comes from a separate
`rocprofv3 --kernel-trace --stats -- python tools/duckdb_probe.py` run. One GPU job; every step of it under its own `timeout`."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import etl_amd  # noqa: E402,F401
import torch  # noqa: E402

from etl_amd import abi, synth  # noqa: E402
from etl_amd.decoder import Decoder  # noqa: E402

HBM_PEAK = 8.0e12


def one(name, prime, buf, offs, names, reps=20, warm=3):
    st = torch.cuda.Stream()
    d = Decoder(0, stream=st.cuda_stream)              # the context's stream: the events below are recorded on it
    prime(d)
    b = d.decode(buf, offs, flags=abi.F_OUTPUT_ON_DEVICE | abi.F_NO_CONTROL)
    assert b.rc == 0, b.error
    out = {"workload": name, "batch_bytes": int(len(buf))}
    calls = [("tuples", lambda: b.duckdb(0, names, what=abi.DL_TUPLES, on_device=True)),
             ("predicates", lambda: b.duckdb(0, names, what=abi.DL_PREDICATES, on_device=True)),
             ("updates", lambda: b.duckdb(0, names, what=abi.DL_UPDATES, on_device=True)),
             ("ndjson", lambda: b.ndjson(0, names, on_device=True))]
    for fmt, call in list(calls):
        try:
            for _ in range(warm):
                r = call(); r.close()
        except Exception as e:
            out[fmt] = {"error": str(e)}
            calls.remove((fmt, call))
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
            out[fmt] = {"status": int(r.status), "rows": int(r.n_rows), "host_rows": int(r.view.n_host_rows), "bytes": int(r.view.n_bytes)}
            r.close()
    for fmt, ts in wall.items():
        ms = sorted(ts)[len(ts) // 2] * 1e3
        o = out[fmt]
        o["ms_median"] = round(ms, 3)
        o["ms_events_median"] = round(sorted(dev[fmt])[len(ts) // 2], 3)
        o["ms_min"] = round(min(ts) * 1e3, 3)
        o["bytes_per_row"] = round(o["bytes"] / max(o["rows"], 1), 1)
        o["out_GBps"] = round(o["bytes"] / (ms * 1e-3) / 1e9, 1)
        o["out_frac_of_hbm_peak"] = round(o["bytes"] / (ms * 1e-3) / HBM_PEAK, 4)
    if "ms_median" in out.get("ndjson", {}):
        for fmt in ("tuples", "predicates", "updates"):
            if "ms_median" in out.get(fmt, {}):
                out[fmt]["ratio_to_ndjson"] = round(out[fmt]["ms_median"] / out["ndjson"]["ms_median"], 2)
    b.close(); d.close()
    return out


def cfg3_toast_updates():
    """cfg3's table and mix, every Update without an old image and with 'u' on one TEXT column: partial Updates only."""
    return synth.Workload([synth.table_mixed()], 0xE710003, rows_per_txn=500, mix=(60, 30, 10), upd_key=0, upd_toast=100, name="cfg3_toast_updates")


def main():
    res = []
    for mk in (synth.cfg2, synth.cfg3, cfg3_toast_updates):
        w = mk()
        buf, offs = w.fill(64 << 20)
        res.append(one(w.name if hasattr(w, "name") else mk.__name__, w.register, buf, offs, [c[0] for c in w.schema_cols(w.tables[0])]))
    buf, offs = synth.type_matrix_stream(44000, mix=True)
    res.append(one("type_matrix", synth.type_matrix_register, buf, offs, [c[0] for c in synth.TYPE_MATRIX_COLS]))
    for r in res:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
