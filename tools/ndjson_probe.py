"""etlg_batch_ndjson on HBM-resident 64 MiB batches (cfg2, cfg3, the type-matrix table), warm, alternating with etlg_batch_protobuf on
the same batch: wall time per call (device output), rows, output bytes per row, and the write rate of the output against the HBM peak.
The kernel split comes from a separate `rocprofv3 --kernel-trace --stats -- python tools/ndjson_probe.py` run. One GPU job; every step
of it under its own `timeout`."""
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


def one(name, prime, buf, offs, names, reps=20):
    d = Decoder(0)
    prime(d)
    b = d.decode(buf, offs, flags=abi.F_OUTPUT_ON_DEVICE | abi.F_NO_CONTROL)
    assert b.rc == 0, b.error
    out = {"workload": name, "batch_bytes": int(len(buf))}
    calls = [("ndjson", lambda: b.ndjson(0, names, on_device=True)), ("protobuf", lambda: b.protobuf(0, on_device=True))]
    for fmt, call in list(calls):
        try:
            r = call(); r.close()                     # warm
        except Exception as e:                        # (the type-matrix rows carry NULL array elements: BigQuery refuses them)
            out[fmt] = {"error": str(e)}
            calls.remove((fmt, call))
    times = {f: [] for f, _ in calls}
    for _ in range(reps):
        for fmt, call in calls:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = call()
            torch.cuda.synchronize()
            times[fmt].append(time.perf_counter() - t0)
            out[fmt] = {"status": int(r.status), "rows": int(r.n_rows), "bytes": int(r.view.n_bytes)}
            r.close()
    for fmt, ts in times.items():
        ms = sorted(ts)[len(ts) // 2] * 1e3
        o = out[fmt]
        o["ms_median"] = round(ms, 3)
        o["bytes_per_row"] = round(o["bytes"] / max(o["rows"], 1), 1)
        o["out_GBps"] = round(o["bytes"] / (ms * 1e-3) / 1e9, 1)
        o["out_frac_of_hbm_peak"] = round(o["bytes"] / (ms * 1e-3) / HBM_PEAK, 4)
    b.close(); d.close()
    return out


def main():
    res = []
    for mk in (synth.cfg2, synth.cfg3):
        w = mk()
        buf, offs = w.fill(64 << 20)
        res.append(one(w.name if hasattr(w, "name") else mk.__name__, w.register, buf, offs, [c[0] for c in w.schema_cols(w.tables[0])]))
    buf, offs = synth.type_matrix_stream(44000, mix=True)
    res.append(one("type_matrix", synth.type_matrix_register, buf, offs, [c[0] for c in synth.TYPE_MATRIX_COLS]))
    for r in res:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
