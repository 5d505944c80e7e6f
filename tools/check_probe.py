"""What ETLG_F_CHECK_CELLS costs on HBM-resident batches of the type-matrix table (31 array + 2 json columns, bench.py's wide70
shape): the batch decoded with and without the flag — synchronous calls (median wall time of `reps` warm calls, device input and
output) and an ASYNC chain of the same batch (wall time per batch) — plus k_chk_cells alone from the library's HIP events
(etlg_ctx_profile) and the bytes it has to read (the heap bytes of the checked cells + their 8-byte slots), and the same for a
table-copy batch of that table. The yardstick is the same run's flag-off decode. One GPU job; run it under its own `timeout`."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import etl_amd  # noqa: E402,F401
import torch  # noqa: E402

from etl_amd import abi, native, synth  # noqa: E402
from etl_amd.decoder import Decoder  # noqa: E402

BASE = abi.F_INPUT_ON_DEVICE | abi.F_OUTPUT_ON_DEVICE | abi.F_NO_CONTROL


def med(ts):
    return sorted(ts)[len(ts) // 2]


def checked_bytes(nrows_full_images):
    L = native.lib()
    tot = 0
    for (_, oid, _, text) in synth.TYPE_MATRIX:
        if text is not None and L.etlg_type_class_of_oid(oid) in (abi.TC_JSON, abi.TC_ARRAY):
            tot += len(text.encode()) + 8
    return tot * nrows_full_images


def wal(reps, chain):
    nrows = int(os.environ.get("CHECK_PROBE_ROWS", "44000"))
    buf, offs = synth.type_matrix_stream(nrows, mix=True)
    full_images = sum(1 for k in range(nrows) if k % 11 != 10)     # Deletes by key carry no checked cell
    tb = torch.from_numpy(buf.copy()).cuda()
    to = torch.from_numpy(offs.view("int32").copy()).cuda()
    torch.cuda.synchronize()
    out = {"workload": "type_matrix", "batch_bytes": int(len(buf)), "frames": int(len(offs) - 1), "checked_bytes": checked_bytes(full_images)}
    for name, extra in (("off", 0), ("on", abi.F_CHECK_CELLS)):
        d = Decoder(0)
        synth.type_matrix_register(d)
        ts = []
        for i in range(reps + 3):
            d.reset_stream_state()
            t0 = time.perf_counter()
            b = d.decode_device(tb.data_ptr(), tb.numel(), to.data_ptr(), len(offs) - 1, BASE | extra)
            dt = time.perf_counter() - t0
            assert b.rc == 0, b.error
            b.close()
            if i >= 3:
                ts.append(dt)
        out["sync_ms_" + name] = round(med(ts) * 1e3, 3)
        out["sync_GBps_" + name] = round(len(buf) / med(ts) / 1e9, 1)
        # ASYNC chain: `chain` batches enqueued back to back (each its own transaction set: the stream state is reset by a Commit)
        ts, enq = [], []
        for i in range(reps // 2 + 1):
            d.reset_stream_state()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            bs = [d.decode_device(tb.data_ptr(), tb.numel(), to.data_ptr(), len(offs) - 1, BASE | abi.F_ASYNC | extra) for _ in range(chain)]
            t1 = time.perf_counter()
            for b in bs:
                assert b.sync() == 0, b.error
            dt = time.perf_counter() - t0
            for b in bs:
                b.close()
            if i:
                ts.append(dt / chain)
                enq.append((t1 - t0) / chain)
        out["async_ms_per_batch_" + name] = round(med(ts) * 1e3, 3)
        out["async_enqueue_ms_per_batch_" + name] = round(med(enq) * 1e3, 3)
        out["async_GBps_" + name] = round(len(buf) / med(ts) / 1e9, 1)
        out["paths_" + name] = d.debug_paths()
        # the kernels alone, timed one at a time
        d.profile(2)
        for _ in range(5):
            d.reset_stream_state()
            b = d.decode_device(tb.data_ptr(), tb.numel(), to.data_ptr(), len(offs) - 1, BASE | extra)
            b.close()
        prof = {k: round(1000 * ms / n, 1) for k, (n, ms) in d.profile_read().items() if n}
        out["kernel_us_" + name] = prof
        d.close()
    k = out["kernel_us_on"].get("k_chk_cells")
    if k:
        out["k_chk_cells_read_GBps"] = round(out["checked_bytes"] / (k * 1e-6) / 1e9, 1)
    return out


def copy(reps):
    nrows = int(os.environ.get("CHECK_PROBE_COPY_ROWS", "44000"))

    def esc(t):
        return "\\N" if t is None else t.replace("\\", "\\\\").replace("\t", "\\t").replace("\n", "\\n")
    tail = "\t".join(esc(t) for _, _, _, t in synth.TYPE_MATRIX[1:]) + "\n"
    rows = [("%d\t" % (i + 1) + tail).encode() for i in range(nrows)]
    import numpy as np
    buf = np.frombuffer(b"".join(rows), dtype=np.uint8)
    offs = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint32)
    tb = torch.from_numpy(buf.copy()).cuda()
    to = torch.from_numpy(offs.view("int32").copy()).cuda()
    torch.cuda.synchronize()
    out = {"workload": "type_matrix_copy", "batch_bytes": int(len(buf)), "rows": nrows, "checked_bytes": checked_bytes(nrows)}
    for name, extra in (("off", 0), ("on", abi.F_CHECK_CELLS)):
        d = Decoder(0)
        d.schema_put(synth.TYPE_MATRIX_REL, 0, synth.TYPE_MATRIX_COLS, name="type_matrix")
        n = len(synth.TYPE_MATRIX_COLS)
        slot = d.table_ready(synth.TYPE_MATRIX_REL, 0, [1] * n, [1] + [0] * (n - 1))
        ts = []
        for i in range(reps + 3):
            t0 = time.perf_counter()
            b = d.copy_decode_device(slot, tb.data_ptr(), tb.numel(), to.data_ptr(), nrows, abi.F_OUTPUT_ON_DEVICE | extra)
            dt = time.perf_counter() - t0
            assert b.rc == 0, b.error
            b.close()
            if i >= 3:
                ts.append(dt)
        out["sync_ms_" + name] = round(med(ts) * 1e3, 3)
        out["sync_GBps_" + name] = round(len(buf) / med(ts) / 1e9, 1)
        d.profile(2)
        for _ in range(5):
            b = d.copy_decode_device(slot, tb.data_ptr(), tb.numel(), to.data_ptr(), nrows, abi.F_OUTPUT_ON_DEVICE | extra)
            b.close()
        out["kernel_us_" + name] = {k: round(1000 * ms / c, 1) for k, (c, ms) in d.profile_read().items() if c}
        out["copy_paths_" + name] = d.debug_copy()
        d.close()
    k = out["kernel_us_on"].get("k_chk_cells")
    if k:
        out["k_chk_cells_read_GBps"] = round(out["checked_bytes"] / (k * 1e-6) / 1e9, 1)
    return out


def main():
    reps = int(os.environ.get("CHECK_PROBE_REPS", "20"))
    print(json.dumps(wal(reps, 8)), flush=True)
    print(json.dumps(copy(reps)), flush=True)


if __name__ == "__main__":
    main()
