"""The table-copy hand-offs beside the calls they share kernels with, on HBM-resident batches, warm, device output, alternating in one
process: per call the median wall time of 20 calls after 3 warm ones.

  copy batches: 400 000 rows — synth.copy_rows(20000, 1) tiled as the bench's copy leg tiles it, escape-heavy and clean=True — under
    a copy of synth.COPY_COLS without the uuid column (a uuid table has no Arrow form):
    etlg_batch_ducklake_copy | etlg_batch_columns(INSERT) | etlg_batch_rowbinary | etlg_batch_protobuf
  WAL batches: the bench's cfg2 / cfg3 batches of 64 MiB: etlg_batch_columns(INSERT) | etlg_batch_rowbinary | etlg_batch_protobuf —
    the existing calls on CDC batches, whose kernels the copy arms share.

`--tree DIR` imports the package from another checkout (built there): run against the parent commit's tree, twice, in the same job, the
spread of its medians is the yardstick for this tree's. A tree without etlg_batch_ducklake_copy times the other calls alone. One GPU
job; every step of it under its own `timeout`."""
import json
import os
import sys
import time

TREE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--tree" in sys.argv:
    TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
sys.path.insert(0, TREE)
import etl_amd  # noqa: E402,F401
import numpy as np  # noqa: E402
import torch  # noqa: E402

from etl_amd import abi, synth  # noqa: E402
from etl_amd.decoder import Batch, Decoder  # noqa: E402

REPS, WARM = 20, 3
COPY_ROWS = 400_000


def timed(name, calls, extra):
    out = dict(extra, workload=name, tree=TREE if "--tree" in sys.argv else ".")
    ok = []
    for fmt, call in calls:
        try:
            for _ in range(WARM):
                call().close()
            ok.append((fmt, call))
        except Exception as e:                                           # (a batch the sink refuses: reported, not timed)
            out[fmt] = {"error": str(e)}
    calls = ok
    wall = {f: [] for f, _ in calls}
    for _ in range(REPS):
        for fmt, call in calls:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = call()
            torch.cuda.synchronize()
            wall[fmt].append(time.perf_counter() - t0)
            out[fmt] = {"rows": int(r.n_rows)}
            if hasattr(r.view, "n_bytes"):
                out[fmt]["bytes"] = int(r.view.n_bytes)
                out[fmt]["status"] = int(r.view.status)
            r.close()
    for fmt, ts in wall.items():
        out[fmt]["ms_median"] = round(sorted(ts)[len(ts) // 2] * 1e3, 3)
        out[fmt]["ms_min"] = round(min(ts) * 1e3, 3)
        out[fmt]["ms_max"] = round(max(ts) * 1e3, 3)
    return out


def row_calls(b, nc):
    flags = [1] * nc + [0, 0]                                            # every destination column Nullable(): no NULL error on any batch
    return [("columns_i", lambda: b.columns(0, on_device=True)),
            ("rowbinary", lambda: b.rowbinary(0, flags, abi.CH_REPLACING_MERGE_TREE, on_device=True)),
            ("protobuf", lambda: b.protobuf(0, on_device=True))]


def wal(mk):
    w = mk()
    buf, offs = w.fill(64 << 20)
    d = Decoder(0)
    w.register(d)
    b = d.decode(buf, offs, flags=abi.F_OUTPUT_ON_DEVICE | abi.F_NO_CONTROL)
    assert b.rc == 0, b.error
    nc = int(b.view().slots[0].n_cols)
    out = timed(w.name if hasattr(w, "name") else mk.__name__, row_calls(b, nc), {"batch_bytes": int(len(buf))})
    b.close(); d.close()
    return out


def copy(clean):
    cols = [c for c in synth.COPY_COLS if c[0] != "u"]
    drop = [c[0] for c in synth.COPY_COLS].index("u")
    base = []
    for r in synth.copy_rows(20000, 1, clean=clean):
        f = r[:-1].split(b"\t")
        del f[drop]
        base.append(b"\t".join(f) + b"\n")
    rows = base * (COPY_ROWS // len(base))
    buf = np.frombuffer(b"".join(rows), dtype=np.uint8)
    offs = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint32)
    d = Decoder(0)
    d.schema_put(42, 0, cols)
    slot = d.table_ready(42, 0, [1] * len(cols), [1] + [0] * (len(cols) - 1))
    tb = torch.from_numpy(buf.copy()).cuda()
    to = torch.from_numpy(offs.view(np.int32).copy()).cuda()
    torch.cuda.synchronize()
    b = d.copy_decode_device(slot, tb.data_ptr(), tb.numel(), to.data_ptr(), len(rows))
    assert b.rc == 0, b.error
    calls = row_calls(b, len(cols))
    if hasattr(Batch, "ducklake_copy"):
        calls.insert(0, ("ducklake_copy", lambda: b.ducklake_copy(0, on_device=True)))
    out = timed("copy_rows clean" if clean else "copy_rows escape-heavy", calls, {"batch_bytes": int(len(buf))})
    if "ducklake_copy" in out:
        out["ducklake_copy"]["ms_over_columns_i"] = round(out["ducklake_copy"]["ms_median"] - out["columns_i"]["ms_median"], 3)
    b.close(); d.close()
    return out


def main():
    for mk in (synth.cfg2, synth.cfg3):
        print(json.dumps(wal(mk)), flush=True)
    for clean in (False, True):
        print(json.dumps(copy(clean)), flush=True)


if __name__ == "__main__":
    main()
