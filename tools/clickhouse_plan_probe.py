"""etlg_clickhouse_plan on HBM-resident batches, warm, medians of 20 wall times after 3 warm calls: 64 MiB of cfg2 and cfg3 and the
three-table cfg5 stream, slot 0, the etlg_batch_rowbinary object (every destination column Nullable()), the passes and the outputs on
the device. Per workload and engine (MergeTree, ReplacingMergeTree: the rows' lengths differ by the CDC columns, and so may a refusal):
  windows  (a) one window over the whole batch; (b) the passes etlg_batch_outline writes for the ranges of etlg_batch_cuts at the
           reference's default budget, BatchConfig::DEFAULT_MAX_BYTES = 8 MiB (crates/etl-config/src/shared/pipeline.rs:68), left on
           the device; (c) a window per event (as many passes as events);
  budgets  max_bytes_per_insert = 64 MiB (the reference's DEFAULT_MAX_BYTES_PER_INSERT), 1 MiB and 1 (a statement per row, the most
           jump levels); stmts_cap as large as the count of a first, counting call;
  (d)      what a driver does today on the same batch: row_offsets and row_event of the object and ev_kind, ev_flags and
           ev_schema_slot copied to host memory, then write_events_inner's refusals and insert_rows' loop as one thread runs them, row
           by row — the C below, compiled here with the system compiler into a temporary directory — for the same statements and
           windows. Its output must equal the device's, word for word.
A workload whose object or plan does not come back OK (an encoding error, a cell left to the host, a partial Update the sink refuses)
is reported with that status and timed as it is: the call then ends at its status, and that is no plan.
The output — this text as `#` lines, then one JSON line per workload and engine — is committed as it is printed
(profiles/clickhouse_plan_probe_mi355x.txt)."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

TREE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, TREE)
import etl_amd  # noqa: E402,F401
import numpy as np  # noqa: E402

EMU = os.environ.get("ETLG_SIMT_RUN") == "1"   # a rehearsal against the SIMT emulator build (tests/simt): device memory is host memory, times mean nothing
if not EMU:
    import torch  # noqa: E402

from etl_amd import abi, synth  # noqa: E402
from etl_amd.decoder import Decoder, EtlError  # noqa: E402
from etl_amd.schema import infer_identity_type  # noqa: E402

DEFAULT_BUDGET = 8 * 1024 * 1024
BUDGETS = (("64MiB", abi.CH_MAX_BYTES_PER_INSERT), ("1MiB", 1 << 20), ("1", 1))
HOST_C = r"""
#include <stdint.h>
/* write_events_inner's refusals (clickhouse/core.rs:1063-1136, :1359-1452) and insert_rows' loop (clickhouse/client.rs:578-600) over
   the windows, on one thread: statements (7 words), windows (6 words); counts = statements, members, bytes, status, event, reason, window */
void host_plan(const uint8_t* kind, const uint8_t* flags, const uint32_t* slots, uint32_t slot, uint32_t replacing, uint32_t ident_ok, uint32_t width_ok,
               const uint64_t* passes, uint64_t n_passes, const uint64_t* row_event, const int64_t* offs, uint64_t n_rows, uint64_t budget,
               uint64_t* stmts, uint64_t* wins, uint64_t* counts) {
  uint64_t ns = 0, members = 0, bytes = 0, r = 0;
  counts[3] = 0; counts[4] = ~0ull; counts[5] = 0; counts[6] = ~0ull;
  for (uint64_t p = 0; p < n_passes; p++) {
    const uint64_t hi = passes[7 * p + 1], s0 = ns;
    uint64_t in_stmt = budget, wm = 0, wb = 0, first_row = ~0ull;   /* in_stmt >= budget: the next row opens a statement */
    for (uint64_t i = passes[7 * p]; i < hi; i++) {
      const uint8_t k = kind[i];
      if ((k != 'I' && k != 'U' && k != 'D') || slots[i] != slot) continue;
      wm++;
      uint32_t why = 0;
      if (k == 'U') why = (flags[i] & 4u) ? 1u : (replacing && !ident_ok) ? 2u : 0u;
      else if (k == 'D') why = (flags[i] & 3u) == 0 ? 3u : (flags[i] & 3u) == 2 ? (!width_ok ? 4u : !ident_ok ? 5u : 0u) : 0u;
      if (why) { counts[3] = 2; counts[4] = i; counts[5] = why; counts[6] = p; return; }
      while (r < n_rows && row_event[r] < i) r++;
      if (r >= n_rows || row_event[r] != i) { counts[3] = 3; counts[4] = i; counts[6] = p; return; }
      const uint64_t len = (uint64_t)(offs[r + 1] - offs[r]);
      if (in_stmt >= budget) {
        uint64_t* s = stmts + 7 * ns++;
        s[0] = p; s[1] = r; s[3] = i; s[5] = (uint64_t)offs[r];
        in_stmt = 0;
      }
      if (first_row == ~0ull) first_row = r;
      in_stmt += len; wb += len;
      uint64_t* s = stmts + 7 * (ns - 1);
      s[2] = r + 1; s[4] = i; s[6] = (uint64_t)offs[r + 1];
    }
    while (r < n_rows && row_event[r] < hi) r++;
    uint64_t* w = wins + 6 * p;
    w[0] = s0; w[1] = ns - s0; w[2] = first_row == ~0ull ? r : first_row; w[3] = r; w[4] = wm; w[5] = wb;
    members += wm; bytes += wb;
  }
  counts[0] = ns; counts[1] = members; counts[2] = bytes;
}
"""


def build_host(tmp):
    src, lib = os.path.join(tmp, "host_plan.c"), os.path.join(tmp, "host_plan.so")
    open(src, "w").write(HOST_C)
    subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-shared", "-fPIC", src, "-o", lib])
    L = C.CDLL(lib)
    L.host_plan.restype = None
    L.host_plan.argtypes = [C.c_void_p] * 3 + [C.c_uint32] * 4 + [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64] + [C.c_void_p] * 3
    return L


def size_model():
    from oracle import size_hint as SH
    m = abi.SizeModel()
    for k, v in SH.MODEL.items():
        setattr(m, k, v)
    return m


def sync():
    if not EMU:
        torch.cuda.synchronize()


def dev_zeros(n):
    return np.zeros(max(1, n), dtype=np.int64) if EMU else torch.zeros(max(1, n), dtype=torch.int64, device="cuda")


def dev_put(a):
    a = np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)
    return a.copy() if EMU else torch.from_numpy(a.copy()).cuda()


def ptr(a):
    return a.ctypes.data if EMU else a.data_ptr()


def to_host(a, n):
    return (a[:n].copy() if EMU else a[:n].cpu().numpy()).view(np.uint64)


def from_device(p, nbytes, dtype):
    if not nbytes:
        return np.zeros(0, dtype=dtype)
    if EMU:
        return np.frombuffer((C.c_uint8 * nbytes).from_address(p), dtype=dtype).copy()
    return abi.device_tensor(p, nbytes, 0).cpu().numpy().view(dtype)


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


def wal(L, mk, engine, reps, small):
    w = mk()
    buf, offs = w.fill((1 << 20) if small else (64 << 20))
    d = Decoder(0)
    w.register(d, ready=not w.cfg.emit_relations)
    b = d.decode(buf, offs, flags=abi.F_OUTPUT_ON_DEVICE)
    assert b.rc == 0, b.error
    v = b.view()
    ne = int(v.n_events)
    out = {"workload": w.name, "engine": "ReplacingMergeTree" if engine == abi.CH_REPLACING_MERGE_TREE else "MergeTree", "batch_bytes": int(len(buf)), "events": ne, "slot": 0}
    cols = w.schema_cols(w.tables[0])
    ident = [1 if c[3] else 0 for c in cols]
    ident_ok = 1 if infer_identity_type(cols, [1] * len(cols), ident) in ("PrimaryKey", "Full") else 0
    try:
        rb = b.rowbinary(0, [1] * len(cols) + [0, 0], engine, on_device=True)
    except EtlError as e:                                                    # the sink's own conversion error: there is nothing to plan
        out["rowbinary_error"] = str(e)[:200]
        b.close(); d.close()
        return out
    ok = rb.status == abi.RB_OK
    R = int(rb.n_rows) if ok else 0
    out["rowbinary"] = {"status": int(rb.status), "rows": R, "bytes": int(rb.view.n_bytes) if ok else 0, "host_rows": int(rb.view.n_host_rows)}

    # ---- (d), the download: the object's two arrays and the three header arrays come down
    def download():
        return (from_device(v.ev_kind, ne, np.uint8), from_device(v.ev_flags, ne, np.uint8), from_device(v.ev_schema_slot, 4 * ne, np.uint32),
                from_device(rb.view.row_event, 8 * R, np.uint64), from_device(rb.view.row_offsets, 8 * (R + 1) if ok else 0, np.int64))
    t_down, arrs = timed(download, reps)
    out["d_arrays_to_host"] = dict(t_down, bytes=6 * ne + 16 * R + 8)
    row_event, row_offs = arrs[3], arrs[4]

    # ---- the windows: one; the outline's passes over the cuts at 8 MiB, on the device; one per event
    m = size_model()
    hints, cuts_dev = dev_zeros(ne + 1), dev_zeros(ne + 1)
    assert d.L.etlg_batch_size_hints(d.h, b.h, C.byref(m), abi.F_OUTPUT_ON_DEVICE, C.c_void_p(ptr(hints))) == abi.OK
    done = hints & 0x7FFFFFFFFFFFFFFF
    sync()
    _, ci = b.cuts(None, DEFAULT_BUDGET, hints=ptr(done), cap=ne, on_device=ptr(cuts_dev))
    k = int(ci.n_cuts)
    cuts = dict(cuts=ptr(cuts_dev), n_cuts=k) if k else {}
    P = int(b.outline(passes_cap=0, trunc_cap=0, on_device={"slots": None}, **cuts).info.n_passes)
    ol = dev_zeros(7 * P)
    b.outline(passes_cap=P, trunc_cap=0, on_device={"passes": ptr(ol)}, **cuts)
    one = np.zeros((1, 7), dtype=np.uint64); one[0, 1] = ne
    each = np.zeros((ne, 7), dtype=np.uint64); each[:, 0] = np.arange(ne); each[:, 1] = np.arange(ne) + 1
    sets = (("a_one_window", dev_put(one.reshape(-1)), 1), ("b_outline_8MiB", ol, P), ("c_window_per_event", dev_put(each.reshape(-1)), ne))
    for tag, pd, npass in sets:
        hp = to_host(pd, 7 * npass)
        for bname, budget in BUDGETS:
            kw = dict(n_passes=npass, max_bytes_per_insert=budget)
            cnt = b.clickhouse_plan(0, ptr(pd), rb, stmts_cap=0, on_device={"statements": None}, **kw).info     # the counting call: no output at all
            S = int(cnt.n_stmts)
            bufs = {"statements": dev_zeros(7 * S), "windows": dev_zeros(6 * npass)}
            where = {n: ptr(a) for n, a in bufs.items()}
            t, o = timed(lambda: b.clickhouse_plan(0, ptr(pd), rb, stmts_cap=S, on_device=where, **kw), reps)
            plan_ok = o.info.status == abi.CHP_OK
            res = dict(t, n_passes=npass, status=int(o.info.status), plan=bool(plan_ok), n_stmts=S, n_members=int(o.info.n_members), n_bytes=int(o.info.n_bytes))
            if not plan_ok:
                res.update(event=int(o.info.event), reason=int(o.info.reason), fail_pass=int(o.info.fail_pass))
            # ---- (d), the loop
            room = S if plan_ok else R                                       # (a loop that ends at a failing event has written the statements in front of it)
            hs, hw, hn = np.zeros(7 * room + 7, dtype=np.uint64), np.zeros(6 * npass + 6, dtype=np.uint64), np.zeros(7, dtype=np.uint64)
            ts = []
            for it in range(2 + reps):
                t0 = time.perf_counter()
                L.host_plan(*[a.ctypes.data for a in arrs[:3]], 0, 1 if engine == abi.CH_REPLACING_MERGE_TREE else 0, ident_ok, 1 if sum(ident) == sum(1 for c in cols if c[3]) else 0,
                            hp.ctypes.data, npass, row_event.ctypes.data, row_offs.ctypes.data, R, budget, hs.ctypes.data, hw.ctypes.data, hn.ctypes.data)
                if it >= 2:
                    ts.append(time.perf_counter() - t0)
            loop = round(sorted(ts)[len(ts) // 2] * 1e3, 4)
            if plan_ok:
                same = (hn[:4].tolist() == [S, int(o.info.n_members), int(o.info.n_bytes), 0]
                        and np.array_equal(to_host(bufs["statements"], 7 * S), hs[:7 * S]) and np.array_equal(to_host(bufs["windows"], 6 * npass), hw[:6 * npass]))
            else:
                same = ok and (int(hn[3]), int(hn[4]), int(hn[5]), int(hn[6])) == (int(o.info.status), int(o.info.event), int(o.info.reason), int(o.info.fail_pass))
            res["host"] = {"loop_ms_median": loop, "download_plus_loop_ms": round(loop + t_down["ms_median"], 4), "equals_device": bool(same),
                           "device_over_host": round(t["ms_median"] / (loop + t_down["ms_median"]), 3)}
            out[tag + "@" + bname] = res
    rb.close()
    b.close(); d.close()
    return out


def main():
    reps = int(os.environ.get("ETLG_PROBE_REPS", "20"))
    small = os.environ.get("ETLG_PROBE_SMALL") == "1"                       # a rehearsal size
    for line in __doc__.split("\n"):
        print(("# " + line).rstrip())
    with tempfile.TemporaryDirectory() as tmp:
        L = build_host(tmp)
        for mk in (synth.cfg2, synth.cfg3, synth.cfg5):
            for engine in (abi.CH_MERGE_TREE, abi.CH_REPLACING_MERGE_TREE):
                print(json.dumps(wal(L, mk, engine, reps, small)), flush=True)


if __name__ == "__main__":
    main()
