"""etlg_bigquery_plan on HBM-resident batches, warm, medians of 20 wall times after 3 warm calls: 64 MiB of cfg2 and cfg3 and the
three-table cfg5 stream, slot 0, the etlg_batch_protobuf object, the passes and the outputs on the device. Per workload:
  windows  (a) one window over the whole batch; (b) the passes etlg_batch_outline writes for the ranges of etlg_batch_cuts at the
           reference's default budget, BatchConfig::DEFAULT_MAX_BYTES = 8 MiB (crates/etl-config/src/shared/pipeline.rs:68), left on
           the device; (c) a window per event (as many passes as events); reqs_cap as large as the count of a first, counting call;
  (d)      what a driver does today on the same batch: row_offsets and row_event of the object and ev_kind, ev_flags and
           ev_schema_slot copied to host memory, then write_events' refusals and its request per table and turn as one thread runs
           them, event by event — the C below, compiled here with the system compiler into a temporary directory — for the same
           requests and windows. Its output must equal the device's, word for word.
A table-copy batch of 400 000 rows (synth.copy_rows tiled, as tools/copy_sinks_probe.py builds it) at two values of max_batch_bytes —
10 MiB, and 64 KiB for a few hundred requests —: the call against row_offsets and row_event copied down and the two functions of the
reference in C (the header arrays are not needed there).
A workload whose object or plan does not come back OK (an encoding error, a cell left to the host, a partial Update the sink refuses)
is reported with that status and timed as it is: the call then ends at its status, and that is no plan.
The output — this text as `#` lines, then one JSON line per workload — is committed as it is printed
(profiles/bigquery_plan_probe_mi355x.txt)."""
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
COPY_ROWS = 400_000
COPY_BUDGETS = (("10MiB", 10 << 20), ("64KiB", 64 << 10))
HOST_C = r"""
#include <stdint.h>
/* write_events' refusals (bigquery/core.rs:997-1034, :1425-1554, :1599-1616, :1680-1696) and its one request per table and turn
   (:1043-1064) over the windows, on one thread: requests (8 words), windows (7 words); counts = requests, members, rows, second rows,
   bytes, status, event, reason, window */
void host_plan(const uint8_t* kind, const uint8_t* flags, const uint32_t* slots, uint32_t slot, uint32_t ident_pk, uint32_t width_ok,
               const uint64_t* passes, uint64_t n_passes, const uint64_t* row_event, const int64_t* offs, uint64_t n_rows,
               uint64_t* reqs, uint64_t* wins, uint64_t* counts) {
  uint64_t nq = 0, members = 0, rows = 0, bytes = 0, r = 0;
  counts[5] = 0; counts[6] = ~0ull; counts[7] = 0; counts[8] = ~0ull;
  for (uint64_t p = 0; p < n_passes; p++) {
    const uint64_t hi = passes[7 * p + 1];
    uint64_t wm = 0, first_row = ~0ull, end_row = 0, first_event = 0, last_event = 0;
    for (uint64_t i = passes[7 * p]; i < hi; i++) {
      const uint8_t k = kind[i];
      if ((k != 'I' && k != 'U' && k != 'D') || slots[i] != slot) continue;
      wm++;
      const uint32_t old = flags[i] & 3u;
      uint32_t why = 0;
      if (k == 'U' && (flags[i] & 4u)) why = 1u;
      else if (k == 'U' && old == 0) why = ident_pk ? 0u : 2u;
      else if (k == 'D' && old == 0) why = 5u;
      else if (k != 'I' && old == 2) why = !width_ok ? 3u : !ident_pk ? 4u : 0u;
      if (why) { counts[5] = 2; counts[6] = i; counts[7] = why; counts[8] = p; return; }
      while (r < n_rows && row_event[r] < i) r++;
      if (r >= n_rows || row_event[r] != i) { counts[5] = 3; counts[6] = i; counts[8] = p; return; }
      if (first_row == ~0ull) { first_row = r; first_event = i; }
      while (r < n_rows && row_event[r] == i) r++;   /* one row, or the two of a key-changing Update */
      end_row = r; last_event = i;
    }
    while (r < n_rows && row_event[r] < hi) r++;
    uint64_t* w = wins + 7 * p;
    const uint64_t wr = wm ? end_row - first_row : 0, wb = wm ? (uint64_t)(offs[end_row] - offs[first_row]) : 0;
    w[0] = nq; w[1] = wm ? 1 : 0; w[2] = wm ? first_row : r; w[3] = r; w[4] = wm; w[5] = wm ? wr - wm : 0; w[6] = wb;
    if (wm) {
      uint64_t* s = reqs + 8 * nq++;
      s[0] = p; s[1] = first_row; s[2] = end_row; s[3] = first_event; s[4] = last_event; s[5] = (uint64_t)offs[first_row]; s[6] = (uint64_t)offs[end_row]; s[7] = wm;
    }
    members += wm; rows += wr; bytes += wb;
  }
  counts[0] = nq; counts[1] = members; counts[2] = rows; counts[3] = rows - members; counts[4] = bytes;
}
/* calculate_target_batches_for_table_copy (:1760-1784) and split_table_rows (:1790-1827): requests (8 words), counts = requests, est, target */
void host_copy(const uint64_t* row_event, const int64_t* offs, uint64_t R, uint64_t budget, uint64_t* reqs, uint64_t* counts) {
  counts[0] = counts[1] = counts[2] = 0;
  if (!R) return;
  const uint64_t est = (uint64_t)(offs[1] - offs[0]), per = est ? budget / est : R, target = per ? (R + per - 1) / per : 1;
  uint64_t nsub = 1, each = R, extra = 0;
  if (!(R <= 1 || target == 1 || R <= target)) { const uint64_t opt = (R + target - 1) / target; nsub = (R + opt - 1) / opt; each = R / nsub; extra = R % nsub; }
  uint64_t a = 0;
  for (uint64_t i = 0; i < nsub; i++) {
    const uint64_t n = each + (i < extra ? 1 : 0);
    uint64_t* s = reqs + 8 * i;
    s[0] = 0; s[1] = a; s[2] = a + n; s[3] = row_event[a]; s[4] = row_event[a + n - 1]; s[5] = (uint64_t)offs[a]; s[6] = (uint64_t)offs[a + n]; s[7] = n;
    a += n;
  }
  counts[0] = nsub; counts[1] = est; counts[2] = target;
}
"""


def build_host(tmp):
    src, lib = os.path.join(tmp, "host_plan.c"), os.path.join(tmp, "host_plan.so")
    open(src, "w").write(HOST_C)
    subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-shared", "-fPIC", src, "-o", lib])
    L = C.CDLL(lib)
    L.host_plan.restype = None
    L.host_plan.argtypes = [C.c_void_p] * 3 + [C.c_uint32] * 3 + [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64] + [C.c_void_p] * 3
    L.host_copy.restype = None
    L.host_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
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


def host_timed(call, reps):
    ts = []
    for it in range(2 + reps):
        t0 = time.perf_counter()
        call()
        if it >= 2:
            ts.append(time.perf_counter() - t0)
    return round(sorted(ts)[len(ts) // 2] * 1e3, 4)


def wal(L, mk, reps, small):
    w = mk()
    buf, offs = w.fill((1 << 20) if small else (64 << 20))
    d = Decoder(0)
    w.register(d, ready=not w.cfg.emit_relations)
    b = d.decode(buf, offs, flags=abi.F_OUTPUT_ON_DEVICE)
    assert b.rc == 0, b.error
    v = b.view()
    ne = int(v.n_events)
    out = {"workload": w.name, "batch_bytes": int(len(buf)), "events": ne, "slot": 0}
    cols = w.schema_cols(w.tables[0])
    ident = [1 if c[3] else 0 for c in cols]
    ident_pk = 1 if infer_identity_type(cols, [1] * len(cols), ident) == "PrimaryKey" else 0
    width_ok = 1 if sum(ident) == sum(1 for c in cols if c[3]) else 0
    try:
        pb = b.protobuf(0, on_device=True)
    except EtlError as e:                                                    # the sink's own validation error: there is nothing to plan
        out["protobuf_error"] = str(e)[:200]
        b.close(); d.close()
        return out
    ok = pb.status == abi.RB_OK
    R = int(pb.n_rows) if ok else 0
    out["protobuf"] = {"status": int(pb.status), "rows": R, "bytes": int(pb.view.n_bytes) if ok else 0, "host_rows": int(pb.view.n_host_rows)}

    # ---- (d), the download: the object's two arrays and the three header arrays come down
    def download():
        return (from_device(v.ev_kind, ne, np.uint8), from_device(v.ev_flags, ne, np.uint8), from_device(v.ev_schema_slot, 4 * ne, np.uint32),
                from_device(pb.view.row_event, 8 * R, np.uint64), from_device(pb.view.row_offsets, 8 * (R + 1) if ok else 0, np.int64))
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
        cnt = b.bigquery_plan(0, ptr(pd), pb, n_passes=npass, reqs_cap=0, on_device={"requests": None}).info     # the counting call: no output at all
        S = int(cnt.n_reqs)
        bufs = {"requests": dev_zeros(8 * S), "windows": dev_zeros(7 * npass)}
        where = {n: ptr(a) for n, a in bufs.items()}
        t, o = timed(lambda: b.bigquery_plan(0, ptr(pd), pb, n_passes=npass, reqs_cap=S, on_device=where), reps)
        plan_ok = o.info.status == abi.BQP_OK
        res = dict(t, n_passes=npass, status=int(o.info.status), plan=bool(plan_ok), n_reqs=S, n_members=int(o.info.n_members), n_rows=int(o.info.n_rows),
                   n_two_row=int(o.info.n_two_row), n_bytes=int(o.info.n_bytes))
        if not plan_ok:
            res.update(event=int(o.info.event), reason=int(o.info.reason), fail_pass=int(o.info.fail_pass))
        # ---- (d), the loop
        room = S if plan_ok else npass                                       # (a loop that ends at a failing event has written the requests in front of it)
        hs, hw, hn = np.zeros(8 * room + 8, dtype=np.uint64), np.zeros(7 * npass + 7, dtype=np.uint64), np.zeros(9, dtype=np.uint64)
        loop = host_timed(lambda: L.host_plan(*[a.ctypes.data for a in arrs[:3]], 0, ident_pk, width_ok, hp.ctypes.data, npass, row_event.ctypes.data,
                                              row_offs.ctypes.data, R, hs.ctypes.data, hw.ctypes.data, hn.ctypes.data), reps)
        if plan_ok:
            same = (hn[:6].tolist() == [S, int(o.info.n_members), int(o.info.n_rows), int(o.info.n_two_row), int(o.info.n_bytes), 0]
                    and np.array_equal(to_host(bufs["requests"], 8 * S), hs[:8 * S]) and np.array_equal(to_host(bufs["windows"], 7 * npass), hw[:7 * npass]))
        else:
            same = ok and (int(hn[5]), int(hn[6]), int(hn[7]), int(hn[8])) == (int(o.info.status), int(o.info.event), int(o.info.reason), int(o.info.fail_pass))
        res["host"] = {"loop_ms_median": loop, "download_plus_loop_ms": round(loop + t_down["ms_median"], 4), "equals_device": bool(same),
                       "device_over_host": round(t["ms_median"] / (loop + t_down["ms_median"]), 3)}
        out[tag] = res
    pb.close()
    b.close(); d.close()
    return out


def copy(L, reps, small):
    cols = [c for c in synth.COPY_COLS if c[0] != "u"]
    drop = [c[0] for c in synth.COPY_COLS].index("u")
    base = []
    for r in synth.copy_rows(2000 if small else 20000, 1, clean=True):
        f = r[:-1].split(b"\t")
        del f[drop]
        base.append(b"\t".join(f) + b"\n")
    rows = base * ((4000 if small else COPY_ROWS) // len(base))
    buf = np.frombuffer(b"".join(rows), dtype=np.uint8)
    offs = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint32)
    d = Decoder(0)
    d.schema_put(42, 0, cols)
    slot = d.table_ready(42, 0, [1] * len(cols), [1] + [0] * (len(cols) - 1))
    b = d.copy_decode(slot, buf, offs, flags=abi.F_OUTPUT_ON_DEVICE)
    assert b.rc == 0, b.error
    out = {"workload": "copy_rows clean", "batch_bytes": int(len(buf)), "rows": len(rows), "slot": int(slot)}
    pb = b.protobuf(slot, on_device=True)
    ok = pb.status == abi.RB_OK
    R = int(pb.n_rows) if ok else 0
    out["protobuf"] = {"status": int(pb.status), "rows": R, "bytes": int(pb.view.n_bytes) if ok else 0}
    t_down, arrs = timed(lambda: (from_device(pb.view.row_event, 8 * R, np.uint64), from_device(pb.view.row_offsets, 8 * (R + 1) if ok else 0, np.int64)), reps)
    out["d_arrays_to_host"] = dict(t_down, bytes=16 * R + 8)
    for bname, budget in COPY_BUDGETS:
        cnt = b.bigquery_plan(slot, None, pb, max_batch_bytes=budget, reqs_cap=0, on_device={"requests": None}).info
        S = int(cnt.n_reqs)
        bufs = {"requests": dev_zeros(8 * S), "windows": dev_zeros(7)}
        where = {n: ptr(a) for n, a in bufs.items()}
        t, o = timed(lambda: b.bigquery_plan(slot, None, pb, max_batch_bytes=budget, reqs_cap=S, on_device=where), reps)
        plan_ok = o.info.status == abi.BQP_OK
        res = dict(t, status=int(o.info.status), plan=bool(plan_ok), n_reqs=S, n_rows=int(o.info.n_rows), n_bytes=int(o.info.n_bytes),
                   est_row_bytes=int(o.info.est_row_bytes), target_batches=int(o.info.target_batches))
        hs, hn = np.zeros(8 * S + 8, dtype=np.uint64), np.zeros(3, dtype=np.uint64)
        loop = host_timed(lambda: L.host_copy(arrs[0].ctypes.data, arrs[1].ctypes.data, R, budget, hs.ctypes.data, hn.ctypes.data), reps)
        same = plan_ok and hn.tolist() == [S, int(o.info.est_row_bytes), int(o.info.target_batches)] and np.array_equal(to_host(bufs["requests"], 8 * S), hs[:8 * S])
        res["host"] = {"loop_ms_median": loop, "download_plus_loop_ms": round(loop + t_down["ms_median"], 4), "equals_device": bool(same),
                       "device_over_host": round(t["ms_median"] / (loop + t_down["ms_median"]), 3)}
        out["copy@" + bname] = res
    pb.close()
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
            print(json.dumps(wal(L, mk, reps, small)), flush=True)
        print(json.dumps(copy(L, reps, small)), flush=True)


if __name__ == "__main__":
    main()
