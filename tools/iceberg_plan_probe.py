"""etlg_iceberg_plan on HBM-resident batches, warm, medians of 20 wall times after 3 warm calls: 64 MiB of cfg2 and cfg3, the three-table
cfg5 stream (slot 0) and a table with nullable and list columns (id int8, v int4 NULL, s text NULL, b bool NULL, ia int4[] NULL with
NULL elements, ta text[] NULL with NULL elements; ETLG_ROWS_PARSE_ARRAYS), the etlg_batch_iceberg object, the passes and the outputs on
the device. Per workload:
  windows  (a) one window over the whole batch; (b) the passes etlg_batch_outline writes with ETLG_OL_RELATIONS_INLINE for the ranges
           of etlg_batch_cuts at the reference's default budget, BatchConfig::DEFAULT_MAX_BYTES = 8 MiB
           (crates/etl-config/src/shared/pipeline.rs:68), left on the device; (c) a window per event (as many passes as events);
           writes_cap as large as the count of a first, counting call;
  (d)      what a driver does today on the same batch: ev_kind, ev_flags, ev_schema_slot, ev_table_id and row_event copied to host
           memory, with every validity / deferred / child validity bitmap and every offsets / child offsets array the slices read
           (a bitmap whose column reports a count of 0 is not read and not copied), then write_events' refusals, its write per table
           and turn and the slice of every column as one thread runs them — the C below, compiled here with the system compiler into a
           temporary directory — for the same writes, windows and slices. Its output must equal the device's, word for word.
A workload whose plan does not come back OK (a partial Update or a key-only Delete, which the sink refuses) is reported with that
status and timed as it is: the call then ends at its status, and that is no plan.
Not measured here: the split of the call's time among the k_icp_* kernels, and table-copy batches.
The output — this text as `#` lines, then one JSON line per workload — is committed as it is printed
(profiles/iceberg_plan_probe_mi355x.txt)."""
import ctypes as C
import json
import os
import struct
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
from etl_amd.decoder import Decoder  # noqa: E402

DEFAULT_BUDGET = 8 * 1024 * 1024
LIST_REL = 16600
LIST_COLS = [("id", 20, False, 1), ("v", 23, True, 0), ("s", 25, True, 0), ("b", 16, True, 0), ("ia", 1007, True, 0), ("ta", 1009, True, 0)]
HOST_C = r"""
#include <stdint.h>
/* a column as the host sees it: kind, width, child_kind, child_width, validity, deferred, offsets, child_validity, child_offsets,
   child_count — a bitmap pointer is 0 when the column reports no bit to count */
static uint64_t ones(const uint64_t* w, uint64_t lo, uint64_t hi) {
  uint64_t n = 0;
  for (uint64_t i = lo; i < hi; ) {
    if (!(i & 63) && i + 64 <= hi) { n += (uint64_t)__builtin_popcountll(w[i >> 6]); i += 64; }
    else { n += (w[i >> 6] >> (i & 63)) & 1u; i++; }
  }
  return n;
}
static void slice(const uint64_t* c, uint64_t r0, uint64_t r1, uint64_t* o) {
  const uint64_t kind = c[0], width = c[1], ck = c[2], cw = c[3], cc = c[9];
  const uint64_t* valid = (const uint64_t*)c[4]; const uint64_t* def = (const uint64_t*)c[5]; const int64_t* offs = (const int64_t*)c[6];
  const uint64_t* cvalid = (const uint64_t*)c[7]; const int64_t* coffs = (const int64_t*)c[8];
  uint64_t b0 = 0, b1 = 0, c0 = 0, c1 = 0, cn = 0;
  if (kind == 13) {
    c0 = (uint64_t)offs[r0]; c1 = (uint64_t)offs[r1];
    if (cw) { b0 = c0 * cw; b1 = c1 * cw; } else if (ck == 0) { b0 = c0; b1 = c1; } else if (cc) { b0 = (uint64_t)coffs[c0]; b1 = (uint64_t)coffs[c1]; }
    if (cvalid) cn = (c1 - c0) - ones(cvalid, c0, c1);
  } else if (width) { b0 = r0 * width; b1 = r1 * width; }
  else if (kind == 0) { b0 = r0; b1 = r1; }
  else { b0 = (uint64_t)offs[r0]; b1 = (uint64_t)offs[r1]; }
  o[0] = valid ? (r1 - r0) - ones(valid, r0, r1) : 0; o[1] = def ? ones(def, r0, r1) : 0; o[2] = b0; o[3] = b1; o[4] = c0; o[5] = c1; o[6] = cn;
}
/* write_events' refusals (iceberg/core.rs:636-680), its one insert_rows per table and turn (:395-409) and the slices, on one thread:
   writes (7 words), slices (7 words per write and column), windows (6 words); counts = writes, members, rows, mixed, status, event,
   reason, window */
void host_plan(const uint8_t* kind, const uint8_t* flags, const uint32_t* slots, const uint32_t* tables, uint32_t slot, uint32_t table_id,
               const uint64_t* passes, uint64_t n_passes, const uint64_t* row_event, uint64_t n_rows, const uint64_t* cols, uint64_t n_cols,
               uint64_t* writes, uint64_t* slices, uint64_t* wins, uint64_t* counts) {
  uint64_t nw = 0, members = 0, rows = 0, mixed = 0, r = 0;
  counts[4] = 0; counts[5] = ~0ull; counts[6] = 0; counts[7] = ~0ull;
  for (uint64_t p = 0; p < n_passes; p++) {
    const uint64_t hi = passes[7 * p + 1];
    uint64_t wm = 0, first_row = ~0ull, end_row = 0, first_event = 0, last_event = 0, other = ~0ull;
    for (uint64_t i = passes[7 * p]; i < hi; i++) {
      const uint8_t k = kind[i];
      if (k != 'I' && k != 'U' && k != 'D') continue;
      if (slots[i] != slot) { if (tables[i] == table_id && other == ~0ull) other = i; continue; }
      wm++;
      const uint32_t old = flags[i] & 3u;
      const uint32_t why = k == 'U' ? ((flags[i] & 4u) ? 1u : 0u) : k == 'D' ? (old == 2 ? 2u : old == 0 ? 3u : 0u) : 0u;
      if (why) { counts[4] = 2; counts[5] = i; counts[6] = why; counts[7] = p; return; }
      while (r < n_rows && row_event[r] < i) r++;
      if (r >= n_rows || row_event[r] != i) { counts[4] = 3; counts[5] = i; counts[7] = p; return; }
      if (first_row == ~0ull) { first_row = r; first_event = i; }
      end_row = ++r; last_event = i;
    }
    while (r < n_rows && row_event[r] < hi) r++;
    if (!wm) other = ~0ull;
    uint64_t* w = wins + 6 * p;
    w[0] = nw; w[1] = wm ? 1 : 0; w[2] = wm ? first_row : r; w[3] = r; w[4] = wm; w[5] = other;
    if (wm) {
      for (uint64_t c = 0; c < n_cols; c++) slice(cols + 10 * c, first_row, end_row, slices + 7 * (nw * n_cols + c));
      uint64_t* s = writes + 7 * nw++;
      s[0] = p; s[1] = first_row; s[2] = end_row; s[3] = first_event; s[4] = last_event; s[5] = wm; s[6] = other;
      rows += end_row - first_row;
    }
    members += wm; mixed += other != ~0ull;
  }
  counts[0] = nw; counts[1] = members; counts[2] = rows; counts[3] = mixed;
}
"""
WIDTH = {1: 4, 2: 8, 3: 4, 4: 8, 5: 4, 6: 8, 7: 8, 8: 8, 9: 16}


def build_host(tmp):
    src, lib = os.path.join(tmp, "host_plan.c"), os.path.join(tmp, "host_plan.so")
    open(src, "w").write(HOST_C)
    subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-shared", "-fPIC", src, "-o", lib])
    L = C.CDLL(lib)
    L.host_plan.restype = None
    L.host_plan.argtypes = [C.c_void_p] * 4 + [C.c_uint32] * 2 + [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64] + [C.c_void_p] * 4
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
    if not nbytes or not p:
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


def list_stream(cap):
    """CopyData-framed pgoutput of Inserts, full Updates with a key image and full-old-row Deletes of the list table, up to `cap`
    bytes: 200 rows per transaction, NULL cells, NULL elements and empty arrays in fixed cycles."""
    def tup(cells):
        out = [struct.pack(">h", len(cells))]
        for c in cells:
            out.append(b"n" if c is None else b"t" + struct.pack(">i", len(c)) + c)
        return b"".join(out)
    tails = []
    for j in range(91):
        ia = None if j % 13 == 4 else b"{}" if j % 4 == 0 else b"{%d,NULL,3}" % j if j % 4 == 1 else b"{7,8,9,10}"
        ta = None if j % 9 == 5 else b"{}" if j % 3 == 0 else b'{a,NULL,"b c"}' if j % 3 == 1 else b"{NULL,some text}"
        tails.append(tup([b"0", None if j % 7 == 2 else b"%d" % -j, None if j % 5 == 1 else b"text %d" % j, None if j % 11 == 3 else b"tf"[j % 2:j % 2 + 1], ia, ta])[2 + 6:])
    ncol, rel = struct.pack(">h", 6), struct.pack(">I", LIST_REL)
    buf, offs, lsn, k = bytearray(), [0], 0x3000000, 0

    def put(msg):
        nonlocal lsn
        lsn += 8
        payload = b"w" + struct.pack(">QQq", lsn, lsn, 0) + msg
        buf.extend(b"d" + struct.pack(">I", len(payload) + 4) + payload)
        offs.append(len(buf))
    while len(buf) + 200 * 160 < cap:
        final = lsn + 8 * 202
        put(b"B" + struct.pack(">QqI", final, 0, 900 + k // 200))
        for _ in range(200):
            idt = b"%d" % (k + 1)
            cell0 = b"t" + struct.pack(">i", len(idt)) + idt
            row = ncol + cell0 + tails[k % 91]
            if k % 11 == 10:
                put(b"D" + rel + b"O" + row)
            elif k % 5 == 4:
                put(b"U" + rel + b"K" + struct.pack(">h", 1) + cell0 + b"N" + row)
            else:
                put(b"I" + rel + b"N" + row)
            k += 1
        put(b"C" + struct.pack(">bQQq", 0, final, final + 8, 0))
    return np.frombuffer(bytes(buf), dtype=np.uint8), np.array(offs, dtype=np.uint32)


def workloads(small):
    cap = (1 << 20) if small else (64 << 20)
    for mk in (synth.cfg2, synth.cfg3, synth.cfg5):
        w = mk()
        buf, offs = w.fill(cap)
        yield w.name, buf, offs, (lambda d, w=w: w.register(d, ready=not w.cfg.emit_relations)), False

    def reg(d):
        d.schema_put(LIST_REL, 0, LIST_COLS, name="list_table")
        d.table_state(LIST_REL, abi.TS_READY)
        d.table_ready(LIST_REL, 0, [1] * 6, [1, 0, 0, 0, 0, 0])
    buf, offs = list_stream(cap)
    yield "nullable_and_list_columns", buf, offs, reg, True


def download_columns(cl, R):
    """Every array of the object the slices read, copied down, and the column records of the C loop (kept alive by the second result)."""
    keep, recs = [], []
    for i in range(int(cl.view.n_cols)):
        k = cl.column(i)
        kind, m = int(k.arrow_kind), int(k.child_count)
        bm = lambda p, count, bits: from_device(p, (bits + 63) // 64 * 8, np.uint64) if count and bits else np.zeros(0, np.uint64)
        arrs = [bm(k.validity, int(k.null_count), R), bm(k.deferred, int(k.deferred_count), R),
                from_device(k.offsets, 8 * (R + 1), np.int64) if k.offsets and kind >= 10 else np.zeros(0, np.int64),
                bm(k.child_validity, int(k.child_null_count), m) if kind == abi.AK_LIST else np.zeros(0, np.uint64),
                from_device(k.child_offsets, 8 * (m + 1), np.int64) if kind == abi.AK_LIST and m and k.child_offsets and int(k.child_kind) >= 10 else np.zeros(0, np.int64)]
        keep.append(arrs)
        recs.append([kind, int(k.value_bytes), int(k.child_kind), WIDTH.get(int(k.child_kind), 0) if kind == abi.AK_LIST else 0]
                    + [a.ctypes.data if len(a) else 0 for a in arrs] + [m])
    return np.array(recs, dtype=np.uint64).reshape(-1), keep


def run(L, name, buf, offs, register, parse_arrays, reps):
    d = Decoder(0)
    register(d)
    b = d.decode(buf, offs, flags=abi.F_OUTPUT_ON_DEVICE)
    assert b.rc == 0, b.error
    v = b.view()
    ne = int(v.n_events)
    cl = b.iceberg(0, parse_arrays=parse_arrays, on_device=True)
    R, nc = int(cl.view.n_rows), int(cl.view.n_cols)
    table_id = int(v.slots[0].table_id)
    out = {"workload": name, "batch_bytes": int(len(buf)), "events": ne, "slot": 0, "changelog": {"rows": R, "cols": nc, "refused": int(cl.changelog.n_host_rows)}}

    # ---- (d), the download: the four header arrays, row_event and the object's bitmaps and offsets come down
    def download():
        return (from_device(v.ev_kind, ne, np.uint8), from_device(v.ev_flags, ne, np.uint8), from_device(v.ev_schema_slot, 4 * ne, np.uint32),
                from_device(v.ev_table_id, 4 * ne, np.uint32), from_device(cl.view.row_event, 8 * R, np.uint64), download_columns(cl, R))
    t_down, arrs = timed(download, reps)
    recs, keep = arrs[5]
    out["d_arrays_to_host"] = dict(t_down, bytes=int(10 * ne + 8 * R + sum(a.nbytes for col in keep for a in col)),
                                   bitmaps_scanned=int(sum(1 for col in keep for a in (col[0], col[1], col[3]) if len(a))))

    # ---- the windows: one; the outline's passes (Relations inline) over the cuts at 8 MiB, on the device; one per event
    m = size_model()
    hints, cuts_dev = dev_zeros(ne + 1), dev_zeros(ne + 1)
    assert d.L.etlg_batch_size_hints(d.h, b.h, C.byref(m), abi.F_OUTPUT_ON_DEVICE, C.c_void_p(ptr(hints))) == abi.OK
    done = hints & 0x7FFFFFFFFFFFFFFF
    sync()
    _, ci = b.cuts(None, DEFAULT_BUDGET, hints=ptr(done), cap=ne, on_device=ptr(cuts_dev))
    k = int(ci.n_cuts)
    cuts = dict(cuts=ptr(cuts_dev), n_cuts=k) if k else {}
    P = int(b.outline(passes_cap=0, trunc_cap=0, relations_inline=True, on_device={"slots": None}, **cuts).info.n_passes)
    ol = dev_zeros(7 * P)
    b.outline(passes_cap=P, trunc_cap=0, relations_inline=True, on_device={"passes": ptr(ol)}, **cuts)
    one = np.zeros((1, 7), dtype=np.uint64); one[0, 1] = ne
    each = np.zeros((ne, 7), dtype=np.uint64); each[:, 0] = np.arange(ne); each[:, 1] = np.arange(ne) + 1
    sets = (("a_one_window", dev_put(one.reshape(-1)), 1), ("b_outline_8MiB", ol, P), ("c_window_per_event", dev_put(each.reshape(-1)), ne))
    for tag, pd, npass in sets:
        hp = to_host(pd, 7 * npass)
        cnt = b.iceberg_plan(0, ptr(pd), cl, n_passes=npass, writes_cap=0, on_device={"writes": None}).info     # the counting call: no output at all
        S = int(cnt.n_writes)
        bufs = {"writes": dev_zeros(7 * S), "slices": dev_zeros(7 * S * nc), "windows": dev_zeros(6 * npass)}
        where = {n: ptr(a) for n, a in bufs.items()}
        t, o = timed(lambda: b.iceberg_plan(0, ptr(pd), cl, n_passes=npass, writes_cap=S, on_device=where), reps)
        plan_ok = o.info.status == abi.ICP_OK
        res = dict(t, n_passes=npass, status=int(o.info.status), plan=bool(plan_ok), n_writes=S, n_members=int(o.info.n_members), n_rows=int(o.info.n_rows),
                   n_mixed=int(o.info.n_mixed), slices=S * nc)
        if not plan_ok:
            res.update(event=int(o.info.event), reason=int(o.info.reason), fail_pass=int(o.info.fail_pass))
        # ---- (d), the loop
        room = S if plan_ok else npass                                       # (a loop that ends at a failing event has written the writes in front of it)
        hs, hsl, hw, hn = np.zeros(7 * room + 7, dtype=np.uint64), np.zeros(7 * room * nc + 7, dtype=np.uint64), np.zeros(6 * npass + 6, dtype=np.uint64), np.zeros(8, dtype=np.uint64)
        loop = host_timed(lambda: L.host_plan(*[a.ctypes.data for a in arrs[:4]], 0, table_id, hp.ctypes.data, npass, arrs[4].ctypes.data, R, recs.ctypes.data, nc,
                                              hs.ctypes.data, hsl.ctypes.data, hw.ctypes.data, hn.ctypes.data), reps)
        if plan_ok:
            same = (hn[:5].tolist() == [S, int(o.info.n_members), int(o.info.n_rows), int(o.info.n_mixed), 0]
                    and np.array_equal(to_host(bufs["writes"], 7 * S), hs[:7 * S]) and np.array_equal(to_host(bufs["slices"], 7 * S * nc), hsl[:7 * S * nc])
                    and np.array_equal(to_host(bufs["windows"], 6 * npass), hw[:6 * npass]))
        else:
            same = (int(hn[4]), int(hn[5]), int(hn[6]), int(hn[7])) == (int(o.info.status), int(o.info.event), int(o.info.reason), int(o.info.fail_pass))
        res["host"] = {"loop_ms_median": loop, "download_plus_loop_ms": round(loop + t_down["ms_median"], 4), "equals_device": bool(same),
                       "device_over_host": round(t["ms_median"] / (loop + t_down["ms_median"]), 3)}
        out[tag] = res
    cl.close()
    b.close(); d.close()
    return out


def main():
    reps = int(os.environ.get("ETLG_PROBE_REPS", "20"))
    small = os.environ.get("ETLG_PROBE_SMALL") == "1"                       # a rehearsal size
    for line in __doc__.split("\n"):
        print(("# " + line).rstrip())
    with tempfile.TemporaryDirectory() as tmp:
        L = build_host(tmp)
        for name, buf, offs, register, parse_arrays in workloads(small):
            print(json.dumps(run(L, name, buf, offs, register, parse_arrays, reps)), flush=True)


if __name__ == "__main__":
    main()
