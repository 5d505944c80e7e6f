"""etlg_snowflake_plan on HBM-resident batches, warm, medians of 20 wall times after 3 warm calls: 64 MiB of cfg2 and cfg3 and the
three-table cfg5 stream, slot 0, the etlg_batch_ndjson object, the passes and the outputs on the device, the reference's thresholds
(flush at 128 KiB, rows of at most 2 MiB). Per workload:
  (a) one window over the whole batch; (b) the passes etlg_batch_outline writes for the ranges of etlg_batch_cuts at the reference's
      default budget, BatchConfig::DEFAULT_MAX_BYTES = 8 MiB (crates/etl-config/src/shared/pipeline.rs:68), left on the device;
      (c) a window per event (as many passes as events). segs_cap as large as the count of a first, counting call, no committed offset;
  (a_committed) (a) with the key of the slot's middle member as the committed offset;
  (d) what a driver does today on the same batch: row_offsets and row_event of the object and ev_kind, ev_flags, ev_schema_slot,
      ev_commit_lsn and ev_tx_ordinal copied to host memory (about 40 bytes per event), then encode_* and push_row's decisions as one
      thread runs them, row by row — the C below, compiled here with the system compiler into a temporary directory — for the same
      segments and windows. Its output must equal the device's, word for word.
A workload whose object or plan does not come back OK (an encoding error, a cell left to the host, a partial Update the sink refuses)
is reported with that status and timed as it is: the call then ends at its status.
The output — this text as `#` lines, then one JSON line per workload — is committed as it is printed
(profiles/snowflake_plan_probe_mi355x.txt)."""
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

DEFAULT_BUDGET = 8 * 1024 * 1024
HOST_C = r"""
#include <stdint.h>
/* encode_insert / encode_update / encode_delete (snowflake/core.rs:345-438) and RowBatchBuilder::push_row (streaming/batch.rs:150-189)
   over the windows, on one thread: segments (13 words), windows (7 words); counts = segments, members, retained, bytes, status, event */
void host_plan(const uint8_t* kind, const uint8_t* flags, const uint32_t* slots, const uint64_t* commit, const uint64_t* ord, uint32_t slot,
               const uint64_t* passes, uint64_t n_passes, const uint64_t* row_event, const int64_t* offs, uint64_t n_rows, uint32_t has_c, uint64_t cl, uint64_t co,
               uint64_t flush, uint64_t max_row, uint64_t* segs, uint64_t* wins, uint64_t* counts) {
  uint64_t ns = 0, members = 0, kept = 0, bytes = 0, r = 0;
  counts[4] = 0; counts[5] = ~0ull;
  for (uint64_t p = 0; p < n_passes; p++) {
    const uint64_t hi = passes[7 * p + 1], s0 = ns;
    uint64_t since = 0, wm = 0, wk = 0, wb = 0, first_row = ~0ull;
    for (uint64_t i = passes[7 * p]; i < hi; i++) {
      const uint8_t k = kind[i];
      if ((k != 'I' && k != 'U' && k != 'D') || slots[i] != slot) continue;
      wm++;
      if (k == 'U' && (flags[i] & 4u)) { counts[4] = 2; counts[5] = i; return; }
      if (has_c && !(commit[i] > cl || (commit[i] == cl && ord[i] > co))) continue;
      if (k == 'D' && (flags[i] & 3u) == 0) { counts[4] = 2; counts[5] = i; return; }
      wk++;
      while (r < n_rows && row_event[r] < i) r++;
      if (r >= n_rows || row_event[r] != i) { counts[4] = 4; counts[5] = i; return; }
      const uint64_t len = (uint64_t)(offs[r + 1] - offs[r]);
      if (len > max_row) { counts[4] = 2; counts[5] = i; return; }
      const int fl = since + len >= flush;
      if (fl) since = 0;
      if (fl || ns == s0) {
        uint64_t* s = segs + 13 * ns++;
        s[0] = p; s[1] = r; s[3] = i; s[5] = (uint64_t)offs[r]; s[7] = len; s[8] = commit[i]; s[9] = ord[i]; s[12] = fl ? 1 : 0;
      }
      if (first_row == ~0ull) first_row = r;
      since += len; wb += len;
      uint64_t* s = segs + 13 * (ns - 1);
      s[2] = r + 1; s[4] = i; s[6] = (uint64_t)offs[r + 1]; s[10] = commit[i]; s[11] = ord[i];
    }
    while (r < n_rows && row_event[r] < hi) r++;
    uint64_t* w = wins + 7 * p;
    w[0] = s0; w[1] = ns - s0; w[2] = first_row == ~0ull ? r : first_row; w[3] = r; w[4] = wm; w[5] = wk; w[6] = wb;
    members += wm; kept += wk; bytes += wb;
  }
  counts[0] = ns; counts[1] = members; counts[2] = kept; counts[3] = bytes;
}
"""


def build_host(tmp):
    src, lib = os.path.join(tmp, "host_plan.c"), os.path.join(tmp, "host_plan.so")
    open(src, "w").write(HOST_C)
    subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-shared", "-fPIC", src, "-o", lib])
    L = C.CDLL(lib)
    L.host_plan.restype = None
    L.host_plan.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32] + [C.c_uint64] * 4 + [C.c_void_p] * 3
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
    names = [c[0] for c in w.schema_cols(w.tables[0])]
    try:
        nd = b.ndjson(0, names, on_device=True)
    except EtlError as e:                                                    # the sink's own encoding error: there is nothing to plan
        out["ndjson_error"] = str(e)[:200]
        b.close(); d.close()
        return out
    ok = nd.status == abi.RB_OK
    R = int(nd.n_rows) if ok else 0
    out["ndjson"] = {"status": int(nd.status), "rows": R, "bytes": int(nd.view.n_bytes) if ok else 0, "host_rows": int(nd.view.n_host_rows)}

    # ---- (d), the download: the object's two arrays and the five header arrays come down
    def download():
        return (from_device(v.ev_kind, ne, np.uint8), from_device(v.ev_flags, ne, np.uint8), from_device(v.ev_schema_slot, 4 * ne, np.uint32),
                from_device(v.ev_commit_lsn, 8 * ne, np.uint64), from_device(v.ev_tx_ordinal, 8 * ne, np.uint64),
                from_device(nd.view.row_event, 8 * R, np.uint64), from_device(nd.view.row_offsets, 8 * (R + 1) if ok else 0, np.int64))
    t_down, arrs = timed(download, reps)
    out["d_arrays_to_host"] = dict(t_down, bytes=22 * ne + 16 * R + 8)
    kind, _, slot, commit, ordn, row_event, row_offs = arrs
    mine = np.flatnonzero(((kind == ord("I")) | (kind == ord("U")) | (kind == ord("D"))) & (slot == 0))
    mid = int(mine[len(mine) // 2])

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
    sets = (("a_one_window", dev_put(one.reshape(-1)), 1, None), ("b_outline_8MiB", ol, P, None), ("c_window_per_event", dev_put(each.reshape(-1)), ne, None),
            ("a_committed", dev_put(one.reshape(-1)), 1, (int(commit[mid]), int(ordn[mid]))))
    F, M = abi.SF_MAX_UNFLUSHED_BYTES, abi.SF_MAX_ROW_BYTES
    for tag, pd, npass, cm in sets:
        kw = dict(n_passes=npass, committed=cm, flush_bytes=F, max_row_bytes=M)
        cnt = b.snowflake_plan(0, ptr(pd), nd, segs_cap=0, on_device={"segments": None}, **kw).info     # the counting call: no output at all
        S = int(cnt.n_segs)
        bufs = {"segments": dev_zeros(13 * S), "windows": dev_zeros(7 * npass)}
        where = {n: ptr(a) for n, a in bufs.items()}
        t, o = timed(lambda: b.snowflake_plan(0, ptr(pd), nd, segs_cap=S, on_device=where, **kw), reps)
        out[tag] = dict(t, n_passes=npass, status=int(o.info.status), n_segs=S, n_members=int(o.info.n_members), n_retained=int(o.info.n_retained), n_bytes=int(o.info.n_bytes))
        if o.info.status != abi.SFP_OK:
            out[tag].update(event=int(o.info.event), reason=int(o.info.reason))
        # ---- (d), the loop
        hp = to_host(pd, 7 * npass)
        room = S if o.info.status == abi.SFP_OK else R                        # (a loop that ends at a failing event has written the segments in front of it)
        hs, hw, hn = np.zeros(13 * room + 13, dtype=np.uint64), np.zeros(7 * npass + 7, dtype=np.uint64), np.zeros(6, dtype=np.uint64)
        has_c, cl, co = (0, 0, 0) if cm is None else (1, cm[0], cm[1])
        ts = []
        for it in range(2 + reps):
            t0 = time.perf_counter()
            L.host_plan(*[a.ctypes.data for a in arrs[:5]], 0, hp.ctypes.data, npass, row_event.ctypes.data, row_offs.ctypes.data, R, has_c, cl, co, F, M,
                        hs.ctypes.data, hw.ctypes.data, hn.ctypes.data)
            if it >= 2:
                ts.append(time.perf_counter() - t0)
        loop = round(sorted(ts)[len(ts) // 2] * 1e3, 4)
        if o.info.status == abi.SFP_OK:
            same = (hn[:5].tolist() == [S, int(o.info.n_members), int(o.info.n_retained), int(o.info.n_bytes), 0]
                    and np.array_equal(to_host(bufs["segments"], 13 * S), hs[:13 * S]) and np.array_equal(to_host(bufs["windows"], 7 * npass), hw[:7 * npass]))
        else:
            same = ok and (int(hn[4]), int(hn[5])) == (int(o.info.status), int(o.info.event))
        out["d_" + tag[2:]] = {"host_loop_ms_median": loop, "download_plus_loop_ms": round(loop + t_down["ms_median"], 4), "equals_device": bool(same),
                               "device_over_host": round(t["ms_median"] / (loop + t_down["ms_median"]), 3)}
    nd.close()
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


if __name__ == "__main__":
    main()
