"""etlg_ducklake_plan on HBM-resident batches, warm, medians of 20 wall times after 3 warm calls: 64 MiB of cfg2 and cfg3 and the
three-table cfg5 stream, slot 0, outputs on the device. Per workload:
  (a) one window over the whole batch; (b) the passes etlg_batch_outline writes for the ranges of etlg_batch_cuts at the reference's
      default budget, BatchConfig::DEFAULT_MAX_BYTES = 8 MiB (crates/etl-config/src/shared/pipeline.rs:68), left on the device;
      (c) a window per event (as many passes as events). Device passes, device outputs, caps as large as the counts of a first,
      counting call, no watermark, no record objects (rec_first = ~0);
  (a_objects) (a) again with the device-resident etlg_batch_duckdb objects of status ETLG_RB_OK given, so that every retained member is
      looked up in their row_event; (a_watermark) (a) with the key of the slot's middle member as the watermark;
  (d) what a driver does today on the same batch: ev_kind, ev_flags, ev_schema_slot, ev_start_lsn, ev_commit_lsn and ev_tx_ordinal copied
      to host memory (30 bytes per event), then the three loops as one thread runs them — the C below, compiled here with the system
      compiler into a temporary directory — for the same ranges, batches and ops (rec_first = ~0). Its output must equal the device's,
      word for word.
The output — this text as `#` lines, then one JSON line per workload — is committed as it is printed
(profiles/ducklake_plan_probe_mi355x.txt)."""
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
from etl_amd.decoder import Decoder  # noqa: E402

DEFAULT_BUDGET = 8 * 1024 * 1024
HOST_C = r"""
#include <stdint.h>
/* retain_mutations_after_sequence_key, prepare_mutation_table_batches and prepare_table_mutations (ducklake/batches.rs:932-946, 727-758,
   1128-1226) over the windows, on one thread: ranges (3 words), batches (13 words), ops (4 words); counts = batches, ops, members, retained */
static uint64_t* op(uint64_t* o, uint32_t kind, uint32_t origin, uint64_t first, uint64_t n) { o[0] = kind | ((uint64_t)origin << 32); o[1] = first; o[2] = n; o[3] = ~0ull; return o + 4; }
void host_plan(const uint8_t* kind, const uint8_t* flags, const uint32_t* slots, const uint64_t* start, const uint64_t* commit, const uint64_t* ord, uint32_t slot,
               const uint64_t* passes, uint64_t n_passes, uint32_t has_wm, uint64_t wl, uint64_t wo, uint64_t seed, uint64_t* ranges, uint64_t* batches, uint64_t* ops,
               uint64_t* counts) {
  uint64_t nb = 0, members = 0, kept = 0;
  uint64_t* o = ops;
  for (uint64_t p = 0; p < n_passes; p++) {
    uint64_t mem[16]; uint32_t cat[16], n = 0;
    const uint64_t hi = passes[7 * p + 1];
    for (uint64_t i = passes[7 * p]; i <= hi; i++) {
      int take = 0;
      if (i < hi) {
        const uint8_t k = kind[i];
        if ((k == 'I' || k == 'U' || k == 'D') && slots[i] == slot) {
          members++;
          if (!has_wm || commit[i] > wl || (commit[i] == wl && ord[i] > wo)) {
            kept++; take = 1;
            mem[n] = i; cat[n] = k == 'I' ? 0u : k == 'D' ? 4u : (flags[i] & 4u) ? 3u : (flags[i] & 3u) ? 1u : 2u; n++;
          }
        }
      }
      if ((take && n == 16) || (i == hi && n)) {
        uint64_t* b = batches + 13 * nb; uint64_t* const o0 = o;
        uint32_t c[5] = {0, 0, 0, 0, 0};
        for (uint32_t m = 0; m < n;) {
          c[cat[m]]++;
          if (cat[m] == 0 || cat[m] == 4) {
            uint32_t e = m + 1;
            while (e < n && cat[e] == cat[m]) { c[cat[e]]++; e++; }
            o = op(o, cat[m] == 0 ? 0 : 1, cat[m] == 0 ? 0 : 1, mem[m], e - m); m = e;
          } else if (cat[m] == 3) { o = op(o, 2, 0, mem[m], 1); m++; }
          else { o = op(o, 1, cat[m] == 1 ? 2 : 3, mem[m], 1); o = op(o, 0, 0, mem[m], 1); m++; }
        }
        const uint64_t f = mem[0], l = mem[n - 1];
        ranges[3 * nb] = f; ranges[3 * nb + 1] = l + 1; ranges[3 * nb + 2] = seed;
        b[0] = f; b[1] = l + 1; b[2] = start[f]; b[3] = commit[l]; b[4] = commit[f]; b[5] = ord[f]; b[6] = ord[l]; b[7] = p; b[8] = (uint64_t)(o0 - ops) / 4;
        b[9] = n | ((uint64_t)((o - o0) / 4) << 32); b[10] = c[0] | ((uint64_t)c[1] << 32); b[11] = c[2] | ((uint64_t)c[3] << 32); b[12] = c[4];
        nb++; n = 0;
      }
    }
  }
  counts[0] = nb; counts[1] = (uint64_t)(o - ops) / 4; counts[2] = members; counts[3] = kept;
}
"""


def build_host(tmp):
    src, lib = os.path.join(tmp, "host_plan.c"), os.path.join(tmp, "host_plan.so")
    open(src, "w").write(HOST_C)
    subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-shared", "-fPIC", src, "-o", lib])
    L = C.CDLL(lib)
    L.host_plan.restype = None
    L.host_plan.argtypes = [C.c_void_p] * 6 + [C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64] + [C.c_void_p] * 4
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
    ne, seed = int(v.n_events), 0x6C62272E07BB0142
    out = {"workload": w.name, "batch_bytes": int(len(buf)), "events": ne, "slot": 0}
    names = [c[0] for c in w.schema_cols(w.tables[0])]
    objs = {k: b.duckdb(0, names, what=wh, on_device=True) for k, wh in (("tuples", abi.DL_TUPLES), ("predicates", abi.DL_PREDICATES), ("updates", abi.DL_UPDATES))}
    given = {k: (r if r.status == abi.RB_OK else None) for k, r in objs.items()}
    out["objects"] = {k: (r.n_rows if given[k] is not None else None) for k, r in objs.items()}

    # ---- (d), the download: the six header arrays come down
    def download():
        return (from_device(v.ev_kind, ne, np.uint8), from_device(v.ev_flags, ne, np.uint8), from_device(v.ev_schema_slot, 4 * ne, np.uint32),
                from_device(v.ev_start_lsn, 8 * ne, np.uint64), from_device(v.ev_commit_lsn, 8 * ne, np.uint64), from_device(v.ev_tx_ordinal, 8 * ne, np.uint64))
    t_down, hdr = timed(download, reps)
    out["d_headers_to_host"] = dict(t_down, bytes=30 * ne)
    kind, _, slot, _, commit, ordn = hdr
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
    sets = (("a_one_window", dev_put(one.reshape(-1)), 1, None, {}), ("b_outline_8MiB", ol, P, None, {}), ("c_window_per_event", dev_put(each.reshape(-1)), ne, None, {}),
            ("a_objects", dev_put(one.reshape(-1)), 1, None, given), ("a_watermark", dev_put(one.reshape(-1)), 1, (int(commit[mid]), int(ordn[mid])), {}))
    for tag, pd, npass, wm, ob in sets:
        kw = dict(n_passes=npass, watermark=wm, seed=seed, **ob)
        cnt = b.ducklake_plan(0, ptr(pd), batches_cap=0, ops_cap=0, on_device={"ranges": None}, **kw).info     # the counting call: no output at all
        if ob and cnt.status != abi.DLP_OK:                                  # an event the hand-off calls left to the host: the plan says so
            out[tag] = {"status": int(cnt.status), "event": int(cnt.event)}
            continue
        assert cnt.status == abi.DLP_OK, (tag, cnt.status, int(cnt.event))
        B, K = int(cnt.n_batches), int(cnt.n_ops)
        bufs = {"ranges": dev_zeros(3 * B), "batches": dev_zeros(13 * B), "ops": dev_zeros(4 * K)}
        where = {n: ptr(a) for n, a in bufs.items()}
        t, o = timed(lambda: b.ducklake_plan(0, ptr(pd), batches_cap=B, ops_cap=K, on_device=where, **kw), reps)
        out[tag] = dict(t, n_passes=npass, n_batches=B, n_ops=K, n_members=int(o.info.n_members), n_retained=int(o.info.n_retained))
        if ob:
            continue
        # ---- (d), the loops
        hp = to_host(pd, 7 * npass)
        hr, hb, ho, hn = np.zeros(3 * B + 3, dtype=np.uint64), np.zeros(13 * B + 13, dtype=np.uint64), np.zeros(4 * K + 8, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
        has_wm, wl, wo = (0, 0, 0) if wm is None else (1, wm[0], wm[1])
        ts = []
        for it in range(2 + reps):
            t0 = time.perf_counter()
            L.host_plan(*[a.ctypes.data for a in hdr], 0, hp.ctypes.data, npass, has_wm, wl, wo, seed, hr.ctypes.data, hb.ctypes.data, ho.ctypes.data, hn.ctypes.data)
            if it >= 2:
                ts.append(time.perf_counter() - t0)
        loop = round(sorted(ts)[len(ts) // 2] * 1e3, 4)
        same = (hn.tolist() == [B, K, int(o.info.n_members), int(o.info.n_retained)] and np.array_equal(to_host(bufs["ranges"], 3 * B), hr[:3 * B])
                and np.array_equal(to_host(bufs["batches"], 13 * B), hb[:13 * B]) and np.array_equal(to_host(bufs["ops"], 4 * K), ho[:4 * K]))
        out["d_" + tag[2:]] = {"host_loop_ms_median": loop, "download_plus_loop_ms": round(loop + t_down["ms_median"], 4), "equals_device": bool(same),
                               "device_over_host": round(t["ms_median"] / (loop + t_down["ms_median"]), 3)}
    for r in objs.values():
        r.close()
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
