"""etlg_batch_outline on HBM-resident batches, warm, medians of 20 wall times after 3 warm calls: 64 MiB of cfg2 and cfg3 and the
three-table cfg5 stream. Per workload:
  (a) one write_events range (no cuts); (b) the ranges of etlg_batch_cuts at the reference's default budget, BatchConfig::DEFAULT_MAX_BYTES
      = 8 MiB (crates/etl-config/src/shared/pipeline.rs:68), the cuts left on the device; (c) a cut behind every event (budget 1).
      Device cuts, device outputs, caps as large as the counts of a first, counting call. The cuts come from a device copy of the hints with
      bit 63 cleared (cfg3 holds partial Updates, whose hints are INCOMPLETE);
  (d) what a driver does today on the same batch: ev_kind, ev_flags, ev_schema_slot and ev_table_id copied to host memory (10 bytes per
      event), then the loop as one thread runs it — the C below, compiled here with the system compiler into a temporary directory —
      for the passes, their ends, the touched words, the census and the truncate entries' counts (the entries themselves would be one more
      download: they lie in the arena). Its counts and passes must equal the device's;
  (e) the existing kernels of finish.hip on cfg2, since the unit was recompiled: etlg_batch_size_hints to device memory and
      etlg_batch_cuts at 8 MiB, 64 KiB and budget 1.
`--tree DIR` imports the package from another checkout (built there): a tree without etlg_batch_outline times (e) alone — run against
the parent commit's tree in the same job, its medians are the yardstick for this tree's. The output — this text as `#` lines, then one
JSON line per workload — is committed as it is printed (profiles/outline_probe_mi355x.txt)."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

TREE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = TREE
if "--tree" in sys.argv:
    TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
sys.path.insert(0, TREE)
import etl_amd  # noqa: E402,F401
import numpy as np  # noqa: E402

EMU = os.environ.get("ETLG_SIMT_RUN") == "1"   # a rehearsal against the SIMT emulator build (tests/simt): device memory is host memory, times mean nothing
if not EMU:
    import torch  # noqa: E402

from etl_amd import abi, synth  # noqa: E402
from etl_amd.decoder import Batch, Decoder  # noqa: E402

DEFAULT_BUDGET = 8 * 1024 * 1024
HOST_C = r"""
#include <stdint.h>
#include <string.h>
/* the write_events loop (clickhouse/core.rs:1063-1164) over the ranges of `cuts`, on one thread: passes (7 words each), their ends, the
   touched words, the census (12 words per slot); counts[0..4) = passes, truncate entries, Relations, rows */
void host_outline(const uint8_t* kind, const uint8_t* flags, const uint32_t* slot, const uint32_t* table, uint64_t n, const uint64_t* cuts, uint64_t n_cuts,
                  uint32_t n_slots, uint64_t* passes, uint64_t* ends, uint64_t* touched, uint64_t* census, uint64_t* counts) {
  const uint64_t W = (n_slots + 63) / 64;
  uint64_t np = 0, nt = 0, nr = 0, nrow = 0, lo = 0;
  for (uint32_t s = 0; s < n_slots; s++) for (int c = 0; c < 12; c++) census[12 * s + c] = c < 6 ? 0 : ~0ull;
  for (uint64_t r = 0; r <= n_cuts; r++) {
    const uint64_t hi = r < n_cuts ? cuts[r] : n;
    uint64_t i = lo;
    while (i < hi) {
      uint64_t* p = passes + 7 * np;
      uint64_t* t = touched + W * np;
      memset(t, 0, W * 8);
      p[0] = i; p[4] = r; p[5] = nt;
      for (; i < hi && kind[i] != 'T' && kind[i] != 'R'; i++) {
        const uint8_t k = kind[i];
        if (k != 'I' && k != 'U' && k != 'D') continue;
        const uint32_t s = slot[i], ok = flags[i] & 3u;
        const int c = k == 'I' ? 0 : k == 'U' ? ((flags[i] & 4u) ? 2 : 1) : ok == 1 ? 3 : ok == 2 ? 4 : 5;
        nrow++;
        if (s >= n_slots) continue;
        t[s >> 6] |= 1ull << (s & 63);
        census[12 * s + c]++;
        if (census[12 * s + 6 + c] == ~0ull) census[12 * s + 6 + c] = i;
      }
      p[1] = i;
      for (; i < hi && kind[i] == 'R'; i++) nr++;
      p[2] = i;
      for (; i < hi && kind[i] == 'T'; i++) nt += table[i];
      p[3] = ends[np] = i; p[6] = nt - p[5];
      np++;
    }
    lo = hi;
  }
  counts[0] = np; counts[1] = nt; counts[2] = nr; counts[3] = nrow;
}
"""


def build_host(tmp):
    src, lib = os.path.join(tmp, "host_outline.c"), os.path.join(tmp, "host_outline.so")
    open(src, "w").write(HOST_C)
    subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-shared", "-fPIC", src, "-o", lib])
    L = C.CDLL(lib)
    L.host_outline.restype = None
    L.host_outline.argtypes = [C.c_void_p] * 4 + [C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32] + [C.c_void_p] * 5
    return L


def size_model():
    sys.path.insert(0, HERE)
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


def ptr(a):
    return a.ctypes.data if EMU else a.data_ptr()


def to_host(a, n):
    return (a[:n].copy() if EMU else a[:n].cpu().numpy()).view(np.uint64)


def from_device(p, nbytes, dtype):
    """`nbytes` of the batch's device memory at `p`, copied to host memory."""
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


def hints_to_device(d, b, m, t):
    rc = d.L.etlg_batch_size_hints(d.h, b.h, C.byref(m), abi.F_OUTPUT_ON_DEVICE, C.c_void_p(ptr(t)))
    assert rc == abi.OK, rc


def wal(L, mk, reps, small, existing):
    w = mk()
    buf, offs = w.fill((1 << 20) if small else (64 << 20))
    d = Decoder(0)
    w.register(d, ready=not w.cfg.emit_relations)
    b = d.decode(buf, offs, flags=abi.F_OUTPUT_ON_DEVICE)
    assert b.rc == 0, b.error
    v = b.view()
    ne, ns, m = int(v.n_events), int(v.n_slots), size_model()
    W = (ns + 63) // 64
    out = {"workload": w.name, "tree": os.path.basename(TREE) if "--tree" in sys.argv else ".", "batch_bytes": int(len(buf)), "events": ne, "slots": ns}
    dev_hints, cuts_dev = dev_zeros(ne + 1), dev_zeros(ne + 1)
    t_hints, _ = timed(lambda: hints_to_device(d, b, m, dev_hints), reps)
    if existing:
        out["e_size_hints_device"] = t_hints
        for tag, budget in (("e_cuts_8MiB", DEFAULT_BUDGET), ("e_cuts_64KiB", 64 << 10), ("e_cuts_budget_1", 1)):
            t, r = timed(lambda: b.cuts(m, budget, cap=ne, on_device=ptr(cuts_dev)), reps)
            out[tag] = dict(t, n_cuts=int(r[1].n_cuts))
    if not hasattr(Batch, "outline"):
        b.close(); d.close()
        return out
    done = dev_hints & 0x7FFFFFFFFFFFFFFF                                  # the completed copy: bit 63 cleared
    sync()
    # ---- (d), the download: the four header arrays come down
    def download():
        return (from_device(v.ev_kind, ne, np.uint8), from_device(v.ev_flags, ne, np.uint8), from_device(v.ev_schema_slot, 4 * ne, np.uint32),
                from_device(v.ev_table_id, 4 * ne, np.uint32))
    t_down, (kind, flags, slot, table) = timed(download, reps)
    out["d_headers_to_host"] = dict(t_down, bytes=10 * ne)
    for tag, budget in (("a_one_range", None), ("b_cuts_8MiB", DEFAULT_BUDGET), ("c_cut_per_event", 1)):
        k = 0
        if budget is not None:
            _, ci = b.cuts(None, budget, hints=ptr(done), cap=ne, on_device=ptr(cuts_dev))
            k = int(ci.n_cuts)
            assert int(ci.stop_event) == ne
        cuts = dict(cuts=ptr(cuts_dev), n_cuts=k) if k else {}
        cnt = b.outline(passes_cap=0, trunc_cap=0, on_device={"slots": None}, **cuts).info    # the counting call: no output at all
        assert cnt.status == abi.OL_OK
        P, K = int(cnt.n_passes), int(cnt.n_trunc)
        bufs = {"passes": dev_zeros(7 * P), "ends": dev_zeros(P), "touched": dev_zeros(W * P), "truncates": dev_zeros(2 * K), "slots": dev_zeros(12 * ns)}
        where = {n: ptr(a) for n, a in bufs.items()}
        t, o = timed(lambda: b.outline(passes_cap=P, trunc_cap=K, on_device=where, **cuts), reps)
        out[tag] = dict(t, n_cuts=k, n_passes=P, n_trunc=K, n_relations=int(o.info.n_relations), n_rows=int(o.info.n_rows), n_ranges=int(o.info.n_ranges))
        # ---- (d), the loop
        hc = to_host(cuts_dev, k)
        hp, he, ht, hs, hn = (np.zeros(7 * (ne + 1), dtype=np.uint64), np.zeros(ne + 1, dtype=np.uint64), np.zeros(W * (ne + 1), dtype=np.uint64),
                              np.zeros(12 * ns + 1, dtype=np.uint64), np.zeros(4, dtype=np.uint64))
        ts = []
        for it in range(2 + reps):
            t0 = time.perf_counter()
            L.host_outline(kind.ctypes.data, flags.ctypes.data, slot.ctypes.data, table.ctypes.data, ne, hc.ctypes.data if k else None, k, ns,
                           hp.ctypes.data, he.ctypes.data, ht.ctypes.data, hs.ctypes.data, hn.ctypes.data)
            if it >= 2:
                ts.append(time.perf_counter() - t0)
        loop = round(sorted(ts)[len(ts) // 2] * 1e3, 4)
        same = (hn.tolist() == [P, K, int(o.info.n_relations), int(o.info.n_rows)] and np.array_equal(to_host(bufs["passes"], 7 * P), hp[:7 * P])
                and np.array_equal(to_host(bufs["ends"], P), he[:P]) and np.array_equal(to_host(bufs["touched"], W * P), ht[:W * P])
                and np.array_equal(to_host(bufs["slots"], 12 * ns), hs[:12 * ns]))
        out["d_" + tag[2:]] = {"host_loop_ms_median": loop, "download_plus_loop_ms": round(loop + t_down["ms_median"], 4), "equals_device": bool(same),
                               "device_over_host": round(t["ms_median"] / (loop + t_down["ms_median"]), 3)}
    b.close(); d.close()
    return out


def main():
    reps = int(os.environ.get("ETLG_PROBE_REPS", "20"))
    small = os.environ.get("ETLG_PROBE_SMALL") == "1"                       # a rehearsal size
    if "--tree" not in sys.argv:
        for line in __doc__.split("\n"):
            print(("# " + line).rstrip())
    with tempfile.TemporaryDirectory() as tmp:
        L = build_host(tmp)
        for mk in (synth.cfg2,) if "--tree" in sys.argv else (synth.cfg2, synth.cfg3, synth.cfg5):
            print(json.dumps(wal(L, mk, reps, small, mk is synth.cfg2)), flush=True)


if __name__ == "__main__":
    main()
