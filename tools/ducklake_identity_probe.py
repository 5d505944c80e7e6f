"""etlg_ducklake_fingerprints on HBM-resident 64 MiB batches (cfg2, cfg3) and on the type-matrix table, warm, medians of 20 calls:
  * the call with ONE range over the batch and with ranges of 1 000 events (wall time: the call ends in its one device stop);
  * beside it the three etlg_batch_duckdb calls whose records it consumes (device output);
  * what it replaces: the download of the same records (bytes, row_offsets, row_event, col_ends into pinned memory) plus a
    single-thread FNV-1a walk over the same stream on the host — the C below, compiled here with the system compiler into a temporary
    directory; it hashes record by record as the reference does (no stream is assembled) and its fingerprints must EQUAL the
    device's, for the one range and for every range of 1 000 events: a parity check at the size the figures are taken at.
The output — this text as `#` lines, then one JSON line per workload — is committed as it is printed
(profiles/ducklake_identity_probe_mi355x.txt). ms_median: 3 warm calls, then the median of ETLG_PROBE_REPS (20) wall times; the host
walk: 2 warm runs, then the median of as many.
The kernel split comes from separate runs, one per workload so that a kernel's average belongs to one workload:
`ETLG_PROBE_ONLY=<cfg2|cfg3|type_matrix> ETLG_PROBE_REPS=3 rocprofv3 --kernel-trace --stats --output-format csv -- python
tools/ducklake_identity_probe.py`; their kernel_stats files are profiles/ducklake_identity_kernel_stats_<workload>.csv (the k_fp_*
rows hold the launches of both range sets)."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import etl_amd  # noqa: E402,F401
import numpy as np  # noqa: E402
import torch  # noqa: E402

from etl_amd import abi, synth  # noqa: E402
from etl_amd.decoder import Decoder  # noqa: E402

HOST_C = r"""
#include <stddef.h>
#include <stdint.h>
typedef struct { const uint64_t* ev; const int64_t* off; const uint8_t* bytes; uint64_t n; } recs;
static uint64_t fnv(uint64_t h, const uint8_t* p, size_t n) { for (size_t i = 0; i < n; i++) h = (h ^ p[i]) * 0x100000001b3ull; return h; }
static uint64_t u64(uint64_t h, uint64_t v) { uint8_t b[8]; for (int i = 0; i < 8; i++) b[i] = (uint8_t)(v >> (8 * i)); return fnv(h, b, 8); }
static uint64_t str(uint64_t h, const uint8_t* p, size_t n) { const uint8_t ff = 0xFF; return fnv(fnv(h, p, n), &ff, 1); }
static uint64_t rec(uint64_t h, const recs* r, uint64_t i) { return str(h, r->bytes + r->off[i], (size_t)(r->off[i + 1] - r->off[i])); }
static uint64_t find(const recs* r, uint64_t* at, uint64_t e) { while (*at < r->n && r->ev[*at] < e) ++*at; return *at < r->n && r->ev[*at] == e ? *at : ~0ull; }
/* the fingerprint of events [first, end) from `seed`; *missing = the first slot event without a record it needs (else ~0) */
uint64_t host_fingerprint(const uint8_t* kind, const uint8_t* flags, const uint32_t* slot_of, const uint64_t* start, const uint64_t* commit, uint32_t slot, uint32_t copy,
                          const recs* t, const recs* p, const recs* u, const uint32_t* ends, const uint32_t* name_len, uint32_t n_cols,
                          uint64_t first, uint64_t end, uint64_t seed, uint64_t* missing) {
  uint64_t h = seed, it = 0, ip = 0, iu = 0;
  *missing = ~0ull;
  for (uint64_t e = first; e < end; e++) {
    const uint8_t k = kind[e];
    if ((k != 'I' && k != 'U' && k != 'D') || slot_of[e] != slot) continue;
    const int partial = k == 'U' && (flags[e] & 4);
    const uint64_t a = (k != 'D' && !partial) ? find(t, &it, e) : 0, b = ((copy || k != 'I') && !partial) ? find(p, &ip, e) : 0, c = partial ? find(u, &iu, e) : 0;
    if (a == ~0ull || b == ~0ull || c == ~0ull) { if (*missing == ~0ull) *missing = e; continue; }
    if (!copy) { h = u64(h, start[e]); h = u64(h, commit[e]); }
    if (copy) { h = rec(h, p, b); h = rec(h, t, a); }
    else if (k == 'I') { h = str(h, (const uint8_t*)"insert", 6); h = rec(h, t, a); }
    else if (k == 'D') { h = str(h, (const uint8_t*)"delete", 6); h = rec(h, p, b); }
    else if (!partial) { if (flags[e] & 3) h = str(h, (const uint8_t*)"update", 6); else h = str(h, (const uint8_t*)"replace", 7); h = rec(h, p, b); h = rec(h, t, a); }
    else {
      h = str(h, (const uint8_t*)"update", 6); h = rec(h, u, c + 1); h = u64(h, n_cols);
      const uint32_t* en = ends + c * n_cols; const uint8_t* s = u->bytes + u->off[c];
      uint32_t prev = 0; int firstp = 1;
      for (uint32_t q = 0; q < n_cols; q++) if (en[q] > prev) {
        const uint32_t skip = (firstp ? 0u : 2u) + name_len[q];
        h = u64(h, q); h = str(h, s + prev + skip, en[q] - prev - skip); firstp = 0; prev = en[q];
      }
    }
  }
  return h;
}
"""


class Recs(C.Structure):
    _fields_ = [("ev", C.c_void_p), ("off", C.c_void_p), ("bytes", C.c_void_p), ("n", C.c_uint64)]


def build_host(tmp):
    src, lib = os.path.join(tmp, "host_fnv.c"), os.path.join(tmp, "host_fnv.so")
    open(src, "w").write(HOST_C)
    subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-shared", "-fPIC", src, "-o", lib])
    L = C.CDLL(lib)
    L.host_fingerprint.restype = C.c_uint64
    L.host_fingerprint.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_uint32] + [C.POINTER(Recs)] * 3 + [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64,
                                                                                                      C.POINTER(C.c_uint64)]
    return L


EMU = os.environ.get("ETLG_SIMT_RUN") == "1"   # a rehearsal against the SIMT emulator build (tests/simt): device memory is host memory, times mean nothing


def sync():
    if not EMU:
        torch.cuda.synchronize()


def med(ts):
    return round(sorted(ts)[len(ts) // 2] * 1e3, 3)


def down(ptr, nbytes, dst=None):
    """`nbytes` of device memory into pinned host memory (a tensor the caller may pass again)."""
    if dst is None:
        dst = torch.empty(max(nbytes, 1), dtype=torch.uint8)
        dst = dst if EMU else dst.pin_memory()
    if nbytes and EMU:
        dst[:nbytes] = torch.frombuffer((C.c_uint8 * nbytes).from_address(ptr), dtype=torch.uint8)
    elif nbytes:
        dst[:nbytes].copy_(abi.device_tensor(ptr, nbytes, 0), non_blocking=True)
    return dst


def one(L, name, prime, buf, offs, names, reps, warm=3):
    d = Decoder(0)
    prime(d)
    b = d.decode(buf, offs, flags=abi.F_OUTPUT_ON_DEVICE | abi.F_NO_CONTROL)
    assert b.rc == 0, b.error
    v = b.view()
    ne, nc = int(v.n_events), len(names)
    out = {"workload": name, "batch_bytes": int(len(buf)), "events": ne}
    whats = (("tuples", abi.DL_TUPLES), ("predicates", abi.DL_PREDICATES), ("updates", abi.DL_UPDATES))
    objs = {k: b.duckdb(0, names, what=w, on_device=True) for k, w in whats}
    for k, r in objs.items():
        out[k] = {"status": r.status, "rows": r.n_rows, "host_rows": int(r.view.n_host_rows), "bytes": int(r.view.n_bytes)}
    if any(r.status != abi.RB_OK for r in objs.values()):
        out["error"] = "a record object came back as NEEDS_HOST: nothing to hash"
        return out
    seed = 0xCBF29CE484222325
    sets = {"one_range": [(0, ne, seed)], "ranges_of_1000": [(k, min(k + 1000, ne), seed ^ k) for k in range(0, ne, 1000)]}
    call = {k: (lambda rs=rs: b.ducklake_fingerprints(0, names, rs, objs["tuples"], objs["predicates"], objs["updates"])) for k, rs in sets.items()}
    for k, w in whats:
        call[k] = (lambda w=w: b.duckdb(0, names, what=w, on_device=True))
    wall = {k: [] for k in call}
    got = {}
    for it in range(warm + reps):
        for k, f in call.items():
            sync()
            t0 = time.perf_counter()
            r = f()
            sync()
            if it >= warm:
                wall[k].append(time.perf_counter() - t0)
            if k in sets:
                got[k] = r
            else:
                r.close()
    for k in call:
        out.setdefault(k, {})["ms_median"] = med(wall[k])
    for k in sets:
        out[k].update(ranges=len(sets[k]), status=int(got[k][1].status), host_event=int(got[k][1].host_event))
    # ---- what the call replaces: download + host walk
    sizes = [(r.view.bytes, int(r.view.n_bytes)) for r in objs.values()] + [(r.view.row_offsets, 8 * (r.n_rows + 1)) for r in objs.values()] + \
            [(r.view.row_event, 8 * r.n_rows) for r in objs.values()] + [(objs["updates"].col_ends_ptr(), 4 * objs["updates"].n_rows * nc)]
    pinned = [down(p, n) for p, n in sizes]
    sync()
    ts = []
    for it in range(warm + reps):
        sync()
        t0 = time.perf_counter()
        for (p, n), dst in zip(sizes, pinned):
            down(p, n, dst)
        sync()
        if it >= warm:
            ts.append(time.perf_counter() - t0)
    out["download"] = {"ms_median": med(ts), "bytes": sum(n for _, n in sizes)}
    ev = [down(p, n) for p, n in ((v.ev_kind, ne), (v.ev_flags, ne), (v.ev_schema_slot, 4 * ne), (v.ev_start_lsn, 8 * ne), (v.ev_commit_lsn, 8 * ne))]
    sync()
    recs = [Recs(pinned[6 + i].data_ptr(), pinned[3 + i].data_ptr(), pinned[i].data_ptr(), r.n_rows) for i, r in enumerate(objs.values())]
    name_len = np.array([len(n.encode()) + n.count('"') + 2 + 3 for n in names], dtype=np.uint32)
    miss = C.c_uint64()

    def host(rs):
        return [L.host_fingerprint(ev[0].data_ptr(), ev[1].data_ptr(), ev[2].data_ptr(), ev[3].data_ptr(), ev[4].data_ptr(), 0, 0, C.byref(recs[0]), C.byref(recs[1]),
                                   C.byref(recs[2]), pinned[9].data_ptr(), name_len.ctypes.data, nc, a, z, s, C.byref(miss)) for a, z, s in rs]
    ts, hashed = [], {}
    for it in range(2 + reps):
        t0 = time.perf_counter()
        hashed["one_range"] = host(sets["one_range"])
        if it >= 2:
            ts.append(time.perf_counter() - t0)
    hashed["ranges_of_1000"] = host(sets["ranges_of_1000"])
    stream_bytes = sum(out[k]["bytes"] for k, _ in whats)
    out["host_fnv"] = {"ms_median": med(ts), "record_bytes": stream_bytes, "GBps": round(stream_bytes / (med(ts) * 1e-3) / 1e9, 3)}
    out["host_total_ms"] = round(out["download"]["ms_median"] + out["host_fnv"]["ms_median"], 3)
    for k in sets:
        if out[k]["status"] == abi.RB_OK:
            out[k]["equals_host"] = [int(x) for x in got[k][0]] == hashed[k]
            out[k]["speedup_vs_download_plus_host"] = round(out["host_total_ms"] / out[k]["ms_median"], 2)
    out["fingerprint"] = "%016x" % int(got["one_range"][0][0]) if out["one_range"]["status"] == abi.RB_OK else None
    for r in objs.values():
        r.close()
    b.close(); d.close()
    return out


def main():
    reps = int(os.environ.get("ETLG_PROBE_REPS", "20"))
    small = os.environ.get("ETLG_PROBE_SMALL") == "1"                           # a rehearsal size
    only = os.environ.get("ETLG_PROBE_ONLY", "")
    for line in __doc__.split("\n"):
        print(("# " + line).rstrip())
    with tempfile.TemporaryDirectory() as tmp:
        L = build_host(tmp)
        for key, mk in (("cfg2", synth.cfg2), ("cfg3", synth.cfg3)):
            if only and only != key:
                continue
            w = mk()
            buf, offs = w.fill((1 << 20) if small else (64 << 20))
            print(json.dumps(one(L, w.name if hasattr(w, "name") else mk.__name__, w.register, buf, offs, [c[0] for c in w.schema_cols(w.tables[0])], reps)), flush=True)
        if only and only != "type_matrix":
            return
        buf, offs = synth.type_matrix_stream(400 if small else 44000, mix=True)
        print(json.dumps(one(L, "type_matrix", synth.type_matrix_register, buf, offs, [c[0] for c in synth.TYPE_MATRIX_COLS], reps)), flush=True)


if __name__ == "__main__":
    main()
