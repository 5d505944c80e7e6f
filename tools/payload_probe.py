"""etlg_batch_payload on HBM-resident 64 MiB batches (cfg2, cfg3), warm, medians of 20 wall times after 3 warm calls. The input stays
where the decode left it (device memory, ETLG_F_INPUT_ON_DEVICE), ev_bytes and the sums go to device memory, eight histogram bounds:
  (a) one range (no cuts);
  (b) the cuts etlg_batch_cuts leaves on the device at the reference's default budget, 8 MiB (crates/etl-config/src/shared/pipeline.rs:68);
  (c) the cuts at budget 1: one range per event and an empty last one;
  (d) (a) with the input in pinned host memory instead: the call uploads the 64 MiB itself;
  (e) what a host does instead, one thread, the frames in pinned memory: the C below walks every frame (tag, cell tags and lengths:
      calculate_tuple_bytes, codec/event.rs:261-297), adds the received bytes, rows and buckets per kind and leaves the bytes per frame;
      a second loop adds bytes and rows per kind over the events of every range. The second loop is given the event -> frame map for
      nothing (ev_bytes and ev_kind as the device produced them): the host leg is the lower bound of a host implementation. Its received
      totals and its sums must equal the device's.
The existing calls of finish.hip are timed by tools/cuts_probe.py (its `--tree` form runs the parent commit's tree). The output — this
text as `#` lines, then one JSON line per workload — is committed as it is printed (profiles/payload_probe_mi355x.txt)."""
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
BOUNDS = [16, 64, 256, 1024, 4096, 16384, 65536, 1 << 20]
HOST_C = r"""
#include <stdint.h>
#include <string.h>
static uint32_t be32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return __builtin_bswap32(v); }
/* value bytes of one tuple (i16 count, then 'n' | 'u' | 't' i32 len bytes); returns the cursor behind it, 0 when it does not parse */
static const uint8_t* tuple_bytes(const uint8_t* c, const uint8_t* e, uint64_t* vb) {
  if (e - c < 2) return 0;
  uint32_t n = ((uint32_t)c[0] << 8) | c[1];
  c += 2;
  for (uint32_t i = 0; i < n; i++) {
    if (c >= e) return 0;
    uint8_t t = *c++;
    if (t == 'n' || t == 'u') continue;
    if ((t != 't' && t != 'b') || e - c < 4) return 0;
    uint32_t len = be32(c);
    c += 4;
    if ((uint64_t)(e - c) < len) return 0;
    *vb += len;
    c += len;
  }
  return c;
}
/* every frame: received bytes[3], rows[3], hist[3][nb + 1]; fbytes[f] = the message's value bytes. Returns the row messages seen. */
uint64_t host_walk(const uint8_t* in, const uint32_t* offs, uint64_t nframes, const uint64_t* bounds, uint32_t nb, uint64_t* bytes, uint64_t* rows,
                   uint64_t* hist, uint32_t* fbytes) {
  uint64_t seen = 0;
  for (uint64_t f = 0; f < nframes; f++) {
    const uint8_t* fr = in + offs[f];
    const uint8_t* e = in + offs[f + 1];
    fbytes[f] = 0;
    if (e - fr < 36 || fr[5] != 'w') continue;
    const uint8_t tag = fr[30];
    const int k = tag == 'I' ? 0 : tag == 'U' ? 1 : tag == 'D' ? 2 : -1;
    if (k < 0) continue;
    const uint8_t* c = fr + 35;
    uint64_t vb = 0;
    uint8_t t = *c++;
    if (t == 'K' || t == 'O') { c = tuple_bytes(c, e, &vb); if (!c) continue; if (tag == 'U') { if (c >= e) continue; t = *c++; } }
    if (t == 'N' && !tuple_bytes(c, e, &vb)) continue;
    bytes[k] += vb; rows[k]++; seen++;
    uint32_t j = 0;
    while (j < nb && vb > bounds[j]) j++;
    hist[(uint64_t)k * (nb + 1) + j]++;
    fbytes[f] = (uint32_t)vb;
  }
  return seen;
}
/* sums[r] = bytes[4], rows[4] of the events [cuts[r - 1], cuts[r]), the last range up to n */
void host_sums(const uint8_t* ev_kind, const uint32_t* ev_bytes, uint64_t n, const uint64_t* cuts, uint64_t n_cuts, uint64_t* sums) {
  uint64_t i = 0;
  for (uint64_t r = 0; r <= n_cuts; r++) {
    const uint64_t end = r < n_cuts ? cuts[r] : n;
    uint64_t* s = sums + 8 * r;
    memset(s, 0, 64);
    for (; i < end; i++) {
      const uint8_t t = ev_kind[i];
      const int k = t == 'I' ? 0 : t == 'U' ? 1 : t == 'D' ? 2 : -1;
      if (k >= 0) { s[k] += ev_bytes[i]; s[4 + k]++; }
    }
  }
}
"""


def build_host(tmp):
    src, lib = os.path.join(tmp, "host_payload.c"), os.path.join(tmp, "host_payload.so")
    open(src, "w").write(HOST_C)
    subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-shared", "-fPIC", src, "-o", lib])
    L = C.CDLL(lib)
    L.host_walk.restype = C.c_uint64
    L.host_walk.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.host_sums.restype = None
    L.host_sums.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
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


def dev_put(a):
    raw = np.frombuffer(np.ascontiguousarray(a).tobytes() + b"\0" * (8 + (-a.nbytes) % 8), dtype=np.uint8).copy()
    return raw if EMU else torch.from_numpy(raw).cuda()


def ptr(a):
    return a.ctypes.data if EMU else a.data_ptr()


def dev_get(p, n, dtype):
    nb = n * np.dtype(dtype).itemsize
    if EMU:
        return np.frombuffer((C.c_uint8 * nb).from_address(p), dtype=dtype).copy()
    return abi.device_tensor(p, nb, 0).cpu().numpy().view(dtype)


def med(ts):
    ts = sorted(ts)
    return {"ms_median": round(ts[len(ts) // 2] * 1e3, 4), "ms_min": round(ts[0] * 1e3, 4), "ms_max": round(ts[-1] * 1e3, 4)}


def timed(call, reps, warm=3, fence=True):
    ts, r = [], None
    for it in range(warm + reps):
        if fence:
            sync()
        t0 = time.perf_counter()
        r = call()
        if fence:
            sync()
        if it >= warm:
            ts.append(time.perf_counter() - t0)
    return med(ts), r


def wal(L, mk, reps, small):
    w = mk()
    buf, offs = w.fill((1 << 20) if small else (64 << 20))
    buf, offs = np.ascontiguousarray(buf), np.ascontiguousarray(offs, dtype=np.uint32)
    nf = len(offs) - 1
    d = Decoder(0)
    w.register(d)
    dbuf, doffs = dev_put(buf), dev_put(offs)
    sync()
    b = d.decode_device(ptr(dbuf), len(buf), ptr(doffs), nf, flags=abi.F_OUTPUT_ON_DEVICE | abi.F_NO_CONTROL)
    assert b.rc == 0, b.error
    ne, m = int(b.view().n_events), size_model()
    out = {"workload": w.name, "batch_bytes": int(len(buf)), "frames": nf, "events": ne}
    ev_dev = dev_put(np.zeros(ne, dtype=np.uint32))
    cuts_dev = dev_put(np.zeros(ne + 1, dtype=np.uint64))
    sums_dev = dev_put(np.zeros((ne + 2) * 8, dtype=np.uint64))
    hints = dev_put(np.zeros(ne + 1, dtype=np.uint64))
    assert d.L.etlg_batch_size_hints(d.h, b.h, C.byref(m), abi.F_OUTPUT_ON_DEVICE, C.c_void_p(ptr(hints))) == abi.OK
    sync()
    h64 = hints.view(np.uint64) if EMU else hints.view(torch.int64)
    h64 &= 0x7FFFFFFFFFFFFFFF                                              # bit 63 cleared in place: partial Updates do not stop the cuts' walk
    sync()
    legs = (("a_one_range", None), ("b_cuts_8MiB", DEFAULT_BUDGET), ("c_cuts_budget_1", 1))
    host_pin = d.host_alloc(len(buf) + 64)
    host_pin[:len(buf)] = buf
    host_cuts = {}
    for tag, budget in legs:
        nc = 0
        if budget is not None:
            _, info = b.cuts(None, budget, hints=ptr(hints), cap=ne, on_device=ptr(cuts_dev))
            nc = int(info.n_cuts)
        call = lambda: b.payload(ptr(dbuf), ptr(doffs), cuts=ptr(cuts_dev) if nc else None, n_cuts=nc, bounds=BOUNDS, nbytes=len(buf), nframes=nf,  # noqa: E731
                                 on_device=(ptr(ev_dev), ptr(sums_dev)))
        t, p = timed(call, reps)
        assert p.info.status == abi.PM_OK and list(p.info.received_bytes)[:3] == list(b.view().payload_bytes)
        out[tag] = dict(t, ranges=nc + 1)
        host_cuts[tag] = (dev_get(ptr(cuts_dev), nc, np.uint64), dev_get(ptr(sums_dev), (nc + 1) * 8, np.uint64), p)
    t, p = timed(lambda: b.payload(host_pin[:len(buf)], offs, bounds=BOUNDS, on_device=(ptr(ev_dev), ptr(sums_dev))), reps)
    out["d_one_range_host_input"] = t
    # ---- (e) one host thread
    ev_bytes, ev_kind = dev_get(ptr(ev_dev), ne, np.uint32), dev_get(b.view().ev_kind, ne, np.uint8)
    bnd = np.array(BOUNDS, dtype=np.uint64)
    fbytes = np.zeros(nf, dtype=np.uint32)

    def walk():
        by, rows, hist = np.zeros(3, dtype=np.uint64), np.zeros(3, dtype=np.uint64), np.zeros((3, len(BOUNDS) + 1), dtype=np.uint64)
        L.host_walk(host_pin.ctypes.data, offs.ctypes.data, nf, bnd.ctypes.data, len(BOUNDS), by.ctypes.data, rows.ctypes.data, hist.ctypes.data, fbytes.ctypes.data)
        return by, rows, hist
    t_walk, (by, rows, hist) = timed(walk, reps, warm=2, fence=False)
    ref = host_cuts["a_one_range"][2]
    same = (by.tolist() == list(ref.info.received_bytes)[:3] and rows.tolist() == list(ref.info.received_rows)[:3] and np.array_equal(hist, ref.hist[:3]))
    out["e_host_walk"] = dict(t_walk, equals_device=bool(same))
    for tag, _ in legs:
        cuts, dev_sums, _ = host_cuts[tag]
        sums = np.zeros((len(cuts) + 1) * 8, dtype=np.uint64)
        t_sum, _ = timed(lambda: L.host_sums(ev_kind.ctypes.data, ev_bytes.ctypes.data, ne, cuts.ctypes.data if len(cuts) else None, len(cuts), sums.ctypes.data),
                         reps, warm=2, fence=False)
        total = round(t_walk["ms_median"] + t_sum["ms_median"], 4)
        out["e_" + tag[2:]] = {"host_sums_ms_median": t_sum["ms_median"], "walk_plus_sums_ms": total, "equals_device": bool(np.array_equal(sums, dev_sums)),
                               "device_over_host": round(out[tag]["ms_median"] / total, 3)}
    d.host_free(host_pin)
    b.close(); d.close()
    return out


def main():
    reps = int(os.environ.get("ETLG_PROBE_REPS", "20"))
    small = os.environ.get("ETLG_PROBE_SMALL") == "1"                       # a rehearsal size
    for line in __doc__.split("\n"):
        print(("# " + line).rstrip())
    with tempfile.TemporaryDirectory() as tmp:
        L = build_host(tmp)
        for mk in (synth.cfg2, synth.cfg3):
            print(json.dumps(wal(L, mk, reps, small)), flush=True)


if __name__ == "__main__":
    main()
