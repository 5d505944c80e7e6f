// etlg_ducklake_fingerprints (include/etlg.h): the FNV-1a-64 batch identities of the DuckLake sink
// (BatchIdHasher, crates/etl-destinations/src/ducklake/batches.rs:260-289; build_mutation_batch_identity :1402-1446,
// build_copy_batch_identity :1449-1464, hash_partial_table_row_ref :1562-1594) over the records etlg_batch_duckdb left in HBM.
//
// FNV-1a is h' = (h ^ b) * P, one dependent multiply per byte. Two facts take the chain apart:
//   1. the low byte of h' depends only on the low byte of h: l' = ((l ^ b) * 0xB3) & 0xFF, per input byte a permutation of 0..255.
//      A run of bytes is, for the low byte, ONE 256-entry permutation; permutations compose.
//   2. h ^ b == h + d with d = (l ^ b) - l. With the low bytes known a run of n bytes is the affine map h -> h * P^n + C
//      (C' = (C + d) * P); affine maps compose.
// Seven kernels of its own and the existing scan (three), plain launches in stream order, no workgroup waits for another:
//   k_fp_plan    per event: what it hashes (the stream walker fp_walk, counting) and which records; events that lack one
//   (scan)       etlg_k_scan_lens: where every event's bytes begin
//   k_fp_write   the stream itself, fp_walk again with a wave writing — event order, slot events only, back to back
//   k_fp_bounds  per range: its bytes [begin, end) of the stream
//   k_fp_perm    (A) per piece — a chunk of kFpChunk stream bytes cut at the ranges' bounds — the low-byte permutation: 256 lanes, one
//                candidate each, walk the piece's bytes out of LDS (uniform addresses: broadcast reads); 24-bit multiplies only
//   k_fp_low     (B) per range: the permutations of its pieces composed in order from the seed's low byte -> every piece's entering byte
//   k_fp_affine  (C) per piece: one lane lays the low bytes down on the chunk's 64-byte grid, 256 lanes take 64 bytes each to (P^n, C) — the
//                64-bit multiplies, one lane-byte each, never 256 per byte — and one lane folds the 256 maps
//   k_fp_fold    (D) per range: the pieces' maps folded in order from the seed
// Piece (chunk c, range i) has id c + i: along the stream a next piece has a larger chunk or a larger range, so ids are unique, and the
// pieces of one range are consecutive.
#include "../../include/etlg.h"
#include "dev_types.h"
#include "device.hip.h"

extern "C" void etlg_k_scan_lens(const uint32_t* lens, uint64_t n, unsigned long long* blk, int64_t* offsets, hipStream_t st);   // columns.hip

namespace etlg {

constexpr uint32_t kFpChunk = 16384;   // stream bytes per chunk (LDS image of k_fp_perm / k_fp_affine)
constexpr uint32_t kFpSub = kFpChunk / 256;   // bytes a lane of k_fp_affine takes
constexpr uint32_t kFpEvWave = 16;     // events a wave of k_fp_write writes, one after the other (64 per workgroup)
constexpr uint64_t kFnvPrime = 0x100000001b3ull;
constexpr uint32_t kFpNone = 0xFFFFFFFFu;
enum : uint32_t { FP_NONE = 0, FP_INSERT, FP_DELETE, FP_UPDATE, FP_REPLACE, FP_PARTIAL, FP_COPY, FP_HOST };

// The 8-bit step: a 24-bit multiply. Only the low byte of the result means anything (and only the low byte of `l` is read: the low
// byte of a product depends on the low bytes of its factors), so the chain needs no mask between steps.
// Written as the instruction v_mul_u32_u24: for __umul24 the compiler, seeing that only the low byte of the chain is consumed, emits
// v_mul_lo_u32, the quarter-rate 32-bit multiply. (What the instruction saves over that was not measured.)
DEV uint32_t fp_mul24(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t r;
  asm("v_mul_u32_u24 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
#else
  return (a & 0xFFFFFFu) * (b & 0xFFFFFFu);
#endif
}
DEV uint32_t fp_low(uint32_t l, uint32_t b) { return fp_mul24(l ^ b, 0xB3u); }

// a `str` hashed through Hasher::write: its bytes, then 0xFF — for the tags, packed little-endian into one word (at most 7 + 1 bytes)
constexpr uint64_t fp_tag(const char* s, uint32_t n) {
  uint64_t v = 0xFFull << (8 * n);
  for (uint32_t i = 0; i < n; i++) v |= (uint64_t)(uint8_t)s[i] << (8 * i);
  return v;
}

// the record of event e, if the object has one (row_event ascends); `pair`: two consecutive records (ETLG_DL_UPDATES)
DEV uint32_t fp_find(const FpRecs& r, uint64_t e, bool pair) {
  uint64_t lo = 0, hi = r.n_rows;
  while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (r.row_event[mid] < e) lo = mid + 1; else hi = mid; }
  if (lo >= r.n_rows || r.row_event[lo] != e) return kFpNone;
  if (pair && (lo + 1 >= r.n_rows || r.row_event[lo + 1] != e)) return kFpNone;
  return (uint32_t)lo;
}

struct FpCount {   // the walker's sink that only counts
  uint64_t n = 0;
  DEV void raw(const u8*, uint64_t k) { n += k; }
  DEV void lit(uint64_t, uint32_t k) { n += k; }
};
struct FpWave {    // ... that writes, the 64 lanes of a wave side by side (every lane walks the same event)
  u8* dst; uint32_t lane;
  DEV void raw(const u8* p, uint64_t k) { for (uint64_t i = lane; i < k; i += 64) dst[i] = p[i]; dst += k; }
  DEV void lit(uint64_t v, uint32_t k) { if (lane < k) dst[lane] = (u8)(v >> (8 * lane)); dst += k; }
};

// THE STREAM WALKER: the bytes one slot event feeds the hasher (include/etlg.h has the table; tests/ducklake_identity.py is its twin).
// A u64 / usize is 8 little-endian bytes, a str its bytes and 0xFF.
template <class S>
DEV void fp_walk(const FpJob& j, uint64_t e, uint32_t tag, uint32_t t, uint32_t p, uint32_t u, S& s) {
  if (tag == FP_NONE || tag == FP_HOST) return;
  auto rec = [&](const FpRecs& r, uint32_t i) {
    const int64_t a = r.row_offsets[i];
    s.raw(r.bytes + a, (uint64_t)(r.row_offsets[i + 1] - a));
    s.lit(0xFF, 1);
  };
  if (tag != FP_COPY) { s.lit(j.ev_start[e], 8); s.lit(j.ev_commit[e], 8); }
  switch (tag) {
    case FP_INSERT: s.lit(fp_tag("insert", 6), 7); rec(j.t, t); break;
    case FP_DELETE: s.lit(fp_tag("delete", 6), 7); rec(j.p, p); break;
    case FP_UPDATE: s.lit(fp_tag("update", 6), 7); rec(j.p, p); rec(j.t, t); break;
    case FP_REPLACE: s.lit(fp_tag("replace", 7), 8); rec(j.p, p); rec(j.t, t); break;
    case FP_COPY: rec(j.p, p); rec(j.t, t); break;
    default: {   // FP_PARTIAL: record u the SET clause, u + 1 the predicate; hash_partial_table_row_ref over the SET clause's pieces
      s.lit(fp_tag("update", 6), 7); rec(j.u, u + 1); s.lit(j.n_cols, 8);
      const uint32_t* ends = j.u_ends + (uint64_t)u * j.n_cols;
      const u8* b = j.u.bytes + j.u.row_offsets[u];
      uint32_t prev = 0;
      bool first = true;
      for (uint32_t c = 0; c < j.n_cols; c++) {
        const uint32_t en = ends[c];
        if (en <= prev) continue;   // a MISSING cell: no piece
        const uint32_t skip = (first ? 0u : 2u) + j.name_len[c];   // ", " and `"name" = `
        if (en - prev >= skip) { s.lit(c, 8); s.raw(b + prev + skip, en - prev - skip); s.lit(0xFF, 1); }
        first = false; prev = en;
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_fp_plan(FpJob j) {
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= j.n_events) return;
  uint32_t tag = FP_NONE, t = kFpNone, p = kFpNone, u = kFpNone;
  const uint32_t kind = j.ev_kind[e];
  if ((kind == 'I' || kind == 'U' || kind == 'D') && j.ev_slot[e] == j.slot) {
    const uint32_t fl = j.ev_flags[e];
    if (kind == 'U' && (fl & ETLG_FLAG_PARTIAL)) {
      u = fp_find(j.u, e, true);
      tag = u != kFpNone ? FP_PARTIAL : FP_HOST;
    } else {
      const bool need_t = kind != 'D', need_p = j.copy || kind != 'I';
      if (need_t) t = fp_find(j.t, e, false);
      if (need_p) p = fp_find(j.p, e, false);
      if ((need_t && t == kFpNone) || (need_p && p == kFpNone)) tag = FP_HOST;
      else tag = j.copy ? FP_COPY : kind == 'I' ? FP_INSERT : kind == 'D' ? FP_DELETE : (fl & 3u) != ETLG_OLD_NONE ? FP_UPDATE : FP_REPLACE;
    }
  }
  uint32_t* pl = j.plan + 4 * e;
  pl[0] = tag; pl[1] = t; pl[2] = p; pl[3] = u;
  FpCount s;
  fp_walk(j, e, tag, t, p, u, s);
  j.lens[e] = (uint32_t)s.n;
  if (tag == FP_HOST) {   // only inside a range: the last range that begins at or before e
    uint32_t lo = 0, hi = j.n_ranges;
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (j.ranges[3 * (uint64_t)mid] <= e) lo = mid + 1; else hi = mid; }
    if (lo && e < j.ranges[3 * (uint64_t)(lo - 1) + 1]) atomicMin(j.result, (unsigned long long)e);
  }
}

__global__ __launch_bounds__(256) void k_fp_write(FpJob j) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t e0 = ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * kFpEvWave;
  for (uint32_t k = 0; k < kFpEvWave; k++) {
    const uint64_t e = e0 + k;
    if (e >= j.n_events) break;
    const uint32_t* pl = j.plan + 4 * e;
    const uint32_t tag = pl[0];
    if (tag == FP_NONE || tag == FP_HOST) continue;
    FpWave s{j.stream + j.offs[e], lane};
    fp_walk(j, e, tag, pl[1], pl[2], pl[3], s);
  }
}

__global__ __launch_bounds__(256) void k_fp_bounds(FpJob j) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= j.n_ranges) return;
  j.bounds[2 * (uint64_t)i] = (uint64_t)j.offs[j.ranges[3 * (uint64_t)i]];
  j.bounds[2 * (uint64_t)i + 1] = (uint64_t)j.offs[j.ranges[3 * (uint64_t)i + 1]];
}

// a chunk's bytes into LDS, 16 per lane and step (the stream's buffer ends in slack: the last load may pass the stream's end)
DEV void fp_stage(const FpJob& j, u8* buf, uint64_t c0, uint64_t c1) {
  for (uint32_t i = threadIdx.x * 16; c0 + i < c1; i += 256 * 16) *(uint4*)(buf + i) = *(const uint4*)(j.stream + c0 + i);
  __syncthreads();
}
// the first range that ends behind c0 (the ranges ascend and are disjoint: so do their bounds)
DEV uint32_t fp_first_range(const FpJob& j, uint64_t c0) {
  uint32_t lo = 0, hi = j.n_ranges;
  while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (j.bounds[2 * (uint64_t)mid + 1] <= c0) lo = mid + 1; else hi = mid; }
  return lo;
}

__global__ __launch_bounds__(256) void k_fp_perm(FpJob j) {
  __shared__ __attribute__((aligned(16))) u8 buf[kFpChunk];
  const uint64_t total = (uint64_t)j.offs[j.n_events], c0 = (uint64_t)blockIdx.x * kFpChunk;
  if (c0 >= total) return;
  const uint64_t c1 = c0 + kFpChunk < total ? c0 + kFpChunk : total;
  fp_stage(j, buf, c0, c1);
  for (uint32_t i = fp_first_range(j, c0); i < j.n_ranges; i++) {
    const uint64_t rb = j.bounds[2 * (uint64_t)i], re = j.bounds[2 * (uint64_t)i + 1];
    if (rb >= c1) break;
    const uint64_t a = rb > c0 ? rb : c0, b = re < c1 ? re : c1;
    if (a >= b) continue;
    uint32_t k = (uint32_t)(a - c0);
    const uint32_t kb = (uint32_t)(b - c0);
    uint32_t l = threadIdx.x;   // this lane's candidate
    auto word = [&](uint32_t w) { l = fp_low(l, w & 0xFFu); l = fp_low(l, (w >> 8) & 0xFFu); l = fp_low(l, (w >> 16) & 0xFFu); l = fp_low(l, w >> 24); };
    for (; k < kb && (k & 15u); k++) l = fp_low(l, buf[k]);
    for (; k + 16 <= kb; k += 16) {   // one 16-byte LDS read (the same address in every lane) per sixteen steps
      const uint4 w = *(const uint4*)(buf + k);
      word(w.x); word(w.y); word(w.z); word(w.w);
    }
    for (; k < kb; k++) l = fp_low(l, buf[k]);
    j.perm[((uint64_t)blockIdx.x + i) * 256 + threadIdx.x] = (u8)l;
  }
}

__global__ __launch_bounds__(256) void k_fp_low(FpJob j) {
  constexpr uint32_t kRows = 64;
  __shared__ __attribute__((aligned(16))) u8 rows[kRows * 256];
  const uint32_t i = blockIdx.x;
  const uint64_t rb = j.bounds[2 * (uint64_t)i], re = j.bounds[2 * (uint64_t)i + 1];
  if (rb >= re) return;
  const uint64_t cf = rb / kFpChunk, np = (re - 1) / kFpChunk - cf + 1, id0 = cf + i;
  uint32_t l = (uint32_t)(j.ranges[3 * (uint64_t)i + 2] & 0xFFu);   // (lane 0 carries it)
  for (uint64_t base = 0; base < np; base += kRows) {
    const uint32_t nb = np - base < kRows ? (uint32_t)(np - base) : kRows;
    const uint4* src = (const uint4*)(j.perm + (id0 + base) * 256);   // the pieces of a range are consecutive
    for (uint32_t q = threadIdx.x; q < nb * 16; q += 256) ((uint4*)rows)[q] = src[q];
    __syncthreads();
    if (threadIdx.x == 0)
      for (uint32_t k = 0; k < nb; k++) { j.lin[id0 + base + k] = (u8)l; l = rows[k * 256 + l]; }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_fp_affine(FpJob j) {
  __shared__ __attribute__((aligned(16))) u8 buf[kFpChunk];
  __shared__ u8 ck[256];
  __shared__ uint64_t m_a[256], m_c[256];
  const uint64_t total = (uint64_t)j.offs[j.n_events], c0 = (uint64_t)blockIdx.x * kFpChunk;
  if (c0 >= total) return;
  const uint64_t c1 = c0 + kFpChunk < total ? c0 + kFpChunk : total;
  fp_stage(j, buf, c0, c1);
  for (uint32_t i = fp_first_range(j, c0); i < j.n_ranges; i++) {
    const uint64_t rb = j.bounds[2 * (uint64_t)i], re = j.bounds[2 * (uint64_t)i + 1];
    if (rb >= c1) break;
    const uint64_t a = rb > c0 ? rb : c0, b = re < c1 ? re : c1;
    if (a >= b) continue;
    const uint64_t id = (uint64_t)blockIdx.x + i;
    const uint32_t ka = (uint32_t)(a - c0), kb = (uint32_t)(b - c0);
    // Sub-pieces lie on the CHUNK's 64-byte grid, not the piece's: lane t owns the chunk's bytes [64 t, 64 t + 64) that fall into the
    // piece, so every whole sub-piece is four aligned 16-byte LDS reads with no test between its bytes; only a piece's first and last
    // sub-piece can be partial and go byte by byte.
    const uint32_t s0 = ka / kFpSub, s1 = (kb - 1) / kFpSub;
    if (threadIdx.x == 0) {   // the low byte every sub-piece is entered with
      uint32_t l = j.lin[id];
      auto word = [&](uint32_t w) { l = fp_low(l, w & 0xFFu); l = fp_low(l, (w >> 8) & 0xFFu); l = fp_low(l, (w >> 16) & 0xFFu); l = fp_low(l, w >> 24); };
      for (uint32_t t = s0; t <= s1; t++) {
        ck[t] = (u8)l;
        uint32_t k = t * kFpSub > ka ? t * kFpSub : ka;
        const uint32_t e = (t + 1) * kFpSub < kb ? (t + 1) * kFpSub : kb;
        if (e - k == kFpSub) {
          for (uint32_t q = 0; q < kFpSub; q += 16) { const uint4 w = *(const uint4*)(buf + k + q); word(w.x); word(w.y); word(w.z); word(w.w); }
        } else {
          for (; k < e; k++) l = fp_low(l, buf[k]);
        }
      }
    }
    __syncthreads();
    {
      const uint32_t t = threadIdx.x;
      uint64_t pa = 1, pc = 0;
      if (t >= s0 && t <= s1) {
        uint32_t l = ck[t], k = t * kFpSub > ka ? t * kFpSub : ka;
        const uint32_t e = (t + 1) * kFpSub < kb ? (t + 1) * kFpSub : kb;
        auto step = [&](uint32_t by) {
          const uint32_t x = l ^ by;
          pc = (pc + (uint64_t)(int64_t)((int32_t)x - (int32_t)l)) * kFnvPrime;
          pa *= kFnvPrime;
          l = fp_mul24(x, 0xB3u) & 0xFFu;
        };
        auto word = [&](uint32_t w) { step(w & 0xFFu); step((w >> 8) & 0xFFu); step((w >> 16) & 0xFFu); step(w >> 24); };
        if (e - k == kFpSub) {
          for (uint32_t q = 0; q < kFpSub; q += 16) { const uint4 w = *(const uint4*)(buf + k + q); word(w.x); word(w.y); word(w.z); word(w.w); }
        } else {
          for (; k < e; k++) step(buf[k]);
        }
      }
      m_a[t] = pa; m_c[t] = pc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint64_t pa = 1, pc = 0;
      for (uint32_t q = s0; q <= s1; q++) { pc = pc * m_a[q] + m_c[q]; pa *= m_a[q]; }
      j.maps[2 * id] = pa; j.maps[2 * id + 1] = pc;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_fp_fold(FpJob j) {
  __shared__ uint64_t m[2 * 256];
  const uint32_t i = blockIdx.x;
  const uint64_t rb = j.bounds[2 * (uint64_t)i], re = j.bounds[2 * (uint64_t)i + 1];
  uint64_t h = j.ranges[3 * (uint64_t)i + 2];
  if (rb < re) {
    const uint64_t cf = rb / kFpChunk, np = (re - 1) / kFpChunk - cf + 1, id0 = cf + i;
    for (uint64_t base = 0; base < np; base += 256) {
      const uint32_t nb = np - base < 256 ? (uint32_t)(np - base) : 256u;
      for (uint32_t q = threadIdx.x; q < 2 * nb; q += 256) m[q] = j.maps[2 * (id0 + base) + q];
      __syncthreads();
      if (threadIdx.x == 0)
        for (uint32_t k = 0; k < nb; k++) h = h * m[2 * k] + m[2 * k + 1];
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) j.result[1 + (uint64_t)i] = h;
}

}  // namespace etlg

// blk: (ceil(n_events / 256) + 1) x u64 scan scratch. n_events and n_ranges are not zero.
extern "C" void etlg_k_fingerprints(const etlg::FpJob* jv, unsigned long long* blk, hipStream_t st) {
  using namespace etlg;
  const FpJob j = *jv;
  const uint32_t rblk = (j.n_ranges + 255) / 256;
  hipLaunchKernelGGL(k_fp_plan, dim3((uint32_t)((j.n_events + 255) / 256)), dim3(256), 0, st, j);
  etlg_k_scan_lens(j.lens, j.n_events, blk, (int64_t*)j.offs, st);
  hipLaunchKernelGGL(k_fp_write, dim3((uint32_t)((j.n_events + 4 * kFpEvWave - 1) / (4 * kFpEvWave))), dim3(256), 0, st, j);
  hipLaunchKernelGGL(k_fp_bounds, dim3(rblk), dim3(256), 0, st, j);
  hipLaunchKernelGGL(k_fp_perm, dim3(j.n_chunks), dim3(256), 0, st, j);
  hipLaunchKernelGGL(k_fp_low, dim3(j.n_ranges), dim3(256), 0, st, j);
  hipLaunchKernelGGL(k_fp_affine, dim3(j.n_chunks), dim3(256), 0, st, j);
  hipLaunchKernelGGL(k_fp_fold, dim3(j.n_ranges), dim3(256), 0, st, j);
}
extern "C" uint32_t etlg_k_fp_chunk_bytes(void) { return etlg::kFpChunk; }
