// Device primitives every kernel source builds on: the DEV qualifier and the declarations the SIMT test emulator
// (tests/simt/simt.h) substitutes, LDS staging, byte readers, wave scans (DPP) and the generic workgroup scans. Nothing here
// knows the batch (DecParams) or a wire format. Everything is __forceinline__ and pointer based: called with a pointer derived
// from LDS the loads become ds_read, with a pointer into the input buffer global_load.
//
// No reference section is restated here: these are the machine-level pieces under the codecs (values.hip.h) and the frame
// machinery (frames.hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace etlg {

typedef uint8_t u8;

#define DEV __device__ __forceinline__
// The declarations the SIMT test emulator (tests/simt/simt.h) has to substitute: reconvergence markers, out-of-line device
// functions defined in this header, and the dynamic LDS window of a kernel.
#ifndef DEV_NOINLINE
#define DEV_NOINLINE __device__ __attribute__((noinline))
#endif
#ifndef ETLG_SCALAR_COPY   // a wave-uniform value in a scalar register of its own (not a member of a spilled register tuple)
#define ETLG_SCALAR_COPY(dst, src) asm volatile("s_mov_b32 %0, %1" : "=s"(dst) : "s"(src))
#endif
#ifndef ETLG_WAVE_PRIO   // s_setprio: the issue arbiter of a SIMD prefers the wave with the higher value (0..3)
#define ETLG_WAVE_PRIO(n) __builtin_amdgcn_s_setprio(n)
#endif
#ifndef ETLG_WAVE_JOIN   // reconvergence point of a divergent region with wave collectives inside: nothing on the GPU
#define ETLG_WAVE_JOIN() ((void)0)
#endif
#ifndef ETLG_CONST_AS      // constant address space (scalar loads of wave-uniform descriptors); the emulator has one address space
#define ETLG_CONST_AS __attribute__((address_space(4)))
#endif
#ifndef ETLG_DYNAMIC_LDS
#define ETLG_DYNAMIC_LDS(name) extern __shared__ __attribute__((aligned(16))) u8 name[]
#endif
// LDS-DMA (plan.hip): every lane moves 16 bytes from its own global address to (wave-uniform LDS base) + 16 * lane; the data
// never passes through VGPRs. The wave waits for its pieces with ETLG_VMEM_WAIT before it reads the window.
#ifndef ETLG_GLDS16
#define ETLG_GLDS16(g, l) __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)(g), (void __attribute__((address_space(3)))*)(l), 16, 0, 0)
#define ETLG_VMEM_WAIT() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
// One aligned ds_read_b32. Volatile keeps the compiler from fusing neighbouring dwords into a ds_read_b64 / b128 with 4-byte
// alignment, which the LDS serves at the misaligned rate (tools/ubench/lds_align.hip: 3.3x the cycles of an aligned read).
#define ETLG_LDS_AS __attribute__((address_space(3)))
#define ETLG_LDS_LD32(p) (*(volatile const ETLG_LDS_AS uint32_t*)(p))
#endif
// A pair of look-back words (plan.hip): ONE 16-byte load / store that bypasses the non-coherent caches (volatile: sc0 sc1), tracked by
// the compiler's own s_waitcnt bookkeeping (an inline-asm load would not be). Each 8-byte half validates itself (status bits),
// so nothing depends on the 16 bytes arriving as one.
#ifndef ETLG_LD_PAIR
typedef unsigned int etlg_v4u __attribute__((ext_vector_type(4)));
#define ETLG_LD_PAIR(ptr, a, l) do { const etlg_v4u t_ = *(const volatile __attribute__((address_space(1))) etlg_v4u*)(ptr); \
    (a) = ((unsigned long long)t_.y << 32) | t_.x; (l) = ((unsigned long long)t_.w << 32) | t_.z; } while (0)
#define ETLG_ST_PAIR(ptr, a, l) do { etlg_v4u t_; t_.x = (unsigned int)(a); t_.y = (unsigned int)((unsigned long long)(a) >> 32); t_.z = (unsigned int)(l); \
    t_.w = (unsigned int)((unsigned long long)(l) >> 32); *(volatile __attribute__((address_space(1))) etlg_v4u*)(ptr) = t_; } while (0)
#endif

// ------------------------------------------------------------- staging (k_fused, k_cells)
// Eight independent 16-byte loads per lane in flight before the first LDS store: one HBM round trip for a
// 113-byte-per-lane tile.
template <int NT>
DEV void stage_chunks(const uint8_t* in, uint8_t* stage, uint32_t a0, uint32_t full_end, uint32_t tid) {
  constexpr int W = 8;
  for (uint32_t c = a0 + 16 * tid; c < full_end; c += 16 * NT * W) {
    uint4 v[W];
#pragma unroll
    for (int k = 0; k < W; k++) {
      const uint32_t ck = c + 16 * NT * k;
      v[k] = make_uint4(0, 0, 0, 0);
      if (ck < full_end) v[k] = *(const uint4*)(in + ck);
    }
#pragma unroll
    for (int k = 0; k < W; k++) {
      const uint32_t ck = c + 16 * NT * k;
      if (ck < full_end) *(uint4*)(stage + (ck - a0)) = v[k];
    }
  }
}

// ------------------------------------------------------------- byte helpers
DEV uint32_t ld_be32(const u8* p) { uint32_t v; __builtin_memcpy(&v, p, 4); return __builtin_bswap32(v); }
DEV uint64_t ld_be64(const u8* p) { uint64_t v; __builtin_memcpy(&v, p, 8); return __builtin_bswap64(v); }
DEV uint32_t ld_be16(const u8* p) { return ((uint32_t)p[0] << 8) | p[1]; }
DEV uint32_t pad4(uint32_t n) { return (n + 3u) & ~3u; }

// Unaligned 4 / 8 byte loads built from ALIGNED dword loads + v_alignbyte. LDS serves a misaligned
// ds_read_b32 / b64 lane by lane (measured: ~1k cycles per wave-wide access with random alignment),
// while aligned dword reads run at full rate. These read up to the end of the last dword touched,
// i.e. at most 3 (ldu32) / 3 (ldu64) bytes beyond the value plus the alignment slack below it.
DEV uint32_t ldu32(const u8* p) {
  const uint32_t sh = (uint32_t)(uintptr_t)p & 3u;
  const uint32_t* q = (const uint32_t*)(p - sh);
  return __builtin_amdgcn_alignbyte(q[1], q[0], sh);
}
DEV uint64_t ldu64(const u8* p) {
  const uint32_t sh = (uint32_t)(uintptr_t)p & 3u;
  const uint32_t* q = (const uint32_t*)(p - sh);
  const uint32_t w0 = q[0], w1 = q[1], w2 = q[2];
  return __builtin_amdgcn_alignbyte(w1, w0, sh) | ((uint64_t)__builtin_amdgcn_alignbyte(w2, w1, sh) << 32);
}
DEV bool is_digit(uint32_t c) { return c - '0' < 10u; }
DEV uint32_t lower(uint32_t c) { return (c - 'A' < 26u) ? c + 32 : c; }

DEV void st64(uint32_t* w, uint64_t v) { w[0] = (uint32_t)v; w[1] = (uint32_t)(v >> 32); }

// Sequential byte reader. With `over` (the caller guarantees 7 readable bytes past any index it
// asks for: LDS-staged tiles keep 16 bytes of slack) it fetches 8 bytes per load, i.e. one memory
// round trip per 8 characters instead of one per character; without it every access is a byte load.
struct ByteWin {
  const u8* s; bool over;
  uint32_t base = 0x80000000u; uint64_t w = 0;
  DEV uint32_t at(uint32_t i) {  // ascending access
    if (!over) return s[i];
    uint32_t d = i - base;
    if (d >= 8u) { base = i; __builtin_memcpy(&w, s + i, 8); d = 0; }
    return (uint32_t)(w >> (8 * d)) & 0xFFu;
  }
  DEV uint32_t at_rev(uint32_t i) {  // descending access
    if (!over) return s[i];
    if (i - base >= 8u) { base = i >= 7u ? i - 7u : 0u; __builtin_memcpy(&w, s + base, 8); }
    return (uint32_t)(w >> (8 * (i - base))) & 0xFFu;
  }
};

// ------------------------------------------------------------- wave scans
// Inclusive scan over the 64 lanes of a wave with DPP (row_shr 1/2/4/8 inside each row of 16, then
// row_bcast:15 into rows 1 and 3 and row_bcast:31 into rows 2 and 3): six VALU instructions, no LDS
// crossbar round trips (a __shfl_up ladder is six dependent ds_bpermute, ~100 cycles each).
// op(older, newer); `idn` is its left identity (lanes without a source read it).
#define ETLG_DPP(ctrl, rmask) { const uint32_t t_ = (uint32_t)__builtin_amdgcn_update_dpp((int)idn, (int)v, ctrl, rmask, 0xF, false); v = op(t_, v); }
template <class F>
DEV uint32_t wave_scan_incl(uint32_t v, F op, uint32_t idn) {
  ETLG_DPP(0x111, 0xF) ETLG_DPP(0x112, 0xF) ETLG_DPP(0x114, 0xF) ETLG_DPP(0x118, 0xF) ETLG_DPP(0x142, 0xA) ETLG_DPP(0x143, 0xC)
  return v;
}
#undef ETLG_DPP
DEV uint32_t wave_scan_add(uint32_t v) { return wave_scan_incl(v, [](uint32_t a, uint32_t b) { return a + b; }, 0u); }
DEV uint32_t wave_scan_max(uint32_t v) { return wave_scan_incl(v, [](uint32_t a, uint32_t b) { return a > b ? a : b; }, 0u); }
DEV uint32_t wave_last(uint32_t v) { return (uint32_t)__builtin_amdgcn_readlane((int)v, 63); }  // lane 63 of an inclusive scan = the wave total

// ------------------------------------------------------------- block scans
DEV uint32_t seg_combine(uint32_t a, uint32_t b) {  // bit31 = "a Begin was seen", low bits = count since
  return (b & 0x80000000u) ? b : ((a & 0x80000000u) | ((a + b) & 0x7FFFFFFFu));
}

template <int OP>  // 0 sum, 1 max, 2 segmented count
DEV uint32_t op_apply(uint32_t a, uint32_t b) {
  if (OP == 0) return a + b;
  if (OP == 1) return a > b ? a : b;
  return seg_combine(a, b);
}

// Inclusive scan across the 256-lane workgroup. `lds` = 4 words of scratch.
// Returns the inclusive value; *total = workgroup aggregate.
template <int OP>
DEV uint32_t block_scan_incl(uint32_t v, uint32_t* lds, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    uint32_t t = __shfl_up(v, d, 64);
    if (lane >= d) v = op_apply<OP>(t, v);
  }
  if (lane == 63) lds[wave] = v;
  __syncthreads();
  uint32_t pre = 0;
  bool have = false;
  for (int w = 0; w < wave; w++) { pre = have ? op_apply<OP>(pre, lds[w]) : lds[w]; have = true; }
  if (have) v = op_apply<OP>(pre, v);
  if (total) {
    uint32_t t = lds[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); w++) t = op_apply<OP>(t, lds[w]);
    *total = t;
  }
  __syncthreads();
  return v;
}

DEV uint64_t block_sum64(uint64_t v, uint64_t* lds) {  // returns the workgroup total
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  if (lane == 0) lds[wave] = v;
  __syncthreads();
  uint64_t t = 0;
  for (int w = 0; w < (int)(blockDim.x >> 6); w++) t += lds[w];
  __syncthreads();
  return t;
}

// Exclusive 64-bit sum scan over the workgroup; *total = aggregate.
DEV uint64_t block_scan_excl64(uint64_t v, uint64_t* lds, uint64_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    uint64_t t = __shfl_up(inc, d, 64);
    if (lane >= d) inc += t;
  }
  if (lane == 63) lds[wave] = inc;
  __syncthreads();
  uint64_t pre = 0, tot = 0;
  for (int w = 0; w < (int)(blockDim.x >> 6); w++) { if (w < wave) pre += lds[w]; tot += lds[w]; }
  __syncthreads();
  if (total) *total = tot;
  return pre + inc - v;
}

// "The tiles' sums become the sums in front of each tile": an in-place exclusive sum scan of the n 64-bit words v[0], v[stride],
// v[2 stride], ... by ONE workgroup of 256, in chunks of 256. Returns the total to every lane. `lds` = 4 words of scratch.
DEV uint64_t carry_scan64(unsigned long long* v, uint32_t n, uint32_t stride, uint64_t* lds) {
  uint64_t carry = 0;
  for (uint32_t t0 = 0; t0 < n; t0 += 256) {   // (uniform trip count: every lane takes part in every scan)
    const uint32_t t = t0 + threadIdx.x;
    const bool on = t < n;
    uint64_t tot;
    const uint64_t ex = block_scan_excl64(on ? v[(uint64_t)t * stride] : 0ull, lds, &tot);
    if (on) v[(uint64_t)t * stride] = carry + ex;
    carry += tot;
  }
  return carry;
}

}  // namespace etlg
