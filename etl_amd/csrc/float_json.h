// float4 / float8 -> the text serde_json writes for them (serialize_f32 / serialize_f64: ryu's `format32` / `format64`), shared by
// the NDJSON row kernels (rowformats.hip.h, nd_row) and a host-side unit test (tests/test_float_json.py compiles this header with g++ and
// checks it against libstdc++'s std::to_chars on tens of millions of bit patterns).
//
// ryu and serde_json are crates.io dependencies of the reference and are not vendored with it: what follows RESTATES their published
// source. The digits are Ryu's shortest round-trip digits (U. Adams, "Ryu: fast float-to-string conversion", PLDI 2018; ryu's
// d2s.rs `d2d`), the layout is ryu's pretty/mod.rs. With the shortest digits d (n of them) and value = d x 10^e, kk = n + e:
//   e >= 0 and kk <= 16 (f32: 13)   the digits, e zeros, ".0"             1000000000000000.0
//   0 < kk <= 16 (13)               a '.' after the first kk digits       12.34
//   -5 < kk <= 0 (f32: -6 < kk)     "0.", -kk zeros, the digits           0.00001
//   otherwise                       "De<kk-1>" (n = 1) / "D.DDDe<kk-1>"   1e16, 1.5e-7, 1.234e33
// exponent without '+' or leading zeros, zero "0.0", negative zero "-0.0", a leading '-' for negative values. NaN / inf never get
// here (the Snowflake sink refuses them first).
// f32 runs through the same d2d as f64 (its mantissa and exponent ranges are inside f64's; the 125-bit tables only get more accurate
// for a 26-bit mv than the paper's bound needs for a 55-bit one), which yields the same shortest, nearest, ties-to-even digits as f2s.
#pragma once
#include <stdint.h>
#include "float_fast.h"
#include "ryu_table.h"

namespace etlg {

ETLG_FD uint32_t ryu_pow5bits(int32_t e) { return (uint32_t)(((uint32_t)e * 1217359u) >> 19) + 1u; }   // bitlength(5^e), 0 <= e <= 3528
ETLG_FD uint32_t ryu_log10_pow2(int32_t e) { return (uint32_t)e * 78913u >> 18; }                   // floor(log10(2^e)), 0 <= e <= 1650
ETLG_FD uint32_t ryu_log10_pow5(int32_t e) { return (uint32_t)e * 732923u >> 20; }                  // floor(log10(5^e)), 0 <= e <= 2620
ETLG_FD bool ryu_mult_pow5(uint64_t v, uint32_t p) {   // 5^p divides v (v != 0)
  uint32_t c = 0;
  while (v % 5u == 0u) { v /= 5u; c++; }
  return c >= p;
}
ETLG_FD bool ryu_mult_pow2(uint64_t v, uint32_t p) { return (v & ((1ull << p) - 1u)) == 0; }   // p < 64
// (m x mul) >> j for a 128-bit mul {hi, lo} and 64 <= j < 192
ETLG_FD uint64_t ryu_mul_shift(uint64_t m, const uint64_t* mul, int32_t j) {
  uint64_t l0, h0, l1, h1;
  mul64x64(m, mul[1], l0, h0);
  mul64x64(m, mul[0], l1, h1);
  const uint64_t lo = l1 + h0, hi = h1 + (lo < l1 ? 1u : 0u);   // (m x lo) >> 64 + m x hi
  const uint32_t s = (uint32_t)(j - 64);
  if (s == 0) return lo;
  if (s >= 64) return hi >> (s - 64);
  return (lo >> s) | (hi << (64 - s));
}

// d2d: the shortest decimal d x 10^e10 that reads back as the float (mantissa without the hidden bit, biased exponent)
ETLG_FD void ryu_d2d(uint64_t ieee_m, uint32_t ieee_e, uint32_t mbits, int32_t bias, uint64_t& out, int32_t& e10) {
  int32_t e2;
  uint64_t m2;
  if (ieee_e == 0) { e2 = 1 - bias - (int32_t)mbits - 2; m2 = ieee_m; }
  else { e2 = (int32_t)ieee_e - bias - (int32_t)mbits - 2; m2 = (1ull << mbits) | ieee_m; }
  const bool accept = (m2 & 1u) == 0;
  const uint64_t mv = 4 * m2;
  const uint32_t mm_shift = ieee_m != 0 || ieee_e <= 1;
  uint64_t vr, vp, vm;
  bool vm_tz = false, vr_tz = false;
  if (e2 >= 0) {
    const uint32_t q = ryu_log10_pow2(e2) - (e2 > 3 ? 1u : 0u);
    e10 = (int32_t)q;
    const int32_t k = 125 + (int32_t)ryu_pow5bits((int32_t)q) - 1;
    const int32_t i = -e2 + (int32_t)q + k;
    vr = ryu_mul_shift(4 * m2, kRyuPow5Inv[q], i);
    vp = ryu_mul_shift(4 * m2 + 2, kRyuPow5Inv[q], i);
    vm = ryu_mul_shift(4 * m2 - 1 - mm_shift, kRyuPow5Inv[q], i);
    if (q <= 21) {   // only one of mp, mv, mm can be a multiple of 5
      if (mv % 5u == 0u) vr_tz = ryu_mult_pow5(mv, q);
      else if (accept) vm_tz = ryu_mult_pow5(mv - 1 - mm_shift, q);
      else vp -= ryu_mult_pow5(mv + 2, q) ? 1u : 0u;
    }
  } else {
    const uint32_t q = ryu_log10_pow5(-e2) - (-e2 > 1 ? 1u : 0u);
    e10 = (int32_t)q + e2;
    const int32_t i = -e2 - (int32_t)q;
    const int32_t k = (int32_t)ryu_pow5bits(i) - 125;
    const int32_t j = (int32_t)q - k;
    vr = ryu_mul_shift(4 * m2, kRyuPow5[i], j);
    vp = ryu_mul_shift(4 * m2 + 2, kRyuPow5[i], j);
    vm = ryu_mul_shift(4 * m2 - 1 - mm_shift, kRyuPow5[i], j);
    if (q <= 1) {    // mv = 4 m2 has at least two trailing zero bits
      vr_tz = true;
      if (accept) vm_tz = mm_shift == 1; else --vp;
    } else if (q < 63) {
      vr_tz = ryu_mult_pow2(mv, q);
    }
  }
  int32_t removed = 0;
  uint32_t last = 0;
  if (vm_tz || vr_tz) {   // the general case (rare)
    while (vp / 10 > vm / 10) {
      vm_tz &= vm % 10 == 0;
      vr_tz &= last == 0;
      last = (uint32_t)(vr % 10);
      vr /= 10; vp /= 10; vm /= 10;
      removed++;
    }
    if (vm_tz) {
      while (vm % 10 == 0) {
        vr_tz &= last == 0;
        last = (uint32_t)(vr % 10);
        vr /= 10; vp /= 10; vm /= 10;
        removed++;
      }
    }
    if (vr_tz && last == 5 && vr % 2 == 0) last = 4;   // round to even when the exact value is ...50..0
    out = vr + (((vr == vm && (!accept || !vm_tz)) || last >= 5) ? 1u : 0u);
  } else {
    bool up = false;
    while (vp / 10 > vm / 10) {
      up = vr % 10 >= 5;
      vr /= 10; vp /= 10; vm /= 10;
      removed++;
    }
    out = vr + ((vr == vm || up) ? 1u : 0u);
  }
  e10 += removed;
}

ETLG_FD uint32_t ryu_dec_len(uint64_t v) { uint32_t n = 1; while (v >= 10) { v /= 10; n++; } return n; }

// The text of a finite float (bits: f32 in the low 32 bits when is32) into `s` (put(u8)); returns its length. `s` may be a counter.
template <class S>
ETLG_FD uint32_t float_json(S& s, uint64_t bits, bool is32) {
  const uint32_t mbits = is32 ? 23u : 52u, ebits = is32 ? 8u : 11u;
  const bool neg = ((bits >> (mbits + ebits)) & 1u) != 0;
  const uint64_t m = bits & ((1ull << mbits) - 1u);
  const uint32_t e = (uint32_t)(bits >> mbits) & ((1u << ebits) - 1u);
  uint32_t len = 0;
  auto put = [&](uint32_t c) { s.put((uint8_t)c); len++; };
  if (neg) put('-');
  if (e == 0 && m == 0) { put('0'); put('.'); put('0'); return len; }
  uint64_t d;
  int32_t k;
  ryu_d2d(m, e, mbits, is32 ? 127 : 1023, d, k);
  const int32_t n = (int32_t)ryu_dec_len(d), kk = n + k, hi = is32 ? 13 : 16, lo = is32 ? -6 : -5;
  char dig[20];
  for (int32_t p = n - 1; p >= 0; p--) { dig[p] = (char)('0' + d % 10); d /= 10; }
  if (k >= 0 && kk <= hi) {
    for (int32_t p = 0; p < n; p++) put(dig[p]);
    for (int32_t p = n; p < kk; p++) put('0');
    put('.'); put('0');
  } else if (kk > 0 && kk <= hi) {
    for (int32_t p = 0; p < n; p++) { if (p == kk) put('.'); put(dig[p]); }
  } else if (kk > lo && kk <= 0) {
    put('0'); put('.');
    for (int32_t p = kk; p < 0; p++) put('0');
    for (int32_t p = 0; p < n; p++) put(dig[p]);
  } else {
    put(dig[0]);
    if (n > 1) { put('.'); for (int32_t p = 1; p < n; p++) put(dig[p]); }
    put('e');
    int32_t x = kk - 1;
    if (x < 0) { put('-'); x = -x; }
    if (x >= 100) put('0' + x / 100);
    if (x >= 10) put('0' + x / 10 % 10);
    put('0' + x % 10);
  }
  return len;
}

}  // namespace etlg
