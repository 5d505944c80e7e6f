// float8 -> the text Rust's `f64` Display writes (`value.to_string()`), shared by the DuckLake literal kernels (rowformats.hip.h, dl_row)
// and a host-side unit test (tests/test_float_display.py compiles this header with g++ and checks it against libstdc++'s
// std::to_chars(..., std::chars_format::fixed) on tens of millions of bit patterns).
//
// Display without a precision prints the shortest digits that read back as the float (core::fmt::float -> flt2dec's shortest strategy:
// Grisu with a Dragon fallback, the same digits as Ryu's d2d in float_json.h) laid out POSITIONALLY, never with an exponent
// (flt2dec::to_shortest_str / digits_to_dec_str). With the digits d (n of them) and value = d x 10^e, kk = n + e:
//   e >= 0          the digits, e zeros                        1, 100000000000000000000 (1e20); DBL_MAX: 17 digits and 292 zeros
//   0 < kk < n      a '.' after the first kk digits            12.34
//   kk <= 0         "0.", -kk zeros, the digits                0.1, 0.000...5 (5e-324: "0." + 323 zeros + "5", 326 bytes; 327 with a '-')
// zero is "0", negative zero "-0", a leading '-' for negative values; never a trailing ".0". NaN / inf never get here (the DuckLake
// sink writes CAST('NaN' AS DOUBLE) ... for them, rowformats.hip.h dl_float).
// A float4 is widened first (`f as f64`, exact), so 0.1f32 prints 0.10000000149011612: f32_widen_bits does that on the bits, so that
// the result does not hang on the denormal mode the kernel was compiled with.
#pragma once
#include <stdint.h>
#include "float_json.h"

namespace etlg {

ETLG_FD uint64_t f32_widen_bits(uint32_t b) {
  const uint64_t sign = (uint64_t)(b >> 31) << 63;
  int32_t e = (int32_t)((b >> 23) & 0xFFu);
  uint32_t m = b & 0x7FFFFFu;
  if (e == 0xFF) return sign | (0x7FFull << 52) | ((uint64_t)m << 29);
  if (e == 0) {
    if (!m) return sign;
    int32_t sh = 0;
    while (!(m & 0x800000u)) { m <<= 1; sh++; }   // a subnormal float4 is a normal float8
    m &= 0x7FFFFFu;
    e = 1 - sh;
  }
  return sign | ((uint64_t)(e - 127 + 1023) << 52) | ((uint64_t)m << 29);
}

// The text of a finite float8 into `s` (put(u8)); returns its length (1 .. 327). `s` may be a counter.
template <class S>
ETLG_FD uint32_t float_display(S& s, uint64_t bits) {
  const bool neg = (bits >> 63) != 0;
  const uint64_t m = bits & ((1ull << 52) - 1u);
  const uint32_t e = (uint32_t)(bits >> 52) & 0x7FFu;
  uint32_t len = 0;
  auto put = [&](uint32_t c) { s.put((uint8_t)c); len++; };
  if (neg) put('-');
  if (e == 0 && m == 0) { put('0'); return len; }
  uint64_t d;
  int32_t k;
  ryu_d2d(m, e, 52u, 1023, d, k);
  const int32_t n = (int32_t)ryu_dec_len(d), kk = n + k;
  char dig[20];
  for (int32_t p = n - 1; p >= 0; p--) { dig[p] = (char)('0' + d % 10); d /= 10; }
  if (k >= 0) {
    for (int32_t p = 0; p < n; p++) put(dig[p]);
    for (int32_t p = 0; p < k; p++) put('0');
  } else if (kk > 0) {
    for (int32_t p = 0; p < n; p++) { if (p == kk) put('.'); put(dig[p]); }
  } else {
    put('0'); put('.');
    for (int32_t p = kk; p < 0; p++) put('0');
    for (int32_t p = 0; p < n; p++) put(dig[p]);
  }
  return len;
}

}  // namespace etlg
