// Host-side check of etl_amd/csrc/float_json.h (the NDJSON kernels' float text: ryu's format32 / format64 layout of the shortest
// round-trip digits) against libstdc++'s std::to_chars(.., chars_format::scientific), itself Ryu-based: its shortest digits and
// exponent, laid out by the rules ryu's pretty/mod.rs follows (restated here independently of the header), must equal the header's
// text byte for byte. Built and run by tests/test_float_json.py.
#include <charconv>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <random>
#include "float_json.h"

struct Buf { std::string s; void put(uint8_t c) { s.push_back((char)c); } };

// the layout from to_chars' scientific text: [-]D[.DDD]e(+|-)XX
template <class F>
static std::string expected(F v, bool is32) {
  char b[64];
  const auto r = std::to_chars(b, b + sizeof b, v, std::chars_format::scientific);
  std::string t(b, r.ptr), out;
  if (t[0] == '-') { out = "-"; t = t.substr(1); }
  const size_t ep = t.find('e');
  std::string digits;
  for (size_t i = 0; i < ep; i++) if (t[i] != '.') digits.push_back(t[i]);
  const int x = atoi(t.c_str() + ep + 1);
  if (digits == "0") return out + "0.0";
  const int n = (int)digits.size(), e = x - (n - 1), kk = n + e, hi = is32 ? 13 : 16, lo = is32 ? -6 : -5;
  if (e >= 0 && kk <= hi) return out + digits + std::string(e, '0') + ".0";
  if (kk > 0 && kk <= hi) return out + digits.substr(0, kk) + "." + digits.substr(kk);
  if (kk > lo && kk <= 0) return out + "0." + std::string(-kk, '0') + digits;
  return out + digits.substr(0, 1) + (n > 1 ? "." + digits.substr(1) : "") + "e" + std::to_string(kk - 1);
}

static uint64_t mism = 0, checked = 0;
static void one64(uint64_t bits) {
  double v; memcpy(&v, &bits, 8);
  if (v != v || v - v != 0) return;   // NaN / inf: refused before the printer
  Buf b;
  const uint32_t n = etlg::float_json(b, bits, false);
  const std::string want = expected(v, false);
  checked++;
  if (b.s != want || n != b.s.size()) { if (mism++ < 20) printf("f64 %016llx: got %s want %s\n", (unsigned long long)bits, b.s.c_str(), want.c_str()); }
}
static void one32(uint32_t bits) {
  float v; memcpy(&v, &bits, 4);
  if (v != v || v - v != 0) return;
  Buf b;
  const uint32_t n = etlg::float_json(b, bits, true);
  const std::string want = expected(v, true);
  checked++;
  if (b.s != want || n != b.s.size()) { if (mism++ < 20) printf("f32 %08x: got %s want %s\n", bits, b.s.c_str(), want.c_str()); }
}

int main(int argc, char** argv) {
  const uint64_t n_random = argc > 1 ? strtoull(argv[1], nullptr, 10) : 10000000ull;
  std::mt19937_64 rng(20261016);
  for (uint64_t i = 0; i < n_random; i++) { one64(rng()); one32((uint32_t)rng()); }
  // every power of two (normal and subnormal), with the neighbours on both sides, in both signs
  for (uint64_t e = 0; e < 2047; e++) for (int64_t d = -2; d <= 2; d++) { const uint64_t b = (e << 52) + (uint64_t)d; one64(b); one64(b | (1ull << 63)); }
  for (uint64_t k = 0; k < 52; k++) { one64(1ull << k); one64((1ull << k) + 1); one64((1ull << k) - 1); }
  for (uint32_t e = 0; e < 255; e++) for (int32_t d = -2; d <= 2; d++) { const uint32_t b = (e << 23) + (uint32_t)d; one32(b); one32(b | 0x80000000u); }
  for (uint32_t k = 0; k < 23; k++) { one32(1u << k); one32((1u << k) + 1); one32((1u << k) - 1); }
  // the extremes: smallest subnormal, largest subnormal, smallest / largest normal, zeros
  for (uint64_t b : {0x0ull, 0x1ull, 0x000fffffffffffffull, 0x0010000000000000ull, 0x7fefffffffffffffull}) { one64(b); one64(b | (1ull << 63)); }
  for (uint32_t b : {0x0u, 0x1u, 0x007fffffu, 0x00800000u, 0x7f7fffffu}) { one32(b); one32(b | 0x80000000u); }
  // around every layout threshold: 10^k and its neighbours for k = -30 .. 30 (both widths), and decimal texts of each length
  for (int k = -30; k <= 30; k++) {
    const double d = strtod(("1e" + std::to_string(k)).c_str(), nullptr);
    uint64_t b; memcpy(&b, &d, 8);
    for (int64_t q = -3; q <= 3; q++) { one64(b + (uint64_t)q); }
    const float f = strtof(("1e" + std::to_string(k)).c_str(), nullptr);
    uint32_t c; memcpy(&c, &f, 4);
    for (int32_t q = -3; q <= 3; q++) { one32(c + (uint32_t)q); }
    for (const char* m : {"1.5", "9.999999", "1.2345678901234567", "12345", "999999999999999", "1234567890123456", "12345678901234567"}) {
      const std::string t = std::string(m) + "e" + std::to_string(k);
      const double dv = strtod(t.c_str(), nullptr); uint64_t db; memcpy(&db, &dv, 8); one64(db);
      const float fv = strtof(t.c_str(), nullptr); uint32_t fb; memcpy(&fb, &fv, 4); one32(fb);
    }
  }
  // random bits near the decimal-exponent band of the fixed layouts (e in [2^-20, 2^60])
  for (uint64_t i = 0; i < n_random / 10; i++) {
    const uint64_t e = 1023 - 20 + rng() % 80;
    one64((e << 52) | (rng() & ((1ull << 52) - 1)));
    const uint32_t e32 = 127 - 20 + (uint32_t)(rng() % 70);
    one32((e32 << 23) | (uint32_t)(rng() & 0x7fffffu));
  }
  printf("checked %llu mismatches %llu\n", (unsigned long long)checked, (unsigned long long)mism);
  return mism ? 1 : 0;
}
