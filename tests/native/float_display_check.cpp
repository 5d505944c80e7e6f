// Host-side check of etl_amd/csrc/float_display.h (the DuckLake literal kernels' float text: Rust's f64 Display, the shortest
// round-trip digits laid out positionally) against libstdc++'s std::to_chars(.., chars_format::fixed) without a precision.
// to_chars writes "-0" and "0" like Display; NaN / inf never reach the printer (the sink writes CASTs).
// Where to_chars' fixed text IS the shortest positional form (every value with a fraction, every integer below 2^53 and the larger
// ones whose shortest digits are exact) the two texts must be equal byte for byte. For the other integers (most doubles of 2^53 and
// more) libstdc++ prints the EXACT integer ("99999999999999991611392" for 1e23) where Display prints the shortest digits and zeros
// ("100000000000000000000000"); there the header's text must have to_chars' length (one more when the digits round up to a power of ten), equal the positional layout of to_chars' own
// shortest digits (chars_format::scientific), agree with the exact text in its leading 17 digits to within the rounding interval, and
// read back (strtod) as the same bits — so every value is checked against to_chars, none is skipped.
// A float4 is widened on its bits (f32_widen_bits) and must equal the compiler's `(double)f` bit for bit before it is printed.
// Built and run by tests/test_float_display.py.
#include <charconv>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <random>
#include "float_display.h"

struct Buf { std::string s; void put(uint8_t c) { s.push_back((char)c); } };
struct Cnt { uint32_t n = 0; void put(uint8_t) { n++; } };

static uint64_t mism = 0, checked = 0, longest = 0, exact_ints = 0;
// to_chars' shortest digits and exponent ([-]D[.DDD]e(+|-)XX), laid out positionally — restated here independently of the header
static std::string from_scientific(double v) {
  char b[64];
  const auto r = std::to_chars(b, b + sizeof b, v, std::chars_format::scientific);
  std::string t(b, r.ptr), out;
  if (t[0] == '-') { out = "-"; t = t.substr(1); }
  const size_t ep = t.find('e');
  std::string digits;
  for (size_t i = 0; i < ep; i++) if (t[i] != '.') digits.push_back(t[i]);
  const int x = atoi(t.c_str() + ep + 1);
  if (digits == "0") return out + "0";
  const int n = (int)digits.size(), e = x - (n - 1), kk = n + e;
  if (e >= 0) return out + digits + std::string(e, '0');
  if (kk > 0) return out + digits.substr(0, kk) + "." + digits.substr(kk);
  return out + "0." + std::string(-kk, '0') + digits;
}
static void one64(uint64_t bits) {
  double v; memcpy(&v, &bits, 8);
  if (v != v || v - v != 0) return;   // NaN / inf: CAST('NaN' AS DOUBLE) ... , not the printer
  Buf b;
  const uint32_t n = etlg::float_display(b, bits);
  Cnt c;
  (void)etlg::float_display(c, bits);   // (the count pass must size it exactly)
  char w[400];
  const auto r = std::to_chars(w, w + sizeof w, v, std::chars_format::fixed);
  std::string want(w, r.ptr);
  checked++;
  if (b.s.size() > longest) longest = b.s.size();
  const std::string lay = from_scientific(v);
  if (want != lay) {   // only the exact integer of a double of 2^53 or more may differ from the shortest form (see above)
    exact_ints++;
    const size_t lead = want[0] == '-' ? 1 : 0;
    // the first 17 digits of both texts as integers: the shortest digits lie within half an ulp (2^-53 of the value, at most 11.2
    // units of the 17th digit) of the exact value, and cutting the exact text adds less than one unit
    const unsigned long long a = strtoull(want.substr(lead, 17).c_str(), nullptr, 10), g = strtoull(b.s.substr(lead, 17).c_str(), nullptr, 10);
    bool close = b.s.size() == want.size() && (a > g ? a - g : g - a) <= 12ull;
    // (rounding up to a power of ten makes the shortest form one digit longer: 1 and zeros against 9999999999999999...)
    if (b.s.size() == want.size() + 1 && b.s.find_first_not_of('0', lead + 1) == std::string::npos && b.s[lead] == '1') close = 100000000000000000ull - a <= 12ull;
    const double back = strtod(b.s.c_str(), nullptr);
    uint64_t bb; memcpy(&bb, &back, 8);
    const bool big_int = (v < 0 ? -v : v) >= 9007199254740992.0 && want.find('.') == std::string::npos;
    if (!big_int || b.s != lay || !close || bb != bits) want = "<" + lay + "> with the length and leading digits of " + want;
    else want = b.s;
  }
  if (b.s != want || n != b.s.size() || c.n != n) { if (mism++ < 20) printf("f64 %016llx: got %s want %s\n", (unsigned long long)bits, b.s.c_str(), want.c_str()); }
}
static void one32(uint32_t bits) {
  float f; memcpy(&f, &bits, 4);
  const double v = (double)f;
  uint64_t want; memcpy(&want, &v, 8);
  const uint64_t got = etlg::f32_widen_bits(bits);
  if (f == f && got != want) { if (mism++ < 20) printf("f32 %08x widens to %016llx, want %016llx\n", bits, (unsigned long long)got, (unsigned long long)want); return; }
  if (f != f && ((got >> 52) & 0x7FF) != 0x7FF) { mism++; return; }
  one64(got);
}

int main(int argc, char** argv) {
  const uint64_t n_random = argc > 1 ? strtoull(argv[1], nullptr, 10) : 10000000ull;
  std::mt19937_64 rng(20261016);
  for (uint64_t i = 0; i < n_random; i++) { one64(rng()); one32((uint32_t)rng()); }
  // every power of two (normal and subnormal), with the neighbours on both sides, in both signs
  for (uint64_t e = 0; e < 2047; e++) for (int64_t d = -2; d <= 2; d++) { const uint64_t b = (e << 52) + (uint64_t)d; one64(b); one64(b | (1ull << 63)); }
  for (uint64_t k = 0; k < 52; k++) { one64(1ull << k); one64((1ull << k) + 1); one64((1ull << k) - 1); }
  // every float4 power of two (normal and subnormal) widened, with its neighbours
  for (uint32_t e = 0; e < 255; e++) for (int32_t d = -2; d <= 2; d++) { const uint32_t b = (e << 23) + (uint32_t)d; one32(b); one32(b | 0x80000000u); }
  for (uint32_t k = 0; k < 23; k++) { one32(1u << k); one32((1u << k) + 1); one32((1u << k) - 1); }
  // the extremes: zeros, smallest / largest subnormal, smallest normal, DBL_MAX / FLT_MAX
  for (uint64_t b : {0x0ull, 0x1ull, 0x000fffffffffffffull, 0x0010000000000000ull, 0x7fefffffffffffffull}) { one64(b); one64(b | (1ull << 63)); }
  for (uint32_t b : {0x0u, 0x1u, 0x007fffffu, 0x00800000u, 0x7f7fffffu}) { one32(b); one32(b | 0x80000000u); }
  // powers of ten 1e-30 .. 1e30 and their neighbours, and decimal texts of each length around them
  for (int k = -30; k <= 30; k++) {
    const double d = strtod(("1e" + std::to_string(k)).c_str(), nullptr);
    uint64_t b; memcpy(&b, &d, 8);
    for (int64_t q = -3; q <= 3; q++) one64(b + (uint64_t)q);
    const float f = strtof(("1e" + std::to_string(k)).c_str(), nullptr);
    uint32_t c; memcpy(&c, &f, 4);
    for (int32_t q = -3; q <= 3; q++) one32(c + (uint32_t)q);
    for (const char* m : {"1.5", "9.999999", "1.2345678901234567", "12345", "999999999999999", "1234567890123456", "12345678901234567"}) {
      const std::string t = std::string(m) + "e" + std::to_string(k);
      const double dv = strtod(t.c_str(), nullptr); uint64_t db; memcpy(&db, &dv, 8); one64(db);
      const float fv = strtof(t.c_str(), nullptr); uint32_t fb; memcpy(&fb, &fv, 4); one32(fb);
    }
  }
  // random bits in the band where the point falls inside or just outside the digits (2^-20 .. 2^60)
  for (uint64_t i = 0; i < n_random / 10; i++) {
    const uint64_t e = 1023 - 20 + rng() % 80;
    one64((e << 52) | (rng() & ((1ull << 52) - 1)));
    const uint32_t e32 = 127 - 20 + (uint32_t)(rng() % 70);
    one32((e32 << 23) | (uint32_t)(rng() & 0x7fffffu));
  }
  printf("checked %llu mismatches %llu longest %llu exact_integers %llu\n", (unsigned long long)checked, (unsigned long long)mism, (unsigned long long)longest, (unsigned long long)exact_ints);
  return mism ? 1 : 0;
}
