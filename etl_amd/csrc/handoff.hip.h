// What more than one hand-off translation unit needs (columns.hip, rowformats.hip, finish.hip): the cell-state accessors, serde_json's
// Display of a json cell (json_display), the Display strings of numeric / time / timetz, and the byte sinks the row formats and the
// formatted Arrow columns write through. Only DEV functions, templates, structs and constants: no kernel, no extern "C".
#pragma once
#include "cellparse.hip.h"   // json_valid, arr_walk, arr_spans: shared with the multi-pass decode (kernels.hip)
#include <type_traits>

namespace etlg {

constexpr int32_t kCeDays1970 = 719163;  // chrono num_days_from_ce of 1970-01-01

DEV uint32_t col_state(const ColJob& j, uint64_t base) { return (j.fixed[base + j.col_index / 4] >> (2 * (j.col_index % 4))) & 3u; }
DEV uint32_t ld32a(const u8* p) { return *(const uint32_t*)p; }   // row slots are 4-byte aligned

// ---- serde_json 1.0.149 `Value::to_string()` of a json / jsonb cell (the sinks' `j.to_string()`: clickhouse/encoding.rs:73,
// bigquery/encoding.rs:173-176, iceberg/encoding.rs:356) from the cell's source text, which json_valid() has accepted. What the parse +
// Display round trip changes (features arbitrary_precision + std, no preserve_order: crates/etl/Cargo.toml:36):
//   * whitespace between tokens goes; the output is compact ("," and ":" without blanks);
//   * an object is a BTreeMap<String, Value>: members leave in the byte order of their DECODED keys, a repeated key keeps its last value;
//   * strings are decoded and written again with serde_json's escapes: \" \\ \b \f \n \r \t, \u00xx (lowercase) for the other bytes
//     below 0x20, everything else raw (so "é" -> the two UTF-8 bytes, "\/" -> "/", a surrogate pair -> four bytes, 0x7f raw);
//   * a number keeps its literal (arbitrary_precision), except: an exponent without a sign gets '+' ("1e309" -> "1e+309": pinned by
//     the reference's own test, codec/text.rs:812-815), and an integer literal that fits u64 / i64 goes through the integer and back
//     (parse_any_number tries buf.parse() first), which only changes "-0" -> "0" (restated from serde_json's source; unpinned).
// Sorting is by selection: one pass over the object's members per member written (keys compared as decoded byte streams, no copy), so an
// object of k members costs k scans of its text. Returns 0; JD_HOST when the cell is beyond what a lane does here (nesting deeper than
// kJsonDepth, an object of more than kJsonMembers members, serde_json's private number token as a key) — the caller hands the cell
// back, as before; JD_BQ_INT when `bq` is set and a number that is WRITTEN (the value of a repeated key that lost is not in the parsed
// Value either) is an integer literal outside u64 / i64 (validate_json_number_for_bigquery, bigquery/validation.rs:64-85).
constexpr uint32_t kJsonDepth = 16, kJsonMembers = 64;
enum : uint32_t { JD_OK = 0, JD_HOST = 1, JD_BQ_INT = 2 };
struct JsIter { uint32_t i, pend, npend; };   // a cursor over a string's decoded bytes (i: behind the opening quote)
DEV int js_next(const u8* s, JsIter& k) {     // the next decoded byte, -1 at the closing quote
  if (k.npend) { const int b = (int)(k.pend & 0xFFu); k.pend >>= 8; k.npend--; return b; }
  const uint32_t c = s[k.i];
  if (c == '"') return -1;
  if (c != '\\') { k.i++; return (int)c; }
  const uint32_t x = s[k.i + 1];
  if (x != 'u') {
    k.i += 2;
    return x == 'b' ? 8 : x == 'f' ? 12 : x == 'n' ? 10 : x == 'r' ? 13 : x == 't' ? 9 : (int)x;   // \" \\ \/ are themselves
  }
  auto h4 = [&](uint32_t at) { uint32_t v = 0; for (uint32_t q = 0; q < 4; q++) v = v * 16 + (uint32_t)arr_hexv(s[at + q]); return v; };
  uint32_t cp = h4(k.i + 2);
  k.i += 6;
  if (cp >= 0xD800 && cp <= 0xDBFF) { cp = 0x10000 + ((cp - 0xD800) << 10) + (h4(k.i + 2) - 0xDC00); k.i += 6; }
  if (cp < 0x80) return (int)cp;
  if (cp < 0x800) { k.pend = 0x80 | (cp & 63); k.npend = 1; return (int)(0xC0 | (cp >> 6)); }
  if (cp < 0x10000) { k.pend = (0x80 | ((cp >> 6) & 63)) | ((0x80 | (cp & 63)) << 8); k.npend = 2; return (int)(0xE0 | (cp >> 12)); }
  k.pend = (0x80 | ((cp >> 12) & 63)) | ((0x80 | ((cp >> 6) & 63)) << 8) | ((0x80 | (cp & 63)) << 16); k.npend = 3;
  return (int)(0xF0 | (cp >> 18));
}
DEV int js_cmp(const u8* s, uint32_t a, uint32_t b) {   // the decoded strings at the opening quotes a and b: <0, 0, >0
  JsIter x{a + 1, 0, 0}, y{b + 1, 0, 0};
  for (;;) {
    const int p = js_next(s, x), q = js_next(s, y);
    if (p != q) return p - q;      // (-1, the end, sorts first: a prefix is smaller)
    if (p < 0) return 0;
  }
}
DEV uint32_t js_skip_string(const u8* s, uint32_t i) {   // from the opening quote to behind the closing one
  for (i++;; i++) { if (s[i] == '"') return i + 1; if (s[i] == '\\') i++; }
}
DEV uint32_t js_ws(const u8* s, uint32_t i, uint32_t n) { while (i < n && (s[i] == ' ' || s[i] == '\t' || s[i] == '\n' || s[i] == '\r')) i++; return i; }
DEV uint32_t js_skip_value(const u8* s, uint32_t i, uint32_t n) {   // from a value's first byte to behind it
  const uint32_t c = s[i];
  if (c == '"') return js_skip_string(s, i);
  if (c == '{' || c == '[') {
    uint32_t d = 0;
    for (;;) {
      const uint32_t x = s[i];
      if (x == '"') { i = js_skip_string(s, i); continue; }
      if (x == '{' || x == '[') d++;
      else if (x == '}' || x == ']') { if (!--d) return i + 1; }
      i++;
    }
  }
  while (i < n && s[i] != ',' && s[i] != '}' && s[i] != ']' && s[i] != ' ' && s[i] != '\t' && s[i] != '\n' && s[i] != '\r') i++;
  return i;
}
template <class S>
DEV uint32_t js_put_string(S& out, const u8* s, uint32_t i) {   // the string at the opening quote i, escaped again; returns behind it
  JsIter k{i + 1, 0, 0};
  out.put('"');
  for (;;) {
    const int b = js_next(s, k);
    if (b < 0) break;
    if (b == '"' || b == '\\') { out.put('\\'); out.put((u8)b); }
    else if (b >= 0x20) out.put((u8)b);
    else {
      out.put('\\');
      if (b == 8) out.put('b'); else if (b == 12) out.put('f'); else if (b == 10) out.put('n'); else if (b == 13) out.put('r'); else if (b == 9) out.put('t');
      else { out.put('u'); out.put('0'); out.put('0'); out.put((u8)('0' + (b >> 4))); out.put((u8)((b & 15) < 10 ? '0' + (b & 15) : 'a' + (b & 15) - 10)); }
    }
  }
  out.put('"');
  return k.i + 1;
}
template <class S>
DEV uint32_t json_display(S& out, const u8* s, uint32_t n, bool bq) {
  uint32_t f_start[kJsonDepth], f_last[kJsonDepth], f_end[kJsonDepth];   // objects: behind '{', the last key written, behind '}'
  uint32_t is_obj = 0, depth = 0;
  uint32_t i = js_ws(s, 0, n);
  constexpr uint32_t NONE = 0xFFFFFFFFu;
  for (;;) {
    // ---- one value at i
    bool opened = false;
    {
      const uint32_t c = s[i];
      if (c == '"') i = js_put_string(out, s, i);
      else if (c == '{' || c == '[') {
        if (depth >= kJsonDepth) return JD_HOST;
        out.put((u8)c);
        if (c == '{') { is_obj |= 1u << depth; f_start[depth] = i + 1; f_last[depth] = NONE; f_end[depth] = 0; }
        else {
          is_obj &= ~(1u << depth);
          i = js_ws(s, i + 1, n);
          if (s[i] == ']') { out.put(']'); i++; goto after_value; }   // (depth not raised: an empty array is a value like any other)
          opened = true;
        }
        depth++;
        if (opened) continue;   // the array's first element sits at i
      } else if (c == 't' || c == 'f' || c == 'n') { const uint32_t e = js_skip_value(s, i, n); for (; i < e; i++) out.put(s[i]); }
      else {   // a number
        const uint32_t e = js_skip_value(s, i, n);
        bool integer = true;
        for (uint32_t q = i; q < e; q++) if (s[q] == '.' || s[q] == 'e' || s[q] == 'E') integer = false;
        if (integer && bq) {   // number.parse::<i64>() / ::<u64>() must succeed
          const bool neg = s[i] == '-';
          const uint32_t d0 = i + (neg ? 1 : 0), nd = e - d0;
          const char* lim = neg ? "9223372036854775808" : "18446744073709551615";
          const uint32_t nl = neg ? 19 : 20;
          bool over = nd > nl;
          if (nd == nl) { for (uint32_t q = 0; q < nl; q++) { if (s[d0 + q] != (u8)lim[q]) { over = s[d0 + q] > (u8)lim[q]; break; } } }
          if (over) return JD_BQ_INT;
        }
        if (e - i == 2 && s[i] == '-' && s[i + 1] == '0') { out.put('0'); i = e; }
        else for (; i < e; i++) { out.put(s[i]); if ((s[i] == 'e' || s[i] == 'E') && s[i + 1] != '+' && s[i + 1] != '-') out.put('+'); }
      }
    }
    // ---- behind a value (or inside a fresh object): what the innermost open container wants next
  after_value:
    for (;;) {
      if (!depth) return JD_OK;
      const uint32_t t = depth - 1;
      if (!((is_obj >> t) & 1u)) {   // array: the text goes on in order
        i = js_ws(s, i, n);
        if (s[i] == ',') { out.put(','); i = js_ws(s, i + 1, n); break; }
        out.put(']'); i++; depth--;
        continue;
      }
      // object: the smallest key above the last one written; of equal keys the last
      uint32_t p = js_ws(s, f_start[t], n), best = NONE, bestv = 0, members = 0;
      const uint32_t last = f_last[t];
      while (s[p] != '}') {
        if (s[p] == ',') p = js_ws(s, p + 1, n);
        const uint32_t kq = p;
        p = js_ws(s, js_skip_string(s, p), n) + 1;   // behind ':'
        p = js_ws(s, p, n);
        const uint32_t v = p;
        p = js_ws(s, js_skip_value(s, p, n), n);
        if (++members > kJsonMembers) return JD_HOST;
        if (last == NONE) {   // the first round also looks for the private token ("$serde_json::private::Number" as a key makes from_str read a number)
          const char* tok = "$serde_json::private::";
          JsIter it{kq + 1, 0, 0};
          bool is_tok = true;
          for (uint32_t q = 0; q < 22 && is_tok; q++) is_tok = js_next(s, it) == (int)tok[q];
          if (is_tok) return JD_HOST;
        }
        if (last != NONE && js_cmp(s, kq, last) <= 0) continue;
        if (best == NONE || js_cmp(s, kq, best) <= 0) { best = kq; bestv = v; }
      }
      f_end[t] = p + 1;
      if (best == NONE) { out.put('}'); i = f_end[t]; depth--; continue; }
      if (last != NONE) out.put(',');
      f_last[t] = best;
      (void)js_put_string(out, s, best);
      out.put(':');
      i = bestv;
      break;
    }
  }
}
struct JsCount { uint32_t n = 0; DEV void put(u8) { n++; } };

// ---- the elements of a json[] / jsonb[] literal (ArrayCell::Json): the one walk every hand-off shares. An element is unescaped into
// private memory (json_display walks its text back and forth) — `tmp`, kJsonElemMax bytes of the caller, one buffer for the check and
// the visits behind it. An element of more than kJsonElemMax unescaped bytes is left to the host: a lane does not look at it.
constexpr uint32_t kJsonElemMax = 256;
// What the check met, for the caller to rank (the sinks rank differently: see the call sites).
struct JsonArrFacts {
  bool too_long = false;    // an element of more than kJsonElemMax bytes (it may not be JSON at all)
  bool bad_json = false;    // an element that is not one JSON value: the reference's decode error (codec/text.rs:126-134)
  bool bad_first = false;   // ... met before any too_long one
  bool limit = false;       // an element beyond json_display's limits (JD_HOST)
  bool bq_int = false;      // JD_BQ_INT (only with bq)
  bool has_null = false;    // a NULL element
  DEV bool any() const { return too_long | bad_json | limit | bq_int | has_null; }
};
// Walks the literal once: the element count, the facts, and on_elem(text, len, display_len) for every element that passed (it is
// unescaped in tmp). VALIDATE: json_valid() runs (the row formats check the text in their counting pass only). Returns arr_spans' error.
template <bool VALIDATE, class E>
DEV uint32_t json_arr_check(const u8* s, uint32_t n, bool bq, u8* tmp, uint32_t& cnt, JsonArrFacts& f, E&& on_elem) {
  return arr_spans(s, n, cnt, [&](uint32_t, bool is_null, uint32_t p0, uint32_t p1, uint32_t ulen) {
    if (is_null) { f.has_null = true; return; }
    if (ulen > kJsonElemMax) { f.too_long = true; return; }
    uint32_t k = 0;
    arr_unescape(s, p0, p1, [&](u8 c) { tmp[k++] = c; });
    if (VALIDATE && !json_valid(tmp, ulen)) { f.bad_first |= !f.too_long; f.bad_json = true; return; }
    JsCount c;
    const uint32_t e = json_display(c, tmp, ulen, bq);
    if (e) { if (e == JD_BQ_INT) f.bq_int = true; else f.limit = true; return; }
    on_elem((const u8*)tmp, ulen, c.n);
  });
}
template <bool VALIDATE>
DEV uint32_t json_arr_check(const u8* s, uint32_t n, u8* tmp, uint32_t& cnt, JsonArrFacts& f) {
  return json_arr_check<VALIDATE>(s, n, false, tmp, cnt, f, [](const u8*, uint32_t, uint32_t) {});
}
// Walks a literal the check has accepted: visit(k, is_null, text, len) for every element k, unescaped in tmp unless it is NULL
template <class V>
DEV void json_arr_visit(const u8* s, uint32_t n, u8* tmp, V&& visit) {
  uint32_t cnt;
  (void)arr_spans(s, n, cnt, [&](uint32_t k, bool is_null, uint32_t p0, uint32_t p1, uint32_t ulen) {
    if (!is_null) { uint32_t q = 0; arr_unescape(s, p0, p1, [&](u8 c) { tmp[q++] = c; }); }
    visit(k, is_null, (const u8*)tmp, ulen);
  });
}

// ---- Display strings of the classes every sink writes as text: PgNumeric (format_numeric_value,
// crates/etl-postgres/src/numeric.rs:460-560), PgTimeTz (etl-postgres/src/time.rs:113-117 + write_utc_offset :210-225) and
// chrono's "%H:%M:%S%.f" (TIME_FORMAT, time.rs:17). `ent`: the numeric's heap entry (etlg_numeric_hdr + i16 digits, 4-byte aligned).
// All of them are written through the same count / write sinks as the rows (RbCount / RbWrite below), so a length is the
// count of the very code that later writes the bytes — except the numeric's, which has a closed form (a scale can be 16383).
DEV uint32_t num_digit(const u8* ent, uint32_t i) { return (uint32_t)ent[8 + 2 * i] | ((uint32_t)ent[9 + 2 * i] << 8); }
DEV uint32_t numeric_str_len(const u8* ent) {
  const uint32_t kind = ent[0];
  if (kind == ETLG_NUM_NAN) return 3;        // "NaN"
  if (kind == ETLG_NUM_PINF) return 8;       // "Infinity"
  if (kind == ETLG_NUM_NINF) return 9;       // "-Infinity"
  const int32_t weight = (int16_t)((uint32_t)ent[2] | ((uint32_t)ent[3] << 8));
  const uint32_t scale = (uint32_t)ent[4] | ((uint32_t)ent[5] << 8), nd = (uint32_t)ent[6] | ((uint32_t)ent[7] << 8);
  const uint32_t frac = scale ? 1u + scale : 0u;
  if (!nd) return 1u + frac;                 // zero keeps its display scale (:492-503)
  uint32_t n = ent[1] ? 1u : 0u;
  if (weight < 0) n += 1u;
  else { const uint32_t d0 = num_digit(ent, 0); n += (d0 >= 1000 ? 4u : d0 >= 100 ? 3u : d0 >= 10 ? 2u : 1u) + 4u * (uint32_t)weight; }
  return n + frac;
}
DEV uint32_t hex_digit(uint32_t d) { return d < 10 ? '0' + d : 'a' + d - 10; }   // lowercase
template <class S> DEV void put_4d(S& s, uint32_t v) { s.put((u8)('0' + v / 1000 % 10)); s.put((u8)('0' + v / 100 % 10)); s.put((u8)('0' + v / 10 % 10)); s.put((u8)('0' + v % 10)); }
template <class S>
DEV void numeric_str(S& s, const u8* ent) {
  const uint32_t kind = ent[0];
  if (kind != ETLG_NUM_VALUE) {
    const char* t = kind == ETLG_NUM_NAN ? "NaN" : kind == ETLG_NUM_PINF ? "Infinity" : "-Infinity";
    for (; *t; t++) s.put((u8)*t);
    return;
  }
  const int32_t weight = (int16_t)((uint32_t)ent[2] | ((uint32_t)ent[3] << 8));
  const uint32_t scale = (uint32_t)ent[4] | ((uint32_t)ent[5] << 8), nd = (uint32_t)ent[6] | ((uint32_t)ent[7] << 8);
  if (!nd) {
    s.put('0');
    if (scale) { s.put('.'); for (uint32_t k = 0; k < scale; k++) s.put('0'); }
    return;
  }
  if (ent[1]) s.put('-');
  if (weight < 0) s.put('0');
  else {
    for (int32_t d = 0; d <= weight; d++) {
      const uint32_t g = (uint32_t)d < nd ? num_digit(ent, (uint32_t)d) : 0u;
      if (d == 0) {  // the first group without its leading zeros (:517-524)
        if (g >= 1000) s.put((u8)('0' + g / 1000 % 10));
        if (g >= 100) s.put((u8)('0' + g / 100 % 10));
        if (g >= 10) s.put((u8)('0' + g / 10 % 10));
        s.put((u8)('0' + g % 10));
      } else put_4d(s, g);
    }
  }
  if (scale) {
    s.put('.');
    // `let mut d = weight + 1` is i16 arithmetic in the reference (:535): at weight = i16::MAX a release build wraps to
    // i16::MIN and prints zeros; restated as such
    int32_t d = (int16_t)(weight + 1);
    for (uint32_t rem = scale; rem; d++) {
      const uint32_t g = (d >= 0 && (uint32_t)d < nd) ? num_digit(ent, (uint32_t)d) : 0u;
      const uint32_t take = rem < 4 ? rem : 4u;
      uint32_t div = 1000;
      for (uint32_t k = 0; k < take; k++, div /= 10) s.put((u8)('0' + g / div % 10));
      rem -= take;
    }
  }
}
template <class S> DEV void put_2d(S& s, uint32_t v) { s.put((u8)('0' + v / 10)); s.put((u8)('0' + v % 10)); }
// chrono's %.f prints nothing, or 3 / 6 / 9 digits; a leap second is kept as nanos >= 10^9 on second 59 and printed as :60
DEV uint32_t time_frac_len(uint32_t nanos) { nanos = nanos >= 1000000000u ? nanos - 1000000000u : nanos; return nanos == 0 ? 0u : nanos % 1000000u == 0 ? 4u : nanos % 1000u == 0 ? 7u : 10u; }
template <class S> DEV void time_str(S& s, uint32_t secs, uint32_t nanos) {
  const uint32_t leap = nanos >= 1000000000u ? 1u : 0u;
  nanos -= leap * 1000000000u;
  put_2d(s, secs / 3600); s.put(':'); put_2d(s, secs / 60 % 60); s.put(':'); put_2d(s, secs % 60 + leap);
  const uint32_t frac = time_frac_len(nanos);
  if (frac) {
    s.put('.');
    uint32_t v = frac == 4 ? nanos / 1000000u : frac == 7 ? nanos / 1000u : nanos, div = frac == 4 ? 100u : frac == 7 ? 100000u : 100000000u;
    for (; div; div /= 10) s.put((u8)('0' + v / div % 10));
  }
}
DEV uint32_t utc_offset_len(int32_t off) { const uint32_t a = (uint32_t)(off < 0 ? -off : off); return a % 60 ? 9u : a % 3600 ? 6u : 3u; }
template <class S> DEV void utc_offset_str(S& s, int32_t off) {   // +HH | +HH:MM | +HH:MM:SS (write_utc_offset)
  const uint32_t a = (uint32_t)(off < 0 ? -off : off);
  s.put(off < 0 ? '-' : '+');
  put_2d(s, a / 3600);
  if (a % 60) { s.put(':'); put_2d(s, a % 3600 / 60); s.put(':'); put_2d(s, a % 60); }
  else if (a % 3600) { s.put(':'); put_2d(s, a % 3600 / 60); }
}
DEV uint32_t timetz_str_len(const u8* slot) { return 8u + time_frac_len(ld32a(slot + 4)) + utc_offset_len((int32_t)ld32a(slot + 8)); }
template <class S> DEV void timetz_str(S& s, const u8* slot) { time_str(s, ld32a(slot), ld32a(slot + 4)); utc_offset_str(s, (int32_t)ld32a(slot + 8)); }

// The byte pass of a row. One thread writes one row, so a byte store per put() was one write request per BYTE at the L2 (64 lanes,
// 64 different lines per instruction): k_rb_rows took 469 us for the 47 MB of a cfg3 batch's rows (profiles/r04q). The bytes are
// collected in a 64-bit accumulator instead and leave eight at a time (unaligned 8-byte stores are fine in global memory); finish()
// writes the last 1-7 bytes one by one — the next row's first bytes belong to another thread.
struct RbGlobalSink {
  u8* p;                // where the accumulator's first byte goes
  uint64_t acc = 0;
  uint32_t n = 0;       // bytes in acc (0..7)
  DEV explicit RbGlobalSink(u8* q) : p(q) {}
  DEV void store8(uint64_t v) { __builtin_memcpy(p, &v, 8); p += 8; }
  // appends the low k bytes of v (1 <= k <= 8; the bytes above them are zero)
  DEV void append(uint64_t v, uint32_t k) {
    acc |= v << (8u * n);
    const uint32_t m = n + k;
    if (m >= 8u) {
      store8(acc);
      acc = n ? v >> (8u * (8u - n)) : 0ull;   // what did not fit (n = 0: k = 8, nothing is left)
      n = m - 8u;
    } else n = m;
  }
  DEV void finish() { for (uint32_t b = 0; b < n; b++) p[b] = (u8)(acc >> (8u * b)); p += n; n = 0; acc = 0; }
};
// The same bytes into a ZEROED image of the output in LDS (k_rb_rows): whole words are OR-ed in (ds_or_b32), so the first and the last
// word of a part may be shared with its neighbours; the image leaves for global memory in 16-byte stores of the whole workgroup.
struct RbLdsSink {
  uint32_t* w;          // the word the accumulator's first byte belongs to
  uint64_t acc = 0;
  uint32_t n;           // bytes in acc (0..3 between calls), counting the bytes of *w in front of this part
  DEV RbLdsSink(uint32_t* word, uint32_t lead) : w(word), n(lead) {}
  DEV void app4(uint32_t v, uint32_t k) {   // 1 <= k <= 4
    acc |= (uint64_t)v << (8u * n);
    n += k;
    if (n >= 4u) { atomicOr(w++, (uint32_t)acc); acc >>= 32; n -= 4u; }
  }
  DEV void append(uint64_t v, uint32_t k) { if (k > 4u) { app4((uint32_t)v, 4u); app4((uint32_t)(v >> 32), k - 4u); } else app4((uint32_t)v, k); }
  DEV void finish() { if (n && (uint32_t)acc) atomicOr(w, (uint32_t)acc); n = 0; acc = 0; }
};
template <class B>
struct RbWriterT : B {
  using B::B;
  using B::append;
  DEV void put(u8 b) { append(b, 1); }
  DEV void varint64(uint64_t v) { while (v >= 0x80) { put((u8)(v | 0x80)); v >>= 7; } put((u8)v); }
  DEV void put32(uint32_t v) { append(v, 4); }
  DEV void put64(uint64_t v) { append(v, 8); }
  DEV void zeros(uint32_t k) { while (k >= 8u) { append(0ull, 8); k -= 8u; } if (k) append(0ull, k); }
  DEV void bytes(const u8* s, uint32_t len) {
    uint32_t k = 0;
    for (; k + 16u <= len; k += 16u) { uint64_t v[2]; __builtin_memcpy(v, s + k, 16); append(v[0], 8); append(v[1], 8); }   // (one request per 16 bytes of a long text)
    for (; k + 8u <= len; k += 8u) { uint64_t v; __builtin_memcpy(&v, s + k, 8); append(v, 8); }
    if (k < len) { uint64_t v = 0; for (uint32_t b = 0; k + b < len; b++) v |= (uint64_t)s[k + b] << (8u * b); append(v, len - k); }
  }
  DEV void hex(const u8* s, uint32_t len, uint32_t alpha = 'a') {   // bytes_to_hex, lowercase (:176-185); alpha 'A': upper case
    auto h1 = [alpha](uint32_t d) -> uint64_t { return d < 10 ? '0' + d : alpha + d - 10; };
    uint32_t k = 0;
    for (; k + 4u <= len; k += 4u) {   // four bytes -> eight digits
      uint64_t v = 0;
      for (uint32_t b = 0; b < 4; b++) { const uint32_t x = s[k + b]; v |= (h1(x >> 4) | (h1(x & 15u) << 8)) << (16u * b); }
      append(v, 8);
    }
    for (; k < len; k++) { const uint32_t x = s[k]; append(h1(x >> 4) | (h1(x & 15u) << 8), 2); }
  }
};
using RbWrite = RbWriterT<RbGlobalSink>;
using RbLdsWrite = RbWriterT<RbLdsSink>;

struct RbCount {
  uint32_t n = 0;
  DEV void put(u8) { n++; }
  DEV void varint64(uint64_t v) { do { n++; v >>= 7; } while (v); }
  DEV void put32(uint32_t) { n += 4; }
  DEV void put64(uint64_t) { n += 8; }
  DEV void zeros(uint32_t k) { n += k; }
  DEV void append(uint64_t, uint32_t k) { n += k; }
  DEV void bytes(const u8*, uint32_t len) { n += len; }
  DEV void hex(const u8*, uint32_t len, uint32_t = 'a') { n += 2 * len; }
};

}  // namespace etlg
