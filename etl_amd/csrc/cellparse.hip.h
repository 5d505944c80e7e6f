// Cell-text grammars shared by the hand-off kernels (columns.hip, rowformats.hip, finish.hip) and the multi-pass decode (kernels.hip): is a json / jsonb text one
// JSON value (json_valid), and the array-literal state machine of the reference with its element parsers (arr_strip_dims, arr_walk,
// arr_spans). cell_text_error() joins them into the question ETLG_F_CHECK_CELLS asks of a DEFERRED cell: would the reference's
// parse_cell_from_postgres_text have failed on this text, and with which code?
#pragma once
#include "values.hip.h"
#include "float_slow.h"

namespace etlg {

DEV int arr_hexv(uint32_t c) { return c - '0' < 10u ? (int)(c - '0') : (c | 0x20u) - 'a' < 6u ? (int)((c | 0x20u) - 'a' + 10) : -1; }
// serde_json 1.0.149 `from_str::<Value>` (call site codec/text.rs:126-134; features arbitrary_precision + std, crates/etl/Cargo.toml:36):
// is the text one JSON value? RFC 8259 grammar; whitespace is space / tab / LF / CR; a number keeps its literal text, so any length
// and exponent is fine; strings reject raw control characters, unknown escapes, a \u surrogate without its partner; an array or
// object may be nested 127 deep (Deserializer::remaining_depth starts at 128 and entering a container that takes it to 0 is
// RecursionLimitExceeded); anything but whitespace behind the value is an error. The text is valid UTF-8 already (the decode
// kernels checked). Iterative: the open containers are a 128-bit stack (1 = object).
DEV bool json_valid(const u8* s, uint32_t n) {
  uint32_t stk[4] = {0, 0, 0, 0};
  uint32_t depth = 0, i = 0;
  enum : uint32_t { X_VALUE = 0, X_VALUE_OR_CLOSE = 1, X_KEY_OR_CLOSE = 2, X_KEY = 3, X_NEXT = 4 };
  uint32_t ex = X_VALUE;
  auto ws = [&]() { while (i < n && (s[i] == ' ' || s[i] == '\t' || s[i] == '\n' || s[i] == '\r')) i++; };
  auto hex4 = [&](uint32_t& v) -> bool {   // at s[i]: 'u' XXXX
    if (n - i < 5) return false;
    v = 0;
    for (uint32_t k = 1; k <= 4; k++) { const int d = arr_hexv(s[i + k]); if (d < 0) return false; v = v * 16 + (uint32_t)d; }
    i += 5;
    return true;
  };
  auto string = [&]() -> bool {   // at the opening quote
    i++;
    while (i < n) {
      const uint32_t c = s[i];
      if (c == '"') { i++; return true; }
      if (c < 0x20) return false;
      if (c != '\\') { i++; continue; }
      if (++i >= n) return false;
      const uint32_t x = s[i];
      if (x == 'u') {
        uint32_t v, w;
        if (!hex4(v)) return false;
        if (v >= 0xDC00 && v <= 0xDFFF) return false;
        if (v >= 0xD800 && v <= 0xDBFF) {
          if (n - i < 2 || s[i] != '\\' || s[i + 1] != 'u') return false;
          i++;
          if (!hex4(w) || w < 0xDC00 || w > 0xDFFF) return false;
        }
        continue;
      }
      if (!(x == '"' || x == '\\' || x == '/' || x == 'b' || x == 'f' || x == 'n' || x == 'r' || x == 't')) return false;
      i++;
    }
    return false;
  };
  auto digits = [&]() -> bool { const uint32_t i0 = i; while (i < n && s[i] - '0' < 10u) i++; return i > i0; };
  auto word = [&](const char* l, uint32_t ln) -> bool { if (n - i < ln) return false; for (uint32_t k = 0; k < ln; k++) if (s[i + k] != (u8)l[k]) return false; i += ln; return true; };
  for (;;) {
    ws();
    if (ex == X_NEXT) {
      if (!depth) return i == n;
      if (i >= n) return false;
      const uint32_t c = s[i++], top = depth - 1;
      const bool obj = (stk[top >> 5] >> (top & 31)) & 1u;
      if (c == ',') { ex = obj ? X_KEY : X_VALUE; continue; }
      if (c != (obj ? '}' : ']')) return false;
      depth--;
      continue;
    }
    if (i >= n) return false;
    const uint32_t c = s[i];
    if (ex == X_KEY_OR_CLOSE || ex == X_KEY) {
      if (ex == X_KEY_OR_CLOSE && c == '}') { i++; depth--; ex = X_NEXT; continue; }
      if (c != '"' || !string()) return false;
      ws();
      if (i >= n || s[i] != ':') return false;
      i++;
      ex = X_VALUE;
      continue;
    }
    if (ex == X_VALUE_OR_CLOSE && c == ']') { i++; depth--; ex = X_NEXT; continue; }
    if (c == '{' || c == '[') {
      if (depth >= 127) return false;
      if (c == '{') stk[depth >> 5] |= 1u << (depth & 31); else stk[depth >> 5] &= ~(1u << (depth & 31));
      depth++; i++;
      ex = c == '{' ? X_KEY_OR_CLOSE : X_VALUE_OR_CLOSE;
      continue;
    }
    bool ok;
    if (c == '"') ok = string();
    else if (c == 't') ok = word("true", 4);
    else if (c == 'f') ok = word("false", 5);
    else if (c == 'n') ok = word("null", 4);
    else {   // -? (0 | [1-9][0-9]*) (. [0-9]+)? ([eE] [+-]? [0-9]+)?
      if (c == '-') i++;
      if (i >= n) return false;
      if (s[i] == '0') i++; else if (s[i] - '1' < 9u) (void)digits(); else return false;
      ok = true;
      if (i < n && s[i] == '.') { i++; ok = digits(); }
      if (ok && i < n && (s[i] == 'e' || s[i] == 'E')) { i++; if (i < n && (s[i] == '+' || s[i] == '-')) i++; ok = digits(); }
    }
    if (!ok) return false;
    ex = X_NEXT;
  }
}

// ---- array literals (parse_cell_from_postgres_text_array, crates/etl/src/postgres/codec/text.rs:228-312; the dimensions
// prefix :163-214) for the element classes with a fixed-width value: bool, int2, int4, int8, oid, float4, float8, date, time,
// timestamp, timestamptz, uuid. One thread per row walks its
// text twice: k_arr_count (shape errors, element parse errors, element count), then k_arr_fill behind the offsets scan.
constexpr uint32_t kArrElemMax = 40;   // an element text longer than this is left to the host (Rust accepts any number of leading zeros)
enum : uint32_t { ARR_HOST = 0x100 };  // not an error: the row is handed back deferred

DEV uint32_t arr_strip_dims(const u8* s, uint32_t n, uint32_t& start) {   // strip_array_dimensions_prefix
  auto at = [&](uint32_t i) -> int { return i < n ? (int)s[i] : -1; };
  start = 0;
  if (at(0) != '[') return 0;
  uint32_t groups = 0, idx = 0;
  auto skip_int = [&](uint32_t i, uint32_t& out) { if (at(i) == '-') i++; const uint32_t st = i; while (at(i) >= '0' && at(i) <= '9') i++; out = i; return i > st; };
  while (at(idx) == '[') {
    uint32_t a, b;
    if (!skip_int(idx + 1, a) || at(a) != ':') return ETLG_E_ARRAY_DIMS;
    if (!skip_int(a + 1, b) || at(b) != ']') return ETLG_E_ARRAY_DIMS;
    idx = b + 1; groups++;
  }
  if (at(idx) != '=') return ETLG_E_ARRAY_DIMS;
  if (groups > 1) return ETLG_E_ARRAY_MULTIDIM;
  start = idx + 1;
  return 0;
}

// Calls elem(k, is_null, value words) per element in text order; returns 0, an etlg_err_code, or ARR_HOST.
// TEXT: string elements (ArrayCell::String: text[], varchar[], and every array type without a dedicated arm) are the unescaped
// bytes themselves; `dst(k)` says where element k's bytes go (nullptr: they are only counted).
// BYTEA elements (ArrayCell::Bytes, parse_bytea_hex_string per element, codec/hex.rs:11-52): TEXT walks with `hex` set — the element's
// characters are "\x" + hex pairs, decoded as they come; w[0] = the byte count.
template <bool TEXT, class F, class D>
DEV uint32_t arr_walk(const u8* s0, uint32_t n0, uint32_t elem_cls, uint32_t& count, F&& elem, D&& dst, bool exact_floats = false) {
  const bool hex = TEXT && elem_cls == ETLG_TC_BYTEA;
  bool hex_bad = false; uint32_t nib = 0;
  uint32_t start;
  count = 0;
  if (const uint32_t e = arr_strip_dims(s0, n0, start)) return e;
  const u8* s = s0 + start;
  const uint32_t n = n0 - start;
  if (n < 2) return ETLG_E_ARRAY_SHORT;
  if (s[0] != '{' || s[n - 1] != '}') return ETLG_E_ARRAY_BRACES;
  const u8* body = s + 1;
  const uint32_t bn = n - 2;
  u8 val[kArrElemMax];
  uint32_t vl = 0, pos = 0;
  bool in_quotes = false, in_escape = false, val_quoted = false, done = bn == 0, too_long = false;
  u8* out = TEXT ? dst(0u) : nullptr;
  while (!done) {
    for (;;) {
      if (pos >= bn) { done = true; break; }
      const u8 c = body[pos++];
      bool push = false;
      if (in_escape) { push = true; in_escape = false; }
      else if (c == '"') { if (!in_quotes) val_quoted = true; in_quotes = !in_quotes; }
      else if (c == '\\') in_escape = true;
      else if ((c == '{' || c == '}') && !in_quotes) return ETLG_E_ARRAY_MULTIDIM;
      else if (c == ',' && !in_quotes) break;
      else push = true;
      if (push) {
        if (vl < kArrElemMax) val[vl] = c; else too_long = true;
        if (hex) {   // characters 0, 1: "\x"; then pairs (an unquoted "null" has no backslash: it never looks like bytes)
          if (vl == 0) hex_bad |= c != '\\';
          else if (vl == 1) hex_bad |= c != 'x';
          else {
            const int h = arr_hexv(c);
            hex_bad |= h < 0;
            if (vl & 1) { if (out && !hex_bad) out[(vl - 3) >> 1] = (u8)((nib << 4) | (uint32_t)(h & 15)); } else nib = (uint32_t)(h & 15);   // (an unquoted NULL is four non-hex characters: it must not write)
          }
        }
        // a text element's bytes leave as they come, except the first four: an unquoted "null" is not text at all
        else if (TEXT && out && vl >= 4) { if (vl == 4) { out[0] = val[0]; out[1] = val[1]; out[2] = val[2]; out[3] = val[3]; } out[vl] = c; }
        vl++;
      }
    }
    if (in_quotes) return ETLG_E_ARRAY_QUOTE;
    if (in_escape) return ETLG_E_ARRAY_ESCAPE;
    if (!TEXT && too_long) return ARR_HOST;
    const bool is_null = !val_quoted && vl == 4 && (val[0] | 0x20) == 'n' && (val[1] | 0x20) == 'u' && (val[2] | 0x20) == 'l' && (val[3] | 0x20) == 'l';
    uint32_t w[4] = {0, 0, 0, 0};
    uint32_t scratch[(kArrElemMax + 7) / 4 + 2];   // a numeric element's heap entry (header + digits of <= 40 characters); a DEFERRED element's text
    if (hex) {
      if (!is_null) {   // "Bytea hex string conversion failed": no "\x", an odd count, a non-hex character (hex.rs:21-50)
        if (vl < 2 || hex_bad || (vl & 1)) return ETLG_E_BYTEA;
        w[0] = (vl - 2) >> 1;
      }
      hex_bad = false;
    } else if (TEXT) {
      if (out && !is_null && vl <= 4) for (uint32_t b = 0; b < vl; b++) out[b] = val[b];
      w[0] = is_null ? 0u : vl;
    } else if (!is_null) {
      uint32_t hcur = 0, st = 0;
      if (const uint32_t e = decode_text_cell<true>(elem_cls, val, vl, w, (u8*)scratch, hcur, st, false)) return e;
      if (st != ETLG_CELL_VALUE) {   // a float text the fast rule does not settle: the exact conversion (finish pass), else the host's
        if (!exact_floats || !(elem_cls == ETLG_TC_F32 || elem_cls == ETLG_TC_F64)) return ARR_HOST;
        const uint64_t bits = parse_float_exact_t([&](uint32_t i) { return (uint32_t)val[i]; }, vl, elem_cls == ETLG_TC_F32);
        w[0] = (uint32_t)bits; w[1] = (uint32_t)(bits >> 32);
      }
    }
    elem(count, is_null, w, (const u8*)scratch);
    count++;
    vl = 0; val_quoted = false;
    if (TEXT) out = dst(count);
  }
  return 0;
}

// The same walk for the row formats' text-like elements (ArrayCell::String / Bytes), which need an element's LENGTH in front of its
// bytes: elem(k, is_null, p0, p1, ulen) gets the element's source characters s0[p0 .. p1) — quotes and backslashes included — and its
// unescaped length; arr_unescape() then replays the span. Same checks, same NULL rule (an unquoted, unescaped "null" of any case).
template <class F>
DEV uint32_t arr_spans(const u8* s0, uint32_t n0, uint32_t& count, F&& elem) {
  uint32_t start;
  count = 0;
  if (const uint32_t e = arr_strip_dims(s0, n0, start)) return e;
  const uint32_t n = n0 - start;
  if (n < 2) return ETLG_E_ARRAY_SHORT;
  if (s0[start] != '{' || s0[start + n - 1] != '}') return ETLG_E_ARRAY_BRACES;
  const uint32_t b0 = start + 1, b1 = start + n - 1;   // the body
  uint32_t pos = b0;
  bool done = b1 == b0;
  while (!done) {
    const uint32_t p0 = pos;
    uint32_t p1 = b1, vl = 0, low4 = 0;
    bool in_quotes = false, in_escape = false, val_quoted = false, escaped = false;
    for (;;) {
      if (pos >= b1) { done = true; p1 = b1; break; }
      const u8 c = s0[pos++];
      bool push = false;
      if (in_escape) { push = true; in_escape = false; }
      else if (c == '"') { if (!in_quotes) val_quoted = true; in_quotes = !in_quotes; }
      else if (c == '\\') { in_escape = true; escaped = true; }
      else if ((c == '{' || c == '}') && !in_quotes) return ETLG_E_ARRAY_MULTIDIM;
      else if (c == ',' && !in_quotes) { p1 = pos - 1; break; }
      else push = true;
      if (push) { if (vl < 4) low4 |= (uint32_t)(c | 0x20) << (8 * vl); vl++; }
    }
    if (in_quotes) return ETLG_E_ARRAY_QUOTE;
    if (in_escape) return ETLG_E_ARRAY_ESCAPE;
    const bool is_null = !val_quoted && vl == 4 && low4 == 0x6C6C756Eu;   // "null" (an escaped n\ull is "null" too: the reference compares the unescaped value)
    (void)escaped;
    elem(count, is_null, p0, p1, vl);
    count++;
  }
  return 0;
}
template <class E>
DEV void arr_unescape(const u8* s0, uint32_t p0, uint32_t p1, E&& emit) {
  bool esc = false;
  for (uint32_t p = p0; p < p1; p++) {
    const u8 c = s0[p];
    if (esc) { emit(c); esc = false; } else if (c == '\\') esc = true; else if (c != '"') emit(c);
  }
}
// a bytea element's unescaped text: "\x" + hex pairs (parse_bytea_hex_string, codec/hex.rs:11-52)? Returns the byte count, or ~0u.
DEV uint32_t arr_bytea_len(const u8* s0, uint32_t p0, uint32_t p1, uint32_t ulen) {
  if (ulen < 2 || (ulen & 1)) return ~0u;
  uint32_t k = 0; bool bad = false;
  arr_unescape(s0, p0, p1, [&](u8 c) { if (k == 0) bad |= c != '\\'; else if (k == 1) bad |= c != 'x'; else bad |= arr_hexv(c) < 0; k++; });
  return bad ? ~0u : (ulen - 2) >> 1;
}

// ETLG_F_CHECK_CELLS: the error parse_cell_from_postgres_text (codec/text.rs:32-153) raises for the text of a json / jsonb / array cell —
// 0 when it accepts the text, ARR_HOST when a lane cannot decide (a non-text element of more than kArrElemMax characters, a json[]
// element of more than kChkJsonElemMax unescaped bytes: the cell stays DEFERRED and its parse stays the host's). The text is valid UTF-8
// already. Errors come in the reference's order: it parses every element where the element ends, so a bad element beats a shape error
// behind it.
constexpr uint32_t kChkJsonElemMax = 256;
DEV_NOINLINE uint32_t cell_text_error(uint32_t cls, uint32_t elem, const u8* s, uint32_t n) {
  if (cls == ETLG_TC_JSON) return json_valid(s, n) ? 0u : (uint32_t)ETLG_E_JSON;
  if (cls != ETLG_TC_ARRAY) return 0;
  uint32_t cnt = 0;
  auto none = [](uint32_t) -> u8* { return nullptr; };
  auto skip = [](uint32_t, bool, const uint32_t*, const u8*) {};
  if (elem == ETLG_TC_JSON) {
    u8 tmp[kChkJsonElemMax];
    uint32_t first = 0;   // what the first element that is not settled as valid gave
    const uint32_t e = arr_spans(s, n, cnt, [&](uint32_t, bool is_null, uint32_t p0, uint32_t p1, uint32_t ulen) {
      if (is_null || first) return;
      if (ulen > kChkJsonElemMax) { first = ARR_HOST; return; }
      uint32_t k = 0;
      arr_unescape(s, p0, p1, [&](u8 c) { tmp[k++] = c; });
      if (!json_valid(tmp, ulen)) first = ETLG_E_JSON;
    });
    return first ? first : e;
  }
  if (elem == ETLG_TC_BYTEA) return arr_walk<true>(s, n, elem, cnt, skip, none);
  const bool typed = elem == ETLG_TC_BOOL || elem == ETLG_TC_I16 || elem == ETLG_TC_I32 || elem == ETLG_TC_I64 || elem == ETLG_TC_U32 || elem == ETLG_TC_F32 ||
                     elem == ETLG_TC_F64 || elem == ETLG_TC_NUMERIC || elem == ETLG_TC_DATE || elem == ETLG_TC_TIME || elem == ETLG_TC_TIMETZ ||
                     elem == ETLG_TC_TIMESTAMP || elem == ETLG_TC_TIMESTAMPTZ || elem == ETLG_TC_UUID;
  // (exact floats: a float text the fast rule leaves open is a valid one, and the walk goes on to the elements behind it)
  if (typed) return arr_walk<false>(s, n, elem, cnt, skip, none, true);
  // ArrayCell::String (text[], varchar[], every array type without a dedicated arm): only the literal's shape can fail
  return arr_spans(s, n, cnt, [](uint32_t, bool, uint32_t, uint32_t, uint32_t) {});
}

}  // namespace etlg
