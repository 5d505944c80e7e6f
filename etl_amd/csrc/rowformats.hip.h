// The row formats of the hand-off: ClickHouse RowBinary, BigQuery protobuf, Snowflake NDJSON and DuckLake SQL literals —
// what their sources (rowformats.hip: RowBinary / protobuf and NDJSON; rowformats_dl.hip: DuckLake) instantiate. One thread per row, run
// twice over the rows columns.hip selected: k_rb_lens counts every row's bytes, the offsets scan (columns.hip, etlg_k_scan_blocks) places
// them, k_rb_rows writes them. Integer / byte work, HBM-bound: no MFMA.
#pragma once
#include "handoff.hip.h"
#include "float_json.h"
#include "float_display.h"

extern "C" void etlg_k_scan_blocks(const uint32_t* lens, uint64_t n, unsigned long long* blk, int64_t* offsets, unsigned long long* tot, hipStream_t st);   // columns.hip

namespace etlg {

// ---- ClickHouse RowBinary (crates/etl-destinations/src/clickhouse/encoding.rs:58-83 which wire type a Cell becomes,
// :188-283 the byte format; core.rs:96-114 the trailing CDC columns). One thread per row, run twice: lengths, then bytes.
constexpr int32_t kDate32Min = -25567, kDate32Max = 120529;   // 1900-01-01 .. 2299-12-31 (encoding.rs:147-173)

// A json cell as the sinks' `j.to_string()`: `head(len)` writes what goes in front of the string (its varint length). The text is
// checked in the counting pass only (a row that fails has length 0 and is not written). Returns 0, RB_E_JSON (not one JSON value: the
// reference fails at decode time, codec/text.rs:126-134), RB_E_HOST_CELL (json_display leaves it to the host), RB_E_BQ_NUMERIC_SCALE.
template <class S, class H>
DEV uint32_t rb_json(S& s, const u8* t, uint32_t tn, bool bq, H head) {
  if (std::is_same<S, RbCount>::value && !json_valid(t, tn)) return RB_E_JSON;
  JsCount c;
  const uint32_t e = json_display(c, t, tn, bq);
  if (e) return e == JD_BQ_INT ? RB_E_BQ_NUMERIC_SCALE : RB_E_HOST_CELL;
  head(c.n);
  if (std::is_same<S, RbCount>::value) s.zeros(c.n); else (void)json_display(s, t, tn, false);
  return 0;
}

// A json[] / jsonb[] literal for RowBinary, NDJSON and DuckLake, which rank alike: a literal the walk does not take apart or an element
// too long to look at makes the cell the host's before anything else (such an element may not be JSON at all); then the decode error;
// then an element beyond json_display's limits. (protobuf ranks its own rules between these: pb_array.) cnt: the element count.
template <class S>
DEV uint32_t json_arr_error(const u8* txt, uint32_t tn, u8* tmp, uint32_t& cnt) {
  JsonArrFacts f;
  if (json_arr_check<std::is_same<S, RbCount>::value>(txt, tn, tmp, cnt, f)) return RB_E_HOST_CELL;
  return f.too_long ? RB_E_HOST_CELL : f.bad_json ? RB_E_JSON : f.limit ? RB_E_HOST_CELL : 0u;
}

// One non-null value of class `cls` whose arena slot words start at `slot` (a row's slot, or the words decode_text_cell produced for
// an array element). Returns 0, RB_E_DATE_RANGE or RB_E_HOST_CELL.
// The counting pass notes where the row's `qparts` pieces (4, or 2 / 1 for narrow tables) begin; the byte pass writes a row with
// parts <= qparts lanes (1, 2 or 4 — chosen when the bytes per row are known), a lane taking qparts / parts pieces.
DEV uint32_t rb_part_col(const RbJob& j, uint32_t q) { return q * j.n_cols / j.qparts; }   // the first column of piece q

template <bool JS = false, class S>
DEV uint32_t rb_scalar(S& s, uint32_t cls, const u8* slot, const u8* heap) {
  const uint32_t w0 = ld32a(slot);
  switch (cls) {
    case ETLG_TC_BOOL: s.put(w0 ? 1 : 0); return 0;
    case ETLG_TC_I16: s.put((u8)w0); s.put((u8)(w0 >> 8)); return 0;
    case ETLG_TC_I32: case ETLG_TC_U32: case ETLG_TC_F32: s.put32(w0); return 0;
    case ETLG_TC_I64: case ETLG_TC_F64: s.put64(((uint64_t)ld32a(slot + 4) << 32) | w0); return 0;
    case ETLG_TC_DATE: {
      const int32_t days = (int32_t)w0 - kCeDays1970;
      if (days < kDate32Min || days > kDate32Max) return RB_E_DATE_RANGE;
      s.put32((uint32_t)days); return 0;
    }
    case ETLG_TC_TIME: {  // String(t.to_string()): chrono NaiveTime Display
      const uint32_t nanos = ld32a(slot + 4);
      s.varint64(8 + time_frac_len(nanos)); time_str(s, w0, nanos);
      return 0;
    }
    case ETLG_TC_TIMETZ: s.varint64(timetz_str_len(slot)); timetz_str(s, slot); return 0;   // String(t.to_string()) (encoding.rs:71)
    case ETLG_TC_NUMERIC: if (!heap) return RB_E_HOST_CELL; { const u8* ent = heap + w0; s.varint64(numeric_str_len(ent)); numeric_str(s, ent); return 0; }   // String(n.to_string()) (:66)
    case ETLG_TC_TIMESTAMP: case ETLG_TC_TIMESTAMPTZ: {
      const int64_t days = (int64_t)(int32_t)w0 - kCeDays1970;
      s.put64((uint64_t)((days * 86400 + (int64_t)ld32a(slot + 4)) * 1000000 + (int64_t)(ld32a(slot + 8) / 1000u))); return 0;
    }
    case ETLG_TC_UUID:  // high u64 LE then low u64 LE of the big-endian 16 bytes (:240-247)
      for (int h = 0; h < 2; h++) for (int k = 7; k >= 0; k--) s.put(slot[8 * h + k]);
      return 0;
    case ETLG_TC_STRING: if (!heap) return RB_E_HOST_CELL; { const uint32_t len = ld32a(slot + 4); s.varint64(len); s.bytes(heap + w0, len); return 0; }
    case ETLG_TC_BYTEA: if (!heap) return RB_E_HOST_CELL; { const uint32_t len = ld32a(slot + 4); s.varint64(2 * len); s.hex(heap + w0, len); return 0; }
    case ETLG_TC_JSON: if (!JS || !heap) return RB_E_HOST_CELL; return rb_json(s, heap + w0, ld32a(slot + 4), false, [&](uint32_t len) { s.varint64(len); });   // String(j.to_string()) (:73)
    default: return RB_E_HOST_CELL;
  }
}

// default_cell(typ) (clickhouse/core.rs:1481-1517) in RowBinary is a run of zero bytes: the type's width for the fixed-width classes
// (false, 0, 0.0, Date32 day 0 = 1970-01-01, DateTime64 0 = the epoch, Uuid::nil()), the varint 0 of an empty Array / an empty String
// (numeric, time, timetz, interval, bytea, text ...) for the rest. One length + one zero run instead of a switch over put32 / put64 /
// put64 x 2: hipcc (ROCm 7.2) compiled that switch inside rb_row's column loop with the output pointer left undefined behind the
// TIMESTAMP / TIMESTAMPTZ arm (k_rb_rows wrote through a stale register on the MI355X; profiles/r04_rowbinary_tombstone_fault.txt).
DEV uint32_t rb_default_zero_bytes(uint32_t cls) {
  uint32_t n = 1;                                                                                          // BOOL, and every String / Array class
  if (cls == ETLG_TC_I16) n = 2;
  if (cls == ETLG_TC_I32 || cls == ETLG_TC_U32 || cls == ETLG_TC_F32 || cls == ETLG_TC_DATE) n = 4;
  if (cls == ETLG_TC_I64 || cls == ETLG_TC_F64 || cls == ETLG_TC_TIMESTAMP || cls == ETLG_TC_TIMESTAMPTZ) n = 8;
  if (cls == ETLG_TC_UUID) n = 16;
  return n;
}

// [c_lo, c_hi): the columns this call writes (the byte pass splits a row among several lanes, k_rb_rows; the trailing columns go with
// the last part); mark(i) is called in front of column i (the counting pass notes where the parts begin).
template <bool JS, class S, class M>
DEV uint32_t rb_row(const RbJob& j, uint64_t r, S& s, uint32_t c_lo, uint32_t c_hi, M&& mark) {   // returns 0, or column << 8 | code of the cell that fails the row
  // The reference converts every cell of every pending row first (cell_to_clickhouse_value, clickhouse/core.rs:1193-1203: Date32
  // range errors) and only then encodes the rows (NULL in a non-nullable column): a range error anywhere beats a NULL error. So a
  // row that meets a cell without an encoding goes on looking for a date out of range; k_rb_lens ranks range errors first across rows.
  // A json cell that is not one JSON value fails earlier still — at decode time in the reference — so it beats both.
  const uint64_t base = j.row_base[r];
  uint32_t err0 = 0, errd = 0;
  // A Delete that carries only the key becomes the tombstone expand_key_row builds (clickhouse/core.rs:1437-1472): the key cells in
  // the primary-key columns, NULL in every other column that is nullable at the source and not an array, default_cell's zero value
  // (:1481-1517) in the rest. The host selects such rows only where the reference accepts them (host_handoff.inc).
  const bool keyrow = j.kcols && j.ev_kind[j.row_event[r]] == 'D' && (j.ev_flags[j.row_event[r]] & 3u) == ETLG_OLD_KEY;
  for (uint32_t i = c_lo; i < c_hi; i++) {
    mark(i);
    const uint32_t cd = j.cols[i], cls = cd & 0xFF;
    uint32_t off = cd >> 16, sti = i;
    const bool nullable = (cd >> 8) & 1;
    if (keyrow) {
      const uint32_t kc = j.kcols[i];
      if (kc & 1u) { off = kc >> 16; sti = (kc >> 8) & 0xFFu; }   // an identity column: its cell sits in the key layout
      else if ((kc & 2u) && cls != ETLG_TC_ARRAY) {                // Cell::Null
        if (!nullable) { if (!err0) err0 = (i << 8) | RB_E_NULL; continue; }
        s.put(1);
        continue;
      } else {                                                    // default_cell(typ)
        if (nullable) s.put(0);
        s.zeros(rb_default_zero_bytes(cls));
        continue;
      }
    }
    const uint32_t st = (j.fixed[base + sti / 4] >> (2 * (sti % 4))) & 3u;
    if (st == ETLG_CELL_NULL) {
      if (!nullable) { if (!err0) err0 = (i << 8) | RB_E_NULL; continue; }   // "NULL value for non-nullable ClickHouse column" (:217-225)
      s.put(1);
      continue;
    }
    const u8* slot = j.fixed + base + off;
    if (cls == ETLG_TC_ARRAY && st != ETLG_CELL_MISSING) {
      // Array(Nullable(T)) (:249-254): varint count, then every element with its null marker. The literal (kept as text in the
      // arena) is walked twice: count, then encode. A literal the device cannot take apart is the host's (it raises the exact error).
      const uint32_t elem = (cd >> 9) & 0x7Fu;
      if (elem == ETLG_TC_JSON && !JS) { if (!err0) err0 = (i << 8) | RB_E_HOST_CELL; continue; }
      const u8* txt = j.heap + ld32a(slot);
      const uint32_t tn = ld32a(slot + 4);
      if (JS && elem == ETLG_TC_JSON) {
        // json[] / jsonb[]: String(j.to_string()) per element (encoding.rs:109); an element that is not JSON is the reference's decode
        // error, as for a scalar cell
        u8 tmp[kJsonElemMax];
        uint32_t cnt = 0;
        const uint32_t bad = json_arr_error<S>(txt, tn, tmp, cnt);
        if (bad == RB_E_JSON) return (i << 8) | bad;
        if (bad) { if (!err0) err0 = (i << 8) | bad; continue; }
        if (nullable) s.put(0);
        s.varint64(cnt);
        json_arr_visit(txt, tn, tmp, [&](uint32_t, bool is_null, const u8* t, uint32_t n) {
          if (is_null) { s.put(1); return; }
          s.put(0);
          JsCount c;
          (void)json_display(c, t, n, false);
          s.varint64(c.n);
          if (std::is_same<S, RbCount>::value) s.zeros(c.n); else (void)json_display(s, t, n, false);
        });
        continue;
      }
      if (elem == ETLG_TC_STRING || elem == ETLG_TC_BYTEA) {
        // text-like elements are String(the unescaped bytes), bytea elements String(bytes_to_hex(..)) (array_cell_to_clickhouse_values,
        // encoding.rs:89-111): the lowercase hex digits of the element's own "\x.." text
        uint32_t cnt = 0; bool bad = false;
        if (arr_spans(txt, tn, cnt, [&](uint32_t, bool is_null, uint32_t p0, uint32_t p1, uint32_t ulen) {
              if (elem == ETLG_TC_BYTEA && !is_null && arr_bytea_len(txt, p0, p1, ulen) == ~0u) bad = true;
            }) || bad) { if (!err0) err0 = (i << 8) | RB_E_HOST_CELL; continue; }
        if (nullable) s.put(0);
        s.varint64(cnt);
        (void)arr_spans(txt, tn, cnt, [&](uint32_t, bool is_null, uint32_t p0, uint32_t p1, uint32_t ulen) {
          if (is_null) { s.put(1); return; }
          s.put(0);
          if (elem == ETLG_TC_STRING) { s.varint64(ulen); arr_unescape(txt, p0, p1, [&](u8 c) { s.put(c); }); }
          else { uint32_t k = 0; s.varint64(ulen - 2); arr_unescape(txt, p0, p1, [&](u8 c) { if (k++ >= 2) s.put((u8)(c - 'A' < 6u ? c | 0x20 : c)); }); }
        });
        continue;
      }
      uint32_t cnt = 0;
      auto none = [](uint32_t) -> u8* { return nullptr; };
      if (arr_walk<false>(txt, tn, elem, cnt, [](uint32_t, bool, const uint32_t*, const u8*) {}, none)) { if (!err0) err0 = (i << 8) | RB_E_HOST_CELL; continue; }
      if (nullable) s.put(0);
      s.varint64(cnt);
      uint32_t ee = 0;
      (void)arr_walk<false>(txt, tn, elem, cnt, [&](uint32_t, bool is_null, const uint32_t* w, const u8* scratch) {
        if (is_null) { s.put(1); return; }
        s.put(0);
        const uint32_t e1 = rb_scalar(s, elem, (const u8*)w, scratch);   // (a numeric element's entry sits in the walk's scratch: String(n.to_string()); timetz: String(t.to_string()))
        if (e1 && !ee) ee = e1;
      }, none);
      if (ee == RB_E_DATE_RANGE) { if (!errd) errd = (i << 8) | ee; }
      else if (ee && !err0) err0 = (i << 8) | ee;
      continue;
    }
    if (st != ETLG_CELL_VALUE && !(cls == ETLG_TC_JSON && st == ETLG_CELL_DEFERRED)) { if (!err0) err0 = (i << 8) | RB_E_HOST_CELL; continue; }   // (json cells are source text in the arena: DEFERRED)
    if (nullable) s.put(0);
    if (const uint32_t e = rb_scalar<JS>(s, cls, slot, j.heap)) {
      if (e == RB_E_JSON) return (i << 8) | e;
      if (e == RB_E_DATE_RANGE) { if (!errd) errd = (i << 8) | e; }
      else if (!err0) err0 = (i << 8) | e;
    }
  }
  if (errd) return errd;
  if (err0) return err0;
  if (c_hi != j.n_cols) return 0;
  // trailing CDC columns (core.rs:96-114); never NULL, a Nullable() destination column still takes its marker byte
  const uint64_t ev = j.row_event[r];
  const uint32_t kind = j.ev_kind[ev];
  // (a table-copy batch: append_cdc_columns(Insert, PgLsn 0, tx_ordinal 0), clickhouse/core.rs:739-773 — the virtual transaction's
  // events are Inserts already; its ordinals count up)
  const uint64_t lsn = j.copy_tail ? 0ull : j.ev_commit[ev], ord = j.copy_tail ? 0ull : j.ev_ord[ev];
  if (j.cdc_nullable & 1u) s.put(0);
  if (j.engine == 0) {
    s.put(6);
    const char* op = kind == 'I' ? "INSERT" : kind == 'U' ? "UPDATE" : "DELETE";
    for (int k = 0; k < 6; k++) s.put((u8)op[k]);
    if (j.cdc_nullable & 2u) s.put(0);
    s.put64(lsn);
  } else {
    s.put64(ord); s.put64(lsn);   // u128 = commit_lsn << 64 | tx_ordinal, little endian
    if (j.cdc_nullable & 2u) s.put(0);
    s.put(kind == 'D' ? 1 : 0);
  }
  return 0;
}


// ---- BigQuery protobuf rows (cell_encode_prost, crates/etl-destinations/src/bigquery/encoding.rs:120-190; the wire format is
// prost's = protobuf's: key = varint(tag << 3 | wire type), wire types 0 varint, 1 fixed64, 2 length-delimited, 5 fixed32; int32 /
// int64 as sign-extended 64-bit varints). Insert rows only: the row's cells with tags 1..n (NULL cells leave nothing), then
// _CHANGE_TYPE = "UPSERT" and _CHANGE_SEQUENCE_NUMBER = "{commit_lsn:016x}/{tx_ordinal:016x}/{0:016x}" (bigquery/core.rs:978-996,
// 1404-1406; EventSequenceKey Display, crates/etl/src/event.rs:346-351).
template <class S> DEV void pb_key(S& s, uint32_t tag, uint32_t wt) { s.varint64(((uint64_t)tag << 3) | wt); }
template <class S> DEV void pb_hex16(S& s, uint64_t v) { for (int k = 15; k >= 0; k--) { const uint32_t d = (uint32_t)(v >> (4 * k)) & 15u; s.put((u8)hex_digit(d)); } }
template <class S> DEV void put_uuid(S& s, const u8* b16) {   // Uuid Display: hyphenated lowercase
  for (int k = 0; k < 16; k++) {
    if (k == 4 || k == 6 || k == 8 || k == 10) s.put('-');
    s.put((u8)hex_digit(b16[k] >> 4)); s.put((u8)hex_digit(b16[k] & 15u));
  }
}
// days from CE (chrono) -> civil date: "%Y-%m-%d" (DATE_FORMAT, etl-postgres/src/time.rs:13); years 0000-9999 (the others are DEFERRED)
template <class S> DEV void pb_date(S& s, int32_t days_ce) {
  const int64_t z = (int64_t)days_ce - kCeDays1970 + 719468;
  const int64_t era = (z >= 0 ? z : z - 146096) / 146097;
  const uint32_t doe = (uint32_t)(z - era * 146097);
  const uint32_t yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
  const uint32_t doy = doe - (365 * yoe + yoe / 4 - yoe / 100);
  const uint32_t mp = (5 * doy + 2) / 153;
  const uint32_t d = doy - (153 * mp + 2) / 5 + 1, m = mp < 10 ? mp + 3 : mp - 9;
  const int64_t y = (int64_t)yoe + era * 400 + (m <= 2 ? 1 : 0);
  put_4d(s, (uint32_t)y); s.put('-'); put_2d(s, m); s.put('-'); put_2d(s, d);
}
// An array cell (array_cell_encode_prost, bigquery/encoding.rs:203-290) behind validate_array_cell_for_bigquery (validation.rs:125-190:
// a NULL element fails the row). Element classes with a fixed-width value, as in RowBinary: bool / int2 / int4 / oid / int8 / float4 /
// float8 and timestamptz (epoch microseconds) leave PACKED — one length-delimited field of the values back to back (varints, or 4- / 8-
// byte words), nothing at all for an empty array; date / time / timestamp / uuid leave as one string field per element. The literal is
// walked once for the element count, the NULLs and the packed length, once for the bytes. A literal the device does not take apart
// (malformed: the reference's decode error, which the host raises; an element of more than 40 characters) is RB_E_HOST_CELL.
template <bool JS, class S>
DEV uint32_t pb_array(S& s, uint32_t tag, uint32_t elem, const u8* txt, uint32_t tn) {
  if (elem == ETLG_TC_JSON && !JS) return RB_E_HOST_CELL;
  if (JS && elem == ETLG_TC_JSON) {   // one string field per element: j.to_string() behind reject_nulls and validate_elements(validate_json_for_bigquery) (validation.rs:185-188)
    // Which report a cell with several problems gets: an element too long to look at makes the cell the host's (it may not even be JSON);
    // then the decode error (an element that is not JSON); then the sink's own, in the reference's order — reject_nulls over the whole
    // array, validate_elements after it; an element beyond json_display's limits last (it could only add the integer rule's report).
    // One walk: an element goes out as soon as it has passed, while nothing in front of it has failed the row.
    u8 tmp[kJsonElemMax];
    uint32_t cnt = 0;
    JsonArrFacts f;
    if (json_arr_check<std::is_same<S, RbCount>::value>(txt, tn, true, tmp, cnt, f, [&](const u8* t, uint32_t n, uint32_t len) {
          if (f.any()) return;   // (nothing of this row will be kept)
          pb_key(s, tag, 2); s.varint64(len);
          if (std::is_same<S, RbCount>::value) s.zeros(len); else (void)json_display(s, t, n, false);
        })) return RB_E_HOST_CELL;
    return f.too_long ? RB_E_HOST_CELL : f.bad_json ? RB_E_JSON : f.has_null ? RB_E_BQ_ARRAY_NULL : f.bq_int ? RB_E_BQ_NUMERIC_SCALE : f.limit ? RB_E_HOST_CELL : 0u;
  }
  if (elem == ETLG_TC_STRING || elem == ETLG_TC_BYTEA) {   // one string / bytes field per element: the unescaped bytes / the decoded bytes
    uint32_t cnt = 0;
    bool has_null = false, bad = false;   // (a bytea element that is not "\x" + hex pairs is the reference's decode error — the host raises it — and comes before the sink's NULL rule)
    if (arr_spans(txt, tn, cnt, [&](uint32_t, bool is_null, uint32_t p0, uint32_t p1, uint32_t ulen) {
          if (is_null) { has_null = true; return; }
          if (elem == ETLG_TC_STRING) { if (!has_null) { pb_key(s, tag, 2); s.varint64(ulen); arr_unescape(txt, p0, p1, [&](u8 c) { s.put(c); }); } return; }
          const uint32_t nb = arr_bytea_len(txt, p0, p1, ulen);
          if (nb == ~0u) { bad = true; return; }
          if (has_null | bad) return;
          pb_key(s, tag, 2); s.varint64(nb);
          uint32_t k = 0, hi = 0;
          arr_unescape(txt, p0, p1, [&](u8 c) { if (k >= 2) { const uint32_t h = (uint32_t)arr_hexv(c); if (k & 1) s.put((u8)((hi << 4) | h)); else hi = h; } k++; });
        })) return RB_E_HOST_CELL;
    return bad ? RB_E_HOST_CELL : has_null ? RB_E_BQ_ARRAY_NULL : 0u;
  }
  const bool packed = elem == ETLG_TC_BOOL || elem == ETLG_TC_I16 || elem == ETLG_TC_I32 || elem == ETLG_TC_U32 || elem == ETLG_TC_I64 ||
                      elem == ETLG_TC_F32 || elem == ETLG_TC_F64 || elem == ETLG_TC_TIMESTAMPTZ;
  auto none = [](uint32_t) -> u8* { return nullptr; };
  auto value64 = [&](const uint32_t* w) -> uint64_t {   // what the varint of an element holds
    if (elem == ETLG_TC_I16 || elem == ETLG_TC_I32) return (uint64_t)(int64_t)(int32_t)w[0];
    if (elem == ETLG_TC_I64) return ((uint64_t)w[1] << 32) | w[0];
    if (elem == ETLG_TC_TIMESTAMPTZ) return (uint64_t)((((int64_t)(int32_t)w[0] - kCeDays1970) * 86400 + (int64_t)w[1]) * 1000000 + (int64_t)(w[2] / 1000u));
    return (uint64_t)w[0];   // bool, oid
  };
  uint32_t cnt = 0, nulls = 0, plen = 0;
  bool scale_bad = false;
  if (arr_walk<false>(txt, tn, elem, cnt, [&](uint32_t, bool is_null, const uint32_t* w, const u8* scratch) {
        if (is_null) { nulls++; return; }
        if (elem == ETLG_TC_F32) plen += 4; else if (elem == ETLG_TC_F64) plen += 8; else if (elem == ETLG_TC_BOOL) plen += 1;
        else if (packed) { uint64_t v = value64(w); do { plen++; v >>= 7; } while (v); }
        else if (elem == ETLG_TC_NUMERIC) {   // validate_elements(validate_numeric_for_bigquery) behind reject_nulls (validation.rs:169-172)
          const u8* ent = scratch + w[0];
          if (ent[0] == ETLG_NUM_VALUE && ((uint32_t)ent[4] | ((uint32_t)ent[5] << 8)) > 38u) scale_bad = true;
        }
      }, none)) return RB_E_HOST_CELL;
  if (nulls) return RB_E_BQ_ARRAY_NULL;
  if (scale_bad) return RB_E_BQ_NUMERIC_SCALE;
  if (!cnt) return 0;
  if (packed) { pb_key(s, tag, 2); s.varint64(plen); }
  (void)arr_walk<false>(txt, tn, elem, cnt, [&](uint32_t, bool, const uint32_t* w, const u8* scratch) {
    switch (elem) {
      case ETLG_TC_NUMERIC: { const u8* ent = scratch + w[0]; pb_key(s, tag, 2); s.varint64(numeric_str_len(ent)); numeric_str(s, ent); break; }
      case ETLG_TC_TIMETZ: pb_key(s, tag, 2); s.varint64(timetz_str_len((const u8*)w)); timetz_str(s, (const u8*)w); break;
      case ETLG_TC_BOOL: s.put(w[0] ? 1 : 0); break;
      case ETLG_TC_F32: s.put32(w[0]); break;
      case ETLG_TC_F64: s.put64(((uint64_t)w[1] << 32) | w[0]); break;
      case ETLG_TC_DATE: pb_key(s, tag, 2); s.varint64(10); pb_date(s, (int32_t)w[0]); break;
      case ETLG_TC_TIME: pb_key(s, tag, 2); s.varint64(8 + time_frac_len(w[1])); time_str(s, w[0], w[1]); break;
      case ETLG_TC_TIMESTAMP: pb_key(s, tag, 2); s.varint64(19 + time_frac_len(w[2])); pb_date(s, (int32_t)w[0]); s.put(' '); time_str(s, w[1], w[2]); break;
      case ETLG_TC_UUID: pb_key(s, tag, 2); s.varint64(36); put_uuid(s, (const u8*)w); break;
      default: s.varint64(value64(w)); break;
    }
  }, none);
  return 0;
}

template <bool JS, class S, class M>
DEV uint32_t pb_row(const RbJob& j, uint64_t r, S& s, uint32_t c_lo, uint32_t c_hi, M&& mark) {
  // (the row's kind sits in the top bits of its base: ColSel / pb_selected)
  const unsigned long long rbase = j.row_base[r];
  const bool del = (rbase & kPbDelete) != 0, keyimg = (rbase & kPbKey) != 0;
  const uint64_t base = rbase & kPbBase;
  uint32_t err0 = 0;
  for (uint32_t i = c_lo; i < c_hi; i++) {
    mark(i);
    const uint32_t cd = j.cols[i], cls = cd & 0xFF, tag = i + 1;
    uint32_t off = cd >> 16, sti = i;
    if (del) {  // bigquery_delete_row (core.rs:1742-1754): only the primary-key cells of the old image, under their column tags
      const uint32_t kc = j.kcols[i];
      if (!(kc & 4u)) continue;
      if (keyimg) { off = kc >> 16; sti = (kc >> 8) & 0xFFu; }
    }
    const uint32_t st = (j.fixed[base + sti / 4] >> (2 * (sti % 4))) & 3u;
    if (st == ETLG_CELL_NULL) continue;                       // Cell::Null => {}
    if (st != ETLG_CELL_VALUE && !((cls == ETLG_TC_JSON || cls == ETLG_TC_ARRAY) && st == ETLG_CELL_DEFERRED)) { if (!err0) err0 = (i << 8) | RB_E_HOST_CELL; continue; }
    const u8* slot = j.fixed + base + off;
    const uint32_t w0 = ld32a(slot);
    if (cls == ETLG_TC_ARRAY) {
      if (const uint32_t e = pb_array<JS>(s, tag, (cd >> 9) & 0x7Fu, j.heap + w0, ld32a(slot + 4))) {
        if (e == RB_E_JSON) return (i << 8) | e;
        if (!err0) err0 = (i << 8) | e;
      }
      continue;
    }
    switch (cls) {
      case ETLG_TC_BOOL: pb_key(s, tag, 0); s.put(w0 ? 1 : 0); break;
      case ETLG_TC_I16: case ETLG_TC_I32: pb_key(s, tag, 0); s.varint64((uint64_t)(int64_t)(int32_t)w0); break;
      case ETLG_TC_I64: pb_key(s, tag, 0); s.varint64(((uint64_t)ld32a(slot + 4) << 32) | w0); break;
      case ETLG_TC_U32: pb_key(s, tag, 0); s.varint64((uint64_t)w0); break;
      case ETLG_TC_F32: pb_key(s, tag, 5); s.put32(w0); break;
      case ETLG_TC_F64: pb_key(s, tag, 1); s.put64(((uint64_t)ld32a(slot + 4) << 32) | w0); break;
      case ETLG_TC_STRING: case ETLG_TC_BYTEA: { const uint32_t len = ld32a(slot + 4); pb_key(s, tag, 2); s.varint64(len); s.bytes(j.heap + w0, len); break; }
      case ETLG_TC_DATE: pb_key(s, tag, 2); s.varint64(10); pb_date(s, (int32_t)w0); break;
      case ETLG_TC_TIME: { const uint32_t ns = ld32a(slot + 4); pb_key(s, tag, 2); s.varint64(8 + time_frac_len(ns)); time_str(s, w0, ns); break; }
      case ETLG_TC_TIMESTAMP: {  // "%Y-%m-%d %H:%M:%S%.f" (TIMESTAMP_FORMAT :21)
        const uint32_t secs = ld32a(slot + 4), ns = ld32a(slot + 8);
        pb_key(s, tag, 2); s.varint64(19 + time_frac_len(ns)); pb_date(s, (int32_t)w0); s.put(' '); time_str(s, secs, ns); break;
      }
      case ETLG_TC_TIMESTAMPTZ: {  // epoch microseconds as int64 (:176-179)
        const int64_t days = (int64_t)(int32_t)w0 - kCeDays1970;
        pb_key(s, tag, 0); s.varint64((uint64_t)((days * 86400 + (int64_t)ld32a(slot + 4)) * 1000000 + (int64_t)(ld32a(slot + 8) / 1000u))); break;
      }
      case ETLG_TC_UUID: pb_key(s, tag, 2); s.varint64(36); put_uuid(s, slot); break;
      case ETLG_TC_TIMETZ: pb_key(s, tag, 2); s.varint64(timetz_str_len(slot)); timetz_str(s, slot); break;   // t.to_string() (:158-161)
      case ETLG_TC_NUMERIC: {  // n.to_string() (:146-149) behind validate_numeric_for_bigquery (bigquery/validation.rs:20-35): more than 38 decimal places would be rounded
        const u8* ent = j.heap + w0;
        if (ent[0] == ETLG_NUM_VALUE && ((uint32_t)ent[4] | ((uint32_t)ent[5] << 8)) > 38u) { if (!err0) err0 = (i << 8) | RB_E_BQ_NUMERIC_SCALE; break; }
        pb_key(s, tag, 2); s.varint64(numeric_str_len(ent)); numeric_str(s, ent); break;
      }
      case ETLG_TC_JSON: {  // j.to_string() (:173-176) behind validate_json_for_bigquery (bigquery/validation.rs:47-85)
        if (!JS) { if (!err0) err0 = (i << 8) | RB_E_HOST_CELL; break; }
        if (const uint32_t e = rb_json(s, j.heap + w0, ld32a(slot + 4), true, [&](uint32_t len) { pb_key(s, tag, 2); s.varint64(len); })) {
          if (e == RB_E_JSON) return (i << 8) | e;   // (the reference's decode fails before the sink validates anything: it beats an earlier cell's report)
          if (!err0) err0 = (i << 8) | e;
        }
        break;
      }
      default: if (!err0) err0 = (i << 8) | RB_E_HOST_CELL; break;   // arrays: packed / repeated fields, host-side validation
    }
  }
  if (err0) return err0;
  if (c_hi != j.n_cols) return 0;
  const uint64_t ev = j.row_event[r];
  pb_key(s, j.n_cols + 1, 2); s.varint64(6);
  { const char* op = del ? "DELETE" : "UPSERT"; for (int k = 0; k < 6; k++) s.put((u8)op[k]); }
  if (j.copy_tail) return 0;   // a copied row has no _CHANGE_SEQUENCE_NUMBER field (write_table_rows, bigquery/core.rs:602-649)
  pb_key(s, j.n_cols + 2, 2); s.varint64(50);
  pb_hex16(s, j.ev_commit[ev]); s.put('/'); pb_hex16(s, j.ev_ord[ev]); s.put('/'); pb_hex16(s, (rbase & kPbSecond) ? 1 : 0);   // bigquery_sequence_key (:1405-1407)
  return 0;
}

// ---- an array cell as a bracketed list, for the two text formats (NDJSON: a JSON array; DuckLake: a list literal). F, the format, gives
// what they differ in: sep(s) between two elements, null(s) for a NULL element, value(s, cls, slot, heap) for an element that has slot
// words, and the writers of the elements that have none — str / bytea / numeric(s, ...) for contiguous bytes (typed arrays), str_elem /
// bytea_elem(s, txt, p0, p1) for a span of the literal (arr_unescape replays it), json(s, text, n) for a json element the check accepted.
//
// An array cell that is still its source literal (DEFERRED): NULL elements as F::null, every element by the scalar rules
// (ArrayCellSerializer, snowflake/encoding.rs:186-224; array_cell_to_sql_literal, ducklake/encoding.rs:470-585). Returns 0, the first
// element's error, RB_E_JSON (a json[] element that is not JSON) or RB_E_HOST_CELL (a literal the walkers do not take apart, a json
// element beyond json_display's limits or longer than kJsonElemMax).
template <class F, bool JS, class S>
DEV uint32_t text_array(S& s, uint32_t elem, const u8* txt, uint32_t tn) {
  uint32_t cnt = 0, k = 0;
  if (elem == ETLG_TC_JSON) {   // json[] / jsonb[] (ArrayCell::Json)
    if (!JS) return RB_E_HOST_CELL;
    u8 tmp[kJsonElemMax];
    if (const uint32_t bad = json_arr_error<S>(txt, tn, tmp, cnt)) return bad;
    s.put('[');
    json_arr_visit(txt, tn, tmp, [&](uint32_t, bool is_null, const u8* t, uint32_t n) {
      if (k++) F::sep(s);
      if (is_null) { F::null(s); return; }
      F::json(s, t, n);
    });
    s.put(']');
    return 0;
  }
  if (elem == ETLG_TC_STRING || elem == ETLG_TC_BYTEA) {   // the unescaped text; bytea: the hex digits of its "\x.." text
    bool bad = false;
    if (arr_spans(txt, tn, cnt, [&](uint32_t, bool is_null, uint32_t p0, uint32_t p1, uint32_t ulen) {
          if (elem == ETLG_TC_BYTEA && !is_null && arr_bytea_len(txt, p0, p1, ulen) == ~0u) bad = true;
        }) || bad) return RB_E_HOST_CELL;
    s.put('[');
    (void)arr_spans(txt, tn, cnt, [&](uint32_t, bool is_null, uint32_t p0, uint32_t p1, uint32_t) {
      if (k++) F::sep(s);
      if (is_null) { F::null(s); return; }
      if (elem == ETLG_TC_STRING) F::str_elem(s, txt, p0, p1); else F::bytea_elem(s, txt, p0, p1);
    });
    s.put(']');
    return 0;
  }
  auto none = [](uint32_t) -> u8* { return nullptr; };
  if (arr_walk<false>(txt, tn, elem, cnt, [](uint32_t, bool, const uint32_t*, const u8*) {}, none)) return RB_E_HOST_CELL;
  uint32_t ee = 0;
  s.put('[');
  (void)arr_walk<false>(txt, tn, elem, cnt, [&](uint32_t, bool is_null, const uint32_t* w, const u8* scratch) {
    if (k++) F::sep(s);
    if (is_null) { F::null(s); return; }
    const uint32_t e1 = F::value(s, elem, (const u8*)w, scratch);
    if (e1 && !ee) ee = e1;
  }, none);
  s.put(']');
  return ee;
}
// A typed array (ETLG_F_FINISH_CELLS: a VALUE cell whose slot holds an etlg_array_hdr entry) from its header — never as text.
template <class F, class S>
DEV uint32_t typed_array(S& s, const u8* h) {
  const uint32_t n = ld32a(h), elem = h[4], eb = h[5];
  const uint32_t* valid = (const uint32_t*)(h + 8);
  const u8* body = h + 8 + 4u * ((n + 31u) / 32u);
  const uint32_t* end = (const uint32_t*)body;
  const u8* data = body + 4u * n;
  uint32_t ee = 0;
  s.put('[');
  for (uint32_t k = 0; k < n; k++) {
    if (k) F::sep(s);
    if (!((valid[k >> 5] >> (k & 31u)) & 1u)) { F::null(s); continue; }
    uint32_t e1 = 0;
    if (eb) e1 = F::value(s, elem, body + (size_t)k * eb, nullptr);
    else {
      const uint32_t a = k ? end[k - 1] : 0u, b = end[k];
      if (elem == ETLG_TC_STRING) F::str(s, data + a, b - a);
      else if (elem == ETLG_TC_BYTEA) F::bytea(s, data + a, b - a);
      else if (elem == ETLG_TC_NUMERIC) e1 = F::numeric(s, data + a);
      else e1 = RB_E_HOST_CELL;
    }
    if (e1 && !ee) ee = e1;
  }
  s.put(']');
  return ee;
}

// ---- Snowflake NDJSON rows (serialize_row, crates/etl-destinations/src/snowflake/encoding.rs:57-72; CellSerializer /
// ArrayCellSerializer :94-280): one serde_json compact map per row, `"<col>":<value>` in column order, then "_cdc_operation" and
// "_cdc_sequence_number" = OffsetToken::new (snowflake/streaming/offset_token.rs:21-23), then '\n'. Every column is written as its key
// (escaped once by the host: RbJob.nd_keys), its value and a ',' — the trailing CDC pair always follows, so the bytes are serde_json's.
// Rows: Insert, the new row of a full Update, the old row of a Delete — only the identity columns for a key image (core.rs:345-438,
// :572-608). Errors are the sink's Error::Encoding (non-finite floats, numeric NaN / Infinity); the host turns the codes into them.

// serde_json's escape table (format_escaped_str): '"' '\\' and the bytes below 0x20 are escaped, everything else is raw
DEV uint32_t nd_esc_extra(uint32_t c) {
  if (c == '"' || c == '\\' || c == 8u || c == 12u || c == '\n' || c == '\r' || c == '\t') return 1;
  return c < 0x20u ? 5u : 0u;
}
template <class S> DEV void nd_esc_put(S& s, uint32_t c) {
  if (c >= 0x20u && c != '"' && c != '\\') { s.put((u8)c); return; }
  s.put('\\');
  switch (c) {
    case '"': s.put('"'); break;
    case '\\': s.put('\\'); break;
    case 8u: s.put('b'); break;
    case 12u: s.put('f'); break;
    case '\n': s.put('n'); break;
    case '\r': s.put('r'); break;
    case '\t': s.put('t'); break;
    default: s.put('u'); s.put('0'); s.put('0'); s.put((u8)('0' + (c >> 4))); s.put((u8)hex_digit(c & 15u)); break;
  }
}
// bit 7 of some byte set <=> one of the eight bytes is below 0x20, '"' or '\\' (the has-less / has-zero tests: exact for "any")
DEV uint64_t nd_swar_esc(uint64_t w) {
  const uint64_t L = 0x0101010101010101ull, q = w ^ (0x22u * L), b = w ^ (0x5Cu * L);
  return (((w - 0x20u * L) & ~w) | ((q - L) & ~q) | ((b - L) & ~b)) & (0x80u * L);
}
// a JSON string of n bytes: the count pass tests eight bytes at a time and looks at single bytes only in a word that has something to
// escape; the byte pass copies 16-byte pieces that have nothing and escapes byte by byte only inside a piece that has
template <class S> DEV void nd_str(S& s, const u8* p, uint32_t n) {
  s.put('"');
  uint32_t k = 0;
  if constexpr (std::is_same<S, RbCount>::value) {
    uint32_t extra = 0;
    for (; k + 8u <= n; k += 8u) {
      uint64_t w; __builtin_memcpy(&w, p + k, 8);
      if (nd_swar_esc(w)) for (uint32_t b = 0; b < 8u; b++) extra += nd_esc_extra(p[k + b]);
    }
    for (; k < n; k++) extra += nd_esc_extra(p[k]);
    s.zeros(n + extra);
  } else {
    for (; k + 16u <= n; k += 16u) {
      uint64_t v[2]; __builtin_memcpy(v, p + k, 16);
      if (!(nd_swar_esc(v[0]) | nd_swar_esc(v[1]))) { s.append(v[0], 8); s.append(v[1], 8); }
      else for (uint32_t b = 0; b < 16u; b++) nd_esc_put(s, p[k + b]);
    }
    for (; k < n; k++) nd_esc_put(s, p[k]);
  }
  s.put('"');
}
template <class S> DEV void nd_lit(S& s, const char* t) { while (*t) s.put((u8)*t++); }
template <class S> DEV void nd_u64(S& s, uint64_t v) {
  u8 d[20];
  uint32_t n = 0;
  if (v >> 32) { do { d[n++] = (u8)('0' + v % 10u); v /= 10u; } while (v >> 32); }
  uint32_t x = (uint32_t)v;
  do { d[n++] = (u8)('0' + x % 10u); x /= 10u; } while (x);
  while (n) s.put(d[--n]);
}
template <class S> DEV void nd_i64(S& s, int64_t v) { if (v < 0) { s.put('-'); nd_u64(s, 0ull - (uint64_t)v); } else nd_u64(s, (uint64_t)v); }
template <class S> DEV uint32_t nd_numeric(S& s, const u8* ent) {   // serialize_pg_numeric (:147-159)
  if (ent[0] == ETLG_NUM_NAN) return ND_E_NUM_NAN;
  if (ent[0] != ETLG_NUM_VALUE) return ND_E_NUM_INF;
  s.put('"'); numeric_str(s, ent); s.put('"');
  return 0;
}
template <class S> DEV uint32_t nd_float(S& s, uint64_t bits, bool is32) {   // reject_non_finite (:162-169), then ryu (float_json.h)
  const uint32_t eb = is32 ? 23u : 52u, emax = is32 ? 0xFFu : 0x7FFu;
  if (((uint32_t)(bits >> eb) & emax) == emax) {
    if (bits & ((1ull << eb) - 1u)) return ND_E_FLOAT_NAN;
    return (bits >> (is32 ? 31 : 63)) & 1u ? ND_E_FLOAT_NINF : ND_E_FLOAT_INF;
  }
  (void)float_json(s, bits, is32);
  return 0;
}
// One non-null value of class `cls` whose slot words start at `slot` (a row's slot, an element's words from the walk or from a typed
// array); `heap`: where a numeric's entry / a text's bytes are (the arena's heap, or the walk's scratch for numeric elements).
template <class S>
DEV uint32_t nd_value(S& s, uint32_t cls, const u8* slot, const u8* heap) {
  const uint32_t w0 = ld32a(slot);
  switch (cls) {
    case ETLG_TC_BOOL: nd_lit(s, w0 ? "true" : "false"); return 0;
    case ETLG_TC_I16: case ETLG_TC_I32: nd_i64(s, (int32_t)w0); return 0;
    case ETLG_TC_U32: nd_u64(s, w0); return 0;
    case ETLG_TC_I64: nd_i64(s, (int64_t)(((uint64_t)ld32a(slot + 4) << 32) | w0)); return 0;
    case ETLG_TC_F32: return nd_float(s, w0, true);
    case ETLG_TC_F64: return nd_float(s, ((uint64_t)ld32a(slot + 4) << 32) | w0, false);
    case ETLG_TC_NUMERIC: return nd_numeric(s, heap + w0);
    case ETLG_TC_DATE: s.put('"'); pb_date(s, (int32_t)w0); s.put('"'); return 0;                                   // DATE_FORMAT
    case ETLG_TC_TIME: s.put('"'); time_str(s, w0, ld32a(slot + 4)); s.put('"'); return 0;                         // TIME_FORMAT
    case ETLG_TC_TIMESTAMP: case ETLG_TC_TIMESTAMPTZ:                                                                // TIMESTAMP_FORMAT / TIMESTAMPTZ_FORMAT_HH_MM
      s.put('"'); pb_date(s, (int32_t)w0); s.put(' '); time_str(s, ld32a(slot + 4), ld32a(slot + 8));
      if (cls == ETLG_TC_TIMESTAMPTZ) nd_lit(s, "+00:00");
      s.put('"'); return 0;
    case ETLG_TC_TIMETZ: s.put('"'); timetz_str(s, slot); s.put('"'); return 0;                                    // PgTimeTz Display
    case ETLG_TC_UUID: s.put('"'); put_uuid(s, slot); s.put('"'); return 0;
    case ETLG_TC_STRING: nd_str(s, heap + w0, ld32a(slot + 4)); return 0;
    case ETLG_TC_BYTEA: s.put('"'); s.hex(heap + w0, ld32a(slot + 4)); s.put('"'); return 0;                       // HexDisplay
    default: return RB_E_HOST_CELL;
  }
}
// NDJSON's arrays: `[e,e,null]`, strings by serde_json's escapes, a json element's Value embedded
struct NdArr {
  template <class S> static DEV void sep(S& s) { s.put(','); }
  template <class S> static DEV void null(S& s) { nd_lit(s, "null"); }
  template <class S> static DEV uint32_t value(S& s, uint32_t cls, const u8* slot, const u8* heap) { return nd_value(s, cls, slot, heap); }
  template <class S> static DEV void str(S& s, const u8* p, uint32_t n) { nd_str(s, p, n); }
  template <class S> static DEV void bytea(S& s, const u8* p, uint32_t n) { s.put('"'); s.hex(p, n); s.put('"'); }
  template <class S> static DEV uint32_t numeric(S& s, const u8* ent) { return nd_numeric(s, ent); }
  template <class S> static DEV void str_elem(S& s, const u8* txt, uint32_t p0, uint32_t p1) {
    s.put('"'); arr_unescape(txt, p0, p1, [&](u8 c) { nd_esc_put(s, c); }); s.put('"');
  }
  template <class S> static DEV void bytea_elem(S& s, const u8* txt, uint32_t p0, uint32_t p1) {   // lowercase
    s.put('"'); uint32_t q = 0; arr_unescape(txt, p0, p1, [&](u8 c) { if (q++ >= 2) s.put((u8)(c - 'A' < 6u ? c | 0x20 : c)); }); s.put('"');
  }
  template <class S> static DEV void json(S& s, const u8* t, uint32_t n) {
    if constexpr (std::is_same<S, RbCount>::value) { JsCount c; (void)json_display(c, t, n, false); s.zeros(c.n); }
    else (void)json_display(s, t, n, false);
  }
};

template <bool JS, class S, class M>
DEV uint32_t nd_row(const RbJob& j, uint64_t r, S& s, uint32_t c_lo, uint32_t c_hi, M&& mark) {   // 0, or column << 8 | code
  const uint64_t base = j.row_base[r], ev = j.row_event[r];
  const uint32_t kind = j.ev_kind[ev];
  // a Delete with a key image: the identity columns only, keyed by their names (identity_column_schemas, core.rs:412-426)
  const bool keyrow = kind == 'D' && (j.ev_flags[ev] & 3u) == ETLG_OLD_KEY;
  uint32_t err0 = 0;
  if (c_lo == 0) s.put('{');
  for (uint32_t i = c_lo; i < c_hi; i++) {
    mark(i);
    const uint32_t cd = j.cols[i], cls = cd & 0xFF;
    uint32_t off = cd >> 16, sti = i;
    if (keyrow) {
      const uint32_t kc = j.kcols[i];
      if (!(kc & 1u)) continue;
      off = kc >> 16; sti = (kc >> 8) & 0xFFu;
    }
    const uint32_t a = j.nd_key_off[i];
    s.bytes(j.nd_keys + a, j.nd_key_off[i + 1] - a);
    const uint32_t st = (j.fixed[base + sti / 4] >> (2 * (sti % 4))) & 3u;
    const u8* slot = j.fixed + base + off;
    uint32_t e = 0;
    if (st == ETLG_CELL_NULL) nd_lit(s, "null");
    else if (cls == ETLG_TC_ARRAY && st == ETLG_CELL_VALUE) e = typed_array<NdArr>(s, j.heap + ld32a(slot));
    else if (cls == ETLG_TC_ARRAY && st == ETLG_CELL_DEFERRED) e = text_array<NdArr, JS>(s, (cd >> 9) & 0x7Fu, j.heap + ld32a(slot), ld32a(slot + 4));
    else if (cls == ETLG_TC_JSON && st == ETLG_CELL_DEFERRED) e = JS ? rb_json(s, j.heap + ld32a(slot), ld32a(slot + 4), false, [](uint32_t) {}) : RB_E_HOST_CELL;   // Cell::Json: the Value itself
    else if (st != ETLG_CELL_VALUE) e = RB_E_HOST_CELL;
    else e = nd_value(s, cls, slot, j.heap);
    if (e == RB_E_JSON) return (i << 8) | e;   // the reference's decode error: before anything the sink would report
    if (e && !err0) err0 = (i << 8) | e;
    s.put(',');
  }
  if (err0) return err0;
  if (c_hi != j.n_cols) return 0;
  nd_lit(s, "\"_cdc_operation\":\"");
  nd_lit(s, kind == 'I' ? "insert" : kind == 'U' ? "update" : "delete");
  nd_lit(s, "\",\"_cdc_sequence_number\":\"");
  const uint64_t lsn = j.nd_zero_token ? 0ull : j.ev_commit[ev], ord = j.nd_zero_token ? 0ull : j.ev_ord[ev];
  pb_hex16(s, lsn); s.put('/'); pb_hex16(s, ord);
  nd_lit(s, "\"}\n");
  return 0;
}

// ---- DuckLake SQL literals (cell_to_sql_literal, crates/etl-destinations/src/ducklake/encoding.rs:366-612): the text every row the
// DuckLake sink writes goes through — `(lit, lit, ...)` per upserted row (table_row_to_sql_literal_ref, hashed into the batch identity
// and inserted as VALUES text) and `"col" = lit AND "col" IS NULL` per row image it deletes / matches by (delete_predicate_from_row,
// batches.rs:1229-1316). RbJob.dl_what says which: DL_ROW_TUPLES, DL_ROW_PRED_IDENT, DL_ROW_PRED_PK (a table-copy
// batch). Records carry no separator; the sink itself has no encoding error on this path.
//
// quote_literal is pg_escape 0.1.1, RESTATED FROM THE CRATE'S DOCUMENTATION (its source is not vendored with the reference and no
// reference test pins more than the plain arm): `'` is doubled; a text that holds a backslash has every backslash doubled and the
// literal is prefixed with " E" (a\b -> " E'a\\b'"); otherwise plain '...'. The quote doubling and the backslash arm are UNPINNED. The
// rule itself is the next three functions — which bytes are doubled, what opens the literal, how a byte is written — and dl_quote is
// the one function that applies it to a text (tests/ducklake_literals.py quote_literal is its twin); a json cell's Display and an array
// element's unescaped characters, which are not contiguous, go through the same three from DlQCount / DlQSink.
// The prefix must be known before the first byte, so both passes run over the text twice.
DEV bool dl_q_special(uint32_t c) { return c == '\'' || c == '\\'; }
template <class S> DEV void dl_q_open(S& s, bool backslash) { if (backslash) { s.put(' '); s.put('E'); } s.put('\''); }
template <class S> DEV void dl_q_put(S& s, uint32_t c) { const bool twice = dl_q_special(c); s.append(twice ? c | (c << 8) : c, twice ? 2u : 1u); }   // (one append: c, or c c)
struct DlQCount { uint32_t n = 0, extra = 0, bs = 0; DEV void put(u8 c) { n++; extra += dl_q_special(c) ? 1u : 0u; bs += c == '\\' ? 1u : 0u; } };
template <class S> struct DlQSink { S& s; DEV void put(u8 c) { dl_q_put(s, c); } };
// (an array element's unescaped characters s0[p0 .. p1): a call of its own, so that the lambda that writes an element replays it once)
DEV_NOINLINE DlQCount arr_q_count(const u8* s0, uint32_t p0, uint32_t p1) {
  DlQCount c;
  arr_unescape(s0, p0, p1, [&](u8 ch) { c.put(ch); });
  return c;
}
// a contiguous text: eight bytes at a time for a byte to double (as nd_str does), then the copy in 16-byte pieces that hold none
template <class S>
DEV void dl_quote(S& s, const u8* text, uint32_t n) {
  auto swar = [](uint64_t w) {   // bit 7 of some byte set <=> one of the eight bytes is '\'' or '\\' (has-zero: exact for "any")
    const uint64_t L = 0x0101010101010101ull, q = w ^ (0x27u * L), b = w ^ (0x5Cu * L);
    return (((q - L) & ~q) | ((b - L) & ~b)) & (0x80u * L);
  };
  DlQCount c;
  uint32_t k = 0;
  for (; k + 8u <= n; k += 8u) {
    uint64_t w; __builtin_memcpy(&w, text + k, 8);
    if (swar(w)) for (uint32_t b = 0; b < 8u; b++) c.put(text[k + b]);
  }
  for (; k < n; k++) c.put(text[k]);
  dl_q_open(s, c.bs != 0);
  if constexpr (std::is_same<S, RbCount>::value) s.zeros(n + c.extra);
  else if (!c.extra) s.bytes(text, n);
  else {
    for (k = 0; k + 16u <= n; k += 16u) {
      uint64_t v[2]; __builtin_memcpy(v, text + k, 16);
      if (!(swar(v[0]) | swar(v[1]))) { s.append(v[0], 8); s.append(v[1], 8); }
      else for (uint32_t b = 0; b < 16u; b++) dl_q_put(s, text[k + b]);
    }
    for (; k < n; k++) dl_q_put(s, text[k]);
  }
  s.put('\'');
}
// CAST(<quote_literal(j.to_string())> AS JSON) (:415). The text is checked in the counting pass only, as rb_json does.
template <class S> DEV uint32_t dl_json(S& s, const u8* t, uint32_t tn, bool check) {
  if (check && std::is_same<S, RbCount>::value && !json_valid(t, tn)) return RB_E_JSON;
  DlQCount c;
  if (json_display(c, t, tn, false)) return RB_E_HOST_CELL;
  nd_lit(s, "CAST(");
  dl_q_open(s, c.bs != 0);
  if constexpr (std::is_same<S, RbCount>::value) s.zeros(c.n + c.extra);
  else { DlQSink<S> k{s}; (void)json_display(k, t, tn, false); }
  s.put('\'');
  nd_lit(s, " AS JSON)");
  return 0;
}
// from_hex('<UPPER-case hex>'): encode_hex, {byte:02X} (:615-617)
template <class S> DEV void dl_bytea(S& s, const u8* p, uint32_t n) { nd_lit(s, "from_hex('"); s.hex(p, n, 'A'); nd_lit(s, "')"); }
// float_literal (:588-612): the three CASTs, else `value.to_string()` of the f64 (a float4 widened first) — float_display.h
template <class S> DEV void dl_float(S& s, uint64_t bits, bool is32) {
  const uint64_t b = is32 ? f32_widen_bits((uint32_t)bits) : bits;
  if (((b >> 52) & 0x7FFu) == 0x7FFu) {
    nd_lit(s, (b & ((1ull << 52) - 1u)) ? "CAST('NaN' AS " : (b >> 63) ? "CAST('-Infinity' AS " : "CAST('Infinity' AS ");
    nd_lit(s, is32 ? "FLOAT)" : "DOUBLE)");
    return;
  }
  (void)float_display(s, b);
}
// %H:%M:%S%.6f — always six fraction digits (a leap second is nanos >= 10^9 on second 59, printed as :60)
template <class S> DEV void dl_time(S& s, uint32_t secs, uint32_t nanos) {
  const uint32_t leap = nanos >= 1000000000u ? 1u : 0u;
  nanos -= leap * 1000000000u;
  put_2d(s, secs / 3600); s.put(':'); put_2d(s, secs / 60 % 60); s.put(':'); put_2d(s, secs % 60 + leap);
  s.put('.');
  const uint32_t us = nanos / 1000u;
  for (uint32_t div = 100000u; div; div /= 10) s.put((u8)('0' + us / div % 10));
}
// numeric / timetz Display through quote_literal: their texts hold neither a quote nor a backslash, so the plain arm
template <class S> DEV void dl_numeric(S& s, const u8* ent) { s.put('\''); numeric_str(s, ent); s.put('\''); }
// One non-null value of class `cls` (nd_value's arguments)
template <class S>
DEV uint32_t dl_value(S& s, uint32_t cls, const u8* slot, const u8* heap) {
  const uint32_t w0 = ld32a(slot);
  switch (cls) {
    case ETLG_TC_BOOL: nd_lit(s, w0 ? "TRUE" : "FALSE"); return 0;
    case ETLG_TC_I16: case ETLG_TC_I32: nd_i64(s, (int32_t)w0); return 0;
    case ETLG_TC_U32: nd_u64(s, w0); return 0;
    case ETLG_TC_I64: nd_i64(s, (int64_t)(((uint64_t)ld32a(slot + 4) << 32) | w0)); return 0;
    case ETLG_TC_F32: dl_float(s, w0, true); return 0;
    case ETLG_TC_F64: dl_float(s, ((uint64_t)ld32a(slot + 4) << 32) | w0, false); return 0;
    case ETLG_TC_NUMERIC: dl_numeric(s, heap + w0); return 0;
    case ETLG_TC_DATE: nd_lit(s, "DATE '"); pb_date(s, (int32_t)w0); s.put('\''); return 0;
    case ETLG_TC_TIME: nd_lit(s, "TIME '"); dl_time(s, w0, ld32a(slot + 4)); s.put('\''); return 0;
    case ETLG_TC_TIMESTAMP: case ETLG_TC_TIMESTAMPTZ:
      nd_lit(s, cls == ETLG_TC_TIMESTAMPTZ ? "TIMESTAMPTZ '" : "TIMESTAMP '");
      pb_date(s, (int32_t)w0); s.put(' '); dl_time(s, ld32a(slot + 4), ld32a(slot + 8));
      if (cls == ETLG_TC_TIMESTAMPTZ) nd_lit(s, "+00:00");   // %:z of a DateTime<Utc>
      s.put('\''); return 0;
    case ETLG_TC_TIMETZ: s.put('\''); timetz_str(s, slot); s.put('\''); return 0;
    case ETLG_TC_UUID: nd_lit(s, "CAST('"); put_uuid(s, slot); nd_lit(s, "' AS UUID)"); return 0;
    case ETLG_TC_STRING: dl_quote(s, heap + w0, ld32a(slot + 4)); return 0;
    case ETLG_TC_BYTEA: dl_bytea(s, heap + w0, ld32a(slot + 4)); return 0;
    default: return RB_E_HOST_CELL;
  }
}
// DuckLake's arrays: `[e, e, NULL]`, strings through quote_literal, a json element as its CAST
struct DlArr {
  template <class S> static DEV void sep(S& s) { s.put(','); s.put(' '); }
  template <class S> static DEV void null(S& s) { nd_lit(s, "NULL"); }
  template <class S> static DEV uint32_t value(S& s, uint32_t cls, const u8* slot, const u8* heap) { return dl_value(s, cls, slot, heap); }
  template <class S> static DEV void str(S& s, const u8* p, uint32_t n) { dl_quote(s, p, n); }
  template <class S> static DEV void bytea(S& s, const u8* p, uint32_t n) { dl_bytea(s, p, n); }
  template <class S> static DEV uint32_t numeric(S& s, const u8* ent) { dl_numeric(s, ent); return 0; }
  template <class S> static DEV void str_elem(S& s, const u8* txt, uint32_t p0, uint32_t p1) {
    const DlQCount c = arr_q_count(txt, p0, p1);
    dl_q_open(s, c.bs != 0);
    if constexpr (std::is_same<S, RbCount>::value) s.zeros(c.n + c.extra);
    else arr_unescape(txt, p0, p1, [&](u8 ch) { dl_q_put(s, ch); });
    s.put('\'');
  }
  template <class S> static DEV void bytea_elem(S& s, const u8* txt, uint32_t p0, uint32_t p1) {   // the hex digits of the element's "\x.." text, in upper case
    nd_lit(s, "from_hex('");
    uint32_t q = 0;
    arr_unescape(txt, p0, p1, [&](u8 c) { if (q++ >= 2) s.put((u8)(c - 'a' < 6u ? c & ~0x20u : c)); });
    nd_lit(s, "')");
  }
  template <class S> static DEV void json(S& s, const u8* t, uint32_t n) { (void)dl_json(s, t, n, false); }
};

// UPD: ETLG_DL_UPDATES (DL_ROW_UPDATES, an instantiation of its own so that the tuples and the predicates compile as they did without it): the
// SET clause of a partial new row (update_assignments_from_partial_row joined by ", ": every cell that is not MISSING), and behind it — the
// row marked kPbSecond — the predicate of the same event
template <bool JS, bool UPD = false, class S, class M>
DEV uint32_t dl_row(const RbJob& j, uint64_t r, S& s, uint32_t c_lo, uint32_t c_hi, M&& mark) {   // 0, or column << 8 | code
  const uint64_t rb = j.row_base[r], base = rb & kPbBase;
  const bool set = UPD && !(rb & kPbSecond);
  const bool pred = j.dl_what != DL_ROW_TUPLES && !set, keyrow = (rb & kPbKey) != 0;   // keyrow: the image has the key layout (the identity cells only)
  const uint32_t kbit = j.dl_what == DL_ROW_PRED_PK ? 4u : 1u;                 // which columns a predicate takes: identity / primary key
  bool first = true;                                                // no predicate / present column in front of this lane's columns?
  if (pred) for (uint32_t i = 0; i < c_lo; i++) if (j.kcols[i] & kbit) first = false;
  if constexpr (UPD) { if (set) for (uint32_t i = 0; i < c_lo; i++) if (((j.fixed[base + i / 4] >> (2 * (i % 4))) & 3u) != ETLG_CELL_MISSING) first = false; }
  uint32_t err0 = 0;
  if (!pred && !set && c_lo == 0) s.put('(');
  for (uint32_t i = c_lo; i < c_hi; i++) {
    mark(i);
    const uint32_t cd = j.cols[i], cls = cd & 0xFF;
    uint32_t off = cd >> 16, sti = i;
    if (pred) {
      const uint32_t kc = j.kcols[i];
      if (!(kc & kbit)) continue;
      if (keyrow) { off = kc >> 16; sti = (kc >> 8) & 0xFFu; }
      if (!first) nd_lit(s, " AND ");
      first = false;
      const uint32_t a = j.nd_key_off[i];
      s.bytes(j.nd_keys + a, j.nd_key_off[i + 1] - a);   // the quoted identifier
    } else if (!set && i) { s.put(','); s.put(' '); }
    const uint32_t st = (j.fixed[base + sti / 4] >> (2 * (sti % 4))) & 3u;
    if constexpr (UPD) {
      if (set) {
        if (st == ETLG_CELL_MISSING) continue;
        if (!first) { s.put(','); s.put(' '); }
        first = false;
        const uint32_t a = j.nd_key_off[i];
        s.bytes(j.nd_keys + a, j.nd_key_off[i + 1] - a);
        nd_lit(s, " = ");   // (a NULL cell: `"c" = NULL`, cell_to_sql_literal_ref(Cell::Null))
      }
    }
    const u8* slot = j.fixed + base + off;
    uint32_t e = 0;
    if (st == ETLG_CELL_NULL) nd_lit(s, pred ? " IS NULL" : "NULL");
    else {
      if (pred) nd_lit(s, " = ");
      if (cls == ETLG_TC_ARRAY && st == ETLG_CELL_VALUE) e = typed_array<DlArr>(s, j.heap + ld32a(slot));
      else if (cls == ETLG_TC_ARRAY && st == ETLG_CELL_DEFERRED) e = text_array<DlArr, JS>(s, (cd >> 9) & 0x7Fu, j.heap + ld32a(slot), ld32a(slot + 4));
      else if (cls == ETLG_TC_JSON && st == ETLG_CELL_DEFERRED) e = JS ? dl_json(s, j.heap + ld32a(slot), ld32a(slot + 4), true) : RB_E_HOST_CELL;
      else if (st != ETLG_CELL_VALUE) e = RB_E_HOST_CELL;
      else e = dl_value(s, cls, slot, j.heap);
    }
    if (e == RB_E_JSON) return (i << 8) | e;   // the reference's decode error: before anything else
    if (e && !err0) err0 = (i << 8) | e;
  }
  if (err0) return err0;
  if (!pred && !set && c_hi == j.n_cols) s.put(')');
  return 0;
}

// ---- the row format of a kernel instantiation: row(j, r, sink, c_lo, c_hi, mark) writes the columns [c_lo, c_hi) of row r into the sink
// (the counting pass: an RbCount) and returns 0 or column << 8 | code. JS: the table has a json column (kernels of their own, as for the
// Arrow columns). A format per sink, so that no kernel carries another sink's arm; RowBinary and protobuf share theirs (j.format).
template <bool JS> struct RbPbFormat {
  template <class S, class M> static DEV uint32_t row(const RbJob& j, uint64_t r, S& s, uint32_t c_lo, uint32_t c_hi, M&& mark) {
    return j.format != FMT_ROWBINARY ? pb_row<JS>(j, r, s, c_lo, c_hi, mark) : rb_row<JS>(j, r, s, c_lo, c_hi, mark);
  }
};
template <bool JS> struct NdFormat {      // Snowflake NDJSON
  template <class S, class M> static DEV uint32_t row(const RbJob& j, uint64_t r, S& s, uint32_t c_lo, uint32_t c_hi, M&& mark) { return nd_row<JS>(j, r, s, c_lo, c_hi, mark); }
};
template <bool JS> struct DlFormat {      // DuckLake tuples and predicates
  template <class S, class M> static DEV uint32_t row(const RbJob& j, uint64_t r, S& s, uint32_t c_lo, uint32_t c_hi, M&& mark) { return dl_row<JS>(j, r, s, c_lo, c_hi, mark); }
};
template <bool JS> struct DlUpdFormat {   // DuckLake partial Updates (ETLG_DL_UPDATES): dl_row with the assignments arm; the counting pass notes where every column ends (col_ends)
  template <class S, class M> static DEV uint32_t row(const RbJob& j, uint64_t r, S& s, uint32_t c_lo, uint32_t c_hi, M&& mark) {
    if constexpr (std::is_same<S, RbCount>::value) {
      const uint32_t e = dl_row<JS, true>(j, r, s, c_lo, c_hi, [&](uint32_t i) { mark(i); if (i) j.col_ends[r * j.n_cols + i - 1] = s.n; });   // (column i - 1 is done)
      if (j.n_cols) j.col_ends[(r + 1) * j.n_cols - 1] = s.n;
      return e;
    } else return dl_row<JS, true>(j, r, s, c_lo, c_hi, mark);
  }
};

template <class F>
__global__ __launch_bounds__(256) void k_rb_lens(RbJob j, unsigned long long* blk) {
  __shared__ uint64_t lds_sum[4];
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  RbCount c;
  if (r < j.n_rows) {
    // (where pieces 1 .. qparts-1 of the row begin, for the byte pass: piece q starts at column q * n_cols / qparts)
    uint32_t next = 1;
    auto mark = [&](uint32_t i) {
      while (next < j.qparts && i == rb_part_col(j, next)) { j.part_off[(uint64_t)(next - 1) * j.n_rows + r] = c.n; next++; }
    };
    const uint32_t e = F::row(j, r, c, 0, j.n_cols, mark);
    // first failing row in event order, rows with a date out of range before all others (bit 62 clear)
    // (and a json cell that is not JSON before those: the reference's decode fails before any sink sees a row)
    if (e) {
      const unsigned long long rank = (e & 0xFFu) == RB_E_JSON ? kRbRankDecode : ((e & 0xFFu) == RB_E_DATE_RANGE || j.format != FMT_ROWBINARY) ? kRbRankEarly : kRbRankLate;
      atomicMin(j.err, rb_report_pack(rank, r, e)); c.n = 0;
    }
    j.lens[r] = c.n;
  }
  const uint64_t t = block_sum64(c.n, lds_sum);   // (the block's sum for the offsets scan)
  if (threadIdx.x == 0) blk[blockIdx.x] = t;
}

// The byte pass. One lane per row is few waves for what each has to do — a 64 MiB cfg3 batch is 175 000 rows of 270 bytes: 2.7 waves per
// SIMD, each a serial chain of loads and stores (132 us; profiles/r05v_rb_rows_ablation.txt) — so a row is split among `parts` lanes
// (1-4, the host picks it from the row count), each writing the columns [part * n / parts, (part + 1) * n / parts) from the byte offset
// the counting pass noted. A wave holds 64 (128, 256) consecutive rows of ONE part — the lanes walk the same columns — and the parts of
// a row sit in ONE workgroup: with a part per workgroup (blockIdx.y) every cache line of the output was written from several XCDs, and
// the kernel got slower, not faster (186 us against 134; profiles/r05y_rb_rows_parts.txt).
__host__ DEV uint32_t rb_rows_per_block(uint32_t parts) { return parts == 1 ? 256u : parts == 2 ? 128u : 64u; }
// ... and the lanes do not store to global memory themselves: 64 lanes x 8 bytes at a stride of a row is 64 write requests per
// instruction (the request rate, not the bytes, bounded the kernel). The workgroup's rows are one contiguous piece of the output: when it
// fits kRbLds, the lanes build it in LDS and the whole workgroup stores it in 16-byte pieces; a piece that does not fit (rows of more
// than ~500 bytes on average) is written directly as before.
constexpr uint32_t kRbLds = 32 * 1024;
template <class F>
__global__ __launch_bounds__(256) void k_rb_rows(RbJob j) {
  __shared__ uint4 img[kRbLds / 16 + 2];
  const uint32_t rpb = rb_rows_per_block(j.parts), part = threadIdx.x / rpb;
  const uint64_t r0 = (uint64_t)blockIdx.x * rpb, r = r0 + threadIdx.x % rpb;
  const uint64_t r1 = r0 + rpb < j.n_rows ? r0 + rpb : j.n_rows;
  const uint64_t g0 = (uint64_t)j.offsets[r0], g1 = (uint64_t)j.offsets[r1];
  const uint32_t pad = (uint32_t)((uintptr_t)(j.out + g0) & 15u);   // the image starts at the 16-byte line the piece starts in
  const bool staged = g1 - g0 + pad <= kRbLds;                      // (uniform in the workgroup)
  const bool active = part < j.parts && r < j.n_rows && j.lens[r];
  const uint32_t q = part * (j.qparts / j.parts);   // the lane's first piece
  const uint32_t c_lo = rb_part_col(j, q), c_hi = part + 1 >= j.parts ? j.n_cols : rb_part_col(j, q + j.qparts / j.parts);
  const uint32_t po = active && q ? j.part_off[(uint64_t)(q - 1) * j.n_rows + r] : 0u;
  auto none = [](uint32_t) {};
  if (!staged) {
    if (active) {
      RbWrite w(j.out + j.offsets[r] + po);
      (void)F::row(j, r, w, c_lo, c_hi, none);
      w.finish();
    }
    return;
  }
  const uint32_t total = pad + (uint32_t)(g1 - g0), nch = (total + 15u) / 16u;
  for (uint32_t k = threadIdx.x; k < nch; k += 256) img[k] = make_uint4(0, 0, 0, 0);
  __syncthreads();
  if (active) {
    const uint32_t o = pad + (uint32_t)((uint64_t)j.offsets[r] - g0) + po;
    RbLdsWrite w((uint32_t*)img + (o >> 2), o & 3u);
    (void)F::row(j, r, w, c_lo, c_hi, none);
    w.finish();
  }
  __syncthreads();
  u8* gb = j.out + g0 - pad;
  for (uint32_t k = threadIdx.x; k < nch; k += 256) {
    const uint32_t b0 = k * 16u;
    if (b0 >= pad && b0 + 16u <= total) *(uint4*)(gb + b0) = img[k];
    else for (uint32_t b = b0 < pad ? pad : b0; b < b0 + 16u && b < total; b++) gb[b] = ((const u8*)img)[b];   // the first / last line: the bytes outside belong to the neighbours
  }
}

// One launch sequence for every format. step 0: lengths + offsets (blk: (nblocks + 1) x u64 scratch); step 1: the bytes
template <class F>
void rb_launch(const RbJob& j, unsigned long long* blk, int64_t* offsets, unsigned long long* tot, int step, hipStream_t st) {
  if (step == 0) {
    hipLaunchKernelGGL(k_rb_lens<F>, dim3((uint32_t)((j.n_rows + 255) / 256)), dim3(256), 0, st, j, blk);
    etlg_k_scan_blocks(j.lens, j.n_rows, blk, offsets, tot, st);
  } else {
    const uint32_t rpb = rb_rows_per_block(j.parts);
    hipLaunchKernelGGL(k_rb_rows<F>, dim3((uint32_t)((j.n_rows + rpb - 1) / rpb)), dim3(256), 0, st, j);
  }
}
template <template <bool> class F>   // kernels of their own for a table with a json column
void rb_launch_js(const RbJob& j, unsigned long long* blk, int64_t* offsets, unsigned long long* tot, int step, hipStream_t st) {
  if (j.has_json) rb_launch<F<true>>(j, blk, offsets, tot, step, st); else rb_launch<F<false>>(j, blk, offsets, tot, step, st);
}

}  // namespace etlg
