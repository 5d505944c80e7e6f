// What the hand-off builders decide before they touch the device: the Arrow kind of every column, where the parts of blocks A, B and C lie, the
// column words of the row formats, the lanes per row of the byte pass. Plain C++, no HIP and no etlg_ctx: tests/native/handoff_plan_check.cpp includes
// this header alone (it supplies etlg_array_elem_class itself). host_handoff_columns.inc and host_handoff_rows.inc are the callers.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/etlg.h"
#include "dev_types.h"
#include "scratch_layout.h"

struct SlotHost {  // one ReplicatedTableSchema instance
  etlg_slot_desc desc;
  std::vector<etlg_slot_col> cols;
  std::vector<uint8_t> pk;   // per replicated column: a primary-key column of the stored schema (ColumnSchema::primary_key)
  int identity_type = 0;   // ReplicatedTableSchema::infer_identity_type (schema.rs:686-721): 0 Missing, 1 PrimaryKey, 2 Full, 3 AlternativeKey
};

// ---- columns (etlg_batch_columns, etlg_batch_iceberg, etlg_batch_ducklake_copy)
struct ColPlan { uint32_t kind, vbytes; bool var; uint32_t child = 0, child_bytes = 0, elem = 0, fmt = 0; };   // fmt: the kernels' internal kind of a formatted string column (columns.hip AK_*_STR)
inline ColPlan list_plan(uint32_t elem) {  // array literals the device parses: element classes with a fixed-width value
  switch (elem) {
    case ETLG_TC_BOOL: return {ETLG_AK_LIST, 0, true, ETLG_AK_BOOLEAN, 0, elem};
    case ETLG_TC_I16: case ETLG_TC_I32: return {ETLG_AK_LIST, 0, true, ETLG_AK_INT32, 4, elem};
    case ETLG_TC_I64: case ETLG_TC_U32: return {ETLG_AK_LIST, 0, true, ETLG_AK_INT64, 8, elem};
    case ETLG_TC_F32: return {ETLG_AK_LIST, 0, true, ETLG_AK_FLOAT32, 4, elem};
    case ETLG_TC_F64: return {ETLG_AK_LIST, 0, true, ETLG_AK_FLOAT64, 8, elem};
    case ETLG_TC_DATE: return {ETLG_AK_LIST, 0, true, ETLG_AK_DATE32, 4, elem};
    case ETLG_TC_TIME: return {ETLG_AK_LIST, 0, true, ETLG_AK_TIME64_US, 8, elem};
    case ETLG_TC_TIMESTAMP: return {ETLG_AK_LIST, 0, true, ETLG_AK_TIMESTAMP_US, 8, elem};
    case ETLG_TC_TIMESTAMPTZ: return {ETLG_AK_LIST, 0, true, ETLG_AK_TIMESTAMP_US_UTC, 8, elem};
    case ETLG_TC_UUID: return {ETLG_AK_LIST, 0, true, ETLG_AK_FIXED16, 16, elem};
    case ETLG_TC_STRING: return {ETLG_AK_LIST, 0, true, ETLG_AK_LARGE_UTF8, 0, elem};   // text[], varchar[], and every array type without a dedicated arm
    // ArrayCell::Numeric / TimeTz: lists of Display strings (iceberg/encoding.rs:902-945); ArrayCell::Bytes: lists of the decoded bytes
    case ETLG_TC_NUMERIC: case ETLG_TC_TIMETZ: return {ETLG_AK_LIST, 0, true, ETLG_AK_LARGE_UTF8, 0, elem};
    case ETLG_TC_BYTEA: return {ETLG_AK_LIST, 0, true, ETLG_AK_LARGE_BINARY, 0, elem};
    case ETLG_TC_JSON: return {ETLG_AK_LIST, 0, true, ETLG_AK_LARGE_UTF8, 0, elem};   // ArrayCell::Json: a list of `j.to_string()` strings (round 6: arr_json_check / k_arr_fill)
    default: return {ETLG_AK_TEXT_FORM, 0, true};
  }
}
inline bool var_child(const ColPlan& p) { return p.child == ETLG_AK_LARGE_UTF8 || p.child == ETLG_AK_LARGE_BINARY; }   // list children with offsets of their own
inline bool text_list(const ColPlan& p) { return p.kind == ETLG_AK_LIST && var_child(p); }   // element offsets in block B, element bytes in block C
inline ColPlan col_plan(uint32_t cls) {
  switch (cls) {
    case ETLG_TC_BOOL: return {ETLG_AK_BOOLEAN, 0, false};
    case ETLG_TC_I16: case ETLG_TC_I32: return {ETLG_AK_INT32, 4, false};
    case ETLG_TC_I64: case ETLG_TC_U32: return {ETLG_AK_INT64, 8, false};
    case ETLG_TC_F32: return {ETLG_AK_FLOAT32, 4, false};
    case ETLG_TC_F64: return {ETLG_AK_FLOAT64, 8, false};
    case ETLG_TC_DATE: return {ETLG_AK_DATE32, 4, false};
    case ETLG_TC_TIME: return {ETLG_AK_TIME64_US, 8, false};
    case ETLG_TC_TIMESTAMP: return {ETLG_AK_TIMESTAMP_US, 8, false};
    case ETLG_TC_TIMESTAMPTZ: return {ETLG_AK_TIMESTAMP_US_UTC, 8, false};
    case ETLG_TC_UUID: return {ETLG_AK_FIXED16, 16, false};
    case ETLG_TC_STRING: return {ETLG_AK_LARGE_UTF8, 0, true};
    case ETLG_TC_BYTEA: return {ETLG_AK_LARGE_BINARY, 0, true};
    // Display strings in every sink (cell_to_string, iceberg/encoding.rs:349-352; n.to_string() / t.to_string()): formatted on the device
    case ETLG_TC_NUMERIC: return {ETLG_AK_LARGE_UTF8, 0, true, 0, 0, 0, etlg::kAkNumericStr};
    case ETLG_TC_TIMETZ: return {ETLG_AK_LARGE_UTF8, 0, true, 0, 0, 0, etlg::kAkTimetzStr};
    default: return {ETLG_AK_TEXT_FORM, 0, true};
  }
}
// DuckLake's Arrow copy staging: arrow_column_kind (ducklake/encoding.rs:236-257) by type class — Int16 for int2, UInt64 for oid, Utf8 /
// Binary (32-bit offsets) for text / bytea, Utf8 of the Display string for numeric / timetz (push_cell :170-171); the rest as
// etlg_batch_columns has it. `fmt`: the kernels' kind where the public one is not theirs. ETLG_AK_NONE: arrow_column_kinds gives None
// for the table (uuid, json, arrays).
inline ColPlan dlc_plan(uint32_t cls) {
  switch (cls) {
    case ETLG_TC_I16: return {ETLG_AK_INT16, 2, false};
    case ETLG_TC_U32: return {ETLG_AK_UINT64, 8, false, 0, 0, 0, ETLG_AK_INT64};   // (the widening of cell_to_i64: col_fixed_body's I64 arm by class)
    case ETLG_TC_STRING: return {ETLG_AK_UTF8, 0, true, 0, 0, 0, ETLG_AK_LARGE_UTF8};
    case ETLG_TC_BYTEA: return {ETLG_AK_BINARY, 0, true, 0, 0, 0, ETLG_AK_LARGE_BINARY};
    case ETLG_TC_NUMERIC: return {ETLG_AK_UTF8, 0, true, 0, 0, 0, etlg::kAkNumericStr};
    case ETLG_TC_TIMETZ: return {ETLG_AK_UTF8, 0, true, 0, 0, 0, etlg::kAkTimetzStr};
    case ETLG_TC_UUID: case ETLG_TC_JSON: case ETLG_TC_ARRAY: return {ETLG_AK_NONE, 0, false};
    default: { const ColPlan p = col_plan(cls); return p.kind == ETLG_AK_TEXT_FORM ? ColPlan{ETLG_AK_NONE, 0, false} : p; }
  }
}

enum class ColCaller { Columns, Iceberg, DuckLakeCopy };   // which entry point build_columns serves
// The kind of every column of the slot for the caller. *not_arrow: the first column the DuckLake copy has no Arrow form for (the call builds
// nothing then), ~0u when there is none
inline std::vector<ColPlan> column_plans(const SlotHost& sh, ColCaller who, uint32_t row_kinds, uint32_t* not_arrow) {
  const bool dlc = who == ColCaller::DuckLakeCopy;
  std::vector<ColPlan> pl(sh.desc.n_cols);
  *not_arrow = ~0u;
  for (uint32_t i = 0; i < sh.desc.n_cols; i++) {
    const uint32_t cls = (uint32_t)sh.cols[i].type_class;
    if (dlc && *not_arrow == ~0u && dlc_plan(cls).kind == ETLG_AK_NONE) *not_arrow = i;
    pl[i] = dlc ? dlc_plan(cls) : col_plan(cls);
    if ((row_kinds & ETLG_ROWS_PARSE_ARRAYS) && cls == ETLG_TC_ARRAY) pl[i] = list_plan((uint32_t)etlg_array_elem_class(sh.cols[i].type_oid));
    if ((row_kinds & ETLG_ROWS_FORMAT_JSON) && cls == ETLG_TC_JSON) pl[i] = {ETLG_AK_LARGE_UTF8, 0, true, 0, 0, 0, etlg::kAkJsonStr};   // `j.to_string()` written on the device (AK_JSON_STR)
  }
  return pl;
}

// Block A: row_event | per column {validity, deferred, values or (offsets, lens)} | changelog: the two CDC columns {validity, deferred, offsets,
// values} (fixed-width strings: sized here) | counters | var-len totals | a scan scratch per column. The view's host copy is the prefix [0, cnt).
constexpr uint32_t kCdcWidth[2] = {6u, 33u};
struct ColPartsA { size_t validity = 0, deferred = 0, values = 0, lens = 0, offsets = 0; };
struct ColumnsLayoutA {
  std::vector<ColPartsA> col; ColPartsA cdc[2];
  size_t cnt = 0;        // per column: nulls, deferred, child nulls, first list error
  size_t tot = 0;        // per var-len column: the bytes behind its offsets (one read-back for both)
  size_t scan = 0, scan_one = 0;   // the var-len columns' first passes run as ONE launch each (etlg_k_col_var_pack): a scan scratch per column
  size_t total = 0;
};
inline ColumnsLayoutA columns_layout_a(const std::vector<ColPlan>& pl, uint64_t n, bool changelog, bool dlc) {
  const size_t nc = pl.size(), bm = ((size_t)n + 63) / 64 * 8;   // bm: bytes of a bitmap
  ColumnsLayoutA o; o.col.resize(nc);
  ScratchLayout l(n * 8);   // row_event first
  for (size_t i = 0; i < nc; i++) {
    if (pl[i].kind == ETLG_AK_NONE) continue;
    ColPartsA& p = o.col[i];
    p.validity = l.take(bm); p.deferred = l.take(bm);
    if (pl[i].var) { p.offsets = l.take((n + 1) * (dlc ? 4 : 8)); p.lens = l.take(n * 4); }
    else p.values = l.take(pl[i].kind == ETLG_AK_BOOLEAN ? bm : n * pl[i].vbytes);
  }
  if (changelog) for (int k = 0; k < 2; k++) {
    o.cdc[k].validity = l.take(bm); o.cdc[k].deferred = l.take(bm);
    o.cdc[k].offsets = l.take((n + 1) * 8); o.cdc[k].values = l.take(n * kCdcWidth[k]);
  }
  o.cnt = l.take(nc * 32); o.tot = l.take(nc * 8);
  o.scan_one = al64((size_t)((uint32_t)((n + 255) / 256) + 1) * 8);
  o.scan = l.skip(o.scan_one * std::max<size_t>(nc, 1));
  o.total = l.total();
  return o;
}

// Block B: the bytes of the var-len columns; list columns: child values (or, for lists of strings, child offsets + lengths + scan scratch)
// and child validity. var_total: per var-len column the bytes (list: the elements) behind its offsets
struct ColPartsB { size_t values = 0, child_validity = 0, child_lens = 0, child_scan = 0, values_bytes = 0; };
struct ColumnsLayoutB { std::vector<ColPartsB> col; size_t total = 0; bool any_text_list = false; };
inline ColumnsLayoutB columns_layout_b(const std::vector<ColPlan>& pl, const std::vector<int64_t>& var_total) {
  ColumnsLayoutB o; o.col.resize(pl.size());
  ScratchLayout l;
  for (size_t i = 0; i < pl.size(); i++) {
    if (!pl[i].var) continue;
    ColPartsB& p = o.col[i];
    const size_t tot = (size_t)var_total[i], bits = (tot + 63) / 64 * 8;
    if (text_list(pl[i])) {   // child offsets first (i64), then lengths, scan scratch, validity
      o.any_text_list = true;
      p.values = l.take((tot + 1) * 8); p.child_lens = l.take(tot * 4); p.child_scan = l.take((tot / 256 + 2) * 8); p.child_validity = l.take(bits);
    } else if (pl[i].kind == ETLG_AK_LIST) {
      p.values_bytes = pl[i].child == ETLG_AK_BOOLEAN ? bits : tot * pl[i].child_bytes;
      p.values = l.take(p.values_bytes); p.child_validity = l.take(bits);
    } else { p.values_bytes = tot; p.values = l.take(tot); }
  }
  o.total = l.total();
  return o;
}

// Block C: the element bytes of lists of strings, 64 bytes apart. text_total: per such column the bytes of all its elements
struct ColumnsLayoutC { std::vector<size_t> values; size_t total = 0; };
inline ColumnsLayoutC columns_layout_c(const std::vector<ColPlan>& pl, const std::vector<int64_t>& text_total) {
  ColumnsLayoutC o; o.values.assign(pl.size(), 0);
  ScratchLayout l;
  for (size_t i = 0; i < pl.size(); i++) if (text_list(pl[i])) { o.values[i] = l.take((size_t)text_total[i]); l.skip(64); }
  o.total = l.total();
  return o;
}

// ---- rows (etlg_batch_rowbinary, _protobuf, _ndjson, _duckdb)
struct NdKeys { std::vector<uint32_t> off; std::string bytes; };   // FMT_NDJSON / FMT_DUCKLAKE: the escaped `"name":` / quoted name of every column, back to back
// What an entry point asks of handoff_rows. format (FMT_*): ClickHouse RowBinary (Insert / Update / Delete rows + the engine's CDC columns), BigQuery
// protobuf, Snowflake NDJSON, DuckLake SQL literals (dl_what: ETLG_DL_TUPLES / ETLG_DL_PREDICATES / ETLG_DL_UPDATES)
struct RowsCall { uint32_t format; const uint8_t* nullable_flags; uint32_t n_flags; int32_t engine; const NdKeys* nd; uint32_t dl_what; };
// ColSel.dl of an etlg_batch_duckdb call, and through dl_row_what RbJob.dl_what (a copied row's predicate is over the primary key: delete_predicate_from_copy_row)
inline uint32_t dl_selection(uint32_t what, bool copy) {
  return what == ETLG_DL_UPDATES ? etlg::DL_SEL_UPDATES : what == ETLG_DL_TUPLES ? etlg::DL_SEL_TUPLES : copy ? etlg::DL_SEL_PRED_PK : etlg::DL_SEL_PRED_IDENT;
}
struct RowWords {
  std::vector<uint32_t> cols;   // [0, nc): RbJob.cols; [nc, 2 nc): the key-layout words of the columns (RbJob.kcols)
  uint32_t dl = etlg::DL_SEL_NONE;
  bool key_ok = false, pk_comparable = true, has_json = false;
  uint32_t host_column = ~0u;   // the first column whose class only the host encodes (the words behind it are not filled in), ~0u: none
};
inline RowWords row_words(const SlotHost& sh, const RowsCall& call, bool copy) {
  const uint32_t nc = sh.desc.n_cols;
  RowWords w; w.cols.resize(2 * (size_t)nc);
  w.dl = call.format == etlg::FMT_DUCKLAKE ? dl_selection(call.dl_what, copy) : (uint32_t)etlg::DL_SEL_NONE;
  // A Delete that carries only the key: the reference expands it into a tombstone row (expand_key_row, clickhouse/core.rs:1437-1472)
  // when the replica identity is the primary key (or Full) — ensure_clickhouse_key_identity_is_primary_key, :1404-1427; identity
  // columns are then exactly the primary-key columns, so the key image has the right width (:1438-1450). The device builds that row
  // unless a nullable non-key column has a type outside the value codec's table (a String cell): is_array_type (type_utils.rs:14-18)
  // decides between NULL and an empty array there, and only the host knows every array type — those slots' key-only Deletes stay
  // with the host, like every slot's under another identity (the host raises the reference's SourceReplicaIdentityError).
  w.key_ok = call.format == etlg::FMT_ROWBINARY && (sh.identity_type == 1 || sh.identity_type == 2) && sh.desc.n_ident != 0;
  for (uint32_t i = 0; i < nc; i++) {
    const etlg_slot_col& sc = sh.cols[i];
    const uint32_t oid = sc.type_oid, cls = (uint32_t)sc.type_class;
    if (!sc.identity && sc.nullable && cls == ETLG_TC_STRING && !(oid == 25 || oid == 1043 || oid == 1042 || oid == 19 || oid == 18)) w.key_ok = false;
    w.cols[nc + i] = (sc.identity ? 1u : 0u) | (sc.nullable ? 2u : 0u) | (sh.pk[i] ? 4u : 0u) | (((uint32_t)sc.key_index & 0xFFu) << 8) | ((uint32_t)sc.off_key << 16);
    // BigQuery compares the old and the new primary key of an update as Cells (bigquery_primary_key_changed, bigquery/core.rs:1557-1645):
    // the device does that where Cell equality is equality of the arena's words / bytes (not floats: NaN != NaN, 0.0 == -0.0; not
    // numeric / timetz / json / arrays, whose cells are compared as parsed values)
    if (sh.pk[i] && (cls == ETLG_TC_F32 || cls == ETLG_TC_F64 || cls == ETLG_TC_NUMERIC || cls == ETLG_TC_TIMETZ || cls == ETLG_TC_JSON || cls == ETLG_TC_ARRAY)) w.pk_comparable = false;
    const uint32_t elem = cls == ETLG_TC_ARRAY ? (uint32_t)etlg_array_elem_class(sc.type_oid) : 0u;
    if (cls == ETLG_TC_JSON || elem == ETLG_TC_JSON) w.has_json = true;
  }
  for (uint32_t i = 0; i < nc; i++) {
    const uint32_t cls = (uint32_t)sh.cols[i].type_class;
    uint32_t elem = 0;
    bool host_class = col_plan(cls).kind == ETLG_AK_TEXT_FORM && cls != ETLG_TC_JSON;   // numeric / timetz / json Display strings are formatted on the device (json: rb_json; a cell beyond json_display's limits is reported as host_event / host_column)
    if (cls == ETLG_TC_ARRAY) {  // arrays of fixed-width elements are encoded on the device (Array(Nullable(T)); BigQuery: packed / repeated fields behind the NULL-element rule)
      elem = (uint32_t)etlg_array_elem_class(sh.cols[i].type_oid);
      host_class = list_plan(elem).kind != ETLG_AK_LIST && elem != ETLG_TC_JSON;   // (text-like / numeric / timetz / bytea / json elements are written on the device too)
    }
    // (DuckLake predicates look at the key columns only: the identity columns, for a table-copy batch the primary-key ones)
    if ((w.dl == etlg::DL_SEL_PRED_PK && !sh.pk[i]) || (w.dl == etlg::DL_SEL_PRED_IDENT && !sh.cols[i].identity)) host_class = false;
    if (host_class) { w.host_column = i; return w; }
    w.cols[i] = cls | ((call.nullable_flags && call.nullable_flags[i]) ? 1u << 8 : 0u) | (elem << 9) | ((uint32_t)sh.cols[i].off_full << 16);
  }
  return w;
}

// Lanes per row in the byte pass (k_rb_rows): enough waves when the rows are few (~8 per SIMD), and few enough rows per workgroup
// (256 / parts) for their bytes to fit its LDS image (32 KB). test_override: the context's rb_parts_test, 0 for none
inline uint32_t rb_parts(uint64_t n, uint64_t total, uint32_t qparts, uint32_t test_override) {
  const uint64_t avg = total / n;
  const uint32_t by_rows = n * 4 <= 8ull * 64 * 1024 ? 4u : n * 2 <= 8ull * 64 * 1024 ? 2u : 1u, by_size = avg > 220 ? 4u : avg > 110 ? 2u : 1u;   // (256 / 128 / 64 rows of the average size in 28 KB)
  if (test_override) return std::min<uint32_t>(qparts, test_override >= 4 ? 4u : test_override >= 2 ? 2u : 1u);
  return std::min(qparts, std::max(by_rows, by_size));
}
