// Stand-alone check of etl_amd/csrc/handoff_plan.h (tests/test_handoff_plan.py builds it with the address and undefined-behaviour
// sanitizers; the header is included alone). Blocks A, B and C of build_columns: every part starts at a multiple of 64, parts are pairwise
// disjoint and inside total(), and every offset equals the offset chain the one-body build_columns walked — written out here link by link
// with this file's own rounding; nothing expected is obtained from the header's layouts. rb_parts at the edges of its thresholds, and
// row_words on tables that make key_ok, pk_comparable and the host class turn false one reason at a time.
#include "handoff_plan.h"

#include <cstdio>

static int bad = 0;
#define CHECK(cond) do { if (!(cond)) { bad++; std::printf("FAILED line %d: %s\n", __LINE__, #cond); } } while (0)
#define CHECK_EQ(a, b) do { const unsigned long long a_ = (unsigned long long)(a), b_ = (unsigned long long)(b); \
    if (a_ != b_) { bad++; std::printf("FAILED line %d: %s = %llu, expected %llu\n", __LINE__, #a, a_, b_); } } while (0)

static size_t up64(size_t x) { return (x + 63) / 64 * 64; }

// the header leaves this to the library: here an array type's oid is 5000 + its element class, any other oid has no dedicated arm
extern "C" int32_t etlg_array_elem_class(uint32_t oid) { return oid >= 5000 && oid < 5000 + ETLG_TC__COUNT ? (int32_t)(oid - 5000) : (int32_t)ETLG_TC_STRING; }

static etlg_slot_col col(uint32_t cls, uint32_t oid = 0, bool nullable = true, bool identity = false, uint32_t key_index = 0xFFFF) {
  etlg_slot_col c{};
  c.type_oid = oid; c.type_class = (uint8_t)cls; c.nullable = nullable; c.identity = identity; c.key_index = (uint16_t)key_index;
  return c;
}
static SlotHost slot_of(const std::vector<etlg_slot_col>& cols) {
  SlotHost sh{};
  sh.cols = cols; sh.pk.assign(cols.size(), 0);
  for (size_t i = 0; i < sh.cols.size(); i++) { sh.cols[i].off_full = (uint16_t)(8 + 16 * i); sh.cols[i].off_key = (uint16_t)(4 + 16 * i); if (sh.cols[i].identity) sh.desc.n_ident++; }
  sh.desc.n_cols = (uint32_t)cols.size();
  return sh;
}
// one column of every class (the text column with oid 25), then an array of every element class
static SlotHost every_class() {
  std::vector<etlg_slot_col> cols;
  for (uint32_t k = 0; k < ETLG_TC__COUNT; k++) if (k != ETLG_TC_ARRAY) cols.push_back(col(k, k == ETLG_TC_STRING ? 25 : 0));
  for (uint32_t e = 0; e < ETLG_TC__COUNT; e++) if (e != ETLG_TC_ARRAY) cols.push_back(col(ETLG_TC_ARRAY, 5000 + e));
  return slot_of(cols);
}

struct Part { size_t at, len; };
static void check_parts(const std::vector<Part>& parts, size_t total) {
  for (size_t i = 0; i < parts.size(); i++) {
    if (!parts[i].len) continue;   // (a part of no bytes lies nowhere)
    CHECK(parts[i].at % 64 == 0);
    CHECK(parts[i].at + parts[i].len <= total);
    for (size_t k = i + 1; k < parts.size(); k++) if (parts[k].len) CHECK(parts[i].at + parts[i].len <= parts[k].at || parts[k].at + parts[k].len <= parts[i].at);
  }
}

// The kind of every column as the one-body build_columns chose it, from the tables of col_plan / list_plan / dlc_plan restated per class
static void check_plans(const SlotHost& sh, ColCaller who, uint32_t row_kinds, const std::vector<ColPlan>& pl, uint32_t not_arrow) {
  const bool dlc = who == ColCaller::DuckLakeCopy;
  uint32_t want_refused = ~0u;
  CHECK_EQ(pl.size(), sh.desc.n_cols);
  for (uint32_t i = 0; i < sh.desc.n_cols; i++) {
    const uint32_t cls = sh.cols[i].type_class;
    ColPlan w = dlc ? dlc_plan(cls) : col_plan(cls);
    if (dlc && w.kind == ETLG_AK_NONE && want_refused == ~0u) want_refused = i;
    if ((row_kinds & ETLG_ROWS_PARSE_ARRAYS) && cls == ETLG_TC_ARRAY) w = list_plan((uint32_t)etlg_array_elem_class(sh.cols[i].type_oid));
    if ((row_kinds & ETLG_ROWS_FORMAT_JSON) && cls == ETLG_TC_JSON) w = ColPlan{ETLG_AK_LARGE_UTF8, 0, true, 0, 0, 0, etlg::kAkJsonStr};
    CHECK_EQ(pl[i].kind, w.kind); CHECK_EQ(pl[i].vbytes, w.vbytes); CHECK_EQ(pl[i].var, w.var); CHECK_EQ(pl[i].child, w.child);
    CHECK_EQ(pl[i].child_bytes, w.child_bytes); CHECK_EQ(pl[i].elem, w.elem); CHECK_EQ(pl[i].fmt, w.fmt);
    // what the tables say, for the classes whose width matters to the layouts
    if (!dlc && cls == ETLG_TC_I64) { CHECK_EQ(pl[i].kind, ETLG_AK_INT64); CHECK_EQ(pl[i].vbytes, 8); }
    if (!dlc && cls == ETLG_TC_BOOL) CHECK_EQ(pl[i].kind, ETLG_AK_BOOLEAN);
    if (dlc && cls == ETLG_TC_I16) { CHECK_EQ(pl[i].kind, ETLG_AK_INT16); CHECK_EQ(pl[i].vbytes, 2); }
    if (cls == ETLG_TC_UUID && !dlc) CHECK_EQ(pl[i].vbytes, 16);
  }
  CHECK_EQ(not_arrow, want_refused);
}

// Block A as the one-body build_columns carved it: row_event | per column validity, deferred, (offsets, lens) or values | the CDC columns | o_cnt | o_tot | o_scan
static void check_block_a(const std::vector<ColPlan>& pl, uint64_t n, bool changelog, bool dlc) {
  const ColumnsLayoutA la = columns_layout_a(pl, n, changelog, dlc);
  const size_t nc = pl.size(), bm = ((size_t)n + 63) / 64 * 8;
  std::vector<Part> parts{{0, (size_t)n * 8}};
  size_t off = up64(n * 8);
  CHECK_EQ(la.col.size(), nc);
  for (size_t i = 0; i < nc; i++) {
    const ColPartsA& p = la.col[i];
    if (pl[i].kind == ETLG_AK_NONE) { CHECK_EQ(p.validity + p.deferred + p.values + p.lens + p.offsets, 0); continue; }
    CHECK_EQ(p.validity, off); off += up64(bm); CHECK_EQ(p.deferred, off); off += up64(bm);
    parts.push_back({p.validity, bm}); parts.push_back({p.deferred, bm});
    if (pl[i].var) {
      const size_t ob = (n + 1) * (dlc ? 4 : 8);
      CHECK_EQ(p.offsets, off); off += up64(ob); CHECK_EQ(p.lens, off); off += up64(n * 4); CHECK_EQ(p.values, 0);
      parts.push_back({p.offsets, ob}); parts.push_back({p.lens, (size_t)n * 4});
    } else {
      const size_t vb = pl[i].kind == ETLG_AK_BOOLEAN ? bm : n * pl[i].vbytes;
      CHECK_EQ(p.values, off); off += up64(vb); CHECK_EQ(p.lens + p.offsets, 0);
      parts.push_back({p.values, vb});
    }
  }
  const uint32_t cdc_w[2] = {6u, 33u};
  for (int k = 0; k < 2; k++) {
    if (!changelog) { CHECK_EQ(la.cdc[k].validity + la.cdc[k].deferred + la.cdc[k].offsets + la.cdc[k].values, 0); continue; }
    CHECK_EQ(la.cdc[k].validity, off); off += up64(bm); CHECK_EQ(la.cdc[k].deferred, off); off += up64(bm);
    CHECK_EQ(la.cdc[k].offsets, off); off += up64((n + 1) * 8); CHECK_EQ(la.cdc[k].values, off); off += up64(n * cdc_w[k]);
    CHECK_EQ(kCdcWidth[k], cdc_w[k]);
    parts.push_back({la.cdc[k].validity, bm}); parts.push_back({la.cdc[k].deferred, bm}); parts.push_back({la.cdc[k].offsets, (size_t)(n + 1) * 8}); parts.push_back({la.cdc[k].values, (size_t)n * cdc_w[k]});
  }
  CHECK_EQ(la.cnt, off); off += up64(nc * 32);
  CHECK_EQ(la.tot, off); off += up64(nc * 8);
  const uint32_t nrb = (uint32_t)((n + 255) / 256);
  const size_t scan_one = up64((size_t)(nrb + 1) * 8);
  CHECK_EQ(la.scan_one, scan_one); CHECK_EQ(la.scan, off); off += scan_one * (nc > 1 ? nc : 1);
  CHECK_EQ(la.total, off);
  parts.push_back({la.cnt, nc * 32}); parts.push_back({la.tot, nc * 8});
  for (size_t i = 0; i < (nc > 1 ? nc : 1); i++) parts.push_back({la.scan + scan_one * i, scan_one});
  check_parts(parts, la.total);
}

// Blocks B and C as the one-body build_columns carved them
static void check_blocks_bc(const std::vector<ColPlan>& pl, uint64_t tot_each, uint64_t text_each) {
  const size_t nc = pl.size();
  std::vector<int64_t> var_total(nc, 0), text_total(nc, 0);
  for (size_t i = 0; i < nc; i++) { if (pl[i].var) var_total[i] = (int64_t)(tot_each + (tot_each ? i : 0)); if (pl[i].kind == ETLG_AK_LIST && var_child(pl[i])) text_total[i] = (int64_t)(text_each + (text_each ? 3 * i : 0)); }
  const ColumnsLayoutB lb = columns_layout_b(pl, var_total);
  std::vector<Part> parts;
  size_t off = 0; bool any_text_list = false;
  for (size_t i = 0; i < nc; i++) {
    const ColPartsB& p = lb.col[i];
    if (!pl[i].var) { CHECK_EQ(p.values + p.child_validity + p.child_lens + p.child_scan + p.values_bytes, 0); continue; }
    const size_t tot = (size_t)var_total[i], bits = (tot + 63) / 64 * 8;
    if (pl[i].kind == ETLG_AK_LIST) {
      if (var_child(pl[i])) {
        any_text_list = true;
        CHECK_EQ(p.values, off); off += up64((tot + 1) * 8); CHECK_EQ(p.child_lens, off); off += up64(tot * 4);
        CHECK_EQ(p.child_scan, off); off += up64((tot / 256 + 2) * 8); CHECK_EQ(p.child_validity, off); off += up64(bits);
        CHECK_EQ(p.values_bytes, 0);
        parts.push_back({p.values, (tot + 1) * 8}); parts.push_back({p.child_lens, tot * 4}); parts.push_back({p.child_scan, (tot / 256 + 2) * 8}); parts.push_back({p.child_validity, bits});
      } else {
        const size_t vbytes = pl[i].child == ETLG_AK_BOOLEAN ? bits : tot * pl[i].child_bytes;
        CHECK_EQ(p.values_bytes, vbytes); CHECK_EQ(p.values, off); off += up64(vbytes); CHECK_EQ(p.child_validity, off); off += up64(bits);
        parts.push_back({p.values, vbytes}); parts.push_back({p.child_validity, bits});
        if (tot) CHECK(p.child_validity - p.values + up64(bits) <= lb.total + 0 - p.values);   // the one memset over values .. validity stays inside
      }
    } else { CHECK_EQ(p.values_bytes, tot); CHECK_EQ(p.values, off); off += up64(tot); parts.push_back({p.values, tot}); }
  }
  CHECK_EQ(lb.total, off); CHECK_EQ(lb.any_text_list, any_text_list);
  check_parts(parts, lb.total);
  const ColumnsLayoutC lc = columns_layout_c(pl, text_total);
  parts.clear(); off = 0;
  for (size_t i = 0; i < nc; i++) {
    if (!(pl[i].kind == ETLG_AK_LIST && var_child(pl[i]))) { CHECK_EQ(lc.values[i], 0); continue; }
    CHECK_EQ(lc.values[i], off); parts.push_back({lc.values[i], (size_t)text_total[i]});
    off += up64((size_t)text_total[i]) + 64;
  }
  CHECK_EQ(lc.total, off);
  check_parts(parts, lc.total);
}

static void check_columns() {
  const SlotHost sh = every_class();
  const uint64_t ns[] = {0, 1, 63, 64, 65, 257}, tots[] = {0, 1, 64, 1000};
  for (int who = 0; who < 3; who++)
    for (uint32_t opts = 0; opts < 4; opts++) {
      const ColCaller w = who == 0 ? ColCaller::Columns : who == 1 ? ColCaller::Iceberg : ColCaller::DuckLakeCopy;
      const uint32_t row_kinds = ETLG_ROWS_INSERT | (opts & 1 ? ETLG_ROWS_PARSE_ARRAYS : 0u) | (opts & 2 ? ETLG_ROWS_FORMAT_JSON : 0u);
      uint32_t not_arrow = 0;
      const std::vector<ColPlan> pl = column_plans(sh, w, row_kinds, &not_arrow);
      check_plans(sh, w, row_kinds, pl, not_arrow);
      for (uint64_t n : ns)
        for (int changelog = 0; changelog < 2; changelog++)
          for (int dlc = 0; dlc < 2; dlc++) check_block_a(pl, n, changelog != 0, dlc != 0);
      for (uint64_t t : tots) for (uint64_t x : tots) check_blocks_bc(pl, t, x);
    }
  // a table the DuckLake copy takes: no refusal; an empty table: the scan scratch of one column is still there
  uint32_t not_arrow = 0;
  column_plans(slot_of({col(ETLG_TC_I16), col(ETLG_TC_STRING, 25), col(ETLG_TC_NUMERIC)}), ColCaller::DuckLakeCopy, ETLG_ROWS_INSERT, &not_arrow);
  CHECK_EQ(not_arrow, ~0u);
  check_block_a({}, 65, true, false);
}

// by_rows: 4 up to 8 * 64 * 1024 / 4 rows, 2 up to 8 * 64 * 1024 / 2, else 1; by_size: 4 above 220 bytes a row, 2 above 110; the larger of the
// two within qparts; a test's override replaces both
static void check_rb_parts() {
  const uint64_t q4 = 8ull * 64 * 1024 / 4, q2 = 8ull * 64 * 1024 / 2;
  CHECK_EQ(q4, 131072); CHECK_EQ(q2, 262144);
  CHECK_EQ(rb_parts(q4 - 1, 50 * (q4 - 1), 4, 0), 4); CHECK_EQ(rb_parts(q4, 50 * q4, 4, 0), 4); CHECK_EQ(rb_parts(q4 + 1, 50 * (q4 + 1), 4, 0), 2);
  CHECK_EQ(rb_parts(q2 - 1, 50 * (q2 - 1), 4, 0), 2); CHECK_EQ(rb_parts(q2, 50 * q2, 4, 0), 2); CHECK_EQ(rb_parts(q2 + 1, 50 * (q2 + 1), 4, 0), 1);
  const uint64_t big = q2 + 1000;   // rows so many that the size alone decides
  CHECK_EQ(rb_parts(big, 110 * big, 4, 0), 1); CHECK_EQ(rb_parts(big, 111 * big, 4, 0), 2); CHECK_EQ(rb_parts(big, 111 * big - 1, 4, 0), 1);
  CHECK_EQ(rb_parts(big, 220 * big, 4, 0), 2); CHECK_EQ(rb_parts(big, 221 * big, 4, 0), 4); CHECK_EQ(rb_parts(big, 221 * big - 1, 4, 0), 2);
  CHECK_EQ(rb_parts(1, 1, 4, 0), 4); CHECK_EQ(rb_parts(1, 1, 2, 0), 2); CHECK_EQ(rb_parts(1, 1000, 1, 0), 1); CHECK_EQ(rb_parts(big, 221 * big, 2, 0), 2);
  CHECK_EQ(rb_parts(1, 1, 4, 1), 1); CHECK_EQ(rb_parts(big, big, 4, 2), 2); CHECK_EQ(rb_parts(big, big, 4, 3), 2); CHECK_EQ(rb_parts(big, big, 4, 4), 4);
  CHECK_EQ(rb_parts(big, big, 4, 9), 4); CHECK_EQ(rb_parts(big, big, 2, 4), 2); CHECK_EQ(rb_parts(big, big, 1, 4), 1);
}

static RowsCall call_of(uint32_t format, const uint8_t* flags = nullptr, uint32_t dl_what = 0) { return RowsCall{format, flags, 0u, ETLG_CH_MERGE_TREE, nullptr, dl_what}; }

static void check_row_words() {
  using namespace etlg;
  // the words themselves
  {
    SlotHost sh = slot_of({col(ETLG_TC_I32, 23, false, true, 0), col(ETLG_TC_STRING, 25), col(ETLG_TC_ARRAY, 5000 + ETLG_TC_I64), col(ETLG_TC_JSON)});
    sh.pk[0] = 1; sh.identity_type = 1;
    const uint8_t nf[6] = {0, 1, 1, 0, 0, 0};
    const RowWords w = row_words(sh, call_of(FMT_ROWBINARY, nf), false);
    CHECK_EQ(w.host_column, ~0u); CHECK(w.key_ok); CHECK(w.pk_comparable); CHECK(w.has_json); CHECK_EQ(w.dl, DL_SEL_NONE);
    CHECK_EQ(w.cols.size(), 8);
    CHECK_EQ(w.cols[0], ETLG_TC_I32 | (8u << 16)); CHECK_EQ(w.cols[1], ETLG_TC_STRING | (1u << 8) | (24u << 16));
    CHECK_EQ(w.cols[2], ETLG_TC_ARRAY | (1u << 8) | ((uint32_t)ETLG_TC_I64 << 9) | (40u << 16)); CHECK_EQ(w.cols[3], ETLG_TC_JSON | (56u << 16));
    CHECK_EQ(w.cols[4], 1u | 4u | (0u << 8) | (4u << 16)); CHECK_EQ(w.cols[5], 2u | (0xFFu << 8) | (20u << 16));
    CHECK(!row_words(slot_of({col(ETLG_TC_I32)}), call_of(FMT_ROWBINARY), false).has_json);
    CHECK(row_words(slot_of({col(ETLG_TC_ARRAY, 5000 + ETLG_TC_JSON)}), call_of(FMT_ROWBINARY), false).has_json);
  }
  // key_ok: RowBinary only; identity PrimaryKey or Full; identity columns there; no nullable non-key String column of a type beyond text / varchar / bpchar / name / char
  {
    SlotHost sh = slot_of({col(ETLG_TC_I32, 23, false, true, 0), col(ETLG_TC_STRING, 25)});
    sh.identity_type = 1;
    CHECK(row_words(sh, call_of(FMT_ROWBINARY), false).key_ok);
    CHECK(!row_words(sh, call_of(FMT_PROTOBUF), false).key_ok); CHECK(!row_words(sh, call_of(FMT_NDJSON), false).key_ok); CHECK(!row_words(sh, call_of(FMT_DUCKLAKE, nullptr, ETLG_DL_TUPLES), false).key_ok);
    sh.identity_type = 2; CHECK(row_words(sh, call_of(FMT_ROWBINARY), false).key_ok);
    sh.identity_type = 0; CHECK(!row_words(sh, call_of(FMT_ROWBINARY), false).key_ok);
    sh.identity_type = 3; CHECK(!row_words(sh, call_of(FMT_ROWBINARY), false).key_ok);
    sh.identity_type = 1; sh.desc.n_ident = 0; CHECK(!row_words(sh, call_of(FMT_ROWBINARY), false).key_ok);
    sh.desc.n_ident = 1;
    for (uint32_t oid : {25u, 1043u, 1042u, 19u, 18u}) { sh.cols[1].type_oid = oid; CHECK(row_words(sh, call_of(FMT_ROWBINARY), false).key_ok); }
    sh.cols[1].type_oid = 3614; CHECK(!row_words(sh, call_of(FMT_ROWBINARY), false).key_ok);   // (a String cell of another type: the host knows whether it is an array)
    sh.cols[1].nullable = 0; CHECK(row_words(sh, call_of(FMT_ROWBINARY), false).key_ok);
    sh.cols[1].nullable = 1; sh.cols[1].identity = 1; CHECK(row_words(sh, call_of(FMT_ROWBINARY), false).key_ok);
  }
  // pk_comparable: no primary-key column of a class whose cells are not compared as words / bytes
  for (uint32_t k = 0; k < ETLG_TC__COUNT; k++) {
    SlotHost sh = slot_of({col(ETLG_TC_I32), col(k, k == ETLG_TC_ARRAY ? 5000 + ETLG_TC_I32 : 25)});
    const bool parsed = k == ETLG_TC_F32 || k == ETLG_TC_F64 || k == ETLG_TC_NUMERIC || k == ETLG_TC_TIMETZ || k == ETLG_TC_JSON || k == ETLG_TC_ARRAY;
    CHECK(row_words(sh, call_of(FMT_PROTOBUF), false).pk_comparable);   // not a key column: no matter
    sh.pk[1] = 1;
    CHECK_EQ(row_words(sh, call_of(FMT_PROTOBUF), false).pk_comparable, !parsed);
  }
  // the host class: a class without an Arrow kind of its own other than json; an array whose elements the device does not take apart (none of
  // today's element classes); DuckLake predicates look at the key columns only
  for (uint32_t k = 0; k < ETLG_TC__COUNT; k++) {
    if (k == ETLG_TC_ARRAY) continue;
    const RowWords w = row_words(slot_of({col(ETLG_TC_I32), col(k, 25)}), call_of(FMT_ROWBINARY), false);
    CHECK_EQ(w.host_column, col_plan(k).kind == ETLG_AK_TEXT_FORM && k != ETLG_TC_JSON ? 1u : ~0u);
    CHECK_EQ(w.host_column, ~0u);   // (every class has a device encoding today)
    CHECK_EQ(row_words(slot_of({col(ETLG_TC_ARRAY, 5000 + k)}), call_of(FMT_ROWBINARY), false).host_column, ~0u);
  }
  {
    SlotHost sh = slot_of({col(ETLG_TC_I32, 23, false, true, 0), col(ETLG_TC_ARRAY, 5000 + ETLG_TC_ARRAY), col(ETLG_TC_I64)});   // (an element class list_plan has no arm for)
    sh.pk[0] = 1; sh.pk[2] = 1;
    CHECK_EQ(row_words(sh, call_of(FMT_ROWBINARY), false).host_column, 1); CHECK_EQ(row_words(sh, call_of(FMT_NDJSON), false).host_column, 1);
    CHECK_EQ(row_words(sh, call_of(FMT_DUCKLAKE, nullptr, ETLG_DL_TUPLES), false).host_column, 1); CHECK_EQ(row_words(sh, call_of(FMT_DUCKLAKE, nullptr, ETLG_DL_UPDATES), false).host_column, 1);
    const RowWords ident = row_words(sh, call_of(FMT_DUCKLAKE, nullptr, ETLG_DL_PREDICATES), false), pk = row_words(sh, call_of(FMT_DUCKLAKE, nullptr, ETLG_DL_PREDICATES), true);
    CHECK_EQ(ident.dl, DL_SEL_PRED_IDENT); CHECK_EQ(ident.host_column, ~0u); CHECK_EQ(pk.dl, DL_SEL_PRED_PK); CHECK_EQ(pk.host_column, ~0u);
    sh.cols[1].identity = 1; CHECK_EQ(row_words(sh, call_of(FMT_DUCKLAKE, nullptr, ETLG_DL_PREDICATES), false).host_column, 1);
    CHECK_EQ(row_words(sh, call_of(FMT_DUCKLAKE, nullptr, ETLG_DL_PREDICATES), true).host_column, ~0u);
    sh.pk[1] = 1; CHECK_EQ(row_words(sh, call_of(FMT_DUCKLAKE, nullptr, ETLG_DL_PREDICATES), true).host_column, 1);
    CHECK_EQ(row_words(sh, call_of(FMT_DUCKLAKE, nullptr, ETLG_DL_TUPLES), true).dl, DL_SEL_TUPLES); CHECK_EQ(row_words(sh, call_of(FMT_DUCKLAKE, nullptr, ETLG_DL_UPDATES), true).dl, DL_SEL_UPDATES);
  }
}

int main() {
  check_columns();
  check_rb_parts();
  check_row_words();
  std::printf("mismatches %d\n", bad);
  return bad ? 1 : 0;
}
