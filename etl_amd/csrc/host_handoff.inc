// Part of host.cpp (included there, one translation unit): the columnar hand-off calls over a decoded, device-resident batch (kernels: columns.hip, rowformats.hip, finish.hip).

extern "C++" {
// ---- columnar hand-off (columns.hip, rowformats.hip, finish.hip)
// What every hand-off call does first: an ASYNC batch is synchronised — one that ended in a decode error gives the caller that error
// (fail-fast, as the reference), not a hand-off of the prefix — and a batch that is not device-resident is refused. `refusal`: the
// entry point's name + NEEDS_DEVICE (a string literal: the error keeps the pointer). Returns ETLG_OK, or what the caller returns.
#define NEEDS_DEVICE " needs a device-resident batch (ETLG_F_OUTPUT_ON_DEVICE, not downloaded)"
static int32_t batch_ready(etlg_ctx* c, etlg_batch* b, const char* refusal) {
  if (b->pending) RC(etlg_batch_sync(c, b));
  if (!b->v.on_device || !b->dev) return lib_error(c, ETLG_InvalidState, refusal);
  return ETLG_OK;
}
namespace {
struct ColPlan { uint32_t kind, vbytes; bool var; uint32_t child = 0, child_bytes = 0, elem = 0, fmt = 0; };   // fmt: the kernels' internal kind of a formatted string column (columns.hip AK_*_STR)
ColPlan list_plan(uint32_t elem) {  // array literals the device parses: element classes with a fixed-width value
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
bool var_child(const ColPlan& p) { return p.child == ETLG_AK_LARGE_UTF8 || p.child == ETLG_AK_LARGE_BINARY; }   // list children with offsets of their own
ColPlan col_plan(uint32_t cls) {
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
ColPlan dlc_plan(uint32_t cls) {
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
}  // namespace
}  // extern "C++"

// The builder behind etlg_batch_columns and etlg_batch_iceberg. sel_kinds: ColSel.kinds (SEL_* bits); changelog: the Iceberg sink's rows — the refused events are counted in the selection's own
// launches and read back with the row count, and the two CDC columns are written behind the data columns by one more launch
// (etlg_k_col_cdc), so both calls stop for the device equally often.
static bool slot_known(const etlg_ctx* c, int32_t slot) { return slot >= 0 && (size_t)slot < c->slots.size(); }
// dlc: etlg_batch_ducklake_copy — a table-copy batch's rows under dlc_plan's kinds, Utf8 / Binary with int32 offsets; the same launches
// and the same stops as etlg_batch_columns(INSERT) on the slot.
enum class ColCaller { Columns, Iceberg, DuckLakeCopy };   // which entry point build_columns serves
static int32_t build_columns(etlg_ctx* c, etlg_batch* b, int32_t slot, uint32_t sel_kinds, uint32_t row_kinds, uint32_t flags, ColCaller who, etlg_columns** out) {
  *out = nullptr;
  const bool changelog = who == ColCaller::Iceberg, dlc = who == ColCaller::DuckLakeCopy;
  if (const int32_t rc = batch_ready(c, b, dlc ? "etlg_batch_ducklake_copy" NEEDS_DEVICE : changelog ? "etlg_batch_iceberg" NEEDS_DEVICE : "etlg_batch_columns" NEEDS_DEVICE)) return rc;
  if (!slot_known(c, slot) || !sel_kinds) return ETLG_InvalidArgument;
  if (dlc && !b->copy.active) return lib_error(c, ETLG_InvalidArgument, "etlg_batch_ducklake_copy takes a table-copy batch (etlg_copy_decode): the sink stages copy rows only as Arrow");
  const bool parse_arrays = (row_kinds & ETLG_ROWS_PARSE_ARRAYS) != 0;
  const bool format_json = (row_kinds & ETLG_ROWS_FORMAT_JSON) != 0;
  const SlotHost& sh = *c->slots[(size_t)slot];
  hipStream_t s = c->stream;
  const etlg_batch_view& bv = b->v;
  std::unique_ptr<etlg_columns, void (*)(etlg_columns*)> cs(new etlg_columns, etlg_columns_free);
  const uint64_t ne = bv.n_events;
  const uint32_t nblk = (uint32_t)((ne + 255) / 256);
  // ---- 1. which events are rows (count -> scan -> scatter); row_event / row_base are sized for every event
  ScratchLayout sel_lay((size_t)(nblk + 1) * 4);
  const size_t o_ice = sel_lay.skip(64);   // changelog: {refused events, -, -, min(event << 8 | reason)} behind the block counts
  HIPCHK(c, c->d_colsel.ensure(sel_lay.total()));
  uint32_t* d_blk = (uint32_t*)c->d_colsel.p;
  cs->m.ctx = c; cs->m.ctx_gen = c->gen;
  cs->changelog = changelog; cs->ci.host_event = ~0ull; cs->ci.n_data_cols = sh.desc.n_cols;
  cs->ducklake = dlc;
  // nothing is built and nothing handed over: the view has no rows and no columns, `di` says why and for which column
  auto dlc_refuse = [&](uint32_t status, uint32_t column) -> int32_t {
    cs->di.status = status; cs->di.column = column;
    cs->v.on_device = (flags & ETLG_F_OUTPUT_ON_DEVICE) ? 1u : 0u;
    *out = cs.release();
    return ETLG_OK;
  };
  if (dlc) for (uint32_t i = 0; i < sh.desc.n_cols; i++) if (dlc_plan(sh.cols[i].type_class).kind == ETLG_AK_NONE) return dlc_refuse(ETLG_DLC_NOT_ARROW, i);
  // pinned {0, 0, 0, ~0} records: the initial values of the columns' counters (and of the changelog's refusal words) go up as an
  // asynchronous copy (a pageable source made it a synchronisation)
  auto cnt_init = [&](size_t want) -> int32_t {
    if (c->h_cnt_init_cols >= want) return ETLG_OK;
    if (c->h_cnt_init) { HIPCHK(c, hipStreamSynchronize(s)); (void)hipHostFree(c->h_cnt_init); c->h_cnt_init = nullptr; c->h_cnt_init_cols = 0; }
    const size_t cap = want + 64;
    HIPCHK(c, hipHostMalloc((void**)&c->h_cnt_init, cap * 32, hipHostMallocDefault));
    for (size_t i = 0; i < cap; i++) { c->h_cnt_init[4 * i] = c->h_cnt_init[4 * i + 1] = c->h_cnt_init[4 * i + 2] = 0ull; c->h_cnt_init[4 * i + 3] = ~0ull; }
    c->h_cnt_init_cols = cap;
    return ETLG_OK;
  };
  ScratchBlk rows_blk{c};
  ScratchLayout rows_lay(ne * 8); const size_t o_row_base = rows_lay.take(ne * 8);   // row_event | row_base
  if (ne) HIPCHK(c, blk_take(c, rows_lay.total(), false, &rows_blk.p, &rows_blk.cap));
  uint64_t* d_row_event = (uint64_t*)rows_blk.p;
  uint64_t* d_row_base = (uint64_t*)((uint8_t*)rows_blk.p + o_row_base);
  uint32_t n_rows32 = 0;
  if (ne) {
    ColSel q{};
    q.ev_kind = bv.ev_kind; q.ev_flags = bv.ev_flags; q.ev_slot = bv.ev_schema_slot; q.ev_body = bv.ev_body_off;
    q.n_events = ne; q.slot = (uint32_t)slot; q.kinds = sel_kinds;
    q.row_full = sh.desc.row_bytes_full; q.row_key = sh.desc.row_bytes_key;
    q.blk = d_blk; q.nblocks = nblk; q.row_event = d_row_event; q.row_base = d_row_base;
    unsigned long long back[(64 + 32) / 8] = {0};   // the row count; changelog: ... up to the refusal words, which ride the same copy
    const size_t back_bytes = changelog ? o_ice + 32 - (size_t)nblk * 4 : 4;
    if (changelog) {
      RC(cnt_init(1));
      q.ice = (unsigned long long*)((uint8_t*)d_blk + o_ice);
      HIPCHK(c, hipMemcpyAsync(q.ice, c->h_cnt_init, 32, hipMemcpyHostToDevice, s));
    }
    etlg_k_col_select(&q, s);
    HIPCHK(c, hipMemcpyAsync(back, d_blk + nblk, back_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    memcpy(&n_rows32, back, 4);
    if (changelog) {
      unsigned long long ice[4];
      memcpy(ice, (const uint8_t*)back + (back_bytes - 32), 32);
      cs->ci.n_host_rows = ice[0];
      if (ice[3] != ~0ull) { cs->ci.host_event = ice[3] >> 8; cs->ci.host_reason = (uint32_t)(ice[3] & 0xFFu); }
    }
  }
  const uint64_t n = n_rows32;
  // ---- 2. block A: row_event | per column {validity, deferred, values or (lens, offsets)} | counters
  const uint32_t nc = sh.desc.n_cols;
  const size_t bm = ((size_t)n + 63) / 64 * 8;   // bytes of a bitmap
  struct Lay { ColPlan pl; size_t validity, deferred, values, lens, offsets; };
  std::vector<Lay> lay(nc);
  ScratchLayout a_lay(n * 8);   // row_event first
  for (uint32_t i = 0; i < nc; i++) {
    Lay& l = lay[i];
    l.pl = dlc ? dlc_plan(sh.cols[i].type_class) : col_plan(sh.cols[i].type_class);
    if (parse_arrays && sh.cols[i].type_class == ETLG_TC_ARRAY) l.pl = list_plan((uint32_t)etlg_array_elem_class(sh.cols[i].type_oid));
    if (format_json && sh.cols[i].type_class == ETLG_TC_JSON) l.pl = {ETLG_AK_LARGE_UTF8, 0, true, 0, 0, 0, etlg::kAkJsonStr};   // `j.to_string()` written on the device (AK_JSON_STR)
    l.validity = l.deferred = l.values = l.lens = l.offsets = 0;
    if (l.pl.kind == ETLG_AK_NONE) continue;
    l.validity = a_lay.take(bm); l.deferred = a_lay.take(bm);
    if (l.pl.var) { l.offsets = a_lay.take((n + 1) * (dlc ? 4 : 8)); l.lens = a_lay.take(n * 4); }
    else l.values = a_lay.take(l.pl.kind == ETLG_AK_BOOLEAN ? bm : n * l.pl.vbytes);
  }
  // changelog: the two CDC columns — per column validity, deferred, offsets, values (fixed-width strings: sized here, in block A)
  const uint32_t cdc_w[2] = {6u, 33u};
  size_t cdc_validity[2] = {0, 0}, cdc_deferred[2] = {0, 0}, cdc_offsets[2] = {0, 0}, cdc_values[2] = {0, 0};
  if (changelog) for (int k = 0; k < 2; k++) {
    cdc_validity[k] = a_lay.take(bm); cdc_deferred[k] = a_lay.take(bm);
    cdc_offsets[k] = a_lay.take((n + 1) * 8); cdc_values[k] = a_lay.take(n * cdc_w[k]);
  }
  const size_t o_cnt = a_lay.take((size_t)nc * 32);   // per column: nulls, deferred, child nulls, first list error
  const size_t o_tot = a_lay.take((size_t)nc * 8);    // per var-len column: the bytes behind its offsets (one read-back for all)
  const uint32_t nrb = (uint32_t)((n + 255) / 256);
  const size_t scan_one = al64((size_t)(nrb + 1) * 8);
  const size_t o_scan = a_lay.skip(scan_one * std::max<uint32_t>(nc, 1u));   // a scan scratch per column: the var-len columns' first passes run as ONE launch each (etlg_k_col_var_pack)
  HIPCHK(c, blk_take(c, a_lay.total() + 64, false, &cs->m.d_a, &cs->m.cap_a));
  uint8_t* A = (uint8_t*)cs->m.d_a;
  if (nc) {   // the counters' initial values
    RC(cnt_init(nc));
    HIPCHK(c, hipMemcpyAsync(A + o_cnt, c->h_cnt_init, (size_t)nc * 32, hipMemcpyHostToDevice, s));
  }
  if (n) HIPCHK(c, hipMemcpyAsync(A, d_row_event, n * 8, hipMemcpyDeviceToDevice, s));
  if (changelog) {
    if (n) {
      CdcJob cj{};
      cj.row_event = d_row_event; cj.ev_kind = bv.ev_kind; cj.ev_commit = bv.ev_commit_lsn; cj.ev_ord = bv.ev_tx_ordinal;
      cj.n_rows = n; cj.zero_token = b->copy.active ? 1u : 0u;   // a table-copy batch (etlg_copy_decode), told as etlg_batch_ndjson tells it
      cj.op_values = A + cdc_values[0]; cj.seq_values = A + cdc_values[1];
      cj.op_offsets = (int64_t*)(A + cdc_offsets[0]); cj.seq_offsets = (int64_t*)(A + cdc_offsets[1]);
      cj.op_validity = (unsigned long long*)(A + cdc_validity[0]); cj.seq_validity = (unsigned long long*)(A + cdc_validity[1]);
      cj.op_deferred = (unsigned long long*)(A + cdc_deferred[0]); cj.seq_deferred = (unsigned long long*)(A + cdc_deferred[1]);
      etlg_k_col_cdc(&cj, s);
    } else {
      for (int k = 0; k < 2; k++) HIPCHK(c, hipMemsetAsync(A + cdc_offsets[k], 0, 8, s));
    }
  }
  std::vector<ColJob> jobs(nc);
  std::vector<int64_t> var_total(nc, 0);
  std::vector<uint32_t> fixed_ids, var_ids;   // columns whose kernels travel in packs (list columns keep launches of their own)
  for (uint32_t i = 0; i < nc; i++) {
    const Lay& l = lay[i];
    if (l.pl.kind == ETLG_AK_NONE) continue;
    ColJob& j = jobs[i];
    j = ColJob{};
    j.fixed = bv.fixed; j.heap = bv.heap; j.row_base = d_row_base; j.n_rows = n;
    j.col_index = i; j.off_full = sh.cols[i].off_full; j.cls = sh.cols[i].type_class; j.kind = l.pl.fmt ? l.pl.fmt : l.pl.kind;
    j.validity = (unsigned long long*)(A + l.validity); j.deferred = (unsigned long long*)(A + l.deferred);
    j.null_count = (unsigned long long*)(A + o_cnt + (size_t)i * 32); j.deferred_count = j.null_count + 1;
    j.child_nulls = j.null_count + 2; j.err = j.null_count + 3; j.elem_cls = l.pl.elem; j.off32 = dlc ? 1u : 0u;
    if (l.pl.var) {
      j.lens = (uint32_t*)(A + l.lens); j.offsets = (const int64_t*)(A + l.offsets);
      if (n) {
        if (l.pl.kind == ETLG_AK_LIST) { j.kind = l.pl.child; etlg_k_col_list(&j, (unsigned long long*)(A + o_scan + scan_one * i), (int64_t*)(A + l.offsets), 0, s); }
        else var_ids.push_back(i);
      } else {
        HIPCHK(c, hipMemsetAsync(A + l.offsets, 0, 8, s));
      }
    } else {
      j.values = A + l.values;
      fixed_ids.push_back(i);
    }
  }
  // every fixed-width column in one launch (per pack of etlg_k_col_pack_max() columns), pass 1 of every var-len column in three
  {
    const uint32_t pm = etlg_k_col_pack_max();
    std::vector<ColJob> pj; std::vector<unsigned long long*> pb, pt; std::vector<int64_t*> po;
    for (size_t k0 = 0; k0 < fixed_ids.size(); k0 += pm) {
      pj.clear();
      for (size_t k = k0; k < std::min(fixed_ids.size(), k0 + pm); k++) pj.push_back(jobs[fixed_ids[k]]);
      etlg_k_col_fixed_pack(pj.data(), (uint32_t)pj.size(), s);
    }
    for (size_t k0 = 0; k0 < var_ids.size(); k0 += pm) {
      pj.clear(); pb.clear(); po.clear(); pt.clear();
      for (size_t k = k0; k < std::min(var_ids.size(), k0 + pm); k++) {
        const uint32_t i = var_ids[k];
        pj.push_back(jobs[i]); pb.push_back((unsigned long long*)(A + o_scan + scan_one * i)); po.push_back((int64_t*)(A + lay[i].offsets));
        pt.push_back((unsigned long long*)(A + o_tot) + i);
      }
      etlg_k_col_var_pack(pj.data(), (uint32_t)pj.size(), pb.data(), po.data(), pt.data(), 0, s);
    }
    if (n) for (uint32_t i = 0; i < nc; i++) if (lay[i].pl.kind == ETLG_AK_LIST)
      HIPCHK(c, hipMemcpyAsync(&var_total[i], A + lay[i].offsets + n * 8, 8, hipMemcpyDeviceToHost, s));
  }
  // the counters and the var-len totals lie next to each other: one read-back for both
  std::vector<uint64_t> cnt((o_tot - o_cnt) / 8 + nc, 0);
  if (nc) HIPCHK(c, hipMemcpyAsync(cnt.data(), A + o_cnt, cnt.size() * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  if (n) for (uint32_t i : var_ids) var_total[i] = (int64_t)cnt[(o_tot - o_cnt) / 8 + i];
  {  // a malformed array literal: the reference's error, for the first such row in event order
    // every column reports the minimum of (row << 8 | code) over its own cells; across columns the order is the reference's parse
    // order — row-major, then column-major (convert_tuple_to_row walks the columns of a row in order) — so the first column wins
    // inside a row: a hand-back in an earlier column of the row ranks before a malformed literal in a later one
    uint64_t first = ~0ull;
    for (uint32_t i = 0; i < nc; i++) if (lay[i].pl.kind == ETLG_AK_LIST || sh.cols[i].type_class == ETLG_TC_JSON) {   // (a json cell that is not one JSON value: the same report)
      const uint64_t k = cnt[(size_t)i * 4 + 3];
      if (k != ~0ull && (first == ~0ull || (k >> 8) < (first >> 8))) first = k;   // strictly earlier row; ties keep the earlier column
    }
    if (first != ~0ull && (first & 0xFF) != kArrHandBack) {   // (kArrHandBack: the first row that is not a plain list was handed back DEFERRED, not malformed — k_arr_count)
      uint64_t ev = 0;
      HIPCHK(c, hipMemcpy(&ev, d_row_event + (first >> 8), 8, hipMemcpyDeviceToHost));
      return set_error(c, (int32_t)(first & 0xFF), (int64_t)ev);
    }
  }
  if (dlc) {   // arrow-rs panics when a StringArray's / BinaryArray's bytes pass i32::MAX: the totals came back with the counters
    const uint64_t cap = c->dlc_offset_cap_test ? c->dlc_offset_cap_test : 0x7FFFFFFFull;
    for (uint32_t i : var_ids) if ((uint64_t)var_total[i] > cap) {
      blk_give(c, c->gen, cs->m.d_a, cs->m.cap_a, false); cs->m.d_a = nullptr;
      return dlc_refuse(ETLG_DLC_OFFSETS_OVERFLOW, i);
    }
  }
  // ---- 3. block B: the bytes of the var-len columns; list columns: child values (or, for lists of strings, child offsets +
  //      lengths) and child validity
  std::vector<size_t> vb(nc, 0);
  ScratchLayout b_lay;
  std::vector<size_t> cvb(nc, 0), vbytes(nc, 0), clen(nc, 0), cscan(nc, 0);   // list columns: child validity offset; bytes behind `values`; child lens; scan scratch
  bool any_text_list = false;
  for (uint32_t i = 0; i < nc; i++) {
    if (!lay[i].pl.var) continue;
    const size_t tot = (size_t)var_total[i];
    if (lay[i].pl.kind == ETLG_AK_LIST) {
      const size_t bits = (tot + 63) / 64 * 8;
      if (var_child(lay[i].pl)) {   // child offsets first (i64), then lengths, scan scratch, validity
        any_text_list = true;
        vb[i] = b_lay.take((tot + 1) * 8); clen[i] = b_lay.take(tot * 4); cscan[i] = b_lay.take((tot / 256 + 2) * 8);
        cvb[i] = b_lay.take(bits);
      } else {
        vbytes[i] = lay[i].pl.child == ETLG_AK_BOOLEAN ? bits : tot * lay[i].pl.child_bytes;
        vb[i] = b_lay.take(vbytes[i]); cvb[i] = b_lay.take(bits);
      }
    } else { vbytes[i] = tot; vb[i] = b_lay.take(tot); }
  }
  const size_t b_bytes = b_lay.total();
  if (b_bytes) HIPCHK(c, blk_take(c, b_bytes + 64, false, &cs->m.d_b, &cs->m.cap_b));
  uint8_t* B = (uint8_t*)cs->m.d_b;
  std::vector<int64_t> text_total(nc, 0);
  std::vector<uint32_t> var2_ids;
  for (uint32_t i = 0; i < nc; i++) {
    if (!lay[i].pl.var || var_total[i] <= 0) continue;
    if (lay[i].pl.kind == ETLG_AK_LIST) {
      jobs[i].child_validity = (uint32_t*)(B + cvb[i]);
      if (var_child(lay[i].pl)) {   // pass A: byte length + validity of every element, then their offsets
        jobs[i].values = nullptr; jobs[i].child_lens = (uint32_t*)(B + clen[i]); jobs[i].child_offsets = (const int64_t*)(B + vb[i]);
        HIPCHK(c, hipMemsetAsync(B + cvb[i], 0, al64(((size_t)var_total[i] + 63) / 64 * 8), s));
        etlg_k_col_list(&jobs[i], nullptr, nullptr, 1, s);
        etlg_k_scan_lens(jobs[i].child_lens, (uint64_t)var_total[i], (unsigned long long*)(B + cscan[i]), (int64_t*)(B + vb[i]), s);
        HIPCHK(c, hipMemcpyAsync(&text_total[i], B + vb[i] + (size_t)var_total[i] * 8, 8, hipMemcpyDeviceToHost, s));
      } else {
        jobs[i].values = B + vb[i];
        HIPCHK(c, hipMemsetAsync(B + vb[i], 0, cvb[i] - vb[i] + al64(((size_t)var_total[i] + 63) / 64 * 8), s));   // bitmaps are OR-ed into
        etlg_k_col_list(&jobs[i], nullptr, nullptr, 1, s);
      }
    } else { jobs[i].values = B + vb[i]; var2_ids.push_back(i); }
  }
  {  // pass 2 of the var-len columns (copy / format), one launch per pack
    const uint32_t pm = etlg_k_col_pack_max();
    std::vector<ColJob> pj;
    for (size_t k0 = 0; k0 < var2_ids.size(); k0 += pm) {
      pj.clear();
      for (size_t k = k0; k < std::min(var2_ids.size(), k0 + pm); k++) pj.push_back(jobs[var2_ids[k]]);
      etlg_k_col_var_pack(pj.data(), (uint32_t)pj.size(), nullptr, nullptr, nullptr, 1, s);
    }
  }
  // ---- 3b. block C: the element bytes of lists of strings
  std::vector<size_t> vc(nc, 0);
  ScratchLayout c_lay;
  if (any_text_list) {
    HIPCHK(c, hipStreamSynchronize(s));
    for (uint32_t i = 0; i < nc; i++) if (lay[i].pl.kind == ETLG_AK_LIST && var_child(lay[i].pl)) { vbytes[i] = (size_t)text_total[i]; vc[i] = c_lay.take(vbytes[i]); c_lay.skip(64); }
    if (c_lay.total()) HIPCHK(c, blk_take(c, c_lay.total() + 64, false, &cs->m.d_c, &cs->m.cap_c));
    for (uint32_t i = 0; i < nc; i++)
      if (lay[i].pl.kind == ETLG_AK_LIST && var_child(lay[i].pl) && var_total[i] > 0) { jobs[i].values = (uint8_t*)cs->m.d_c + vc[i]; etlg_k_col_list(&jobs[i], nullptr, nullptr, 1, s); }
  }
  uint8_t* Cb = (uint8_t*)cs->m.d_c; const size_t c_bytes = c_lay.total();
  if (nc) HIPCHK(c, hipMemcpyAsync(cnt.data(), A + o_cnt, (size_t)nc * 32, hipMemcpyDeviceToHost, s));   // again: the child null counts
  // ---- 4. the view (device pointers, or a host copy of the blocks)
  const bool on_dev = (flags & ETLG_F_OUTPUT_ON_DEVICE) != 0;
  const uint8_t* base_a = A; const uint8_t* base_b = B; const uint8_t* base_c = Cb;
  if (!on_dev) {
    HIPCHK(c, blk_take(c, al64(o_cnt) + al64(b_bytes) + c_bytes + 64, true, (void**)&cs->m.h, &cs->m.cap_h));
    if (o_cnt) HIPCHK(c, hipMemcpyAsync(cs->m.h, A, o_cnt, hipMemcpyDeviceToHost, s));
    if (b_bytes) HIPCHK(c, hipMemcpyAsync(cs->m.h + al64(o_cnt), B, b_bytes, hipMemcpyDeviceToHost, s));
    if (c_bytes) HIPCHK(c, hipMemcpyAsync(cs->m.h + al64(o_cnt) + al64(b_bytes), Cb, c_bytes, hipMemcpyDeviceToHost, s));
    base_a = cs->m.h; base_b = cs->m.h + al64(o_cnt); base_c = cs->m.h + al64(o_cnt) + al64(b_bytes);
  }
  HIPCHK(c, hipStreamSynchronize(s));   // row_base (freed on return) is read by the kernels above
  if (!on_dev) {
    blk_give(c, c->gen, cs->m.d_a, cs->m.cap_a, false); blk_give(c, c->gen, cs->m.d_b, cs->m.cap_b, false); blk_give(c, c->gen, cs->m.d_c, cs->m.cap_c, false);
    cs->m.d_a = cs->m.d_b = cs->m.d_c = nullptr;
  }
  cs->cols.resize(nc + (changelog ? 2u : 0u));
  if (changelog) for (uint32_t t = 0; t < 2; t++) {
    etlg_column& k = cs->cols[nc + t];
    k = etlg_column{};
    k.type_class = ETLG_TC_STRING; k.arrow_kind = ETLG_AK_LARGE_UTF8;
    k.validity = base_a + cdc_validity[t]; k.deferred = base_a + cdc_deferred[t];
    k.offsets = (const int64_t*)(base_a + cdc_offsets[t]); k.values = base_a + cdc_values[t]; k.values_bytes = n * cdc_w[t];
  }
  for (uint32_t i = 0; i < nc; i++) {
    etlg_column& k = cs->cols[i];
    const Lay& l = lay[i];
    k = etlg_column{};
    k.type_class = sh.cols[i].type_class; k.arrow_kind = l.pl.kind; k.value_bytes = l.pl.vbytes; k.nullable = sh.cols[i].nullable;
    if (l.pl.kind == ETLG_AK_NONE) continue;
    k.null_count = cnt[(size_t)i * 4]; k.deferred_count = cnt[(size_t)i * 4 + 1];
    k.validity = base_a + l.validity; k.deferred = base_a + l.deferred;
    if (l.pl.var) { k.offsets = (const int64_t*)(base_a + l.offsets); k.values = base_b ? base_b + vb[i] : nullptr; k.values_bytes = (uint64_t)vbytes[i]; }
    if (l.pl.kind == ETLG_AK_LIST) {
      k.child_kind = l.pl.child; k.child_count = (uint64_t)var_total[i]; k.child_null_count = cnt[(size_t)i * 4 + 2];
      k.child_validity = base_b ? base_b + cvb[i] : nullptr;
      if (var_child(l.pl)) {   // element texts / bytes: offsets in block B, bytes in block C
        k.child_offsets = base_b ? (const int64_t*)(base_b + vb[i]) : nullptr;
        k.values = base_c ? base_c + vc[i] : nullptr;
      }
    }
    if (!l.pl.var) { k.values = base_a + l.values; k.values_bytes = l.pl.kind == ETLG_AK_BOOLEAN ? ((n + 63) / 64) * 8 : n * l.pl.vbytes; }
  }
  cs->v.n_rows = n; cs->v.n_cols = (uint32_t)cs->cols.size(); cs->v.on_device = on_dev ? 1u : 0u; cs->v.cols = cs->cols.data();
  cs->v.row_event = (const uint64_t*)base_a;
  *out = cs.release();
  return ETLG_OK;
}

static_assert(SEL_INSERT == ETLG_ROWS_INSERT && SEL_UPDATE_NEW == ETLG_ROWS_UPDATE, "etlg_batch_columns passes the public row kinds through as ColSel.kinds");
int32_t etlg_batch_columns(etlg_ctx* c, etlg_batch* b, int32_t slot, uint32_t row_kinds, uint32_t flags, etlg_columns** out) {
  if (!c || !b || !out || b->ctx != c) return ETLG_InvalidArgument;
  return build_columns(c, b, slot, row_kinds & (SEL_INSERT | SEL_UPDATE_NEW), row_kinds, flags, ColCaller::Columns, out);
}

int32_t etlg_batch_iceberg(etlg_ctx* c, etlg_batch* b, int32_t slot, uint32_t opts, uint32_t flags, etlg_columns** out) {
  if (!c || !b || !out || b->ctx != c) return ETLG_InvalidArgument;
  *out = nullptr;
  if (opts & ~(ETLG_ROWS_PARSE_ARRAYS | ETLG_ROWS_FORMAT_JSON)) return lib_error(c, ETLG_InvalidArgument, "etlg_batch_iceberg: opts takes ETLG_ROWS_PARSE_ARRAYS | ETLG_ROWS_FORMAT_JSON only (the row kinds are fixed)");
  return build_columns(c, b, slot, SEL_INSERT | SEL_UPDATE_NEW | SEL_DELETE_OLD, opts, flags, ColCaller::Iceberg, out);
}

// DuckLake's copy payload for a table arrow_column_kinds accepts (prepare_copy_rows -> copy_rows_to_arrow_record_batch,
// ducklake/encoding.rs:32-49, :303-340): build_columns' third caller, with a kind table of its own.
int32_t etlg_batch_ducklake_copy(etlg_ctx* c, etlg_batch* b, int32_t slot, uint32_t flags, etlg_columns** out) {
  if (!c || !b || !out || b->ctx != c) return ETLG_InvalidArgument;
  return build_columns(c, b, slot, SEL_INSERT, ETLG_ROWS_INSERT, flags, ColCaller::DuckLakeCopy, out);
}

int32_t etlg_columns_ducklake_get(const etlg_columns* cs, etlg_ducklake_copy_info* out) {
  if (!cs || !out || !cs->ducklake) return ETLG_InvalidArgument;
  *out = cs->di;
  return ETLG_OK;
}

int32_t etlg_columns_changelog_get(const etlg_columns* cs, etlg_changelog_info* out) {
  if (!cs || !out || !cs->changelog) return ETLG_InvalidArgument;
  *out = cs->ci;
  return ETLG_OK;
}

// The records k_size_hints and the finish pass read (SlotRec / ColRec) for the slots [0, ns): every slot for the size hints, the slots the batch's view
// lists for the finish pass. `what`: the ETLG_FINISH_* bits whose finishable columns (arrays the device takes apart, floats) `fin` lists; 0 for the hints
static bool fin_elem_ok(int32_t e) {
  return e == ETLG_TC_BOOL || e == ETLG_TC_I16 || e == ETLG_TC_I32 || e == ETLG_TC_I64 || e == ETLG_TC_U32 || e == ETLG_TC_F32 || e == ETLG_TC_F64 || e == ETLG_TC_DATE ||
         e == ETLG_TC_TIME || e == ETLG_TC_TIMETZ || e == ETLG_TC_TIMESTAMP || e == ETLG_TC_TIMESTAMPTZ || e == ETLG_TC_UUID || e == ETLG_TC_NUMERIC || e == ETLG_TC_BYTEA ||
         e == ETLG_TC_STRING;
}
struct SlotTable { std::vector<SlotRec> slots; std::vector<ColRec> cols; std::vector<uint32_t> fin; uint32_t maxfin = 0; bool any_arrays = false; };
static SlotTable slot_table(const etlg_ctx* c, uint32_t ns, uint32_t what) {
  SlotTable t; t.slots.resize(ns);
  for (uint32_t i = 0; i < ns; i++) {
    const SlotHost& sh = *c->slots[i];
    SlotRec& r = t.slots[i] = SlotRec{sh.desc.n_cols, sh.desc.n_ident, sh.desc.row_bytes_full, sh.desc.row_bytes_key, (uint32_t)t.cols.size(), (uint32_t)t.fin.size(), 0u};
    uint32_t k = 0;
    for (const etlg_slot_col& col : sh.cols) {
      const int32_t elem = col.type_class == ETLG_TC_ARRAY ? etlg_array_elem_class(col.type_oid) : 0;
      t.cols.push_back(ColRec{(uint32_t)col.type_class | (col.identity ? 1u << 8 : 0u) | ((uint32_t)elem << 16), (uint32_t)col.off_full | ((uint32_t)col.off_key << 16), (uint32_t)col.key_index});
      const bool arr = (what & ETLG_FINISH_ARRAYS) && col.type_class == ETLG_TC_ARRAY && fin_elem_ok(elem);
      const bool flt = (what & ETLG_FINISH_FLOATS) && (col.type_class == ETLG_TC_F32 || col.type_class == ETLG_TC_F64);
      if (arr || flt) { t.fin.push_back(k); r.n_fin++; t.any_arrays |= arr; }
      k++;
    }
    t.maxfin = std::max(t.maxfin, r.n_fin);
  }
  return t;
}

// k_size_hints over every event of a ready batch with at least one event, enqueued on the context's stream: the slot / column tables go
// up into a scratch block taken here, with `extra` bytes behind them (*extra_at); the hints go to `out` (device memory), or `hints_off`
// bytes into `extra` when out is null.
static int32_t size_hints_enqueue(etlg_ctx* c, etlg_batch* b, const etlg_size_model* m, ScratchBlk& dblk, size_t extra, size_t hints_off, unsigned long long* out,
                                  uint8_t** extra_at) {
  const etlg_batch_view& bv = b->v;
  const uint64_t ne = bv.n_events;
  hipStream_t s = c->stream;
  const uint32_t ns = (uint32_t)c->slots.size();
  const SlotTable t = slot_table(c, ns, 0u);
  const size_t slot_bytes = t.slots.size() * sizeof(HintSlotRec), col_bytes = t.cols.size() * sizeof(HintColRec);
  std::vector<uint8_t> tab(slot_bytes + col_bytes + 1);   // the slots, then the columns, in k_size_hints' narrower records: one upload
  HintSlotRec* hs = (HintSlotRec*)tab.data(); HintColRec* hc = (HintColRec*)(tab.data() + slot_bytes);
  for (const SlotRec& r : t.slots) *hs++ = HintSlotRec{r.n_cols, r.n_ident, r.row_full, r.row_key, r.cols_base};
  for (const ColRec& r : t.cols) *hc++ = HintColRec{r.cls() | (r.identity() ? 1u << 8 : 0u) | (r.off_full() << 16), r.off_key()};
  ScratchLayout lay(slot_bytes + col_bytes);
  const size_t o_extra = lay.skip(extra + 64);
  HIPCHK(c, blk_take(c, lay.total(), false, &dblk.p, &dblk.cap));
  uint8_t* d = (uint8_t*)dblk.p;
  *extra_at = d + o_extra;
  HIPCHK(c, hipMemcpyAsync(d, tab.data(), slot_bytes + col_bytes, hipMemcpyHostToDevice, s));
  HintJob j{};
  j.ev_kind = bv.ev_kind; j.ev_flags = bv.ev_flags; j.ev_table = bv.ev_table_id; j.ev_slot = bv.ev_schema_slot; j.ev_body = bv.ev_body_off;
  j.fixed = bv.fixed; j.heap = bv.heap; j.n_events = ne;
  j.slots = (const HintSlotRec*)d; j.cols = (const HintColRec*)(d + slot_bytes); j.n_slots = ns;
  j.m_begin = m->begin_event; j.m_commit = m->commit_event; j.m_insert = m->insert_event; j.m_update = m->update_event; j.m_delete = m->delete_event;
  j.m_truncate = m->truncate_event; j.m_relation = m->relation_event; j.m_rts = m->replicated_table_schema; j.m_row = m->table_row; j.m_cell = m->cell;
  j.out = out ? out : (unsigned long long*)(*extra_at + hints_off);
  etlg_k_size_hints(&j, s);
  return ETLG_OK;
}

int32_t etlg_batch_size_hints(etlg_ctx* c, etlg_batch* b, const etlg_size_model* m, uint32_t flags, uint64_t* out) {
  if (!c || !b || !m || b->ctx != c) return ETLG_InvalidArgument;
  if (const int32_t rc = batch_ready(c, b, "etlg_batch_size_hints" NEEDS_DEVICE)) return rc;
  const uint64_t ne = b->v.n_events;
  if (!ne) return ETLG_OK;
  if (!out) return ETLG_InvalidArgument;
  hipStream_t s = c->stream;
  const bool on_dev = (flags & ETLG_F_OUTPUT_ON_DEVICE) != 0;
  ScratchBlk dblk{c};
  uint8_t* staged = nullptr;
  RC(size_hints_enqueue(c, b, m, dblk, on_dev ? 0 : ne * 8, 0, on_dev ? (unsigned long long*)out : nullptr, &staged));
  if (!on_dev) HIPCHK(c, hipMemcpyAsync(out, staged, ne * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));   // the tables are freed on return
  return ETLG_OK;
}

// write_events cut points (include/etlg.h; k_cut_* in finish.hip). Two stops for the device: the first learns L = stop_event - first
// and total, from which the host bounds the cuts — every closed batch sums to at least `budget` — and with the bound sizes the jump
// levels and the launch that writes the cuts; the second brings the counts (and the cuts, for a host caller). A range that cannot hold a
// cut ends at the first stop.
int32_t etlg_batch_cuts(etlg_ctx* c, etlg_batch* b, const etlg_size_model* m, const uint64_t* hints, uint64_t first, uint64_t end, uint64_t budget,
                        uint64_t carry_in, uint32_t flags, uint64_t* cuts_out, uint64_t cuts_cap, etlg_cuts_info* info) {
  if (!c || !b || b->ctx != c || !info) return ETLG_InvalidArgument;
  *info = etlg_cuts_info{};
  if (!m && !hints) return lib_error(c, ETLG_InvalidArgument, "etlg_batch_cuts: without `hints` the library evaluates them and needs the size model");
  if (budget < 1 || budget > (1ull << 62) || carry_in >= budget) return lib_error(c, ETLG_InvalidArgument, "etlg_batch_cuts: budget in [1, 2^62] and carry_in < budget");
  if (cuts_cap && !cuts_out) return lib_error(c, ETLG_InvalidArgument, "etlg_batch_cuts: cuts_cap without cuts_out");
  if (const int32_t rc = batch_ready(c, b, "etlg_batch_cuts" NEEDS_DEVICE)) return rc;
  const uint64_t ne = b->v.n_events;
  if (first > end || end > ne) return lib_error(c, ETLG_InvalidArgument, "etlg_batch_cuts: first <= end <= n_events");
  const uint64_t n = end - first;
  if (n >= 0xFFFFFFF0ull) return lib_error(c, ETLG_InvalidArgument, "etlg_batch_cuts: the range is beyond what one call cuts (32-bit jump tables)");
  info->stop_event = first; info->carry_out = carry_in;
  if (!n) return ETLG_OK;
  hipStream_t s = c->stream;
  const bool on_dev = (flags & ETLG_F_OUTPUT_ON_DEVICE) != 0;
  uint64_t tile = c->cuts_tile_test ? c->cuts_tile_test : 2048u;
  while ((n + tile - 1) / tile > (1ull << 30)) tile *= 2;   // (a grid's width; only a test's tile gets here)
  const uint64_t n_tiles = (n + tile - 1) / tile;
  const CutsLayout lay = cuts_layout(n, n_tiles, ne, !hints);
  ScratchBlk ablk{c};
  uint8_t* d = nullptr;
  if (hints) { HIPCHK(c, blk_take(c, lay.total + 64, false, &ablk.p, &ablk.cap)); d = (uint8_t*)ablk.p; }
  else RC(size_hints_enqueue(c, b, m, ablk, lay.total, lay.hints, nullptr, &d));   // k_size_hints, as etlg_batch_size_hints launches it
  CutJob j{};
  j.first = first; j.n = n; j.budget = budget; j.carry_in = carry_in; j.tile = (uint32_t)tile; j.n_tiles = (uint32_t)n_tiles;
  j.hdr = (unsigned long long*)(d + lay.hdr); j.tsum = (unsigned long long*)(d + lay.tsum); j.tinc = (unsigned long long*)(d + lay.tinc); j.q = (unsigned long long*)(d + lay.q);
  j.hints = hints ? (const unsigned long long*)hints : (const unsigned long long*)(d + lay.hints);
  etlg_k_cuts(&j, 0, 0, s);
  uint64_t head[2] = {0, 0};
  HIPCHK(c, hipMemcpyAsync(head, j.hdr, sizeof head, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));   // stop 1: L and total
  const uint64_t L = head[0], total = head[1];
  info->stop_event = first + L; info->total = total; info->carry_out = carry_in + total;
  const uint64_t by_sum = (carry_in + total) / budget, max_cuts = by_sum < L ? by_sum : L;
  if (!max_cuts) return ETLG_OK;
  uint32_t levels = 0;
  while ((max_cuts >> levels) != 0) levels++;   // 2^levels > max_cuts >= n_cuts
  const uint64_t emit = cuts_cap < max_cuts ? cuts_cap : max_cuts;
  ScratchLayout jlay((size_t)levels * (L + 2) * 4);   // the jump levels | the cuts of a host caller
  const size_t o_cuts = jlay.take(on_dev ? 0 : emit * 8);
  ScratchBlk jblk{c};
  HIPCHK(c, blk_take(c, jlay.total() + 64, false, &jblk.p, &jblk.cap));
  j.jump = (uint32_t*)jblk.p; j.L = L; j.levels = levels; j.cuts_cap = emit;
  j.cuts = on_dev ? (unsigned long long*)cuts_out : (unsigned long long*)((uint8_t*)jblk.p + o_cuts);
  etlg_k_cuts(&j, 1, emit, s);
  uint64_t tail[2] = {0, 0};   // n_cuts, carry_out
  HIPCHK(c, hipMemcpyAsync(tail, j.hdr + 2, sizeof tail, hipMemcpyDeviceToHost, s));
  std::vector<uint64_t> back;
  if (!on_dev && emit) { back.resize(emit); HIPCHK(c, hipMemcpyAsync(back.data(), j.cuts, emit * 8, hipMemcpyDeviceToHost, s)); }
  HIPCHK(c, hipStreamSynchronize(s));   // stop 2
  info->n_cuts = tail[0]; info->carry_out = tail[1];
  if (!on_dev && emit) memcpy(cuts_out, back.data(), (size_t)(tail[0] < emit ? tail[0] : emit) * 8);
  return ETLG_OK;
}

int32_t etlg_cuts_locate(etlg_ctx* c, const uint64_t* cuts, uint64_t n_cuts, uint32_t cuts_on_device, const uint64_t* row_event, uint64_t n_rows,
                         uint32_t flags, uint64_t* rows_out) {
  if (!c) return ETLG_InvalidArgument;
  if (!n_cuts) return ETLG_OK;
  if (!cuts || !rows_out || (n_rows && !row_event)) return lib_error(c, ETLG_InvalidArgument, "etlg_cuts_locate: null cuts, rows_out or row_event");
  hipStream_t s = c->stream;
  const bool on_dev = (flags & ETLG_F_OUTPUT_ON_DEVICE) != 0;
  ScratchBlk dblk{c};
  ScratchLayout lay(cuts_on_device ? 0 : n_cuts * 8);   // a host caller's cuts | a host caller's output
  const size_t o_out = lay.take(on_dev ? 0 : n_cuts * 8);
  uint8_t* d = nullptr;
  if (!cuts_on_device || !on_dev) { HIPCHK(c, blk_take(c, lay.total() + 64, false, &dblk.p, &dblk.cap)); d = (uint8_t*)dblk.p; }
  if (!cuts_on_device) HIPCHK(c, hipMemcpyAsync(d, cuts, n_cuts * 8, hipMemcpyHostToDevice, s));
  unsigned long long* out_d = on_dev ? (unsigned long long*)rows_out : (unsigned long long*)(d + o_out);
  etlg_k_cuts_locate(cuts_on_device ? (const unsigned long long*)cuts : (const unsigned long long*)d, n_cuts, (const unsigned long long*)row_event, n_rows, out_d, s);
  if (!on_dev) HIPCHK(c, hipMemcpyAsync(rows_out, out_d, n_cuts * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));   // the one stop (a device caller's too: the uploaded cuts are freed on return)
  return ETLG_OK;
}

// Source payload accounting (include/etlg.h; k_payf_* in kernels.hip, k_paye_* in finish.hip). Everything is sized from what the host
// knows — the frame and event counts of the view, the cuts' count — and the device's own counts (ordinal-taking frames, Begins) stay on
// the device, so the launches go out in one piece and the call stops once, for the header, the histogram and a host caller's outputs.
// The frame side starts from k_classify (classify_begin, as etlg_frame_tags): a frame whose offsets do not lie inside [0, len) is
// FT_BAD there and no later kernel looks at its bytes.
int32_t etlg_batch_payload(etlg_ctx* c, etlg_batch* b, const uint8_t* buf, size_t len, const uint32_t* frame_offsets, size_t nframes, const uint64_t* cuts,
                           uint64_t n_cuts, uint32_t cuts_on_device, const uint64_t* hist_bounds, uint32_t n_bounds, uint32_t flags, uint32_t* ev_bytes_out,
                           etlg_payload_sums* sums_out, uint64_t* hist_out, etlg_payload_info* info) {
  (void)flush_deferred(c);
  if (!c || !b || b->ctx != c || !info) return ETLG_InvalidArgument;
  clear_error(c);
  *info = etlg_payload_info{};
  info->n_ranges = n_cuts + 1; info->mismatch_event = ~0ull;
  if (b->pending) (void)etlg_batch_sync(c, b);   // (a batch that ended in a decode error is accepted: its events were delivered)
  if (!b->finished || !b->v.on_device || !b->dev) return lib_error(c, ETLG_InvalidArgument, "etlg_batch_payload needs a finished, device-resident batch (ETLG_F_OUTPUT_ON_DEVICE, not downloaded)");
  const etlg_batch_view& bv = b->v;
  const uint64_t ne = bv.n_events, nf = bv.n_frames;
  if (!frame_offsets) return lib_error(c, ETLG_InvalidArgument, "etlg_batch_payload: frame_offsets is required (etlg_scan_boundaries returns them for an input without a sidecar)");
  if (nframes < nf) return lib_error(c, ETLG_InvalidArgument, "etlg_batch_payload: fewer frames than the batch consumed");
  if (n_bounds > kPayBuckets - 1 || (n_bounds && !hist_bounds)) return lib_error(c, ETLG_InvalidArgument, "etlg_batch_payload: at most 64 histogram bounds");
  for (uint32_t i = 1; i < n_bounds; i++)
    if (hist_bounds[i] <= hist_bounds[i - 1]) return lib_error(c, ETLG_InvalidArgument, "etlg_batch_payload: histogram bounds must be strictly ascending");
  if ((n_cuts && !cuts) || n_cuts >= (1ull << 40)) return lib_error(c, ETLG_InvalidArgument, "etlg_batch_payload: cuts must be ascending and none above n_events");
  if (!cuts_on_device)
    for (uint64_t k = 0; k < n_cuts; k++)
      if (cuts[k] > ne || (k && cuts[k] < cuts[k - 1])) return lib_error(c, ETLG_InvalidArgument, "etlg_batch_payload: cuts must be ascending and none above n_events");
  RC(batch_too_large(c, len, nframes));
  const bool out_dev = (flags & ETLG_F_OUTPUT_ON_DEVICE) != 0, copy = b->copy.active, want_sums = sums_out != nullptr;
  const uint32_t n_hist = 4 * (n_bounds + 1);
  // the failing frame had recorded its metrics when the error came after the transaction-state check (k_finalize, kernels.hip: `at_err`)
  const uint64_t n_recv = nf + (!copy && nf < nframes && b->err_rank != 0xFF && b->err_rank >= RK_SCHEMA ? 1 : 0);
  hipStream_t s = c->stream;
  PayJob j{};
  if (copy) {
    HIPCHK(c, hipSetDevice(c->device));
    RC(drain_pending(c));
    j.in = buf; j.offs = frame_offsets;
    if (!(flags & ETLG_F_INPUT_ON_DEVICE)) { RC(upload_input(c, buf, 0, frame_offsets, nframes)); j.offs = (const uint32_t*)c->d_offs.p; }   // (the rows' bytes are not read)
  } else if (nframes) {
    DecParams p;
    RC(classify_begin(c, buf, len, frame_offsets, nframes, flags, p));   // k_classify: envelope + tag of every frame
    j.in = p.in; j.offs = p.offs; j.f_tag = p.f_tag;
  }
  j.in_len = len; j.n_frames = (uint32_t)nf; j.n_recv = (uint32_t)n_recv; j.copy = copy ? 1u : 0u;
  uint64_t tile = c->pay_tile_test ? c->pay_tile_test : 256u, etile = c->pay_tile_test ? c->pay_tile_test : 2048u;
  while ((n_recv + tile - 1) / tile > (1ull << 30)) tile *= 2;   // (a grid's width; only a test's tile gets here)
  while ((ne + etile - 1) / etile > (1ull << 30)) etile *= 2;
  j.tile = (uint32_t)tile; j.n_tiles = (uint32_t)((n_recv + tile - 1) / tile); j.etile = (uint32_t)etile; j.n_etiles = (uint32_t)((ne + etile - 1) / etile);
  j.n_bounds = n_bounds; j.n_events = ne; j.entry_ord = b->entry_ord; j.n_cuts = n_cuts;
  j.ev_kind = bv.ev_kind; j.ev_ord = (const unsigned long long*)bv.ev_tx_ordinal;
  const uint64_t n_ranges = n_cuts + 1;
  const bool evb_here = !(out_dev && ev_bytes_out);
  const PayLayout lay = payload_layout(PAY_H_WORDS, n_hist, n_recv, nf, ne, j.n_tiles, j.n_etiles, n_cuts, evb_here, want_sums, !cuts_on_device, !out_dev);
  const size_t o_hist = lay.hist, o_bounds = lay.bounds;
  ScratchBlk blk{c};
  HIPCHK(c, blk_take(c, lay.total + 64, false, &blk.p, &blk.cap));
  uint8_t* d = (uint8_t*)blk.p;
  j.hdr = (unsigned long long*)(d + lay.hdr); j.hist = (unsigned long long*)(d + o_hist); j.bounds = (const unsigned long long*)(d + o_bounds);
  j.fbytes = (uint32_t*)(d + lay.fbytes); j.tcnt = (unsigned long long*)(d + lay.tcnt); j.r2f = (uint32_t*)(d + lay.r2f); j.brank = (uint32_t*)(d + lay.brank);
  j.etb = (unsigned long long*)(d + lay.etb); j.ev_bytes = evb_here ? (uint32_t*)(d + lay.evb) : ev_bytes_out;
  if (want_sums) {
    j.tsum = (unsigned long long*)(d + lay.tsum); j.pb = (unsigned long long*)(d + lay.pb); j.pr = (uint32_t*)(d + lay.pr);
    j.cuts = cuts_on_device ? (const unsigned long long*)cuts : (const unsigned long long*)(d + lay.cuts);
    j.sums = out_dev ? (unsigned long long*)sums_out : (unsigned long long*)(d + lay.sums);
    if (!cuts_on_device && n_cuts) HIPCHK(c, hipMemcpyAsync(d + lay.cuts, cuts, n_cuts * 8, hipMemcpyHostToDevice, s));
  }
  static_assert(sizeof(etlg_payload_sums) == 64, "k_paye_ranges writes 8 words per range");
  HIPCHK(c, hipMemsetAsync(d, 0, o_bounds, s));   // the header and the histogram
  const uint64_t none = ~0ull;
  HIPCHK(c, hipMemcpyAsync(j.hdr + PAY_H_MISMATCH, &none, 8, hipMemcpyHostToDevice, s));
  if (n_bounds) HIPCHK(c, hipMemcpyAsync(d + o_bounds, hist_bounds, (size_t)n_bounds * 8, hipMemcpyHostToDevice, s));
  etlg_k_payload_frames(&j, s);
  etlg_k_payload_events(&j, s);
  std::vector<uint64_t> back((o_bounds) / 8);
  HIPCHK(c, hipMemcpyAsync(back.data(), d, o_bounds, hipMemcpyDeviceToHost, s));
  if (!out_dev && ev_bytes_out && ne) HIPCHK(c, hipMemcpyAsync(ev_bytes_out, j.ev_bytes, ne * 4, hipMemcpyDeviceToHost, s));
  if (!out_dev && want_sums) HIPCHK(c, hipMemcpyAsync(sums_out, j.sums, n_ranges * 64, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));   // the one stop
  if (back[PAY_H_BAD_CUTS]) return lib_error(c, ETLG_InvalidArgument, "etlg_batch_payload: cuts must be ascending and none above n_events");
  for (int k = 0; k < 4; k++) { info->received_bytes[k] = back[PAY_H_BYTES + k]; info->received_rows[k] = back[PAY_H_ROWS + k]; }
  info->mismatch_event = back[PAY_H_MISMATCH];
  info->status = back[PAY_H_MISMATCH] != none ? (int32_t)ETLG_PM_MISMATCH : (int32_t)ETLG_PM_OK;
  if (hist_out) memcpy(hist_out, back.data() + o_hist / 8, (size_t)n_hist * 8);
  return ETLG_OK;
}

// The finish pass (include/etlg.h): typed arrays and exact floats in the arena. Tables: one record per host slot, the columns' classes
// and offsets, and per slot the list of its FINISHABLE columns (arrays of a class the device takes apart, floats) — a thread per
// (event, row image, finishable column). Two device stops: the entry sizes' total (the heap may have to grow), then the counters.
int32_t finish_cells(etlg_ctx* c, etlg_batch* b, uint32_t what, etlg_finish_stats* stats) {
  etlg_finish_stats st{};
  if (stats) *stats = st;
  etlg_batch_view& bv = b->v;
  const uint64_t ne = bv.n_events;
  what &= ETLG_FINISH_ARRAYS | ETLG_FINISH_FLOATS;
  if (!ne || !what) return ETLG_OK;
  hipStream_t s = c->stream;
  const uint32_t ns = (uint32_t)std::min<size_t>(c->slots.size(), b->n_slots_view == ~(size_t)0 ? c->slots.size() : std::max<size_t>(b->n_slots_view, bv.n_slots));
  const SlotTable tab = slot_table(c, ns, what);
  const std::vector<uint32_t>& fin = tab.fin; const uint32_t maxfin = tab.maxfin; const bool any_arrays = tab.any_arrays;
  if (!maxfin) return ETLG_OK;
  const uint64_t n = ne * 2ull * maxfin;
  const uint32_t nb = (uint32_t)((n + 255) / 256);
  ScratchLayout lay(tab.slots.size() * sizeof(SlotRec));   // slots | columns | finishable columns | stats | with arrays: lens, counts, offsets, scan scratch
  const size_t o_cols = lay.take(tab.cols.size() * sizeof(ColRec)), o_fin = lay.take(fin.size() * 4 + 4), o_stats = lay.skip(64);
  const size_t o_lens = lay.take(any_arrays ? n * 4 : 0), o_cnts = lay.take(any_arrays ? n * 4 : 0), o_offs = lay.take(any_arrays ? (n + 1) * 8 : 0),
               o_blk = lay.take(any_arrays ? ((size_t)nb + 2) * 8 : 0);
  ScratchBlk dblk{c};
  HIPCHK(c, blk_take(c, lay.total() + 64, false, &dblk.p, &dblk.cap));
  uint8_t* d = (uint8_t*)dblk.p;
  HIPCHK(c, hipMemcpyAsync(d, tab.slots.data(), tab.slots.size() * sizeof(SlotRec), hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(d + o_cols, tab.cols.data(), tab.cols.size() * sizeof(ColRec), hipMemcpyHostToDevice, s));
  if (!fin.empty()) HIPCHK(c, hipMemcpyAsync(d + o_fin, fin.data(), fin.size() * 4, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemsetAsync(d + o_stats, 0, 64, s));
  OutSet* os = b->dev;
  FinJob j{};
  j.ev_kind = bv.ev_kind; j.ev_flags = bv.ev_flags; j.ev_slot = bv.ev_schema_slot; j.ev_body = bv.ev_body_off;
  j.fixed = (uint8_t*)os->fixed.p; j.heap = (uint8_t*)os->heap.p; j.n_events = ne;
  j.slots = (const SlotRec*)d; j.cols = (const ColRec*)(d + o_cols); j.fin = (const uint32_t*)(d + o_fin);
  j.n_slots = ns; j.maxfin = maxfin; j.what = what;
  j.stats = (unsigned long long*)(d + o_stats);
  j.heap_base = (bv.heap_bytes + 3) & ~3ull;
  uint64_t added = 0;
  if (any_arrays) {
    j.lens = (uint32_t*)(d + o_lens); j.offsets = (const int64_t*)(d + o_offs); j.counts = (uint32_t*)(d + o_cnts);
    etlg_k_finish(&j, (unsigned long long*)(d + o_blk), (int64_t*)(d + o_offs), 0, s);
    int64_t tot = 0;
    HIPCHK(c, hipMemcpyAsync(&tot, (const int64_t*)(d + o_offs) + n, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    added = (uint64_t)tot;
    if (j.heap_base + added > 0xFFFFFFF0ull) return lib_error(c, ETLG_InvalidArgument, "the typed arrays would take the batch's heap beyond 4 GiB");
    if (j.heap_base + added > os->heap.cap) {   // the heap grows: a new allocation, the bytes so far moved over (every reference is an offset)
      DevBuf nh;
      HIPCHK(c, nh.ensure(j.heap_base + added + 64));
      if (bv.heap_bytes) HIPCHK(c, hipMemcpyAsync(nh.p, os->heap.p, bv.heap_bytes, hipMemcpyDeviceToDevice, s));
      HIPCHK(c, hipStreamSynchronize(s));
      os->heap.release();
      os->heap = nh;
      j.heap = (uint8_t*)os->heap.p;
      bv.heap = (const uint8_t*)os->heap.p;
    }
  }
  etlg_k_finish(&j, nullptr, nullptr, 1, s);
  unsigned long long hst[8] = {0};
  HIPCHK(c, hipMemcpyAsync(hst, d + o_stats, 64, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  if (added) {
    bv.heap_bytes = j.heap_base + added;
    if (b->d_res_blk) {   // (the header a shard sends to its peers, etlg_batch_header_to_device, is read from the device block)
      const uint64_t hb = bv.heap_bytes;
      HIPCHK(c, hipMemcpy((uint8_t*)b->d_res_blk + offsetof(DevResult, heap_bytes), &hb, 8, hipMemcpyHostToDevice));
    }
  }
  st.deferred_seen = hst[0]; st.arrays_typed = hst[1]; st.floats_settled = hst[2]; st.left_deferred = hst[3];
  st.heap_bytes_added = added;
  if (stats) *stats = st;
  return ETLG_OK;
}

int32_t etlg_batch_finish_cells(etlg_ctx* c, etlg_batch* b, uint32_t what, etlg_finish_stats* stats) {
  if (!c || !b || b->ctx != c) return ETLG_InvalidArgument;
  if (const int32_t rc = batch_ready(c, b, "etlg_batch_finish_cells" NEEDS_DEVICE)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return finish_cells(c, b, what, stats);
}

int32_t etlg_columns_view_get(const etlg_columns* cs, etlg_columns_view* out) {
  if (!cs || !out) return ETLG_InvalidArgument;
  *out = cs->v;
  return ETLG_OK;
}

void etlg_columns_free(etlg_columns* cs) {
  if (!cs) return;
  handoff_release(cs->m);
  delete cs;
}

struct NdKeys { std::vector<uint32_t> off; std::string bytes; };   // FMT_NDJSON: the escaped `"name":` of every column, back to back
// n NUL-separated names, each as '"' + its characters through esc(bytes, ch) + close; off: where every key begins, and the end
static NdKeys quoted_names(const char* names, uint32_t n, const char* close, void (*esc)(std::string&, unsigned char)) {
  NdKeys k;
  const char* p = names;
  for (uint32_t i = 0; i < n; i++) {
    k.off.push_back((uint32_t)k.bytes.size());
    k.bytes.push_back('"');
    for (; *p; p++) esc(k.bytes, (unsigned char)*p);
    p++;
    k.bytes += close;
  }
  k.off.push_back((uint32_t)k.bytes.size());
  return k;
}
static int32_t handoff_rows(etlg_ctx* c, etlg_batch* b, int32_t slot, const uint8_t* nullable_flags, uint32_t n_flags, int32_t engine,
                            uint32_t flags, uint32_t format, etlg_rowbinary** out, const NdKeys* nd = nullptr, uint32_t dl_what = 0u);

int32_t etlg_batch_rowbinary(etlg_ctx* c, etlg_batch* b, int32_t slot, const uint8_t* nullable_flags, uint32_t n_flags, int32_t engine,
                             uint32_t flags, etlg_rowbinary** out) {
  if (!c || !b || !out || b->ctx != c || !nullable_flags) return ETLG_InvalidArgument;
  return handoff_rows(c, b, slot, nullable_flags, n_flags, engine, flags, FMT_ROWBINARY, out);
}

int32_t etlg_batch_protobuf(etlg_ctx* c, etlg_batch* b, int32_t slot, uint32_t flags, etlg_rowbinary** out) {
  if (!c || !b || !out || b->ctx != c) return ETLG_InvalidArgument;
  return handoff_rows(c, b, slot, nullptr, 0u, ETLG_CH_MERGE_TREE, flags, FMT_PROTOBUF, out);
}

// Snowflake NDJSON (snowflake/encoding.rs:57-72): the column names are escaped here once — serde_json's table (format_escaped_str) — and
// go up with the column words as the `"name":` keys of nd_row.
int32_t etlg_batch_ndjson(etlg_ctx* c, etlg_batch* b, int32_t slot, const char* col_names, uint32_t n_names, uint32_t flags, etlg_rowbinary** out) {
  if (!c || !b || !out || b->ctx != c || (n_names && !col_names)) return ETLG_InvalidArgument;
  *out = nullptr;
  if (!slot_known(c, slot)) return lib_error(c, ETLG_InvalidArgument, "unknown schema slot");
  if (n_names != c->slots[(size_t)slot]->desc.n_cols) return lib_error(c, ETLG_InvalidArgument, "Snowflake row width mismatch: one column name per replicated column");
  const NdKeys k = quoted_names(col_names, n_names, "\":", [](std::string& o, unsigned char ch) {
    static const char hexd[] = "0123456789abcdef";
    if (ch == '"' || ch == '\\') { o.push_back('\\'); o.push_back((char)ch); }
    else if (ch == 8) o += "\\b";
    else if (ch == 12) o += "\\f";
    else if (ch == '\n') o += "\\n";
    else if (ch == '\r') o += "\\r";
    else if (ch == '\t') o += "\\t";
    else if (ch < 0x20) { o += "\\u00"; o.push_back(hexd[ch >> 4]); o.push_back(hexd[ch & 15]); }
    else o.push_back((char)ch);
  });
  return handoff_rows(c, b, slot, nullptr, 0u, ETLG_CH_MERGE_TREE, flags & ETLG_F_OUTPUT_ON_DEVICE, FMT_NDJSON, out, &k);
}

// DuckLake SQL literals (ducklake/encoding.rs:366-612, batches.rs:1229-1316): the column names are quoted here once, as
// quote_double_identifier does (ducklake/sql.rs:10-12: '"' doubled, nothing else changed), and go up with the column words like the
// NDJSON keys; dl_row puts ` = <literal>` / ` IS NULL` behind them.
int32_t etlg_batch_duckdb(etlg_ctx* c, etlg_batch* b, int32_t slot, int32_t what, const char* col_names, uint32_t n_names, uint32_t flags,
                          etlg_rowbinary** out) {
  if (!c || !b || !out || b->ctx != c || (n_names && !col_names)) return ETLG_InvalidArgument;
  *out = nullptr;
  if ((uint32_t)what != ETLG_DL_TUPLES && (uint32_t)what != ETLG_DL_PREDICATES && (uint32_t)what != ETLG_DL_UPDATES) return lib_error(c, ETLG_InvalidArgument, "etlg_batch_duckdb: what must be ETLG_DL_TUPLES, ETLG_DL_PREDICATES or ETLG_DL_UPDATES");
  if (!slot_known(c, slot)) return lib_error(c, ETLG_InvalidArgument, "unknown schema slot");
  if (n_names != c->slots[(size_t)slot]->desc.n_cols) return lib_error(c, ETLG_InvalidArgument, "DuckLake row width mismatch: one column name per replicated column");
  const NdKeys k = quoted_names(col_names, n_names, "\"", [](std::string& o, unsigned char ch) { if (ch == '"') o.push_back('"'); o.push_back((char)ch); });
  return handoff_rows(c, b, slot, nullptr, 0u, ETLG_CH_MERGE_TREE, flags & ETLG_F_OUTPUT_ON_DEVICE, FMT_DUCKLAKE, out, &k, (uint32_t)what);
}

// ColSel.dl of an etlg_batch_duckdb call, and through dl_row_what RbJob.dl_what (a copied row's predicate is over the primary key: delete_predicate_from_copy_row)
static uint32_t dl_selection(uint32_t what, bool copy) {
  return what == ETLG_DL_UPDATES ? DL_SEL_UPDATES : what == ETLG_DL_TUPLES ? DL_SEL_TUPLES : copy ? DL_SEL_PRED_PK : DL_SEL_PRED_IDENT;
}
// format (FMT_*): ClickHouse RowBinary (Insert / Update / Delete rows + the engine's CDC columns), BigQuery protobuf, Snowflake NDJSON,
// DuckLake SQL literals (dl_what: ETLG_DL_TUPLES / ETLG_DL_PREDICATES / ETLG_DL_UPDATES)
static int32_t handoff_rows(etlg_ctx* c, etlg_batch* b, int32_t slot, const uint8_t* nullable_flags, uint32_t n_flags, int32_t engine,
                            uint32_t flags, uint32_t format, etlg_rowbinary** out, const NdKeys* nd, uint32_t dl_what) {
  *out = nullptr;
  if (const int32_t rc = batch_ready(c, b, "etlg_batch_rowbinary" NEEDS_DEVICE)) return rc;   // (the message names this entry point for all four formats)
  if (!slot_known(c, slot) || (engine != ETLG_CH_MERGE_TREE && engine != ETLG_CH_REPLACING_MERGE_TREE)) return ETLG_InvalidArgument;
  const SlotHost& sh = *c->slots[(size_t)slot];
  const uint32_t nc = sh.desc.n_cols;
  if (format == FMT_ROWBINARY && n_flags != nc + 2) return lib_error(c, ETLG_ConversionError, "ClickHouse RowBinary row width mismatch");
  std::unique_ptr<etlg_rowbinary, void (*)(etlg_rowbinary*)> rb(new etlg_rowbinary, etlg_rowbinary_free);
  const bool on_dev = (flags & ETLG_F_OUTPUT_ON_DEVICE) != 0;
  rb->v.on_device = on_dev ? 1u : 0u; rb->v.host_event = ~0ull;
  const uint32_t dl = format == FMT_DUCKLAKE ? dl_selection(dl_what, b->copy.active) : (uint32_t)DL_SEL_NONE;
  const bool dl_upd = dl == DL_SEL_UPDATES;   // partial Updates: two records per event and the col_ends array
  rb->updates = dl_upd;
  if (format == FMT_DUCKLAKE) { rb->dl_batch = b; rb->dl_serial = b->serial; rb->dl_slot = slot; rb->dl_what = dl_what; }
  std::vector<uint32_t> cols(2 * (size_t)nc);   // [nc, 2 nc): the key-layout words of the columns (RbJob.kcols)
  // A Delete that carries only the key: the reference expands it into a tombstone row (expand_key_row, clickhouse/core.rs:1437-1472)
  // when the replica identity is the primary key (or Full) — ensure_clickhouse_key_identity_is_primary_key, :1404-1427; identity
  // columns are then exactly the primary-key columns, so the key image has the right width (:1438-1450). The device builds that row
  // unless a nullable non-key column has a type outside the value codec's table (a String cell): is_array_type (type_utils.rs:14-18)
  // decides between NULL and an empty array there, and only the host knows every array type — those slots' key-only Deletes stay
  // with the host, like every slot's under another identity (the host raises the reference's SourceReplicaIdentityError).
  bool key_ok = format == FMT_ROWBINARY && (sh.identity_type == 1 || sh.identity_type == 2) && sh.desc.n_ident != 0;
  bool pk_comparable = true;
  for (uint32_t i = 0; i < nc; i++) {
    const etlg_slot_col& sc = sh.cols[i];
    const uint32_t oid = sc.type_oid;
    if (!sc.identity && sc.nullable && sc.type_class == ETLG_TC_STRING && !(oid == 25 || oid == 1043 || oid == 1042 || oid == 19 || oid == 18)) key_ok = false;
    cols[nc + i] = (sc.identity ? 1u : 0u) | (sc.nullable ? 2u : 0u) | (sh.pk[i] ? 4u : 0u) | (((uint32_t)sc.key_index & 0xFFu) << 8) | ((uint32_t)sc.off_key << 16);
    // BigQuery compares the old and the new primary key of an update as Cells (bigquery_primary_key_changed, bigquery/core.rs:1557-1645):
    // the device does that where Cell equality is equality of the arena's words / bytes (not floats: NaN != NaN, 0.0 == -0.0; not
    // numeric / timetz / json / arrays, whose cells are compared as parsed values)
    if (sh.pk[i]) { const uint32_t k = sc.type_class; if (k == ETLG_TC_F32 || k == ETLG_TC_F64 || k == ETLG_TC_NUMERIC || k == ETLG_TC_TIMETZ || k == ETLG_TC_JSON || k == ETLG_TC_ARRAY) pk_comparable = false; }
  }
  for (uint32_t i = 0; i < nc; i++) {
    const uint32_t cls = sh.cols[i].type_class;
    uint32_t elem = 0;
    bool host_class = col_plan(cls).kind == ETLG_AK_TEXT_FORM && cls != ETLG_TC_JSON;   // numeric / timetz / json Display strings are formatted on the device (json: rb_json; a cell beyond json_display's limits is reported as host_event / host_column)
    if (cls == ETLG_TC_ARRAY) {  // arrays of fixed-width elements are encoded on the device (Array(Nullable(T)); BigQuery: packed / repeated fields behind the NULL-element rule)
      elem = (uint32_t)etlg_array_elem_class(sh.cols[i].type_oid);
      const ColPlan lp = list_plan(elem);
      host_class = lp.kind != ETLG_AK_LIST && elem != ETLG_TC_JSON;   // (text-like / numeric / timetz / bytea / json elements are written on the device too)
    }
    // (DuckLake predicates look at the key columns only: the identity columns, for a table-copy batch the primary-key ones)
    if ((dl == DL_SEL_PRED_PK && !sh.pk[i]) || (dl == DL_SEL_PRED_IDENT && !sh.cols[i].identity)) host_class = false;
    if (host_class) {
      rb->v.status = ETLG_RB_NEEDS_HOST; rb->v.host_column = i;
      *out = rb.release();
      return ETLG_OK;
    }
    cols[i] = cls | ((nullable_flags && nullable_flags[i]) ? 1u << 8 : 0u) | (elem << 9) | ((uint32_t)sh.cols[i].off_full << 16);
  }
  hipStream_t s = c->stream;
  const etlg_batch_view& bv = b->v;
  const uint64_t ne = bv.n_events;
  const uint64_t nr_cap = format != FMT_ROWBINARY ? 2 * ne : ne;   // BigQuery: an update that changes the primary key is two rows
  const uint32_t nblk = (uint32_t)((ne + 255) / 256);
  // block S (freed on return): block counts | host-row counter | error word | column words | row_base
  const size_t nd_bytes = nd ? (size_t)(nc + 1) * 4 + nd->bytes.size() : 0;   // (FMT_NDJSON / FMT_DUCKLAKE: the keys' offsets and bytes behind the column words)
  ScratchLayout s_lay((size_t)(nblk + 1) * 4);
  const size_t o_cnt = s_lay.skip(64), o_cols = s_lay.take((size_t)nc * 8 + 8 + nd_bytes), o_base = s_lay.take(nr_cap * 8);
  rb->m.ctx = c; rb->m.ctx_gen = c->gen;
  ScratchBlk sblk{c};
  HIPCHK(c, blk_take(c, s_lay.total() + 64, false, &sblk.p, &sblk.cap));
  void* d_s = sblk.p;
  uint8_t* S = (uint8_t*)d_s;
  // pinned staging: [host rows = 0 | error word = ~0 | total | pad to 64 | column words] goes up in one copy (S + o_cnt .. lies the same
  // way); [row count] and [host rows | error word | total] come back in one copy each. (From / to pageable memory every one of these
  // small copies was a stop of its own.)
  const size_t up_bytes = 64 + (size_t)nc * 8 + nd_bytes, hand_bytes = al64(up_bytes) + 64;
  if (c->h_hand_cap < hand_bytes) {
    if (c->h_hand) { HIPCHK(c, hipStreamSynchronize(s)); (void)hipHostFree(c->h_hand); c->h_hand = nullptr; c->h_hand_cap = 0; }
    HIPCHK(c, hipHostMalloc((void**)&c->h_hand, hand_bytes + 4096, hipHostMallocDefault));
    c->h_hand_cap = hand_bytes + 4096;
  }
  {
    unsigned long long* up = (unsigned long long*)c->h_hand;
    up[0] = 0ull; up[1] = ~0ull; up[2] = 0ull;
    if (nc) memcpy(c->h_hand + 64, cols.data(), (size_t)nc * 8);
    if (nd) {
      memcpy(c->h_hand + 64 + (size_t)nc * 8, nd->off.data(), (size_t)(nc + 1) * 4);
      if (!nd->bytes.empty()) memcpy(c->h_hand + 64 + (size_t)nc * 12 + 4, nd->bytes.data(), nd->bytes.size());
    }
    HIPCHK(c, hipMemcpyAsync(S + o_cnt, c->h_hand, up_bytes, hipMemcpyHostToDevice, s));
  }
  volatile unsigned long long* down = (volatile unsigned long long*)(c->h_hand + al64(up_bytes));   // [0] row count, [1..3] host rows, error word, total
  // block A: row_event | row_offsets | lens | scan scratch (sized for every event being a row)
  const uint32_t nblk_r = (uint32_t)((nr_cap + 255) / 256);
  ScratchLayout a_lay(nr_cap * 8);
  const size_t o_off = a_lay.take((nr_cap + 1) * 8), o_len = a_lay.take(nr_cap * 4), o_scan = a_lay.take((size_t)(nblk_r + 1) * 8);
  const size_t o_part = a_lay.skip(3 * al64(nr_cap * 4));   // (where the parts of a row begin, k_rb_rows)
  HIPCHK(c, blk_take(c, a_lay.total() + 64, false, &rb->m.d_a, &rb->m.cap_a));
  uint8_t* A = (uint8_t*)rb->m.d_a;
  uint32_t n32 = 0;
  unsigned long long cnt[2] = {0, ~0ull};
  if (ne) {
    ColSel q{};
    q.ev_kind = bv.ev_kind; q.ev_flags = bv.ev_flags; q.ev_slot = bv.ev_schema_slot; q.ev_body = bv.ev_body_off;
    // ReplacingMergeTree keys its dedup on the source primary key: the reference refuses Update events of a table whose replica
    // identity is neither PrimaryKey nor Full (clickhouse_update_row -> ensure_clickhouse_key_identity_is_primary_key,
    // clickhouse/core.rs:1359-1427). Such Updates are not encoded here: they are left to the host (n_host_rows), which raises
    // the reference's SourceReplicaIdentityError when it meets the first of them.
    const bool upd_ok = format != FMT_ROWBINARY || engine != ETLG_CH_REPLACING_MERGE_TREE || sh.identity_type == 1 || sh.identity_type == 2;
    // Snowflake: inserts, full updates, deletes with a full old row or a key image (core.rs:345-438, snowflake_update_row /
    // snowflake_delete_row :572-608); partial updates and deletes without an old row stay with the host (SourceReplicaIdentityError)
    q.n_events = ne; q.slot = (uint32_t)slot; q.kinds = format == FMT_NDJSON ? SEL_INSERT | SEL_UPDATE_NEW | SEL_DELETE_OLD | SEL_DELETE_KEY : format != FMT_ROWBINARY ? SEL_INSERT   // (pb_selected / dl_selected pick the rest)
                      : SEL_INSERT | SEL_DELETE_OLD | (upd_ok ? SEL_UPDATE_NEW : 0u) | (key_ok ? SEL_DELETE_KEY : 0u);
    q.host_rows = (unsigned long long*)(S + o_cnt);
    q.row_full = sh.desc.row_bytes_full; q.row_key = sh.desc.row_bytes_key;
    q.blk = (uint32_t*)S; q.nblocks = nblk; q.row_event = (uint64_t*)A; q.row_base = (uint64_t*)(S + o_base);
    if (format == FMT_DUCKLAKE) {  // dl_selected (ducklake/core.rs:1824-1945, batches.rs:1128-1226)
      q.dl = dl;
      q.dl_ident = sh.desc.n_ident != 0 ? 1u : 0u;
      if (dl_upd) { q.n_cols = nc; q.fixed = bv.fixed; q.kcols = (const uint32_t*)(S + o_cols) + nc; }   // (the new row's cell states, the identity bits)
    }
    if (format == FMT_PROTOBUF) {  // BigQuery: inserts, updates (one or two rows) and deletes (bigquery/core.rs:978-1036); the events the reference refuses stay with the host
      q.pb = 1; q.n_cols = nc; q.identity_pk = sh.identity_type == 1 ? 1u : 0u; q.pk_comparable = pk_comparable ? 1u : 0u;
      q.fixed = bv.fixed; q.heap = bv.heap; q.cols = (const uint32_t*)(S + o_cols); q.kcols = (const uint32_t*)(S + o_cols) + nc;
    }
    etlg_k_col_select(&q, s);
    HIPCHK(c, hipMemcpyAsync((void*)&down[0], S + (size_t)nblk * 4, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    n32 = (uint32_t)down[0];
  }
  const uint64_t n = n32;
  RbJob j{};
  j.fixed = bv.fixed; j.heap = bv.heap; j.row_event = (const uint64_t*)A; j.row_base = (const uint64_t*)(S + o_base);
  j.ev_kind = bv.ev_kind; j.ev_commit = bv.ev_commit_lsn; j.ev_ord = bv.ev_tx_ordinal;
  j.n_rows = n; j.n_cols = nc; j.engine = (uint32_t)engine;
  j.cdc_nullable = nullable_flags ? (nullable_flags[nc] ? 1u : 0u) | (nullable_flags[nc + 1] ? 2u : 0u) : 0u;
  j.format = format;
  j.copy_tail = ((format == FMT_ROWBINARY || format == FMT_PROTOBUF) && b->copy.active) ? 1u : 0u;   // a table-copy batch: write_table_rows' rows (clickhouse/core.rs:739-773, bigquery/core.rs:602-649)
  j.cols = (const uint32_t*)(S + o_cols); j.kcols = (key_ok || format != FMT_ROWBINARY) ? (const uint32_t*)(S + o_cols) + nc : nullptr; j.ev_flags = bv.ev_flags; j.lens = (uint32_t*)(A + o_len); j.offsets = (const int64_t*)(A + o_off);
  j.err = (unsigned long long*)(S + o_cnt) + 1;
  for (uint32_t i = 0; i < nc; i++) if (sh.cols[i].type_class == ETLG_TC_JSON || (sh.cols[i].type_class == ETLG_TC_ARRAY && (uint32_t)etlg_array_elem_class(sh.cols[i].type_oid) == ETLG_TC_JSON)) j.has_json = 1;
  j.qparts = nc >= 4 ? 4u : nc >= 2 ? 2u : 1u; j.parts = 1;
  j.part_off = (uint32_t*)(A + o_part);
  if (nd) {
    j.kcols = (const uint32_t*)(S + o_cols) + nc;
    j.nd_key_off = (const uint32_t*)(S + o_cols + (size_t)nc * 8); j.nd_keys = S + o_cols + (size_t)nc * 12 + 4;
    j.nd_zero_token = b->copy.active ? 1u : 0u;   // a table-copy batch (etlg_copy_decode): Insert rows under OffsetToken::zero (core.rs:683-699)
    if (dl) j.dl_what = dl_row_what(dl);
    if (dl_upd && n && nc) {  // col_ends: a block of its own, sized by the rows the select pass counted (not by 2 x events x columns)
      HIPCHK(c, blk_take(c, (size_t)n * nc * 4 + 64, false, &rb->m.d_c, &rb->m.cap_c));
      j.col_ends = (uint32_t*)rb->m.d_c;
    }
  }
  int64_t total = 0;
  if (n) {
    etlg_k_rowbinary(&j, (unsigned long long*)(A + o_scan), (int64_t*)(A + o_off), (unsigned long long*)(S + o_cnt) + 2, 0, s);
  } else {
    HIPCHK(c, hipMemsetAsync(A + o_off, 0, 8, s));
  }
  HIPCHK(c, hipMemcpyAsync((void*)&down[1], S + o_cnt, 24, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  cnt[0] = down[1]; cnt[1] = down[2]; total = (int64_t)down[3];
  rb->v.n_host_rows = cnt[0];
  if (cnt[1] != ~0ull) {  // the first row (event order) with a cell that has no encoding
    const RbReport rep = rb_report_unpack(cnt[1]); const uint32_t code = rep.code, col = rep.col;
    uint64_t ev = 0;
    HIPCHK(c, hipMemcpy(&ev, A + rep.row * 8, 8, hipMemcpyDeviceToHost));
    if (code == RB_E_JSON) return set_error(c, ETLG_E_JSON, (int64_t)ev);   // a json cell that is not one JSON value: the decode error of codec/text.rs:126-134, as etlg_batch_columns reports it
    if (code == RB_E_HOST_CELL) {
      rb->v.status = ETLG_RB_NEEDS_HOST; rb->v.host_event = ev; rb->v.host_column = col;
      blk_give(c, c->gen, rb->m.d_a, rb->m.cap_a, false); blk_give(c, c->gen, rb->m.d_c, rb->m.cap_c, false); rb->m.d_a = rb->m.d_c = nullptr;
      *out = rb.release();
      return ETLG_OK;
    }
    if (code >= ND_E_FIRST && code <= ND_E_LAST) {  // Error::Encoding of the serde message (snowflake/encoding.rs:162-180, error.rs:25-26, 52)
      const int32_t k = lib_error(c, ETLG_InvalidData, "Snowflake encoding error");
      static const char* const what[ND_E_LAST - ND_E_FIRST + 1] = {"Snowflake does not support NaN/Infinity float values: NaN", "Snowflake does not support NaN/Infinity float values: inf",
          "Snowflake does not support NaN/Infinity float values: -inf", "Snowflake NUMBER does not support NaN", "Snowflake NUMBER does not support Infinity"};   // ND_E_FLOAT_NAN, _FLOAT_INF, _FLOAT_NINF, _NUM_NAN, _NUM_INF
      c->err_detail = std::string("Encoding error: ") + what[code - ND_E_FIRST];
      c->err.detail = c->err_detail.c_str();
      c->err.frame_index = (int64_t)ev;
      return k;
    }
    if (code == RB_E_BQ_NUMERIC_SCALE || code == RB_E_BQ_ARRAY_NULL) {  // BigQueryTableRow::try_from_tagged_cells (bigquery/encoding.rs:37-45) around validate_numeric_for_bigquery (validation.rs:20-35) / reject_nulls (:127-141): the wrapper keeps the kind
      const int32_t k = lib_error(c, code == RB_E_BQ_ARRAY_NULL ? ETLG_NullValuesNotSupportedInArrayInDestination : ETLG_UnsupportedValueInDestination, "Cell validation failed for BigQuery compatibility");
      c->err_detail = "Cell at index " + std::to_string(col) + " failed validation";
      c->err.detail = c->err_detail.c_str();
      c->err.frame_index = (int64_t)ev;
      return k;
    }
    const int32_t k = lib_error(c, ETLG_ConversionError, code == RB_E_NULL ? "NULL value for non-nullable ClickHouse column" : "Date out of ClickHouse Date32 range");
    c->err.frame_index = (int64_t)ev;
    return k;
  }
  if (total) {
    HIPCHK(c, blk_take(c, (size_t)total + 64, false, &rb->m.d_b, &rb->m.cap_b));
    j.out = (uint8_t*)rb->m.d_b;
    {  // lanes per row in the byte pass (k_rb_rows): enough waves when the rows are few (~8 per SIMD), and few enough rows per
       // workgroup (256 / parts) for their bytes to fit its LDS image (32 KB)
      const uint64_t avg = (uint64_t)total / n;
      const uint32_t by_rows = n * 4 <= 8ull * 64 * 1024 ? 4u : n * 2 <= 8ull * 64 * 1024 ? 2u : 1u, by_size = avg > 220 ? 4u : avg > 110 ? 2u : 1u;   // (256 / 128 / 64 rows of the average size in 28 KB)
      j.parts = std::min(j.qparts, std::max(by_rows, by_size));
      if (c->rb_parts_test) j.parts = std::min<uint32_t>(j.qparts, c->rb_parts_test >= 4 ? 4u : c->rb_parts_test >= 2 ? 2u : 1u);
    }
    etlg_k_rowbinary(&j, nullptr, nullptr, nullptr, 1, s);
  }
  const uint8_t* base_a = A; const uint8_t* base_b = (const uint8_t*)rb->m.d_b;
  if (!on_dev) {
    const size_t ce_bytes = rb->m.d_c ? (size_t)n * nc * 4 : 0;
    HIPCHK(c, blk_take(c, o_len + al64((size_t)total) + ce_bytes + 64, true, (void**)&rb->m.h, &rb->m.cap_h));
    HIPCHK(c, hipMemcpyAsync(rb->m.h, A, o_off + (n + 1) * 8, hipMemcpyDeviceToHost, s));
    if (total) HIPCHK(c, hipMemcpyAsync(rb->m.h + o_len, rb->m.d_b, (size_t)total, hipMemcpyDeviceToHost, s));
    base_a = rb->m.h; base_b = rb->m.h + o_len;
    if (ce_bytes) HIPCHK(c, hipMemcpyAsync(rb->m.h + o_len + al64((size_t)total), rb->m.d_c, ce_bytes, hipMemcpyDeviceToHost, s));
    if (ce_bytes) rb->col_ends = (const uint32_t*)(rb->m.h + o_len + al64((size_t)total));
  } else rb->col_ends = (const uint32_t*)rb->m.d_c;
  HIPCHK(c, hipStreamSynchronize(s));   // block S is freed on return
  if (!on_dev) { blk_give(c, c->gen, rb->m.d_a, rb->m.cap_a, false); blk_give(c, c->gen, rb->m.d_b, rb->m.cap_b, false); blk_give(c, c->gen, rb->m.d_c, rb->m.cap_c, false); rb->m.d_a = rb->m.d_b = rb->m.d_c = nullptr; }
  rb->v.n_rows = n; rb->v.n_bytes = (uint64_t)total;
  rb->v.row_event = (const uint64_t*)base_a; rb->v.row_offsets = (const int64_t*)(base_a + o_off); rb->v.bytes = total ? base_b : nullptr;
  *out = rb.release();
  return ETLG_OK;
}

// DuckLake batch identities (fingerprint.hip): the three record objects of one batch and slot stay where they are, in HBM; what goes up is
// the ranges and the quoted names' lengths, what comes back the fingerprints and the first event that lacks a record — one stop, at the end.
int32_t etlg_ducklake_fingerprints(etlg_ctx* c, etlg_batch* b, int32_t slot, const etlg_rowbinary* tuples, const etlg_rowbinary* predicates,
                                   const etlg_rowbinary* updates, const char* col_names, uint32_t n_names, const etlg_dl_range* ranges,
                                   uint32_t n_ranges, uint64_t* out, etlg_dl_fp_info* info) {
  if (!c || !b || b->ctx != c || !tuples || !predicates || !info || (n_names && !col_names) || (n_ranges && (!ranges || !out))) return ETLG_InvalidArgument;
  info->status = ETLG_RB_OK; info->_pad = 0; info->host_event = ~0ull;
  if (const int32_t rc = batch_ready(c, b, "etlg_ducklake_fingerprints" NEEDS_DEVICE)) return rc;
  if (!slot_known(c, slot)) return lib_error(c, ETLG_InvalidArgument, "unknown schema slot");
  const uint32_t nc = c->slots[(size_t)slot]->desc.n_cols;
  if (n_names != nc) return lib_error(c, ETLG_InvalidArgument, "DuckLake row width mismatch: one column name per replicated column");
  auto mine = [&](const etlg_rowbinary* r, uint32_t what) { return r->dl_batch == b && r->dl_serial == b->serial && r->dl_slot == slot && r->dl_what == what && r->v.on_device && r->v.status == ETLG_RB_OK; };
  if (!mine(tuples, ETLG_DL_TUPLES) || !mine(predicates, ETLG_DL_PREDICATES) || (updates && !mine(updates, ETLG_DL_UPDATES)))
    return lib_error(c, ETLG_InvalidArgument, "etlg_ducklake_fingerprints takes the ETLG_DL_TUPLES, ETLG_DL_PREDICATES and ETLG_DL_UPDATES objects etlg_batch_duckdb built for this batch and slot, on the device (ETLG_F_OUTPUT_ON_DEVICE) and with status ETLG_RB_OK");
  const etlg_batch_view& bv = b->v;
  const uint64_t ne = bv.n_events;
  for (uint32_t i = 0; i < n_ranges; i++)
    if (ranges[i].first_event > ranges[i].end_event || ranges[i].end_event > ne || (i && ranges[i].first_event < ranges[i - 1].end_event))
      return lib_error(c, ETLG_InvalidArgument, "etlg_ducklake_fingerprints: the ranges must be [first, end) within the batch's events, ascending and disjoint");
  if (!n_ranges) return ETLG_OK;
  if (!ne) { for (uint32_t i = 0; i < n_ranges; i++) out[i] = ranges[i].seed; return ETLG_OK; }
  std::vector<uint64_t> up(3 * (size_t)n_ranges);
  for (uint32_t i = 0; i < n_ranges; i++) { up[3 * (size_t)i] = ranges[i].first_event; up[3 * (size_t)i + 1] = ranges[i].end_event; up[3 * (size_t)i + 2] = ranges[i].seed; }
  std::vector<uint32_t> name_len(nc);   // quote_double_identifier's length + " = "
  { const char* p = col_names; for (uint32_t i = 0; i < nc; i++) { uint32_t n = 2 + 3; for (; *p; p++) n += *p == '"' ? 2u : 1u; p++; name_len[i] = n; } }
  const etlg_rowbinary_view& tv = tuples->v; const etlg_rowbinary_view& pv = predicates->v;
  const uint64_t u_rows = updates ? updates->v.n_rows : 0, u_bytes = updates ? updates->v.n_bytes : 0;
  // an upper bound of the stream: every record's bytes once, and per event the LSNs, the tag and two 0xFF (a partial Update: the column
  // count and per column its index and 0xFF as well)
  const uint64_t n_max = tv.n_bytes + pv.n_bytes + u_bytes + ne * 26 + (u_rows / 2) * (8 + 9 * (uint64_t)nc);
  const uint64_t chunk = etlg_k_fp_chunk_bytes(), n_chunks = n_max / chunk + 1, n_pieces = n_chunks + n_ranges;
  if (n_chunks > 0x7FFFFFFFull) return lib_error(c, ETLG_InvalidArgument, "etlg_ducklake_fingerprints: the batch's records are beyond what one call hashes");
  ScratchLayout lay(up.size() * 8);   // the ranges first
  const size_t o_names = lay.take((size_t)nc * 4 + 4), o_plan = lay.take(ne * 16), o_lens = lay.take(ne * 4), o_offs = lay.take((ne + 1) * 8),
               o_blk = lay.take((ne / 256 + 2) * 8), o_bounds = lay.take((size_t)n_ranges * 16), o_result = lay.take(((size_t)n_ranges + 1) * 8),
               o_lin = lay.take(n_pieces), o_maps = lay.take(n_pieces * 16), o_perm = lay.take(n_pieces * 256), o_stream = lay.take(n_max);
  hipStream_t s = c->stream;
  ScratchBlk dblk{c};
  HIPCHK(c, blk_take(c, lay.total() + 64, false, &dblk.p, &dblk.cap));
  uint8_t* d = (uint8_t*)dblk.p;
  HIPCHK(c, hipMemcpyAsync(d, up.data(), up.size() * 8, hipMemcpyHostToDevice, s));
  if (nc) HIPCHK(c, hipMemcpyAsync(d + o_names, name_len.data(), (size_t)nc * 4, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemsetAsync(d + o_result, 0xFF, 8, s));
  FpJob j{};
  j.ev_kind = bv.ev_kind; j.ev_flags = bv.ev_flags; j.ev_slot = bv.ev_schema_slot; j.ev_start = bv.ev_start_lsn; j.ev_commit = bv.ev_commit_lsn;
  j.n_events = ne; j.slot = (uint32_t)slot; j.copy = b->copy.active ? 1u : 0u; j.n_cols = nc; j.n_ranges = n_ranges;
  j.t = FpRecs{tv.row_event, tv.row_offsets, tv.bytes, tv.n_rows};
  j.p = FpRecs{pv.row_event, pv.row_offsets, pv.bytes, pv.n_rows};
  if (updates) { j.u = FpRecs{updates->v.row_event, updates->v.row_offsets, updates->v.bytes, u_rows}; j.u_ends = updates->col_ends; }
  j.name_len = (const uint32_t*)(d + o_names); j.ranges = (const uint64_t*)d;
  j.plan = (uint32_t*)(d + o_plan); j.lens = (uint32_t*)(d + o_lens); j.offs = (const int64_t*)(d + o_offs); j.stream = d + o_stream;
  j.bounds = (uint64_t*)(d + o_bounds); j.perm = d + o_perm; j.lin = d + o_lin; j.maps = (uint64_t*)(d + o_maps);
  j.result = (unsigned long long*)(d + o_result); j.n_chunks = (uint32_t)n_chunks;
  etlg_k_fingerprints(&j, (unsigned long long*)(d + o_blk), s);
  std::vector<uint64_t> back((size_t)n_ranges + 1);
  HIPCHK(c, hipMemcpyAsync(back.data(), d + o_result, back.size() * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));   // the one stop; the scratch block is freed on return
  if (back[0] != ~0ull) { info->status = ETLG_RB_NEEDS_HOST; info->host_event = back[0]; return ETLG_OK; }
  memcpy(out, back.data() + 1, (size_t)n_ranges * 8);
  return ETLG_OK;
}

int32_t etlg_rowbinary_view_get(const etlg_rowbinary* rb, etlg_rowbinary_view* out) {
  if (!rb || !out) return ETLG_InvalidArgument;
  *out = rb->v;
  return ETLG_OK;
}

int32_t etlg_rowbinary_col_ends_get(const etlg_rowbinary* rb, const uint32_t** col_ends) {
  if (!rb || !col_ends || !rb->updates) return ETLG_InvalidArgument;
  *col_ends = rb->col_ends;
  return ETLG_OK;
}

void etlg_rowbinary_free(etlg_rowbinary* rb) {
  if (!rb) return;
  handoff_release(rb->m);
  delete rb;
}

