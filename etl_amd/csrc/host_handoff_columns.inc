// Part of host.cpp (included there behind host_handoff.inc, one translation unit): the Arrow columns of a decoded, device-resident batch —
// etlg_batch_columns, etlg_batch_iceberg, etlg_batch_ducklake_copy (kernels: columns.hip). The kinds and the layouts of blocks A, B and C
// are handoff_plan.h's; here are the steps that touch the device, in the order build_columns lists them.

extern "C++" {
namespace {
// pinned {0, 0, 0, ~0} records: the initial values of the columns' counters (and of the changelog's refusal words) go up as an
// asynchronous copy (a pageable source made it a synchronisation)
int32_t counter_seeds(etlg_ctx* c, size_t want) {
  bool grew = false;
  RC(pinned_grow(c, (void**)&c->h_cnt_init, &c->h_cnt_init_cols, want, want + 64, 32, &grew));
  if (grew) for (size_t i = 0; i < c->h_cnt_init_cols; i++) { c->h_cnt_init[4 * i] = c->h_cnt_init[4 * i + 1] = c->h_cnt_init[4 * i + 2] = 0ull; c->h_cnt_init[4 * i + 3] = ~0ull; }
  return ETLG_OK;
}
// the columns that travel in one launch: fn(ids, count) per pack of etlg_k_col_pack_max() columns
template <class F> void for_each_pack(const std::vector<uint32_t>& ids, F fn) {
  const uint32_t pm = etlg_k_col_pack_max();
  for (size_t k0 = 0; k0 < ids.size(); k0 += pm) fn(ids.data() + k0, (uint32_t)std::min<size_t>(pm, ids.size() - k0));
}
// A malformed array literal (or a json cell that is not one JSON value: the same report): the reference's error, for the first such row in
// event order. Every column reports the minimum of (row << 8 | code) over its own cells; across columns the order is the reference's parse
// order — row-major, then column-major (convert_tuple_to_row walks the columns of a row in order) — so the first column wins inside a
// row: a hand-back in an earlier column of the row ranks before a malformed literal in a later one. ~0: no such cell (kArrHandBack: the
// first row that is not a plain list was handed back DEFERRED, not malformed — k_arr_count)
uint64_t first_cell_error(const std::vector<ColPlan>& plans, const SlotHost& sh, const std::vector<uint64_t>& cnt) {
  uint64_t first = ~0ull;
  for (size_t i = 0; i < plans.size(); i++) if (plans[i].kind == ETLG_AK_LIST || sh.cols[i].type_class == ETLG_TC_JSON) {
    const uint64_t k = cnt[i * 4 + 3];
    if (k != ~0ull && (first == ~0ull || (k >> 8) < (first >> 8))) first = k;   // strictly earlier row; ties keep the earlier column
  }
  return first != ~0ull && (first & 0xFF) != kArrHandBack ? first : ~0ull;
}

// One build_columns call. changelog: the Iceberg sink's rows — the refused events are counted in the selection's own launches and read back
// with the row count, and the two CDC columns are written behind the data columns by one more launch (etlg_k_col_cdc), so both calls stop
// for the device equally often. dlc: a table-copy batch's rows under dlc_plan's kinds, Utf8 / Binary with int32 offsets; the same
// launches and the same stops as etlg_batch_columns(INSERT) on the slot.
struct ColumnsBuild {
  etlg_ctx* const c; etlg_batch* const b; const int32_t slot; const uint32_t sel_kinds; const bool changelog, dlc, on_dev;
  const SlotHost& sh; const etlg_batch_view& bv; const hipStream_t s; const uint32_t nc; const uint64_t ne; const uint32_t nblk;
  // Members go in reverse order: rows_blk (row_event | row_base, which every kernel up to pass 2 / block C reads) returns to the pool
  // before `cs` gives its blocks back. Which stop covers the release: a return from select_rows — its own; from read_counters onwards —
  // the stop of read_counters (first_cell_error's return follows it and a synchronous copy; the offsets refusal follows it directly);
  // a return from publish — its final stop, which also stands in front of give_device_blocks. HIPCHK returns in between follow a failed call.
  std::unique_ptr<etlg_columns, void (*)(etlg_columns*)> cs{new etlg_columns, etlg_columns_free};
  ScratchBlk rows_blk{c};
  std::vector<ColPlan> plans;
  uint32_t* d_blk = nullptr; size_t o_ice = 0;   // the select scratch: block counts, and behind them the changelog's {refused events, -, -, min(event << 8 | reason)}
  uint64_t* d_row_event = nullptr; uint64_t* d_row_base = nullptr;
  uint64_t n = 0;
  ColumnsLayoutA la; ColumnsLayoutB lb; ColumnsLayoutC lc;
  uint8_t* A = nullptr; uint8_t* B = nullptr;
  std::vector<ColJob> jobs; std::vector<uint32_t> var_ids;   // var_ids: the var-len columns that are not lists
  std::vector<int64_t> var_total, text_total; std::vector<uint64_t> cnt;

  ColumnsBuild(etlg_ctx* c_, etlg_batch* b_, int32_t slot_, uint32_t sel_kinds_, uint32_t flags, ColCaller who)
      : c(c_), b(b_), slot(slot_), sel_kinds(sel_kinds_), changelog(who == ColCaller::Iceberg), dlc(who == ColCaller::DuckLakeCopy), on_dev((flags & ETLG_F_OUTPUT_ON_DEVICE) != 0),
        sh(*c_->slots[(size_t)slot_]), bv(b_->v), s(c_->stream), nc(sh.desc.n_cols), ne(bv.n_events), nblk((uint32_t)((ne + 255) / 256)) {
    cs->m.ctx = c; cs->m.ctx_gen = c->gen;
    cs->changelog = changelog; cs->ci.host_event = ~0ull; cs->ci.n_data_cols = nc;
    cs->ducklake = dlc;
    cs->of_batch = b; cs->of_serial = b->serial; cs->of_slot = slot;
  }
  uint8_t* a_cnt() const { return A + la.cnt; }

  // nothing is built and nothing handed over: the view has no rows and no columns, `di` says why and for which column
  int32_t refuse(uint32_t status, uint32_t column, etlg_columns** out) {
    give_device_blocks(c, cs->m);
    cs->di.status = status; cs->di.column = column;
    cs->v.on_device = on_dev ? 1u : 0u;
    *out = cs.release();
    return ETLG_OK;
  }

  // ---- 1. which events are rows (count -> scan -> scatter); row_event / row_base are sized for every event
  int32_t select_scratch() {
    ScratchLayout sel_lay((size_t)(nblk + 1) * 4);
    o_ice = sel_lay.skip(64);
    HIPCHK(c, c->d_colsel.ensure(sel_lay.total()));
    d_blk = (uint32_t*)c->d_colsel.p;
    return ETLG_OK;
  }
  int32_t select_rows() {
    ScratchLayout rows_lay(ne * 8); const size_t o_row_base = rows_lay.take(ne * 8);   // row_event | row_base
    if (ne) HIPCHK(c, blk_take(c, rows_lay.total(), false, &rows_blk.p, &rows_blk.cap));
    d_row_event = (uint64_t*)rows_blk.p;
    d_row_base = (uint64_t*)((uint8_t*)rows_blk.p + o_row_base);
    if (!ne) return ETLG_OK;
    ColSel q = col_select_common(bv, sh, slot, d_blk, nblk, d_row_event, d_row_base);
    q.kinds = sel_kinds;
    unsigned long long back[(64 + 32) / 8] = {0};   // the row count; changelog: ... up to the refusal words, which ride the same copy
    const size_t back_bytes = changelog ? o_ice + 32 - (size_t)nblk * 4 : 4;
    if (changelog) {
      RC(counter_seeds(c, 1));
      q.ice = (unsigned long long*)((uint8_t*)d_blk + o_ice);
      HIPCHK(c, hipMemcpyAsync(q.ice, c->h_cnt_init, 32, hipMemcpyHostToDevice, s));
    }
    etlg_k_col_select(&q, s);
    HIPCHK(c, hipMemcpyAsync(back, d_blk + nblk, back_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    uint32_t n_rows32 = 0;
    memcpy(&n_rows32, back, 4);
    n = n_rows32;
    if (changelog) {
      unsigned long long ice[4];
      memcpy(ice, (const uint8_t*)back + (back_bytes - 32), 32);
      cs->ci.n_host_rows = ice[0];
      if (ice[3] != ~0ull) { cs->ci.host_event = ice[3] >> 8; cs->ci.host_reason = (uint32_t)(ice[3] & 0xFFu); }
    }
    return ETLG_OK;
  }

  // ---- 2. block A (columns_layout_a): the counters' initial values, row_event, the changelog's CDC columns
  int32_t block_a() {
    la = columns_layout_a(plans, n, changelog, dlc);
    HIPCHK(c, blk_take(c, la.total + 64, false, &cs->m.d_a, &cs->m.cap_a));
    A = (uint8_t*)cs->m.d_a;
    if (nc) {
      RC(counter_seeds(c, nc));
      HIPCHK(c, hipMemcpyAsync(a_cnt(), c->h_cnt_init, (size_t)nc * 32, hipMemcpyHostToDevice, s));
    }
    if (n) HIPCHK(c, hipMemcpyAsync(A, d_row_event, n * 8, hipMemcpyDeviceToDevice, s));
    if (changelog && n) {
      CdcJob cj{};
      cj.row_event = d_row_event; cj.ev_kind = bv.ev_kind; cj.ev_commit = bv.ev_commit_lsn; cj.ev_ord = bv.ev_tx_ordinal;
      cj.n_rows = n; cj.zero_token = b->copy.active ? 1u : 0u;   // a table-copy batch (etlg_copy_decode), told as etlg_batch_ndjson tells it
      cj.op_values = A + la.cdc[0].values; cj.seq_values = A + la.cdc[1].values;
      cj.op_offsets = (int64_t*)(A + la.cdc[0].offsets); cj.seq_offsets = (int64_t*)(A + la.cdc[1].offsets);
      cj.op_validity = (unsigned long long*)(A + la.cdc[0].validity); cj.seq_validity = (unsigned long long*)(A + la.cdc[1].validity);
      cj.op_deferred = (unsigned long long*)(A + la.cdc[0].deferred); cj.seq_deferred = (unsigned long long*)(A + la.cdc[1].deferred);
      etlg_k_col_cdc(&cj, s);
    } else if (changelog) {
      for (int k = 0; k < 2; k++) HIPCHK(c, hipMemsetAsync(A + la.cdc[k].offsets, 0, 8, s));
    }
    return ETLG_OK;
  }

  // ---- 3. pass 1: validity, deferred bits and values of the fixed-width columns; lengths and offsets of the var-len ones. List columns keep
  // launches of their own; every fixed-width column goes in one launch per pack, pass 1 of every other var-len column in three
  int32_t pass1() {
    jobs.assign(nc, ColJob{}); var_total.assign(nc, 0);
    std::vector<uint32_t> fixed_ids;
    auto scan_of = [&](uint32_t i) { return (unsigned long long*)(A + la.scan + la.scan_one * i); };
    for (uint32_t i = 0; i < nc; i++) {
      const ColPlan& pl = plans[i]; const ColPartsA& l = la.col[i];
      if (pl.kind == ETLG_AK_NONE) continue;
      ColJob& j = jobs[i];
      j.fixed = bv.fixed; j.heap = bv.heap; j.row_base = d_row_base; j.n_rows = n;
      j.col_index = i; j.off_full = sh.cols[i].off_full; j.cls = sh.cols[i].type_class; j.kind = pl.fmt ? pl.fmt : pl.kind;
      j.validity = (unsigned long long*)(A + l.validity); j.deferred = (unsigned long long*)(A + l.deferred);
      j.null_count = (unsigned long long*)(a_cnt() + (size_t)i * 32); j.deferred_count = j.null_count + 1;
      j.child_nulls = j.null_count + 2; j.err = j.null_count + 3; j.elem_cls = pl.elem; j.off32 = dlc ? 1u : 0u;
      if (!pl.var) { j.values = A + l.values; fixed_ids.push_back(i); continue; }
      j.lens = (uint32_t*)(A + l.lens); j.offsets = (const int64_t*)(A + l.offsets);
      if (!n) HIPCHK(c, hipMemsetAsync(A + l.offsets, 0, 8, s));
      else if (pl.kind == ETLG_AK_LIST) { j.kind = pl.child; etlg_k_col_list(&j, scan_of(i), (int64_t*)(A + l.offsets), 0, s); }
      else var_ids.push_back(i);
    }
    std::vector<ColJob> pj; std::vector<unsigned long long*> pb, pt; std::vector<int64_t*> po;
    for_each_pack(fixed_ids, [&](const uint32_t* ids, uint32_t k) {
      pj.clear();
      for (uint32_t t = 0; t < k; t++) pj.push_back(jobs[ids[t]]);
      etlg_k_col_fixed_pack(pj.data(), k, s);
    });
    for_each_pack(var_ids, [&](const uint32_t* ids, uint32_t k) {
      pj.clear(); pb.clear(); po.clear(); pt.clear();
      for (uint32_t t = 0; t < k; t++) {
        const uint32_t i = ids[t];
        pj.push_back(jobs[i]); pb.push_back(scan_of(i)); po.push_back((int64_t*)(A + la.col[i].offsets)); pt.push_back((unsigned long long*)(A + la.tot) + i);
      }
      etlg_k_col_var_pack(pj.data(), k, pb.data(), po.data(), pt.data(), 0, s);
    });
    if (n) for (uint32_t i = 0; i < nc; i++) if (plans[i].kind == ETLG_AK_LIST)
      HIPCHK(c, hipMemcpyAsync(&var_total[i], A + la.col[i].offsets + n * 8, 8, hipMemcpyDeviceToHost, s));
    return ETLG_OK;
  }

  // ---- 4. the stop behind pass 1. The counters and the var-len totals lie next to each other: one read-back for both
  int32_t read_counters() {
    const size_t tot_at = (la.tot - la.cnt) / 8;
    cnt.assign(tot_at + nc, 0);
    if (nc) HIPCHK(c, hipMemcpyAsync(cnt.data(), a_cnt(), cnt.size() * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (n) for (uint32_t i : var_ids) var_total[i] = (int64_t)cnt[tot_at + i];
    return ETLG_OK;
  }
  int32_t cell_error(uint64_t first) {   // first_cell_error's word: the code, and the row whose event the error names
    uint64_t ev = 0;
    HIPCHK(c, hipMemcpy(&ev, d_row_event + (first >> 8), 8, hipMemcpyDeviceToHost));
    return set_error(c, (int32_t)(first & 0xFF), (int64_t)ev);
  }
  // arrow-rs panics when a StringArray's / BinaryArray's bytes pass i32::MAX: the totals came back with the counters. ~0u: every column fits
  uint32_t offsets_overflow() const {
    const uint64_t cap = c->dlc_offset_cap_test ? c->dlc_offset_cap_test : 0x7FFFFFFFull;
    for (uint32_t i : var_ids) if ((uint64_t)var_total[i] > cap) return i;
    return ~0u;
  }

  // ---- 5. block B (columns_layout_b) and pass 2: list columns fill their children (lists of strings: byte length + validity of every
  // element, then their offsets), the other var-len columns copy / format their bytes, one launch per pack
  int32_t block_b_pass2() {
    lb = columns_layout_b(plans, var_total);
    if (lb.total) HIPCHK(c, blk_take(c, lb.total + 64, false, &cs->m.d_b, &cs->m.cap_b));
    B = (uint8_t*)cs->m.d_b;
    text_total.assign(nc, 0);
    std::vector<uint32_t> var2_ids;
    for (uint32_t i = 0; i < nc; i++) {
      if (!plans[i].var || var_total[i] <= 0) continue;
      const ColPartsB& l = lb.col[i]; ColJob& j = jobs[i];
      const size_t tot = (size_t)var_total[i], bits = al64((tot + 63) / 64 * 8);
      if (plans[i].kind != ETLG_AK_LIST) { j.values = B + l.values; var2_ids.push_back(i); continue; }
      j.child_validity = (uint32_t*)(B + l.child_validity);
      if (var_child(plans[i])) {
        j.values = nullptr; j.child_lens = (uint32_t*)(B + l.child_lens); j.child_offsets = (const int64_t*)(B + l.values);
        HIPCHK(c, hipMemsetAsync(B + l.child_validity, 0, bits, s));
        etlg_k_col_list(&j, nullptr, nullptr, 1, s);
        etlg_k_scan_lens(j.child_lens, (uint64_t)tot, (unsigned long long*)(B + l.child_scan), (int64_t*)(B + l.values), s);
        HIPCHK(c, hipMemcpyAsync(&text_total[i], B + l.values + tot * 8, 8, hipMemcpyDeviceToHost, s));
      } else {
        j.values = B + l.values;
        HIPCHK(c, hipMemsetAsync(B + l.values, 0, l.child_validity - l.values + bits, s));   // bitmaps are OR-ed into
        etlg_k_col_list(&j, nullptr, nullptr, 1, s);
      }
    }
    std::vector<ColJob> pj;
    for_each_pack(var2_ids, [&](const uint32_t* ids, uint32_t k) {
      pj.clear();
      for (uint32_t t = 0; t < k; t++) pj.push_back(jobs[ids[t]]);
      etlg_k_col_var_pack(pj.data(), k, nullptr, nullptr, nullptr, 1, s);
    });
    return ETLG_OK;
  }

  // ---- 6. block C (columns_layout_c): the element bytes of lists of strings, behind a stop of its own for their totals
  int32_t block_c() {
    lc.values.assign(nc, 0);
    if (!lb.any_text_list) return ETLG_OK;
    HIPCHK(c, hipStreamSynchronize(s));
    lc = columns_layout_c(plans, text_total);
    if (lc.total) HIPCHK(c, blk_take(c, lc.total + 64, false, &cs->m.d_c, &cs->m.cap_c));
    for (uint32_t i = 0; i < nc; i++)
      if (text_list(plans[i]) && var_total[i] > 0) { jobs[i].values = (uint8_t*)cs->m.d_c + lc.values[i]; etlg_k_col_list(&jobs[i], nullptr, nullptr, 1, s); }
    return ETLG_OK;
  }

  // ---- 7. the view (device pointers, or a host copy of the blocks) and the etlg_column records
  int32_t publish(etlg_columns** out) {
    if (nc) HIPCHK(c, hipMemcpyAsync(cnt.data(), a_cnt(), (size_t)nc * 32, hipMemcpyDeviceToHost, s));   // again: the child null counts
    const uint8_t* base_a = A; const uint8_t* base_b = B; const uint8_t* base_c = (const uint8_t*)cs->m.d_c;
    if (!on_dev) {
      const size_t b_at = al64(la.cnt), c_at = b_at + al64(lb.total);
      RC(host_copy(c, cs->m, s, la.cnt, b_at, lb.total, c_at, lc.total));
      base_a = cs->m.h; base_b = cs->m.h + b_at; base_c = cs->m.h + c_at;
    }
    HIPCHK(c, hipStreamSynchronize(s));   // row_base (freed on return) is read by the kernels above
    if (!on_dev) give_device_blocks(c, cs->m);
    cs->cols.assign(nc + (changelog ? 2u : 0u), etlg_column{});
    if (changelog) for (uint32_t t = 0; t < 2; t++) {
      etlg_column& k = cs->cols[nc + t];
      k.type_class = ETLG_TC_STRING; k.arrow_kind = ETLG_AK_LARGE_UTF8;
      k.validity = base_a + la.cdc[t].validity; k.deferred = base_a + la.cdc[t].deferred;
      k.offsets = (const int64_t*)(base_a + la.cdc[t].offsets); k.values = base_a + la.cdc[t].values; k.values_bytes = n * kCdcWidth[t];
    }
    for (uint32_t i = 0; i < nc; i++) {
      etlg_column& k = cs->cols[i];
      const ColPlan& pl = plans[i]; const ColPartsA& l = la.col[i];
      k.type_class = sh.cols[i].type_class; k.arrow_kind = pl.kind; k.value_bytes = pl.vbytes; k.nullable = sh.cols[i].nullable;
      if (pl.kind == ETLG_AK_NONE) continue;
      k.null_count = cnt[(size_t)i * 4]; k.deferred_count = cnt[(size_t)i * 4 + 1];
      k.validity = base_a + l.validity; k.deferred = base_a + l.deferred;
      if (pl.var) { k.offsets = (const int64_t*)(base_a + l.offsets); k.values = base_b ? base_b + lb.col[i].values : nullptr; k.values_bytes = (uint64_t)lb.col[i].values_bytes; }
      else { k.values = base_a + l.values; k.values_bytes = pl.kind == ETLG_AK_BOOLEAN ? ((n + 63) / 64) * 8 : n * pl.vbytes; }
      if (pl.kind != ETLG_AK_LIST) continue;
      k.child_kind = pl.child; k.child_count = (uint64_t)var_total[i]; k.child_null_count = cnt[(size_t)i * 4 + 2];
      k.child_validity = base_b ? base_b + lb.col[i].child_validity : nullptr;
      if (var_child(pl)) {   // element texts / bytes: offsets in block B, bytes in block C
        k.child_offsets = base_b ? (const int64_t*)(base_b + lb.col[i].values) : nullptr;
        k.values = base_c ? base_c + lc.values[i] : nullptr; k.values_bytes = (uint64_t)text_total[i];
      }
    }
    cs->v.n_rows = n; cs->v.n_cols = (uint32_t)cs->cols.size(); cs->v.on_device = on_dev ? 1u : 0u; cs->v.cols = cs->cols.data();
    cs->v.row_event = (const uint64_t*)base_a;
    *out = cs.release();
    return ETLG_OK;
  }
};
}  // namespace

// The builder behind etlg_batch_columns, etlg_batch_iceberg and etlg_batch_ducklake_copy. sel_kinds: ColSel.kinds (SEL_* bits); row_kinds: the
// caller's ETLG_ROWS_* word, of which the PARSE_ARRAYS / FORMAT_JSON bits choose kinds.
static int32_t build_columns(etlg_ctx* c, etlg_batch* b, int32_t slot, uint32_t sel_kinds, uint32_t row_kinds, uint32_t flags, ColCaller who, etlg_columns** out) {
  *out = nullptr;
  const bool dlc = who == ColCaller::DuckLakeCopy;
  if (const int32_t rc = batch_ready(c, b, dlc ? "etlg_batch_ducklake_copy" NEEDS_DEVICE : who == ColCaller::Iceberg ? "etlg_batch_iceberg" NEEDS_DEVICE : "etlg_batch_columns" NEEDS_DEVICE)) return rc;
  if (!slot_known(c, slot) || !sel_kinds) return ETLG_InvalidArgument;
  if (dlc && !b->copy.active) return lib_error(c, ETLG_InvalidArgument, "etlg_batch_ducklake_copy takes a table-copy batch (etlg_copy_decode): the sink stages copy rows only as Arrow");
  ColumnsBuild q(c, b, slot, sel_kinds, flags, who);
  uint32_t not_arrow = ~0u;
  q.plans = column_plans(q.sh, who, row_kinds, &not_arrow);
  RC(q.select_scratch());
  if (not_arrow != ~0u) return q.refuse(ETLG_DLC_NOT_ARROW, not_arrow, out);
  RC(q.select_rows());      // 1. which events are rows                       (stop)
  RC(q.block_a());          // 2. block A
  RC(q.pass1());            // 3. pass 1
  RC(q.read_counters());    // 4. counters, totals, first malformed cell       (stop)
  if (const uint64_t bad = first_cell_error(q.plans, q.sh, q.cnt); bad != ~0ull) return q.cell_error(bad);
  if (const uint32_t col = dlc ? q.offsets_overflow() : ~0u; col != ~0u) return q.refuse(ETLG_DLC_OFFSETS_OVERFLOW, col, out);
  RC(q.block_b_pass2());    // 5. block B and pass 2
  RC(q.block_c());          // 6. block C                                      (stop, with lists of strings)
  return q.publish(out);    // 7. the view                                     (stop)
}
}  // extern "C++"

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
