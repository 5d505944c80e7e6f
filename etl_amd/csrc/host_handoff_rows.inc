// Part of host.cpp (included there behind host_handoff.inc, one translation unit): the row formats of a decoded, device-resident batch —
// etlg_batch_rowbinary, etlg_batch_protobuf, etlg_batch_ndjson, etlg_batch_duckdb (kernels: rowformats.hip, rowformats_dl.hip; the
// selection: columns.hip). The column words and the lanes per row are handoff_plan.h's; here are the steps that touch the device.

extern "C++" {
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
// quote_double_identifier (ducklake/sql.rs:10-12): '"' doubled, nothing else changed
static NdKeys dl_quoted_names(const char* names, uint32_t n) {
  return quoted_names(names, n, "\"", [](std::string& o, unsigned char ch) { if (ch == '"') o.push_back('"'); o.push_back((char)ch); });
}

namespace {
// The first row (event order) with a cell that has no encoding: the error the reference raises for it, from RB_E_JSON to the Date32 / NULL
// message. `ev`: the row's event. *hand_over: the cell is the host's (RB_E_HOST_CELL) — no error; the object goes to the caller with status
// ETLG_RB_NEEDS_HOST and without blocks A and C.
int32_t rows_report_error(etlg_ctx* c, etlg_rowbinary& rb, const RbReport& rep, uint64_t ev, bool* hand_over) {
  const uint32_t code = rep.code, col = rep.col;
  if (code == RB_E_JSON) return set_error(c, ETLG_E_JSON, (int64_t)ev);   // a json cell that is not one JSON value: the decode error of codec/text.rs:126-134, as etlg_batch_columns reports it
  if (code == RB_E_HOST_CELL) {
    rb.v.status = ETLG_RB_NEEDS_HOST; rb.v.host_event = ev; rb.v.host_column = col;
    give_device_blocks(c, rb.m);   // (block B is not taken yet)
    *hand_over = true;
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

// One handoff_rows call.
struct RowsBuild {
  etlg_ctx* const c; etlg_batch* const b; const int32_t slot; const RowsCall call; const bool on_dev;
  const SlotHost& sh; const etlg_batch_view& bv; const hipStream_t s; const uint32_t nc; const uint64_t ne;
  const uint64_t nr_cap;   // BigQuery: an update that changes the primary key is two rows
  const uint32_t nblk;
  // Members go in reverse order: block S (sblk: block counts, counters, column words, row_base — read by the selection, by both passes of
  // k_rowbinary and by their read-backs) returns to the pool before `rb` gives its blocks back. Which stop covers the release: the
  // NEEDS_HOST class return of handoff_rows comes before block S is taken; the error and RB_E_HOST_CELL returns come behind the stop of
  // sizes() (and the synchronous copy of the event), when only pass 0 has been launched; a return from publish — its final stop, which
  // also stands in front of give_device_blocks. HIPCHK returns in between follow a failed call.
  std::unique_ptr<etlg_rowbinary, void (*)(etlg_rowbinary*)> rb{new etlg_rowbinary, etlg_rowbinary_free};
  ScratchBlk sblk{c};
  RowWords w;
  size_t o_cnt = 0, o_cols = 0, o_base = 0;                // block S: block counts | host-row counter, error word, total | column words (+ keys) | row_base
  size_t o_off = 0, o_len = 0, o_scan = 0, o_part = 0;     // block A: row_event | row_offsets | lens | scan scratch | where the parts of a row begin (k_rb_rows)
  uint8_t* S = nullptr; uint8_t* A = nullptr;
  volatile unsigned long long* down = nullptr;             // pinned: [0] row count, [1..3] host rows, error word, total
  uint64_t n = 0; int64_t total = 0; unsigned long long err_word = ~0ull;
  RbJob j{};

  RowsBuild(etlg_ctx* c_, etlg_batch* b_, int32_t slot_, const RowsCall& call_, uint32_t flags)
      : c(c_), b(b_), slot(slot_), call(call_), on_dev((flags & ETLG_F_OUTPUT_ON_DEVICE) != 0), sh(*c_->slots[(size_t)slot_]), bv(b_->v), s(c_->stream),
        nc(sh.desc.n_cols), ne(bv.n_events), nr_cap(call.format != FMT_ROWBINARY ? 2 * ne : ne), nblk((uint32_t)((ne + 255) / 256)) {
    rb->v.on_device = on_dev ? 1u : 0u; rb->v.host_event = ~0ull;
    rb->m.ctx = c; rb->m.ctx_gen = c->gen;
    if (call.format == FMT_DUCKLAKE) { rb->dl_batch = b; rb->dl_serial = b->serial; rb->dl_slot = slot; rb->dl_what = call.dl_what; }
    if (call.format == FMT_NDJSON) { rb->nd_batch = b; rb->nd_serial = b->serial; rb->nd_slot = slot; }
    if (call.format == FMT_PROTOBUF) { rb->pb_batch = b; rb->pb_serial = b->serial; rb->pb_slot = slot; }
    if (call.format == FMT_ROWBINARY) { rb->ch_batch = b; rb->ch_serial = b->serial; rb->ch_slot = slot; rb->ch_engine = call.engine; }
  }
  const uint32_t* s_cols() const { return (const uint32_t*)(S + o_cols); }
  unsigned long long* s_cnt() const { return (unsigned long long*)(S + o_cnt); }

  // ---- 2. block S (freed on return), the pinned staging, block A (sized for every event being a row). Staging: [host rows = 0 | error
  // word = ~0 | total | pad to 64 | column words] goes up in one copy (S + o_cnt .. lies the same way); [row count] and [host rows | error
  // word | total] come back in one copy each. (From / to pageable memory every one of these small copies was a stop of its own.)
  int32_t blocks_and_staging() {
    const NdKeys* nd = call.nd;
    const size_t nd_bytes = nd ? (size_t)(nc + 1) * 4 + nd->bytes.size() : 0;   // (FMT_NDJSON / FMT_DUCKLAKE: the keys' offsets and bytes behind the column words)
    ScratchLayout s_lay((size_t)(nblk + 1) * 4);
    o_cnt = s_lay.skip(64); o_cols = s_lay.take((size_t)nc * 8 + 8 + nd_bytes); o_base = s_lay.take(nr_cap * 8);
    HIPCHK(c, blk_take(c, s_lay.total() + 64, false, &sblk.p, &sblk.cap));
    S = (uint8_t*)sblk.p;
    const size_t up_bytes = 64 + (size_t)nc * 8 + nd_bytes, hand_bytes = al64(up_bytes) + 64;
    RC(pinned_grow(c, (void**)&c->h_hand, &c->h_hand_cap, hand_bytes, hand_bytes + 4096, 1, nullptr));
    unsigned long long* up = (unsigned long long*)c->h_hand;
    up[0] = 0ull; up[1] = ~0ull; up[2] = 0ull;
    if (nc) memcpy(c->h_hand + 64, w.cols.data(), (size_t)nc * 8);
    if (nd) {
      memcpy(c->h_hand + 64 + (size_t)nc * 8, nd->off.data(), (size_t)(nc + 1) * 4);
      if (!nd->bytes.empty()) memcpy(c->h_hand + 64 + (size_t)nc * 12 + 4, nd->bytes.data(), nd->bytes.size());
    }
    HIPCHK(c, hipMemcpyAsync(s_cnt(), c->h_hand, up_bytes, hipMemcpyHostToDevice, s));
    down = (volatile unsigned long long*)(c->h_hand + al64(up_bytes));
    const uint32_t nblk_r = (uint32_t)((nr_cap + 255) / 256);
    ScratchLayout a_lay(nr_cap * 8);
    o_off = a_lay.take((nr_cap + 1) * 8); o_len = a_lay.take(nr_cap * 4); o_scan = a_lay.take((size_t)(nblk_r + 1) * 8);
    o_part = a_lay.skip(3 * al64(nr_cap * 4));
    HIPCHK(c, blk_take(c, a_lay.total() + 64, false, &rb->m.d_a, &rb->m.cap_a));
    A = (uint8_t*)rb->m.d_a;
    return ETLG_OK;
  }

  // ---- 3. which events are rows, and of which kind: the common selection with the format's additions                         (stop)
  int32_t select() {
    if (!ne) return ETLG_OK;
    const uint32_t format = call.format;
    ColSel q = col_select_common(bv, sh, slot, (uint32_t*)S, nblk, (uint64_t*)A, (uint64_t*)(S + o_base));
    // ReplacingMergeTree keys its dedup on the source primary key: the reference refuses Update events of a table whose replica
    // identity is neither PrimaryKey nor Full (clickhouse_update_row -> ensure_clickhouse_key_identity_is_primary_key,
    // clickhouse/core.rs:1359-1427). Such Updates are not encoded here: they are left to the host (n_host_rows), which raises
    // the reference's SourceReplicaIdentityError when it meets the first of them.
    const bool upd_ok = format != FMT_ROWBINARY || call.engine != ETLG_CH_REPLACING_MERGE_TREE || sh.identity_type == 1 || sh.identity_type == 2;
    // Snowflake: inserts, full updates, deletes with a full old row or a key image (core.rs:345-438, snowflake_update_row /
    // snowflake_delete_row :572-608); partial updates and deletes without an old row stay with the host (SourceReplicaIdentityError)
    q.kinds = format == FMT_NDJSON ? SEL_INSERT | SEL_UPDATE_NEW | SEL_DELETE_OLD | SEL_DELETE_KEY : format != FMT_ROWBINARY ? SEL_INSERT   // (pb_selected / dl_selected pick the rest)
                      : SEL_INSERT | SEL_DELETE_OLD | (upd_ok ? SEL_UPDATE_NEW : 0u) | (w.key_ok ? SEL_DELETE_KEY : 0u);
    q.host_rows = s_cnt();
    if (format == FMT_DUCKLAKE) {  // dl_selected (ducklake/core.rs:1824-1945, batches.rs:1128-1226)
      q.dl = w.dl;
      q.dl_ident = sh.desc.n_ident != 0 ? 1u : 0u;
      if (w.dl == DL_SEL_UPDATES) { q.n_cols = nc; q.fixed = bv.fixed; q.kcols = s_cols() + nc; }   // (the new row's cell states, the identity bits)
    }
    if (format == FMT_PROTOBUF) {  // BigQuery: inserts, updates (one or two rows) and deletes (bigquery/core.rs:978-1036); the events the reference refuses stay with the host
      q.pb = 1; q.n_cols = nc; q.identity_pk = sh.identity_type == 1 ? 1u : 0u; q.pk_comparable = w.pk_comparable ? 1u : 0u;
      q.fixed = bv.fixed; q.heap = bv.heap; q.cols = s_cols(); q.kcols = s_cols() + nc;
    }
    etlg_k_col_select(&q, s);
    HIPCHK(c, hipMemcpyAsync((void*)&down[0], S + (size_t)nblk * 4, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    n = (uint32_t)down[0];
    return ETLG_OK;
  }

  // ---- 4. the job, and pass 0: every row's size, their offsets, the total, the first cell without an encoding                 (stop)
  int32_t sizes() {
    const uint32_t format = call.format; const uint8_t* nullable_flags = call.nullable_flags;
    j.fixed = bv.fixed; j.heap = bv.heap; j.row_event = (const uint64_t*)A; j.row_base = (const uint64_t*)(S + o_base);
    j.ev_kind = bv.ev_kind; j.ev_commit = bv.ev_commit_lsn; j.ev_ord = bv.ev_tx_ordinal;
    j.n_rows = n; j.n_cols = nc; j.engine = (uint32_t)call.engine;
    j.cdc_nullable = nullable_flags ? (nullable_flags[nc] ? 1u : 0u) | (nullable_flags[nc + 1] ? 2u : 0u) : 0u;
    j.format = format;
    j.copy_tail = ((format == FMT_ROWBINARY || format == FMT_PROTOBUF) && b->copy.active) ? 1u : 0u;   // a table-copy batch: write_table_rows' rows (clickhouse/core.rs:739-773, bigquery/core.rs:602-649)
    j.cols = s_cols(); j.kcols = (w.key_ok || format != FMT_ROWBINARY) ? s_cols() + nc : nullptr; j.ev_flags = bv.ev_flags; j.lens = (uint32_t*)(A + o_len); j.offsets = (const int64_t*)(A + o_off);
    j.err = s_cnt() + 1;
    j.has_json = w.has_json ? 1u : 0u;
    j.qparts = nc >= 4 ? 4u : nc >= 2 ? 2u : 1u; j.parts = 1;
    j.part_off = (uint32_t*)(A + o_part);
    if (call.nd) {
      j.kcols = s_cols() + nc;
      j.nd_key_off = (const uint32_t*)(S + o_cols + (size_t)nc * 8); j.nd_keys = S + o_cols + (size_t)nc * 12 + 4;
      j.nd_zero_token = b->copy.active ? 1u : 0u;   // a table-copy batch (etlg_copy_decode): Insert rows under OffsetToken::zero (core.rs:683-699)
      if (w.dl) j.dl_what = dl_row_what(w.dl);
      if (w.dl == DL_SEL_UPDATES && n && nc) {  // col_ends: a block of its own, sized by the rows the select pass counted (not by 2 x events x columns)
        HIPCHK(c, blk_take(c, (size_t)n * nc * 4 + 64, false, &rb->m.d_c, &rb->m.cap_c));
        j.col_ends = (uint32_t*)rb->m.d_c;
      }
    }
    if (n) etlg_k_rowbinary(&j, (unsigned long long*)(A + o_scan), (int64_t*)(A + o_off), s_cnt() + 2, 0, s);
    else HIPCHK(c, hipMemsetAsync(A + o_off, 0, 8, s));
    HIPCHK(c, hipMemcpyAsync((void*)&down[1], s_cnt(), 24, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    rb->v.n_host_rows = down[1]; err_word = down[2]; total = (int64_t)down[3];
    return ETLG_OK;
  }

  // ---- 5. the first row (event order) with a cell that has no encoding: its event, then rows_report_error
  int32_t report_error(etlg_rowbinary** out) {
    const RbReport rep = rb_report_unpack(err_word);
    uint64_t ev = 0;
    HIPCHK(c, hipMemcpy(&ev, A + rep.row * 8, 8, hipMemcpyDeviceToHost));
    bool hand_over = false;
    const int32_t rc = rows_report_error(c, *rb, rep, ev, &hand_over);
    if (hand_over) *out = rb.release();
    return rc;
  }

  // ---- 6. block B and pass 1: the bytes
  int32_t bytes() {
    if (!total) return ETLG_OK;
    HIPCHK(c, blk_take(c, (size_t)total + 64, false, &rb->m.d_b, &rb->m.cap_b));
    j.out = (uint8_t*)rb->m.d_b;
    j.parts = rb_parts(n, (uint64_t)total, j.qparts, c->rb_parts_test);
    etlg_k_rowbinary(&j, nullptr, nullptr, nullptr, 1, s);
    return ETLG_OK;
  }

  // ---- 7. the view (device pointers, or a host copy: row_event and the offsets of the rows there are | the bytes | col_ends)   (stop)
  int32_t publish(etlg_rowbinary** out) {
    const uint8_t* base_a = A; const uint8_t* base_b = (const uint8_t*)rb->m.d_b;
    rb->col_ends = (const uint32_t*)rb->m.d_c;
    if (!on_dev) {
      const size_t ce_bytes = rb->m.d_c ? (size_t)n * nc * 4 : 0, ce_at = o_len + al64((size_t)total);
      RC(host_copy(c, rb->m, s, o_off + (n + 1) * 8, o_len, (size_t)total, ce_at, ce_bytes));
      base_a = rb->m.h; base_b = rb->m.h + o_len;
      rb->col_ends = ce_bytes ? (const uint32_t*)(rb->m.h + ce_at) : nullptr;
    }
    HIPCHK(c, hipStreamSynchronize(s));   // block S is freed on return
    if (!on_dev) give_device_blocks(c, rb->m);
    rb->v.n_rows = n; rb->v.n_bytes = (uint64_t)total;
    rb->v.row_event = (const uint64_t*)base_a; rb->v.row_offsets = (const int64_t*)(base_a + o_off); rb->v.bytes = total ? base_b : nullptr;
    *out = rb.release();
    return ETLG_OK;
  }
};
}  // namespace

// The builder behind the four row formats (RowsCall says which).
static int32_t handoff_rows(etlg_ctx* c, etlg_batch* b, int32_t slot, const RowsCall& call, uint32_t flags, etlg_rowbinary** out) {
  *out = nullptr;
  if (const int32_t rc = batch_ready(c, b, "etlg_batch_rowbinary" NEEDS_DEVICE)) return rc;   // (the message names this entry point for all four formats)
  if (!slot_known(c, slot) || (call.engine != ETLG_CH_MERGE_TREE && call.engine != ETLG_CH_REPLACING_MERGE_TREE)) return ETLG_InvalidArgument;
  if (call.format == FMT_ROWBINARY && call.n_flags != c->slots[(size_t)slot]->desc.n_cols + 2) return lib_error(c, ETLG_ConversionError, "ClickHouse RowBinary row width mismatch");
  RowsBuild q(c, b, slot, call, flags);
  q.w = row_words(q.sh, call, b->copy.active);   // 1. column words
  q.rb->updates = q.w.dl == DL_SEL_UPDATES;      // partial Updates: two records per event and the col_ends array
  if (q.w.host_column != ~0u) {                  // a column only the host encodes: nothing is built
    q.rb->v.status = ETLG_RB_NEEDS_HOST; q.rb->v.host_column = q.w.host_column;
    *out = q.rb.release();
    return ETLG_OK;
  }
  RC(q.blocks_and_staging());                    // 2. block S, staging, block A
  RC(q.select());                                // 3. select                          (stop)
  RC(q.sizes());                                 // 4. sizes                           (stop)
  if (q.err_word != ~0ull) return q.report_error(out);   // 5. error
  RC(q.bytes());                                 // 6. bytes
  return q.publish(out);                         // 7. the view                        (stop)
}
}  // extern "C++"

int32_t etlg_batch_rowbinary(etlg_ctx* c, etlg_batch* b, int32_t slot, const uint8_t* nullable_flags, uint32_t n_flags, int32_t engine,
                             uint32_t flags, etlg_rowbinary** out) {
  if (!c || !b || !out || b->ctx != c || !nullable_flags) return ETLG_InvalidArgument;
  return handoff_rows(c, b, slot, RowsCall{FMT_ROWBINARY, nullable_flags, n_flags, engine, nullptr, 0u}, flags, out);
}

int32_t etlg_batch_protobuf(etlg_ctx* c, etlg_batch* b, int32_t slot, uint32_t flags, etlg_rowbinary** out) {
  if (!c || !b || !out || b->ctx != c) return ETLG_InvalidArgument;
  return handoff_rows(c, b, slot, RowsCall{FMT_PROTOBUF, nullptr, 0u, ETLG_CH_MERGE_TREE, nullptr, 0u}, flags, out);
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
  return handoff_rows(c, b, slot, RowsCall{FMT_NDJSON, nullptr, 0u, ETLG_CH_MERGE_TREE, &k, 0u}, flags & ETLG_F_OUTPUT_ON_DEVICE, out);
}

// DuckLake SQL literals (ducklake/encoding.rs:366-612, batches.rs:1229-1316): the column names are quoted here once, as
// quote_double_identifier does, and go up with the column words like the NDJSON keys; dl_row puts ` = <literal>` / ` IS NULL` behind them.
int32_t etlg_batch_duckdb(etlg_ctx* c, etlg_batch* b, int32_t slot, int32_t what, const char* col_names, uint32_t n_names, uint32_t flags,
                          etlg_rowbinary** out) {
  if (!c || !b || !out || b->ctx != c || (n_names && !col_names)) return ETLG_InvalidArgument;
  *out = nullptr;
  if ((uint32_t)what != ETLG_DL_TUPLES && (uint32_t)what != ETLG_DL_PREDICATES && (uint32_t)what != ETLG_DL_UPDATES) return lib_error(c, ETLG_InvalidArgument, "etlg_batch_duckdb: what must be ETLG_DL_TUPLES, ETLG_DL_PREDICATES or ETLG_DL_UPDATES");
  if (!slot_known(c, slot)) return lib_error(c, ETLG_InvalidArgument, "unknown schema slot");
  if (n_names != c->slots[(size_t)slot]->desc.n_cols) return lib_error(c, ETLG_InvalidArgument, "DuckLake row width mismatch: one column name per replicated column");
  const NdKeys k = dl_quoted_names(col_names, n_names);
  return handoff_rows(c, b, slot, RowsCall{FMT_DUCKLAKE, nullptr, 0u, ETLG_CH_MERGE_TREE, &k, (uint32_t)what}, flags & ETLG_F_OUTPUT_ON_DEVICE, out);
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
