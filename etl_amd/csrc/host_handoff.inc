// Part of host.cpp (included there, one translation unit): what the hand-off calls over a decoded, device-resident batch share, and the calls
// that build neither columns nor rows — size hints, cuts, locate, outline, DuckLake plan, Snowflake plan, ClickHouse plan, BigQuery plan, Iceberg plan, payload, finish, fingerprints (kernels: finish.hip, kernels.hip,
// fingerprint.hip). The two builders follow in host_handoff_columns.inc and host_handoff_rows.inc.

extern "C++" {
// ---- hand-off (columns.hip, rowformats.hip, finish.hip)
// What every hand-off call does first: an ASYNC batch is synchronised — one that ended in a decode error gives the caller that error
// (fail-fast, as the reference), not a hand-off of the prefix — and a batch that is not device-resident is refused. `refusal`: the
// entry point's name + NEEDS_DEVICE (a string literal: the error keeps the pointer). Returns ETLG_OK, or what the caller returns.
#define NEEDS_DEVICE " needs a device-resident batch (ETLG_F_OUTPUT_ON_DEVICE, not downloaded)"
// `code`: what the refusal returns — ETLG_InvalidState everywhere but in etlg_batch_outline, etlg_ducklake_plan, etlg_snowflake_plan, etlg_clickhouse_plan, etlg_bigquery_plan and etlg_iceberg_plan, whose contracts list the batch among their arguments.
static int32_t batch_ready(etlg_ctx* c, etlg_batch* b, const char* refusal, int32_t code = ETLG_InvalidState) {
  if (b->pending) RC(etlg_batch_sync(c, b));
  if (!b->v.on_device || !b->dev) return lib_error(c, code, refusal);
  return ETLG_OK;
}
static bool slot_known(const etlg_ctx* c, int32_t slot) { return slot >= 0 && (size_t)slot < c->slots.size(); }
static NdKeys dl_quoted_names(const char* names, uint32_t n);   // (host_handoff_rows.inc)

// ---- shared by build_columns and handoff_rows
// The ColSel fields every selection sets alike: the batch's events, the slot and its row widths, the block counts and the two outputs.
// The caller adds `kinds` and what its format needs.
static ColSel col_select_common(const etlg_batch_view& bv, const SlotHost& sh, int32_t slot, uint32_t* blk, uint32_t nblk, uint64_t* row_event, uint64_t* row_base) {
  ColSel q{};
  q.ev_kind = bv.ev_kind; q.ev_flags = bv.ev_flags; q.ev_slot = bv.ev_schema_slot; q.ev_body = bv.ev_body_off;
  q.n_events = bv.n_events; q.slot = (uint32_t)slot;
  q.row_full = sh.desc.row_bytes_full; q.row_key = sh.desc.row_bytes_key;
  q.blk = blk; q.nblocks = nblk; q.row_event = row_event; q.row_base = row_base;
  return q;
}
// A pinned staging buffer of the context that only grows: at least `want` units are there on return. A smaller one is freed behind a stop
// (copies from it may be in flight) and `new_cap` units of `unit` bytes are allocated; *grew says the content is new.
static int32_t pinned_grow(etlg_ctx* c, void** ptr, size_t* cap, size_t want, size_t new_cap, size_t unit, bool* grew) {
  if (grew) *grew = false;
  if (*cap >= want) return ETLG_OK;
  if (*ptr) { HIPCHK(c, hipStreamSynchronize(c->stream)); (void)hipHostFree(*ptr); *ptr = nullptr; *cap = 0; }
  HIPCHK(c, hipHostMalloc(ptr, new_cap * unit, hipHostMallocDefault));
  *cap = new_cap;
  if (grew) *grew = true;
  return ETLG_OK;
}
// the object keeps no device block: a host view has been copied out, or nothing was built
static void give_device_blocks(etlg_ctx* c, HandoffBlocks& m) {
  blk_give(c, c->gen, m.d_a, m.cap_a, false); blk_give(c, c->gen, m.d_b, m.cap_b, false); blk_give(c, c->gen, m.d_c, m.cap_c, false);
  m.d_a = m.d_b = m.d_c = nullptr;
}
// The host view: one pinned block that takes the first a_bytes of block A at 0, b_bytes of block B at b_at and c_bytes of block C at c_at
// (enqueued; the caller stops before it reads them or gives the device blocks back)
static int32_t host_copy(etlg_ctx* c, HandoffBlocks& m, hipStream_t s, size_t a_bytes, size_t b_at, size_t b_bytes, size_t c_at, size_t c_bytes) {
  HIPCHK(c, blk_take(c, c_at + c_bytes + 64, true, (void**)&m.h, &m.cap_h));
  if (a_bytes) HIPCHK(c, hipMemcpyAsync(m.h, m.d_a, a_bytes, hipMemcpyDeviceToHost, s));
  if (b_bytes) HIPCHK(c, hipMemcpyAsync(m.h + b_at, m.d_b, b_bytes, hipMemcpyDeviceToHost, s));
  if (c_bytes) HIPCHK(c, hipMemcpyAsync(m.h + c_at, m.d_c, c_bytes, hipMemcpyDeviceToHost, s));
  return ETLG_OK;
}
}  // extern "C++"

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

// The write_events pass plan (include/etlg.h; k_ol_* in finish.hip). Everything is sized from what the host knows — the window, the
// cuts' count, the caller's caps — so the launches go out in one piece and the call stops once: for the header and, for a host caller,
// the staged outputs, of which the written parts are then copied to the caller. A device caller's memory is written by the last two
// kernels alone, and by neither when a cut is bad.
int32_t etlg_batch_outline(etlg_ctx* c, etlg_batch* b, uint64_t first, uint64_t end, const uint64_t* cuts, uint64_t n_cuts, uint32_t cuts_on_device, uint32_t opts,
                           uint32_t flags, etlg_outline_pass* passes_out, uint64_t* ends_out, uint64_t* touched_out, uint64_t passes_cap, etlg_outline_trunc* trunc_out,
                           uint64_t trunc_cap, etlg_outline_slot* slots_out, etlg_outline_info* info) {
  if (!c || !b || b->ctx != c || !info) return ETLG_InvalidArgument;
  *info = etlg_outline_info{};
  if (const int32_t rc = batch_ready(c, b, "etlg_batch_outline" NEEDS_DEVICE, ETLG_InvalidArgument)) return rc;   // (etlg_batch_cuts' rule; the code is this call's)
  if (b->copy.active) return lib_error(c, ETLG_InvalidArgument, "etlg_batch_outline: a table-copy batch has no write_events passes");
  const etlg_batch_view& bv = b->v;
  if (first > end || end > bv.n_events) return lib_error(c, ETLG_InvalidArgument, "etlg_batch_outline: first <= end <= n_events");
  if (n_cuts && !cuts) return lib_error(c, ETLG_InvalidArgument, "etlg_batch_outline: n_cuts without cuts");
  if (n_cuts > (1ull << 38)) return lib_error(c, ETLG_InvalidArgument, "etlg_batch_outline: more cuts than one call takes (2^38: a grid of 2^30 workgroups marks them)");
  static_assert(sizeof(etlg_outline_pass) == 56 && sizeof(etlg_outline_trunc) == 16 && sizeof(etlg_outline_slot) == 96, "k_ol_write / k_ol_fix write 7, 2 and 12 words");
  const uint64_t n = end - first, ns = bv.n_slots, W = (ns + 63) / 64;
  const bool on_dev = (flags & ETLG_F_OUTPUT_ON_DEVICE) != 0;
  if (!trunc_out) trunc_cap = 0;
  if (!passes_out && !ends_out && !touched_out) passes_cap = 0;
  const uint64_t P = passes_cap < n ? passes_cap : n, T = trunc_cap < bv.fixed_bytes / 8 ? trunc_cap : bv.fixed_bytes / 8;   // what can be written at the most
  uint64_t tile = c->ol_tile_test ? c->ol_tile_test : 2048u;
  while ((n + tile - 1) / tile > (1ull << 30)) tile *= 2;   // (a grid's width; only a test's tile gets here)
  const uint64_t n_tiles = (n + tile - 1) / tile;
  const OutlineLayout lay = outline_layout(n, n_tiles, ns, W, P, T, n_cuts, passes_out != nullptr, ends_out != nullptr, touched_out != nullptr, slots_out != nullptr,
                                           !cuts_on_device, !on_dev);
  hipStream_t s = c->stream;
  ScratchBlk blk{c};
  HIPCHK(c, blk_take(c, lay.total + 64, false, &blk.p, &blk.cap));
  uint8_t* d = (uint8_t*)blk.p;
  HIPCHK(c, hipMemsetAsync(d + lay.zero_at, 0, lay.ones_at - lay.zero_at, s));
  HIPCHK(c, hipMemsetAsync(d + lay.ones_at, 0xFF, lay.ones_end - lay.ones_at, s));
  if (!cuts_on_device && n_cuts) HIPCHK(c, hipMemcpyAsync(d + lay.cuts, cuts, n_cuts * 8, hipMemcpyHostToDevice, s));
  typedef unsigned long long* W64;
  OutlineJob j{};
  j.ev_kind = bv.ev_kind; j.ev_flags = bv.ev_flags; j.ev_slot = bv.ev_schema_slot; j.ev_table = bv.ev_table_id; j.ev_body = bv.ev_body_off; j.fixed = bv.fixed;
  j.first = first; j.n = n; j.n_cuts = n_cuts; j.cuts = cuts_on_device ? (const unsigned long long*)cuts : (const unsigned long long*)(d + lay.cuts);
  j.inline_rel = (opts & ETLG_OL_RELATIONS_INLINE) ? 1u : 0u; j.n_slots = (uint32_t)ns; j.W = (uint32_t)W; j.tile = (uint32_t)tile; j.n_tiles = (uint32_t)n_tiles;
  j.hdr = (W64)(d + lay.hdr); j.bad = (W64)(d + lay.bad); j.bitmap = (uint32_t*)(d + lay.bitmap); j.tsum = (W64)(d + lay.tsum);
  j.crow = (W64)(d + lay.crow); j.cfirst = (W64)(d + lay.cfirst);
  if (passes_out) { j.de = (W64)(d + lay.de); j.re = (W64)(d + lay.re); j.tf = (W64)(d + lay.tf); }
  if (touched_out) j.touched = (W64)(d + lay.touched);
  j.passes_cap = P; j.trunc_cap = T;
  j.passes_out = !passes_out ? nullptr : on_dev ? (W64)passes_out : (W64)(d + lay.s_passes);
  j.ends_out = !ends_out ? nullptr : on_dev ? (W64)ends_out : (W64)(d + lay.s_ends);
  j.touched_out = !touched_out ? nullptr : on_dev ? (W64)touched_out : (W64)(d + lay.s_touched);
  j.trunc_out = !trunc_out ? nullptr : on_dev ? (W64)trunc_out : (W64)(d + lay.s_trunc);
  j.slots_out = !slots_out ? nullptr : on_dev ? (W64)slots_out : (W64)(d + lay.s_slots);
  etlg_k_outline(&j, s);
  uint64_t head[9] = {};   // hdr, and `bad` 64 bytes behind it
  HIPCHK(c, hipMemcpyAsync(head, j.hdr, sizeof head, hipMemcpyDeviceToHost, s));
  std::vector<uint8_t> back;
  if (!on_dev && lay.total > lay.stage_at) { back.resize(lay.total - lay.stage_at); HIPCHK(c, hipMemcpyAsync(back.data(), d + lay.stage_at, back.size(), hipMemcpyDeviceToHost, s)); }
  HIPCHK(c, hipStreamSynchronize(s));   // the one stop
  if (head[8] != ~0ull) { info->status = ETLG_OL_BAD_CUTS; info->bad_cut = head[8]; return ETLG_OK; }
  info->n_passes = head[OL_H_PASSES]; info->n_trunc = head[OL_H_TRUNC]; info->n_relations = head[OL_H_REL]; info->n_rows = head[OL_H_ROWS];
  info->n_ranges = n_cuts ? head[OL_H_RANGES] : 1; info->status = ETLG_OL_OK;
  if (!on_dev) {
    const uint64_t np = info->n_passes < P ? info->n_passes : P, nt = info->n_trunc < T ? info->n_trunc : T;
    const auto staged = [&](size_t at) { return back.data() + (at - lay.stage_at); };
    if (passes_out && np) memcpy(passes_out, staged(lay.s_passes), np * 56);
    if (ends_out && np) memcpy(ends_out, staged(lay.s_ends), np * 8);
    if (touched_out && np && W) memcpy(touched_out, staged(lay.s_touched), np * W * 8);
    if (trunc_out && nt) memcpy(trunc_out, staged(lay.s_trunc), nt * 16);
    if (slots_out && ns) memcpy(slots_out, staged(lay.s_slots), ns * 96);
  }
  return ETLG_OK;
}

// The DuckLake atomic-batch plan (include/etlg.h; k_dlp_* in finish.hip). Everything is sized from what the host knows — the events,
// the passes' count, the caller's caps — so the launches go out in one piece and the call stops once: for the header and, for a host
// caller, the staged outputs, of which the written parts are then copied to the caller. A device caller's memory is written by the last
// two kernels alone, and by neither when a status word is set.
int32_t etlg_ducklake_plan(etlg_ctx* c, etlg_batch* b, int32_t slot, const etlg_outline_pass* passes, uint64_t n_passes, uint32_t passes_on_device,
                           uint32_t has_watermark, uint64_t wm_commit_lsn, uint64_t wm_tx_ordinal, uint64_t seed, const etlg_rowbinary* tuples,
                           const etlg_rowbinary* predicates, const etlg_rowbinary* updates, uint32_t flags, etlg_dl_range* ranges_out, etlg_dl_batch* batches_out,
                           uint64_t batches_cap, etlg_dl_op* ops_out, uint64_t ops_cap, etlg_dl_plan_info* info) {
  if (!c || !b || b->ctx != c || !info) return ETLG_InvalidArgument;
  *info = etlg_dl_plan_info{};
  info->event = info->bad_pass = ~0ull;
  if (const int32_t rc = batch_ready(c, b, "etlg_ducklake_plan" NEEDS_DEVICE, ETLG_InvalidArgument)) return rc;
  if (b->copy.active) return lib_error(c, ETLG_InvalidArgument, "etlg_ducklake_plan: a table-copy batch is one batch of all its rows, there is nothing to plan");
  if (!slot_known(c, slot)) return lib_error(c, ETLG_InvalidArgument, "unknown schema slot");
  if (n_passes && !passes) return lib_error(c, ETLG_InvalidArgument, "etlg_ducklake_plan: n_passes without passes");
  const etlg_batch_view& bv = b->v;
  const uint64_t n = bv.n_events;
  if (n_passes > (1ull << 38) || n > (1ull << 38)) return lib_error(c, ETLG_InvalidArgument, "etlg_ducklake_plan: more passes or events than one call takes (2^38: a grid of 2^30 workgroups walks them)");
  auto mine = [&](const etlg_rowbinary* r, uint32_t what) { return !r || (r->dl_batch == b && r->dl_serial == b->serial && r->dl_slot == slot && r->dl_what == what && r->v.on_device && r->v.status == ETLG_RB_OK); };
  if (!mine(tuples, ETLG_DL_TUPLES) || !mine(predicates, ETLG_DL_PREDICATES) || !mine(updates, ETLG_DL_UPDATES))
    return lib_error(c, ETLG_InvalidArgument, "etlg_ducklake_plan takes the ETLG_DL_TUPLES, ETLG_DL_PREDICATES and ETLG_DL_UPDATES objects etlg_batch_duckdb built for this batch and slot, on the device (ETLG_F_OUTPUT_ON_DEVICE) and with status ETLG_RB_OK");
  static_assert(sizeof(etlg_dl_range) == 24 && sizeof(etlg_dl_batch) == 8 * kDlpBatchWords && sizeof(etlg_dl_op) == 8 * kDlpOpWords && sizeof(etlg_outline_pass) == 56,
                "k_dlp_groups / k_dlp_ops write 3, 13 and 4 words; the windows are words 0 and 1 of 7");
  if (!n_passes || !n) return ETLG_OK;   // no window, or no event a window could hold: no member, no group
  const bool on_dev = (flags & ETLG_F_OUTPUT_ON_DEVICE) != 0;
  if (!ranges_out && !batches_out) batches_cap = 0;
  if (!ops_out) ops_cap = 0;
  const uint64_t B = batches_cap < n ? batches_cap : n, K = ops_cap < 2 * n ? ops_cap : 2 * n;   // what can be written at the most
  uint64_t tile = c->dlp_tile_test ? c->dlp_tile_test : 2048u;
  while ((n + tile - 1) / tile > (1ull << 30)) tile *= 2;   // (a grid's width; only a test's tile gets here)
  const uint64_t n_tiles = (n + tile - 1) / tile;
  const DlpLayout lay = dlp_layout(n, n_tiles, n_passes, B, K, ranges_out != nullptr, batches_out != nullptr, !passes_on_device, !on_dev);
  hipStream_t s = c->stream;
  ScratchBlk blk{c};
  HIPCHK(c, blk_take(c, lay.total + 64, false, &blk.p, &blk.cap));
  uint8_t* d = (uint8_t*)blk.p;
  HIPCHK(c, hipMemsetAsync(d + lay.hdr, 0, 32, s));
  HIPCHK(c, hipMemsetAsync(d + lay.hdr + 32, 0xFF, 32, s));
  if (!passes_on_device) HIPCHK(c, hipMemcpyAsync(d + lay.passes, passes, n_passes * 56, hipMemcpyHostToDevice, s));
  typedef unsigned long long* W64;
  DlpJob j{};
  j.ev_kind = bv.ev_kind; j.ev_flags = bv.ev_flags; j.ev_slot = bv.ev_schema_slot; j.ev_start = bv.ev_start_lsn; j.ev_commit = bv.ev_commit_lsn; j.ev_ord = bv.ev_tx_ordinal;
  j.n_events = n; j.passes = passes_on_device ? (const unsigned long long*)passes : (const unsigned long long*)(d + lay.passes); j.n_passes = n_passes;
  j.slot = (uint32_t)slot; j.no_ident = c->slots[(size_t)slot]->desc.n_ident == 0 ? 1u : 0u;
  j.has_wm = has_watermark ? 1u : 0u; j.tile = (uint32_t)tile; j.n_tiles = (uint32_t)n_tiles; j.wm_lsn = wm_commit_lsn; j.wm_ord = wm_tx_ordinal; j.seed = seed;
  const auto recs = [](const etlg_rowbinary* r) { return r ? DlpRecs{(const unsigned long long*)r->v.row_event, r->v.n_rows, 1u, 0u} : DlpRecs{nullptr, 0, 0u, 0u}; };
  j.t = recs(tuples); j.p = recs(predicates); j.u = recs(updates);
  j.hdr = (W64)(d + lay.hdr); j.tsum = (W64)(d + lay.tsum); j.code = d + lay.code; j.rpre = (W64)(d + lay.rpre);
  j.glens = (uint32_t*)(d + lay.glens); j.gpre = (const int64_t*)(d + lay.gpre); j.dense = (W64)(d + lay.dense); j.gstart = (W64)(d + lay.gstart);
  j.mpos = (W64)(d + lay.mpos); j.oplens = (uint32_t*)(d + lay.oplens); j.opre = (const int64_t*)(d + lay.opre);
  j.batches_cap = B; j.ops_cap = K;
  j.ranges_out = !ranges_out ? nullptr : on_dev ? (W64)ranges_out : (W64)(d + lay.s_ranges);
  j.batches_out = !batches_out ? nullptr : on_dev ? (W64)batches_out : (W64)(d + lay.s_batches);
  j.ops_out = !ops_out ? nullptr : on_dev ? (W64)ops_out : (W64)(d + lay.s_ops);
  etlg_k_ducklake_plan(&j, (W64)(d + lay.gblk), (W64)(d + lay.oblk), s);
  uint64_t head[DLP_H_WORDS] = {};
  HIPCHK(c, hipMemcpyAsync(head, j.hdr, sizeof head, hipMemcpyDeviceToHost, s));
  std::vector<uint8_t> back;
  if (!on_dev && lay.total > lay.stage_at) { back.resize(lay.total - lay.stage_at); HIPCHK(c, hipMemcpyAsync(back.data(), d + lay.stage_at, back.size(), hipMemcpyDeviceToHost, s)); }
  HIPCHK(c, hipStreamSynchronize(s));   // the one stop
  if (head[DLP_H_BAD] != ~0ull) { info->status = ETLG_DLP_BAD_PASSES; info->bad_pass = head[DLP_H_BAD]; return ETLG_OK; }
  if (head[DLP_H_REFUSED] != ~0ull) { info->status = ETLG_DLP_REFUSED; info->event = head[DLP_H_REFUSED] >> 2; info->reason = (uint32_t)(head[DLP_H_REFUSED] & 3u); return ETLG_OK; }
  if (head[DLP_H_NOTPREFIX] != ~0ull) { info->status = ETLG_DLP_NOT_PREFIX; info->event = head[DLP_H_NOTPREFIX]; return ETLG_OK; }
  if (head[DLP_H_NEEDSHOST] != ~0ull) { info->status = ETLG_DLP_NEEDS_HOST; info->event = head[DLP_H_NEEDSHOST]; return ETLG_OK; }
  info->n_batches = head[DLP_H_BATCHES]; info->n_ops = head[DLP_H_OPS]; info->n_members = head[DLP_H_MEMBERS]; info->n_retained = head[DLP_H_RETAINED];
  info->n_dropped = info->n_members - info->n_retained;
  if (!on_dev) {
    const uint64_t nb = info->n_batches < B ? info->n_batches : B, nk = info->n_ops < K ? info->n_ops : K;
    const auto staged = [&](size_t at) { return back.data() + (at - lay.stage_at); };
    if (ranges_out && nb) memcpy(ranges_out, staged(lay.s_ranges), nb * 24);
    if (batches_out && nb) memcpy(batches_out, staged(lay.s_batches), nb * 104);
    if (ops_out && nk) memcpy(ops_out, staged(lay.s_ops), nk * 32);
  }
  return ETLG_OK;
}

// The Snowflake row-batch plan (include/etlg.h; k_sfp_* in finish.hip). Everything is sized from what the host knows — the events, the
// passes' count, the object's n_rows and n_bytes, the caller's cap — so the launches go out in one piece and the call stops once: for
// the header and, for a host caller, the staged outputs. The bound on the segments: two neighbouring segments of a window hold at least
// flush_bytes (the first plus the row that closed it do), so a window has at most 2 * bytes / flush_bytes + 1 of them, and never more
// than rows; the jump levels cover the first bound, the emit grid the sum over the windows.
int32_t etlg_snowflake_plan(etlg_ctx* c, etlg_batch* b, int32_t slot, const etlg_outline_pass* passes, uint64_t n_passes, uint32_t passes_on_device,
                            uint32_t has_committed, uint64_t c_commit_lsn, uint64_t c_tx_ordinal, const etlg_rowbinary* ndjson, uint64_t flush_bytes,
                            uint64_t max_row_bytes, uint32_t flags, etlg_sf_segment* segs_out, uint64_t segs_cap, etlg_sf_window* windows_out, etlg_sf_plan_info* info) {
  if (!c || !b || b->ctx != c || !info) return ETLG_InvalidArgument;
  *info = etlg_sf_plan_info{};
  info->event = info->bad_pass = ~0ull;
  if (const int32_t rc = batch_ready(c, b, "etlg_snowflake_plan" NEEDS_DEVICE, ETLG_InvalidArgument)) return rc;
  if (!slot_known(c, slot)) return lib_error(c, ETLG_InvalidArgument, "unknown schema slot");
  if (n_passes && !passes) return lib_error(c, ETLG_InvalidArgument, "etlg_snowflake_plan: n_passes without passes");
  if (flush_bytes < 1 || flush_bytes > (1ull << 32) || max_row_bytes < 1) return lib_error(c, ETLG_InvalidArgument, "etlg_snowflake_plan: flush_bytes in [1, 2^32] and max_row_bytes >= 1");
  const bool copy = b->copy.active;
  if (copy && has_committed) return lib_error(c, ETLG_InvalidArgument, "etlg_snowflake_plan: a table-copy batch is written under the zero token, there is no committed offset to compare with");
  const etlg_batch_view& bv = b->v;
  const uint64_t n = bv.n_events;
  if (n_passes > (1ull << 38) || n > (1ull << 38)) return lib_error(c, ETLG_InvalidArgument, "etlg_snowflake_plan: more passes or events than one call takes (2^38: a grid of 2^30 workgroups walks them)");
  if (!ndjson || ndjson->nd_batch != b || ndjson->nd_serial != b->serial || ndjson->nd_slot != slot || !ndjson->v.on_device ||
      (ndjson->v.status != ETLG_RB_OK && ndjson->v.status != ETLG_RB_NEEDS_HOST))
    return lib_error(c, ETLG_InvalidArgument, "etlg_snowflake_plan takes the object etlg_batch_ndjson built for this batch and slot, on the device (ETLG_F_OUTPUT_ON_DEVICE)");
  const bool rows = ndjson->v.status == ETLG_RB_OK;
  const uint64_t R = rows ? ndjson->v.n_rows : 0, n_bytes = rows ? ndjson->v.n_bytes : 0;
  if (R >= 0xFFFFFFF0ull) return lib_error(c, ETLG_InvalidArgument, "etlg_snowflake_plan: the object has more rows than one call plans (32-bit jump tables)");
  static_assert(sizeof(etlg_sf_segment) == 8 * kSfpSegWords && sizeof(etlg_sf_window) == 8 * kSfpWinWords && sizeof(etlg_outline_pass) == 56,
                "k_sfp_emit / k_sfp_windows write 13 and 7 words; the windows are words 0 and 1 of 7");
  etlg_outline_pass all{};   // a table-copy batch without passes: one window over all rows
  if (copy && !n_passes) { all.first_event = 0; all.data_end = n; passes = &all; n_passes = 1; passes_on_device = 0; }
  if (!n_passes || !n) {     // no window, or no event a window could hold: no member, no segment
    if (!rows) { info->status = ETLG_SFP_NEEDS_HOST; info->event = ndjson->v.host_event; }
    return ETLG_OK;
  }
  const bool on_dev = (flags & ETLG_F_OUTPUT_ON_DEVICE) != 0;
  if (!segs_out) segs_cap = 0;
  const uint64_t per_window = std::min<uint64_t>(R, 2 * (n_bytes / flush_bytes) + 2), all_windows = std::min<uint64_t>(R, 2 * (n_bytes / flush_bytes) + 1 + n_passes);
  uint32_t levels = 1;
  while ((per_window >> levels) != 0) levels++;   // 2^levels > the segments of any window
  const uint64_t E = std::min(segs_cap, all_windows);   // what can be written at the most
  uint64_t tile = c->sfp_tile_test ? c->sfp_tile_test : 2048u;
  while ((n + tile - 1) / tile > (1ull << 30)) tile *= 2;   // (a grid's width; only a test's tile gets here)
  const uint64_t n_tiles = (n + tile - 1) / tile;
  const SfpLayout lay = sfp_layout(n, n_tiles, n_passes, R, levels, E, windows_out != nullptr, !passes_on_device, !on_dev);
  hipStream_t s = c->stream;
  ScratchBlk blk{c};
  HIPCHK(c, blk_take(c, lay.total + 64, false, &blk.p, &blk.cap));
  uint8_t* d = (uint8_t*)blk.p;
  HIPCHK(c, hipMemsetAsync(d + lay.hdr, 0, 128, s));
  HIPCHK(c, hipMemsetAsync(d + lay.hdr + 32, 0xFF, 32, s));
  if (!passes_on_device) HIPCHK(c, hipMemcpyAsync(d + lay.passes, passes, n_passes * 56, hipMemcpyHostToDevice, s));
  typedef unsigned long long* W64;
  SfpJob j{};
  j.ev_kind = bv.ev_kind; j.ev_flags = bv.ev_flags; j.ev_slot = bv.ev_schema_slot; j.ev_commit = bv.ev_commit_lsn; j.ev_ord = bv.ev_tx_ordinal;
  j.n_events = n; j.passes = passes_on_device ? (const unsigned long long*)passes : (const unsigned long long*)(d + lay.passes); j.n_passes = n_passes;
  j.row_event = rows ? (const unsigned long long*)ndjson->v.row_event : nullptr; j.q = rows ? (const unsigned long long*)ndjson->v.row_offsets : nullptr; j.n_rows = R;
  j.slot = (uint32_t)slot; j.has_c = has_committed ? 1u : 0u; j.zero_keys = copy ? 1u : 0u; j.tile = (uint32_t)tile; j.n_tiles = (uint32_t)n_tiles; j.levels = levels;
  j.c_lsn = c_commit_lsn; j.c_ord = c_tx_ordinal; j.flush = flush_bytes; j.max_row = max_row_bytes;
  j.hdr = (W64)(d + lay.hdr); j.tsum = (W64)(d + lay.tsum); j.code = d + lay.code; j.pre = (W64)(d + lay.pre); j.wrow = (W64)(d + lay.wrow);
  j.slens = (uint32_t*)(d + lay.slens); j.spre = (const int64_t*)(d + lay.spre); j.jump = (uint32_t*)(d + lay.jump);
  j.segs_cap = E;
  j.segs_out = !segs_out ? nullptr : on_dev ? (W64)segs_out : (W64)(d + lay.s_segs);
  j.windows_out = !windows_out ? nullptr : on_dev ? (W64)windows_out : (W64)(d + lay.s_wins);
  etlg_k_snowflake_plan(&j, (W64)(d + lay.sblk), E, rows, s);
  uint64_t head[SFP_H_WORDS] = {};
  HIPCHK(c, hipMemcpyAsync(head, j.hdr, sizeof head, hipMemcpyDeviceToHost, s));
  std::vector<uint8_t> back;
  if (!on_dev && rows && lay.total > lay.stage_at) { back.resize(lay.total - lay.stage_at); HIPCHK(c, hipMemcpyAsync(back.data(), d + lay.stage_at, back.size(), hipMemcpyDeviceToHost, s)); }
  HIPCHK(c, hipStreamSynchronize(s));   // the one stop
  if (head[SFP_H_BAD] != ~0ull) { info->status = ETLG_SFP_BAD_PASSES; info->bad_pass = head[SFP_H_BAD]; return ETLG_OK; }
  if (head[SFP_H_FAILED] != ~0ull) {
    info->status = ETLG_SFP_FAILED; info->event = head[SFP_H_FAILED] >> 2; info->reason = (uint32_t)(head[SFP_H_FAILED] & 3u);
    if (info->reason == ETLG_SFP_R_ROW_TOO_LARGE) info->row_bytes = head[SFP_H_ROWBYTES];
    return ETLG_OK;
  }
  if (head[SFP_H_NOTPREFIX] != ~0ull) { info->status = ETLG_SFP_NOT_PREFIX; info->event = head[SFP_H_NOTPREFIX]; return ETLG_OK; }
  if (!rows) { info->status = ETLG_SFP_NEEDS_HOST; info->event = ndjson->v.host_event; return ETLG_OK; }
  if (head[SFP_H_NEEDSHOST] != ~0ull) { info->status = ETLG_SFP_NEEDS_HOST; info->event = head[SFP_H_NEEDSHOST]; return ETLG_OK; }
  info->n_segs = head[SFP_H_SEGS]; info->n_members = head[SFP_H_MEMBERS]; info->n_retained = head[SFP_H_RETAINED];
  info->n_dropped = info->n_members - info->n_retained; info->n_rows = info->n_retained; info->n_bytes = head[SFP_H_BYTES];
  if (!on_dev) {
    const uint64_t ns = info->n_segs < E ? info->n_segs : E;
    const auto staged = [&](size_t at) { return back.data() + (at - lay.stage_at); };
    if (segs_out && ns) memcpy(segs_out, staged(lay.s_segs), ns * 104);
    if (windows_out) memcpy(windows_out, staged(lay.s_wins), n_passes * 56);
  }
  return ETLG_OK;
}

// The ClickHouse statement plan (include/etlg.h; k_chp_* in finish.hip). As etlg_snowflake_plan above, everything is sized from what the
// host knows — the events, the passes' count, the object's n_rows and n_bytes, the budget, the caller's cap — so the launches go out in
// one piece and the call stops once: for the header and, for a host caller, the staged outputs. The bound on the statements: every
// statement of a window but its last holds at least max_bytes_per_insert bytes, so a window has at most bytes / budget + 1 of them, and
// never more than rows; the jump levels cover the first bound, the emit grid the sum over the windows. The two slot constants of the
// refusals — the identity type, and whether the identity columns are as many as the primary-key columns — come from SlotHost.
int32_t etlg_clickhouse_plan(etlg_ctx* c, etlg_batch* b, int32_t slot, const etlg_outline_pass* passes, uint64_t n_passes, uint32_t passes_on_device,
                             const etlg_rowbinary* rowbinary, uint64_t max_bytes_per_insert, uint32_t flags, etlg_ch_statement* stmts_out, uint64_t stmts_cap,
                             etlg_ch_window* windows_out, etlg_ch_plan_info* info) {
  if (!c || !b || b->ctx != c || !info) return ETLG_InvalidArgument;
  *info = etlg_ch_plan_info{};
  info->event = info->bad_pass = info->fail_pass = ~0ull;
  if (const int32_t rc = batch_ready(c, b, "etlg_clickhouse_plan" NEEDS_DEVICE, ETLG_InvalidArgument)) return rc;
  if (!slot_known(c, slot)) return lib_error(c, ETLG_InvalidArgument, "unknown schema slot");
  if (n_passes && !passes) return lib_error(c, ETLG_InvalidArgument, "etlg_clickhouse_plan: n_passes without passes");
  if (max_bytes_per_insert < 1 || max_bytes_per_insert > (1ull << 63))
    return lib_error(c, ETLG_InvalidArgument, "etlg_clickhouse_plan: max_bytes_per_insert in [1, 2^63] (with 0 the sink's loop never ends)");
  const bool copy = b->copy.active;
  const etlg_batch_view& bv = b->v;
  const uint64_t n = bv.n_events;
  if (n_passes > (1ull << 38) || n > (1ull << 38)) return lib_error(c, ETLG_InvalidArgument, "etlg_clickhouse_plan: more passes or events than one call takes (2^38: a grid of 2^30 workgroups walks them)");
  const etlg_rowbinary* rb = rowbinary;
  if (!rb || rb->ch_batch != b || rb->ch_serial != b->serial || rb->ch_slot != slot || !rb->v.on_device || (rb->v.status != ETLG_RB_OK && rb->v.status != ETLG_RB_NEEDS_HOST))
    return lib_error(c, ETLG_InvalidArgument, "etlg_clickhouse_plan takes the object etlg_batch_rowbinary built for this batch and slot, on the device (ETLG_F_OUTPUT_ON_DEVICE)");
  const bool rows = rb->v.status == ETLG_RB_OK;
  const uint64_t R = rows ? rb->v.n_rows : 0, n_bytes = rows ? rb->v.n_bytes : 0;
  if (R >= 0xFFFFFFF0ull) return lib_error(c, ETLG_InvalidArgument, "etlg_clickhouse_plan: the object has more rows than one call plans (32-bit jump tables)");
  static_assert(sizeof(etlg_ch_statement) == 8 * kChpStmtWords && sizeof(etlg_ch_window) == 8 * kChpWinWords && sizeof(etlg_outline_pass) == 56,
                "k_chp_emit / k_chp_windows write 7 and 6 words; the windows are words 0 and 1 of 7");
  etlg_outline_pass all{};   // a table-copy batch without passes: one window over all rows
  if (copy && !n_passes) { all.first_event = 0; all.data_end = n; passes = &all; n_passes = 1; passes_on_device = 0; }
  if (!n_passes || !n) {     // no window, or no event a window could hold: no member, no statement
    if (!rows) { info->status = ETLG_CHP_NEEDS_HOST; info->event = rb->v.host_event; }
    return ETLG_OK;
  }
  const SlotHost& sh = *c->slots[(size_t)slot];
  uint32_t n_pk = 0;
  for (const uint8_t k : sh.pk) n_pk += k ? 1u : 0u;
  const bool on_dev = (flags & ETLG_F_OUTPUT_ON_DEVICE) != 0;
  if (!stmts_out) stmts_cap = 0;
  const uint64_t full = n_bytes / max_bytes_per_insert;   // statements that reached the budget, at the most
  const uint64_t per_window = std::min<uint64_t>(R, full + 1), all_windows = std::min<uint64_t>(R, full + n_passes);
  uint32_t levels = 1;
  while ((per_window >> levels) != 0) levels++;   // 2^levels > the statements of any window
  const uint64_t E = std::min(stmts_cap, all_windows);   // what can be written at the most
  uint64_t tile = c->chp_tile_test ? c->chp_tile_test : 2048u;
  while ((n + tile - 1) / tile > (1ull << 30)) tile *= 2;   // (a grid's width; only a test's tile gets here)
  const uint64_t n_tiles = (n + tile - 1) / tile;
  const ChpLayout lay = chp_layout(n, n_tiles, n_passes, R, levels, E, windows_out != nullptr, !passes_on_device, !on_dev);
  hipStream_t s = c->stream;
  ScratchBlk blk{c};
  HIPCHK(c, blk_take(c, lay.total + 64, false, &blk.p, &blk.cap));
  uint8_t* d = (uint8_t*)blk.p;
  HIPCHK(c, hipMemsetAsync(d + lay.hdr, 0, 128, s));
  HIPCHK(c, hipMemsetAsync(d + lay.hdr + 32, 0xFF, 32, s));
  if (!passes_on_device) HIPCHK(c, hipMemcpyAsync(d + lay.passes, passes, n_passes * 56, hipMemcpyHostToDevice, s));
  typedef unsigned long long* W64;
  ChpJob j{};
  j.ev_kind = bv.ev_kind; j.ev_flags = bv.ev_flags; j.ev_slot = bv.ev_schema_slot;
  j.n_events = n; j.passes = passes_on_device ? (const unsigned long long*)passes : (const unsigned long long*)(d + lay.passes); j.n_passes = n_passes;
  j.row_event = rows ? (const unsigned long long*)rb->v.row_event : nullptr; j.q = rows ? (const unsigned long long*)rb->v.row_offsets : nullptr; j.n_rows = R;
  j.slot = (uint32_t)slot; j.tile = (uint32_t)tile; j.n_tiles = (uint32_t)n_tiles; j.levels = levels; j.rows = rows ? 1u : 0u;
  j.replacing = rb->ch_engine == ETLG_CH_REPLACING_MERGE_TREE ? 1u : 0u;
  j.ident_ok = (sh.identity_type == 1 || sh.identity_type == 2) ? 1u : 0u; j.width_ok = sh.desc.n_ident == n_pk ? 1u : 0u;
  j.budget = max_bytes_per_insert;
  j.hdr = (W64)(d + lay.hdr); j.tsum = (W64)(d + lay.tsum); j.code = d + lay.code; j.pre = (W64)(d + lay.pre); j.wrow = (W64)(d + lay.wrow);
  j.slens = (uint32_t*)(d + lay.slens); j.spre = (const int64_t*)(d + lay.spre); j.jump = (uint32_t*)(d + lay.jump);
  j.stmts_cap = E;
  j.stmts_out = !stmts_out ? nullptr : on_dev ? (W64)stmts_out : (W64)(d + lay.s_stmts);
  j.windows_out = !windows_out ? nullptr : on_dev ? (W64)windows_out : (W64)(d + lay.s_wins);
  etlg_k_clickhouse_plan(&j, (W64)(d + lay.sblk), E, s);
  uint64_t head[CHP_H_WORDS] = {};
  HIPCHK(c, hipMemcpyAsync(head, j.hdr, sizeof head, hipMemcpyDeviceToHost, s));
  std::vector<uint8_t> back;
  if (!on_dev && rows && lay.total > lay.stage_at) { back.resize(lay.total - lay.stage_at); HIPCHK(c, hipMemcpyAsync(back.data(), d + lay.stage_at, back.size(), hipMemcpyDeviceToHost, s)); }
  HIPCHK(c, hipStreamSynchronize(s));   // the one stop
  if (head[CHP_H_BAD] != ~0ull) { info->status = ETLG_CHP_BAD_PASSES; info->bad_pass = head[CHP_H_BAD]; return ETLG_OK; }
  if (head[CHP_H_FAILED] != ~0ull) {
    info->status = ETLG_CHP_FAILED; info->event = head[CHP_H_FAILED] >> 3; info->reason = (uint32_t)(head[CHP_H_FAILED] & 7u); info->fail_pass = head[CHP_H_FAILPASS];
    return ETLG_OK;
  }
  if (!rows) { info->status = ETLG_CHP_NEEDS_HOST; info->event = rb->v.host_event; return ETLG_OK; }
  if (head[CHP_H_NEEDSHOST] != ~0ull) { info->status = ETLG_CHP_NEEDS_HOST; info->event = head[CHP_H_NEEDSHOST]; info->fail_pass = head[CHP_H_NOROWPASS]; return ETLG_OK; }
  info->n_stmts = head[CHP_H_STMTS]; info->n_members = head[CHP_H_MEMBERS]; info->n_rows = info->n_members; info->n_bytes = head[CHP_H_BYTES];
  if (!on_dev) {
    const uint64_t ns = info->n_stmts < E ? info->n_stmts : E;
    const auto staged = [&](size_t at) { return back.data() + (at - lay.stage_at); };
    if (stmts_out && ns) memcpy(stmts_out, staged(lay.s_stmts), ns * 56);
    if (windows_out) memcpy(windows_out, staged(lay.s_wins), n_passes * 48);
  }
  return ETLG_OK;
}

// The BigQuery request plan (include/etlg.h; k_bqp_* in finish.hip). As etlg_clickhouse_plan above, everything is sized from what the
// host knows — the events, the passes' count, the object's n_rows, the caller's cap — so the launches go out in one piece and the call
// stops once: for the header and, for a host caller, the staged outputs. A window has one request at the most, so the emit grid is
// min(reqs_cap, n_passes); a table-copy batch has at most n_rows of them, so its one kernel runs min(reqs_cap, n_rows) threads — the
// length of row 0, which decides the real count, stays on the device. The two slot constants of the refusals — the identity is
// PrimaryKey, and the identity columns are as many as the primary-key columns — come from SlotHost.
int32_t etlg_bigquery_plan(etlg_ctx* c, etlg_batch* b, int32_t slot, const etlg_outline_pass* passes, uint64_t n_passes, uint32_t passes_on_device,
                           const etlg_rowbinary* protobuf, uint64_t max_batch_bytes, uint32_t flags, etlg_bq_request* reqs_out, uint64_t reqs_cap,
                           etlg_bq_window* windows_out, etlg_bq_plan_info* info) {
  if (!c || !b || b->ctx != c || !info) return ETLG_InvalidArgument;
  *info = etlg_bq_plan_info{};
  info->event = info->bad_pass = info->fail_pass = ~0ull;
  if (const int32_t rc = batch_ready(c, b, "etlg_bigquery_plan" NEEDS_DEVICE, ETLG_InvalidArgument)) return rc;
  if (!slot_known(c, slot)) return lib_error(c, ETLG_InvalidArgument, "unknown schema slot");
  if (n_passes && !passes) return lib_error(c, ETLG_InvalidArgument, "etlg_bigquery_plan: n_passes without passes");
  const bool copy = b->copy.active;
  if (copy && n_passes) return lib_error(c, ETLG_InvalidArgument, "etlg_bigquery_plan: a table-copy batch takes no passes (split_table_rows cuts the rows of the whole call)");
  if (copy && (max_batch_bytes < 1 || max_batch_bytes > (1ull << 63)))
    return lib_error(c, ETLG_InvalidArgument, "etlg_bigquery_plan: max_batch_bytes in [1, 2^63] for a table-copy batch");
  const etlg_batch_view& bv = b->v;
  const uint64_t n = bv.n_events;
  if (n_passes > (1ull << 38) || n > (1ull << 38)) return lib_error(c, ETLG_InvalidArgument, "etlg_bigquery_plan: more passes or events than one call takes (2^38: a grid of 2^30 workgroups walks them)");
  const etlg_rowbinary* pb = protobuf;
  if (!pb || pb->pb_batch != b || pb->pb_serial != b->serial || pb->pb_slot != slot || !pb->v.on_device || (pb->v.status != ETLG_RB_OK && pb->v.status != ETLG_RB_NEEDS_HOST))
    return lib_error(c, ETLG_InvalidArgument, "etlg_bigquery_plan takes the object etlg_batch_protobuf built for this batch and slot, on the device (ETLG_F_OUTPUT_ON_DEVICE)");
  const bool rows = pb->v.status == ETLG_RB_OK;
  const uint64_t R = rows ? pb->v.n_rows : 0;
  if (R > (1ull << 39)) return lib_error(c, ETLG_InvalidArgument, "etlg_bigquery_plan: the object has more rows than one call plans (2^39)");
  static_assert(sizeof(etlg_bq_request) == 8 * kBqpReqWords && sizeof(etlg_bq_window) == 8 * kBqpWinWords && sizeof(etlg_outline_pass) == 56,
                "k_bqp_emit / k_bqp_copy / k_bqp_windows write 8 and 7 words; the windows are words 0 and 1 of 7");
  if (!rows && (copy || !n_passes || !n)) { info->status = ETLG_BQP_NEEDS_HOST; info->event = pb->v.host_event; return ETLG_OK; }   // (no refusal can come first)
  if (!copy && (!n_passes || !n)) return ETLG_OK;   // no window, or no event a window could hold: no member, no request
  const SlotHost& sh = *c->slots[(size_t)slot];
  uint32_t n_pk = 0;
  for (const uint8_t k : sh.pk) n_pk += k ? 1u : 0u;
  const bool on_dev = (flags & ETLG_F_OUTPUT_ON_DEVICE) != 0;
  if (!reqs_out) reqs_cap = 0;
  const uint64_t E = std::min(reqs_cap, copy ? R : n_passes);   // what can be written at the most
  const uint64_t ne = copy ? 0 : n;                              // a table-copy batch walks no event
  uint64_t tile = c->bqp_tile_test ? c->bqp_tile_test : 2048u;
  while ((ne + tile - 1) / tile > (1ull << 30)) tile *= 2;   // (a grid's width; only a test's tile gets here)
  const uint64_t n_tiles = (ne + tile - 1) / tile, n_win = copy ? 1 : n_passes;
  const BqpLayout lay = bqp_layout(ne, n_tiles, n_passes, n_win, E, windows_out != nullptr, !copy && !passes_on_device, !on_dev);
  hipStream_t s = c->stream;
  ScratchBlk blk{c};
  HIPCHK(c, blk_take(c, lay.total + 64, false, &blk.p, &blk.cap));
  uint8_t* d = (uint8_t*)blk.p;
  HIPCHK(c, hipMemsetAsync(d + lay.hdr, 0, 128, s));
  HIPCHK(c, hipMemsetAsync(d + lay.hdr + 32, 0xFF, 32, s));
  if (!copy && !passes_on_device) HIPCHK(c, hipMemcpyAsync(d + lay.passes, passes, n_passes * 56, hipMemcpyHostToDevice, s));
  typedef unsigned long long* W64;
  BqpJob j{};
  j.ev_kind = bv.ev_kind; j.ev_flags = bv.ev_flags; j.ev_slot = bv.ev_schema_slot;
  j.n_events = ne; j.passes = passes_on_device ? (const unsigned long long*)passes : (const unsigned long long*)(d + lay.passes); j.n_passes = n_passes;
  j.row_event = rows ? (const unsigned long long*)pb->v.row_event : nullptr; j.q = rows ? (const unsigned long long*)pb->v.row_offsets : nullptr; j.n_rows = R;
  j.slot = (uint32_t)slot; j.tile = (uint32_t)tile; j.n_tiles = (uint32_t)n_tiles; j.rows = rows ? 1u : 0u;
  j.ident_pk = sh.identity_type == 1 ? 1u : 0u; j.width_ok = sh.desc.n_ident == n_pk ? 1u : 0u;
  j.budget = max_batch_bytes;
  j.hdr = (W64)(d + lay.hdr); j.tsum = (W64)(d + lay.tsum); j.code = d + lay.code; j.pre = (W64)(d + lay.pre); j.wrow = (W64)(d + lay.wrow);
  j.slens = (uint32_t*)(d + lay.slens); j.spre = (const int64_t*)(d + lay.spre);
  j.reqs_cap = E;
  j.reqs_out = !reqs_out ? nullptr : on_dev ? (W64)reqs_out : (W64)(d + lay.s_reqs);
  j.windows_out = !windows_out ? nullptr : on_dev ? (W64)windows_out : (W64)(d + lay.s_wins);
  etlg_k_bigquery_plan(&j, (W64)(d + lay.sblk), E, copy, s);
  uint64_t head[BQP_H_WORDS] = {};
  HIPCHK(c, hipMemcpyAsync(head, j.hdr, sizeof head, hipMemcpyDeviceToHost, s));
  std::vector<uint8_t> back;
  if (!on_dev && rows && lay.total > lay.stage_at) { back.resize(lay.total - lay.stage_at); HIPCHK(c, hipMemcpyAsync(back.data(), d + lay.stage_at, back.size(), hipMemcpyDeviceToHost, s)); }
  HIPCHK(c, hipStreamSynchronize(s));   // the one stop
  if (head[BQP_H_BAD] != ~0ull) { info->status = ETLG_BQP_BAD_PASSES; info->bad_pass = head[BQP_H_BAD]; return ETLG_OK; }
  if (head[BQP_H_FAILED] != ~0ull) {
    info->status = ETLG_BQP_FAILED; info->event = head[BQP_H_FAILED] >> 3; info->reason = (uint32_t)(head[BQP_H_FAILED] & 7u); info->fail_pass = head[BQP_H_FAILPASS];
    return ETLG_OK;
  }
  if (!rows) { info->status = ETLG_BQP_NEEDS_HOST; info->event = pb->v.host_event; return ETLG_OK; }
  if (head[BQP_H_NEEDSHOST] != ~0ull) { info->status = ETLG_BQP_NEEDS_HOST; info->event = head[BQP_H_NEEDSHOST]; info->fail_pass = head[BQP_H_NOROWPASS]; return ETLG_OK; }
  info->n_reqs = head[BQP_H_REQS]; info->n_members = head[BQP_H_MEMBERS]; info->n_rows = head[BQP_H_ROWS]; info->n_two_row = head[BQP_H_TWOROW];
  info->n_bytes = head[BQP_H_BYTES]; info->est_row_bytes = head[BQP_H_EST]; info->target_batches = head[BQP_H_TARGET];
  if (!on_dev) {
    const uint64_t nr = info->n_reqs < E ? info->n_reqs : E;
    const auto staged = [&](size_t at) { return back.data() + (at - lay.stage_at); };
    if (reqs_out && nr) memcpy(reqs_out, staged(lay.s_reqs), nr * 64);
    if (windows_out) memcpy(windows_out, staged(lay.s_wins), n_win * 56);
  }
  return ETLG_OK;
}

// The Iceberg write plan (include/etlg.h; k_icp_* in finish.hip). As etlg_bigquery_plan above, everything is sized from what the host
// knows — the events, the passes' count, the caller's cap, and from the object's column records which bitmaps can hold a counted bit and
// how many words each has — so the launches go out in one piece and the call stops once: for the header and, for a host caller, the
// staged outputs. A window has one write at the most, so at most min(writes_cap, n_passes) writes and that many times n_cols slices
// can be written. The column and bitmap records go up in one copy. The slot's table id is the context's (SlotHost.desc.table_id).
static uint32_t icp_fixed_width(uint32_t kind) {   // bytes of a list element of a fixed-width kind; 0: bit-packed or var-len
  switch (kind) {
    case ETLG_AK_INT32: case ETLG_AK_FLOAT32: case ETLG_AK_DATE32: return 4;
    case ETLG_AK_INT64: case ETLG_AK_FLOAT64: case ETLG_AK_TIME64_US: case ETLG_AK_TIMESTAMP_US: case ETLG_AK_TIMESTAMP_US_UTC: return 8;
    case ETLG_AK_FIXED16: return 16;
    default: return 0;
  }
}
int32_t etlg_iceberg_plan(etlg_ctx* c, etlg_batch* b, int32_t slot, const etlg_outline_pass* passes, uint64_t n_passes, uint32_t passes_on_device,
                          const etlg_columns* changelog, uint32_t flags, etlg_ice_write* writes_out, uint64_t writes_cap, etlg_ice_slice* slices_out,
                          etlg_ice_window* windows_out, etlg_ice_plan_info* info) {
  if (!c || !b || b->ctx != c || !info) return ETLG_InvalidArgument;
  *info = etlg_ice_plan_info{};
  info->event = info->bad_pass = info->fail_pass = ~0ull;
  if (const int32_t rc = batch_ready(c, b, "etlg_iceberg_plan" NEEDS_DEVICE, ETLG_InvalidArgument)) return rc;
  if (!slot_known(c, slot)) return lib_error(c, ETLG_InvalidArgument, "unknown schema slot");
  if (n_passes && !passes) return lib_error(c, ETLG_InvalidArgument, "etlg_iceberg_plan: n_passes without passes");
  const bool copy = b->copy.active;
  if (copy && n_passes) return lib_error(c, ETLG_InvalidArgument, "etlg_iceberg_plan: a table-copy batch takes no passes (write_table_rows writes the rows of the whole call)");
  const etlg_batch_view& bv = b->v;
  const uint64_t n = bv.n_events;
  if (n_passes > (1ull << 38) || n > (1ull << 38)) return lib_error(c, ETLG_InvalidArgument, "etlg_iceberg_plan: more passes or events than one call takes (2^38: a grid of 2^30 workgroups walks them)");
  const etlg_columns* cl = changelog;
  if (!cl || !cl->changelog || cl->of_batch != b || cl->of_serial != b->serial || cl->of_slot != slot || !cl->v.on_device)
    return lib_error(c, ETLG_InvalidArgument, "etlg_iceberg_plan takes the object etlg_batch_iceberg built for this batch and slot, on the device (ETLG_F_OUTPUT_ON_DEVICE)");
  const uint64_t R = cl->v.n_rows;
  const uint32_t nc = cl->v.n_cols;
  static_assert(sizeof(etlg_ice_write) == 8 * kIcpWriteWords && sizeof(etlg_ice_window) == 8 * kIcpWinWords && sizeof(etlg_ice_slice) == 8 * kIcpSliceWords &&
                    sizeof(etlg_outline_pass) == 56 && sizeof(IcpCol) == 56 && sizeof(IcpBitmap) == 16,
                "k_icp_emit / k_icp_windows write 7, 7 and 6 words; the windows are words 0 and 1 of 7; icp_layout sizes the records");
  if (!copy && (!n_passes || !n)) return ETLG_OK;   // no window, or no event a window could hold: no member, no write
  const bool on_dev = (flags & ETLG_F_OUTPUT_ON_DEVICE) != 0;
  if (!writes_out && !slices_out) writes_cap = 0;
  const uint64_t n_win = copy ? 1 : n_passes;
  const uint64_t E = std::min(writes_cap, copy ? std::min<uint64_t>(R, 1) : n_passes);   // what can be written at the most
  if (E > (1ull << 38) / ((uint64_t)nc + 1)) return lib_error(c, ETLG_InvalidArgument, "etlg_iceberg_plan: more slices than one call writes (2^38: lower writes_cap)");
  const uint64_t ne = copy ? 0 : n;                                // a table-copy batch walks no event
  uint64_t tile = c->icp_tile_test ? c->icp_tile_test : 2048u;
  while ((ne + tile - 1) / tile > (1ull << 30)) tile *= 2;   // (a grid's width; only a test's tile gets here)
  const uint64_t n_tiles = (ne + tile - 1) / tile;
  // the records: a bitmap joins the word space only when its column reports a bit to count
  std::vector<IcpCol> cols(nc);
  std::vector<IcpBitmap> bitmaps;
  uint64_t W = 0;
  const auto bitmap = [&](const uint8_t* p, uint64_t count, uint64_t bits) -> uint32_t {
    if (!count || !bits || !p) return kIcpNoBitmap;
    bitmaps.push_back(IcpBitmap{(const unsigned long long*)p, W});
    W += (bits + 63) / 64;
    return (uint32_t)(bitmaps.size() - 1);
  };
  for (uint32_t i = 0; i < nc; i++) {
    const etlg_column& k = cl->cols[i];
    IcpCol& o = cols[i];
    o.offsets = (const long long*)k.offsets; o.child_offsets = (const long long*)k.child_offsets; o.child_count = k.child_count;
    o.kind = k.arrow_kind; o.child_kind = k.child_kind; o.width = k.value_bytes; o.child_width = k.arrow_kind == ETLG_AK_LIST ? icp_fixed_width(k.child_kind) : 0u;
    o.bm_valid = bitmap(k.validity, k.null_count, R); o.bm_deferred = bitmap(k.deferred, k.deferred_count, R);
    o.bm_child = k.arrow_kind == ETLG_AK_LIST ? bitmap(k.child_validity, k.child_null_count, k.child_count) : kIcpNoBitmap;
  }
  const uint32_t n_bitmaps = (uint32_t)bitmaps.size();
  bitmaps.push_back(IcpBitmap{nullptr, W});   // the closing entry
  uint64_t wtile = c->icp_words_test ? c->icp_words_test : 1024u;
  while ((W + wtile - 1) / wtile > (1ull << 30)) wtile *= 2;
  const uint64_t n_wtiles = (W + wtile - 1) / wtile;
  const IcpLayout lay = icp_layout(ne, n_tiles, n_passes, n_win, E, nc, n_bitmaps, W, n_wtiles, writes_out != nullptr, slices_out != nullptr, windows_out != nullptr,
                                   !copy && !passes_on_device, !on_dev);
  hipStream_t s = c->stream;
  ScratchBlk blk{c};
  HIPCHK(c, blk_take(c, lay.total + 64, false, &blk.p, &blk.cap));
  uint8_t* d = (uint8_t*)blk.p;
  HIPCHK(c, hipMemsetAsync(d + lay.hdr, 0, 128, s));
  HIPCHK(c, hipMemsetAsync(d + lay.hdr + 32, 0xFF, 32, s));
  std::vector<uint8_t> up(lay.passes - lay.up_at);   // the column records | the bitmap records: one copy
  if (nc) memcpy(up.data() + (lay.cols - lay.up_at), cols.data(), (size_t)nc * sizeof(IcpCol));
  memcpy(up.data() + (lay.bitmaps - lay.up_at), bitmaps.data(), bitmaps.size() * sizeof(IcpBitmap));
  HIPCHK(c, hipMemcpyAsync(d + lay.up_at, up.data(), up.size(), hipMemcpyHostToDevice, s));
  if (!copy && !passes_on_device) HIPCHK(c, hipMemcpyAsync(d + lay.passes, passes, n_passes * 56, hipMemcpyHostToDevice, s));
  typedef unsigned long long* W64;
  IcpJob j{};
  j.ev_kind = bv.ev_kind; j.ev_flags = bv.ev_flags; j.ev_slot = bv.ev_schema_slot; j.ev_table = bv.ev_table_id;
  j.n_events = ne; j.passes = passes_on_device ? (const unsigned long long*)passes : (const unsigned long long*)(d + lay.passes); j.n_passes = n_passes;
  j.row_event = (const unsigned long long*)cl->v.row_event; j.n_rows = R;
  j.slot = (uint32_t)slot; j.table_id = c->slots[(size_t)slot]->desc.table_id; j.tile = (uint32_t)tile; j.n_tiles = (uint32_t)n_tiles;
  j.n_cols = nc; j.n_bitmaps = n_bitmaps; j.cols = (const IcpCol*)(d + lay.cols); j.bitmaps = (const IcpBitmap*)(d + lay.bitmaps);
  j.n_words = W; j.wtile = (uint32_t)wtile; j.n_wtiles = (uint32_t)n_wtiles;
  j.hdr = (W64)(d + lay.hdr); j.tsum = (W64)(d + lay.tsum); j.fsum = (W64)(d + lay.fsum); j.bsum = (W64)(d + lay.bsum); j.code = d + lay.code;
  j.pre = (W64)(d + lay.pre); j.fpre = (W64)(d + lay.fpre); j.bpre = (W64)(d + lay.bpre); j.wrow = (W64)(d + lay.wrow);
  j.slens = (uint32_t*)(d + lay.slens); j.spre = (const int64_t*)(d + lay.spre);
  j.writes_cap = E;
  j.writes_out = !writes_out ? nullptr : on_dev ? (W64)writes_out : (W64)(d + lay.s_writes);
  j.slices_out = !slices_out ? nullptr : on_dev ? (W64)slices_out : (W64)(d + lay.s_slices);
  j.windows_out = !windows_out ? nullptr : on_dev ? (W64)windows_out : (W64)(d + lay.s_wins);
  etlg_k_iceberg_plan(&j, (W64)(d + lay.sblk), E * ((uint64_t)nc + 1), s);
  uint64_t head[ICP_H_WORDS] = {};
  HIPCHK(c, hipMemcpyAsync(head, j.hdr, sizeof head, hipMemcpyDeviceToHost, s));
  std::vector<uint8_t> back;
  if (!on_dev && lay.total > lay.stage_at) { back.resize(lay.total - lay.stage_at); HIPCHK(c, hipMemcpyAsync(back.data(), d + lay.stage_at, back.size(), hipMemcpyDeviceToHost, s)); }
  HIPCHK(c, hipStreamSynchronize(s));   // the one stop
  if (head[ICP_H_BAD] != ~0ull) { info->status = ETLG_ICP_BAD_PASSES; info->bad_pass = head[ICP_H_BAD]; return ETLG_OK; }
  if (head[ICP_H_FAILED] != ~0ull) {
    info->status = ETLG_ICP_FAILED; info->event = head[ICP_H_FAILED] >> 3; info->reason = (uint32_t)(head[ICP_H_FAILED] & 7u); info->fail_pass = head[ICP_H_FAILPASS];
    return ETLG_OK;
  }
  if (head[ICP_H_NEEDSHOST] != ~0ull) { info->status = ETLG_ICP_NEEDS_HOST; info->event = head[ICP_H_NEEDSHOST]; info->fail_pass = head[ICP_H_NOROWPASS]; return ETLG_OK; }
  info->n_writes = head[ICP_H_WRITES]; info->n_members = head[ICP_H_MEMBERS]; info->n_rows = head[ICP_H_ROWS]; info->n_mixed = head[ICP_H_MIXED];
  if (!on_dev) {
    const uint64_t nw = info->n_writes < E ? info->n_writes : E;
    const auto staged = [&](size_t at) { return back.data() + (at - lay.stage_at); };
    if (writes_out && nw) memcpy(writes_out, staged(lay.s_writes), nw * 56);
    if (slices_out && nw && nc) memcpy(slices_out, staged(lay.s_slices), nw * nc * 56);
    if (windows_out) memcpy(windows_out, staged(lay.s_wins), n_win * 48);
  }
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
  std::vector<uint32_t> name_len(nc);   // the quoted identifier's length + " = "
  { const NdKeys k = dl_quoted_names(col_names, nc); for (uint32_t i = 0; i < nc; i++) name_len[i] = k.off[i + 1] - k.off[i] + 3; }
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

