// Part of host.cpp (included there, one translation unit): what runs a batch — arena download, scratch, side inputs, output arenas, the kernel ladder (plan -> fused / cells -> multi-pass), the control pre-pass (synchronous and pipelined), finish_batch (results, redo paths, carried state).

namespace {

// Copies a device-resident batch into host vectors and returns its OutSet to the pool.
int32_t download_batch(etlg_ctx* c, etlg_batch* b) {
  OutSet* os = b->dev;
  if (!os) return ETLG_OK;
  // The batch is complete when this runs (its result block has been read on the host), so the copies need no ordering against
  // the decode streams: they travel on a stream of their own and overlap the upload and decode of the batches issued after this
  // one (PCIe is full duplex: a host-to-host pipeline costs max(upload, download) per batch, not their sum).
  RC(ensure_stream(c, &c->d2h_stream));
  hipStream_t s = c->d2h_stream;
  etlg_batch_view& v = b->v;
  const size_t n = (size_t)v.n_events;
  // layout of the pinned block: 8-byte arrays first, then 4-byte, then bytes (every part 64-byte aligned)
  ScratchLayout lay;
  const size_t o_start = lay.take(n * 8), o_commit = lay.take(n * 8), o_ord = lay.take(n * 8), o_body = lay.take(n * 8);
  const size_t o_table = lay.take(n * 4), o_slot = lay.take(n * 4), o_kind = lay.take(n), o_flags = lay.take(n);
  const size_t o_fixed = lay.take((size_t)v.fixed_bytes), o_heap = lay.take((size_t)v.heap_bytes);
  const size_t total = lay.total() + 64;
  if (b->h_arena_cap < total) {
    if (b->h_arena) { c->harena_pool.emplace_back(b->h_arena, b->h_arena_cap); b->h_arena = nullptr; b->h_arena_cap = 0; }
    // smallest pooled block that fits, else a new one (rounded up so that similar batches can share it)
    size_t best = (size_t)-1;
    for (size_t i = 0; i < c->harena_pool.size(); i++)
      if (c->harena_pool[i].second >= total && (best == (size_t)-1 || c->harena_pool[i].second < c->harena_pool[best].second)) best = i;
    if (best != (size_t)-1) {
      b->h_arena = c->harena_pool[best].first; b->h_arena_cap = c->harena_pool[best].second;
      c->harena_pool.erase(c->harena_pool.begin() + (long)best);
    } else {
      const size_t cap = (total + (total >> 2) + 4095) & ~(size_t)4095;
      HIPCHK(c, hipHostMalloc((void**)&b->h_arena, cap, hipHostMallocDefault));
      b->h_arena_cap = cap;
    }
  }
  uint8_t* h = b->h_arena;
  const struct { size_t off; const DevBuf& d; size_t width; } arrays[] = {{o_kind, os->kind, 1}, {o_flags, os->flags, 1}, {o_table, os->table, 4}, {o_slot, os->slot, 4},
                                                                          {o_start, os->start, 8}, {o_commit, os->commit, 8}, {o_ord, os->ord, 8}, {o_body, os->body, 8}};
  if (n) for (const auto& a : arrays) HIPCHK(c, hipMemcpyAsync(h + a.off, a.d.p, n * a.width, hipMemcpyDeviceToHost, s));
  if (v.fixed_bytes) HIPCHK(c, hipMemcpyAsync(h + o_fixed, os->fixed.p, (size_t)v.fixed_bytes, hipMemcpyDeviceToHost, s));
  if (v.heap_bytes) HIPCHK(c, hipMemcpyAsync(h + o_heap, os->heap.p, (size_t)v.heap_bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  c->out_pool.push_back(os);
  b->dev = nullptr;
  v.on_device = 0;
  v.ev_kind = h + o_kind; v.ev_flags = h + o_flags; v.ev_table_id = (const uint32_t*)(h + o_table); v.ev_schema_slot = (const uint32_t*)(h + o_slot);
  v.ev_start_lsn = (const uint64_t*)(h + o_start); v.ev_commit_lsn = (const uint64_t*)(h + o_commit);
  v.ev_tx_ordinal = (const uint64_t*)(h + o_ord); v.ev_body_off = (const uint64_t*)(h + o_body);
  v.fixed = h + o_fixed; v.heap = h + o_heap;
  return ETLG_OK;
}

// ------------------------------------------------------------ decode orchestration
// Per-frame scratch of the multi-pass kernels (context-shared, grow-only): (re)binds the pointers of `p`.
int32_t setup_scratch(etlg_ctx* c, DecParams& p, int set) {
  const uint32_t nf = p.nframes, nblocks = p.nblocks;
  CtlSet& cs = c->sets[set];
  HIPCHK(c, cs.d_tag.ensure(nf + 16)); HIPCHK(c, cs.d_emit.ensure(nf + 16));
  HIPCHK(c, cs.d_ffixed.ensure((size_t)nf * 4 + 16)); HIPCHK(c, cs.d_fheap.ensure((size_t)nf * 4 + 16));
  HIPCHK(c, cs.d_blk32.ensure((size_t)(nblocks + 1) * 4 * 3 + 64));
  HIPCHK(c, cs.d_blk64.ensure((size_t)(nblocks + 1) * 8 * 5 + 64));
  p.f_tag = (uint8_t*)cs.d_tag.p; p.f_emit = (uint8_t*)cs.d_emit.p;
  p.f_fixed = (uint32_t*)cs.d_ffixed.p; p.f_heap = (uint32_t*)cs.d_fheap.p;
  p.blk_cnt = (uint32_t*)cs.d_blk32.p; p.blk_last = p.blk_cnt + (nblocks + 1); p.blk_ev = p.blk_last + (nblocks + 1);
  p.blk_fixed = (uint64_t*)cs.d_blk64.p; p.blk_heap = p.blk_fixed + (nblocks + 1); p.blk_payload = p.blk_heap + (nblocks + 1);
  return ETLG_OK;
}

// "The side inputs stand": nothing the last upload was built from has changed, and it holds no epochs of some batch's own control frames.
bool side_inputs_stand(const etlg_ctx* c) { return c->side_valid && !c->side_dirty && !c->slots_dirty && c->last_epochs.empty(); }

// A set that was uploaded on the other decode stream: the first kernels of stream `s` that read it wait for the copy (SideSet::synced,
// one bit per decode stream).
uint32_t side_stream_bit(const etlg_ctx* c, hipStream_t s) { return 1u << ((s == c->stream2 && c->stream2) ? 1 : 0); }
int32_t wait_for_side_upload(etlg_ctx* c, SideSet* ss, hipStream_t s) {
  const uint32_t bit = side_stream_bit(c, s);
  if (ss && !(ss->synced & bit)) { HIPCHK(c, hipStreamWaitEvent(s, ss->ready, 0)); ss->synced |= bit; }
  return ETLG_OK;
}

// Side inputs of one batch: table states + the shared-table-cache timeline (`eps`: the epochs its own Relation / DDL frames
// create) + schema slots + the fixed-width plan's tables. Re-uploaded only when they change, into a set no unfinished batch reads.
// The steps of build_side_inputs, in its order, and what they hand to each other:
struct SideBuild {
  etlg_ctx* c; etlg_batch* b; const std::vector<EpochRec>& eps;
  hipStream_t s;
  std::vector<DevTable> tv; std::vector<DevEpoch> ev; std::vector<int32_t> live;   // the records, and the slots a frame of this batch can decode against
  std::vector<DevSlot> ds; std::vector<DevCol> dc; std::vector<uint8_t> ce;       // slots, columns, one element-class byte per column
  std::vector<PlanTab> pt; std::vector<uint32_t> pc;                              // the fixed-width plan's tables and column words
  SideSet* ss = nullptr;

  void point(SideSet* set, uint32_t n_tables, uint32_t n_epochs) {
    DecParams& p = b->params;
    const uint8_t* d = (const uint8_t*)set->dev.p;
    p.tables = (const DevTable*)(d + set->o_tables); p.epochs = (const DevEpoch*)(d + set->o_epochs); p.n_tables = n_tables; p.n_epochs = n_epochs;
    p.slots = (const DevSlot*)(d + set->o_slots); p.cols = (const DevCol*)(d + set->o_cols);
    p.n_slots = set->n_slots; p.n_cols = set->n_cols;
    if (p.flags & kDecCopyRows) p.copy_slot = (int32_t)(std::lower_bound(c->last_live.begin(), c->last_live.end(), b->copy.slot) - c->last_live.begin());   // device index of the caller's slot
    side_use(b, set);
  }
  // nothing the side inputs are built from has changed since the last upload (the common case: one call per batch)
  bool unchanged() const { return eps.empty() && side_inputs_stand(c) && !b->have_snapshot && !b->copy.active; }
  void records() {   // tables (sorted by id) with their epochs in frame order, live slots, host slots -> device indexes
    std::map<uint32_t, DevTable> tabs;
    auto get = [&](uint32_t id) -> DevTable& {
      auto it = tabs.find(id);
      if (it == tabs.end()) { DevTable t{}; t.table_id = id; t.init_slot = -1; it = tabs.emplace(id, t).first; }
      return it->second;
    };
    for (auto& kv : c->states) { DevTable& t = get(kv.first); t.state_kind = (uint32_t)kv.second.kind; t.state_lsn = kv.second.lsn; }
    const ControlState& cs0 = b->have_snapshot ? b->snapshot : c->cs;  // cache as of batch start
    for (auto& kv : cs0.cache) { DevTable& t = get(kv.first); t.init_kind = kv.second.kind; t.init_slot = kv.second.slot; }
    for (auto& e : eps) get(e.table_id);
    for (auto& kv : tabs) {
      DevTable t = kv.second;
      t.ep_begin = (uint32_t)ev.size();
      for (auto& e : eps) if (e.table_id == t.table_id) ev.push_back(e.ep);  // already in frame order
      t.ep_end = (uint32_t)ev.size();
      tv.push_back(t);
    }
    for (auto& t : tv) if (t.init_kind == 2u && t.init_slot >= 0) live.push_back(t.init_slot);
    for (auto& e : ev) if (e.kind == 2u && e.slot >= 0) live.push_back(e.slot);
    if (b->copy.active && b->copy.slot >= 0) live.push_back(b->copy.slot);
    std::sort(live.begin(), live.end());
    live.erase(std::unique(live.begin(), live.end()), live.end());
    auto dev_index = [&](int32_t host_slot) -> int32_t {   // position in `live`; -1 stays -1
      if (host_slot < 0) return host_slot;
      return (int32_t)(std::lower_bound(live.begin(), live.end(), host_slot) - live.begin());
    };
    for (auto& t : tv) if (t.init_kind == 2u) t.init_slot = dev_index(t.init_slot);
    for (auto& e : ev) if (e.kind == 2u) e.slot = dev_index(e.slot);
  }
  bool same_as_last_upload() const {
    return c->side_valid && !c->slots_dirty && live == c->last_live && tv.size() == c->last_tables.size() && ev.size() == c->last_epochs.size() &&
           (tv.empty() || !memcmp(tv.data(), c->last_tables.data(), tv.size() * sizeof(DevTable))) &&
           (ev.empty() || !memcmp(ev.data(), c->last_epochs.data(), ev.size() * sizeof(DevEpoch)));
  }
  // the fixed-width plan (plan.hip): tables the apply worker owns outright, Ready for the whole batch, whose replicated columns are all
  // bool / int2 / int4 / int8 / oid
  void plan_tables() {
    if (!ev.empty() || c->worker != ETLG_WORKER_APPLY) return;
    for (const DevTable& t : tv) {  // tv is sorted by table id
      if (t.state_kind != ETLG_TS_READY || t.init_kind != 2u || t.init_slot < 0 || (size_t)t.init_slot >= live.size()) continue;
      const int32_t host_slot = live[(size_t)t.init_slot];   // (t.init_slot is the device index by now)
      if (host_slot < 0 || (size_t)host_slot >= c->slots.size()) continue;
      const SlotHost& sh = *c->slots[(size_t)host_slot];
      bool ok = sh.desc.n_cols > 0;
      for (auto& sc : sh.cols) if (!int_class(sc.type_class)) ok = false;
      if (!ok) continue;
      PlanTab e{};
      e.rel_id = t.table_id; e.slot = (uint32_t)host_slot; e.n_cols = sh.desc.n_cols; e.row_dwords = sh.desc.row_bytes_full / 4;   // (the plan writes the arena's id, it does not index the slot table)
      e.cols_base = (uint32_t)pc.size();
      for (auto& sc : sh.cols) pc.push_back((uint32_t)sc.type_class | ((uint32_t)(sc.nullable ? 1 : 0) << 8) | ((uint32_t)sc.off_full << 16));
      // Deletes by key (round 6): the key-layout row of the table, one key word per column (a key row never outgrows the full
      // row the tile's LDS is sized by). A table without an identity column, or with more of them than the key word has bits for, keeps key_dwords 0:
      // its Deletes give the batch up as before.
      e.n_ident = sh.desc.n_ident; e.key_dwords = sh.desc.n_ident && sh.desc.n_ident < 256 && sh.desc.row_bytes_key <= 255 * 4 ? sh.desc.row_bytes_key / 4 : 0;
      e.keys_base = (uint32_t)pc.size();
      for (auto& sc : sh.cols) pc.push_back(sc.identity ? (1u | ((uint32_t)sc.key_index << 8) | ((uint32_t)(sc.off_key / 4) << 24)) : 0u);
      pt.push_back(e);
    }
  }
  int32_t take_free_set() {   // one no unfinished batch reads (a batch that is decoded again lets go of the set its first attempt read)
    side_release(b);
    for (SideSet* x : c->side_sets) if (x->users == 0) { ss = x; break; }
    if (!ss) { ss = new SideSet(); c->side_sets.push_back(ss); HIPCHK(c, hipEventCreateWithFlags(&ss->ready, hipEventDisableTiming)); }
    return ETLG_OK;
  }
  // ETLG_F_CHECK_CELLS: the element class of every array column, in DevCol order (build_slots pushes no column for a dead slot),
  // stored directly behind the DevCol records (chk_elem_table, values.hip.h)
  int32_t element_classes() {
    ss->chk_any = false; ss->chk_maxc = 0;
    for (int32_t li : live) {
      if (li < 0 || (size_t)li >= c->slots.size()) continue;
      const SlotHost& sh = *c->slots[(size_t)li];
      bool any = false;
      for (const etlg_slot_col& sc : sh.cols) {
        ce.push_back(sc.type_class == ETLG_TC_ARRAY ? (uint8_t)etlg_array_elem_class(sc.type_oid) : (uint8_t)0);
        any |= sc.type_class == ETLG_TC_ARRAY || sc.type_class == ETLG_TC_JSON;
      }
      if (any) { ss->chk_any = true; ss->chk_maxc = std::max<uint32_t>(ss->chk_maxc, sh.desc.n_cols); }
    }
    if (ce.size() != dc.size()) return lib_error(c, ETLG_InvalidState, "side inputs: element classes and columns differ in number");
    return ETLG_OK;
  }
  int32_t upload() {   // ONE copy from the set's pinned block, `ready` recorded behind it
    const decode_plan::SideLayout lay = decode_plan::side_layout(tv.size(), ev.size(), ds.size(), dc.size(), pt.size(), pc.size());
    ss->o_tables = lay.tables; ss->o_epochs = lay.epochs; ss->o_slots = lay.slots; ss->o_cols = lay.cols; ss->o_ptabs = lay.ptabs; ss->o_pcols = lay.pcols;
    if (lay.total > ss->h_cap) {
      if (ss->h) (void)hipHostFree(ss->h);
      ss->h = nullptr; ss->h_cap = 0;
      const size_t want = lay.total + lay.total / 2 + 4096;
      HIPCHK(c, hipHostMalloc((void**)&ss->h, want, hipHostMallocDefault));
      ss->h_cap = want;
    }
    HIPCHK(c, ss->dev.ensure(ss->h_cap));
    auto put = [&](size_t at, const void* from, size_t bytes) { if (bytes) memcpy(ss->h + at, from, bytes); };
    put(lay.tables, tv.data(), tv.size() * sizeof(DevTable)); put(lay.epochs, ev.data(), ev.size() * sizeof(DevEpoch));
    put(lay.slots, ds.data(), ds.size() * sizeof(DevSlot)); put(lay.cols, dc.data(), dc.size() * sizeof(DevCol)); put(lay.elems, ce.data(), ce.size());
    put(lay.ptabs, pt.data(), pt.size() * sizeof(PlanTab)); put(lay.pcols, pc.data(), pc.size() * 4);
    HIPCHK(c, hipMemcpyAsync(ss->dev.p, ss->h, lay.total, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipEventRecord(ss->ready, s));
    ss->synced = side_stream_bit(c, s);
    ss->n_slots = (uint32_t)ds.size(); ss->n_cols = (uint32_t)dc.size();
    c->side_cur = ss;
    c->last_tables = tv; c->last_epochs = ev; c->side_valid = true;
    c->slots_dirty = false; c->last_live = live;
    return ETLG_OK;
  }
  void keep_plan_summary() {
    const decode_plan::PlanSummary ps = decode_plan::plan_summary(pt, pc, tv);
    c->n_plan_tabs = ps.n_tabs; c->plan_max_row = ps.max_row; c->plan_uniform_dw = ps.uniform_dw; c->plan_uniform_key_dw = ps.uniform_key_dw;
    c->plan_key_below = ps.key_below; c->plan_key_max = ps.key_max; c->plan_covers_all = ps.covers_all;
  }
};

int32_t build_side_inputs(etlg_ctx* c, etlg_batch* b, const std::vector<EpochRec>& eps) {
  SlowScope slow_scope_build_side_inputs(c, "build_side_inputs");
  SideBuild sb{c, b, eps, c->stream};
  if (sb.unchanged()) {
    sb.point(c->side_cur, (uint32_t)c->last_tables.size(), 0u);
    b->any_sync_done = c->last_any_sync_done;
    return ETLG_OK;
  }
  sb.records();
  if (!sb.same_as_last_upload()) {  // table states, the cache timeline or the slots changed: a new upload
    build_slots(c, sb.live, sb.ds, sb.dc);
    sb.plan_tables();
    RC(sb.take_free_set());
    RC(sb.element_classes());
    RC(sb.upload());
    sb.keep_plan_summary();
  }
  sb.point(c->side_cur, (uint32_t)sb.tv.size(), (uint32_t)sb.ev.size());
  // (decode_tail does the same wait for the batches whose side inputs are known before their stream is; a control-path batch learns its set here)
  RC(wait_for_side_upload(c, c->side_cur, sb.s));
  b->any_sync_done = false;
  for (auto& t : sb.tv) if (t.state_kind == ETLG_TS_SYNC_DONE) b->any_sync_done = true;
  c->last_any_sync_done = b->any_sync_done;
  if (!b->have_snapshot) c->side_dirty = false;   // built from the live control state
  return ETLG_OK;
}

// Output arrays (capacity bounds: one event per frame; rows bounded by the widest slot; truncate bodies by 2x frame bytes;
// heap by 2.5x input). Called again when the control path created wider slots.
int32_t setup_outputs(etlg_ctx* c, etlg_batch* b) {
  SlowScope slow_scope_setup_outputs(c, "setup_outputs");
  DecParams& p = b->params;
  if (!b->dev) b->dev = take_outset(c);
  OutSet* os = b->dev;
  // (table-copy rows decoded in place are sized like the Insert frames they would rewrite to: the bounds count on the five
  // header bytes a frame has per cell)
  const uint64_t blen = b->copy.active ? std::max<uint64_t>(b->len, b->copy.syn_len) : b->len;
  const decode_plan::OutCaps caps = decode_plan::out_caps(p.nframes, blen, max_row_bytes(c));
  const size_t evcap = caps.evcap;
  const uint64_t fixed_cap = caps.fixed_cap, heap_cap = caps.heap_cap;
  HIPCHK(c, os->kind.ensure(evcap)); HIPCHK(c, os->flags.ensure(evcap));
  HIPCHK(c, os->table.ensure(evcap * 4)); HIPCHK(c, os->slot.ensure(evcap * 4));
  HIPCHK(c, os->start.ensure(evcap * 8)); HIPCHK(c, os->commit.ensure(evcap * 8));
  HIPCHK(c, os->ord.ensure(evcap * 8)); HIPCHK(c, os->body.ensure(evcap * 8));
  // The fixed arena's bound follows the widest slot, which a stream with DDL keeps widening (ALTER TABLE ADD COLUMN): grown to the
  // exact bound each time, every arena of the pool was re-allocated again and again (hipFree + hipMalloc synchronise the device:
  // 1.9 ms per cfg5 batch, ETLG_HOST_TIMES). The context remembers the largest bound it has seen with head room, and every arena
  // that has to grow goes there at once.
  if (fixed_cap > c->fixed_hint) c->fixed_hint = fixed_cap + fixed_cap / 2;
  if (os->fixed.cap < fixed_cap) HIPCHK(c, os->fixed.ensure(std::max<uint64_t>(fixed_cap, c->fixed_hint)));
  HIPCHK(c, os->heap.ensure(heap_cap));
  p.ev_kind = (uint8_t*)os->kind.p; p.ev_flags = (uint8_t*)os->flags.p; p.ev_table = (uint32_t*)os->table.p; p.ev_slot = (uint32_t*)os->slot.p;
  p.ev_start = (uint64_t*)os->start.p; p.ev_commit = (uint64_t*)os->commit.p; p.ev_ord = (uint64_t*)os->ord.p; p.ev_body = (uint64_t*)os->body.p;
  p.fixed = (uint8_t*)os->fixed.p; p.heap = (uint8_t*)os->heap.p; p.fixed_cap = fixed_cap; p.heap_cap = heap_cap;
  return ETLG_OK;
}

// The fixed-width plan's eligibility by context — everything but the batch's own size and the back-off; no side effect.
// (copy_rows: table-copy rows; n_epochs: the batch's own control frames changed a table under it)
bool plan_possible(const etlg_ctx* c, bool copy_rows, uint32_t n_epochs) {
  if (c->plan_mode == 0 || (c->fused_kernel >= 0 && c->fused_kernel != 3)) return false;  // ETLG_PLAN=0 / a forced generic kernel
  if (!c->n_plan_tabs || !c->plan_covers_all || n_epochs || copy_rows || c->worker != ETLG_WORKER_APPLY || c->fused_dbg) return false;
  return c->plan_max_row <= 512;   // 64 rows of the widest table sit in LDS beside the staging window
}
// Should this batch try the fixed-width plan first? Consumes a turn of the back-off (plan_skip): once per batch.
bool plan_wanted(etlg_ctx* c, const etlg_batch* b) {
  const DecParams& p = b->params;
  if (!plan_possible(c, (p.flags & kDecCopyRows) != 0, p.n_epochs)) return false;
  if (p.nframes >= (1u << 29) || p.fixed_cap >= (1ull << 34)) return false;   // descriptor: mark 30 bits, fixed dwords 32 bits
  if (c->fused_kernel == 3) return true;
  if (c->plan_skip) { c->plan_skip--; return false; }  // backing off after a batch that did not conform
  return true;
}

// The optimistic first attempt's preparation: as if the batch held no Relation / DDL frame — side inputs (unchanged: no stream work),
// outputs, and whether the fixed-width plan goes first (b->plan_decided).
int32_t prepare_optimistic(etlg_ctx* c, etlg_batch* b) {
  b->params.flags |= kDecNoControl;
  RC(build_side_inputs(c, b, std::vector<EpochRec>()));
  RC(setup_outputs(c, b));
  b->plan_decided = plan_wanted(c, b) ? 1 : 0;
  return ETLG_OK;
}

// Look-back descriptor buffers: four in rotation. The launch of batch k uses buffer k mod 4 and zeroes the head of buffer
// (k + 2) mod 4, so the stream carries no memset between kernels (only when a buffer grows or a larger batch left a tail).
// Distance two, not one: batch k+1 may run BESIDE batch k on the second stream (it uses a buffer batch k-1 cleared, which
// completed before k+1 started), and the buffer k clears was last used by batch k-2, which completed before k started.
hipError_t sync_decode_streams(etlg_ctx* c) {
  const hipError_t e = hipStreamSynchronize(c->stream);
  return (e == hipSuccess && c->stream2) ? hipStreamSynchronize(c->stream2) : e;
}
int32_t take_descriptors(etlg_ctx* c, size_t dbytes, uint8_t** cur_out, uint8_t** oth_out) {
  SlowScope slow_scope_take_descriptors(c, "take_descriptors");
  hipStream_t s = c->stream;
  if (dbytes > c->desc_half) {
    const size_t half = (dbytes * 2 + 4095) & ~(size_t)4095;
    HIPCHK(c, sync_decode_streams(c));   // earlier launches may still be using the old buffer
    HIPCHK(c, c->d_desc.ensure(half * 4));
    HIPCHK(c, hipMemsetAsync(c->d_desc.p, 0, half * 4, s));
    HIPCHK(c, hipStreamSynchronize(s));
    c->desc_half = half; for (size_t& d : c->desc_dirty) d = 0;
  }
  const uint32_t cur = c->desc_cur & 3u, oth = (cur + 2u) & 3u;
  uint8_t* dcur = (uint8_t*)c->d_desc.p + cur * c->desc_half;
  uint8_t* doth = (uint8_t*)c->d_desc.p + oth * c->desc_half;
  if (c->desc_dirty[cur]) { HIPCHK(c, hipMemsetAsync(dcur, 0, c->desc_dirty[cur], s)); c->desc_dirty[cur] = 0; }
  c->desc_dirty[cur] = dbytes;                                   // this launch writes it
  if (c->desc_dirty[oth] <= dbytes) c->desc_dirty[oth] = 0;       // ... and clears that much of the one after next
  c->desc_cur = (cur + 1u) & 3u;
  *cur_out = dcur; *oth_out = doth;
  return ETLG_OK;
}

// ... for the q.ntiles tiles of a generic single-pass launch (k_fused, k_cells, k_rows): three words per tile and per group of 64, a ticket
int32_t take_tile_descriptors(etlg_ctx* c, FusedParams& q) {
  const size_t ngroups = (q.ntiles + 63) / 64;
  const size_t per = (size_t)q.ntiles + ngroups;  // tile descriptors followed by group descriptors
  const size_t dbytes = per * 8 * 3 + 64;
  uint8_t *dcur, *doth;
  RC(take_descriptors(c, dbytes, &dcur, &doth));
  q.d_txn = (unsigned long long*)dcur; q.d_outa = q.d_txn + per; q.d_outb = q.d_outa + per;
  q.ticket = (uint32_t*)(q.d_outb + per);
  q.d_clear = (unsigned long long*)doth; q.clear_words = (uint32_t)(dbytes / 8);
  return ETLG_OK;
}

// A batch whose decode was enqueued behind its boundary scan (DecParams.nframes_dev) and that now needs its frame count on the host — a
// kernel that does not read the count from the device, or a second attempt: the scan is waited for; when it did not hold (or the batch
// outgrew the bound its grids were sized by) the boundaries are scanned again, synchronously, with the hints / one-lane fallback of
// scan_collect. From here on the batch is an ordinary batch with a sidecar of its own.
int32_t resolve_scan_count(etlg_ctx* c, etlg_batch* b) {
  if (!b->scan_chained) return ETLG_OK;
  DecParams& p = b->params;
  HIPCHK(c, hipStreamSynchronize(b->scan_s));
  uint32_t res[4] = {0, 1, 0, 0};
  HIPCHK(c, hipMemcpy(res, b->d_scan_res, 16, hipMemcpyDeviceToHost));
  size_t nframes = res[0];
  if (res[1] != 0 || res[2] != 0 || nframes == 0) {   // (a count beyond the bound with no flag raised: the offsets are complete — the buffer holds len / 24 + 1024 of them — only the grids were too small)
    HIPCHK(c, sync_decode_streams(c));   // (nothing may still be reading the offsets this scan rewrites)
    HIPCHK(c, device_scan(c, b->d_in_ptr, b->len, &nframes, c->stream, *b->scan_offs));
    RC(batch_too_large(c, 0, nframes));
    p.offs = (const uint32_t*)b->scan_offs->p;
    b->user_offs = p.offs;
    if (res[2] != 0) {
      // the run that did not hold left its hints, and nobody collected it (scan_collect cleans up after the runs it makes itself). Hints are
      // only guesses — a scan checks every one against the chain — but stale ones cost every later scan a second run: clean now
      const size_t ntiles = (b->len + etlg_k_bounds_tile_bytes() - 1) / etlg_k_bounds_tile_bytes();
      HIPCHK(c, hipMemsetAsync((uint8_t*)c->d_scan.p + c->scan_half, 0xFF, std::min(ntiles, c->scan_tiles_cap) * 4, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
    }
  }
  const bool outgrown = nframes > p.nframes;
  p.nframes = (uint32_t)nframes; p.nblocks = ((uint32_t)nframes + kBlock - 1) / kBlock;
  p.nframes_dev = nullptr;
  b->scan_chained = false;
  if (outgrown) RC(setup_outputs(c, b));   // (the event arrays and the arena were sized by the bound)
  c->scan_last_nf = nframes; c->scan_last_len = b->len;
  return ETLG_OK;
}

// ---- the single-pass kernels of the ladder: enqueue_single puts ONE of them over the batch — level 0 = the fixed-width plan (plan.hip),
// level 1 = k_rows (rows.hip) where it may run, else the generic fused kernel (fused.hip) or, for wide frames, the column-parallel one
// (cells.hip). The numbers of every launch come from decode_plan.h.

// The average frame a launch's LDS windows are sized by (decoded behind its scan: params.nframes is a bound, the stream's estimate counts)
uint64_t avg_frame_of(const etlg_batch* b) {
  return decode_plan::avg_frame(b->len, b->scan_chained && b->nf_est ? b->nf_est : b->params.nframes);
}

// Prefixes of the sidecar pre-pass go to a buffer of their own, four in rotation like the look-back descriptors and for the same reason:
// batch k + 1 runs beside batch k on the other decode stream, batch k - 2 is complete before k starts. The pre-pass runs on the batch's own
// decode stream — with two decode streams that is beside the decode of the batch BEFORE. (A stream of its own at the highest priority,
// eight buffers, the pre-pass up to six batches ahead: 1 355 GB/s against 1 698 on the bench's chain — the events it takes cost
// the host more than the overlap gains; profiles/r04_plan_development.json.)
int32_t take_pre_buffer(etlg_ctx* c, size_t pbytes, PlanParams& q) {
  constexpr uint32_t NB = etlg_ctx::kPreBufs;
  if (pbytes > c->pre_half) {
    HIPCHK(c, sync_decode_streams(c));
    const size_t half = (pbytes * 2 + 4095) & ~(size_t)4095;
    HIPCHK(c, c->d_pre.ensure(half * NB));
    HIPCHK(c, hipMemsetAsync(c->d_pre.p, 0, half * NB, c->stream));   // tickets start at zero (every launch leaves its own that way), no word carries a status tag
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->pre_half = half;
  }
  const decode_plan::PreSlot ps = decode_plan::pre_slot(c->pre_seq++, NB);
  uint8_t* pbuf = (uint8_t*)c->d_pre.p + (size_t)ps.slot * c->pre_half;
  q.pre_ticket = (uint32_t*)pbuf;
  q.pre_out = (unsigned long long*)(pbuf + 64);
  q.pre_tag = ps.tag;
  return ETLG_OK;
}

int32_t enqueue_plan(etlg_ctx* c, etlg_batch* b) {
  const DecParams& p = b->params;
  PlanParams& q = c->pq;
  const decode_plan::PlanGeom g = decode_plan::plan_geom(p.nframes, avg_frame_of(b), c->plan_margin_pct, c->plan_max_row, etlg_k_plan_pre_group_log());
  q.ntiles = g.ntiles; q.rows_off = g.rows_off; q.lds_bytes = g.lds_bytes; q.max_row_dw = g.max_row_dw;
  q.n_tabs = c->n_plan_tabs; q.tabs = (const PlanTab*)((const uint8_t*)b->side->dev.p + b->side->o_ptabs); q.cols = (const uint32_t*)((const uint8_t*)b->side->dev.p + b->side->o_pcols);
  q.dbg = c->plan_dbg;
  // the sidecar pre-pass (k_plan_pre, plan.hip) leaves every tile's prefix in memory: the decode kernel
  // then has no look-back. Needs one row size for all planned tables (a frame is priced by its length alone).
  const bool pre = c->plan_pre != 0 && c->plan_uniform_dw != 0;
  q.desc = nullptr; q.d_clear = nullptr; q.clear_words = 0;
  if (!pre) {   // (behind the pre-pass no kernel reads or writes a look-back word: no buffer is taken, none is cleared)
    uint8_t *dcur, *doth;
    RC(take_descriptors(c, g.dbytes, &dcur, &doth));
    q.desc = (unsigned long long*)dcur;
    q.d_clear = (unsigned long long*)doth; q.clear_words = (uint32_t)(g.dbytes / 8);
  }
  q.pre = nullptr; q.pre_out = nullptr; q.pre_ticket = nullptr; q.pre_tag = 0; q.pre_row_dw = c->plan_uniform_dw;
  q.pre_key_dw = c->plan_uniform_key_dw; q.pre_key_below = c->plan_deletes ? c->plan_key_below : 0u; q.pre_key_max = c->plan_deletes ? c->plan_key_max : 0u;
  if (pre) {
    RC(take_pre_buffer(c, g.pbytes, q));
    launch(c, kPlanPre, p);
    q.pre = q.pre_out;
    if (c->plan_pre == 1) q.dbg |= 512u;   // one tile per wave: without the look-back nothing is gained from a single lock-step round
  }
  launch(c, kPlan, p);
  b->used_fused = true; b->used_cells = false;
  return ETLG_OK;
}

// What the kernels of level 1 are chosen by: the widest live slot, whether k_cells can run (it keeps the side tables in LDS: FusedParams::
// side_bytes, set here), the average frame, and whether the batch is table-copy rows decoded in place.
struct GenericFacts { uint32_t widest = 1; bool cells_ok = false, direct = false; uint64_t avg = 0; };
int32_t generic_facts(etlg_ctx* c, etlg_batch* b, GenericFacts& f) {
  const DecParams& p = b->params;
  FusedParams& q = c->fq;
  q.side_bytes = decode_plan::side_lds_bytes(p.n_tables, p.n_epochs, p.n_slots, p.n_cols, (c->fused_dbg & 16) != 0);
  for (int32_t li : c->last_live) f.widest = std::max<uint32_t>(f.widest, c->slots[(size_t)li]->desc.n_cols);
  f.cells_ok = f.widest <= etlg_k_cells_maxc() && q.side_bytes != 0;
  // table-copy rows: the rows -> arena kernel is k_cells with another first phase; where k_cells cannot run (or another kernel is
  // forced) the rows are rewritten as Insert frames first
  if (b->copy.active && b->copy.direct && (!f.cells_ok || c->fused_kernel >= 0)) RC(copy_use_frames(c, b));
  f.direct = b->copy.active && b->copy.direct;
  f.avg = avg_frame_of(b);
  return ETLG_OK;
}

// The row-synchronous kernel (rows.hip) takes the batches k_cells / k_fused-64 would: WAL frames (not table-copy rows), no table in SyncDone
// state (ownership would need the transaction look-back before the slots), tables of up to 64 columns. *taken: it was enqueued.
int32_t try_enqueue_rows(etlg_ctx* c, etlg_batch* b, const GenericFacts& f, bool* taken) {
  const DecParams& p = b->params;
  FusedParams& q = c->fq;
  uint32_t maxh = 1, maxh_old = 0, maxrow = 16;
  bool ok = !b->copy.active && !(p.flags & kDecCopyRows) && !b->any_sync_done && !(c->fused_dbg & ~(8u | 32u)) && q.side_bytes != 0 && ((uintptr_t)p.in & 15) == 0 &&
            f.widest <= etlg_k_rows_max_cols() && !b->no_rows && c->rows_mode != 0 && (c->fused_kernel < 0 || c->fused_kernel == 4);
  for (int32_t li : c->last_live) {
    const SlotHost& sh = *c->slots[(size_t)li];
    uint32_t nh = 0, nhi = 0;
    for (auto& sc : sh.cols) if (!heapless_class(sc.type_class)) { nh++; if (sc.identity) nhi++; }
    maxh = std::max(maxh, nh); maxh_old = std::max(maxh_old, nhi);
    maxrow = std::max<uint32_t>(maxrow, sh.desc.row_bytes_full + std::max<uint32_t>(sh.desc.row_bytes_key, sh.desc.n_ident == sh.desc.n_cols ? sh.desc.row_bytes_full : 0u));
  }
  if (maxh > etlg_k_rows_max_heap_cols()) ok = false;
  if (ok && c->fused_kernel != 4 && c->rows_skip) { c->rows_skip--; ok = false; }   // backing off after a batch that was handed back
  if (!ok) return ETLG_OK;
  const uint64_t stat = etlg_k_rows_static_lds();
  const uint64_t max_wgs = 4ull * (uint64_t)etlg_k_rows_waves_per_simd() / (uint64_t)etlg_k_rows_waves();   // (the register file: ETLG_ROWS_MINBLOCKS waves per SIMD)
  const decode_plan::RowsChoice r = decode_plan::rows_choice(decode_plan::RowsIn{f.avg, maxrow, maxh, maxh_old, f.widest, q.side_bytes, stat, c->rows_win_min, c->rows_cf, max_wgs},
                                                             etlg_k_rows_table_bytes);
  if (!r.taken) {
    if (c->rows_trace) fprintf(stderr, "[rows] not taken: cf %u need %llu maxrow %u widest %u avg %llu\n", r.cf, (unsigned long long)r.need, maxrow, f.widest, (unsigned long long)f.avg);
    return ETLG_OK;
  }
  q.blk = r.cf; q.maxc = f.widest; q.rows_maxh_old = maxh_old; q.rows_maxh = maxh;
  q.lds_bytes = r.lds_bytes;
  q.seq_lookback = 0; q.in_aligned = 1; q.dbg = c->fused_dbg; q.copy_rel = 0;
  q.ntiles = (p.nframes + r.cf - 1) / r.cf;
  RC(take_tile_descriptors(c, q));
  if (c->rows_lds >= 0) q.lds_bytes = (uint32_t)c->rows_lds;   // (ETLG_ROWS_LDS, experiments)
  if (c->rows_trace) fprintf(stderr, "[rows] cf %u maxc %u maxh %u lds %u (static %llu) side %u tables %llu need %llu (window min %llu, avg frame %llu) -> %d workgroups per CU by the runtime's count, %llu planned\n", r.cf, f.widest, maxh, q.lds_bytes, (unsigned long long)stat, q.side_bytes, (unsigned long long)r.tabb, (unsigned long long)r.need, (unsigned long long)c->rows_win_min, (unsigned long long)f.avg, etlg_k_rows_occupancy(q.lds_bytes), (unsigned long long)r.wgs);
  launch(c, kRows, p);
  launch_chk_cells(c, b);
  b->used_fused = true; b->used_cells = false; b->used_rows = true;
  *taken = true;
  return ETLG_OK;
}

int32_t enqueue_generic(etlg_ctx* c, etlg_batch* b, const GenericFacts& f, int kernel) {   // k_fused / k_cells / k_copy_cells
  const DecParams& p = b->params;
  FusedParams& q = c->fq;
  const bool use_cells = kernel == 2;
  q.blk = kernel == 0 ? 256u : 64u;
  q.maxc = f.widest;
  const uint64_t stat = !use_cells ? 0 : f.direct ? etlg_k_copy_cells_static_lds(f.widest) : etlg_k_cells_static_lds(f.widest);
  q.lds_bytes = decode_plan::generic_window(kernel, f.avg, c->lds_margin_pct, f.direct, q.side_bytes, use_cells && !f.direct ? etlg_k_cells_table_bytes(f.widest) : 0,
                                            use_cells && !f.direct ? etlg_k_cells_lds_floor(f.widest) : 0, stat, [&](uint32_t window) { return etlg_k_copy_cells_lds(f.widest, window); });
  q.seq_lookback = (b->any_sync_done || (c->fused_dbg & 32)) ? 1u : 0u;
  q.ntiles = (p.nframes + q.blk - 1) / q.blk;
  q.in_aligned = ((uintptr_t)p.in & 15) == 0;
  q.dbg = c->fused_dbg;
  RC(take_tile_descriptors(c, q));
  q.copy_rel = f.direct ? b->copy.rel_id : 0u;
  launch(c, f.direct ? kCopyCells : use_cells ? kCells : kFused, p);
  launch_chk_cells(c, b);
  b->used_fused = true;
  b->used_cells = use_cells;
  return ETLG_OK;
}

int32_t enqueue_single(etlg_ctx* c, etlg_batch* b, int level) {
  SlowScope slow_scope_enqueue_single(c, "enqueue_single");
  if (b->scan_chained && level != 0) RC(resolve_scan_count(c, b));   // (only the plan kernels read the count on the device)
  b->level = level;
  b->used_rows = false;
  if (level == 0) return enqueue_plan(c, b);
  GenericFacts f;
  RC(generic_facts(c, b, f));
  bool any_var = false;   // a table the batch may carry has TEXT / NUMERIC / ... columns: one lane per frame crawls on those
  for (int32_t li : c->last_live) for (auto& sc : c->slots[(size_t)li]->cols) if (!fixed_class(sc.type_class)) any_var = true;
  const int kernel = decode_plan::generic_kernel(f.avg, any_var, f.cells_ok, c->fused_kernel, f.direct);
  if (kernel != 0 || c->fused_kernel == 4) {
    bool taken = false;
    RC(try_enqueue_rows(c, b, f, &taken));
    if (taken) return ETLG_OK;
  }
  return enqueue_generic(c, b, f, kernel);
}

// The control pre-pass, device half: classify + transaction scan + compaction of the R / M frames (k_ctrl_list also gathers their
// bytes), then the result block, the head of the list and the head of the gathered bytes to pinned memory WITHOUT asking for their
// sizes first (one round trip instead of three; what does not fit is fetched afterwards). `ahead`: on the control stream, beside the
// decode of the batch before (etlg_decode); otherwise on the context's stream, collected at once (run_control_pass).
int32_t ctl_begin(etlg_ctx* c, etlg_batch* b, DecParams& p, hipStream_t s, bool ahead) {
  SlowScope slow_scope_ctl_begin(c, "ctl_begin");
  StreamSwitch sw{c, c->stream};
  c->stream = s;
  const uint32_t nf = p.nframes;
  // which set of buffers this pre-pass writes: a pre-pass that runs ahead takes them in turn (two may be in flight, etlg_decode); one
  // that is collected at once takes set 0 — behind whatever is still running on the control stream
  const int set = ahead ? b->ctl_set : 0;
  if (!ahead) { b->ctl_set = 0; if (c->ctl_stream) HIPCHK(c, hipStreamSynchronize(c->ctl_stream)); }
  CtlSet& cs = c->sets[set];
  if (!cs.h_ctl_list) {
    HIPCHK(c, hipHostMalloc((void**)&cs.h_ctl_list, sizeof(CtrlFrame) * etlg_ctx::kCtlListCap, hipHostMallocDefault));
    HIPCHK(c, hipHostMalloc((void**)&cs.h_ctl_stage, etlg_ctx::kCtlStageCap, hipHostMallocDefault));
  }
  if (ahead) {
    if (c->mp_tail_set) { HIPCHK(c, hipStreamWaitEvent(s, c->mp_tail, 0)); c->mp_tail_set = false; }   // the multi-pass kernels share the per-frame scratch
    RC(take_result(c, &b->h_ctl));
    RC(take_event(c, &b->ctl_ev));
    HIPCHK(c, hipMemcpyAsync(p.res, c->d_init_ring, sizeof(DevResult), hipMemcpyDeviceToDevice, s));
  }
  RC(setup_scratch(c, p, set));
  launch(c, 0, p);
  launch(c, 1, p);
  HIPCHK(c, cs.d_ctrl.ensure((size_t)nf * sizeof(CtrlFrame) + 64));
  p.ctrl = (CtrlFrame*)cs.d_ctrl.p; p.ctrl_cap = nf;
  {  // room for the control frames' bytes: a batch rarely carries more than a few hundred KB of them
    size_t want = std::min<size_t>(std::max<size_t>(b->len / 16, 64 << 10), 8 << 20);
    if (c->ctrl_stage_cap_test) want = c->ctrl_stage_cap_test;   // ETLG_CTRL_STAGE_CAP (tests): a staging buffer too small for the batch's control frames
    HIPCHK(c, cs.d_ctrl_stage.ensure(want));
    p.ctrl_stage = (uint8_t*)cs.d_ctrl_stage.p; p.ctrl_stage_cap = (uint32_t)want;
  }
  launch(c, 2, p);
  HIPCHK(c, hipMemcpyAsync(ahead ? b->h_ctl : b->h_res, p.res, sizeof(DevResult), hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(cs.h_ctl_list, cs.d_ctrl.p, (size_t)std::min<uint32_t>(nf, etlg_ctx::kCtlListCap) * sizeof(CtrlFrame), hipMemcpyDeviceToHost, s));
  if (b->in_dev) HIPCHK(c, hipMemcpyAsync(cs.h_ctl_stage, cs.d_ctrl_stage.p, std::min<size_t>(p.ctrl_stage_cap, etlg_ctx::kCtlStageCap), hipMemcpyDeviceToHost, s));
  if (ahead) { HIPCHK(c, hipEventRecord(b->ctl_ev, s)); b->ctl_started = true; }
  return ETLG_OK;
}

// One Relation / DDL frame through the host control plane (handle_relation / handle_ddl): the frame's bytes from its CopyData envelope on.
HostErr apply_ctrl_frame(etlg_ctx* c, const CtrlFrame& cf, const uint8_t* fr, size_t flen, std::vector<EpochRec>& eps) {
  // classify guaranteed 'd' len 'w' hdr tag: body starts at +31
  uint64_t wal_start = 0;
  for (int k = 0; k < 8; k++) wal_start = wal_start << 8 | fr[6 + k];
  return cf.tag == 'R' ? handle_relation(c, cf, fr + 31, flen - 31, eps) : handle_ddl(c, cf, wal_start, fr + 31, flen - 31, eps);
}

// The control pre-pass of one batch (device half above, unless it ran ahead), then the host control plane (handle_relation /
// handle_ddl) in frame order. Fills b->ctrl / ctrl_raw, `eps`, the host error of the batch.
int32_t run_control_pass(etlg_ctx* c, etlg_batch* b, std::vector<EpochRec>& eps) {
  SlowScope slow_scope_run_control_pass(c, "run_control_pass");
  hipStream_t s = c->stream;
  const uint32_t nf = b->params.nframes;
  ht_start(c);
  b->snapshot = c->cs; b->have_snapshot = true; b->snap_gen = c->cs_gen;
  b->ctrl.clear(); b->ctrl_raw.clear();
  b->host_err_code = 0; b->host_err_frame = -1; b->host_err_rank = 0;
  b->ctrl_done = true;
  if (!nf) return ETLG_OK;
  const bool ahead = b->ctl_started;
  DecParams& p = ahead ? b->ctl_params : b->params;
  if (ahead) {
    HIPCHK(c, hipEventSynchronize(b->ctl_ev));
    s = c->ctl_stream;   // what did not fit the pinned heads is fetched on the stream the pre-pass ran on
  } else {
    RC(ctl_begin(c, b, p, s, false));
    HIPCHK(c, hipStreamSynchronize(s));
  }
  ht_mark(c, 0);
  const DevResult& cr = ahead ? *b->h_ctl : *b->h_res;
  const CtlSet& cs = c->sets[b->ctl_set];   // (the set this batch's pre-pass wrote)
  const uint32_t nctrl = std::min<uint32_t>(cr.n_ctrl, p.ctrl_cap);
  if (!nctrl) return ETLG_OK;
  std::vector<CtrlFrame>& ctrl = b->ctrl;
  ctrl.resize(nctrl);
  const uint32_t nhead = std::min<uint32_t>(nctrl, etlg_ctx::kCtlListCap);
  memcpy(ctrl.data(), cs.h_ctl_list, (size_t)nhead * sizeof(CtrlFrame));
  if (nctrl > nhead) HIPCHK(c, hipMemcpy(ctrl.data() + nhead, (const CtrlFrame*)cs.d_ctrl.p + nhead, (size_t)(nctrl - nhead) * sizeof(CtrlFrame), hipMemcpyDeviceToHost));
  std::sort(ctrl.begin(), ctrl.end(), [](const CtrlFrame& a, const CtrlFrame& b2) { return a.frame < b2.frame; });
  ht_mark(c, 1);
  // the frames' bytes: already on the host, or the gathered copy k_ctrl_list left in the staging buffer (its head is in pinned
  // memory already); a frame that did not fit there is fetched from the input by itself
  std::vector<uint8_t> stage, extra;
  std::vector<size_t> at(nctrl + 1, 0);
  for (uint32_t i = 0; i < nctrl; i++) at[i + 1] = at[i] + (ctrl[i].stage_off == 0xFFFFFFFFu ? ctrl[i].o1 - ctrl[i].o0 : 0u);
  const uint8_t* staged_bytes = cs.h_ctl_stage;
  if (b->in_dev) {
    const uint32_t staged = std::min<uint32_t>(cr.ctrl_bytes, p.ctrl_stage_cap);
    bool wait = false;
    if (staged > etlg_ctx::kCtlStageCap) {   // more gathered bytes than the pinned head holds: one copy of everything
      stage.resize((size_t)staged + 16);
      HIPCHK(c, hipMemcpyAsync(stage.data(), cs.d_ctrl_stage.p, staged, hipMemcpyDeviceToHost, s));
      staged_bytes = stage.data(); wait = true;
    }
    extra.resize(at[nctrl] + 16);
    for (uint32_t i = 0; i < nctrl; i++)
      if (ctrl[i].stage_off == 0xFFFFFFFFu && ctrl[i].o1 > ctrl[i].o0) {
        HIPCHK(c, hipMemcpyAsync(extra.data() + at[i], b->dev_in + ctrl[i].o0, ctrl[i].o1 - ctrl[i].o0, hipMemcpyDeviceToHost, s));
        wait = true;
      }
    if (wait) HIPCHK(c, hipStreamSynchronize(s));
  }
  ht_mark(c, 2);
  for (uint32_t i = 0; i < nctrl; i++) {
    const CtrlFrame& cf = ctrl[i];
    const uint8_t* fr = !b->in_dev ? b->host_in + cf.o0 : cf.stage_off != 0xFFFFFFFFu ? staged_bytes + cf.stage_off : extra.data() + at[i];
    const size_t flen = cf.o1 - cf.o0;
    b->ctrl_raw.emplace_back(fr, fr + flen);
    const HostErr he = apply_ctrl_frame(c, cf, fr, flen, eps);
    if (he.code) { b->host_err_code = he.code; b->host_err_frame = cf.frame; b->host_err_rank = he.rank; b->params.host_err_frame = cf.frame; break; }
  }
  ht_mark(c, 3);
  return ETLG_OK;
}

// The path that knows about control frames: control pre-pass (unless the caller asserted there are none), side inputs with
// the batch's own epochs, then the generic single-pass kernel or — forced, oversized, or behind a host error — the
// multi-pass kernels. Synchronous callers only (immediate carry).
int32_t standard_path(etlg_ctx* c, etlg_batch* b) {
  SlowScope slow_scope_standard_path(c, "standard_path");
  DecParams& p = b->params;
  const uint32_t nf = p.nframes;
  std::vector<EpochRec> eps;
  p.flags &= ~kDecNoControl;
  if (b->user_no_ctrl) p.flags |= kDecNoControl;
  else { RC(run_control_pass(c, b, eps)); c->path_n[kPathControl]++; b->n_slots_view = c->slots.size(); }
  b->eps_saved = eps;
  ht_start(c);
  RC(build_side_inputs(c, b, eps));
  ht_mark(c, 4);
  RC(setup_outputs(c, b));
  ht_mark(c, 5);
  // (always the generic kernel: the fixed-width plan behind a control pass gave wrong ddl_fixed batches on the MI355X and gained one batch
  // per stream — measured and dropped in round 6, profiles/r06zw_plan_behind_control_dropped.txt)
  if (nf && !b->host_err_code && single_pass_ok(c, b->len)) { const int32_t rc = enqueue_single(c, b, 1); ht_mark(c, 6); return rc; }
  if (p.carry) {
    // chained to a batch in flight and in need of the multi-pass kernels (the host control plane failed on one of its frames): they
    // take the carried state from the host. The batch is marked "did not run" — the batches behind it stop at that — and is decoded
    // when it is synced, from the exact state (finish_batch, the forced re-run).
    DevResult poison = *c->h_init; poison.fused_fail = kFailNotRun;
    if (!c->h_poison) { HIPCHK(c, hipHostMalloc((void**)&c->h_poison, sizeof(DevResult), hipHostMallocDefault)); *c->h_poison = poison; }
    HIPCHK(c, hipMemcpyAsync(b->d_res_blk, c->h_poison, sizeof(DevResult), hipMemcpyHostToDevice, c->stream));
    b->level = 1; b->used_fused = true; b->used_cells = false;
    return ETLG_OK;
  }
  // The multi-pass kernels take scratch set 0 on the decode stream. With ETLG_CTL_HOLD the pre-pass of the batch BEHIND this one went
  // out on the control stream before this (held) batch was flushed, and it may be writing the same set (the sets alternate per
  // pre-pass, not per batch that reaches this line): it finishes first. Rare path — a host control-plane error, or a forced /
  // oversized batch — so the wait costs nothing that matters.
  if (c->ctl_stream) HIPCHK(c, hipStreamSynchronize(c->ctl_stream));
  RC(setup_scratch(c, p));
  launch_multipass(c, p, b->ctrl_done && nf != 0 && !b->ctl_started);
  b->level = 2; b->used_fused = false; b->used_cells = false;
  return ETLG_OK;
}

// Finishes every pending ASYNC batch, oldest first.
// ---- the states of a batch, made explicit (VERDICT r5 #8). The flags of etlg_batch carry them; this is the one place that names the
// combinations, and — with ETLG_DEBUG_INVARIANTS=1 — checks what must hold between the entry points (etlg_decode, etlg_batch_sync):
//
//   BUILDING            etlg_decode is assembling it (not pending, not finished): never visible between calls
//   SCAN_DEFERRED       ASYNC without a sidecar, boundary scan in flight, decode NOT enqueued (etlg_ctx::deferred names it; at most one,
//                       always the newest batch); the next call on the context enqueues its decode (flush_deferred)
//   CTL_HELD            default flags behind a control batch: its control pre-pass runs ahead, decode not enqueued (the same pointer)
//   ISSUED              first attempt enqueued, result block in flight
//   ISSUED_BEHIND_SCAN  ... enqueued behind its own boundary scan, frame count read on the device (params.nframes_dev)
//   POISONED            ISSUED, but a batch before it in the chain was decoded again: what it produced started from the wrong state;
//                       it is decoded again when it is finished (force_rerun)
//   FINISHED            result read, view filled, rc set; owned by the caller until etlg_batch_free
//
// Transitions: BUILDING -> {SCAN_DEFERRED, CTL_HELD, ISSUED, ISSUED_BEHIND_SCAN} (etlg_decode, ASYNC) | FINISHED (synchronous);
// SCAN_DEFERRED / CTL_HELD -> ISSUED (flush_deferred); ISSUED* -> POISONED (finish_batch of an earlier batch that was decoded again);
// ISSUED* / POISONED -> FINISHED (finish_batch: second attempts happen inside it, synchronously). Batches finish in issue order.
enum class BatchState { BUILDING, SCAN_DEFERRED, CTL_HELD, ISSUED, ISSUED_BEHIND_SCAN, POISONED, FINISHED };
BatchState batch_state(const etlg_batch* b) {
  if (b->finished) return BatchState::FINISHED;
  if (!b->pending) return BatchState::BUILDING;
  if (b->deferred) return b->defer_ctl ? BatchState::CTL_HELD : BatchState::SCAN_DEFERRED;
  if (b->force_rerun) return BatchState::POISONED;
  return b->scan_chained ? BatchState::ISSUED_BEHIND_SCAN : BatchState::ISSUED;
}
void check_invariants(etlg_ctx* c, const char* where) {
  auto fail = [&](const char* what, size_t i) {
    fprintf(stderr, "[etlg] INVARIANT VIOLATED after %s: %s (pending batch %zu of %zu)\n", where, what, i, c->pending.size());
    abort();
  };
  if (c->pending.size() >= etlg_ctx::kResRing - 1) fail("more batches in flight than the result ring holds", 0);
  bool seen_deferred = false;
  uint32_t first_seq = 0, last_seq = 0; bool have_seq = false;
  for (size_t i = 0; i < c->pending.size(); i++) {
    const etlg_batch* b = c->pending[i];
    if (b->ctx != c || !b->pending || b->finished) fail("a batch in the pending list is not pending", i);
    if (b->copy.staged) fail("a batch names the staged input of an etlg_copy_decode call that has returned", i);
    const BatchState st = batch_state(b);
    if (seen_deferred) fail("a batch was queued behind one whose decode is not enqueued yet", i);
    switch (st) {
      case BatchState::SCAN_DEFERRED:
        if (c->deferred != b) fail("a deferred batch the context does not name", i);
        if (!b->scan || !b->scan_offs || b->scan_chained || b->kdone) fail("SCAN_DEFERRED without a scan of its own / with a decode enqueued", i);
        seen_deferred = true;
        break;
      case BatchState::CTL_HELD:
        if (c->deferred != b) fail("a held batch the context does not name", i);
        // (ctl_started may be false: an error earlier in the chain rolled the control state back, the pre-pass of this batch is stale and
        // flush_deferred runs it again — finish_batch, "it took the control path")
        if (b->kdone) fail("CTL_HELD with a decode enqueued", i);
        seen_deferred = true;
        break;
      case BatchState::ISSUED_BEHIND_SCAN:
        if (!b->scan || !b->scan_offs || !b->d_scan_res || !b->scan_s || b->params.nframes_dev != b->d_scan_res || b->level != 0) fail("ISSUED_BEHIND_SCAN without the scan's result words / not on the plan", i);
        // fall through
      case BatchState::ISSUED: case BatchState::POISONED:
        if (!b->d_res_blk || !b->h_res || !b->done || !b->kdone || !b->dev) fail("an issued batch without its result block / events / outputs", i);
        if (have_seq && (uint32_t)(b->res_seq_no - last_seq) == 0) fail("two issued batches with one result-ring number", i);
        if (!have_seq) { first_seq = b->res_seq_no; have_seq = true; }
        last_seq = b->res_seq_no;
        if ((uint32_t)(last_seq - first_seq) >= etlg_ctx::kResRing) fail("the issued batches span more than one lap of the result ring", i);
        break;
      default: fail("a BUILDING / FINISHED batch in the pending list", i);
    }
  }
  if (c->deferred && !seen_deferred) fail("the context names a deferred batch that is not the newest pending one", 0);
}

int32_t drain_pending(etlg_ctx* c) {
  SlowScope slow_scope_drain_pending(c, "drain_pending");
  while (!c->pending.empty()) (void)finish_batch(c, c->pending.front());
  return ETLG_OK;
}

// ---- finish_batch, step by step. What the steps hand to each other:
struct FinishState {
  bool forced = false;           // a batch before this one in the chain was decoded again: this one started from a state that was not final
  bool decoded_again = false, redone_mp = false;   // a second attempt wrote the batch's result block at finish time; ... and it was the multi-pass kernels
  bool plan_gave_up = false; uint32_t plan_streak_before = 0;
  bool spare = false; uint32_t spare_in_txn = 0; uint64_t spare_lsn = 0, spare_ord = 0;   // the batches behind this one stand if the second attempt leaves the carried state the first one published (these words)
};

// A step that fails finishes the batch with that error: the code and the context's error record, without the detail string
// (flush_deferred stores both for a batch that was never enqueued).
int32_t finished_with(etlg_ctx* c, etlg_batch* b, int32_t rc) {
  b->pending = false; b->finished = true; b->rc = rc; b->err = c->err;
  if (!c->err.detail) b->err_detail.clear();   // (a library / HIP error has none)
  return rc;
}
#define FB(step) do { const int32_t rc_ = (step); if (rc_ != ETLG_OK) return finished_with(c, b, rc_); } while (0)

int32_t wait_for_result(etlg_ctx* c, etlg_batch* b) {   // (by its own event: batches queued behind this one keep running)
  HIPCHK(c, b->done ? hipEventSynchronize(b->done) : hipStreamSynchronize(c->stream));
  return ETLG_OK;
}
int32_t fetch_result(etlg_ctx* c, etlg_batch* b) {   // behind a second attempt: its result block, waited for
  HIPCHK(c, hipMemcpyAsync(b->h_res, b->d_res_blk, sizeof(DevResult), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ETLG_OK;
}

// k_rows handed the batch back. A tile beyond its LDS window: the kernel reported what it would have needed, the next attempt
// (and the batches behind it) size the tile by that; anything else, or a second failure: not that kernel for this batch
void note_rows_hand_back(etlg_ctx* c, etlg_batch* b, uint32_t ff, const DevResult& r0) {
  const uint32_t why = ff >> 8;
  const uint64_t win = r0.dbg_t[11];
  if (why == 0x1u && b->rows_tries++ < 2 && win <= 100 * 1024) {
    // (the head room decides how many tiles share a CU, not how large the window is — the window takes whatever its share of the LDS
    // leaves: with win / 8 cfg5's tiles missed the four-per-CU budget by a few hundred bytes and ran three per CU)
    c->rows_win_min = std::max<uint64_t>(c->rows_win_min, win + win / (uint64_t)c->rows_win_room);   // (ETLG_ROWS_WIN_ROOM)
    c->rows_resized++;
  } else b->no_rows = true;
}

// Batches behind this one may be running beside it (second stream), chained to a result that is being replaced: both decode streams drain, and the successors are marked for a second attempt of their own — or, for now, spared:
// Round 6: what a batch takes from its predecessor is three words — in_txn, final_lsn, next_ord (DevResult.out_*; the generic kernels
// also refuse to start behind a failed block and mark themselves, load_carry). A fixed-width plan that GAVE THE BATCH UP over a shape
// it does not cover (a Delete, an Update with a key image: fused_fail == 2, no error) has still published those words from the
// Begin / Commit frames it did read, and the plan batches behind it ran from them. When the second attempt ends without an error
// and leaves the SAME three words, every batch behind this one started from the final state: none of them is decoded again
// (they used to be, all of them: a cfg2 stream with a Delete in every 10th batch ran 46 batches twice in 240). Decided in settle_spare,
// once the second attempt's result is in; only chains of plain sidecar batches (no scan in flight, no control pass running ahead).
int32_t mark_or_spare_successors(etlg_ctx* c, etlg_batch* b, bool first_attempt, uint32_t ff, const DevResult& r0, FinishState& st) {
  if (c->pending.empty()) return ETLG_OK;
  HIPCHK(c, sync_decode_streams(c));
  bool plain = c->chain_spare && first_attempt && b->level == 0 && ff == kFailPlanGaveUp && r0.first_err == kNoErr && !b->copy.active && !b->ctl_async && !b->scan_chained;
  for (const etlg_batch* pb : c->pending) if (pb->copy.active || pb->deferred || pb->ctl_async || pb->scan_chained || pb->force_rerun) plain = false;
  st.spare = plain;
  if (st.spare) { st.spare_in_txn = r0.out_in_txn; st.spare_lsn = r0.out_final_lsn; st.spare_ord = r0.out_next_ord; }
  // (table-copy batches are not chained to anything: the ones behind this one stand)
  else for (etlg_batch* pb : c->pending) if (!pb->copy.active) { pb->force_rerun = true; if (pb->deferred) pb->ctl_started = false; }   // (a pre-pass that ran ahead started from a state that was not final)
  return ETLG_OK;
}

// The rungs of the second-attempt ladder, and which one a batch takes — from what its last attempt left (`ff`: its fused_fail bits,
// kFailNotRun for a batch marked by a predecessor's second attempt) and from how it was decoded. Nothing is enqueued here.
enum class Rung {
  COPY_FRAMES,         // the rows -> arena kernel met something it leaves to the other path: the rows become Insert frames, decoded as a batch of those (and, should that fail as well, once more by the multi-pass kernels)
  SAME_WITH_COUNT,     // decoded behind its boundary scan and the count read on the device was not usable: the same path again, with the count
  SAME_AGAIN,          // the batch before this one failed, so this one never ran: the same path again, now from the right state
  CONTROL_AGAIN,       // ... and it took the control path: its control pass ran against a history that has changed
  EMPTY_AGAIN,         // ... and it is EMPTY: no single-pass kernel to enqueue again (round 6: this divided by its zero frames)
  GENERIC_AFTER_ROWS,  // k_rows handed the batch back (a tile beyond its window / image): k_cells / k_fused, and back off
  GENERIC_AFTER_PLAN,  // the fixed-width plan did not cover the batch: generic kernel, and back off
  CONTROL_PATH,        // a Relation / DDL frame: the control path
  MULTI_PASS,          // an error (or a look-back give-up): the multi-pass kernels know the exact cut at the failing frame
};
Rung choose_second_attempt(const etlg_batch* b, uint32_t ff, const DevResult& r0, bool ctrl_hint) {
  if (b->copy.active && b->copy.direct) return Rung::COPY_FRAMES;
  if ((ff & kFailScanCount) && r0.first_err == kNoErr && !(ff & ~kFailScanCount)) return Rung::SAME_WITH_COUNT;
  if (ff & kFailNotRun) return b->ctl_async ? Rung::CONTROL_AGAIN : !b->params.nframes ? Rung::EMPTY_AGAIN : Rung::SAME_AGAIN;
  if (b->used_rows && (ff & kFailRowsBack) && !ctrl_hint) return Rung::GENERIC_AFTER_ROWS;   // (errors recorded beside a tile that gave up mean nothing: its frames were left out of the transaction scan)
  if (b->level == 0) return Rung::GENERIC_AFTER_PLAN;
  if (ctrl_hint && !(ff & kFailLookback)) return Rung::CONTROL_PATH;
  return Rung::MULTI_PASS;
}

int32_t single_again(etlg_ctx* c, etlg_batch* b, const std::vector<EpochRec>& eps, int level) {   // side inputs, then ONE single-pass kernel
  RC(build_side_inputs(c, b, eps));
  return enqueue_single(c, b, level);
}
int32_t enqueue_second_attempt(etlg_ctx* c, etlg_batch* b, Rung rung, FinishState& st) {
  const std::vector<EpochRec> no_eps;
  if (rung == Rung::SAME_WITH_COUNT) c->scan_chain_redone++;
  if (rung == Rung::SAME_AGAIN || rung == Rung::CONTROL_AGAIN || rung == Rung::EMPTY_AGAIN) c->path_n[kPathChainRerun]++;
  switch (rung) {
    case Rung::COPY_FRAMES:
      RC(copy_use_frames(c, b));
      RC(setup_outputs(c, b));
      return enqueue_single(c, b, 1);
    case Rung::SAME_WITH_COUNT: case Rung::SAME_AGAIN:
      return single_again(c, b, no_eps, b->level);
    case Rung::CONTROL_AGAIN:
      // Back to the state before the batch — its own snapshot, unless a rollback since then has already discarded everything behind the failed batch — and again.
      if (b->have_snapshot && b->snap_gen == c->cs_gen) { c->cs = b->snapshot; c->slots.resize(b->snapshot.n_slots); c->slots_dirty = true; c->side_dirty = true; }
      b->ctrl_done = false; b->ctl_started = false; b->have_snapshot = false;
      return standard_path(c, b);
    case Rung::EMPTY_AGAIN: case Rung::CONTROL_PATH:
      return standard_path(c, b);
    case Rung::GENERIC_AFTER_ROWS:
      if (b->no_rows) { c->rows_redone++; c->rows_skip = c->rows_penalty; c->rows_penalty = std::min<uint32_t>(c->rows_penalty * 2, 1024); c->rows_streak = 0; }
      return single_again(c, b, b->eps_saved, 1);
    case Rung::GENERIC_AFTER_PLAN:
      c->path_n[kPathPlanRedone]++;
      // (the back-off: the batches behind a give-up skip the plan for a while, twice as long after every give-up that follows closely. A
      // give-up whose successors stand — `spare`, decided after this attempt — costs one wasted kernel and one generic decode, less than
      // four batches on the generic kernel do: when at least four plan batches finished since the last one, there is no back-off for it)
      st.plan_gave_up = true; st.plan_streak_before = c->plan_streak;
      c->plan_skip = c->plan_penalty; c->plan_penalty = std::min<uint32_t>(c->plan_penalty * 2, 4096); c->plan_streak = 0;
      return single_again(c, b, no_eps, 1);
    case Rung::MULTI_PASS:
      RC(build_side_inputs(c, b, b->eps_saved)); RC(setup_scratch(c, b->params));
      launch_multipass(c, b->params, false);
      b->level = 2; b->used_fused = false;
      c->path_n[kPathRedoneMulti]++; st.redone_mp = true;
  }
  return ETLG_OK;
}

// When the optimistic attempt did not hold, the batch is decoded again on the next path (plan -> generic single pass -> control path /
// multi-pass exact error cut), synchronously, until an attempt holds or the multi-pass kernels have had it.
int32_t second_attempts(etlg_ctx* c, etlg_batch* b, FinishState& st) {
  hipStream_t s = c->stream;
  for (int guard = 0; guard < 8; guard++) {
    const DevResult& r0 = *b->h_res;
    const bool failed = st.forced || r0.first_err != kNoErr || r0.fused_fail;
    const bool ctrl_hint = r0.first_err != kNoErr && (uint32_t)(r0.first_err & 0xFF) == ETLG_E_CTRL_HINT && !b->user_no_ctrl && !b->ctrl_done;
    if (!failed || (b->level == 2 && !ctrl_hint)) break;
    // ---- decode again. Every earlier batch is finished, so the host's carried state is exact: no device chaining.
    st.decoded_again = true;
    DecParams& p = b->params;
    p.carry = nullptr; p.flags &= ~kDecLateCarry;
    carried_from_host(c, p);
    // the batch is decoded against the side inputs of NOW: its view lists the schema slots of now (an optimistic ASYNC batch queued
    // behind one that carried the stream's first Relation frames was enqueued when there were none: its events named slots its view
    // did not list — found by tools/async_fuzz.py). A control pass below (standard_path) sets the count again behind its own frames.
    if (!b->ctl_async && !b->ctrl_done) b->n_slots_view = c->slots.size();   // (a batch whose control pass has run keeps what that pass counted)
    const uint32_t ff = st.forced ? kFailNotRun : r0.fused_fail;
    st.forced = false;
    if (c->rows_trace) fprintf(stderr, "[%s] batch redone: first_err frame %llu rank %u code %u, fused_fail %u (len %zu, frames %u, level %d, scan %d chained %d deferred %d)\n", b->used_rows ? "rows" : b->used_cells ? "cells" : b->level == 0 ? "plan" : "fused", (unsigned long long)(r0.first_err >> 16), (unsigned)((r0.first_err >> 8) & 0xFF), (unsigned)(r0.first_err & 0xFF), r0.fused_fail, b->len, b->params.nframes, b->level, (int)b->scan, (int)b->scan_chained, (int)b->deferred);
    if (b->used_rows && (ff & kFailRowsBack)) note_rows_hand_back(c, b, ff, r0);
    if (c->ctl_stream) HIPCHK(c, hipStreamSynchronize(c->ctl_stream));   // (a pre-pass running ahead shares the scratch and the pinned heads with what follows)
    RC(mark_or_spare_successors(c, b, guard == 0, ff, r0, st));
    HIPCHK(c, hipMemcpyAsync(b->d_res_blk, c->d_init_ring, sizeof(DevResult), hipMemcpyDeviceToDevice, s));
    if (b->copy.active && !b->copy.direct) { RC(copy_repoint_frames(c, b)); launch_copy(c, b->copy, p); }
    if (b->scan_chained) RC(resolve_scan_count(c, b));   // (a second attempt has its frame count in hand)
    const Rung rung = choose_second_attempt(b, ff, r0, ctrl_hint);   // (behind the count: an empty batch takes a rung of its own)
    RC(enqueue_second_attempt(c, b, rung, st));
    RC(fetch_result(c, b));
  }
  return ETLG_OK;
}

// The spare decision (mark_or_spare_successors), with the second attempt's result in: the successors stand, or are marked after all.
void settle_spare(etlg_ctx* c, etlg_batch* b, FinishState& st) {
  const DevResult& r1 = *b->h_res;
  if (c->rows_trace) fprintf(stderr, "[spare] first attempt left in_txn %u lsn %llx ord %llu, second err %d ff %u host_err %d in_txn %u lsn %llx ord %llu\n", st.spare_in_txn, (unsigned long long)st.spare_lsn, (unsigned long long)st.spare_ord, r1.first_err != kNoErr, r1.fused_fail, (int)b->host_err_code, r1.out_in_txn, (unsigned long long)r1.out_final_lsn, (unsigned long long)r1.out_next_ord);
  if (r1.first_err == kNoErr && !r1.fused_fail && !b->host_err_code && (r1.out_in_txn != 0) == (st.spare_in_txn != 0) &&
      (!r1.out_in_txn || (r1.out_final_lsn == st.spare_lsn && r1.out_next_ord == st.spare_ord))) {   // (outside a transaction the other two words are dead: a Begin sets both before anything reads them — apply.rs:2279-2296 — and every other frame that would is an "Invalid transaction state"; the kernels leave different leftovers there)
    c->chain_spared++;
    if (st.plan_gave_up && st.plan_streak_before >= 4) { c->plan_skip = 0; c->plan_penalty = 4; }
  }
  else { st.spare = false; for (etlg_batch* pb : c->pending) if (!pb->copy.active) pb->force_rerun = true; }
}

// The result ring is re-initialised once per lap, when the batch that takes slot 0 (slot 1 for the last block) is ISSUED. With
// batches in flight across that point, a batch of the old lap that is decoded again at finish time writes its block after the new lap's
// re-initialisation has gone out: what the second attempt leaves behind — payload shards that are added to, first_err / fused_fail
// that are min-ed / or-ed into, carry_ready — would meet the slot's next user 32 batches later (found by tools/copy_async_fuzz.py:
// a transaction's payload_bytes 489 instead of 71 behind a table-copy batch that had been redone through the frame rewrite). The
// block is cleared again in that case; the decode streams are idle here (the second attempt was waited for), and nothing else may
// start before the clear is done (the slot's next user may run on the other decode stream).
int32_t reclear_lapped_block(etlg_ctx* c, etlg_batch* b) {
  const uint32_t ring_n = etlg_ctx::kResRing;
  const uint32_t sl = (uint32_t)(b->d_res_blk - (DevResult*)c->d_res.p);
  const uint32_t next_lap = (b->res_seq_no / ring_n + 1) * ring_n;
  const uint32_t cleaner = sl == ring_n - 1 ? next_lap + 1 : next_lap;   // the batch whose issue re-initialises this slot for the next lap
  if (c->res_seq <= cleaner) return ETLG_OK;
  HIPCHK(c, hipMemcpyAsync(b->d_res_blk, c->d_init_ring, sizeof(DevResult), hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, sync_decode_streams(c));
  c->ring_recleared++;
  return ETLG_OK;
}

void count_path(etlg_ctx* c, const etlg_batch* b, const FinishState& st) {
  if (b->copy.active) c->copy_n[b->copy.direct ? 0 : 1]++;
  if (b->level == 0) { c->path_n[kPathPlan]++; if (++c->plan_streak >= 16) c->plan_penalty = 4; }
  else if (b->used_fused && b->used_rows) { c->rows_n++; if (++c->rows_streak >= 16) c->rows_penalty = 4; }
  else if (b->used_fused) c->path_n[b->used_cells ? kPathCells : kPathFused]++;
  else if (!st.redone_mp) c->path_n[kPathMulti]++;
}

// First error: device (frame, rank) vs host control plane (frame, rank). Returns the code (0: none) and the failing frame.
int32_t first_error(const etlg_batch* b, const DevResult& r, int64_t* frame_out, uint32_t* rank_out) {
  int32_t code = 0; int64_t frame = -1; uint32_t rank = 0xFF;
  if (r.first_err != kNoErr) { frame = (int64_t)(r.first_err >> 16); rank = (uint32_t)((r.first_err >> 8) & 0xFF); code = (int32_t)(r.first_err & 0xFF); }
  if (b->host_err_code) {
    const int64_t hf = b->host_err_frame;
    if (frame < 0 || hf < frame || (hf == frame && b->host_err_rank < rank)) { frame = hf; rank = b->host_err_rank; code = b->host_err_code; }
  }
  *frame_out = frame; *rank_out = rank;
  return code;
}

// Control-plane state of a batch that failed at `frame`: keep only effects of frames before the failing one.
void rollback_control_state(etlg_ctx* c, etlg_batch* b, int64_t frame) {
  bool later = false;
  for (auto& cf : b->ctrl) if ((int64_t)cf.frame >= frame) later = true;
  if (!later && !b->host_err_code) return;
  // roll back, then replay the prefix (rare path; errors end the stream anyway)
  c->cs = b->snapshot;
  c->cs_gen++;
  c->slots.resize(b->snapshot.n_slots);
  c->slots_dirty = true; c->side_dirty = true;
  // Effects of the control frames before `frame` are re-applied from the copies of their bytes kept
  // by the first pass (the input itself may be device-resident, or have come without a sidecar).
  std::vector<EpochRec> eps;
  for (size_t i = 0; i < b->ctrl.size() && i < b->ctrl_raw.size(); i++) {
    const CtrlFrame& cf = b->ctrl[i];
    if ((int64_t)cf.frame >= frame) break;
    (void)apply_ctrl_frame(c, cf, b->ctrl_raw[i].data(), b->ctrl_raw[i].size(), eps);
  }
  b->n_slots_view = c->slots.size();
}

// What the batch leaves in the context (stream state, "the stream carries control frames") and the view of its arrays.
void carry_state_and_view(etlg_ctx* c, etlg_batch* b, const DevResult& r, int32_t code, int64_t frame) {
  if (!b->user_no_ctrl) c->last_had_ctrl = b->ctrl_done && !b->ctrl.empty();
  b->have_snapshot = false;
  b->snapshot = ControlState{};
  b->ctrl_raw.clear();
  b->eps_saved.clear();
  b->entry_ord = c->next_ord;   // batches finish in issue order: what the context holds here is what this batch started from
  c->in_txn = r.out_in_txn != 0; c->final_lsn = r.out_final_lsn; c->next_ord = r.out_next_ord;
  b->copy_span = r.copy_span;
  if (b->scan && !code && r.n_frames) { c->scan_last_nf = r.n_frames; c->scan_last_len = b->len; }   // (sizes the grids of the next batch that is decoded behind its scan)

  etlg_batch_view& v = b->v;
  v.n_events = r.n_events; v.n_frames = code ? (uint64_t)frame : r.n_frames;
  v.fixed_bytes = r.fixed_bytes; v.heap_bytes = r.heap_bytes;
  for (int i = 0; i < 3; i++) v.payload_bytes[i] = r.payload[i];
  OutSet* os = b->dev;
  v.on_device = 1;
  v.ev_kind = (const uint8_t*)os->kind.p; v.ev_flags = (const uint8_t*)os->flags.p; v.ev_table_id = (const uint32_t*)os->table.p; v.ev_schema_slot = (const uint32_t*)os->slot.p;
  v.ev_start_lsn = (const uint64_t*)os->start.p; v.ev_commit_lsn = (const uint64_t*)os->commit.p; v.ev_tx_ordinal = (const uint64_t*)os->ord.p; v.ev_body_off = (const uint64_t*)os->body.p;
  v.fixed = (const uint8_t*)os->fixed.p; v.heap = (const uint8_t*)os->heap.p;
}

// TableCopyPayloadMetadata: the bytes of the rows that were decoded
void copy_payload_bytes(etlg_batch* b) {
  const CopyJob& j = b->copy;
  const uint64_t done = b->v.n_frames;
  uint32_t o[2] = {0, 0};
  if (b->rc == ETLG_OK && j.direct && done == j.nrows && b->used_cells && b->copy_span) { o[1] = b->copy_span; }   // the rows -> arena kernel measured them (no device round trips here)
  else {
    (void)hipMemcpy(&o[0], j.d_row_offs, 4, hipMemcpyDeviceToHost);
    (void)hipMemcpy(&o[1], j.d_row_offs + done, 4, hipMemcpyDeviceToHost);
  }
  b->v.payload_bytes[0] = o[1] - o[0]; b->v.payload_bytes[1] = 0; b->v.payload_bytes[2] = 0;
}

// Finishes one batch: waits for its result block; when the optimistic attempt did not hold, decodes the batch again on
// the next path (second_attempts); resolves device vs host error, commits or rolls back the control-plane state, updates
// the carried transaction state of the context and (for host output) copies the arenas back. Batches finish in issue order.
int32_t finish_batch(etlg_ctx* c, etlg_batch* b) {
  SlowScope slow_scope_finish_batch(c, "finish_batch");
  // A table-copy batch decodes inside a virtual transaction of its own (etlg_copy_decode): whatever finishing it does to the carried
  // transaction state of the context — the state a second attempt starts from, the state the batch leaves — is undone on the way out.
  // (For a synchronous call this runs inside etlg_copy_decode's own save / restore and changes nothing.)
  struct TxnKeep { etlg_ctx* c; bool on, in_txn; uint64_t lsn, ord; ~TxnKeep() { if (on) { c->in_txn = in_txn; c->final_lsn = lsn; c->next_ord = ord; } } } txn_keep{c, b->copy.active, c->in_txn, c->final_lsn, c->next_ord};
  if (b->copy.active) { c->in_txn = true; c->final_lsn = 0; c->next_ord = 0; }
  if (b->deferred) RC(flush_deferred(c));   // its boundary scan is still in flight: collect it and enqueue the decode first (a failure: the batch is finished, with that error)
  if (b->pending) {  // must be the oldest pending batch
    if (c->pending.empty() || c->pending.front() != b) return lib_error(c, ETLG_InvalidArgument, "ASYNC batches must be synced in issue order");
    c->pending.erase(c->pending.begin());
  }
  FinishState st;
  ht_start(c);
  FB(wait_for_result(c, b));
  ht_mark(c, 7);
  st.forced = b->force_rerun;
  b->force_rerun = false;
  FB(second_attempts(c, b, st));
  if (st.spare) settle_spare(c, b, st);
  if (st.decoded_again) FB(reclear_lapped_block(c, b));
  count_path(c, b, st);
  DevResult r = *b->h_res;
  if (b->used_fused) for (int k = 0; k < 3; k++) { r.payload[k] = 0; for (int sh = 0; sh < 32; sh++) r.payload[k] += r.pay_shard[sh][k]; }
  for (int i = 0; i < 12; i++) c->last_dbg[i] = r.dbg_t[i];
  c->res_pool.push_back(b->h_res);
  b->h_res = nullptr;
  int64_t frame = -1;
  const int32_t code = first_error(b, r, &frame, &b->err_rank);
  if (code && b->have_snapshot) rollback_control_state(c, b, frame);
  carry_state_and_view(c, b, r, code, frame);
  b->pending = false; b->finished = true;
  side_release(b);   // its kernels are done: the set may take the next change of the side inputs
  if (b->finish_what && b->v.n_events) FB(finish_cells(c, b, b->finish_what, nullptr));   // ETLG_F_FINISH_CELLS: typed arrays, exact floats (host_handoff.inc)
  if (!b->out_dev) FB(download_batch(c, b));
  fill_view_common(b);
  clear_error(c);
  b->rc = code ? set_error(c, code, frame) : (int32_t)ETLG_OK;
  b->err = c->err; b->err_detail = c->err_detail;
  if (b->copy.active) copy_payload_bytes(b);
  return b->rc;
}
#undef FB

}  // namespace

