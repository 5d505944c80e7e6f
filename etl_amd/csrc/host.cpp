// Host side of libetl_gfx950.so: the C ABI of include/etlg.h. One translation unit in these files —
//   host_state.h          context, batch and pool structures, kernel launchers
//   host_control.inc      control plane (schemas, Relation / DDL messages)
//   host.cpp              this file: error helpers, pools, knobs, lifecycle, scan / tags / shard-plan / control-stream calls, sync, download, free
//   host_decode.inc       etlg_decode / etlg_copy_decode in named steps, the ASYNC chain (flush_deferred, choose_decode_stream, decode_tail)
//   host_handoff.inc      what the hand-off calls share; etlg_batch_size_hints / _cuts / _payload / _finish_cells
//   host_handoff_columns.inc   etlg_batch_columns / _iceberg / _ducklake_copy
//   host_handoff_rows.inc      etlg_batch_rowbinary / _protobuf / _ndjson / _duckdb
//   host_orchestrate.inc  side inputs, outputs, kernel ladder (enqueue_plan, try_enqueue_rows, enqueue_generic), control pre-pass, finish_batch
// host_state.h brings decode_plan.h and handoff_plan.h: what the decode and the hand-off decide before they touch the device, plain C++ without HIP.
#include "host_state.h"

namespace {

int32_t set_error(etlg_ctx* c, int32_t code, int64_t frame, const char* detail = nullptr) {
  c->err.code = code;
  c->err.kind = kErrTable[code].kind;
  c->err.description = kErrTable[code].description;
  c->err_detail = detail ? detail : "";
  c->err.detail = c->err_detail.empty() ? nullptr : c->err_detail.c_str();
  c->err.frame_index = frame;
  return c->err.kind;
}
int32_t lib_error(etlg_ctx* c, int32_t kind, const char* what) {
  c->err.code = 0; c->err.kind = kind; c->err.description = what; c->err.detail = nullptr; c->err.frame_index = -1;
  return kind;
}
void clear_error(etlg_ctx* c) { c->err = etlg_error{}; c->err.frame_index = -1; c->err_detail.clear(); }
// An error record travels with its detail string (context <-> batch): the copy's `detail` points into the copy's own string.
void copy_error(etlg_error& to, std::string& to_detail, const etlg_error& from, const std::string& from_detail) {
  to = from; to_detail = from_detail; to.detail = to_detail.empty() ? nullptr : to_detail.c_str();
}

#define HIPCHK(ctx, call)                                                        \
  do {                                                                           \
    hipError_t _e = (call);                                                      \
    if (_e != hipSuccess) return lib_error((ctx), ETLG_DeviceError, hipGetErrorString(_e)); \
  } while (0)
#define RC(expr) do { const int32_t rc_ = (expr); if (rc_ != ETLG_OK) return rc_; } while (0)   // pass a non-OK code on

#include "host_control.inc"   // control plane: schema slots, wire reader, JSON pull parser, Relation / DDL handlers, device slot table

void side_release(etlg_batch* b) { if (b->side) { b->side->users--; b->side = nullptr; } }
void side_use(etlg_batch* b, SideSet* ss) { if (b->side == ss) return; side_release(b); b->side = ss; ss->users++; }

// etlg_ctx_profile: a pair of events around one launch on `s` (etlg_ctx_profile_read collects them)
struct ProfScope {
  etlg_ctx* c; hipStream_t s; ProfRec r;
  ProfScope(etlg_ctx* c_, int which, hipStream_t s_) : c(c_), s(s_) {
    r.which = which;
    if (c->prof) { (void)hipEventCreate(&r.a); (void)hipEventCreate(&r.b); (void)hipEventRecord(r.a, s); }
  }
  ~ProfScope() { if (c->prof) { (void)hipEventRecord(r.b, s); c->prof_recs.push_back(r); } }
};

void launch_raw(etlg_ctx* c, int which, const DecParams& p) {
  if (which == kFused) etlg_k_launch_fused((int)c->fq.blk, &p, &c->fq, c->stream);
  else if (which == kPlan) etlg_k_launch_plan(&p, &c->pq, c->stream);
  else if (which == kPlanPre) etlg_k_launch_plan_pre(&p, &c->pq, c->stream);
  else if (which == kCells) etlg_k_launch_cells(&p, &c->fq, c->stream);
  else if (which == kCopyCells) etlg_k_launch_copy_cells(&p, &c->fq, c->stream);
  else if (which == kRows) etlg_k_launch_rows(&p, &c->fq, c->stream);
  else if (which == kWriteChk) etlg_k_launch(7, &p, c->stream);
  else etlg_k_launch(which, &p, c->stream);
}

// ETLG_F_CHECK_CELLS behind a single-pass kernel: k_chk_cells over the arena it wrote, unless no slot the batch can decode against has
// a json / jsonb / array column (the side inputs know: SideSet::chk_any). The event count is read on the device; p.nframes bounds it.
void launch_chk_cells(etlg_ctx* c, const etlg_batch* b) {
  if (!b->check_cells || !b->side || !b->side->chk_any || !b->params.nframes) return;
  ProfScope prof(c, kChkCells, c->stream);
  etlg_k_launch_chk_cells(&b->params, b->side->chk_maxc, b->params.nframes, c->stream);
}

void launch(etlg_ctx* c, int which, const DecParams& p) {
  ProfScope prof(c, which, c->stream);
  launch_raw(c, which, p);
}

void launch_copy(etlg_ctx* c, const CopyJob& j, const DecParams& p) {
  if (!j.nrows) return;
  ProfScope prof(c, kCopy, c->stream);
  etlg_k_launch_copy(j.d_rows, j.d_row_offs, j.nrows, j.rows_len, j.ncols, j.rel_id, j.d_out, j.d_out_offs, j.lds, c->copy_lane_per_byte ? 1 : 0, &p, c->stream);
}

// The context's frame buffers, large enough for the batch's rows as Insert frames, under every name the batch holds for them.
int32_t copy_point_at_frames(etlg_ctx* c, etlg_batch* b) {
  CopyJob& j = b->copy;
  HIPCHK(c, c->d_copy_out.ensure(j.syn_len + 64)); HIPCHK(c, c->d_copy_out_offs.ensure(((size_t)j.nrows + 1) * 4));
  j.d_out = (uint8_t*)c->d_copy_out.p; j.d_out_offs = (uint32_t*)c->d_copy_out_offs.p;
  DecParams& p = b->params;
  p.in = j.d_out; p.offs = j.d_out_offs; p.in_len = j.syn_len;
  b->d_in_ptr = j.d_out; b->dev_in = j.d_out; b->user_offs = j.d_out_offs;
  return ETLG_OK;
}

// A table-copy batch whose first attempt was (or would have been) the rows -> arena kernel goes on as a batch of Insert frames:
// the rows are rewritten (copy.hip, with the reference's row-level errors) and every parameter that named the rows names the frames.
int32_t copy_use_frames(etlg_ctx* c, etlg_batch* b) {
  CopyJob& j = b->copy;
  // the frame buffers are the context's own: an ASYNC batch that needs them (k_cells cannot take its schema, or a kernel is forced) lets
  // everything enqueued before it finish — an earlier batch may still be reading them
  if (j.async) HIPCHK(c, hipStreamSynchronize(c->stream));
  RC(copy_point_at_frames(c, b));
  j.direct = false;
  b->len = (size_t)j.syn_len;
  launch_copy(c, j, b->params);
  return ETLG_OK;
}

// A batch on the frame path that is decoded AGAIN (finish_batch: its rows go through the rewrite once more): the context's frame buffers may
// have been re-allocated since its first attempt — a later, larger ASYNC batch grew them (DevBuf::ensure frees the old allocation) — and
// what they hold now is a later batch's frames. Every name the batch holds for them is refreshed first; the streams are idle here (the
// first attempt and everything queued behind it have been waited for), so growing them again is safe too. (the stale pointers
// were a device use-after-free on the bad-row path of an ASYNC frames-at-enqueue batch.)
int32_t copy_repoint_frames(etlg_ctx* c, etlg_batch* b) {
  CopyJob& j = b->copy;
  if (!j.active || j.direct) return ETLG_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->stream2) HIPCHK(c, hipStreamSynchronize(c->stream2));
  return copy_point_at_frames(c, b);
}

// The multi-pass pipeline (also the exact first-error path).
void launch_multipass(etlg_ctx* c, const DecParams& p, bool classify_done) {
  if (!classify_done) { if (p.nframes) launch(c, 0, p); launch(c, 1, p); }
  if (p.nframes) launch(c, 3, p);
  launch(c, 4, p);
  if (p.nframes) launch(c, (p.flags & kDecCheckCells) ? kWriteChk : 5, p);
  launch(c, 6, p);
  if (c->mp_tail) { (void)hipEventRecord(c->mp_tail, c->stream); c->mp_tail_set = true; }   // a pre-pass that runs ahead waits for it (shared scratch)
}

OutSet* take_outset(etlg_ctx* c) {
  if (!c->out_pool.empty()) { OutSet* o = c->out_pool.back(); c->out_pool.pop_back(); return o; }
  return new OutSet();
}

uint32_t max_row_bytes(const etlg_ctx* c) {
  uint32_t m = 16;
  for (auto& s : c->slots) m = std::max(m, 2 * s->desc.row_bytes_full);
  return m;
}

void fill_view_common(etlg_batch* b) {
  etlg_ctx* c = b->ctx;
  b->slot_descs.clear();
  // the slots that existed when the batch's own control frames had been applied — not the ones a LATER batch's control plane has
  // created meanwhile (the control pre-pass runs ahead of the decode: etlg_ctx::ctl_stream)
  const size_t n = std::min(c->slots.size(), b->n_slots_view);
  for (size_t i = 0; i < n; i++) b->slot_descs.push_back(c->slots[i]->desc);
  b->v.n_slots = (uint32_t)b->slot_descs.size();
  b->v.slots = b->slot_descs.data();
}

int32_t finish_batch(etlg_ctx* c, etlg_batch* b);
extern "C" int32_t finish_cells(etlg_ctx* c, etlg_batch* b, uint32_t what, etlg_finish_stats* stats);   // (host_handoff.inc)
int32_t drain_pending(etlg_ctx* c);
int32_t download_batch(etlg_ctx* c, etlg_batch* b);
struct BatchGuard { etlg_batch* b; ~BatchGuard() { if (b) etlg_batch_free(b); } };  // an etlg_decode that fails half way returns what the batch took from the context's pools
int32_t build_side_inputs(etlg_ctx* c, etlg_batch* b, const std::vector<EpochRec>& eps);
int32_t setup_outputs(etlg_ctx* c, etlg_batch* b);
int32_t setup_scratch(etlg_ctx* c, DecParams& p, int set = 0);
bool plan_wanted(etlg_ctx* c, const etlg_batch* b);
bool plan_possible(const etlg_ctx* c, bool copy_rows, uint32_t n_epochs);
bool side_inputs_stand(const etlg_ctx* c);
int32_t wait_for_side_upload(etlg_ctx* c, SideSet* ss, hipStream_t s);
int32_t prepare_optimistic(etlg_ctx* c, etlg_batch* b);
int32_t enqueue_single(etlg_ctx* c, etlg_batch* b, int level);
int32_t standard_path(etlg_ctx* c, etlg_batch* b);
int32_t ctl_begin(etlg_ctx* c, etlg_batch* b, DecParams& p, hipStream_t s, bool ahead);
struct SlowScope {   // ETLG_HOST_TIMES=2: names any of the instrumented calls that takes more than a millisecond
  etlg_ctx* c; const char* what; std::chrono::steady_clock::time_point t0;
  SlowScope(etlg_ctx* c_, const char* w) : c(c_), what(w) { if (c && c->host_times_slow) t0 = std::chrono::steady_clock::now(); }
  ~SlowScope() {
    if (!c || !c->host_times_slow) return;
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    if (us > 1000.0) fprintf(stderr, "etlg host times: %s took %.0f us\n", what, us);
  }
};
static inline void ht_start(etlg_ctx* c) { if (c->host_times) c->host_mark = std::chrono::steady_clock::now(); }
static inline void ht_mark(etlg_ctx* c, int i) {
  if (!c->host_times) return;
  const auto t = std::chrono::steady_clock::now();
  const double us = std::chrono::duration<double, std::micro>(t - c->host_mark).count();
  c->host_us[i] += us; c->host_n[i]++;
  if (c->host_times_slow && us > 500.0) fprintf(stderr, "etlg host times: segment %d took %.0f us\n", i, us);   // ETLG_HOST_TIMES=2: outliers as they happen
  c->host_mark = t;
}
int32_t decode_tail(etlg_ctx* c, etlg_batch* b, size_t nframes, bool async, etlg_batch* prev);
int32_t flush_deferred(etlg_ctx* c);   // (an entry point that finds a deferred batch enqueues its decode first; a failure there belongs to THAT batch: `(void)`)
void check_invariants(etlg_ctx* c, const char* where);
struct StreamSwitch { etlg_ctx* c; hipStream_t saved; ~StreamSwitch() { c->stream = saved; } };   // work for another stream through the launchers: c->stream names it for a while
struct InvariantScope { etlg_ctx* c; const char* where; ~InvariantScope() { if (c && c->debug_invariants) check_invariants(c, where); } };
hipError_t sync_decode_streams(etlg_ctx* c);

// ---- plumbing shared by the entry points and the orchestration

int32_t take_event(etlg_ctx* c, hipEvent_t* out) {   // from the context's pool of untimed events (etlg_batch_free gives them back)
  if (c->ev_pool.empty()) { hipEvent_t e = nullptr; HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming)); c->ev_pool.push_back(e); }
  *out = c->ev_pool.back(); c->ev_pool.pop_back();
  return ETLG_OK;
}
int32_t take_result(etlg_ctx* c, DevResult** out) {   // a pinned result block, likewise
  if (c->res_pool.empty()) { DevResult* r = nullptr; HIPCHK(c, hipHostMalloc((void**)&r, sizeof(DevResult), hipHostMallocDefault)); c->res_pool.push_back(r); }
  *out = c->res_pool.back(); c->res_pool.pop_back();
  return ETLG_OK;
}
// ---- the streams a context creates on first use
int32_t ensure_stream(etlg_ctx* c, hipStream_t* s) {   // scan_stream, h2d_stream, d2h_stream: a stream and nothing else
  if (!*s) HIPCHK(c, hipStreamCreateWithFlags(s, hipStreamNonBlocking));
  return ETLG_OK;
}
int32_t ensure_stream2(etlg_ctx* c) {   // the second decode stream and the event behind its last kernel
  if (c->stream2) return ETLG_OK;
  HIPCHK(c, hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
  HIPCHK(c, hipEventCreateWithFlags(&c->tail2, hipEventDisableTiming));
  return ETLG_OK;
}
int32_t ensure_ctl_stream(etlg_ctx* c, bool* created) {   // the control stream, the event behind the multi-pass kernels, the ring of pre-pass result blocks
  *created = !c->ctl_stream;
  if (c->ctl_stream) return ETLG_OK;
  HIPCHK(c, hipStreamCreateWithFlags(&c->ctl_stream, hipStreamNonBlocking));
  HIPCHK(c, hipEventCreateWithFlags(&c->mp_tail, hipEventDisableTiming));
  HIPCHK(c, c->d_ctl_res.ensure(sizeof(DevResult) * etlg_ctx::kCtlRing));
  return ETLG_OK;
}
int32_t ensure_res_stream(etlg_ctx* c) {   // highest priority: its small copies are blit kernels, and the decode streams keep every wave slot of the chip taken
  if (c->res_stream) return ETLG_OK;
  int lo = 0, hi = 0;
  (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
  HIPCHK(c, hipStreamCreateWithPriority(&c->res_stream, hipStreamNonBlocking, hi));
  return ETLG_OK;
}

// "This batch may take a single-pass kernel": their offsets inside the batch are 31 bits wide, and ETLG_FORCE_MULTIPASS asks for the others.
bool single_pass_ok(const etlg_ctx* c, uint64_t len) { return !c->force_multipass && len < (1ull << 31); }

// The base fill of a DecParams: which input and how many frames (all a classify pass reads) ...
void base_params(DecParams& p, const uint8_t* in, const uint32_t* offs, size_t nframes, size_t len) {
  p = DecParams{};
  p.in = in; p.offs = offs;
  p.nframes = (uint32_t)nframes; p.nblocks = (p.nframes + kBlock - 1) / kBlock; p.in_len = len;
}
// ... the carried transaction state as the host holds it (exact once every earlier batch is finished) ...
void carried_from_host(const etlg_ctx* c, DecParams& p) { p.in_txn = c->in_txn; p.final_lsn = c->final_lsn; p.next_ord = c->next_ord; }
// ... and what a decode or a control pre-pass adds: the worker, no table-copy slot, no host error, the host's carried state
void batch_params(const etlg_ctx* c, DecParams& p, const uint8_t* in, const uint32_t* offs, size_t nframes, size_t len) {
  base_params(p, in, offs, nframes, len);
  p.worker_kind = (uint32_t)c->worker; p.sync_table = c->sync_table; p.copy_slot = -1; p.host_err_frame = 0xFFFFFFFFu;
  carried_from_host(c, p);
}

// Offsets are 32 bits wide and the kernels read up to `slack` bytes past the input; descriptors keep 30 bits for a frame number.
int32_t batch_too_large(etlg_ctx* c, uint64_t len, uint64_t nframes, uint64_t slack = 16) {
  if (len > 0xFFFFFFFFull - slack || nframes >= (1u << 30)) return lib_error(c, ETLG_InvalidArgument, "batch too large (max 4 GiB, 2^30 frames)");
  return ETLG_OK;
}

// Host input of a synchronous call: the bytes (and the sidecar, when the caller has one) go to the context's staging buffers on its stream.
int32_t upload_input(etlg_ctx* c, const uint8_t* buf, size_t len, const uint32_t* offs, size_t nframes) {
  HIPCHK(c, c->d_in.ensure(len + 64));
  if (offs) HIPCHK(c, c->d_offs.ensure((nframes + 1) * 4));
  if (len) HIPCHK(c, hipMemcpyAsync(c->d_in.p, buf, len, hipMemcpyHostToDevice, c->stream));
  if (offs) HIPCHK(c, hipMemcpyAsync(c->d_offs.p, offs, (nframes + 1) * 4, hipMemcpyHostToDevice, c->stream));
  return ETLG_OK;
}

// The synchronous calls that start from k_classify (etlg_frame_tags, etlg_shard_plan, etlg_control_stream), behind their own argument
// checks: everything in flight finishes, host input is uploaded, `p` names the batch and the per-frame scratch, and the envelope + tag
// of every frame is on its way (p.f_tag, on the context's stream).
int32_t classify_begin(etlg_ctx* c, const uint8_t* buf, size_t len, const uint32_t* offs, size_t nframes, uint32_t flags, DecParams& p) {
  HIPCHK(c, hipSetDevice(c->device));
  RC(drain_pending(c));
  const bool in_dev = flags & ETLG_F_INPUT_ON_DEVICE;
  if (!in_dev) RC(upload_input(c, buf, len, offs, nframes));
  base_params(p, in_dev ? buf : (const uint8_t*)c->d_in.p, in_dev ? offs : (const uint32_t*)c->d_offs.p, nframes, len);
  RC(setup_scratch(c, p));
  launch(c, 0, p);
  return ETLG_OK;
}

// Every ETLG_* environment variable of the host layer, read ONCE, when the context is created: name, field, default, parse rule — flag_on:
// set by a value that starts with '1'; flag_off: cleared by one that starts with '0'; truth: an integer, non-zero = on; integer. (ETLG_ROWS_NW
// belongs to the kernel launcher in rows.hip.)
void read_knobs(etlg_ctx* c) {
  auto flag_on = [](const char* name, bool& f) { const char* e = getenv(name); f = e && e[0] == '1'; };
  auto flag_off = [](const char* name, bool& f) { const char* e = getenv(name); f = !(e && e[0] == '0'); };
  auto truth = [](const char* name, bool& f, bool dflt) { const char* e = getenv(name); f = e ? atoi(e) != 0 : dflt; };
  auto integer = [](const char* name, auto& f, long dflt) { const char* e = getenv(name); f = (std::remove_reference_t<decltype(f)>)(e ? atol(e) : dflt); };
  int host_times = 0;
  flag_on("ETLG_FORCE_MULTIPASS", c->force_multipass);            // tests exercise both paths
  flag_on("ETLG_RING_H2D", c->ring_h2d);                          // measurement / bisect: the result ring re-initialised from the host template
  flag_on("ETLG_COPY_KERNEL", c->copy_lane_per_byte);             // the lane-per-byte COPY splitter
  flag_off("ETLG_COPY_DIRECT", c->copy_direct);                   // 0: table-copy rows always through the row -> frame rewrite
  flag_off("ETLG_CTL_OVERLAP", c->ctl_overlap_mode);              // 0: batches on the control path stay on one decode stream
  truth("ETLG_CHAIN_SPARE", c->chain_spare, true);                // 0: the batches behind a plan batch that was decoded again are always decoded again
  truth("ETLG_PLAN_DELETES", c->plan_deletes, true);              // 0: a Delete gives the batch up to the generic kernels
  truth("ETLG_SCAN_CHAIN", c->scan_chain_mode, true);             // 0: a batch without a sidecar always waits for its frame count on the host
  truth("ETLG_CTL_HOLD", c->ctl_hold_mode, true);                 // 0: the held batch is flushed before the next pre-pass goes out
  truth("ETLG_DEBUG_INVARIANTS", c->debug_invariants, false);     // check_invariants at every entry point
  truth("ETLG_ROWS_TRACE", c->rows_trace, false);                 // k_rows' sizing and every second attempt on stderr
  integer("ETLG_HOST_TIMES", host_times, 0);                      // 1: host microseconds per segment of the control path; 2: ... and outliers as they happen
  integer("ETLG_CTRL_STAGE_CAP", c->ctrl_stage_cap_test, 0);      // tests: a staging buffer too small for the batch's control frames
  integer("ETLG_DLC_OFFSET_CAP", c->dlc_offset_cap_test, 0);      // tests: the int32 offsets' byte cap of etlg_batch_ducklake_copy, so that the overflow report is reachable at test size
  integer("ETLG_RB_PARTS", c->rb_parts_test, 0);                  // tests: lanes per row in k_rb_rows (1-4) instead of the choice by row count
  integer("ETLG_CUTS_TILE", c->cuts_tile_test, 0);                // tests: events per scan tile of etlg_batch_cuts, so that a small batch crosses every level of its scan
  integer("ETLG_OL_TILE", c->ol_tile_test, 0);                    // tests: events per tile of etlg_batch_outline, so that a small batch crosses every level of its scan
  integer("ETLG_DLP_TILE", c->dlp_tile_test, 0);                  // tests: events per tile of etlg_ducklake_plan, so that a small batch crosses every level of its scan
  integer("ETLG_SFP_TILE", c->sfp_tile_test, 0);                  // tests: events per tile of etlg_snowflake_plan, so that a small batch crosses every level of its scan
  integer("ETLG_CHP_TILE", c->chp_tile_test, 0);                  // tests: events per tile of etlg_clickhouse_plan, so that a small batch crosses every level of its scan
  integer("ETLG_BQP_TILE", c->bqp_tile_test, 0);                  // tests: events per tile of etlg_bigquery_plan, so that a small batch crosses every level of its scan
  integer("ETLG_ICP_TILE", c->icp_tile_test, 0);                  // tests: events per tile of etlg_iceberg_plan, so that a small batch crosses every level of its event scans
  integer("ETLG_ICP_WORDS", c->icp_words_test, 0);                // tests: bitmap words per tile of etlg_iceberg_plan, so that a small object crosses every level of its popcount scan
  integer("ETLG_PAY_TILE", c->pay_tile_test, 0);                 // tests: frames / events per scan tile of etlg_batch_payload, so that a small batch crosses every level of its scans
  integer("ETLG_FUSED_DBG", c->fused_dbg, 0);                     // ablation bits, profiling only (results are wrong)
  integer("ETLG_FUSED_KERNEL", c->fused_kernel, -1);              // 0 k_fused/256, 1 k_fused/64, 2 k_cells, 3 k_plan, 4 k_rows whenever eligible
  integer("ETLG_ROWS", c->rows_mode, 1);                          // 0: never k_rows
  integer("ETLG_ROWS_CF", c->rows_cf, 0);                         // k_rows' frames per tile
  integer("ETLG_ROWS_LDS", c->rows_lds, -1);                      // k_rows' dynamic LDS bytes
  integer("ETLG_ROWS_WIN_ROOM", c->rows_win_room, 64);            // head room of a resized k_rows window (a divisor)
  integer("ETLG_LDS_MARGIN_PCT", c->lds_margin_pct, -1);          // k_fused / k_cells: margin of the staging window over the average tile
  integer("ETLG_COPY_LDS", c->copy_lds, -1);                      // the COPY splitter's staging window
  integer("ETLG_PLAN", c->plan_mode, 1);                          // 0: no fixed-width plan
  integer("ETLG_PLAN_PRE", c->plan_pre, 1);                       // 0: k_plan runs its look-back itself; 1 / 2: tile prefixes from k_plan_pre
  integer("ETLG_PLAN_MARGIN", c->plan_margin_pct, 4);             // k_plan's LDS window = 64 average frames + this margin
  integer("ETLG_PLAN_DBG", c->plan_dbg, 0);                       // bit 0 = no LDS staging (tests of the in-place reader)
  integer("ETLG_OVERLAP", c->overlap_mode, 1);                    // 0: one decode stream
  integer("ETLG_CTL_ASYNC", c->ctl_async_mode, 1);                // 0: control batches are decoded synchronously
  c->host_times = host_times == 1 || host_times == 2; c->host_times_slow = host_times == 2;
  if (c->rows_win_room <= 0) c->rows_win_room = 64;
}

}  // namespace

// Live contexts: a batch may be freed after its context (garbage-collected bindings do that), in which case
// it must not touch the context's pools.
static std::mutex g_live_mu;
static std::map<const etlg_ctx*, uint64_t> g_live_ctx;  // context -> generation (an address can be reused by a later context)
static uint64_t g_ctx_gen = 0;
static bool ctx_alive(const etlg_ctx* c, uint64_t gen) { std::lock_guard<std::mutex> l(g_live_mu); auto it = g_live_ctx.find(c); return it != g_live_ctx.end() && it->second == gen; }

// ====================================================================== C API
// Pooled blocks of the hand-off calls: hipMalloc / hipFree synchronise the device and cost ~100 us each.
static hipError_t blk_take(etlg_ctx* c, size_t bytes, bool host, void** out, size_t* cap) {
  auto& pool = host ? c->blk_host : c->blk_dev;
  size_t best = (size_t)-1;
  for (size_t i = 0; i < pool.size(); i++)
    if (pool[i].second >= bytes && (best == (size_t)-1 || pool[i].second < pool[best].second)) best = i;
  if (best != (size_t)-1 && pool[best].second <= 4 * bytes + (1u << 20)) {
    *out = pool[best].first; *cap = pool[best].second;
    pool.erase(pool.begin() + (long)best);
    return hipSuccess;
  }
  const size_t want = (bytes + (bytes >> 2) + 4095) & ~(size_t)4095;
  const hipError_t e = host ? hipHostMalloc(out, want, hipHostMallocDefault) : hipMalloc(out, want);
  if (e == hipSuccess) *cap = want;
  return e;
}
static void blk_give(etlg_ctx* c, uint64_t gen, void* p, size_t cap, bool host) {
  if (!p) return;
  if (c && ctx_alive(c, gen)) { (host ? c->blk_host : c->blk_dev).emplace_back(p, cap); return; }
  if (host) (void)hipHostFree(p); else (void)hipFree(p);
}
static void handoff_release(HandoffBlocks& m) {
  blk_give(m.ctx, m.ctx_gen, m.d_a, m.cap_a, false); blk_give(m.ctx, m.ctx_gen, m.d_b, m.cap_b, false); blk_give(m.ctx, m.ctx_gen, m.d_c, m.cap_c, false);
  blk_give(m.ctx, m.ctx_gen, m.h, m.cap_h, true);
  m.d_a = m.d_b = m.d_c = nullptr; m.h = nullptr;
}
struct ScratchBlk {  // a device block for the duration of one call
  etlg_ctx* c; void* p = nullptr; size_t cap = 0;
  ~ScratchBlk() { if (p) blk_give(c, c->gen, p, cap, false); }
};

// ASYNC with HOST input: the bytes and their offsets (frames or rows) are copied into ONE device block the batch owns, on a copy stream
// of their own, beside the decode of the batch before it; `done` is recorded behind the two copies and whoever reads the block waits for
// it on the device. The caller keeps the host buffers untouched until the batch is synced, as for every ASYNC batch (include/etlg.h).
// Block and event go back to the pools when this goes out of scope, unless a batch has adopted them (etlg_batch_free returns them then).
struct StagedInput {
  etlg_ctx* c; void* blk = nullptr; size_t cap = 0, o_offs = 0; hipEvent_t done = nullptr;
  explicit StagedInput(etlg_ctx* c_) : c(c_) {}
  StagedInput(const StagedInput&) = delete;
  ~StagedInput() { if (blk) blk_give(c, c->gen, blk, cap, false); if (done) c->ev_pool.push_back(done); }
  int32_t upload(const uint8_t* buf, size_t len, const uint32_t* offs, size_t n) {
    o_offs = (len + 16 + 255) & ~(size_t)255;   // the kernels' readers may touch up to 16 bytes past the input
    HIPCHK(c, blk_take(c, o_offs + (n + 1) * 4 + 64, false, &blk, &cap));
    RC(ensure_stream(c, &c->h2d_stream));
    RC(take_event(c, &done));
    if (len) HIPCHK(c, hipMemcpyAsync(blk, buf, len, hipMemcpyHostToDevice, c->h2d_stream));
    HIPCHK(c, hipMemcpyAsync((uint8_t*)blk + o_offs, offs, (n + 1) * 4, hipMemcpyHostToDevice, c->h2d_stream));
    HIPCHK(c, hipEventRecord(done, c->h2d_stream));
    c->staged_async++;
    return ETLG_OK;
  }
  const uint8_t* bytes() const { return (const uint8_t*)blk; }
  const uint32_t* offs() const { return (const uint32_t*)((const uint8_t*)blk + o_offs); }
  void adopted_by(etlg_batch* b) { if (blk) { b->stage_blk = blk; b->stage_cap = cap; b->h2d_done = done; blk = nullptr; done = nullptr; } }
};

// A context spreads its work over up to seven HIP streams; ROCm multiplexes a process's streams onto GPU_MAX_HW_QUEUES hardware
// queues (default 4), and two decode streams that share one queue serialise consecutive batches (etl_amd/__init__.py has the
// measurements). The runtime reads the variable when it initialises (first HIP call of the process): a host that loads this
// library before its first HIP call gets a workable default, an explicit setting of the caller's is respected.
__attribute__((constructor)) static void etlg_runtime_defaults(void) { (void)setenv("GPU_MAX_HW_QUEUES", "16", 0); }

extern "C" {

uint32_t etlg_abi_version(void) { return ETLG_ABI_VERSION; }

const etlg_err_desc* etlg_err_table(int32_t code) { return (code >= 0 && code < ETLG_E__COUNT) ? &kErrTable[code] : nullptr; }
int32_t etlg_type_class_of_oid(uint32_t oid) { return type_class(oid); }
int32_t etlg_array_elem_class(uint32_t oid) { for (const auto& a : kArrayOids) if (a.oid == oid) return a.elem; return ETLG_TC_STRING; }
uint32_t etlg_slot_bytes(int32_t cls) { return slot_bytes(cls); }

static char g_create_err[256] = "";
const char* etlg_create_error(void) { return g_create_err; }

int32_t etlg_ctx_create(int32_t hip_device, etlg_ctx** out) {
  if (!out) return ETLG_InvalidArgument;
  *out = nullptr;
  g_create_err[0] = 0;
  auto fail = [&](const char* what, hipError_t e) {
    snprintf(g_create_err, sizeof g_create_err, "%s: %s", what, hipGetErrorString(e));
    return (int32_t)ETLG_DeviceError;
  };
  hipError_t e = hipInit(0);
  if (e != hipSuccess) return fail("hipInit", e);
  int ndev = 0;
  e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess) return fail("hipGetDeviceCount", e);
  if (ndev <= 0 || hip_device < 0 || hip_device >= ndev) { snprintf(g_create_err, sizeof g_create_err, "device %d of %d not available", hip_device, ndev); return ETLG_DeviceError; }
  e = hipSetDevice(hip_device);
  if (e != hipSuccess) return fail("hipSetDevice", e);
  auto* c = new etlg_ctx();
  c->device = hip_device;
  e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e != hipSuccess) { delete c; return fail("hipStreamCreateWithFlags", e); }
  c->own_stream = true;
  e = hipHostMalloc((void**)&c->h_init, sizeof(DevResult), hipHostMallocDefault);
  if (e != hipSuccess) { (void)hipStreamDestroy(c->stream); delete c; return fail("hipHostMalloc", e); }
  { DevResult init{}; init.first_err = kNoErr; *c->h_init = init; }
  e = hipHostMalloc((void**)&c->h_init_ring, sizeof(DevResult) * etlg_ctx::kResRing, hipHostMallocDefault);
  if (e != hipSuccess) { delete c; return fail("hipHostMalloc", e); }
  for (uint32_t i = 0; i < etlg_ctx::kResRing; i++) c->h_init_ring[i] = *c->h_init;
  e = hipMalloc((void**)&c->d_init_ring, sizeof(DevResult) * etlg_ctx::kResRing);
  if (e == hipSuccess) e = hipMemcpy(c->d_init_ring, c->h_init_ring, sizeof(DevResult) * etlg_ctx::kResRing, hipMemcpyHostToDevice);
  if (e != hipSuccess) { delete c; return fail("hipMalloc", e); }
  // (a kernel whose static + dynamic LDS request exceeds a CU's 160 KB is refused here, not at its first launch)
  if (etlg_k_fused_set_lds() || etlg_k_cells_set_lds() || etlg_k_copy_set_lds() || etlg_k_rows_set_lds()) {
    snprintf(g_create_err, sizeof g_create_err, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) refused a kernel's LDS request");
    delete c; return ETLG_DeviceError;
  }
  read_knobs(c);
  clear_error(c);
  (void)etlg_k_plan_set_lds();
  { int ncu = 0; if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, hip_device) == hipSuccess && ncu > 0) c->n_cus = ncu; }
  { std::lock_guard<std::mutex> l(g_live_mu); c->gen = ++g_ctx_gen; g_live_ctx[c] = c->gen; }
  *out = c;
  return ETLG_OK;
}

void etlg_ctx_destroy(etlg_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)drain_pending(c);
  { std::lock_guard<std::mutex> l(g_live_mu); g_live_ctx.erase(c); }
  (void)sync_decode_streams(c);
  if (c->host_times) {
    static const char* names[8] = {"pre-pass kernels + result", "control list", "control bytes", "host control plane", "side inputs", "outputs", "enqueue decode", "wait for the batch"};
    for (int i = 0; i < 8; i++) if (c->host_n[i]) fprintf(stderr, "etlg host times: %-26s %8.1f us x %llu\n", names[i], c->host_us[i] / (double)c->host_n[i], (unsigned long long)c->host_n[i]);
  }
  if (c->h_scan) { (void)hipHostFree(c->h_scan); c->h_scan = nullptr; }
  for (DevBuf* b : {&c->d_copy_in, &c->d_copy_offs, &c->d_copy_out, &c->d_copy_out_offs, &c->d_scan, &c->d_in, &c->d_offs, &c->d_res, &c->d_desc, &c->d_colsel}) b->release();
  for (CtlSet& cs : c->sets) cs.release();
  for (SideSet* ss : c->side_sets) { ss->dev.release(); if (ss->h) (void)hipHostFree(ss->h); if (ss->ready) (void)hipEventDestroy(ss->ready); delete ss; }
  for (OutSet* o : c->out_pool) { o->release(); delete o; }
  for (DevBuf* o : c->offs_pool) { o->release(); delete o; }
  for (auto& b : c->blk_dev) (void)hipFree(b.first);
  for (auto& b : c->blk_host) (void)hipHostFree(b.first);
  if (c->ctl_stream) (void)hipStreamDestroy(c->ctl_stream);
  if (c->mp_tail) (void)hipEventDestroy(c->mp_tail);
  for (void* h : {(void*)c->h_cnt_init, (void*)c->h_hand}) if (h) (void)hipHostFree(h);
  c->d_ctl_res.release();
  for (hipStream_t st : {c->scan_stream, c->h2d_stream, c->d2h_stream, c->res_stream, c->stream2}) if (st) (void)hipStreamDestroy(st);
  c->d_pre.release();
  for (hipEvent_t ev : {c->tail2, c->fence_ev}) if (ev) (void)hipEventDestroy(ev);
  for (auto& r : c->prof_recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
  for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
  for (auto& pr : c->harena_pool) (void)hipHostFree(pr.first);
  for (DevResult* h : {c->h_init, c->h_poison, c->h_init_ring}) if (h) (void)hipHostFree(h);
  if (c->d_init_ring) (void)hipFree(c->d_init_ring);
  for (DevResult* r : c->res_pool) (void)hipHostFree(r);
  if (c->own_stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

// The calls that change what later batches decode against: the deferred batch goes out, the arguments are checked, then everything in
// flight finishes (it was issued against the state before the call).
static bool settle(etlg_ctx* c, bool args_ok = true) {
  (void)flush_deferred(c);
  if (!c || !args_ok) return false;
  (void)drain_pending(c);
  return true;
}

int32_t etlg_ctx_set_stream(etlg_ctx* c, void* s) {
  if (!settle(c)) return ETLG_InvalidArgument;
  (void)hipStreamSynchronize(c->stream);
  if (c->own_stream) (void)hipStreamDestroy(c->stream);
  if (s) { c->stream = (hipStream_t)s; c->own_stream = false; }
  else { if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) return ETLG_DeviceError; c->own_stream = true; }
  return ETLG_OK;
}

int32_t etlg_ctx_set_worker(etlg_ctx* c, int32_t kind, uint32_t table_id, uint64_t bootstrap) {
  if (!settle(c)) return ETLG_InvalidArgument;
  c->worker = kind; c->sync_table = table_id; c->bootstrap = bootstrap; c->side_valid = false; c->side_dirty = true;
  return ETLG_OK;
}

int32_t etlg_schema_put(etlg_ctx* c, uint32_t table_id, uint64_t snapshot, const char* nsp, const char* name, uint32_t ncols, const etlg_col* cols) {
  if (!settle(c, !ncols || cols)) return ETLG_InvalidArgument;
  auto s = std::make_shared<StoredSchema>();
  s->table_id = table_id; s->snapshot = snapshot; s->nsp = nsp ? nsp : ""; s->name = name ? name : "";
  for (uint32_t i = 0; i < ncols; i++) {
    StoredCol sc;
    sc.name = cols[i].name ? cols[i].name : ""; sc.type_oid = cols[i].type_oid; sc.typmod = cols[i].type_modifier;
    sc.attnum = cols[i].attnum; sc.nullable = cols[i].nullable != 0; sc.pk = cols[i].primary_key != 0;
    s->cols.push_back(std::move(sc));
  }
  c->cs.store[table_id][snapshot] = s;
  return ETLG_OK;
}

int32_t etlg_table_state(etlg_ctx* c, uint32_t table_id, int32_t kind, uint64_t lsn) {
  if (!settle(c)) return ETLG_InvalidArgument;
  if (kind == ETLG_TS_ABSENT) c->states.erase(table_id); else c->states[table_id] = TState{kind, lsn};
  c->side_dirty = true;
  return ETLG_OK;
}

int32_t etlg_table_ready(etlg_ctx* c, uint32_t table_id, uint64_t snapshot, const uint8_t* rmask, const uint8_t* imask, uint32_t n) {
  if (!settle(c, rmask && imask)) return -ETLG_InvalidArgument;
  SchemaPtr sch = get_at_or_before(c->cs, table_id, snapshot);
  if (!sch || sch->cols.size() != n) return -ETLG_MissingTableSchema;
  std::vector<uint8_t> r(rmask, rmask + n), i(imask, imask + n);
  const int32_t slot = make_slot(c, sch, r, i);
  c->cs.cache[table_id] = CacheEntry{2, sch->snapshot, slot};
  c->side_dirty = true;
  return slot;
}

int32_t etlg_table_forget(etlg_ctx* c, uint32_t table_id) {
  if (!settle(c)) return ETLG_InvalidArgument;
  c->cs.cache.erase(table_id);
  c->side_dirty = true;
  return ETLG_OK;
}

int32_t etlg_table_cache_get(const etlg_ctx* c, uint32_t table_id, int32_t* kind, uint64_t* snapshot, int32_t* slot) {
  if (!c || !kind || !snapshot || !slot) return 0;
  auto it = c->cs.cache.find(table_id);
  if (it == c->cs.cache.end()) return 0;
  *kind = (int32_t)it->second.kind; *snapshot = it->second.snapshot; *slot = it->second.slot;
  return 1;
}

int32_t etlg_ctx_reset_stream_state(etlg_ctx* c) {
  if (!settle(c)) return ETLG_InvalidArgument;
  c->in_txn = false; c->final_lsn = 0; c->next_ord = 0;
  return ETLG_OK;
}

const etlg_error* etlg_last_error(const etlg_ctx* c) { return c ? &c->err : nullptr; }

int32_t etlg_ctx_slots(const etlg_ctx* c, uint32_t* n, const etlg_slot_desc** slots) {
  if (!c || !n || !slots) return ETLG_InvalidArgument;
  static thread_local std::vector<etlg_slot_desc> tmp;
  tmp.clear();
  for (auto& s : c->slots) tmp.push_back(s->desc);
  *n = (uint32_t)tmp.size(); *slots = tmp.data();
  return ETLG_OK;
}

// ---- debugging aids (not part of etlg.h): counters of the context, copied into the caller's words
static int32_t debug_words(const etlg_ctx* c, unsigned long long* out, const unsigned long long* w, int n) {
  if (!c || !out) return ETLG_InvalidArgument;
  for (int i = 0; i < n; i++) out[i] = w[i];
  return ETLG_OK;
}
// per-phase cycle sums of the last finished batch
int32_t etlg_ctx_debug_times(etlg_ctx* c, unsigned long long* out12) { return debug_words(c, out12, c ? c->last_dbg : nullptr, 12); }
// batches finished per path (PathIdx, host_state.h): the first four, all eight
int32_t etlg_ctx_debug_paths(etlg_ctx* c, unsigned long long* out4) { return debug_words(c, out4, c ? c->path_n : nullptr, 4); }
int32_t etlg_ctx_debug_paths8(etlg_ctx* c, unsigned long long* out8) { return debug_words(c, out8, c ? c->path_n : nullptr, kPathCount); }
// ASYNC batches that were enqueued beside their predecessor on the second decode stream
unsigned long long etlg_ctx_debug_overlapped(etlg_ctx* c) { return c ? c->overlapped : 0; }
unsigned long long etlg_ctx_debug_ctl_ahead(etlg_ctx* c) { return c ? c->ctl_ahead_n : 0; }
unsigned long long etlg_ctx_debug_staged(etlg_ctx* c) { return c ? c->staged_async : 0; }   // ASYNC batches whose host input was staged on the copy stream

int32_t etlg_host_alloc(etlg_ctx* c, size_t bytes, void** out) {
  if (!c || !out || !bytes) return ETLG_InvalidArgument;
  *out = nullptr;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipHostMalloc(out, bytes, hipHostMallocDefault));
  return ETLG_OK;
}
void etlg_host_free(void* p) { if (p) (void)hipHostFree(p); }
// debugging aid (not part of etlg.h), three words: [0] batches k_rows produced, [1] batches it handed back to k_cells / k_fused, [2] ... it took again with a larger window
int32_t etlg_ctx_debug_rows(etlg_ctx* c, unsigned long long* out3) {
  const unsigned long long w[3] = {c ? c->rows_n : 0, c ? c->rows_redone : 0, c ? c->rows_resized : 0};
  return debug_words(c, out3, w, 3);
}

int32_t etlg_ctx_profile(etlg_ctx* c, int32_t enable) {
  if (!c) return ETLG_InvalidArgument;
  c->prof = enable != 0;
  c->prof_serial = enable == 2;   // 2: time kernels one at a time (ASYNC batches stay on one stream), for per-kernel durations that do not overlap
  if (!enable) { for (int i = 0; i < kProfSlots; i++) { c->prof_ms[i] = 0; c->prof_n[i] = 0; } }
  return ETLG_OK;
}

int32_t etlg_ctx_profile_read(etlg_ctx* c, etlg_kernel_stat* out, uint32_t cap, uint32_t* n) {
  if (!c || !n) return ETLG_InvalidArgument;
  (void)hipStreamSynchronize(c->stream);
  for (auto& r : c->prof_recs) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) { c->prof_ms[r.which] += ms; c->prof_n[r.which]++; }
    (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b);
  }
  c->prof_recs.clear();
  uint32_t k = 0;
  for (int i = 0; i < kProfSlots && k < cap; i++) { out[k].name = i == kPlan ? "k_plan" : i == kPlanPre ? "k_plan_pre" : i == kFused ? "k_fused" : i == kCells ? "k_cells" : i == kBounds ? "k_bounds" : i == kCopy ? "k_copy_frames" : i == kCopyCells ? "k_copy_cells" : i == kRows ? "k_rows" : i == kWriteChk ? "k_write_chk" : i == kChkCells ? "k_chk_cells" : etlg_k_name(i); out[k].launches = c->prof_n[i]; out[k].total_ms = c->prof_ms[i]; k++; }
  *n = k;
  return ETLG_OK;
}

// Record boundaries on the device (scan.hip): fills c->d_offs with nframes + 1 offsets of the frames
// of `d_in[0, len)` and returns nframes. Optimistic kernel + hint reruns + one-lane fallback.
// One record-boundary scan in flight (scan.hip). scan_launch enqueues a run and returns; scan_collect waits for it, reruns it
// with hints / on one lane when tiles guessed wrong, and returns the frame count.
hipError_t scan_launch(etlg_ctx* c, ScanJob& j, bool sequential) {
  const size_t len = j.len;
  hipStream_t s = j.s;
  const size_t tb = etlg_k_bounds_tile_bytes();
  const size_t ntiles = (len + tb - 1) / tb;
  // scratch: result block | tile summaries | base indexes | the tiles' scratch rows, and the hints behind them. A run writes everything it
  // reads (no descriptor to clear, no memset on the stream); the result travels through pinned host memory.
  if (!c->h_scan) { hipError_t e = hipHostMalloc((void**)&c->h_scan, 64); if (e != hipSuccess) return e; }
  if (ntiles > c->scan_tiles_cap) {  // (re)allocation: the layout is by capacity; only the hints need initialising
    const size_t tcap = ntiles + ntiles / 4 + 64;
    const size_t body = (etlg_k_bounds_scratch_bytes(tcap) + 63) & ~(size_t)63;
    const size_t need = body + ((tcap * 4 + 63) & ~(size_t)63) + 64;
    hipError_t e = c->d_scan.ensure(need); if (e != hipSuccess) return e;
    e = hipMemsetAsync((uint8_t*)c->d_scan.p + body, 0xFF, tcap * 4, s); if (e != hipSuccess) return e;
    c->scan_tiles_cap = tcap; c->scan_half = body;
  }
  uint8_t* base = (uint8_t*)c->d_scan.p;
  hipError_t e = j.offs->ensure((j.cap + 2) * 4); if (e != hipSuccess) return e;
  j.cur = j.res ? (uint8_t*)j.res : base;
  c->h_scan[0] = 0; c->h_scan[1] = 0;
  ProfScope prof(c, kBounds, s);
  etlg_k_launch_bounds(j.d_in, len, (uint32_t*)j.offs->p, (uint32_t)std::min<size_t>(j.cap + 2, 0xFFFFFFFFu), base, j.res, (uint32_t*)(base + c->scan_half), c->h_scan,
                       sequential ? 1 : 0, s);
  return hipSuccess;
}

hipError_t scan_begin(etlg_ctx* c, ScanJob& j, const uint8_t* d_in, size_t len, hipStream_t s, DevBuf& offs, uint32_t* res = nullptr) {
  j = ScanJob{};
  j.d_in = d_in; j.len = len; j.s = s; j.offs = &offs; j.res = res;
  j.cap = len / 24 + 1024;  // frames the offsets buffer can take; grown to the worst case (5-byte frames) on demand
  if (len == 0) {
    hipError_t e = offs.ensure(64); if (e != hipSuccess) return e;
    return hipMemsetAsync(offs.p, 0, 4, s);
  }
  return scan_launch(c, j, false);
}

hipError_t scan_collect(etlg_ctx* c, ScanJob& j, size_t* nframes_out) {
  *nframes_out = 0;
  if (j.len == 0) return hipSuccess;
  const size_t len = j.len;
  hipStream_t s = j.s;
  const size_t tb = etlg_k_bounds_tile_bytes();
  const size_t ntiles = (len + tb - 1) / tb;
  bool used_hints = false, hints_set = false, overflow = false;
  hipError_t rc = hipSuccess;
  for (int run = 0;; run++) {
    const bool sequential = run >= 4;
    hipError_t e = hipStreamSynchronize(s); if (e != hipSuccess) return e;
    uint32_t nf = c->h_scan[0], flags = 0, nbad = 0;
    if (c->h_scan[1]) {  // the run did not hold: the details are in the device result block
      uint32_t res[16];
      e = hipMemcpy(res, j.cur, 64, hipMemcpyDeviceToHost); if (e != hipSuccess) return e;
      nf = res[0]; flags = res[1]; nbad = res[2];
      if (nbad) hints_set = true;
      if (flags & 4u) overflow = true;   // a tile with more frames than its scratch row holds (malformed input): hints do not help, one lane does
    }
    bool again_same = false;
    if (flags & 2u) {  // offsets buffer too small
      if (j.cap >= len / 5 + 2) { rc = hipErrorOutOfMemory; break; }
      j.cap = len / 5 + 2;
      run--; again_same = true;
    } else if (sequential || (!(flags & 4u) && nbad == 0)) {
      if (used_hints) c->scan_reruns++;
      if (sequential) c->scan_seq++;
      *nframes_out = nf;
      break;
    } else {
      used_hints = true;  // some tiles guessed wrong (their hints are set now), or a spin gave up: run again
    }
    if (overflow && !again_same) run = 3;   // (the next run is the one-lane one)
    e = scan_launch(c, j, again_same ? sequential : run + 1 >= 4); if (e != hipSuccess) return e;
  }
  if (hints_set) { const hipError_t e = hipMemsetAsync((uint8_t*)c->d_scan.p + c->scan_half, 0xFF, ntiles * 4, s); if (e != hipSuccess) return e; }   // rare: leave the hints clean for the next scan
  return rc;
}

// Record boundaries on the device: fills `offs` with nframes + 1 offsets of the frames of `d_in[0, len)` and returns nframes.
hipError_t device_scan(etlg_ctx* c, const uint8_t* d_in, size_t len, size_t* nframes_out, hipStream_t s, DevBuf& offs) {
  ScanJob j;
  hipError_t e = scan_begin(c, j, d_in, len, s, offs); if (e != hipSuccess) return e;
  return scan_collect(c, j, nframes_out);
}


int32_t etlg_scan_boundaries(etlg_ctx* c, const uint8_t* buf, size_t len, uint32_t flags, uint32_t* offsets_out, size_t cap,
                             size_t* nframes_out) {
  (void)flush_deferred(c);
  if (!c || !nframes_out || (!offsets_out && cap)) return ETLG_InvalidArgument;
  clear_error(c);
  RC(batch_too_large(c, len, 0));
  HIPCHK(c, hipSetDevice(c->device));
  const bool in_dev = flags & ETLG_F_INPUT_ON_DEVICE, out_dev = flags & ETLG_F_OUTPUT_ON_DEVICE;
  const uint8_t* d_in_ptr = buf;
  if (!in_dev) {
    RC(upload_input(c, buf, len, nullptr, 0));
    d_in_ptr = (const uint8_t*)c->d_in.p;
  }
  size_t nf = 0;
  HIPCHK(c, device_scan(c, d_in_ptr, len, &nf, c->stream, c->d_offs));
  *nframes_out = nf;
  if (nf + 1 > cap) return lib_error(c, ETLG_InvalidArgument, "offsets_out too small for nframes + 1 entries");
  HIPCHK(c, hipMemcpyAsync(offsets_out, c->d_offs.p, (nf + 1) * 4, out_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ETLG_OK;
}

int32_t etlg_frame_tags(etlg_ctx* c, const uint8_t* buf, size_t len, const uint32_t* frame_offsets, size_t nframes, uint32_t flags,
                        uint8_t* tags_out) {
  (void)flush_deferred(c);
  if (!c || !frame_offsets || (!tags_out && nframes)) return ETLG_InvalidArgument;
  clear_error(c);
  RC(batch_too_large(c, len, nframes));
  if (!nframes) return ETLG_OK;
  const bool out_dev = flags & ETLG_F_OUTPUT_ON_DEVICE;
  hipStream_t s = c->stream;
  DecParams p;
  RC(classify_begin(c, buf, len, frame_offsets, nframes, flags, p));   // k_classify: envelope + tag of every frame
  HIPCHK(c, hipMemcpyAsync(tags_out, p.f_tag, nframes, out_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  return ETLG_OK;
}

int32_t etlg_shard_plan(etlg_ctx* c, const uint8_t* buf, size_t len, const uint32_t* frame_offsets, size_t nframes, uint32_t n_shards,
                        uint32_t flags, uint64_t* cuts_out) {
  (void)flush_deferred(c);
  if (!c || !frame_offsets || !cuts_out || !n_shards || n_shards > 4096) return ETLG_InvalidArgument;
  clear_error(c);
  RC(batch_too_large(c, len, nframes));
  cuts_out[0] = 0;
  for (uint32_t k = 1; k <= n_shards; k++) cuts_out[k] = nframes;
  if (!nframes) { for (uint32_t k = 1; k < n_shards; k++) cuts_out[k] = 0; return ETLG_OK; }
  if (n_shards == 1) return ETLG_OK;
  hipStream_t s = c->stream;
  DecParams p;
  RC(classify_begin(c, buf, len, frame_offsets, nframes, flags, p));   // k_classify: the tags stay on the device
  HIPCHK(c, c->d_colsel.ensure((size_t)n_shards * 4 + 64));
  uint32_t* d_cuts = (uint32_t*)c->d_colsel.p;
  etlg_k_shard_cuts(p.f_tag, p.offs, p.nframes, n_shards, d_cuts, s);
  std::vector<uint32_t> h(n_shards - 1);
  HIPCHK(c, hipMemcpyAsync(h.data(), d_cuts, (size_t)(n_shards - 1) * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  for (uint32_t k = 1; k < n_shards; k++) cuts_out[k] = std::max<uint64_t>(h[k - 1], cuts_out[k - 1]);   // (cuts never go back: a shard may be empty)
  return ETLG_OK;
}

int32_t etlg_shard_replay(etlg_ctx* c, const uint8_t* buf, size_t len, const uint32_t* frame_offsets, size_t nframes) {
  if (!c) return ETLG_InvalidArgument;
  int32_t rc = ETLG_OK;
  if (nframes) {
    if (!buf || !frame_offsets) return ETLG_InvalidArgument;
    etlg_batch* b = nullptr;
    rc = etlg_decode(c, buf, len, frame_offsets, nframes, ETLG_F_OUTPUT_ON_DEVICE, &b);   // the control path: default flags, synchronous; the events are dropped
    const etlg_error saved = c->err; const std::string detail = c->err_detail;
    if (b) etlg_batch_free(b);
    if (rc != ETLG_OK) { copy_error(c->err, c->err_detail, saved, detail); return rc; }
  }
  return etlg_ctx_reset_stream_state(c);   // the shard behind starts outside any transaction, at ordinal 0 (its first frame follows a Commit)
}

int32_t etlg_control_stream(etlg_ctx* c, const uint8_t* buf, size_t len, const uint32_t* frame_offsets, size_t nframes, uint32_t flags,
                            uint8_t* out_bytes, size_t out_cap, uint32_t* out_offsets, size_t out_offsets_cap,
                            size_t* n_bytes, size_t* n_frames, uint32_t* last_tag) {
  (void)flush_deferred(c);
  if (!c || !frame_offsets || !n_bytes || !n_frames) return ETLG_InvalidArgument;
  clear_error(c);
  *n_bytes = 0; *n_frames = 0;
  if (last_tag) *last_tag = 0;
  RC(batch_too_large(c, len, nframes));
  if (!nframes) return ETLG_OK;
  hipStream_t s = c->stream;
  DecParams p;
  RC(classify_begin(c, buf, len, frame_offsets, nframes, flags, p));   // k_classify: envelope + tag of every frame
  constexpr uint32_t kCap = 1u << 16;   // control frames of one range the list holds
  // scratch: hdr (16 words) | list (kCap) | span (2 per frame) | keep frames (<= 3 per frame: the frame, its Begin, its Commit) |
  // lens (3 per frame) | out offsets (3 per frame + 1): 16 + 12 kCap + 1 words
  ScratchBlk blk{c};
  constexpr size_t kCtlWords = 16 + 12 * (size_t)kCap + 1;
  HIPCHK(c, blk_take(c, kCtlWords * 4 + 256, false, &blk.p, &blk.cap));
  uint32_t* d_hdr = (uint32_t*)blk.p;
  uint32_t* d_list = d_hdr + 16; uint32_t* d_span = d_list + kCap; uint32_t* d_keep = d_span + 2 * kCap;
  uint32_t* d_lens = d_keep + 3 * kCap; uint32_t* d_oo = d_lens + 3 * kCap;
  HIPCHK(c, hipMemsetAsync(d_hdr, 0, 8, s));
  etlg_k_ctl_pick(p.f_tag, p.nframes, d_hdr, d_list, kCap, s);
  uint32_t hdr[2] = {0, 0};
  HIPCHK(c, hipMemcpyAsync(hdr, d_hdr, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  if (last_tag) *last_tag = hdr[1];
  const uint32_t n = hdr[0];
  if (!n) { if (out_offsets && out_offsets_cap) out_offsets[0] = 0; return ETLG_OK; }   // the common case: one kernel pair, one 8-byte copy
  if (n > kCap) return lib_error(c, ETLG_Unsupported, "more than 65536 control frames in one range: extract the control stream of smaller ranges");
  std::vector<uint32_t> list(n), span(2 * (size_t)n);
  HIPCHK(c, hipMemcpy(list.data(), d_list, (size_t)n * 4, hipMemcpyDeviceToHost));
  std::sort(list.begin(), list.end());   // the pick is unordered (atomics); the span kernel does not care, the stream does
  HIPCHK(c, hipMemcpyAsync(d_list, list.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
  etlg_k_ctl_span(p.f_tag, p.nframes, d_list, n, d_span, s);
  HIPCHK(c, hipMemcpyAsync(span.data(), d_span, (size_t)n * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  std::vector<uint32_t> keep(list);
  for (uint32_t i = 0; i < n; i++) {
    if (span[2 * i] == 0xFFFFFFFFu) continue;        // not inside a transaction of this range: the frame travels alone
    keep.push_back(span[2 * i]);
    if (span[2 * i + 1] != 0xFFFFFFFFu) keep.push_back(span[2 * i + 1]);
  }
  std::sort(keep.begin(), keep.end());
  keep.erase(std::unique(keep.begin(), keep.end()), keep.end());
  const uint32_t nk = (uint32_t)keep.size();   // <= 3 n
  if ((size_t)nk > 3 * (size_t)kCap) return lib_error(c, ETLG_Unsupported, "control stream of this range holds more frames than its scratch block");
  std::vector<uint32_t> lens(nk), oo((size_t)nk + 1, 0);
  HIPCHK(c, hipMemcpyAsync(d_keep, keep.data(), (size_t)nk * 4, hipMemcpyHostToDevice, s));
  etlg_k_ctl_gather(p.in, p.offs, d_keep, nk, d_lens, nullptr, nullptr, s);
  HIPCHK(c, hipMemcpyAsync(lens.data(), d_lens, (size_t)nk * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  for (uint32_t i = 0; i < nk; i++) oo[i + 1] = oo[i] + lens[i];
  *n_bytes = oo[nk]; *n_frames = nk;
  if (!out_bytes || !out_offsets || out_cap < oo[nk] || out_offsets_cap < (size_t)nk + 1)
    return lib_error(c, ETLG_InvalidArgument, "control stream does not fit the output buffers (n_bytes / n_frames hold what it needs)");
  ScratchBlk stage{c};
  HIPCHK(c, blk_take(c, (size_t)oo[nk] + 64, false, &stage.p, &stage.cap));
  HIPCHK(c, hipMemcpyAsync(d_oo, oo.data(), (size_t)nk * 4, hipMemcpyHostToDevice, s));
  etlg_k_ctl_gather(p.in, p.offs, d_keep, nk, d_lens, d_oo, (uint8_t*)stage.p, s);
  HIPCHK(c, hipMemcpyAsync(out_bytes, stage.p, oo[nk], hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  memcpy(out_offsets, oo.data(), ((size_t)nk + 1) * 4);
  return ETLG_OK;
}

// debugging aid (not part of etlg.h): [0] scans that needed a rerun with hints, [1] scans that fell back to the one-lane walk
int32_t etlg_ctx_debug_scan(etlg_ctx* c, unsigned long long* out2) {
  const unsigned long long w[2] = {c ? c->scan_reruns : 0, c ? c->scan_seq : 0};
  return debug_words(c, out2, w, 2);
}

// debugging aid (not part of etlg.h): table-copy batches [0] produced by the rows -> arena kernel, [1] decoded through the row -> frame rewrite
int32_t etlg_ctx_debug_copy(etlg_ctx* c, unsigned long long* out2) { return debug_words(c, out2, c ? c->copy_n : nullptr, 2); }

// debugging aid (not part of etlg.h), six words: [0] result blocks cleared again after a second attempt behind their lap's re-initialisation,
// [1] chains finished early because their last batch was marked for a second attempt, [2] always 0 (it counted the batches of the re-issue
// experiment, tools/experiments/r06_chain_reissue.diff), [3] batches whose decode was enqueued behind their boundary scan, [4] ... that were
// decoded again with the count in hand, [5] second attempts of a plan batch whose successors stood
int32_t etlg_ctx_debug_ring(etlg_ctx* c, unsigned long long* out6) {   // (callers pass eight words)
  if (!c) return ETLG_InvalidArgument;
  const unsigned long long w[6] = {c->ring_recleared, c->chain_healed, 0, c->scan_chained_n, c->scan_chain_redone, c->chain_spared};
  return debug_words(c, out6, w, 6);
}

}  // extern "C"

#include "host_decode.inc"   // etlg_decode and etlg_copy_decode in named steps, the ASYNC chain (flush_deferred, decode_tail)

extern "C" {

int32_t etlg_batch_sync(etlg_ctx* c, etlg_batch* b) {
  if (!c || !b) return ETLG_InvalidArgument;
  InvariantScope inv_scope{c, "etlg_batch_sync"};
  if (b->pending) {
    // batches finish in issue order: the carried transaction state of the context is the state after the LAST finished one
    while (b->pending && !c->pending.empty()) (void)finish_batch(c, c->pending.front());
  }
  // the context's last error becomes this batch's (the reference returns the error of the call that hit it)
  copy_error(c->err, c->err_detail, b->err, b->err_detail);
  return b->rc;
}

int32_t etlg_batch_header_to_device(etlg_ctx* c, etlg_batch* b, void* dst) {
  if (!c || !b || !dst) return ETLG_InvalidArgument;
  static_assert(offsetof(DevResult, n_frames) == 56, "header layout");
  if (b->deferred) RC(flush_deferred(c));
  if (b->pending && b->kdone && c->res_stream) {   // in flight: behind its kernels on the stream its result block travels on (etlg_ctx_fence joins)
    HIPCHK(c, hipMemcpyAsync(dst, b->d_res_blk, 64, hipMemcpyDeviceToDevice, c->res_stream));
    c->hdr_in_flight = true;
    return ETLG_OK;
  }
  HIPCHK(c, hipMemcpyAsync(dst, b->d_res_blk, 64, hipMemcpyDeviceToDevice, c->stream));
  return ETLG_OK;
}

int32_t etlg_ctx_fence(etlg_ctx* c) {
  if (!c) return ETLG_InvalidArgument;
  (void)flush_deferred(c);
  if (c->tail2_set) { HIPCHK(c, hipStreamWaitEvent(c->stream, c->tail2, 0)); c->tail2_set = false; }
  if (c->hdr_in_flight && c->res_stream) {
    if (!c->fence_ev) HIPCHK(c, hipEventCreateWithFlags(&c->fence_ev, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(c->fence_ev, c->res_stream));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->fence_ev, 0));
    c->hdr_in_flight = false;
  }
  return ETLG_OK;
}

int32_t etlg_batch_download(etlg_ctx* c, etlg_batch* b) {
  if (!c || !b) return ETLG_InvalidArgument;
  if (b->pending) (void)etlg_batch_sync(c, b);
  return download_batch(c, b);
}

int32_t etlg_batch_view_get(const etlg_batch* b, etlg_batch_view* out) {
  if (!b || !out) return ETLG_InvalidArgument;
  *out = b->v;
  return ETLG_OK;
}

void etlg_batch_free(etlg_batch* b) {
  if (!b) return;
  if (b->ctx && ctx_alive(b->ctx, b->ctx_gen)) {
    etlg_ctx* c = b->ctx;
    if (b->pending) {  // freed without a sync: it still has to finish, in order, for the context's carried state to be right
      while (b->pending && !c->pending.empty()) (void)finish_batch(c, c->pending.front());
      b->pending = false;
    }
    if (b->h_res) (void)hipStreamSynchronize(c->stream);
    side_release(b);
    if (b->ctl_ev) { if (b->ctl_started && c->ctl_stream) (void)hipStreamSynchronize(c->ctl_stream); c->ev_pool.push_back(b->ctl_ev); }
    if (b->h_ctl) c->res_pool.push_back(b->h_ctl);
    for (hipEvent_t e : {b->done, b->kdone}) if (e) c->ev_pool.push_back(e);
    if (b->dev) c->out_pool.push_back(b->dev);
    if (b->scan_offs) c->offs_pool.push_back(b->scan_offs);
    if (b->h2d_done) c->ev_pool.push_back(b->h2d_done);
    if (b->stage_blk) blk_give(c, c->gen, b->stage_blk, b->stage_cap, false);
    if (b->h_res) c->res_pool.push_back(b->h_res);
    if (b->h_arena) c->harena_pool.emplace_back(b->h_arena, b->h_arena_cap);
  } else {  // the context is gone (its pools with it): release what the batch owns outright
    if (b->dev) { b->dev->release(); delete b->dev; }
    if (b->scan_offs) { b->scan_offs->release(); delete b->scan_offs; }
    if (b->stage_blk) (void)hipFree(b->stage_blk);
    for (hipEvent_t e : {b->h2d_done, b->done, b->kdone, b->ctl_ev}) if (e) (void)hipEventDestroy(e);
    for (void* p : {(void*)b->h_ctl, (void*)b->h_res, (void*)b->h_arena}) if (p) (void)hipHostFree(p);
  }
  delete b;
}

#include "host_handoff.inc"           // hand-off: what the calls share; etlg_batch_size_hints / _cuts / _outline / _payload / _finish_cells, etlg_ducklake_plan / _fingerprints, etlg_snowflake_plan, etlg_clickhouse_plan, etlg_bigquery_plan, etlg_iceberg_plan (finish.hip, fingerprint.hip)
#include "host_handoff_columns.inc"   // etlg_batch_columns / _iceberg / _ducklake_copy in named steps (columns.hip)
#include "host_handoff_rows.inc"      // etlg_batch_rowbinary / _protobuf / _ndjson / _duckdb in named steps (rowformats.hip, rowformats_dl.hip)

}  // extern "C"

#include "host_orchestrate.inc"   // arena download, side inputs, outputs, kernel ladder, control pre-pass, finish_batch
