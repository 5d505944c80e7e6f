// Part of host.cpp (included there, one translation unit): the decode entry points — etlg_decode in named steps (DecodeCall), etlg_copy_decode —
// and the ASYNC chain behind them: flush_deferred, choose_decode_stream, take_ring_slot, decode_tail. What runs a batch once it is enqueued
// (side inputs, outputs, the kernel ladder, the control pass, finish_batch) is host_orchestrate.inc.

namespace {

void finish_before(etlg_ctx* c, const etlg_batch* stop) {   // the pending batches in front of `stop`, oldest first (nullptr: all of them)
  if (!stop) { (void)drain_pending(c); return; }
  while (!c->pending.empty() && c->pending.front() != stop) (void)finish_batch(c, c->pending.front());
}
// A chain behind a batch that has to be decoded again does not heal by itself: every batch enqueued behind one that is marked for a
// second attempt starts from that batch's unusable result, refuses to run, and is itself decoded again — synchronously — when it is
// synced; with the caller keeping its window full that went on for the rest of the stream (one fixed-width batch with an UPDATE in it,
// and every later batch was a poisoned first attempt plus a synchronous second one). The batches in flight in front of `b` (nullptr: all)
// are finished first, once; the batch then starts a fresh chain from the host's exact state.
void heal_chain(etlg_ctx* c, const etlg_batch* b) { finish_before(c, b); c->chain_healed++; }

// The first attempt of this batch is optimistic: a single-pass kernel that runs as if the batch held no Relation / DDL frame (they are
// <0.1 % of frames and absent from almost every batch): no classify / control-list kernels, no host round trip. A control frame makes that
// kernel report ETLG_E_CTRL_HINT and the batch takes the control path then (finish_batch). Not when the batch before this one held control
// frames and the caller asserts nothing: streams that change schemas often (DDL messages every few hundred transactions) would pay for a
// wasted kernel on every batch.
bool optimistic_first(const etlg_ctx* c, const etlg_batch* b) {
  return b->params.nframes && single_pass_ok(c, b->len) && (b->user_no_ctrl || !c->last_had_ctrl) && !b->ctl_async;
}

// ---- etlg_decode, step by step: the call's arguments, what the steps decide, and what they hand to each other
struct DecodeCall {
  etlg_ctx* c; const uint8_t* buf; size_t len; const uint32_t* frame_offsets; size_t nframes; uint32_t flags; etlg_batch** out;
  bool in_dev, out_dev, no_ctrl, scan;
  // the route: may_hold — this call may turn out to be one that holds the deferred batch; async_ok — the batch can join the chain; ctl_ahead —
  // its control pre-pass runs ahead on the control stream; async — it is enqueued and handed out pending; hold — its pre-pass goes out before
  // the held batch is flushed
  bool may_hold = false, async_ok = false, ctl_ahead = false, async = false, hold = false;
  // (in place before the first HIP call of the steps: an early return gives the block and the event back, and — BatchGuard, released only once
  // the batch is the caller's — what the batch took from the context's pools)
  StagedInput staged;
  etlg_batch* b = nullptr;
  BatchGuard guard{nullptr};
  const uint8_t* d_in_ptr = nullptr;   // device address of the input

  DecodeCall(etlg_ctx* c_, const uint8_t* buf_, size_t len_, const uint32_t* offs_, size_t nframes_, uint32_t flags_, etlg_batch** out_)
      : c(c_), buf(buf_), len(len_), frame_offsets(offs_), nframes(nframes_), flags(flags_), out(out_), in_dev(flags_ & ETLG_F_INPUT_ON_DEVICE),
        out_dev(flags_ & ETLG_F_OUTPUT_ON_DEVICE), no_ctrl(flags_ & ETLG_F_NO_CONTROL), scan(offs_ == nullptr), staged(c_) {}

  // what may_hold and hold share: the call has the shape of a batch on the pipelined control path (whatever its input turns out to be), and
  // the batch the previous call left deferred is on that path too
  bool ctl_pipeline_shape() const { return (flags & ETLG_F_ASYNC) && out_dev && !no_ctrl && !scan && nframes && c->ctl_async_mode && c->last_had_ctrl; }
  bool deferred_is_held() const { return c->ctl_hold_mode && c->deferred && c->deferred->defer_ctl; }
  bool behind_marked_batch() const { return async && !c->pending.empty() && c->pending.back()->force_rerun; }
  int32_t wait_for_staged(std::initializer_list<hipStream_t> streams, hipEvent_t done) {
    for (hipStream_t w : streams) if (w) HIPCHK(c, hipStreamWaitEvent(w, done, 0));
    return ETLG_OK;
  }

  // ---- admission. (The batch a call left deferred — a boundary scan in flight, a control pre-pass running ahead — is flushed once this call
  // knows whether it is itself a batch of the pipelined control path: such a batch sends its own pre-pass out FIRST.)
  int32_t admit() {
    // ASYNC table-copy batches still in flight (etlg_copy_decode) finish before a WAL batch is taken: a chained batch would read the state
    // the last of them leaves — the end of a virtual transaction — as its carried transaction state
    if (!c->copy.active) for (const etlg_batch* pb : c->pending) if (pb->copy.active) { (void)flush_deferred(c); RC(drain_pending(c)); clear_error(c); break; }
    // Can this call turn out to be one that HOLDS the deferred batch (`hold`, route())? If not, the deferred batch is flushed right here,
    // before this batch's upload is put in front of the decode streams: its control pass and decode kernels must not queue behind the copy
    // of the batch after it (the upload / decode overlap the staging exists for).
    may_hold = ctl_pipeline_shape() && deferred_is_held();
    if (!may_hold) (void)flush_deferred(c);
    return ETLG_OK;
  }
  // ---- ASYNC with HOST input (the staging batcher of a Rust host, crates/etl-gfx950/src/batcher.rs: pinned buffers from etlg_host_alloc):
  // the bytes and the sidecar are copied into a device block the batch owns, on a copy stream of their own, and from here on the batch IS a
  // device-input batch — it joins the chain, and its upload runs beside the decode of the batch before it (double buffering: the caller
  // fills its next buffer meanwhile). The caller keeps the host buffers untouched until the batch is synced, as for every ASYNC batch.
  int32_t stage_host_input() {
    if (!((flags & ETLG_F_ASYNC) && out_dev && !in_dev && !scan && len && nframes && !c->copy.active && single_pass_ok(c, len))) return ETLG_OK;
    RC(staged.upload(buf, len, frame_offsets, nframes));
    RC(ensure_stream2(c));   // the chain may put this batch on either decode stream: both exist before anything waits
    // (a call that may hold the deferred batch lets only the control stream wait now — its pre-pass reads the upload; the decode streams
    // get their wait once the held batch has been enqueued on them: drain(), prepass_ahead())
    RC(wait_for_staged({may_hold ? (hipStream_t) nullptr : c->stream, may_hold ? (hipStream_t) nullptr : c->stream2, c->ctl_stream, c->scan_stream}, staged.done));
    buf = staged.bytes(); frame_offsets = staged.offs();
    in_dev = true;
    return ETLG_OK;
  }
  // ---- the route. ASYNC batches are chained on the device (DecParams.carry) and may be decoded again when they are synced, so everything
  // they read must still be there then: device-resident input AND sidecar (the context's staging and scan buffers are shared by all
  // batches). Anything else is decoded synchronously; etlg_batch_sync on such a batch returns its stored result. Without the caller's
  // no-control assertion the first attempt is optimistic as long as the stream has not been carrying Relation / DDL frames; on a stream
  // that does carry them (last_had_ctrl) the control pre-pass runs ahead on its own stream (ctl_begin) — that needs the sidecar.
  void route() {
    async_ok = (flags & ETLG_F_ASYNC) && out_dev && in_dev && (!c->copy.active || c->copy.async) && single_pass_ok(c, len);
    // (the pre-pass + host control plane of this batch may only run ahead of batches that are themselves on the control path: each of
    // those holds a snapshot of the control state it started from. An OPTIMISTIC batch still pending — enqueued before the context knew
    // the stream carries Relation / DDL frames — may have to be decoded again when it is synced, against the schemas of ITS position in
    // the stream; a control plane that had run ahead of it had changed them under it: rows decoded against the table's next schema,
    // found by tools/async_fuzz.py. Such a batch waits for the chain to drain first — once per stream, at the transition.)
    bool pending_optimistic = false;
    for (const etlg_batch* pb : c->pending) if (pb->pending && !pb->ctl_async) pending_optimistic = true;
    ctl_ahead = async_ok && ctl_pipeline_shape() && !pending_optimistic;
    async = async_ok && (no_ctrl || !c->last_had_ctrl || ctl_ahead);
    // The pipelined control path, one step deeper (round 4): when the batch held back by the previous call is on that path too, THIS
    // batch's pre-pass goes out before the held one is flushed — i.e. before the host waits for the held batch's pre-pass, runs its
    // control plane (~120 us of host work per 64 MiB of cfg5) and enqueues its decode. The pre-pass of batch k + 1 then runs while the
    // host works on batch k instead of beside batch k's decode kernel (where its small kernels only get going as that one drains, and
    // the host's wait for them was 130 us per batch). The pre-pass kernels read the input and the transaction state the pre-pass before
    // them left on the device — nothing the host control plane of the held batch changes. Two pre-passes in flight: two sets of buffers.
    hold = ctl_ahead && deferred_is_held();
  }
  // ---- draining, and the guard of the result ring
  int32_t drain() {
    if (!hold) {
      (void)flush_deferred(c);
      if (may_hold && staged.done) RC(wait_for_staged({c->stream, c->stream2}, staged.done));
    }
    if (!async) { RC(drain_pending(c)); clear_error(c); }
    // The result blocks live in a ring of kResRing: include/etlg.h asks for fewer than 32 batches in flight, and a caller that keeps more
    // (etlg_copy_decode(ASYNC) queues batches back to back too) must not get a block that a batch in flight — or one being decoded again —
    // still writes: the oldest batches are finished first (ADVICE r5). They stay the caller's: their sync returns what was found here.
    while (c->pending.size() >= etlg_ctx::kResRing - 2) (void)finish_batch(c, c->pending.front());
    return ETLG_OK;
  }
  // ---- the batch: host input of a synchronous call goes to the context's staging buffer; the batch adopts what was staged for it
  int32_t make_batch() {
    d_in_ptr = buf;
    if (!in_dev) {
      RC(upload_input(c, buf, len, nullptr, 0));
      d_in_ptr = (const uint8_t*)c->d_in.p;
    }
    b = new etlg_batch();
    b->ctx = c; b->ctx_gen = c->gen;
    guard.b = b;
    b->user_no_ctrl = no_ctrl; b->out_dev = out_dev; b->in_dev = in_dev; b->scan = scan; b->len = len;
    b->finish_what = (flags & ETLG_F_FINISH_CELLS) ? (uint32_t)(ETLG_FINISH_ARRAYS | ETLG_FINISH_FLOATS) : 0u;
    b->check_cells = (flags & ETLG_F_CHECK_CELLS) != 0;
    staged.adopted_by(b);   // the batch owns the block and the event from here (etlg_batch_free)
    if (c->copy.active && c->copy.staged) { c->copy.staged->adopted_by(b); c->copy.staged = nullptr; }   // an ASYNC table-copy batch whose rows were staged by etlg_copy_decode: likewise
    b->host_in = in_dev ? nullptr : buf; b->host_offs = (in_dev || scan) ? nullptr : frame_offsets; b->dev_in = in_dev ? buf : nullptr;
    b->d_in_ptr = d_in_ptr; b->user_offs = frame_offsets;
    return ETLG_OK;
  }

  // ---- the ways out. The decode goes out (decode_tail) and the batch is the caller's: pending at the end of the chain (ASYNC), or finished here
  int32_t enqueue_now(size_t nf) {
    RC(decode_tail(c, b, nf, async, (async && !c->pending.empty()) ? c->pending.back() : nullptr));
    guard.b = nullptr;
    *out = b;
    if (!async) return finish_batch(c, b);
    b->pending = true; b->v.on_device = 1; fill_view_common(b); c->pending.push_back(b);
    return ETLG_OK;
  }
  int32_t hand_out_deferred() {   // ... or pending with its decode NOT enqueued: the next call on the context does that (flush_deferred)
    b->deferred = true; b->pending = true; b->v.on_device = 1;
    c->deferred = b; c->pending.push_back(b);
    guard.b = nullptr;
    *out = b;
    return ETLG_OK;
  }
  // Round 6: when the batch will be decoded by the fixed-width plan behind its sidecar pre-pass (the cfg2 shape) and the stream has
  // shown how many frames a batch of this size holds, the decode is enqueued AT ONCE behind the scan: the grids are sized by a bound,
  // the kernels read the count the scan leaves on the device (DecParams.nframes_dev), and the host never waits between a scan and
  // the decode behind it (VERDICT r5 #4). A scan that did not hold, or a batch beyond the bound, comes back with fused_fail bit 5
  // and takes the round-5 route when it is finished (finish_batch).
  bool scan_chains(const decode_plan::ScanBound& sb) const {
    return c->scan_chain_mode && c->scan_last_nf && len && no_ctrl && !c->prof_serial && plan_possible(c, c->copy.active, 0) && c->plan_pre != 0 &&
           c->plan_uniform_dw != 0 && !c->plan_skip && side_inputs_stand(c) && sb.bound < (1u << 29) && !behind_marked_batch();
  }
  void take_scan_offsets() {   // an offsets buffer of the batch's own, from the context's pool
    if (c->offs_pool.empty()) c->offs_pool.push_back(new DevBuf());
    b->scan_offs = c->offs_pool.back(); c->offs_pool.pop_back();
  }
  // ASYNC: the scan on its own stream, the decode streams wait for its event; otherwise scan and decode follow each other on the context's
  // stream and the call waits once, at its end.
  int32_t scan_chained(const decode_plan::ScanBound& sb) {
    take_scan_offsets();
    if (async) RC(ensure_stream(c, &c->scan_stream));
    b->scan_s = async ? c->scan_stream : c->stream;
    HIPCHK(c, b->scan_offs->ensure((sb.offs_cap + 2) * 4 + 128));
    b->d_scan_res = (uint32_t*)((uint8_t*)b->scan_offs->p + (((sb.offs_cap + 2) * 4 + 63) & ~(size_t)63));   // (the scan's result words live with the batch: no copy behind the scan)
    HIPCHK(c, scan_begin(c, c->scan_job, d_in_ptr, len, b->scan_s, *b->scan_offs, b->d_scan_res));
    b->nf_est = sb.nf_est;
    if (async) {
      hipEvent_t sev = nullptr;
      RC(take_event(c, &sev));
      HIPCHK(c, hipEventRecord(sev, c->scan_stream));
      RC(ensure_stream2(c));
      for (hipStream_t w : {c->stream, c->stream2}) HIPCHK(c, hipStreamWaitEvent(w, sev, 0));
      c->ev_pool.push_back(sev);   // (recorded and waited for: the waits keep their own reference to this recording)
    }
    b->scan_chained = true;
    c->scan_chained_n++;
    return enqueue_now((size_t)sb.bound);
  }
  // The scan of THIS batch runs on its own stream while the previous batch is still being decoded on the context's, and nobody waits for
  // it here: the call returns with the scan in flight and the NEXT call (or the batch's sync) collects the frame count and enqueues the
  // decode. The input must be complete when the call is made (include/etlg.h).
  int32_t scan_deferred() {
    take_scan_offsets();
    RC(ensure_stream(c, &c->scan_stream));
    HIPCHK(c, scan_begin(c, c->scan_job, d_in_ptr, len, c->scan_stream, *b->scan_offs));
    return hand_out_deferred();
  }
  int32_t scan_now() {   // a synchronous call without a sidecar: the frame count, waited for
    HIPCHK(c, device_scan(c, d_in_ptr, len, &nframes, c->stream, c->d_offs));
    return batch_too_large(c, 0, nframes);
  }
  // The pre-pass goes out now, on the control stream; the host control plane and the decode follow when the next call comes in.
  int32_t prepass_ahead() {
    bool created = false;
    RC(ensure_ctl_stream(c, &created));
    if (created && b->h2d_done) HIPCHK(c, hipStreamWaitEvent(c->ctl_stream, b->h2d_done, 0));
    b->nframes_in = nframes; b->ctl_async = true;
    DecParams& cp = b->ctl_params;
    batch_params(c, cp, d_in_ptr, frame_offsets, nframes, len);
    cp.flags = kDecCtlPrePass;
    etlg_batch* prev = c->pending.empty() ? nullptr : c->pending.back();
    if (prev && prev->pending) {
      if (prev->ctl_async && prev->ctl_params.res) cp.carry = prev->ctl_params.res;   // the pre-passes chain among themselves (control stream order)
      else if (prev->kdone) { HIPCHK(c, hipStreamWaitEvent(c->ctl_stream, prev->kdone, 0)); cp.carry = prev->d_res_blk; }   // an optimistic batch: its decode result
      else { RC(drain_pending(c)); carried_from_host(c, cp); }   // (the state the drained batches left)
    }
    b->ctl_set = (int)(c->ctl_seq & 1u);   // (the held batch's pre-pass wrote the other set)
    cp.res = (DevResult*)c->d_ctl_res.p + (c->ctl_seq++ % etlg_ctx::kCtlRing);
    { const int32_t rc = ctl_begin(c, b, cp, c->ctl_stream, true); if (rc != ETLG_OK) { if (hold) (void)flush_deferred(c); return rc; } }
    if (hold) {   // now the held batch: its pre-pass result, its control plane, its decode
      const int32_t rc_ = flush_deferred(c);
      // (the held batch could not be enqueued: this batch's pre-pass was chained to a control result that will never be the state the
      // decode before it leaves — it starts again from the host's state when it is flushed)
      if (rc_ != ETLG_OK) { b->force_rerun = true; b->ctl_started = false; }
      if (b->h2d_done) RC(wait_for_staged({c->stream, c->stream2}, b->h2d_done));
    }
    b->defer_ctl = true;
    c->ctl_ahead_n++;
    return hand_out_deferred();
  }
};

}  // namespace

extern "C" {

int32_t etlg_copy_decode(etlg_ctx* c, int32_t schema_slot, const uint8_t* buf, size_t len, const uint32_t* row_offsets, size_t nrows,
                         uint32_t flags, etlg_batch** out) {
  (void)flush_deferred(c);
  if (!c || !out || !row_offsets) return ETLG_InvalidArgument;
  *out = nullptr;
  clear_error(c);
  if (schema_slot < 0 || (size_t)schema_slot >= c->slots.size()) return lib_error(c, ETLG_InvalidArgument, "unknown schema slot");
  const SlotHost& sh = *c->slots[(size_t)schema_slot];
  const uint32_t ncols = sh.desc.n_cols;
  const uint64_t per_row = etlg_k_copy_bytes_per_row(ncols);
  const uint64_t syn_len = (uint64_t)len + (uint64_t)nrows * per_row;
  RC(batch_too_large(c, syn_len, nrows, 64));
  HIPCHK(c, hipSetDevice(c->device));
  const bool in_dev = flags & ETLG_F_INPUT_ON_DEVICE;
  hipStream_t s = c->stream;
  CopyJob j;
  j.active = true; j.slot = schema_slot; j.nrows = (uint32_t)nrows; j.ncols = ncols; j.rel_id = sh.desc.table_id; j.rows_len = len;
  j.syn_len = syn_len;
  // first attempt: the rows go straight into the arena (k_copy_cells, cells.hip); a batch with anything unusual in it — a malformed
  // row, rows that do not fit a tile's window — fails there and is decoded again through the row -> frame rewrite below
  j.direct = c->copy_direct && nrows != 0 && single_pass_ok(c, len) && ncols <= etlg_k_cells_maxc();
  // ASYNC (the reference's caller streams rows continuously, postgres/stream/table_copy.rs:78-99): the batch is enqueued behind the
  // table-copy batches already in flight — they share nothing but the stream: every batch decodes inside a virtual transaction of its
  // own — and etlg_batch_sync finishes it. Only the rows -> arena kernel is enqueued that way; what it leaves to the frame rewrite
  // (the context's shared buffers) is done when the batch is synced.
  j.async = (flags & ETLG_F_ASYNC) && (flags & ETLG_F_OUTPUT_ON_DEVICE) && j.direct;
  // Batches of the OTHER kind still in flight finish first: finish_batch writes the stream state a WAL batch leaves into the context,
  // and the rows below must neither see that state nor be chained to it. (A synchronous call finishes everything, as before.)
  bool drain = !j.async;
  for (const etlg_batch* pb : c->pending) if (!pb->copy.active) drain = true;
  if (drain) { RC(drain_pending(c)); clear_error(c); }
  // (a staging block / event that no batch has adopted when the call returns — an early return, or a decode that failed before there was
  // a batch — goes back to the pools)
  StagedInput staged(c);
  if (in_dev) { j.d_rows = buf; j.d_row_offs = row_offsets; }
  else if (j.async) {   // host rows: beside the decode of the batch before it
    RC(staged.upload(buf, len, row_offsets, nrows));
    HIPCHK(c, hipStreamWaitEvent(s, staged.done, 0));
    j.d_rows = staged.bytes(); j.d_row_offs = staged.offs();
    j.staged = &staged;
  } else {
    HIPCHK(c, c->d_copy_in.ensure(len + 64)); HIPCHK(c, c->d_copy_offs.ensure((nrows + 1) * 4));
    if (len) HIPCHK(c, hipMemcpyAsync(c->d_copy_in.p, buf, len, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(c->d_copy_offs.p, row_offsets, (nrows + 1) * 4, hipMemcpyHostToDevice, s));
    j.d_rows = (const uint8_t*)c->d_copy_in.p; j.d_row_offs = (const uint32_t*)c->d_copy_offs.p;
  }
  if (!j.direct) {
    HIPCHK(c, c->d_copy_out.ensure(syn_len + 64)); HIPCHK(c, c->d_copy_out_offs.ensure((nrows + 1) * 4));
    j.d_out = (uint8_t*)c->d_copy_out.p; j.d_out_offs = (uint32_t*)c->d_copy_out_offs.p;
    if (nrows == 0) HIPCHK(c, hipMemsetAsync(j.d_out_offs, 0, 4, s));
  }
  const uint64_t avg = nrows ? (len + nrows - 1) / nrows : 0;
  j.lds = (uint32_t)std::min<uint64_t>(((256 * avg * 9 / 8 + 1024) + 255) & ~255ull, 150 * 1024);
  if (c->copy_lds >= 0) j.lds = (uint32_t)c->copy_lds;   // ETLG_COPY_LDS, measurement knob: 0 = rows read in place (no staging window, more waves per CU)
  // the rows decode inside a virtual transaction of their own; the context's stream state is left alone (finish_batch keeps it
  // that way for a batch that is finished later)
  const bool sv_in = c->in_txn; const uint64_t sv_lsn = c->final_lsn, sv_ord = c->next_ord;
  c->in_txn = true; c->final_lsn = 0; c->next_ord = 0;
  c->copy = j;
  const uint32_t dflags = (flags & (ETLG_F_OUTPUT_ON_DEVICE | ETLG_F_FINISH_CELLS | ETLG_F_CHECK_CELLS)) | ETLG_F_INPUT_ON_DEVICE | ETLG_F_NO_CONTROL | (j.async ? (uint32_t)ETLG_F_ASYNC : 0u);
  const int32_t rc = j.direct ? etlg_decode(c, j.d_rows, len, j.d_row_offs, nrows, dflags, out)
                              : etlg_decode(c, j.d_out, (size_t)syn_len, j.d_out_offs, nrows, dflags, out);
  c->copy = CopyJob{};
  c->in_txn = sv_in; c->final_lsn = sv_lsn; c->next_ord = sv_ord;
  return rc;
}

// The steps of DecodeCall in order: admission, staging of host input, the route, draining, the batch, then one of the ways out — the decode
// chained behind the batch's own boundary scan, the scan left in flight, the control pre-pass ahead (both deferred), or the decode enqueued now.
int32_t etlg_decode(etlg_ctx* c, const uint8_t* buf, size_t len, const uint32_t* frame_offsets, size_t nframes, uint32_t flags, etlg_batch** out) {
  if (!c || !out) return ETLG_InvalidArgument;
  InvariantScope inv_scope{c, "etlg_decode"};
  SlowScope slow_scope_decode(c, "etlg_decode");
  *out = nullptr;
  clear_error(c);
  RC(batch_too_large(c, len, nframes));
  HIPCHK(c, hipSetDevice(c->device));
  DecodeCall d(c, buf, len, frame_offsets, nframes, flags, out);
  RC(d.admit());
  RC(d.stage_host_input());
  d.route();
  RC(d.drain());
  RC(d.make_batch());
  if (d.scan) {   // record boundaries: no sidecar of the caller's, the device scan (scan.hip)
    const decode_plan::ScanBound sb = decode_plan::scan_bound(len, c->scan_last_nf, c->scan_last_len);
    if (d.scan_chains(sb)) return d.scan_chained(sb);
    if (d.async) return d.scan_deferred();
    RC(d.scan_now());
  }
  if (d.ctl_ahead) return d.prepass_ahead();
  if (d.behind_marked_batch()) { heal_chain(c, nullptr); clear_error(c); }
  return d.enqueue_now(d.nframes);
}

}  // extern "C"

namespace {

// The decode of a batch whose boundary scan was left in flight by etlg_decode: collect the frame count, enqueue the kernels.
// A failure here belongs to THAT batch (its sync reports it), not to the call that happens to run this.
int32_t flush_deferred(etlg_ctx* c) {
  SlowScope slow_scope_flush_deferred(c, "flush_deferred");
  etlg_batch* b = c ? c->deferred : nullptr;
  if (!b) return ETLG_OK;
  c->deferred = nullptr;
  b->deferred = false;
  size_t nframes = 0;
  int32_t rc = ETLG_OK;
  const bool pre_pass_ahead = b->defer_ctl;
  if (b->defer_ctl) { b->defer_ctl = false; nframes = b->nframes_in; }   // its control pre-pass ran ahead: decode_tail collects it (standard_path -> ctl_finish)
  else {
    const hipError_t e = scan_collect(c, c->scan_job, &nframes);
    if (e != hipSuccess) rc = lib_error(c, ETLG_DeviceError, hipGetErrorString(e));
    else if ((rc = batch_too_large(c, 0, nframes)) == ETLG_OK) { c->scan_last_nf = nframes; c->scan_last_len = b->len; }
  }
  if (rc == ETLG_OK) {
    // A batch whose boundary scan was deferred joined the chain when the stream had shown no Relation / DDL frame. If it has by now (a
    // batch before this one was synced in between), this batch takes the control path — which starts from the HOST's carried state and
    // control plane: everything before it is finished first. (It used to run its control pass from the state of the last SYNCED batch
    // with the batches in between still pending: rows decoded against missing table state — found by tools/async_fuzz.py, round 4.)
    if (!pre_pass_ahead && !b->user_no_ctrl && c->last_had_ctrl) finish_before(c, b);
    etlg_batch* prev = nullptr;   // the batch issued just before this one, if it is still in flight
    for (size_t i = 0; i < c->pending.size(); i++) if (c->pending[i] == b && i > 0) prev = c->pending[i - 1];
    if (prev && prev->force_rerun) { heal_chain(c, b); prev = nullptr; }   // (as in etlg_decode: a chain behind a batch that is decoded again is finished first, once)
    // This batch was in flight (its scan) when a batch before it was marked for a second attempt, and was marked with it; but its
    // DECODE goes out only now. With nothing in flight in front of it, it starts from the final state: one attempt is enough. (Left
    // marked, it was decoded again at its sync and marked everything behind it in turn: a chain without a sidecar never healed.)
    if (!prev && !pre_pass_ahead) b->force_rerun = false;
    rc = decode_tail(c, b, nframes, true, prev);
  }
  if (rc != ETLG_OK) {  // nothing was enqueued for it: it is finished, with this error
    for (size_t i = 0; i < c->pending.size(); i++) if (c->pending[i] == b) { c->pending.erase(c->pending.begin() + (long)i); break; }
    b->pending = false; b->finished = true; b->rc = rc;
    copy_error(b->err, b->err_detail, c->err, c->err_detail);
    return rc;
  }
  fill_view_common(b);
  return ETLG_OK;
}

// ---- two streams. A batch whose first attempt is a single-pass kernel (k_plan, k_fused, k_cells) and whose predecessor in the
//      chain is one too, and still in flight, is enqueued on the OTHER decode stream and told (flags bit 4) that the state it
//      starts from arrives late: its kernel does not read the predecessor's result block at its start; the few tiles without a
//      Begin before them in the batch poll for it (plan.hip plan_late_carry, lookback.hip.h txn_lookback). So the tail of batch k — its last waves, the write-back of its dirty lines, the dispatch of
//      the next kernel — overlaps the staging and parsing of batch k+1: 63.9 -> 50.1 us per 64 MiB cfg2 batch measured with two
//      independent chains (profiles/r03_plan_development.json). Ordering kept: k+1 starts after k-1 has completed (look-back
//      buffers rotate with distance two; k's waves are all dispatched by then, so a tile of k+1 that polls cannot hold a slot k
//      needs), side inputs unchanged (a change drains the chain), no lap boundary of the result ring.
// Leaves the chosen stream in c->stream (decode_tail puts the context's back) and b->sidx; the plain single-pass case also sets up side inputs, outputs and b->plan_decided: the choice needs them.
int32_t choose_decode_stream(etlg_ctx* c, etlg_batch* b, bool async, etlg_batch* prev) {
  DecParams& p = b->params;
  const hipStream_t first = c->stream;
  const uint32_t res_slot = c->res_seq % etlg_ctx::kResRing;
  bool beside = false;
  // (what both cases below ask for: a predecessor in flight on a single-pass kernel, a single-pass kernel for this batch, no lap boundary of the ring)
  const bool may_go_beside = async && prev && prev->pending && prev->level <= 1 && prev->used_fused && !prev->force_rerun && c->overlap_mode && p.nframes &&
                             single_pass_ok(c, b->len) && c->res_seq != 0 && res_slot >= 2 && !b->copy.active && !c->prof_serial;
  if (may_go_beside && optimistic_first(c, b) && side_inputs_stand(c)) {
    RC(prepare_optimistic(c, b));   // the unchanged-inputs path: no stream work
    beside = true;   // (a look-back buffer that has to grow synchronises both streams: take_descriptors)
  }
  // Batches on the pipelined control path (their pre-pass ran ahead, ctl_async) alternate between the two decode streams as well
  // (round 4): the decode kernel of batch k+1 — enqueued by standard_path, behind its own control pass, side-input set and
  // outputs, all of which go to the stream chosen here — starts beside the tail of batch k's; it reads the carried transaction state
  // late like every batch that runs beside its predecessor (flags bit 4). cfg5: the decode kernels were a single-stream chain.
  else if (may_go_beside && prev->ctl_async && b->ctl_async && c->ctl_overlap_mode) beside = true;
  if (beside) {
    RC(ensure_stream2(c));
    b->sidx = prev->sidx ^ 1;
    c->stream = b->sidx ? c->stream2 : first;
    // the batch before the predecessor must be complete; it is, when it ran on this stream — otherwise wait for its event
    etlg_batch* pp = nullptr;
    for (size_t i = 0; i + 1 < c->pending.size(); i++) if (c->pending[i + 1] == prev) pp = c->pending[i];
    if (pp && pp->pending && pp->kdone && pp->sidx != b->sidx) HIPCHK(c, hipStreamWaitEvent(c->stream, pp->kdone, 0));
    p.flags |= kDecLateCarry;
    c->overlapped++;
  } else {
    b->sidx = 0;
    if (c->tail2_set) { HIPCHK(c, hipStreamWaitEvent(c->stream, c->tail2, 0)); c->tail2_set = false; }   // join: everything enqueued on stream2 so far
  }
  return wait_for_side_upload(c, b->side, c->stream);   // the set was uploaded on the other decode stream: the first batch over here waits for it
}

// Result block: next slot of a ring that is re-initialised once per lap. Slot 31 is the carry source of the batch in
// slot 0, so it is re-initialised one batch later than the others.
int32_t take_ring_slot(etlg_ctx* c, etlg_batch* b, etlg_batch* prev) {
  hipStream_t s = c->stream;
  const uint32_t seq = c->res_seq++;
  const uint32_t slot = seq % etlg_ctx::kResRing;
  DevResult* ring = (DevResult*)c->d_res.p;
  // the blocks about to be re-initialised belong to batches whose result copies travel on res_stream: with two decode streams a
  // batch completes within microseconds of its predecessor, so "the copy of the batch before last is long done" no longer holds —
  // wait (on the device) for the copy of the latest batch, which is behind all the others
  { SlowScope sw1(c, "ring: wait event");
  if ((slot == 0 || slot == 1) && prev && prev->pending && prev->done) HIPCHK(c, hipStreamWaitEvent(s, prev->done, 0)); }
  { SlowScope sw2(c, "ring: init copy");
  const void* init = c->ring_h2d ? (const void*)c->h_init_ring : (const void*)c->d_init_ring;
  const hipMemcpyKind kind = c->ring_h2d ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  if (seq == 0) HIPCHK(c, hipMemcpyAsync(ring, init, sizeof(DevResult) * etlg_ctx::kResRing, kind, s));
  else if (slot == 0) HIPCHK(c, hipMemcpyAsync(ring, init, sizeof(DevResult) * (etlg_ctx::kResRing - 1), kind, s));
  else if (slot == 1) HIPCHK(c, hipMemcpyAsync(ring + (etlg_ctx::kResRing - 1), init, sizeof(DevResult), kind, s)); }
  b->d_res_blk = ring + slot;
  b->res_seq_no = seq;
  return ETLG_OK;
}

// ---- decode_tail, step by step. The parameters: which sidecar (the batch's own scan, the caller's on the device, or the caller's
// uploaded to the context's staging buffer), the worker, the table-copy job, and the carried transaction state — the host's (every
// earlier batch is finished), or, behind pending ASYNC batches, whatever the batch issued just before this one leaves in its result block
int32_t tail_params(etlg_ctx* c, etlg_batch* b, size_t nframes, bool async, const etlg_batch* prev) {
  const uint32_t* offs = b->user_offs;
  if (b->scan) offs = (const uint32_t*)(b->scan_offs ? b->scan_offs->p : c->d_offs.p);
  else if (!b->in_dev) {
    HIPCHK(c, c->d_offs.ensure((nframes + 1) * 4));
    HIPCHK(c, hipMemcpyAsync(c->d_offs.p, b->user_offs, (nframes + 1) * 4, hipMemcpyHostToDevice, c->stream));
    offs = (const uint32_t*)c->d_offs.p;
  }
  DecParams& p = b->params;
  batch_params(c, p, b->d_in_ptr, offs, nframes, b->len);
  p.flags = c->fused_dbg & kDecAblations;  // profiling ablations (results are wrong)
  if (b->check_cells) p.flags |= kDecCheckCells;   // ETLG_F_CHECK_CELLS: the multi-pass kernels validate json / array cells (k_write_chk)
  if (c->copy.active) { p.flags |= kDecCopyRows; p.copy_slot = c->copy.slot; b->copy = c->copy; }
  p.carry = (async && prev && !c->copy.active) ? prev->d_res_blk : nullptr;   // (table-copy batches: a virtual transaction each, nothing carried)
  p.nframes_dev = b->scan_chained ? b->d_scan_res : nullptr;
  return ETLG_OK;
}

// The first attempt: the single-pass kernel the stream decision has prepared (b->plan_decided), or prepared here, when the attempt is
// optimistic; the control path otherwise (standard_path).
int32_t first_attempt(etlg_ctx* c, etlg_batch* b) {
  if (b->plan_decided < 0 && optimistic_first(c, b)) RC(prepare_optimistic(c, b));
  if (b->plan_decided >= 0) return enqueue_single(c, b, b->plan_decided ? 0 : 1);
  return standard_path(c, b);
}

// The result block travels to the pinned block the batch holds. ASYNC: on a second stream — on the decode stream the next batch's kernel
// follows this one directly (a 200-byte device-to-host copy is a 4 us blit kernel plus two dispatch gaps when it sits between them)
int32_t enqueue_result_copy(etlg_ctx* c, etlg_batch* b, bool async) {
  hipStream_t s = c->stream;
  if (!async) { HIPCHK(c, hipMemcpyAsync(b->h_res, b->d_res_blk, sizeof(DevResult), hipMemcpyDeviceToHost, s)); return ETLG_OK; }
  RC(take_event(c, &b->kdone));
  RC(take_event(c, &b->done));
  RC(ensure_res_stream(c));
  HIPCHK(c, hipEventRecord(b->kdone, s));
  if (b->sidx) { HIPCHK(c, hipEventRecord(c->tail2, s)); c->tail2_set = true; }
  HIPCHK(c, hipStreamWaitEvent(c->res_stream, b->kdone, 0));
  HIPCHK(c, hipMemcpyAsync(b->h_res, b->d_res_blk, sizeof(DevResult), hipMemcpyDeviceToHost, c->res_stream));
  HIPCHK(c, hipEventRecord(b->done, c->res_stream));
  return ETLG_OK;
}

// Everything of etlg_decode that needs the frame count: parameters, stream, result block, the first kernel, the result copy.
int32_t decode_tail(etlg_ctx* c, etlg_batch* b, size_t nframes, bool async, etlg_batch* prev) {
  SlowScope slow_scope_decode_tail(c, "decode_tail");
  b->plan_decided = -1;
  RC(tail_params(c, b, nframes, async, prev));
  HIPCHK(c, c->d_res.ensure(sizeof(DevResult) * etlg_ctx::kResRing));
  // (decided before anything is enqueued for the batch; everything below then runs on the chosen stream)
  StreamSwitch sw{c, c->stream};
  SlowScope slow_scope_pre(c, "decode_tail: whole after params");
  RC(choose_decode_stream(c, b, async, prev));
  SlowScope slow_scope_ring(c, "decode_tail: result ring and after");
  RC(take_ring_slot(c, b, prev));
  b->params.res = b->d_res_blk;
  { SlowScope slow_scope_pool(c, "decode_tail: pinned result block");
  RC(take_result(c, &b->h_res)); }
  if (b->copy.active && !b->copy.direct) launch_copy(c, b->copy, b->params);  // rows -> Insert frames (writes p.in / p.offs), row-level errors
  RC(first_attempt(c, b));
  if (b->n_slots_view == ~(size_t)0) b->n_slots_view = c->slots.size();
  SlowScope slow_scope_tail(c, "decode_tail: result copy");
  return enqueue_result_copy(c, b, async);
}

}  // namespace
