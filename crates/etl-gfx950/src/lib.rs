//! etl-gfx950 — the Rust side of the MI355X-native decode stage for supabase/etl.
//!
//! ```text
//! ReplicationMessageStream ──bytes──▶ StagingBatcher ──64 MiB + sidecar──▶ GpuDecoder::decode ──arena──▶ materialize::events ──▶ EventBatch
//! ```
//! * [`ffi`]         raw binding of `include/etlg.h` (checked against the header by the etl-gfx950 test suite);
//! * [`batcher`]     frames + offsets sidecar accumulation in a ring of pinned buffers, flush policy (apply.rs:1910-1967);
//! * [`copy`]        table copy: `CopyOutStream` items staged as bytes, `GpuDecoder::copy_decode` → `Vec<TableRow>` (table_copy.rs:70-103);
//! * [`flush`]       `last_received_lsn` / `last_commit_end_lsn` / effective flush LSN for a loop that decodes batches (apply.rs:2039-2051,
//!                   1918-1928, 2000, 885-912);
//! * [`materialize`] arena → `Event` / `TableRow` / `Cell`, DEFERRED cells finished with the reference's own parser;
//!
//! None of this has met a Rust compiler (the etl-gfx950 image has none). What HAS been executed is the twin of the call sequence in C++
//! through the same C ABI — tests/native/shim_twin.cpp, run by tests/test_shim_twin.py on the MI355X against the oracle's events and a
//! model of the reference's LSN rules: `StagingBatcher` (ring of pinned buffers, `push_xlog_data`, `take` / `recycle`), `decode_async` /
//! `finish`, `decode_unstaged`, `FlushTracker`, `InFlight`'s drop order. A change here wants the same change there.
//! * [`GpuDecoder`]  safe wrapper of one context: side inputs mirror `SchemaStore` / `StateStore` / `SharedTableCache`
//!                   (crates/etl/src/store/schema/base.rs:19-69, store/state/base.rs:25-139, replication/table_cache.rs:88-154).
pub mod batcher;
pub mod copy;
pub mod ffi;
pub mod flush;
pub mod materialize;

use std::ffi::{CStr, CString};
use std::ptr;

use etl::error::{ErrorKind, EtlError, EtlResult};
use etl::etl_error;
use etl::event::Event;

use crate::batcher::StagedBatch;
use crate::ffi::*;

/// `etlg_error_kind` → the reference's `ErrorKind` (crates/etl/src/error.rs:85-170). Descriptions are the reference's own
/// static strings (`etlg_err_table`), so `EtlError::kind()` / `description()` read as if the CPU decoder had failed.
fn kind_of(k: i32) -> ErrorKind {
    match k {
        ETLG_ConversionError => ErrorKind::ConversionError,
        ETLG_InvalidData => ErrorKind::InvalidData,
        ETLG_ValidationError => ErrorKind::ValidationError,
        ETLG_InvalidState => ErrorKind::InvalidState,
        ETLG_MissingTableSchema => ErrorKind::MissingTableSchema,
        ETLG_CorruptedTableSchema => ErrorKind::CorruptedTableSchema,
        ETLG_DeserializationError => ErrorKind::DeserializationError,
        ETLG_SourceConnectionFailed => ErrorKind::SourceConnectionFailed,
        ETLG_IoError => ErrorKind::IoError,
        ETLG_UnsupportedValueInDestination => ErrorKind::UnsupportedValueInDestination,
        ETLG_NullValuesNotSupportedInArrayInDestination => ErrorKind::NullValuesNotSupportedInArrayInDestination,
        _ => ErrorKind::Unknown,
    }
}

pub struct GpuDecoder {
    ctx: *mut etlg_ctx,
    check_cells: bool,
}

// One context per apply-loop stream, used from one task at a time (`&mut self`), like the loop's own state.
unsafe impl Send for GpuDecoder {}

impl GpuDecoder {
    pub fn new(hip_device: i32) -> EtlResult<Self> {
        let mut ctx = ptr::null_mut();
        let rc = unsafe { etlg_ctx_create(hip_device, &mut ctx) };
        if rc != ETLG_OK {
            let why = unsafe { CStr::from_ptr(etlg_create_error()) }.to_string_lossy().into_owned();
            return Err(etl_error!(ErrorKind::ConfigError, "MI355X decode context could not be created", why));
        }
        debug_assert_eq!(unsafe { etlg_abi_version() }, ETLG_ABI_VERSION);
        Ok(Self { ctx, check_cells: false })
    }

    fn last_error(&self) -> EtlError {
        let e = unsafe { &*etlg_last_error(self.ctx) };
        let desc: &'static str = if e.description.is_null() { "GPU decode failed" } else { unsafe { CStr::from_ptr(e.description) }.to_str().unwrap_or("GPU decode failed") };
        let detail = if e.detail.is_null() { format!("frame {}", e.frame_index) } else { format!("{} (frame {})", unsafe { CStr::from_ptr(e.detail) }.to_string_lossy(), e.frame_index) };
        etl_error!(kind_of(e.kind), desc, detail)
    }

    /// `SchemaStore::store_table_schema` mirror: stored columns in attnum order.
    pub fn put_schema(&mut self, table_id: u32, snapshot_lsn: u64, schema: &str, table: &str, cols: &[(String, u32, i32, i32, bool, bool)]) -> EtlResult<()> {
        let names: Vec<CString> = cols.iter().map(|c| CString::new(c.0.as_str()).unwrap()).collect();
        let raw: Vec<etlg_col> = cols
            .iter()
            .zip(&names)
            .map(|(c, n)| etlg_col { name: n.as_ptr(), type_oid: c.1, type_modifier: c.2, attnum: c.3, nullable: c.4 as u8, primary_key: c.5 as u8, _pad: [0; 2] })
            .collect();
        let (s, t) = (CString::new(schema).unwrap(), CString::new(table).unwrap());
        match unsafe { etlg_schema_put(self.ctx, table_id, snapshot_lsn, s.as_ptr(), t.as_ptr(), raw.len() as u32, raw.as_ptr()) } {
            ETLG_OK => Ok(()),
            _ => Err(self.last_error()),
        }
    }

    /// Table replication state as `should_apply_changes` sees it (apply.rs:2836-2867).
    pub fn set_table_state(&mut self, table_id: u32, state_kind: i32, lsn: u64) {
        unsafe { etlg_table_state(self.ctx, table_id, state_kind, lsn) };
    }

    /// `SharedTableCache::note_ready` after a table copy (table_cache.rs:122); returns the schema slot.
    pub fn table_ready(&mut self, table_id: u32, snapshot_lsn: u64, replication_mask: &[u8], identity_mask: &[u8]) -> EtlResult<u32> {
        debug_assert_eq!(replication_mask.len(), identity_mask.len());
        let slot = unsafe { etlg_table_ready(self.ctx, table_id, snapshot_lsn, replication_mask.as_ptr(), identity_mask.as_ptr(), replication_mask.len() as u32) };
        if slot < 0 { Err(self.last_error()) } else { Ok(slot as u32) }
    }

    /// `SharedTableCache::remove_table` (table_cache.rs:131-145).
    pub fn forget_table(&mut self, table_id: u32) {
        unsafe { etlg_table_forget(self.ctx, table_id) };
    }

    pub fn set_worker(&mut self, table_sync_table: Option<u32>, bootstrap_snapshot_lsn: u64) {
        let (kind, id) = match table_sync_table { Some(t) => (ETLG_WORKER_TABLE_SYNC, t), None => (ETLG_WORKER_APPLY, 0) };
        unsafe { etlg_ctx_set_worker(self.ctx, kind, id, bootstrap_snapshot_lsn) };
    }

    /// `ETLG_F_CHECK_CELLS` for every batch `decode_async` enqueues (default off: the crate behaves as before). With it a json /
    /// jsonb cell that is not one JSON value and an array literal the reference rejects are decode errors at their frame, like every
    /// other cell error — which is what makes `finish`'s "events BEFORE the failing frame" promise hold for json and array errors.
    /// Without it such a cell comes back as deferred text, `materialize::events` finds it, and the whole batch's events are lost.
    pub fn set_check_cells(&mut self, on: bool) {
        self.check_cells = on;
    }

    /// The raw context, for `StagingBatcher::new` (its buffers are pinned through the context's device).
    pub fn raw(&self) -> *mut etlg_ctx {
        self.ctx
    }

    /// Enqueues one staged batch: `ETLG_F_ASYNC | ETLG_F_OUTPUT_ON_DEVICE`, host input. The library uploads the pinned buffer on its
    /// copy stream beside the decode of the batch issued before (include/etlg.h) and returns at once; the staged buffer travels with
    /// the handle and must not be touched until `finish` gives it back. Keep fewer than 32 batches in flight and finish them in
    /// issue order.
    pub fn decode_async(&mut self, staged: StagedBatch) -> Result<InFlight, (StagedBatch, EtlError)> {
        let mut batch = ptr::null_mut();
        // (ETLG_F_FINISH_CELLS: arrays arrive typed and floats exact — materialize.rs then parses no array text on the host)
        let flags = ETLG_F_ASYNC | ETLG_F_OUTPUT_ON_DEVICE | ETLG_F_FINISH_CELLS | if staged.control_free { ETLG_F_NO_CONTROL } else { 0 } | if self.check_cells { ETLG_F_CHECK_CELLS } else { 0 };
        let rc = unsafe { etlg_decode(self.ctx, staged.frames_ptr(), staged.len, staged.offsets_ptr(), staged.nframes, flags, &mut batch) };
        if batch.is_null() {
            let _ = rc;
            let e = self.last_error();
            return Err((staged, e));
        }
        Ok(InFlight { ctx: self.ctx, batch, staged: Some(staged) })
    }

    /// Has the batch been decoded? Never blocks... it is `finish` that waits. (The C ABI has no non-blocking probe: a loop that
    /// wants one keeps a batch in flight for one fill period of the next buffer — by then it is done — and calls `finish`.)
    ///
    /// Collects a batch issued by `decode_async`: waits for it (`etlg_batch_sync`, issue order), copies the arena to the host
    /// (`etlg_batch_download`) and materialises the events. On a decode error (fail-fast, apply.rs:2475-2481) the events BEFORE the
    /// failing frame are returned with the error. The staged buffer comes back for `StagingBatcher::recycle`.
    pub fn finish(&mut self, f: InFlight, schemas: &mut dyn materialize::SlotSchemas) -> (Vec<Event>, StagedBatch, EtlResult<()>) {
        let mut f = f;
        let (batch, staged) = f.take();
        let rc = unsafe { etlg_batch_sync(self.ctx, batch) };
        let status = if rc == ETLG_OK { Ok(()) } else { Err(self.last_error()) };
        if unsafe { etlg_batch_download(self.ctx, batch) } != ETLG_OK {
            let e = self.last_error();
            unsafe { etlg_batch_free(batch) };
            return (Vec::new(), staged, Err(e));
        }
        let mut view = std::mem::MaybeUninit::<etlg_batch_view>::uninit();
        unsafe { etlg_batch_view_get(batch, view.as_mut_ptr()) };
        let view = unsafe { view.assume_init() };
        let events = unsafe { materialize::events(&view, schemas) };
        unsafe { etlg_batch_free(batch) };
        match events {
            Ok(ev) => (ev, staged, status),
            Err(e) => (Vec::new(), staged, Err(e)),
        }
    }

    /// One message that does not fit a staging buffer (`StagingBatcher::can_stage` says no: a pgoutput tuple may approach 1 GB), decoded by
    /// itself: re-framed into an ordinary (unpinned) buffer and handed to the library synchronously. Call it with nothing in flight
    /// (dispatch and collect first — the event order holds, and the context carries `remote_final_lsn` / the next ordinal from the
    /// batches before into this one and on into the batches behind). Twin: tests/native/shim_twin.cpp, the `!can_stage` branch.
    pub fn decode_unstaged(&mut self, payload: &[u8], schemas: &mut dyn materialize::SlotSchemas) -> (Vec<Event>, EtlResult<()>) {
        let mut framed = Vec::with_capacity(payload.len() + 5 + 64);
        framed.push(b'd');
        framed.extend_from_slice(&((payload.len() as u32 + 4).to_be_bytes()));
        framed.extend_from_slice(payload);
        let offs = [0u32, framed.len() as u32];
        framed.resize(framed.len() + 64, 0);            // (head room the library's staging copy does not need; kept for symmetry with the ring)
        let mut batch = ptr::null_mut();
        let rc = unsafe { etlg_decode(self.ctx, framed.as_ptr(), offs[1] as usize, offs.as_ptr(), 1, ETLG_F_OUTPUT_ON_DEVICE, &mut batch) };
        if batch.is_null() {
            return (Vec::new(), Err(self.last_error()));
        }
        let status = if rc == ETLG_OK { Ok(()) } else { Err(self.last_error()) };
        if unsafe { etlg_batch_download(self.ctx, batch) } != ETLG_OK {
            let e = self.last_error();
            unsafe { etlg_batch_free(batch) };
            return (Vec::new(), Err(e));
        }
        let mut view = std::mem::MaybeUninit::<etlg_batch_view>::uninit();
        unsafe { etlg_batch_view_get(batch, view.as_mut_ptr()) };
        let view = unsafe { view.assume_init() };
        let events = unsafe { materialize::events(&view, schemas) };
        unsafe { etlg_batch_free(batch) };
        match events {
            Ok(ev) => (ev, status),
            Err(e) => (Vec::new(), Err(e)),
        }
    }

    /// Synchronous form: one staged batch in, its events out (`decode_async` + `finish`).
    pub fn decode(&mut self, staged: StagedBatch, schemas: &mut dyn materialize::SlotSchemas) -> (Vec<Event>, StagedBatch, EtlResult<()>) {
        match self.decode_async(staged) {
            Ok(f) => self.finish(f, schemas),
            Err((staged, e)) => (Vec::new(), staged, Err(e)),
        }
    }
}

/// A batch between `decode_async` and `finish`: the library's handle plus the pinned buffer it is reading.
pub struct InFlight {
    ctx: *mut etlg_ctx,
    batch: *mut etlg_batch,
    staged: Option<StagedBatch>,
}

unsafe impl Send for InFlight {}

impl InFlight {
    pub fn frames(&self) -> &[crate::batcher::FrameMeta] {
        &self.staged.as_ref().expect("batch already collected").meta
    }

    /// Takes the handle and the staged buffer out (for `finish`); what is left drops as a no-op.
    fn take(&mut self) -> (*mut etlg_batch, StagedBatch) {
        (std::mem::replace(&mut self.batch, ptr::null_mut()), self.staged.take().expect("batch already collected"))
    }
}

/// A batch that is dropped without `finish` — an apply loop that bails out with batches still queued (`status?` in gpu_collect) — must
/// not release its pinned buffer while the library's upload or kernels may still be reading it, and must not leave the context's
/// ASYNC chain with an unfinished link: the batch is waited for and freed FIRST, the staged buffer (hipHostFree) goes after it.
/// The decoder has to outlive its in-flight batches (drop the queue before the `GpuDecoder`).
impl Drop for InFlight {
    fn drop(&mut self) {
        if !self.batch.is_null() {
            unsafe {
                let _ = etlg_batch_sync(self.ctx, self.batch);
                etlg_batch_free(self.batch);
            }
            self.batch = ptr::null_mut();
        }
        // self.staged drops here, after the library is done with it
    }
}

/// The reference's own type sizes for `etlg_batch_size_hints` (the device evaluates Event::size_hint, event.rs:295-320, with
/// them): layouts are not ABI-stable, so they are taken from THIS build of the `etl` crate, once.
pub fn reference_size_model() -> etlg_size_model {
    use etl::data::{Cell, TableRow};
    use etl::event::{BeginEvent, CommitEvent, DeleteEvent, InsertEvent, RelationEvent, TruncateEvent, UpdateEvent};
    use etl::schema::ReplicatedTableSchema;
    use std::mem::size_of;
    etlg_size_model {
        begin_event: size_of::<BeginEvent>() as u32,
        commit_event: size_of::<CommitEvent>() as u32,
        insert_event: size_of::<InsertEvent>() as u32,
        update_event: size_of::<UpdateEvent>() as u32,
        delete_event: size_of::<DeleteEvent>() as u32,
        truncate_event: size_of::<TruncateEvent>() as u32,
        relation_event: size_of::<RelationEvent>() as u32,
        replicated_table_schema: size_of::<ReplicatedTableSchema>() as u32,
        table_row: size_of::<TableRow>() as u32,
        cell: size_of::<Cell>() as u32,
        _reserved: [0; 2],
    }
}

impl GpuDecoder {
    /// Device-resident decode + per-event size hints, for a batcher that wants the reference's cut points
    /// (EventBatch::push, apply.rs:656-657; flush rule :1932-1935) without materialising `Event`s first. Entries with
    /// ETLG_SIZE_HINT_INCOMPLETE set hold everything but the parts only the host can size (json / array cells, partial rows).
    pub fn size_hints(&mut self, batch: *mut etlg_batch, n_events: usize) -> EtlResult<Vec<u64>> {
        let model = reference_size_model();
        let mut out = vec![0u64; n_events];
        let rc = unsafe { etlg_batch_size_hints(self.ctx, batch, &model, 0, out.as_mut_ptr()) };
        if rc == ETLG_OK { Ok(out) } else { Err(self.last_error()) }
    }

    /// The write_events cut points of events `[first, end)` of a device-resident batch, found on the device (etlg_batch_cuts): the
    /// exclusive ends of the batches the reference's rule closes (apply.rs:656-657, :1932-1945) when it starts with `carry_in` bytes and
    /// flushes at `budget` — no hint is downloaded. At most `cap` cuts come back; `info.n_cuts` is the full count (resume from the last
    /// cut with carry 0), `info.stop_event < end` names the first event the host has to size (json / array cells, partial rows), and
    /// `info.carry_out` is what the next range, or the next decoded batch, starts with.
    pub fn cuts(&mut self, batch: *mut etlg_batch, first: u64, end: u64, budget: u64, carry_in: u64, cap: usize) -> EtlResult<(Vec<u64>, etlg_cuts_info)> {
        let model = reference_size_model();
        let mut out = vec![0u64; cap];
        let mut info = etlg_cuts_info { n_cuts: 0, stop_event: first, carry_out: carry_in, total: 0 };
        let rc = unsafe {
            etlg_batch_cuts(self.ctx, batch, &model, std::ptr::null(), first, end, budget, carry_in, 0, if cap == 0 { std::ptr::null_mut() } else { out.as_mut_ptr() }, cap as u64, &mut info)
        };
        if rc != ETLG_OK {
            return Err(self.last_error());
        }
        out.truncate(info.n_cuts.min(cap as u64) as usize);
        Ok((out, info))
    }

    /// The pass plan of a sink's `write_events` loop over events `[first, end)` of a device-resident batch, built on the device
    /// (etlg_batch_outline): where the passes of the loop all five destinations share end (clickhouse/core.rs:1063-1164), which slots
    /// each pass holds rows of, where its Relation events `[data_end, rel_end)` and its Truncates are, and what every slot holds by kind.
    /// `cuts`: the range ends `GpuDecoder::cuts` returned, empty for one range; `opts`: `ETLG_OL_RELATIONS_INLINE` for Iceberg's loop. At
    /// most `passes_cap` passes and `trunc_cap` truncate entries come back; `info.n_passes` / `info.n_trunc` are the full counts — call
    /// again with larger caps. `info.status == ETLG_OL_BAD_CUTS` comes with nothing but `info.bad_cut`.
    pub fn outline(&mut self, batch: *mut etlg_batch, first: u64, end: u64, cuts: &[u64], opts: u32, passes_cap: usize, trunc_cap: usize) -> EtlResult<Outline> {
        let mut view = std::mem::MaybeUninit::<etlg_batch_view>::uninit();
        unsafe { etlg_batch_view_get(batch, view.as_mut_ptr()) };
        let n_slots = unsafe { view.assume_init() }.n_slots as usize;
        let words = (n_slots + 63) / 64;
        let mut out = Outline {
            passes: vec![etlg_outline_pass { first_event: 0, data_end: 0, rel_end: 0, end_event: 0, range: 0, trunc_first: 0, n_trunc: 0 }; passes_cap],
            ends: vec![0u64; passes_cap],
            touched: vec![0u64; passes_cap * words],
            words,
            truncates: vec![etlg_outline_trunc { table_id: 0, schema_slot: 0, event: 0 }; trunc_cap],
            slots: vec![etlg_outline_slot { rows: [0; 6], first: [u64::MAX; 6] }; n_slots],
            info: etlg_outline_info { n_passes: 0, n_trunc: 0, n_relations: 0, n_rows: 0, n_ranges: 0, bad_cut: 0, status: 0, _pad: 0 },
        };
        fn ptr<T>(v: &mut Vec<T>) -> *mut T { if v.is_empty() { std::ptr::null_mut() } else { v.as_mut_ptr() } }
        let rc = unsafe {
            etlg_batch_outline(
                self.ctx, batch, first, end, if cuts.is_empty() { std::ptr::null() } else { cuts.as_ptr() }, cuts.len() as u64, 0, opts, 0,
                ptr(&mut out.passes), ptr(&mut out.ends), ptr(&mut out.touched), passes_cap as u64, ptr(&mut out.truncates), trunc_cap as u64, ptr(&mut out.slots), &mut out.info,
            )
        };
        if rc != ETLG_OK {
            return Err(self.last_error());
        }
        let (p, k) = (out.info.n_passes.min(passes_cap as u64) as usize, out.info.n_trunc.min(trunc_cap as u64) as usize);
        out.passes.truncate(p);
        out.ends.truncate(p);
        out.touched.truncate(p * words);
        out.truncates.truncate(k);
        Ok(out)
    }

    /// The DuckLake sink's atomic batches of one schema slot of a device-resident batch, cut on the device (etlg_ducklake_plan): the
    /// replay filter (`retain_mutations_after_sequence_key`, ducklake/batches.rs:932-946), the groups of 16 with their identity fields
    /// (`prepare_mutation_table_batches` :727-758) and each group's DuckDB operations (`prepare_table_mutations` :1128-1226).
    /// `passes`: what `GpuDecoder::outline` returned — only `[first_event, data_end)` is read. `watermark`: the sequence key already
    /// applied. `tuples` / `predicates` / `updates`: the device-resident `etlg_batch_duckdb` objects of this batch and slot, or null.
    /// At most `batches_cap` groups and `ops_cap` ops come back; `info.n_batches` / `info.n_ops` are the full counts — call again with
    /// larger caps. With `info.status != ETLG_DLP_OK` nothing but `info` is set. `ranges` is what `etlg_ducklake_fingerprints` takes.
    #[allow(clippy::too_many_arguments)]
    pub fn ducklake_plan(
        &mut self, batch: *mut etlg_batch, schema_slot: i32, passes: &[etlg_outline_pass], watermark: Option<(u64, u64)>, seed: u64, tuples: *const etlg_rowbinary,
        predicates: *const etlg_rowbinary, updates: *const etlg_rowbinary, batches_cap: usize, ops_cap: usize,
    ) -> EtlResult<DuckLakePlan> {
        let mut out = DuckLakePlan {
            ranges: (0..batches_cap).map(|_| etlg_dl_range { first_event: 0, end_event: 0, seed: 0 }).collect(),
            batches: vec![
                etlg_dl_batch {
                    first_event: 0, end_event: 0, first_start_lsn: 0, last_commit_lsn: 0, first_commit_lsn: 0, first_tx_ordinal: 0, last_tx_ordinal: 0, window: 0, op_first: 0,
                    n_members: 0, n_ops: 0, n_cat: [0; 5], _pad: 0,
                };
                batches_cap
            ],
            ops: vec![etlg_dl_op { kind: 0, origin: 0, first_event: 0, n: 0, rec_first: 0 }; ops_cap],
            info: etlg_dl_plan_info { n_batches: 0, n_ops: 0, n_members: 0, n_retained: 0, n_dropped: 0, event: 0, bad_pass: 0, status: 0, reason: 0 },
        };
        fn ptr<T>(v: &mut Vec<T>) -> *mut T { if v.is_empty() { std::ptr::null_mut() } else { v.as_mut_ptr() } }
        let (has_wm, wm_lsn, wm_ord) = match watermark { Some((l, o)) => (1, l, o), None => (0, 0, 0) };
        let rc = unsafe {
            etlg_ducklake_plan(
                self.ctx, batch, schema_slot, if passes.is_empty() { std::ptr::null() } else { passes.as_ptr() }, passes.len() as u64, 0, has_wm, wm_lsn, wm_ord, seed,
                tuples, predicates, updates, 0, ptr(&mut out.ranges), ptr(&mut out.batches), batches_cap as u64, ptr(&mut out.ops), ops_cap as u64, &mut out.info,
            )
        };
        if rc != ETLG_OK {
            return Err(self.last_error());
        }
        let ok = out.info.status == ETLG_DLP_OK;
        let (b, k) = if ok { (out.info.n_batches.min(batches_cap as u64) as usize, out.info.n_ops.min(ops_cap as u64) as usize) } else { (0, 0) };
        out.ranges.truncate(b);
        out.batches.truncate(b);
        out.ops.truncate(k);
        Ok(out)
    }

    /// The Snowflake sink's row batches of one schema slot of a device-resident batch, planned on the device (etlg_snowflake_plan): what
    /// `encode_insert` / `encode_update` / `encode_delete` (snowflake/core.rs:345-438) and `RowBatchBuilder::push_row`
    /// (snowflake/streaming/batch.rs:150-189) decide per row — the committed-offset test, the three refusals and where the encoder is
    /// flushed — as segments of consecutive rows of `ndjson`, the device-resident `etlg_batch_ndjson` object of this batch and slot.
    /// `passes`: what `GpuDecoder::outline` returned — only `[first_event, data_end)` is read; empty on a table-copy batch (one window
    /// over all rows). `committed`: the channel's committed offset. The reference's thresholds are `ETLG_SF_MAX_UNFLUSHED_BYTES` and
    /// `ETLG_SF_MAX_ROW_BYTES`. At most `segs_cap` segments come back; `info.n_segs` is the full count — call again with a larger cap.
    /// With `info.status != ETLG_SFP_OK` nothing but `info` is set. Per segment the host flushes when `flush_before != 0`, checks the
    /// compressed size with `first_row_bytes`, writes `bytes[byte_first..byte_end]` in one `write_all` and extends the offset range.
    #[allow(clippy::too_many_arguments)]
    pub fn snowflake_plan(
        &mut self, batch: *mut etlg_batch, schema_slot: i32, passes: &[etlg_outline_pass], committed: Option<(u64, u64)>, ndjson: *const etlg_rowbinary, flush_bytes: u64,
        max_row_bytes: u64, segs_cap: usize,
    ) -> EtlResult<SnowflakePlan> {
        let n_windows = if passes.is_empty() { 1 } else { passes.len() };
        let mut out = SnowflakePlan {
            segments: vec![
                etlg_sf_segment {
                    window: 0, first_row: 0, end_row: 0, first_event: 0, last_event: 0, byte_first: 0, byte_end: 0, first_row_bytes: 0, first_commit_lsn: 0, first_tx_ordinal: 0,
                    last_commit_lsn: 0, last_tx_ordinal: 0, flush_before: 0, _pad: 0,
                };
                segs_cap
            ],
            windows: vec![etlg_sf_window { seg_first: 0, n_segs: 0, first_row: 0, end_row: 0, n_members: 0, n_retained: 0, n_bytes: 0 }; n_windows],
            info: etlg_sf_plan_info { n_segs: 0, n_members: 0, n_retained: 0, n_dropped: 0, n_rows: 0, n_bytes: 0, event: 0, row_bytes: 0, bad_pass: 0, status: 0, reason: 0 },
        };
        let (has_c, c_lsn, c_ord) = match committed { Some((l, o)) => (1, l, o), None => (0, 0, 0) };
        let rc = unsafe {
            etlg_snowflake_plan(
                self.ctx, batch, schema_slot, if passes.is_empty() { std::ptr::null() } else { passes.as_ptr() }, passes.len() as u64, 0, has_c, c_lsn, c_ord, ndjson,
                flush_bytes, max_row_bytes, 0, if segs_cap == 0 { std::ptr::null_mut() } else { out.segments.as_mut_ptr() }, segs_cap as u64, out.windows.as_mut_ptr(),
                &mut out.info,
            )
        };
        if rc != ETLG_OK {
            return Err(self.last_error());
        }
        let ok = out.info.status == ETLG_SFP_OK;
        out.segments.truncate(if ok { out.info.n_segs.min(segs_cap as u64) as usize } else { 0 });
        if !ok {
            out.windows.clear();
        }
        Ok(out) // (no passes: `windows` has one entry, the whole-batch window of a table-copy batch; all zeros for any other batch)
    }

    /// The ClickHouse sink's INSERT statements of one schema slot of a device-resident batch, cut on the device (etlg_clickhouse_plan):
    /// which events `write_events_inner` (clickhouse/core.rs:1063-1136) refuses and where `insert_rows` (clickhouse/client.rs:565-649)
    /// opens and commits each statement, as ranges of consecutive rows of `rowbinary`, the device-resident `etlg_batch_rowbinary` object
    /// of this batch and slot; the object's engine decides the refusals. `passes`: what `GpuDecoder::outline` returned — only
    /// `[first_event, data_end)` is read; empty on a table-copy batch (one window over all rows). The reference's budget is
    /// `ETLG_CH_MAX_BYTES_PER_INSERT`. At most `stmts_cap` statements come back; `info.n_stmts` is the full count — call again with a
    /// larger cap. With `info.status != ETLG_CHP_OK` nothing but `info` is set; for `ETLG_CHP_FAILED` the reference has written the
    /// passes in front of `info.fail_pass`: plan again with those alone. Per statement the host does one INSERT of
    /// `bytes[byte_first..byte_end]`.
    pub fn clickhouse_plan(
        &mut self, batch: *mut etlg_batch, schema_slot: i32, passes: &[etlg_outline_pass], rowbinary: *const etlg_rowbinary, max_bytes_per_insert: u64, stmts_cap: usize,
    ) -> EtlResult<ClickHousePlan> {
        let n_windows = if passes.is_empty() { 1 } else { passes.len() };
        let mut out = ClickHousePlan {
            statements: vec![etlg_ch_statement { window: 0, first_row: 0, end_row: 0, first_event: 0, last_event: 0, byte_first: 0, byte_end: 0 }; stmts_cap],
            windows: vec![etlg_ch_window { stmt_first: 0, n_stmts: 0, first_row: 0, end_row: 0, n_members: 0, n_bytes: 0 }; n_windows],
            info: etlg_ch_plan_info { n_stmts: 0, n_members: 0, n_rows: 0, n_bytes: 0, event: 0, bad_pass: 0, fail_pass: 0, status: 0, reason: 0 },
        };
        let rc = unsafe {
            etlg_clickhouse_plan(
                self.ctx, batch, schema_slot, if passes.is_empty() { std::ptr::null() } else { passes.as_ptr() }, passes.len() as u64, 0, rowbinary, max_bytes_per_insert, 0,
                if stmts_cap == 0 { std::ptr::null_mut() } else { out.statements.as_mut_ptr() }, stmts_cap as u64, out.windows.as_mut_ptr(), &mut out.info,
            )
        };
        if rc != ETLG_OK {
            return Err(self.last_error());
        }
        let ok = out.info.status == ETLG_CHP_OK;
        out.statements.truncate(if ok { out.info.n_stmts.min(stmts_cap as u64) as usize } else { 0 });
        if !ok {
            out.windows.clear();
        }
        Ok(out) // (no passes: `windows` has one entry, the whole-batch window of a table-copy batch; all zeros for any other batch)
    }

    /// The BigQuery sink's append requests of one schema slot of a device-resident batch, planned on the device (etlg_bigquery_plan):
    /// which events `write_events` (bigquery/core.rs:956-1040) refuses and which rows form the `create_append_request` of each pass
    /// (:1043-1064), as ranges of consecutive rows of `protobuf`, the device-resident `etlg_batch_protobuf` object of this batch and
    /// slot; an Update that changed the primary key is two rows of one event. `passes`: what `GpuDecoder::outline` returned — only
    /// `[first_event, data_end)` is read; empty on a table-copy batch, whose rows `split_table_rows` (:1790-1827) cuts by
    /// `max_batch_bytes`, the client crate's `MAX_BATCH_SIZE_BYTES` (ignored elsewhere). At most `reqs_cap` requests come back;
    /// `info.n_reqs` is the full count — call again with a larger cap. With `info.status != ETLG_BQP_OK` nothing but `info` is set;
    /// for `ETLG_BQP_FAILED` the reference has written the passes in front of `info.fail_pass`: plan again with those alone.
    pub fn bigquery_plan(
        &mut self, batch: *mut etlg_batch, schema_slot: i32, passes: &[etlg_outline_pass], protobuf: *const etlg_rowbinary, max_batch_bytes: u64, reqs_cap: usize,
    ) -> EtlResult<BigQueryPlan> {
        let n_windows = if passes.is_empty() { 1 } else { passes.len() };
        let mut out = BigQueryPlan {
            requests: vec![etlg_bq_request { window: 0, first_row: 0, end_row: 0, first_event: 0, last_event: 0, byte_first: 0, byte_end: 0, n_members: 0 }; reqs_cap],
            windows: vec![etlg_bq_window { req_first: 0, n_reqs: 0, first_row: 0, end_row: 0, n_members: 0, n_two_row: 0, n_bytes: 0 }; n_windows],
            info: etlg_bq_plan_info {
                n_reqs: 0, n_members: 0, n_rows: 0, n_two_row: 0, n_bytes: 0, est_row_bytes: 0, target_batches: 0, event: 0, bad_pass: 0, fail_pass: 0, status: 0, reason: 0,
            },
        };
        let rc = unsafe {
            etlg_bigquery_plan(
                self.ctx, batch, schema_slot, if passes.is_empty() { std::ptr::null() } else { passes.as_ptr() }, passes.len() as u64, 0, protobuf, max_batch_bytes, 0,
                if reqs_cap == 0 { std::ptr::null_mut() } else { out.requests.as_mut_ptr() }, reqs_cap as u64, out.windows.as_mut_ptr(), &mut out.info,
            )
        };
        if rc != ETLG_OK {
            return Err(self.last_error());
        }
        let ok = out.info.status == ETLG_BQP_OK;
        out.requests.truncate(if ok { out.info.n_reqs.min(reqs_cap as u64) as usize } else { 0 });
        if !ok {
            out.windows.clear();
        }
        Ok(out) // (no passes: `windows` has one entry, the whole-batch window of a table-copy batch; all zeros for any other batch)
    }

    /// The Iceberg sink's writes of one schema slot of a device-resident batch, planned on the device (etlg_iceberg_plan): which events
    /// `write_events` (iceberg/core.rs:300-440) refuses, which rows of `changelog` — the device-resident `etlg_batch_iceberg` object of
    /// this batch and slot — form the `insert_rows` of each pass (:395-409), and per write and column of the object the Arrow slice over
    /// those rows. `passes`: what `GpuDecoder::outline` returned WITH `ETLG_OL_RELATIONS_INLINE` — only `[first_event, data_end)` is
    /// read; empty on a table-copy batch. `n_cols`: the object's `etlg_columns_view.n_cols`. At most `writes_cap` writes (and
    /// `writes_cap * n_cols` slices) come back; `info.n_writes` is the full count — call again with a larger cap. With `info.status !=
    /// ETLG_ICP_OK` nothing but `info` is set; for `ETLG_ICP_FAILED` the reference has written the passes in front of `info.fail_pass`:
    /// plan again with those alone.
    pub fn iceberg_plan(
        &mut self, batch: *mut etlg_batch, schema_slot: i32, passes: &[etlg_outline_pass], changelog: *const etlg_columns, n_cols: usize, writes_cap: usize,
    ) -> EtlResult<IcebergPlan> {
        let n_windows = if passes.is_empty() { 1 } else { passes.len() };
        let mut out = IcebergPlan {
            writes: vec![etlg_ice_write { window: 0, first_row: 0, end_row: 0, first_event: 0, last_event: 0, n_members: 0, other_slot_event: 0 }; writes_cap],
            slices: vec![
                etlg_ice_slice { null_count: 0, deferred_count: 0, byte_first: 0, byte_end: 0, child_first: 0, child_end: 0, child_null_count: 0 };
                writes_cap * n_cols
            ],
            windows: vec![etlg_ice_window { write_first: 0, n_writes: 0, first_row: 0, end_row: 0, n_members: 0, other_slot_event: 0 }; n_windows],
            info: etlg_ice_plan_info { n_writes: 0, n_members: 0, n_rows: 0, n_mixed: 0, event: 0, bad_pass: 0, fail_pass: 0, status: 0, reason: 0 },
            n_cols,
        };
        let rc = unsafe {
            etlg_iceberg_plan(
                self.ctx, batch, schema_slot, if passes.is_empty() { std::ptr::null() } else { passes.as_ptr() }, passes.len() as u64, 0, changelog, 0,
                if writes_cap == 0 { std::ptr::null_mut() } else { out.writes.as_mut_ptr() }, writes_cap as u64,
                if writes_cap * n_cols == 0 { std::ptr::null_mut() } else { out.slices.as_mut_ptr() }, out.windows.as_mut_ptr(), &mut out.info,
            )
        };
        if rc != ETLG_OK {
            return Err(self.last_error());
        }
        let ok = out.info.status == ETLG_ICP_OK;
        let n = if ok { out.info.n_writes.min(writes_cap as u64) as usize } else { 0 };
        out.writes.truncate(n);
        out.slices.truncate(n * n_cols);
        if !ok {
            out.windows.clear();
        }
        Ok(out) // (no passes: `windows` has one entry, the whole-batch window of a table-copy batch; all zeros for any other batch)
    }

    /// Source payload accounting of a device-resident batch, on the device (etlg_batch_payload), as plain values: per event the value
    /// bytes of its message (what `StreamingPayloadMetadata::{insert,update,delete}` is built from, apply.rs:2459-2463; the kind is the
    /// event's), per range of `cuts` the merged bytes and rows per kind (what `EventBatch::push` accumulates, apply.rs:656-658; rows == 0
    /// is `None`), the histogram of `etl_row_size_bytes` over `bounds` and, in the info, what `record_received` counts — every row
    /// message of the batch, owned or not. Called on a batch in flight, BEFORE `finish` (which downloads the arena and frees the batch):
    /// the batch is waited for here, and its staged buffer is the input the call reads again. `cuts` as `GpuDecoder::cuts` returns them,
    /// empty for one range. A batch that ended in a decode error is accounted up to the error (its events are delivered).
    pub fn payload(&mut self, f: &InFlight, cuts: &[u64], bounds: &[u64]) -> EtlResult<PayloadAccount> {
        let (batch, staged) = (f.batch, f.staged.as_ref().expect("batch already collected"));
        let _ = unsafe { etlg_batch_sync(self.ctx, batch) };             // (a decode error is `finish`'s to report)
        let mut view = std::mem::MaybeUninit::<etlg_batch_view>::uninit();
        unsafe { etlg_batch_view_get(batch, view.as_mut_ptr()) };
        let n_events = unsafe { view.assume_init() }.n_events as usize;
        let mut acc = PayloadAccount {
            ev_bytes: vec![0u32; n_events],
            sums: (0..cuts.len() + 1).map(|_| etlg_payload_sums { bytes: [0; 4], rows: [0; 4] }).collect(),
            hist: vec![0u64; 4 * (bounds.len() + 1)],
            info: etlg_payload_info { received_bytes: [0; 4], received_rows: [0; 4], n_ranges: 0, status: 0, _pad: 0, mismatch_event: u64::MAX },
        };
        let rc = unsafe {
            etlg_batch_payload(
                self.ctx, batch, staged.frames_ptr(), staged.len, staged.offsets_ptr(), staged.nframes,
                if cuts.is_empty() { std::ptr::null() } else { cuts.as_ptr() }, cuts.len() as u64, 0,
                if bounds.is_empty() { std::ptr::null() } else { bounds.as_ptr() }, bounds.len() as u32, 0,
                if n_events == 0 { std::ptr::null_mut() } else { acc.ev_bytes.as_mut_ptr() }, acc.sums.as_mut_ptr(), acc.hist.as_mut_ptr(), &mut acc.info,
            )
        };
        if rc == ETLG_OK { Ok(acc) } else { Err(self.last_error()) }
    }
}

/// What `GpuDecoder::outline` returns. `touched[p * words + s / 64]` holds bit `s % 64` when pass `p` has rows of slot `s`.
pub struct Outline {
    pub passes: Vec<etlg_outline_pass>,
    pub ends: Vec<u64>,
    pub touched: Vec<u64>,
    pub words: usize,
    pub truncates: Vec<etlg_outline_trunc>,
    pub slots: Vec<etlg_outline_slot>,
    pub info: etlg_outline_info,
}

impl Outline {
    /// The truncate entries pass `p` acts on: the first entry per table, as `truncate_schemas.entry(id).or_insert(schema)` keeps it
    /// (clickhouse/core.rs:1148-1155). Entries beyond `trunc_cap` are not there to be looked at.
    pub fn truncated_tables(&self, p: usize) -> Vec<etlg_outline_trunc> {
        let (lo, n) = (self.passes[p].trunc_first as usize, self.passes[p].n_trunc as usize);
        let mut out: Vec<etlg_outline_trunc> = Vec::new();
        for t in self.truncates.iter().skip(lo).take(n) {
            if !out.iter().any(|o| o.table_id == t.table_id) {
                out.push(*t);
            }
        }
        out
    }
}

/// What `GpuDecoder::ducklake_plan` returns.
pub struct DuckLakePlan {
    pub ranges: Vec<etlg_dl_range>,
    pub batches: Vec<etlg_dl_batch>,
    pub ops: Vec<etlg_dl_op>,
    pub info: etlg_dl_plan_info,
}

impl DuckLakePlan {
    /// The ops of group `b` that were written (those beyond `ops_cap` are not there to be looked at).
    pub fn ops_of(&self, b: usize) -> &[etlg_dl_op] {
        let (lo, n) = (self.batches[b].op_first as usize, self.batches[b].n_ops as usize);
        let hi = (lo + n).min(self.ops.len());
        &self.ops[lo.min(hi)..hi]
    }
}

/// What `GpuDecoder::snowflake_plan` returns.
pub struct SnowflakePlan {
    pub segments: Vec<etlg_sf_segment>,
    pub windows: Vec<etlg_sf_window>,
    pub info: etlg_sf_plan_info,
}

impl SnowflakePlan {
    /// The segments of window `w` that were written (those beyond `segs_cap` are not there to be looked at).
    pub fn segments_of(&self, w: usize) -> &[etlg_sf_segment] {
        let (lo, n) = (self.windows[w].seg_first as usize, self.windows[w].n_segs as usize);
        let hi = (lo + n).min(self.segments.len());
        &self.segments[lo.min(hi)..hi]
    }
}

/// What `GpuDecoder::clickhouse_plan` returns.
pub struct ClickHousePlan {
    pub statements: Vec<etlg_ch_statement>,
    pub windows: Vec<etlg_ch_window>,
    pub info: etlg_ch_plan_info,
}

impl ClickHousePlan {
    /// The statements of window `w` that were written (those beyond `stmts_cap` are not there to be looked at).
    pub fn statements_of(&self, w: usize) -> &[etlg_ch_statement] {
        let (lo, n) = (self.windows[w].stmt_first as usize, self.windows[w].n_stmts as usize);
        let hi = (lo + n).min(self.statements.len());
        &self.statements[lo.min(hi)..hi]
    }
}

/// What `GpuDecoder::bigquery_plan` returns.
pub struct BigQueryPlan {
    pub requests: Vec<etlg_bq_request>,
    pub windows: Vec<etlg_bq_window>,
    pub info: etlg_bq_plan_info,
}

impl BigQueryPlan {
    /// The requests of window `w` that were written (those beyond `reqs_cap` are not there to be looked at).
    pub fn requests_of(&self, w: usize) -> &[etlg_bq_request] {
        let (lo, n) = (self.windows[w].req_first as usize, self.windows[w].n_reqs as usize);
        let hi = (lo + n).min(self.requests.len());
        &self.requests[lo.min(hi)..hi]
    }
}

/// What `GpuDecoder::iceberg_plan` returns.
pub struct IcebergPlan {
    pub writes: Vec<etlg_ice_write>,
    pub slices: Vec<etlg_ice_slice>,
    pub windows: Vec<etlg_ice_window>,
    pub info: etlg_ice_plan_info,
    pub n_cols: usize,
}

impl IcebergPlan {
    /// The slices of write `k`, one per column of the changelog object.
    pub fn slices_of(&self, k: usize) -> &[etlg_ice_slice] {
        &self.slices[k * self.n_cols..(k + 1) * self.n_cols]
    }
}

/// What `GpuDecoder::payload` returns. `hist[k * (bounds + 1) + j]`: messages of kind k (ETLG_PK_*) in bucket j, the last the overflow.
pub struct PayloadAccount {
    pub ev_bytes: Vec<u32>,
    pub sums: Vec<etlg_payload_sums>,
    pub hist: Vec<u64>,
    pub info: etlg_payload_info,
}

/// The multi-GPU recipe (one `GpuDecoder` per device, one process or task per GPU — the reference itself has a single
/// apply task, apply.rs:1210-1336, so this is an extension a host opts into): `shard_plan` cuts a staged stream behind Commit frames,
/// every rank extracts the control stream of its own range (`control_stream`), the ranks exchange those few hundred bytes, every rank
/// replays the streams of the ranks before it (`shard_replay`, rank order) and then decodes its own range. Python twin with the
/// collectives: etl_amd/shard.py; the C entry points are the ones tests/test_shard_decode.py compares against that model.
impl GpuDecoder {
    /// Commit-aligned, byte-balanced frame ranges `[cuts[k], cuts[k + 1])` of a staged batch (etlg_shard_plan).
    pub fn shard_plan(&mut self, staged: &StagedBatch, n_shards: u32) -> EtlResult<Vec<u64>> {
        let mut cuts = vec![0u64; n_shards as usize + 1];
        let rc = unsafe { etlg_shard_plan(self.ctx, staged.frames_ptr(), staged.len, staged.offsets_ptr(), staged.nframes, n_shards, 0, cuts.as_mut_ptr()) };
        if rc == ETLG_OK { Ok(cuts) } else { Err(self.last_error()) }
    }

    /// The Relation / DDL-message transactions of a frame range of a staged batch, reduced to {Begin, control frames, Commit}
    /// (etlg_control_stream): what this rank broadcasts. Returns (bytes, offsets).
    pub fn control_stream(&mut self, staged: &StagedBatch, f0: usize, f1: usize) -> EtlResult<(Vec<u8>, Vec<u32>)> {
        let offs = unsafe { std::slice::from_raw_parts(staged.offsets_ptr(), staged.nframes + 1) };
        let (b0, b1) = (offs[f0] as usize, offs[f1] as usize);
        let rel: Vec<u32> = offs[f0..=f1].iter().map(|o| o - offs[f0]).collect();
        let (mut bytes, mut out_offs) = (vec![0u8; 1 << 16], vec![0u32; 1 << 10]);
        loop {
            let (mut nb, mut nf, mut last) = (0usize, 0usize, 0u32);
            let rc = unsafe {
                etlg_control_stream(self.ctx, staged.frames_ptr().add(b0), b1 - b0, rel.as_ptr(), f1 - f0, 0, bytes.as_mut_ptr(), bytes.len(),
                                    out_offs.as_mut_ptr(), out_offs.len(), &mut nb, &mut nf, &mut last)
            };
            if rc == ETLG_OK {
                bytes.truncate(nb);
                out_offs.truncate(nf + 1);
                return Ok((bytes, out_offs));
            }
            if nb <= bytes.len() && nf + 1 <= out_offs.len() { return Err(self.last_error()); }
            bytes = vec![0u8; nb + 64];
            out_offs = vec![0u32; nf + 2];
        }
    }

    /// Applies the control stream of an EARLIER rank's range (etlg_shard_replay): same schema slots in the same order on every rank;
    /// leaves the context outside any transaction, where a commit-aligned shard starts.
    pub fn shard_replay(&mut self, bytes: &[u8], offsets: &[u32]) -> EtlResult<()> {
        let nframes = offsets.len().saturating_sub(1);
        let rc = unsafe { etlg_shard_replay(self.ctx, if nframes == 0 { ptr::null() } else { bytes.as_ptr() }, bytes.len(), offsets.as_ptr(), nframes) };
        if rc == ETLG_OK { Ok(()) } else { Err(self.last_error()) }
    }
}

impl Drop for GpuDecoder {
    fn drop(&mut self) {
        unsafe { etlg_ctx_destroy(self.ctx) };
    }
}
