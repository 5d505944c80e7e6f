//! Table copy through the GPU stage: the rows of a `CopyOutStream` are staged as bytes and decoded a batch at a time
//! (`etlg_copy_decode`), instead of one `parse_table_row_from_postgres_copy_bytes` call per stream item
//! (crates/etl/src/postgres/stream/table_copy.rs:70-103, crates/etl/src/postgres/codec/table_row.rs:47-254).
//!
//! ```text
//! CopyOutStream ──row bytes──▶ CopyStaging ──rows + offsets (pinned)──▶ GpuDecoder::copy_decode ──arena──▶ materialize::table_rows ──▶ Vec<TableRow>
//! ```
//! The per-row `TableCopyPayloadMetadata` (table_copy.rs:84: the byte length of the text row) stays exact: `CopyStaging` keeps
//! every row's length, and the batch's `payload_bytes[0]` is their sum over the rows that decoded.
//! A device-resident copy batch gets the same call as a WAL batch: `etlg_batch_payload` with the rows and their offsets reports them under `ETLG_PK_COPY`.
use etl::bail;
use etl::data::TableRow;
use etl::error::{ErrorKind, EtlResult};

use crate::batcher::PinnedBuf;
use crate::ffi::*;
use crate::materialize;
use crate::GpuDecoder;

/// Rows of one table-copy batch in page-locked memory: the row payloads back to back exactly as `CopyOutStream` yields them (one
/// COPY text row per item, no `'d'` framing) and `nrows + 1` byte offsets.
pub struct CopyStaging {
    rows: PinnedBuf,
    offsets: PinnedBuf,
    len: usize,
    nrows: usize,
}

impl CopyStaging {
    /// `cap_bytes` of row payload; offsets are sized for rows of at least two bytes (an empty-looking row is still `"\n"` plus a
    /// field).
    pub fn new(decoder: &GpuDecoder, cap_bytes: usize) -> EtlResult<Self> {
        let max_rows = cap_bytes / 2 + 2;
        let mut s = Self { rows: PinnedBuf::new(decoder.raw(), cap_bytes)?, offsets: PinnedBuf::new(decoder.raw(), (max_rows + 1) * 4)?, len: 0, nrows: 0 };
        s.set_offset(0, 0);
        Ok(s)
    }
    fn set_offset(&mut self, i: usize, v: u32) {
        self.offsets.bytes_mut(i * 4, 4).copy_from_slice(&v.to_ne_bytes());
    }
    /// Does the next stream item fit? (If not: `GpuDecoder::copy_decode` what is staged, then `clear`.)
    pub fn fits(&self, row: &[u8]) -> bool {
        self.len + row.len() <= self.rows.capacity() && (self.nrows + 2) * 4 <= self.offsets.capacity() && self.len + row.len() < u32::MAX as usize
    }
    /// Stages one `CopyOutStream` item.
    pub fn push(&mut self, row: &[u8]) -> EtlResult<()> {
        if !self.fits(row) {
            bail!(ErrorKind::InvalidState, "Table-copy staging buffer is full", format!("{} bytes staged, row of {} bytes", self.len, row.len()));
        }
        self.rows.bytes_mut(self.len, row.len()).copy_from_slice(row);
        self.len += row.len();
        self.nrows += 1;
        let (n, l) = (self.nrows, self.len as u32);
        self.set_offset(n, l);
        Ok(())
    }
    pub fn nrows(&self) -> usize {
        self.nrows
    }
    pub fn staged_bytes(&self) -> usize {
        self.len
    }
    /// Byte length of staged row `i`: its `TableCopyPayloadMetadata` (table_copy.rs:84).
    pub fn row_len(&self, i: usize) -> u64 {
        let at = |k: usize| u32::from_ne_bytes(self.offsets.bytes(k * 4, 4).try_into().expect("four bytes")) as u64;
        at(i + 1) - at(i)
    }
    pub fn clear(&mut self) {
        self.len = 0;
        self.nrows = 0;
    }
}

impl GpuDecoder {
    /// Decodes the staged rows against schema slot `schema_slot` (what `table_ready` returned for the table's
    /// `ReplicatedTableSchema`; its replicated columns are the `column_schemas` `TableCopyStream::wrap` was given,
    /// table_copy.rs:64-66). Fail-fast like the stream (table_copy.rs:88-92): on a bad row the rows BEFORE it are returned together
    /// with the reference's error for that row.
    pub fn copy_decode(&mut self, schema_slot: u32, staged: &CopyStaging) -> (Vec<TableRow>, EtlResult<()>) {
        let mut batch = std::ptr::null_mut();
        let rc = unsafe {
            etlg_copy_decode(self.ctx, schema_slot as i32, staged.rows.as_ptr(), staged.len, staged.offsets.as_ptr() as *const u32, staged.nrows, 0, &mut batch)
        };
        if batch.is_null() {
            return (Vec::new(), Err(self.last_error()));
        }
        let status = if rc == ETLG_OK { Ok(()) } else { Err(self.last_error()) };
        let mut view = std::mem::MaybeUninit::<etlg_batch_view>::uninit();
        unsafe { etlg_batch_view_get(batch, view.as_mut_ptr()) };
        let view = unsafe { view.assume_init() };
        let rows = unsafe { materialize::table_rows(&view) };
        unsafe { etlg_batch_free(batch) };
        match rows {
            Ok(r) => (r, status),
            Err(e) => (Vec::new(), Err(e)),
        }
    }

    /// The ASYNC form: enqueues the staged rows (`ETLG_F_ASYNC | ETLG_F_OUTPUT_ON_DEVICE`, host input — the library uploads the pinned
    /// buffers on its copy stream beside the decode of the batch before, include/etlg.h) and returns at once, so that the stream keeps
    /// filling the next `CopyStaging` while this one decodes (two or three in rotation, like the WAL batcher's ring). The staging
    /// travels with the handle and comes back from `copy_finish`. Fewer than 32 in flight, finished in issue order.
    /// Twin: tests/native/shim_twin.cpp `twin_copy_run` (tests/test_shim_twin.py: rows against the oracle's, fail-fast, drop order).
    pub fn copy_decode_async(&mut self, schema_slot: u32, staged: CopyStaging) -> Result<CopyInFlight, (CopyStaging, etl::error::EtlError)> {
        let mut batch = std::ptr::null_mut();
        let rc = unsafe {
            etlg_copy_decode(self.ctx, schema_slot as i32, staged.rows.as_ptr(), staged.len, staged.offsets.as_ptr() as *const u32, staged.nrows,
                             ETLG_F_ASYNC | ETLG_F_OUTPUT_ON_DEVICE, &mut batch)
        };
        if batch.is_null() {
            let _ = rc;
            let e = self.last_error();
            return Err((staged, e));
        }
        Ok(CopyInFlight { ctx: self.ctx, batch, staged: Some(staged) })
    }

    /// Collects a batch issued by `copy_decode_async`: waits for it (`etlg_batch_sync`), copies the arena to the host and materialises
    /// the rows. Fail-fast like the stream (table_copy.rs:88-92): on a bad row the rows BEFORE it come back with the reference's error;
    /// the batches behind it are not affected (table-copy batches share no state).
    pub fn copy_finish(&mut self, f: CopyInFlight) -> (Vec<TableRow>, CopyStaging, EtlResult<()>) {
        let mut f = f;
        let batch = std::mem::replace(&mut f.batch, std::ptr::null_mut());
        let staged = f.staged.take().expect("a batch in flight holds its staging");
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
        let rows = unsafe { materialize::table_rows(&view) };
        unsafe { etlg_batch_free(batch) };
        match rows {
            Ok(r) => (r, staged, status),
            Err(e) => (Vec::new(), staged, Err(e)),
        }
    }
}

/// DuckLake's Arrow copy staging of a table-copy batch (`etlg_batch_ducklake_copy`): what `prepare_copy_rows` builds with
/// `copy_rows_to_arrow_record_batch` (crates/etl-destinations/src/ducklake/encoding.rs:32-49, :303-340), as column buffers in host
/// memory. `view.cols[i].offsets` of an `ETLG_AK_UTF8` / `ETLG_AK_BINARY` column points at `n_rows + 1` i32 entries.
pub struct DuckLakeCopyColumns {
    cols: *mut etlg_columns,
    pub view: etlg_columns_view,
    /// `ETLG_DLC_OK`, or why nothing was built: `ETLG_DLC_NOT_ARROW` (the sink takes `prepare_rows`) / `ETLG_DLC_OFFSETS_OVERFLOW`
    /// (split the batch), with the column it was decided by.
    pub info: etlg_ducklake_copy_info,
}

impl Drop for DuckLakeCopyColumns {
    fn drop(&mut self) {
        if !self.cols.is_null() {
            unsafe { etlg_columns_free(self.cols) };
            self.cols = std::ptr::null_mut();
        }
    }
}

impl GpuDecoder {
    /// The call after `copy_decode_async`, while the batch is still on the device: the sink's Arrow payload for a table whose columns
    /// `arrow_column_kinds` accepts (the call waits for the batch itself). The caller must not ask for a table with an array column
    /// outside the value codec's table (`is_array_type`, crates/etl-postgres/src/type_utils.rs:14-18): only it can tell those.
    pub fn copy_ducklake_arrow(&mut self, schema_slot: u32, f: &CopyInFlight) -> EtlResult<DuckLakeCopyColumns> {
        let mut cols = std::ptr::null_mut();
        let rc = unsafe { etlg_batch_ducklake_copy(self.ctx, f.batch, schema_slot as i32, 0, &mut cols) };
        if rc != ETLG_OK || cols.is_null() {
            return Err(self.last_error());
        }
        let mut view = std::mem::MaybeUninit::<etlg_columns_view>::uninit();
        let mut info = std::mem::MaybeUninit::<etlg_ducklake_copy_info>::uninit();
        unsafe {
            etlg_columns_view_get(cols, view.as_mut_ptr());
            etlg_columns_ducklake_get(cols, info.as_mut_ptr());
            Ok(DuckLakeCopyColumns { cols, view: view.assume_init(), info: info.assume_init() })
        }
    }

    /// The fingerprints of the copy batch's atomic batches (`build_copy_batch_identity`,
    /// crates/etl-destinations/src/ducklake/batches.rs:1449-1464), hashed on the device while the batch is still there
    /// (`etlg_ducklake_fingerprints` over the `ETLG_DL_PREDICATES` / `ETLG_DL_TUPLES` records, which stay in device memory): one per
    /// range of rows, from the range's seed — the `BatchIdHasher` state after `"copy"` and `table_name.id()`, which the caller hashes
    /// itself, as it formats the id (`build_batch_identity`, batches.rs:1536-1553). `col_names`: the slot's replicated column names,
    /// each NUL-terminated, back to back. `info.status == ETLG_RB_NEEDS_HOST` (a record object handed back by the device, or a row without a
    /// record): no fingerprint was written, the host hashes the batch from `info.host_event` on.
    pub fn copy_ducklake_fingerprints(&mut self, schema_slot: u32, f: &CopyInFlight, col_names: &[u8], n_names: u32, ranges: &[etlg_dl_range]) -> EtlResult<(Vec<u64>, etlg_dl_fp_info)> {
        let names = col_names.as_ptr() as *const std::os::raw::c_char;
        let mut recs = [std::ptr::null_mut::<etlg_rowbinary>(); 2];
        for (k, what) in [ETLG_DL_TUPLES, ETLG_DL_PREDICATES].into_iter().enumerate() {
            let rc = unsafe { etlg_batch_duckdb(self.ctx, f.batch, schema_slot as i32, what, names, n_names, ETLG_F_OUTPUT_ON_DEVICE, &mut recs[k]) };
            if rc != ETLG_OK || recs[k].is_null() {
                let e = self.last_error();
                unsafe { etlg_rowbinary_free(recs[0]) };
                return Err(e);
            }
        }
        let mut out = vec![0u64; ranges.len()];
        let mut info = etlg_dl_fp_info { status: ETLG_RB_OK, _pad: 0, host_event: u64::MAX };
        // a record object the device handed back (a DEFERRED cell ...): nothing to hash — the same answer as for a missing record
        for r in recs {
            let mut v = std::mem::MaybeUninit::<etlg_rowbinary_view>::uninit();
            let v = unsafe {
                etlg_rowbinary_view_get(r, v.as_mut_ptr());
                v.assume_init()
            };
            if v.status == ETLG_RB_NEEDS_HOST {
                info.status = ETLG_RB_NEEDS_HOST;
                info.host_event = info.host_event.min(v.host_event);
            }
        }
        if info.status == ETLG_RB_NEEDS_HOST {
            unsafe {
                etlg_rowbinary_free(recs[0]);
                etlg_rowbinary_free(recs[1]);
            }
            return Ok((out, info));
        }
        let rc = unsafe {
            etlg_ducklake_fingerprints(self.ctx, f.batch, schema_slot as i32, recs[0], recs[1], std::ptr::null(), names, n_names, ranges.as_ptr(),
                                       ranges.len() as u32, out.as_mut_ptr(), &mut info)
        };
        let status = if rc == ETLG_OK { Ok(()) } else { Err(self.last_error()) };
        unsafe {
            etlg_rowbinary_free(recs[0]);
            etlg_rowbinary_free(recs[1]);
        }
        status.map(|_| (out, info))
    }
}

/// A table-copy batch in flight. Dropping it without `copy_finish` frees the batch FIRST (the library waits for its kernels and its
/// upload: `etlg_batch_free` finishes a pending batch) and only then the pinned staging — the order `InFlight` keeps for WAL batches
/// (lib.rs; both exercised by tests/native/shim_twin.cpp).
pub struct CopyInFlight {
    ctx: *mut etlg_ctx,
    batch: *mut etlg_batch,
    staged: Option<CopyStaging>,
}

impl Drop for CopyInFlight {
    fn drop(&mut self) {
        let _ = self.ctx;
        if !self.batch.is_null() {
            unsafe { etlg_batch_free(self.batch) };
            self.batch = std::ptr::null_mut();
        }
        self.staged.take();
    }
}
