//! Raw binding of `include/etlg.h` (ABI version 1). One `extern "C"` item per exported symbol, one `#[repr(C)]` struct per
//! C struct, same field order and types; `tests/test_rust_shim.py` in the etl-gfx950 repository parses this file and the
//! header and fails when they drift apart.
#![allow(non_camel_case_types, dead_code)]

use std::os::raw::{c_char, c_void};

pub const ETLG_ABI_VERSION: u32 = 1;

#[repr(C)]
pub struct etlg_ctx {
    _private: [u8; 0],
}
#[repr(C)]
pub struct etlg_batch {
    _private: [u8; 0],
}

// ---- errors (etlg_error_kind / etlg_err_code)
pub const ETLG_OK: i32 = 0;
pub const ETLG_ConversionError: i32 = 1;
pub const ETLG_InvalidData: i32 = 2;
pub const ETLG_ValidationError: i32 = 3;
pub const ETLG_InvalidState: i32 = 4;
pub const ETLG_MissingTableSchema: i32 = 5;
pub const ETLG_CorruptedTableSchema: i32 = 6;
pub const ETLG_DeserializationError: i32 = 7;
pub const ETLG_SourceConnectionFailed: i32 = 8;
pub const ETLG_IoError: i32 = 9;
pub const ETLG_UnsupportedValueInDestination: i32 = 10;
pub const ETLG_NullValuesNotSupportedInArrayInDestination: i32 = 11;
pub const ETLG_InvalidArgument: i32 = 100;
pub const ETLG_DeviceError: i32 = 101;
pub const ETLG_Unsupported: i32 = 102;

#[repr(C)]
pub struct etlg_error {
    pub kind: i32,
    pub code: i32,
    pub description: *const c_char,
    pub detail: *const c_char,
    pub frame_index: i64,
}

#[repr(C)]
pub struct etlg_err_desc {
    pub kind: i32,
    pub description: *const c_char,
}

// ---- schemas
pub const ETLG_TC_STRING: u8 = 0;
pub const ETLG_TC_BOOL: u8 = 1;
pub const ETLG_TC_I16: u8 = 2;
pub const ETLG_TC_I32: u8 = 3;
pub const ETLG_TC_I64: u8 = 4;
pub const ETLG_TC_U32: u8 = 5;
pub const ETLG_TC_F32: u8 = 6;
pub const ETLG_TC_F64: u8 = 7;
pub const ETLG_TC_NUMERIC: u8 = 8;
pub const ETLG_TC_BYTEA: u8 = 9;
pub const ETLG_TC_DATE: u8 = 10;
pub const ETLG_TC_TIME: u8 = 11;
pub const ETLG_TC_TIMETZ: u8 = 12;
pub const ETLG_TC_TIMESTAMP: u8 = 13;
pub const ETLG_TC_TIMESTAMPTZ: u8 = 14;
pub const ETLG_TC_UUID: u8 = 15;
pub const ETLG_TC_JSON: u8 = 16;
pub const ETLG_TC_ARRAY: u8 = 17;

#[repr(C)]
pub struct etlg_col {
    pub name: *const c_char,
    pub type_oid: u32,
    pub type_modifier: i32,
    pub attnum: i32,
    pub nullable: u8,
    pub primary_key: u8,
    pub _pad: [u8; 2],
}

pub const ETLG_TS_ABSENT: i32 = 0;
pub const ETLG_TS_READY: i32 = 1;
pub const ETLG_TS_SYNC_DONE: i32 = 2;
pub const ETLG_TS_OTHER: i32 = 3;
pub const ETLG_WORKER_APPLY: i32 = 0;
pub const ETLG_WORKER_TABLE_SYNC: i32 = 1;

// ---- decode flags
pub const ETLG_F_INPUT_ON_DEVICE: u32 = 1 << 0;
pub const ETLG_F_OUTPUT_ON_DEVICE: u32 = 1 << 1;
pub const ETLG_F_NO_CONTROL: u32 = 1 << 2;
pub const ETLG_F_ASYNC: u32 = 1 << 3;
pub const ETLG_F_FINISH_CELLS: u32 = 1 << 4;
pub const ETLG_F_CHECK_CELLS: u32 = 1 << 5;
pub const ETLG_FINISH_ARRAYS: u32 = 1;
pub const ETLG_FINISH_FLOATS: u32 = 2;

// ---- batch (arena)
pub const ETLG_EV_BEGIN: u8 = b'B';
pub const ETLG_EV_COMMIT: u8 = b'C';
pub const ETLG_EV_RELATION: u8 = b'R';
pub const ETLG_EV_INSERT: u8 = b'I';
pub const ETLG_EV_UPDATE: u8 = b'U';
pub const ETLG_EV_DELETE: u8 = b'D';
pub const ETLG_EV_TRUNCATE: u8 = b'T';
pub const ETLG_OLD_NONE: u8 = 0;
pub const ETLG_OLD_FULL: u8 = 1;
pub const ETLG_OLD_KEY: u8 = 2;
pub const ETLG_FLAG_PARTIAL: u8 = 4;
pub const ETLG_CELL_VALUE: u8 = 0;
pub const ETLG_CELL_NULL: u8 = 1;
pub const ETLG_CELL_MISSING: u8 = 2;
pub const ETLG_CELL_DEFERRED: u8 = 3;
pub const ETLG_NUM_VALUE: u8 = 0;
pub const ETLG_NUM_NAN: u8 = 1;
pub const ETLG_NUM_PINF: u8 = 2;
pub const ETLG_NUM_NINF: u8 = 3;

#[repr(C)]
pub struct etlg_numeric_hdr {
    pub kind: u8,
    pub sign: u8,
    pub weight: i16,
    pub scale: u16,
    pub ndigits: u16,
}

#[repr(C)]
pub struct etlg_slot_col {
    pub type_oid: u32,
    pub stored_index: u16,
    pub type_class: u8,
    pub nullable: u8,
    pub identity: u8,
    pub _pad: u8,
    pub off_full: u16,
    pub off_key: u16,
    pub key_index: u16,
}

#[repr(C)]
pub struct etlg_slot_desc {
    pub table_id: u32,
    pub n_stored: u32,
    pub snapshot_lsn: u64,
    pub n_cols: u32,
    pub n_ident: u32,
    pub row_bytes_full: u32,
    pub row_bytes_key: u32,
    pub state_bytes_full: u32,
    pub state_bytes_key: u32,
    pub cols: *const etlg_slot_col,
}

#[repr(C)]
pub struct etlg_batch_view {
    pub n_events: u64,
    pub n_frames: u64,
    pub fixed_bytes: u64,
    pub heap_bytes: u64,
    pub payload_bytes: [u64; 3],
    pub ev_kind: *const u8,
    pub ev_flags: *const u8,
    pub ev_table_id: *const u32,
    pub ev_schema_slot: *const u32,
    pub ev_start_lsn: *const u64,
    pub ev_commit_lsn: *const u64,
    pub ev_tx_ordinal: *const u64,
    pub ev_body_off: *const u64,
    pub fixed: *const u8,
    pub heap: *const u8,
    pub on_device: u32,
    pub n_slots: u32,
    pub slots: *const etlg_slot_desc,
}

#[repr(C)]
pub struct etlg_column {
    pub type_class: u32,
    pub arrow_kind: u32,
    pub value_bytes: u32,
    pub nullable: u32,
    pub null_count: u64,
    pub deferred_count: u64,
    pub validity: *const u8,
    pub deferred: *const u8,
    pub values: *const u8,
    pub offsets: *const i64,
    pub values_bytes: u64,
    pub child_kind: u32,
    pub _pad: u32,
    pub child_count: u64,
    pub child_null_count: u64,
    pub child_validity: *const u8,
    pub child_offsets: *const i64,
}

#[repr(C)]
pub struct etlg_columns_view {
    pub n_rows: u64,
    pub n_cols: u32,
    pub on_device: u32,
    pub cols: *const etlg_column,
    pub row_event: *const u64,
}

#[repr(C)]
pub struct etlg_rowbinary_view {
    pub n_rows: u64,
    pub n_bytes: u64,
    pub n_host_rows: u64,
    pub status: u32,
    pub on_device: u32,
    pub host_event: u64,
    pub host_column: u32,
    pub _pad: u32,
    pub bytes: *const u8,
    pub row_offsets: *const i64,
    pub row_event: *const u64,
}

#[repr(C)]
pub struct etlg_size_model {
    pub begin_event: u32,
    pub commit_event: u32,
    pub insert_event: u32,
    pub update_event: u32,
    pub delete_event: u32,
    pub truncate_event: u32,
    pub relation_event: u32,
    pub replicated_table_schema: u32,
    pub table_row: u32,
    pub cell: u32,
    pub _reserved: [u32; 2],
}

pub const ETLG_SIZE_HINT_INCOMPLETE: u64 = 1 << 63;

/// A typed array in the heap (include/etlg.h: the finish pass).
#[repr(C)]
pub struct etlg_array_hdr {
    pub n_elems: u32,
    pub elem_class: u8,
    pub elem_bytes: u8,
    pub reserved: u16,
}

#[repr(C)]
pub struct etlg_changelog_info {
    pub n_host_rows: u64,
    pub host_event: u64,
    pub host_reason: u32,
    pub n_data_cols: u32,
}

#[repr(C)]
pub struct etlg_ducklake_copy_info {
    pub status: u32,
    pub column: u32,
    pub _pad: [u32; 2],
}

#[repr(C)]
pub struct etlg_dl_range {
    pub first_event: u64,
    pub end_event: u64,
    pub seed: u64,
}

#[repr(C)]
pub struct etlg_dl_fp_info {
    pub status: u32,
    pub _pad: u32,
    pub host_event: u64,
}

#[repr(C)]
pub struct etlg_cuts_info {
    pub n_cuts: u64,
    pub stop_event: u64,
    pub carry_out: u64,
    pub total: u64,
}

#[repr(C)]
pub struct etlg_payload_sums {
    pub bytes: [u64; 4],
    pub rows: [u64; 4],
}

#[repr(C)]
pub struct etlg_payload_info {
    pub received_bytes: [u64; 4],
    pub received_rows: [u64; 4],
    pub n_ranges: u64,
    pub status: i32,
    pub _pad: u32,
    pub mismatch_event: u64,
}

#[derive(Clone, Copy)]
#[repr(C)]
pub struct etlg_outline_pass {
    pub first_event: u64,
    pub data_end: u64,
    pub rel_end: u64,
    pub end_event: u64,
    pub range: u64,
    pub trunc_first: u64,
    pub n_trunc: u64,
}

#[derive(Clone, Copy)]
#[repr(C)]
pub struct etlg_outline_trunc {
    pub table_id: u32,
    pub schema_slot: u32,
    pub event: u64,
}

#[derive(Clone, Copy)]
#[repr(C)]
pub struct etlg_outline_slot {
    pub rows: [u64; 6],
    pub first: [u64; 6],
}

#[derive(Clone, Copy)]
#[repr(C)]
pub struct etlg_outline_info {
    pub n_passes: u64,
    pub n_trunc: u64,
    pub n_relations: u64,
    pub n_rows: u64,
    pub n_ranges: u64,
    pub bad_cut: u64,
    pub status: u32,
    pub _pad: u32,
}

#[derive(Clone, Copy)]
#[repr(C)]
pub struct etlg_dl_batch {
    pub first_event: u64,
    pub end_event: u64,
    pub first_start_lsn: u64,
    pub last_commit_lsn: u64,
    pub first_commit_lsn: u64,
    pub first_tx_ordinal: u64,
    pub last_tx_ordinal: u64,
    pub window: u64,
    pub op_first: u64,
    pub n_members: u32,
    pub n_ops: u32,
    pub n_cat: [u32; 5],
    pub _pad: u32,
}

#[derive(Clone, Copy)]
#[repr(C)]
pub struct etlg_dl_op {
    pub kind: u32,
    pub origin: u32,
    pub first_event: u64,
    pub n: u64,
    pub rec_first: u64,
}

#[derive(Clone, Copy)]
#[repr(C)]
pub struct etlg_dl_plan_info {
    pub n_batches: u64,
    pub n_ops: u64,
    pub n_members: u64,
    pub n_retained: u64,
    pub n_dropped: u64,
    pub event: u64,
    pub bad_pass: u64,
    pub status: u32,
    pub reason: u32,
}

#[derive(Clone, Copy)]
#[repr(C)]
pub struct etlg_sf_segment {
    pub window: u64,
    pub first_row: u64,
    pub end_row: u64,
    pub first_event: u64,
    pub last_event: u64,
    pub byte_first: u64,
    pub byte_end: u64,
    pub first_row_bytes: u64,
    pub first_commit_lsn: u64,
    pub first_tx_ordinal: u64,
    pub last_commit_lsn: u64,
    pub last_tx_ordinal: u64,
    pub flush_before: u32,
    pub _pad: u32,
}

#[derive(Clone, Copy)]
#[repr(C)]
pub struct etlg_sf_window {
    pub seg_first: u64,
    pub n_segs: u64,
    pub first_row: u64,
    pub end_row: u64,
    pub n_members: u64,
    pub n_retained: u64,
    pub n_bytes: u64,
}

#[derive(Clone, Copy)]
#[repr(C)]
pub struct etlg_sf_plan_info {
    pub n_segs: u64,
    pub n_members: u64,
    pub n_retained: u64,
    pub n_dropped: u64,
    pub n_rows: u64,
    pub n_bytes: u64,
    pub event: u64,
    pub row_bytes: u64,
    pub bad_pass: u64,
    pub status: u32,
    pub reason: u32,
}

#[derive(Clone, Copy)]
#[repr(C)]
pub struct etlg_ch_statement {
    pub window: u64,
    pub first_row: u64,
    pub end_row: u64,
    pub first_event: u64,
    pub last_event: u64,
    pub byte_first: u64,
    pub byte_end: u64,
}

#[derive(Clone, Copy)]
#[repr(C)]
pub struct etlg_ch_window {
    pub stmt_first: u64,
    pub n_stmts: u64,
    pub first_row: u64,
    pub end_row: u64,
    pub n_members: u64,
    pub n_bytes: u64,
}

#[derive(Clone, Copy)]
#[repr(C)]
pub struct etlg_ch_plan_info {
    pub n_stmts: u64,
    pub n_members: u64,
    pub n_rows: u64,
    pub n_bytes: u64,
    pub event: u64,
    pub bad_pass: u64,
    pub fail_pass: u64,
    pub status: u32,
    pub reason: u32,
}

#[derive(Clone, Copy)]
#[repr(C)]
pub struct etlg_bq_request {
    pub window: u64,
    pub first_row: u64,
    pub end_row: u64,
    pub first_event: u64,
    pub last_event: u64,
    pub byte_first: u64,
    pub byte_end: u64,
    pub n_members: u64,
}

#[derive(Clone, Copy)]
#[repr(C)]
pub struct etlg_bq_window {
    pub req_first: u64,
    pub n_reqs: u64,
    pub first_row: u64,
    pub end_row: u64,
    pub n_members: u64,
    pub n_two_row: u64,
    pub n_bytes: u64,
}

#[derive(Clone, Copy)]
#[repr(C)]
pub struct etlg_bq_plan_info {
    pub n_reqs: u64,
    pub n_members: u64,
    pub n_rows: u64,
    pub n_two_row: u64,
    pub n_bytes: u64,
    pub est_row_bytes: u64,
    pub target_batches: u64,
    pub event: u64,
    pub bad_pass: u64,
    pub fail_pass: u64,
    pub status: u32,
    pub reason: u32,
}

#[derive(Clone, Copy)]
#[repr(C)]
pub struct etlg_ice_write {
    pub window: u64,
    pub first_row: u64,
    pub end_row: u64,
    pub first_event: u64,
    pub last_event: u64,
    pub n_members: u64,
    pub other_slot_event: u64,
}

#[derive(Clone, Copy)]
#[repr(C)]
pub struct etlg_ice_window {
    pub write_first: u64,
    pub n_writes: u64,
    pub first_row: u64,
    pub end_row: u64,
    pub n_members: u64,
    pub other_slot_event: u64,
}

#[derive(Clone, Copy)]
#[repr(C)]
pub struct etlg_ice_slice {
    pub null_count: u64,
    pub deferred_count: u64,
    pub byte_first: u64,
    pub byte_end: u64,
    pub child_first: u64,
    pub child_end: u64,
    pub child_null_count: u64,
}

#[derive(Clone, Copy)]
#[repr(C)]
pub struct etlg_ice_plan_info {
    pub n_writes: u64,
    pub n_members: u64,
    pub n_rows: u64,
    pub n_mixed: u64,
    pub event: u64,
    pub bad_pass: u64,
    pub fail_pass: u64,
    pub status: u32,
    pub reason: u32,
}

#[repr(C)]
pub struct etlg_finish_stats {
    pub deferred_seen: u64,
    pub arrays_typed: u64,
    pub floats_settled: u64,
    pub left_deferred: u64,
    pub heap_bytes_added: u64,
}

#[repr(C)]
pub struct etlg_columns {
    _private: [u8; 0],
}

#[repr(C)]
pub struct etlg_rowbinary {
    _private: [u8; 0],
}

pub const ETLG_ROWS_INSERT: u32 = 1;
pub const ETLG_ROWS_UPDATE: u32 = 2;
pub const ETLG_ROWS_PARSE_ARRAYS: u32 = 4;
pub const ETLG_ROWS_FORMAT_JSON: u32 = 8;
pub const ETLG_ICE_PARTIAL_UPDATE: u32 = 1;
pub const ETLG_ICE_KEY_ONLY_DELETE: u32 = 2;
pub const ETLG_ICE_DELETE_WITHOUT_OLD_ROW: u32 = 3;
pub const ETLG_DLC_OK: u32 = 0;
pub const ETLG_DLC_NOT_ARROW: u32 = 1;
pub const ETLG_DLC_OFFSETS_OVERFLOW: u32 = 2;
pub const ETLG_AK_INT16: u32 = 14;
pub const ETLG_AK_UINT64: u32 = 15;
pub const ETLG_AK_UTF8: u32 = 16;
pub const ETLG_AK_BINARY: u32 = 17;
pub const ETLG_CH_MERGE_TREE: i32 = 0;
pub const ETLG_CH_REPLACING_MERGE_TREE: i32 = 1;
pub const ETLG_RB_OK: u32 = 0;
pub const ETLG_RB_NEEDS_HOST: u32 = 3;
pub const ETLG_PK_INSERT: u32 = 0;
pub const ETLG_PK_UPDATE: u32 = 1;
pub const ETLG_PK_DELETE: u32 = 2;
pub const ETLG_PK_COPY: u32 = 3;
pub const ETLG_PM_OK: u32 = 0;
pub const ETLG_PM_MISMATCH: u32 = 1;
pub const ETLG_OL_RELATIONS_INLINE: u32 = 1;
pub const ETLG_OL_OK: u32 = 0;
pub const ETLG_OL_BAD_CUTS: u32 = 1;
pub const ETLG_DLP_OK: u32 = 0;
pub const ETLG_DLP_BAD_PASSES: u32 = 1;
pub const ETLG_DLP_REFUSED: u32 = 2;
pub const ETLG_DLP_NOT_PREFIX: u32 = 3;
pub const ETLG_DLP_NEEDS_HOST: u32 = 4;
pub const ETLG_DLP_R_UPDATE_IDENTITY: u32 = 1;
pub const ETLG_DLP_R_DELETE_IDENTITY: u32 = 2;
pub const ETLG_DLP_R_DELETE_NO_OLD: u32 = 3;
pub const ETLG_DLP_CAT_INSERT: u32 = 0;
pub const ETLG_DLP_CAT_UPDATE_FULL: u32 = 1;
pub const ETLG_DLP_CAT_REPLACE: u32 = 2;
pub const ETLG_DLP_CAT_UPDATE_PARTIAL: u32 = 3;
pub const ETLG_DLP_CAT_DELETE: u32 = 4;
pub const ETLG_DLP_OP_UPSERT: u32 = 0;
pub const ETLG_DLP_OP_DELETE: u32 = 1;
pub const ETLG_DLP_OP_UPDATE: u32 = 2;
pub const ETLG_DLP_ORIGIN_NONE: u32 = 0;
pub const ETLG_DLP_ORIGIN_DELETE: u32 = 1;
pub const ETLG_DLP_ORIGIN_UPDATE: u32 = 2;
pub const ETLG_DLP_ORIGIN_REPLACE: u32 = 3;
pub const ETLG_SF_MAX_UNFLUSHED_BYTES: u64 = 131072;
pub const ETLG_SF_MAX_ROW_BYTES: u64 = 2097152;
pub const ETLG_SFP_OK: u32 = 0;
pub const ETLG_SFP_BAD_PASSES: u32 = 1;
pub const ETLG_SFP_FAILED: u32 = 2;
pub const ETLG_SFP_NOT_PREFIX: u32 = 3;
pub const ETLG_SFP_NEEDS_HOST: u32 = 4;
pub const ETLG_SFP_R_PARTIAL_UPDATE: u32 = 1;
pub const ETLG_SFP_R_DELETE_NO_OLD: u32 = 2;
pub const ETLG_SFP_R_ROW_TOO_LARGE: u32 = 3;
pub const ETLG_CH_MAX_BYTES_PER_INSERT: u64 = 67108864;
pub const ETLG_CHP_OK: u32 = 0;
pub const ETLG_CHP_BAD_PASSES: u32 = 1;
pub const ETLG_CHP_FAILED: u32 = 2;
pub const ETLG_CHP_NEEDS_HOST: u32 = 3;
pub const ETLG_CHP_R_PARTIAL_UPDATE: u32 = 1;
pub const ETLG_CHP_R_UPDATE_IDENTITY: u32 = 2;
pub const ETLG_CHP_R_DELETE_NO_OLD: u32 = 3;
pub const ETLG_CHP_R_KEY_WIDTH: u32 = 4;
pub const ETLG_CHP_R_KEY_IDENTITY: u32 = 5;
pub const ETLG_BQP_OK: u32 = 0;
pub const ETLG_BQP_BAD_PASSES: u32 = 1;
pub const ETLG_BQP_FAILED: u32 = 2;
pub const ETLG_BQP_NEEDS_HOST: u32 = 3;
pub const ETLG_BQP_R_PARTIAL_UPDATE: u32 = 1;
pub const ETLG_BQP_R_UPDATE_NO_OLD_IDENTITY: u32 = 2;
pub const ETLG_BQP_R_KEY_WIDTH: u32 = 3;
pub const ETLG_BQP_R_KEY_IDENTITY: u32 = 4;
pub const ETLG_BQP_R_DELETE_NO_OLD: u32 = 5;
pub const ETLG_ICP_OK: u32 = 0;
pub const ETLG_ICP_BAD_PASSES: u32 = 1;
pub const ETLG_ICP_FAILED: u32 = 2;
pub const ETLG_ICP_NEEDS_HOST: u32 = 3;
pub const ETLG_DL_TUPLES: i32 = 0;
pub const ETLG_DL_PREDICATES: i32 = 1;
pub const ETLG_DL_UPDATES: i32 = 3;

#[repr(C)]
pub struct etlg_kernel_stat {
    pub name: *const c_char,
    pub launches: u64,
    pub total_ms: f64,
}

extern "C" {
    pub fn etlg_err_table(code: i32) -> *const etlg_err_desc;
    pub fn etlg_type_class_of_oid(type_oid: u32) -> i32;
    pub fn etlg_array_elem_class(array_type_oid: u32) -> i32;
    pub fn etlg_slot_bytes(type_class: i32) -> u32;

    pub fn etlg_abi_version() -> u32;
    pub fn etlg_ctx_create(hip_device: i32, out: *mut *mut etlg_ctx) -> i32;
    pub fn etlg_create_error() -> *const c_char;
    pub fn etlg_ctx_destroy(ctx: *mut etlg_ctx);
    pub fn etlg_ctx_set_stream(ctx: *mut etlg_ctx, hip_stream: *mut c_void) -> i32;
    pub fn etlg_ctx_set_worker(ctx: *mut etlg_ctx, worker_kind: i32, table_sync_table_id: u32, bootstrap_snapshot_lsn: u64) -> i32;
    pub fn etlg_schema_put(
        ctx: *mut etlg_ctx,
        table_id: u32,
        snapshot_lsn: u64,
        schema_name: *const c_char,
        table_name: *const c_char,
        ncols: u32,
        cols: *const etlg_col,
    ) -> i32;
    pub fn etlg_table_state(ctx: *mut etlg_ctx, table_id: u32, state_kind: i32, lsn: u64) -> i32;
    pub fn etlg_table_ready(
        ctx: *mut etlg_ctx,
        table_id: u32,
        snapshot_lsn: u64,
        replication_mask: *const u8,
        identity_mask: *const u8,
        nmask: u32,
    ) -> i32;
    pub fn etlg_table_forget(ctx: *mut etlg_ctx, table_id: u32) -> i32;
    pub fn etlg_table_cache_get(ctx: *const etlg_ctx, table_id: u32, kind: *mut i32, snapshot_lsn: *mut u64, schema_slot: *mut i32) -> i32;
    pub fn etlg_ctx_reset_stream_state(ctx: *mut etlg_ctx) -> i32;

    pub fn etlg_decode(
        ctx: *mut etlg_ctx,
        buf: *const u8,
        len: usize,
        frame_offsets: *const u32,
        nframes: usize,
        flags: u32,
        out: *mut *mut etlg_batch,
    ) -> i32;
    pub fn etlg_last_error(ctx: *const etlg_ctx) -> *const etlg_error;
    pub fn etlg_copy_decode(
        ctx: *mut etlg_ctx,
        schema_slot: i32,
        buf: *const u8,
        len: usize,
        row_offsets: *const u32,
        nrows: usize,
        flags: u32,
        out: *mut *mut etlg_batch,
    ) -> i32;
    pub fn etlg_scan_boundaries(
        ctx: *mut etlg_ctx,
        buf: *const u8,
        len: usize,
        flags: u32,
        offsets_out: *mut u32,
        cap: usize,
        nframes_out: *mut usize,
    ) -> i32;
    pub fn etlg_frame_tags(
        ctx: *mut etlg_ctx,
        buf: *const u8,
        len: usize,
        frame_offsets: *const u32,
        nframes: usize,
        flags: u32,
        tags_out: *mut u8,
    ) -> i32;

    pub fn etlg_control_stream(
        ctx: *mut etlg_ctx,
        buf: *const u8,
        len: usize,
        frame_offsets: *const u32,
        nframes: usize,
        flags: u32,
        out_bytes: *mut u8,
        out_cap: usize,
        out_offsets: *mut u32,
        out_offsets_cap: usize,
        n_bytes: *mut usize,
        n_frames: *mut usize,
        last_tag: *mut u32,
    ) -> i32;
    pub fn etlg_shard_plan(
        ctx: *mut etlg_ctx,
        buf: *const u8,
        len: usize,
        frame_offsets: *const u32,
        nframes: usize,
        n_shards: u32,
        flags: u32,
        cuts_out: *mut u64,
    ) -> i32;
    pub fn etlg_shard_replay(ctx: *mut etlg_ctx, buf: *const u8, len: usize, frame_offsets: *const u32, nframes: usize) -> i32;
    pub fn etlg_host_alloc(ctx: *mut etlg_ctx, bytes: usize, out: *mut *mut c_void) -> i32;
    pub fn etlg_host_free(p: *mut c_void);
    pub fn etlg_batch_view_get(batch: *const etlg_batch, out: *mut etlg_batch_view) -> i32;
    pub fn etlg_batch_sync(ctx: *mut etlg_ctx, batch: *mut etlg_batch) -> i32;
    pub fn etlg_batch_header_to_device(ctx: *mut etlg_ctx, batch: *mut etlg_batch, dst_device_8xu64: *mut c_void) -> i32;
    pub fn etlg_ctx_fence(ctx: *mut etlg_ctx) -> i32;
    pub fn etlg_batch_download(ctx: *mut etlg_ctx, batch: *mut etlg_batch) -> i32;
    pub fn etlg_batch_free(batch: *mut etlg_batch);
    pub fn etlg_batch_columns(ctx: *mut etlg_ctx, batch: *mut etlg_batch, schema_slot: i32, row_kinds: u32, flags: u32, out: *mut *mut etlg_columns) -> i32;
    pub fn etlg_columns_view_get(cols: *const etlg_columns, out: *mut etlg_columns_view) -> i32;
    pub fn etlg_columns_free(cols: *mut etlg_columns);
    pub fn etlg_batch_iceberg(ctx: *mut etlg_ctx, batch: *mut etlg_batch, schema_slot: i32, opts: u32, flags: u32, out: *mut *mut etlg_columns) -> i32;
    pub fn etlg_columns_changelog_get(cols: *const etlg_columns, out: *mut etlg_changelog_info) -> i32;
    pub fn etlg_batch_ducklake_copy(ctx: *mut etlg_ctx, batch: *mut etlg_batch, schema_slot: i32, flags: u32, out: *mut *mut etlg_columns) -> i32;
    pub fn etlg_columns_ducklake_get(cols: *const etlg_columns, out: *mut etlg_ducklake_copy_info) -> i32;
    pub fn etlg_batch_rowbinary(
        ctx: *mut etlg_ctx,
        batch: *mut etlg_batch,
        schema_slot: i32,
        nullable_flags: *const u8,
        n_flags: u32,
        engine: i32,
        flags: u32,
        out: *mut *mut etlg_rowbinary,
    ) -> i32;
    pub fn etlg_batch_protobuf(ctx: *mut etlg_ctx, batch: *mut etlg_batch, schema_slot: i32, flags: u32, out: *mut *mut etlg_rowbinary) -> i32;
    pub fn etlg_batch_ndjson(
        ctx: *mut etlg_ctx,
        batch: *mut etlg_batch,
        schema_slot: i32,
        col_names: *const c_char,
        n_names: u32,
        flags: u32,
        out: *mut *mut etlg_rowbinary,
    ) -> i32;
    pub fn etlg_batch_duckdb(
        ctx: *mut etlg_ctx,
        batch: *mut etlg_batch,
        schema_slot: i32,
        what: i32,
        col_names: *const c_char,
        n_names: u32,
        flags: u32,
        out: *mut *mut etlg_rowbinary,
    ) -> i32;
    pub fn etlg_rowbinary_view_get(rb: *const etlg_rowbinary, out: *mut etlg_rowbinary_view) -> i32;
    pub fn etlg_rowbinary_col_ends_get(rb: *const etlg_rowbinary, col_ends: *mut *const u32) -> i32;
    pub fn etlg_rowbinary_free(rb: *mut etlg_rowbinary);
    pub fn etlg_ducklake_fingerprints(
        ctx: *mut etlg_ctx,
        batch: *mut etlg_batch,
        schema_slot: i32,
        tuples: *const etlg_rowbinary,
        predicates: *const etlg_rowbinary,
        updates: *const etlg_rowbinary,
        col_names: *const c_char,
        n_names: u32,
        ranges: *const etlg_dl_range,
        n_ranges: u32,
        out: *mut u64,
        info: *mut etlg_dl_fp_info,
    ) -> i32;
    pub fn etlg_batch_size_hints(ctx: *mut etlg_ctx, batch: *mut etlg_batch, model: *const etlg_size_model, flags: u32, out: *mut u64) -> i32;
    pub fn etlg_batch_cuts(
        ctx: *mut etlg_ctx,
        batch: *mut etlg_batch,
        model: *const etlg_size_model,
        hints: *const u64,
        first: u64,
        end: u64,
        budget: u64,
        carry_in: u64,
        flags: u32,
        cuts_out: *mut u64,
        cuts_cap: u64,
        info: *mut etlg_cuts_info,
    ) -> i32;
    pub fn etlg_cuts_locate(ctx: *mut etlg_ctx, cuts: *const u64, n_cuts: u64, cuts_on_device: u32, row_event: *const u64, n_rows: u64, flags: u32, rows_out: *mut u64) -> i32;
    pub fn etlg_batch_payload(
        ctx: *mut etlg_ctx,
        batch: *mut etlg_batch,
        buf: *const u8,
        len: usize,
        frame_offsets: *const u32,
        nframes: usize,
        cuts: *const u64,
        n_cuts: u64,
        cuts_on_device: u32,
        hist_bounds: *const u64,
        n_bounds: u32,
        flags: u32,
        ev_bytes_out: *mut u32,
        sums_out: *mut etlg_payload_sums,
        hist_out: *mut u64,
        info: *mut etlg_payload_info,
    ) -> i32;
    pub fn etlg_batch_outline(
        ctx: *mut etlg_ctx,
        batch: *mut etlg_batch,
        first: u64,
        end: u64,
        cuts: *const u64,
        n_cuts: u64,
        cuts_on_device: u32,
        opts: u32,
        flags: u32,
        passes_out: *mut etlg_outline_pass,
        ends_out: *mut u64,
        touched_out: *mut u64,
        passes_cap: u64,
        trunc_out: *mut etlg_outline_trunc,
        trunc_cap: u64,
        slots_out: *mut etlg_outline_slot,
        info: *mut etlg_outline_info,
    ) -> i32;
    pub fn etlg_ducklake_plan(
        ctx: *mut etlg_ctx,
        batch: *mut etlg_batch,
        schema_slot: i32,
        passes: *const etlg_outline_pass,
        n_passes: u64,
        passes_on_device: u32,
        has_watermark: u32,
        wm_commit_lsn: u64,
        wm_tx_ordinal: u64,
        seed: u64,
        tuples: *const etlg_rowbinary,
        predicates: *const etlg_rowbinary,
        updates: *const etlg_rowbinary,
        flags: u32,
        ranges_out: *mut etlg_dl_range,
        batches_out: *mut etlg_dl_batch,
        batches_cap: u64,
        ops_out: *mut etlg_dl_op,
        ops_cap: u64,
        info: *mut etlg_dl_plan_info,
    ) -> i32;
    pub fn etlg_snowflake_plan(
        ctx: *mut etlg_ctx,
        batch: *mut etlg_batch,
        schema_slot: i32,
        passes: *const etlg_outline_pass,
        n_passes: u64,
        passes_on_device: u32,
        has_committed: u32,
        c_commit_lsn: u64,
        c_tx_ordinal: u64,
        ndjson: *const etlg_rowbinary,
        flush_bytes: u64,
        max_row_bytes: u64,
        flags: u32,
        segs_out: *mut etlg_sf_segment,
        segs_cap: u64,
        windows_out: *mut etlg_sf_window,
        info: *mut etlg_sf_plan_info,
    ) -> i32;
    pub fn etlg_clickhouse_plan(
        ctx: *mut etlg_ctx,
        batch: *mut etlg_batch,
        schema_slot: i32,
        passes: *const etlg_outline_pass,
        n_passes: u64,
        passes_on_device: u32,
        rowbinary: *const etlg_rowbinary,
        max_bytes_per_insert: u64,
        flags: u32,
        stmts_out: *mut etlg_ch_statement,
        stmts_cap: u64,
        windows_out: *mut etlg_ch_window,
        info: *mut etlg_ch_plan_info,
    ) -> i32;
    pub fn etlg_bigquery_plan(
        ctx: *mut etlg_ctx,
        batch: *mut etlg_batch,
        schema_slot: i32,
        passes: *const etlg_outline_pass,
        n_passes: u64,
        passes_on_device: u32,
        protobuf: *const etlg_rowbinary,
        max_batch_bytes: u64,
        flags: u32,
        reqs_out: *mut etlg_bq_request,
        reqs_cap: u64,
        windows_out: *mut etlg_bq_window,
        info: *mut etlg_bq_plan_info,
    ) -> i32;
    pub fn etlg_iceberg_plan(
        ctx: *mut etlg_ctx,
        batch: *mut etlg_batch,
        schema_slot: i32,
        passes: *const etlg_outline_pass,
        n_passes: u64,
        passes_on_device: u32,
        changelog: *const etlg_columns,
        flags: u32,
        writes_out: *mut etlg_ice_write,
        writes_cap: u64,
        slices_out: *mut etlg_ice_slice,
        windows_out: *mut etlg_ice_window,
        info: *mut etlg_ice_plan_info,
    ) -> i32;
    pub fn etlg_batch_finish_cells(ctx: *mut etlg_ctx, batch: *mut etlg_batch, what: u32, stats: *mut etlg_finish_stats) -> i32;
    pub fn etlg_ctx_slots(ctx: *const etlg_ctx, n_slots: *mut u32, slots: *mut *const etlg_slot_desc) -> i32;

    pub fn etlg_ctx_profile(ctx: *mut etlg_ctx, enable: i32) -> i32;
    pub fn etlg_ctx_profile_read(ctx: *mut etlg_ctx, out: *mut etlg_kernel_stat, cap: u32, n: *mut u32) -> i32;
}
