/*
 * etlg.h — C ABI of libetl_gfx950.so, the MI355X-native batched pgoutput decode
 * + CDC event-transform stage that drops in upstream of supabase/etl's
 * Destination::write_events.
 *
 * The reference has no FFI for this path (it is 100 % Rust, monomorphised
 * generics).  Each entry point below names the reference code it replaces
 * (paths relative to the supabase/etl checkout):
 *
 *   etlg_ctx_create / _destroy   one per apply-loop stream; owns what
 *                                ApplyLoop keeps in `self.state` + the
 *                                SharedTableCache
 *                                (crates/etl/src/replication/apply.rs:942-963,
 *                                 crates/etl/src/replication/table_cache.rs:88-154)
 *   etlg_ctx_set_worker          WorkerContext::{Apply,TableSync} ownership rule
 *                                (apply.rs:2626-2639, 2836-2867, 3514-3519) and the
 *                                bootstrap snapshot id (apply.rs:2410-2413)
 *   etlg_schema_put              SchemaStore::store_table_schema /
 *                                get_table_schema at-or-before lookup
 *                                (crates/etl/src/store/schema/base.rs:19-69,
 *                                 crates/etl/src/store/schema/table.rs:61-71)
 *   etlg_table_state             StateStore::get_table_state for the
 *                                should_apply_changes filter (apply.rs:2836-2867)
 *   etlg_table_ready             SharedTableCache::note_ready as done by the
 *                                table-copy path before streaming starts
 *                                (table_cache.rs:122)
 *   etlg_decode                  the body of the hot loop for N messages:
 *                                ReplicationMessage::parse +
 *                                LogicalReplicationMessage::parse
 *                                (postgres-replication 0.6.7, call sites
 *                                 apply.rs:2037-2125) → handle_*_message
 *                                (apply.rs:2279-2617) → codec::parse_event_from_*
 *                                (crates/etl/src/postgres/codec/event.rs:303-547)
 *                                → parse_cell_from_postgres_text
 *                                (crates/etl/src/postgres/codec/text.rs:32-153)
 *   etlg_last_error              EtlError {kind, description, detail}
 *                                (crates/etl/src/error.rs:27-76, 85-170)
 *   etlg_batch_*                 the Vec<Event> pushed into EventBatch
 *                                (apply.rs:1918-1928), as a columnar arena
 *
 * Conventions mirrored from the Rust side: callee allocates results, caller
 * frees through the exported free; a context is NOT re-entrant (the apply
 * loop is `&mut self`); decode is fail-fast: the first bad frame stops the
 * batch, all events before it stay valid, and the error carries the
 * reference's ErrorKind + static description string.
 *
 * No torch types, no C++ types: plain pointers and sizes only.
 */
#ifndef ETLG_H
#define ETLG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ETLG_ABI_VERSION 1u

/* ------------------------------------------------------------------ errors */

/* Subset of crates/etl/src/error.rs:85-170 `ErrorKind` reachable from the
 * decode path. Values are ours; names are the reference's. */
typedef enum etlg_error_kind {
  ETLG_OK = 0,
  ETLG_ConversionError = 1,        /* error.rs ConversionError */
  ETLG_InvalidData = 2,            /* error.rs InvalidData */
  ETLG_ValidationError = 3,        /* error.rs ValidationError */
  ETLG_InvalidState = 4,           /* error.rs InvalidState */
  ETLG_MissingTableSchema = 5,     /* error.rs MissingTableSchema */
  ETLG_CorruptedTableSchema = 6,   /* error.rs CorruptedTableSchema */
  ETLG_DeserializationError = 7,   /* error.rs DeserializationError */
  ETLG_SourceConnectionFailed = 8, /* wire-level parse failure: tokio_postgres::Error
                                      without SQLSTATE (error.rs:947) */
  ETLG_IoError = 9,                /* io::Error from cstr accessors (error.rs:564) */
  ETLG_UnsupportedValueInDestination = 10, /* error.rs:136; only from etlg_batch_protobuf (bigquery/validation.rs) */
  ETLG_NullValuesNotSupportedInArrayInDestination = 11, /* error.rs:134; only from etlg_batch_protobuf (reject_nulls, bigquery/validation.rs:127-141) */
  /* library-level (no reference analog) */
  ETLG_InvalidArgument = 100,
  ETLG_DeviceError = 101,
  ETLG_Unsupported = 102
} etlg_error_kind;

typedef struct etlg_error {
  int32_t kind;            /* etlg_error_kind */
  int32_t code;            /* etlg_err_code: identifies the static description */
  const char* description; /* the reference's static description string */
  const char* detail;      /* optional dynamic detail (may be NULL) */
  int64_t frame_index;     /* index of the offending CopyData frame, -1 if n/a */
} etlg_error;

/* One code per distinct (kind, static description) pair produced on this
 * path; the table lives in etlg_err_table() so oracle, kernels and tests
 * share numbering but not code. */
typedef enum etlg_err_code {
  ETLG_E_NONE = 0,
  ETLG_E_WIRE = 1,                /* SourceConnectionFailed / "PostgreSQL connection failed" */
  ETLG_E_TXN_STATE = 2,           /* InvalidState / "Invalid transaction state" */
  ETLG_E_COMMIT_LSN = 3,          /* ValidationError / "Invalid commit LSN" */
  ETLG_E_MISSING_SHARED_STATE = 4,/* InvalidState / "Missing shared table state" */
  ETLG_E_WAITING_RELATION = 5,    /* InvalidState / "Waiting for relation state cannot decode row event" */
  ETLG_E_TUPLE_WIDTH = 6,         /* ConversionError / "Tuple data field count does not match schema" */
  ETLG_E_FULL_ROW_MISSING = 7,    /* ConversionError / "Tuple missing source value for full row image" */
  ETLG_E_REQUIRED_NULL = 8,       /* InvalidData / "Required column missing from tuple" */
  ETLG_E_BINARY_FORMAT = 9,       /* ConversionError / "Binary format not supported in tuple data" */
  ETLG_E_UTF8 = 10,               /* ConversionError / "UTF-8 conversion failed" */
  ETLG_E_OLD_ROW_WIDTH = 11,      /* ConversionError / "Old tuple row width does not match schema" */
  ETLG_E_KEY_SHAPE = 12,          /* ConversionError / "Replica-identity tuple shape does not match schema" */
  ETLG_E_KEY_MISSING_COLS = 13,   /* ConversionError / "Replica-identity tuple missing key columns" */
  ETLG_E_KEY_MISSING_VALUE = 14,  /* ConversionError / "Replica-identity tuple missing source value" */
  ETLG_E_BOOL = 15,               /* InvalidData / "Invalid boolean value" */
  ETLG_E_INT = 16,                /* ConversionError / "Integer parsing failed" */
  ETLG_E_FLOAT = 17,              /* ConversionError / "Float parsing failed" */
  ETLG_E_NUMERIC = 18,            /* ConversionError / "Numeric parsing failed" */
  ETLG_E_BYTEA = 19,              /* ConversionError / "Bytea hex string conversion failed" */
  ETLG_E_DATETIME = 20,           /* ConversionError / "Datetime parsing failed" */
  ETLG_E_UUID = 21,               /* InvalidData / "UUID parsing failed" */
  ETLG_E_JSON = 22,               /* DeserializationError / "JSON deserialization failed" */
  ETLG_E_ARRAY_SHORT = 23,        /* ConversionError / "Array input too short" */
  ETLG_E_ARRAY_BRACES = 24,       /* ConversionError / "Array input missing braces" */
  ETLG_E_ARRAY_DIMS = 25,         /* ConversionError / "Array input has a malformed dimensions prefix" */
  ETLG_E_ARRAY_MULTIDIM = 26,     /* ConversionError / "Multidimensional array input is not supported" */
  ETLG_E_ARRAY_QUOTE = 27,        /* ConversionError / "Array input contains an unterminated quote" */
  ETLG_E_ARRAY_ESCAPE = 28,       /* ConversionError / "Array input contains an unterminated escape" */
  ETLG_E_SCHEMA_NOT_FOUND = 29,   /* MissingTableSchema / "Table schema not found" */
  ETLG_E_UNKNOWN_COLUMNS = 30,    /* CorruptedTableSchema / "Replication stream contains columns missing from the stored table schema" */
  ETLG_E_DDL_PARSE = 31,          /* ConversionError / "Failed to parse schema change message" */
  ETLG_E_IO = 32,                 /* IoError / "I/O operation failed" */
  ETLG_E_BOOTSTRAP_SNAPSHOT = 33, /* InvalidState / "Bootstrap table schema snapshot exceeded requested snapshot" */
  ETLG_E_SNAPSHOT_MISMATCH = 34,  /* InvalidState / "Table schema snapshot mismatch" */
  ETLG_E_CTRL_HINT = 35,          /* InvalidArgument / "Control frame found in a batch declared control-free" */
  /* table-copy rows (crates/etl/src/postgres/codec/table_row.rs:57-254) */
  ETLG_E_COPY_UNTERMINATED = 36,  /* ConversionError / "Row data not properly terminated" */
  ETLG_E_COPY_MORE_COLS = 37,     /* ConversionError / "Postgres COPY row contains more columns than the table schema" */
  ETLG_E_COPY_FEWER_COLS = 38,    /* ConversionError / "Postgres COPY row contains fewer columns than the table schema" */
  ETLG_E__COUNT
} etlg_err_code;

typedef struct etlg_err_desc {
  int32_t kind;
  const char* description;
} etlg_err_desc;

/* Static (kind, description) for a code; NULL if out of range. */
const etlg_err_desc* etlg_err_table(int32_t code);

/* ----------------------------------------------------------------- schemas */

/* Value class a column decodes to; determined by the column's *stored* type
 * OID exactly as parse_cell_from_postgres_text switches on it
 * (crates/etl/src/postgres/codec/text.rs:32-153; unknown OIDs are TEXT,
 * crates/etl-postgres/src/type_utils.rs:9-11). */
typedef enum etlg_type_class {
  ETLG_TC_STRING = 0, /* everything without a dedicated arm -> Cell::String */
  ETLG_TC_BOOL = 1,
  ETLG_TC_I16 = 2,
  ETLG_TC_I32 = 3,
  ETLG_TC_I64 = 4,
  ETLG_TC_U32 = 5, /* oid */
  ETLG_TC_F32 = 6,
  ETLG_TC_F64 = 7,
  ETLG_TC_NUMERIC = 8,
  ETLG_TC_BYTEA = 9,
  ETLG_TC_DATE = 10,
  ETLG_TC_TIME = 11,
  ETLG_TC_TIMETZ = 12,
  ETLG_TC_TIMESTAMP = 13,
  ETLG_TC_TIMESTAMPTZ = 14,
  ETLG_TC_UUID = 15,
  ETLG_TC_JSON = 16,
  ETLG_TC_ARRAY = 17, /* any `_xxx` array type; element class via etlg_array_elem_class */
  ETLG_TC__COUNT
} etlg_type_class;

/* OID -> class; never fails (unknown -> STRING). */
int32_t etlg_type_class_of_oid(uint32_t type_oid);
/* For an array OID: element class (STRING for arrays without a dedicated arm). */
int32_t etlg_array_elem_class(uint32_t array_type_oid);
/* Bytes a column of this class occupies in a row's fixed block (multiple of 4). */
uint32_t etlg_slot_bytes(int32_t type_class);

/* A stored column, in attnum order — what ColumnSchema carries
 * (crates/etl-postgres/src/schema.rs:213). */
typedef struct etlg_col {
  const char* name; /* NUL-terminated UTF-8; masks are built by name (crates/etl/src/schema.rs:30-61) */
  uint32_t type_oid;
  int32_t type_modifier;
  int32_t attnum;       /* ordinal_position */
  uint8_t nullable;     /* !attnotnull */
  uint8_t primary_key;  /* 1 if part of the primary key */
  uint8_t _pad[2];
} etlg_col;

/* Table replication state as seen by should_apply_changes
 * (apply.rs:2844-2850): Ready, SyncDone{lsn}, or anything else. */
typedef enum etlg_table_state_kind {
  ETLG_TS_ABSENT = 0,   /* no state stored -> never owned */
  ETLG_TS_READY = 1,
  ETLG_TS_SYNC_DONE = 2,/* owned iff lsn <= remote_final_lsn */
  ETLG_TS_OTHER = 3     /* Init/DataSync/FinishedCopy/SyncWait/Catchup/Errored */
} etlg_table_state_kind;

typedef enum etlg_worker_kind {
  ETLG_WORKER_APPLY = 0,
  ETLG_WORKER_TABLE_SYNC = 1
} etlg_worker_kind;

/* --------------------------------------------------------------- lifecycle */

typedef struct etlg_ctx etlg_ctx;
typedef struct etlg_batch etlg_batch;

uint32_t etlg_abi_version(void);

/* hip_device >= 0 selects the GPU. There is no CPU backend: creation fails
 * with ETLG_DeviceError when no gfx950 device is available. */
int32_t etlg_ctx_create(int32_t hip_device, etlg_ctx** out);
/* Human-readable reason of the last failed etlg_ctx_create on this thread's process. */
const char* etlg_create_error(void);
void etlg_ctx_destroy(etlg_ctx* ctx);

/* Run all device work of this context on an existing hipStream_t
 * (e.g. torch.cuda.current_stream().cuda_stream). NULL = own stream. */
int32_t etlg_ctx_set_stream(etlg_ctx* ctx, void* hip_stream);

int32_t etlg_ctx_set_worker(etlg_ctx* ctx, int32_t worker_kind,
                            uint32_t table_sync_table_id,
                            uint64_t bootstrap_snapshot_lsn);

int32_t etlg_schema_put(etlg_ctx* ctx, uint32_t table_id, uint64_t snapshot_lsn,
                        const char* schema_name, const char* table_name,
                        uint32_t ncols, const etlg_col* cols);

int32_t etlg_table_state(etlg_ctx* ctx, uint32_t table_id, int32_t state_kind,
                         uint64_t lsn);

/* Pre-populate the shared table cache with a Ready replicated schema built
 * from the stored schema at `snapshot_lsn` (at-or-before) and byte masks over
 * its columns (1 = replicated / identity). Returns the schema slot id (>= 0)
 * or a negative etlg_error_kind. */
int32_t etlg_table_ready(etlg_ctx* ctx, uint32_t table_id, uint64_t snapshot_lsn,
                         const uint8_t* replication_mask,
                         const uint8_t* identity_mask, uint32_t nmask);

/* Drop the shared-table-cache entry of a table (idempotent): SharedTableCache::remove_table
 * (crates/etl/src/replication/table_cache.rs:131-145), as the table-sync worker does before it restarts a table
 * (crates/etl/src/replication/table_sync/mod.rs:233). Rows of that table then fail with "Missing shared table state"
 * until a Relation message or etlg_table_ready installs a schema again. Stored schemas and slot ids are untouched. */
int32_t etlg_table_forget(etlg_ctx* ctx, uint32_t table_id);

/* The shared-table-cache entry of a table (SharedTableCache::get, table_cache.rs:99-102): returns 0 if there is none, else 1
 * with *kind = 1 WaitingForRelation | 2 Ready, *snapshot_lsn = the entry's snapshot id, *schema_slot = the Ready schema (-1 while waiting). */
int32_t etlg_table_cache_get(const etlg_ctx* ctx, uint32_t table_id, int32_t* kind, uint64_t* snapshot_lsn, int32_t* schema_slot);

/* Reset the transaction state (remote_final_lsn = None, next ordinal = 0),
 * as a fresh ApplyLoop does. */
int32_t etlg_ctx_reset_stream_state(etlg_ctx* ctx);

/* ------------------------------------------------------------------ decode */

enum {
  ETLG_F_INPUT_ON_DEVICE = 1u << 0,  /* buf / frame_offsets are device pointers */
  ETLG_F_OUTPUT_ON_DEVICE = 1u << 1, /* do not copy the arenas to the host; view holds device pointers */
  ETLG_F_NO_CONTROL = 1u << 2,       /* caller asserts: no R/M/T frame in this batch (skips the
                                        control-plane round trip; verified on device) */
  ETLG_F_ASYNC = 1u << 3,            /* with OUTPUT_ON_DEVICE | NO_CONTROL: enqueue only, do not synchronize;
                                        counts become valid after etlg_batch_sync. The input must be COMPLETE in
                                        device memory when the call is made: the batch may be decoded on a private
                                        stream beside its predecessor, not behind work enqueued on the context's
                                        stream (etlg_ctx_fence orders the other direction). Sync batches in issue
                                        order and keep fewer than 32 of them in flight per context (their
                                        result blocks live in a ring of 32; a batch that reports an error is
                                        decoded again, on the exact-error path, when it is synced).
                                        With frame_offsets = NULL the record-boundary scan of the batch runs on a
                                        private stream beside the previous batch's decode and the call returns with
                                        that scan in flight (the next call on the context, or the batch's sync,
                                        enqueues the decode): the input must be COMPLETE in device memory when the
                                        call is made (not merely enqueued on the context's stream).
                                        With HOST input (no INPUT_ON_DEVICE) and a sidecar: the bytes and the sidecar are
                                        uploaded into a device block the batch owns, on a private copy stream beside the
                                        decode of the batch before it, and the batch joins the chain like a device-input
                                        one. Truly asynchronous only from pinned memory (etlg_host_alloc); the caller must
                                        not touch buf / frame_offsets until the batch is synced (two staging buffers in
                                        rotation: fill one while the other is in flight). Without a sidecar a host-input
                                        batch is decoded synchronously, as before */
  ETLG_F_FINISH_CELLS = 1u << 4,     /* round 6: run etlg_batch_finish_cells(ETLG_FINISH_ARRAYS | ETLG_FINISH_FLOATS) on the batch
                                        before it is handed over (an ASYNC batch: when it is synced; a host-output batch: before
                                        the download): array cells come back TYPED (etlg_array_hdr entries) and no float cell
                                        comes back DEFERRED. Also honoured by etlg_copy_decode */
  ETLG_F_CHECK_CELLS = 1u << 5       /* json / jsonb cells that are not one JSON value and array literals the reference rejects are
                                        decode errors AT THEIR FRAME, as in the reference (parse_cell_from_postgres_text validates
                                        while it decodes the frame, codec/text.rs:126-134, 163-312; the apply loop stops there,
                                        apply.rs:2475-2481), instead of DEFERRED text whose error the next reader of the cell finds.
                                        The contract is with the DEFERRED rules below. etlg_decode and etlg_copy_decode, every
                                        combination of the other flags. Without it nothing changes */
};

/* Pinned (page-locked) host memory for the staging buffers of a host that feeds etlg_decode with ETLG_F_ASYNC: what the
 * reference's apply loop accumulates per batch (EventBatch, crates/etl/src/replication/apply.rs:1918-1928) becomes two or more
 * 64 MiB buffers of raw CopyData frames + their u32 offsets (crates/etl-gfx950/src/batcher.rs). Freed with etlg_host_free. */
int32_t etlg_host_alloc(etlg_ctx* ctx, size_t bytes, void** out);
void etlg_host_free(void* p);

/* buf = `nframes` concatenated CopyData frames exactly as on the socket:
 *   'd' | Int32-BE length (incl. itself) | payload
 * payload = XLogData 'w' | u64 wal_start | u64 wal_end | i64 ts | pgoutput msg
 *         | keepalive 'k' | u64 wal_end | i64 ts | u8 reply
 * frame_offsets: optional sidecar of nframes+1 byte offsets (the host learns
 * each frame length on receipt); NULL = the device scans record boundaries
 * itself and nframes is ignored. (The sidecar is also what lets fixed-width
 * batches skip every inter-tile dependency: frames are priced by their length
 * before they are read — DESIGN.md 3.0, k_plan_pre. Results do not depend on it.)
 * Returns 0, or the etlg_error_kind of the first failing frame (the batch is
 * still returned and holds every event before it). */
int32_t etlg_decode(etlg_ctx* ctx, const uint8_t* buf, size_t len,
                    const uint32_t* frame_offsets, size_t nframes,
                    uint32_t flags, etlg_batch** out);

const etlg_error* etlg_last_error(const etlg_ctx* ctx);

/* Table-copy rows. Replaces parse_table_row_from_postgres_copy_bytes
 * (crates/etl/src/postgres/codec/table_row.rs:47-254) applied to every item of the
 * TableCopyStream (crates/etl/src/postgres/stream/table_copy.rs:54-79).
 * buf = nrows COPY ... TO STDOUT (text format) row payloads exactly as CopyOutStream
 * yields them (one row per CopyData message, WITHOUT the 'd' framing), concatenated;
 * row_offsets = nrows + 1 byte offsets (required; host or device as buf).
 * schema_slot = the ReplicatedTableSchema to decode against: the value etlg_table_ready
 * returned (its replicated columns are the reference's `column_schemas`).
 * The rows come back in the same arena as a batch of Insert events: kind 'I',
 * table_id / schema_slot of the slot, start_lsn = commit_lsn = 0, tx_ordinal = row index,
 * one full-layout row per event; payload_bytes[0] = bytes of the rows decoded
 * (TableCopyPayloadMetadata). NULL fields ("\N") are NULL cells whatever the column's
 * nullability, as in the reference. Fail-fast: the first bad row ends the batch with the
 * reference's error; rows before it are valid. The stream state of the context
 * (transaction carry) is not touched.
 * flags: ETLG_F_INPUT_ON_DEVICE, ETLG_F_OUTPUT_ON_DEVICE, ETLG_F_ASYNC.
 * ETLG_F_ASYNC (with ETLG_F_OUTPUT_ON_DEVICE): enqueue only — the reference's caller streams rows continuously
 * (crates/etl/src/postgres/stream/table_copy.rs:78-99; the table-sync worker batches them, crates/etl/src/replication/table_sync/copy.rs) and
 * the next batch can be handed over while this one decodes. The call returns with the batch in flight; etlg_batch_sync finishes it
 * (counts, error, payload_bytes become valid then). Batches are synced in issue order, fewer than 32 in flight per context, as for
 * etlg_decode. Table-copy batches are independent of each other (a virtual transaction each): a batch that ends in an error does not
 * touch the batches behind it. Host rows are uploaded into a device block the batch owns, on a copy stream beside the decode of the
 * batch before it — truly asynchronous only from pinned memory (etlg_host_alloc); the caller keeps buf / row_offsets untouched (and
 * device-resident input alive) until the batch is synced. What the rows -> arena kernel leaves to the frame rewrite (a malformed row,
 * rows wider than a tile's window) is redone when the batch is synced. Mixing kinds on one context is allowed and serialises: a WAL
 * batch (etlg_decode) finishes the table-copy batches in flight first, and the other way round. */
int32_t etlg_copy_decode(etlg_ctx* ctx, int32_t schema_slot, const uint8_t* buf, size_t len,
                         const uint32_t* row_offsets, size_t nrows, uint32_t flags, etlg_batch** out);

/* Record-boundary scan on its own: the frame_offsets sidecar of `buf` (the same scan
 * etlg_decode runs when it is given none), e.g. to cut a staged stream into shards.
 * Follows 'd' | Int32-BE length from offset 0; a malformed header turns the rest of
 * the buffer into one last frame (which then fails in etlg_decode as a wire error).
 * Replaces the per-message framing the reference gets from its socket codec
 * (postgres/stream/replication_message.rs:89-230: one CopyData payload per stream item).
 * flags: ETLG_F_INPUT_ON_DEVICE (buf is a device pointer), ETLG_F_OUTPUT_ON_DEVICE
 * (offsets_out is a device pointer). offsets_out receives *nframes_out + 1 entries;
 * cap = entries available.
 * Device memory the scan keeps on the context (grow-only, released with the context): a scratch row of 360 16-bit
 * offsets per 8 KiB tile of the largest input scanned so far plus summaries — about 9 % of that input (5.9 MB for
 * 64 MiB, ~470 MB for an input near 4 GiB) — and, per batch in flight without a sidecar, an offsets buffer of
 * len / 24 + 1 024 entries. A tile with more than 360 frames (malformed input: frames shorter than a keepalive)
 * sends the whole scan to the one-lane kernel: correct, slow. */
int32_t etlg_scan_boundaries(etlg_ctx* ctx, const uint8_t* buf, size_t len, uint32_t flags,
                             uint32_t* offsets_out, size_t cap, size_t* nframes_out);

/* The pgoutput tag of every frame of a staged stream (the same classification etlg_decode runs first): tags_out[i] is
 * 'B' 'C' 'R' 'I' 'U' 'D' 'T' 'M' 'Y' 'O', 'k' for a keepalive, 0 for a malformed frame. It is what a host needs to cut
 * a stream into commit-aligned shards (cuts go after a 'C') and to find the rare Relation / DDL-message frames whose effects
 * every later shard must see (etl_amd/shard.py: plan_shards, control_stream) without reading the stream back.
 * Replaces, as a pre-pass, the message-kind dispatch of the apply loop (crates/etl/src/replication/apply.rs:2087-2125).
 * frame_offsets: nframes + 1 entries (required; e.g. from etlg_scan_boundaries).
 * flags: ETLG_F_INPUT_ON_DEVICE (buf / frame_offsets are device pointers), ETLG_F_OUTPUT_ON_DEVICE (tags_out is one). */
int32_t etlg_frame_tags(etlg_ctx* ctx, const uint8_t* buf, size_t len, const uint32_t* frame_offsets, size_t nframes,
                        uint32_t flags, uint8_t* tags_out);

/* Commit-aligned shard cuts of a staged stream (multi-GPU recipe): frames [0, nframes) as n_shards contiguous
 * ranges balanced by bytes, every interior cut right after a Commit ('C') frame — the transaction state (commit_lsn, next ordinal:
 * crates/etl/src/replication/apply.rs:942-963) is then shard-local. The frames are classified and the cuts found on the device; only
 * the n_shards - 1 cut indexes come back. cuts_out (HOST, n_shards + 1 entries): shard k = frames [cuts_out[k], cuts_out[k + 1]);
 * cuts_out[0] = 0, cuts_out[n_shards] = nframes; a stream with fewer Commits than shards leaves some ranges empty (cuts never go back).
 * The reference has no counterpart: it decodes one ordered stream in one task (apply.rs:1210-1336).
 * flags: ETLG_F_INPUT_ON_DEVICE (buf / frame_offsets are device pointers). n_shards <= 4096. */
int32_t etlg_shard_plan(etlg_ctx* ctx, const uint8_t* buf, size_t len, const uint32_t* frame_offsets, size_t nframes, uint32_t n_shards,
                        uint32_t flags, uint64_t* cuts_out);

/* Step 3 of the recipe: apply the control stream of a shard BEFORE this context's own (etlg_control_stream of that range, as the ranks
 * exchanged it) — its Relation and DDL-message frames update the schema store and the shared table cache exactly as in place
 * (apply.rs:2160-2276, 2363-2440) — drop the events it decodes to, and leave the context outside any transaction at ordinal 0, which is
 * where a commit-aligned shard starts. Call once per earlier shard, in rank order, then decode the own shard. HOST buffers; nframes = 0
 * only resets the transaction state. An error (a Relation frame the reference would reject) is the error of the shard that owns the
 * frame: it is returned here, and that shard's own decode reports it with its frame index. */
int32_t etlg_shard_replay(etlg_ctx* ctx, const uint8_t* buf, size_t len, const uint32_t* frame_offsets, size_t nframes);

/* The control stream of a frame range, extracted on the device (multi-GPU recipe): for every transaction of the
 * range that holds a Relation ('R') or logical-decoding Message ('M') frame, its Begin, those frames in order and its Commit
 * (a control frame outside any transaction of the range travels alone). Decoding that stream on another context has the same
 * effect on the schema store and the shared table cache as decoding the whole range (crates/etl/src/replication/apply.rs:
 * 2160-2276, 2363-2440 are the only writers) — it is what the ranks broadcast before they decode their shards.
 * out_bytes / out_offsets: HOST buffers for the frames and their n_frames + 1 offsets; n_bytes / n_frames are always set (a call
 * whose buffers are too small fails with ETLG_InvalidArgument and says what it needs). last_tag: the pgoutput tag of the range's
 * last frame ('C' when the range ends on a transaction boundary). Ranges without control frames — almost all — cost one
 * classification pass and an 8-byte copy; nothing else of the range leaves the device. */
int32_t etlg_control_stream(etlg_ctx* ctx, const uint8_t* buf, size_t len, const uint32_t* frame_offsets, size_t nframes,
                            uint32_t flags, uint8_t* out_bytes, size_t out_cap, uint32_t* out_offsets, size_t out_offsets_cap,
                            size_t* n_bytes, size_t* n_frames, uint32_t* last_tag);

/* ------------------------------------------------------------ batch (arena) */

/* Event kinds: the pgoutput tag of the message that produced the event. */
enum {
  ETLG_EV_BEGIN = 'B',
  ETLG_EV_COMMIT = 'C',
  ETLG_EV_RELATION = 'R',
  ETLG_EV_INSERT = 'I',
  ETLG_EV_UPDATE = 'U',
  ETLG_EV_DELETE = 'D',
  ETLG_EV_TRUNCATE = 'T'
};

/* ev_flags for U/D: bits 0-1 = old row kind, bit 2 = new row is Partial. */
enum {
  ETLG_OLD_NONE = 0,
  ETLG_OLD_FULL = 1, /* OldTableRow::Full */
  ETLG_OLD_KEY = 2,  /* OldTableRow::Key  */
  ETLG_FLAG_PARTIAL = 4
};

/* 2-bit per-cell state stored at the head of every row block. */
enum {
  ETLG_CELL_VALUE = 0,
  ETLG_CELL_NULL = 1,
  ETLG_CELL_MISSING = 2, /* only inside a Partial new row */
  ETLG_CELL_DEFERRED = 3 /* slot = (heap_off, len) of the source text; the host finishes
                            it with the reference's own parse_cell_from_postgres_text */
};

/* Which cells come back DEFERRED (the same rule is implemented by the oracle's CONTRACT mode):
 *  - json / jsonb and every array type: always;
 *  - date / time / timetz / timestamp / timestamptz: never. Texts in the fixed layout of the reference's fast paths
 *    (codec/time.rs:89-154) and the shapes it hands to chrono (`parse_from_str` with "%Y-%m-%d", "%H:%M:%S%.f",
 *    "%Y-%m-%d %H:%M:%S%.f": one-digit fields, whitespace in front of numbers, signed / long years, leap second
 *    :60 = second 59 with nanos + 10^9, more than nine fraction digits) are both decoded on the device; a text
 *    neither accepts is "Datetime parsing failed";
 *  - float4 / float8: decoded on the device whenever the result is certain: Clinger's exact path (mantissa
 *    <= 2^53, |exponent| <= 22: one IEEE operation), else the Eisel-Lemire algorithm on the first 19
 *    significant digits (as Rust's dec2flt does; a longer mantissa must round the same way for w and
 *    w + 1), plus zero, inf / infinity / nan. The rare text for which that is inconclusive (about 1 in
 *    10^4 of random decimal texts, essentially none of Postgres' own shortest-round-trip output) is
 *    DEFERRED. The rule is etl_amd/csrc/float_fast.h; the oracle evaluates the same header for the
 *    DECISION and glibc strtod / strtof for the value. Malformed text is the reference's
 *    "Float parsing failed". */

/* ---- ETLG_F_CHECK_CELLS: the errors of DEFERRED json / array text, raised by the decode.
 *
 *  1. The first frame (table copy: row) that holds, in a row image the reference parses, a json / jsonb cell that is not one JSON
 *     value (serde_json::from_str: ETLG_E_JSON) or an array literal the reference rejects — ETLG_E_ARRAY_DIMS / _MULTIDIM / _SHORT /
 *     _BRACES / _QUOTE / _ESCAPE, an element its type's parser refuses (that parser's own code: ETLG_E_INT, ETLG_E_BOOL,
 *     ETLG_E_DATETIME ...), ETLG_E_BYTEA for a bytea[] element, ETLG_E_JSON for a json[] / jsonb[] element — ends the batch exactly
 *     like any other decode error: the same etlg_error (kind, code, description, frame_index), n_frames = that frame, every event
 *     before it in the arena, the carried transaction state as of that frame, control-plane effects of later frames rolled back.
 *  2. The order is the reference's. Between frames the earliest frame wins, whatever the kind of error. Inside a frame the old image
 *     is read before the new one and cells in column order: an invalid json in column 1 beats a malformed int4 in column 3 of the
 *     same row, and the other way round; invalid UTF-8 inside a json cell is ETLG_E_UTF8 (str::from_utf8 precedes the type switch).
 *     Inside an array literal an element is parsed where it ends, so a bad element beats a shape error behind it. Cells the
 *     reference never parses raise nothing: frames should_apply_changes skips, the non-identity positions of a full-width key
 *     tuple, unchanged-toast ('u') cells that take the old image's value.
 *  3. What a lane of the device cannot decide is NOT an error and stays DEFERRED as without the flag: an array literal with a
 *     non-text element of more than 40 characters (the reference accepts any number of leading zeros), a json[] / jsonb[] element
 *     of more than 256 unescaped bytes. These are the only cells of a batch that came back ETLG_OK under the flag whose host parse
 *     can still fail.
 *  4. Valid cells stay DEFERRED source text: the flag changes no byte of an error-free batch's arena. With ETLG_F_FINISH_CELLS as
 *     well, the finish pass runs on the (possibly cut) batch as it does after any other error.
 *  5. Cost: one more kernel (k_chk_cells) behind the single-pass decode kernel of a batch that can decode against a schema with a
 *     json / jsonb / array column, none otherwise; no host stop, an ASYNC call returns as fast as without the flag. A batch that
 *     holds such a cell is decoded a second time by the multi-pass kernels (like a batch with any other error), which find the
 *     exact cut. */

/* ---- the finish pass (round 6): typed arrays and exact floats in the arena itself.
 *
 * The reference decodes an array cell to Cell::Array(ArrayCell::*) at decode time (parse_cell_from_postgres_text_array,
 * crates/etl/src/postgres/codec/text.rs:163-312) and every float text with Rust's correctly rounded str::parse (:52-59).
 * etlg_decode leaves array cells — and the rare float text its fast rule cannot decide — ETLG_CELL_DEFERRED (above);
 * etlg_batch_finish_cells settles them on the device, in place:
 *  - ETLG_FINISH_ARRAYS: every DEFERRED cell of an array column whose element class is bool / int2 / int4 / int8 / oid /
 *    float4 / float8 / date / time / timetz / timestamp / timestamptz / uuid / numeric / bytea / text-like
 *    (etlg_array_elem_class) and whose literal the reference accepts becomes ETLG_CELL_VALUE; its slot then holds
 *    (heap_off, bytes) of an etlg_array_hdr entry appended behind the batch's heap (heap_bytes grows; the source text
 *    stays where it was). NULL elements, quoting, escapes, the optional dimensions prefix, the unquoted-NULL rule:
 *    exactly the reference's state machine. A literal the reference REJECTS (unbalanced quotes, a multidimensional
 *    array, an element its type's parser refuses ...), a json / jsonb element, or a numeric / timetz element of more
 *    than 40 characters is left DEFERRED: the host's parse_cell_from_postgres_text then raises the reference's own
 *    error (or finishes the cell), as before.
 *  - ETLG_FINISH_FLOATS: every DEFERRED float4 / float8 cell gets its correctly rounded bits (the conversion Rust's
 *    dec2flt falls back to: 768 decimal digits shifted into place, core::num::dec2flt::slow) and becomes
 *    ETLG_CELL_VALUE; float elements of arrays likewise. With both bits set the only DEFERRED cells left in a batch
 *    are json / jsonb, json arrays and literals the reference rejects.
 * The batch must be device-resident and finished (an ASYNC batch is synced first). Events, row blocks and every
 * heap reference that existed stay where they are. */
enum { ETLG_FINISH_ARRAYS = 1u, ETLG_FINISH_FLOATS = 2u };

/* A typed array in the heap (4-byte aligned, a multiple of 4 bytes long):
 *   etlg_array_hdr
 *   uint32_t validity[(n_elems + 31) / 32]      bit k set: element k is a value (clear: NULL)
 *   elem_bytes != 0:  n_elems slots of elem_bytes bytes, each laid out like a row slot of elem_class (NULL: zeros)
 *   elem_bytes == 0:  uint32_t end[n_elems] — element k is data[end[k-1] .. end[k]) (end[-1] = 0) — then the data,
 *                     zero padded to 4 bytes: String / Bytes elements are their unescaped bytes; a Numeric element is an
 *                     etlg_numeric_hdr + digits, padded to 4 bytes (its end offset includes the padding) */
typedef struct etlg_array_hdr {
  uint32_t n_elems;
  uint8_t elem_class; /* etlg_type_class of the elements */
  uint8_t elem_bytes; /* etlg_slot_bytes(elem_class) for fixed-width elements, 0 for String / Bytes / Numeric */
  uint16_t reserved;  /* 0 */
} etlg_array_hdr;

typedef struct etlg_finish_stats {
  uint64_t deferred_seen;  /* DEFERRED cells of array / float columns the pass looked at */
  uint64_t arrays_typed;
  uint64_t floats_settled;
  uint64_t left_deferred;  /* of deferred_seen: still DEFERRED (the host finishes them) */
  uint64_t heap_bytes_added;
} etlg_finish_stats;

/* what: ETLG_FINISH_* bits. stats may be NULL. Idempotent (a second call finds nothing it can settle). */
int32_t etlg_batch_finish_cells(etlg_ctx* ctx, etlg_batch* batch, uint32_t what, etlg_finish_stats* stats);

/* Numeric heap entry header (followed by ndigits little-endian i16 base-10000
 * digits): mirrors PgNumeric (crates/etl-postgres/src/numeric.rs:75-96). */
enum { ETLG_NUM_VALUE = 0, ETLG_NUM_NAN = 1, ETLG_NUM_PINF = 2, ETLG_NUM_NINF = 3 };
typedef struct etlg_numeric_hdr {
  uint8_t kind; /* ETLG_NUM_* */
  uint8_t sign; /* 0 positive, 1 negative */
  int16_t weight;
  uint16_t scale;
  uint16_t ndigits;
} etlg_numeric_hdr;

/* One replicated column of a schema slot. */
typedef struct etlg_slot_col {
  uint32_t type_oid;
  uint16_t stored_index; /* index into the stored (attnum-ordered) schema */
  uint8_t type_class;    /* etlg_type_class */
  uint8_t nullable;
  uint8_t identity;      /* replicated && identity */
  uint8_t _pad;
  uint16_t off_full;     /* byte offset of the slot inside a full-layout row block */
  uint16_t off_key;      /* byte offset inside a key-layout row block (identity cols only) */
  uint16_t key_index;    /* position among identity columns, 0xFFFF if not identity */
} etlg_slot_col;

/* A ReplicatedTableSchema instance (crates/etl/src/schema.rs:380-441): the
 * stored schema at one snapshot + replication/identity masks. */
typedef struct etlg_slot_desc {
  uint32_t table_id;
  uint32_t n_stored;     /* columns in the stored schema */
  uint64_t snapshot_lsn; /* snapshot id of the stored schema */
  uint32_t n_cols;       /* replicated columns */
  uint32_t n_ident;      /* replicated identity columns */
  uint32_t row_bytes_full; /* state bytes (padded to 4) + slots */
  uint32_t row_bytes_key;
  uint32_t state_bytes_full; /* = 4*ceil(n_cols/16) */
  uint32_t state_bytes_key;  /* = 4*ceil(n_ident/16) */
  const etlg_slot_col* cols; /* n_cols entries, replicated order */
} etlg_slot_desc;

/* Columnar view of a decoded batch. Every array has n_events entries.
 *
 *   kind 'B': table_id = xid;            body = i64 commit timestamp
 *   kind 'C': flags    = commit flags;   body = u64 end_lsn, i64 timestamp
 *   kind 'R': table_id, schema_slot;     no body
 *   kind 'I': table_id, schema_slot;     body = new row (full layout)
 *   kind 'U': flags = old kind|partial;  body = [old row][new row]
 *   kind 'D': flags = old kind;          body = [old row]
 *   kind 'T': flags = options, table_id = n owned tables;
 *                                         body = n x {u32 table_id, u32 schema_slot}
 *
 * Row block (full layout: all replicated columns; key layout: identity
 * columns only): 2-bit cell states, column i at bits 2*(i%4) of byte i/4,
 * padded to 4 bytes; then one slot per column at off_full/off_key.
 * Slot contents, little-endian, zero for NULL/MISSING cells:
 *   BOOL u32 0/1 | I16 i32 | I32 i32 | U32 u32 | I64 i64 | F32 u32 bits (8-byte slot)
 *   F64 u64 bits | DATE i32 days from CE (chrono NaiveDate, 8-byte slot)
 *   TIME u32 secs-of-day, u32 nanos | TIMESTAMP/TIMESTAMPTZ i32 days, u32 secs, u32 nanos
 *   TIMETZ u32 secs, u32 nanos, i32 offset seconds east | UUID 16 bytes
 *   STRING/BYTEA/NUMERIC/JSON/ARRAY and any DEFERRED cell: u32 heap_off, u32 len
 * Heap entries are 4-byte aligned and zero padded; STRING/DEFERRED hold the
 * source text verbatim, BYTEA the decoded bytes, NUMERIC an etlg_numeric_hdr
 * + digits (len = 8 + 2*ndigits). A toast cell resolved from the old row
 * aliases the old row's heap entry (Cell::clone).
 * body_off is in bytes into `fixed`; bodies are contiguous in event order.
 */
typedef struct etlg_batch_view {
  uint64_t n_events;
  uint64_t n_frames;        /* frames consumed (index of the failing frame on error) */
  uint64_t fixed_bytes;
  uint64_t heap_bytes;
  uint64_t payload_bytes[3]; /* insert/update/delete value bytes (codec/event.rs:261-297) */
  const uint8_t* ev_kind;
  const uint8_t* ev_flags;
  const uint32_t* ev_table_id;
  const uint32_t* ev_schema_slot;
  const uint64_t* ev_start_lsn;
  const uint64_t* ev_commit_lsn;
  const uint64_t* ev_tx_ordinal;
  const uint64_t* ev_body_off;
  const uint8_t* fixed;
  const uint8_t* heap;
  uint32_t on_device;       /* 1: the pointers above are device pointers */
  uint32_t n_slots;         /* schema slots known to the context (ids are stable across batches) */
  const etlg_slot_desc* slots; /* host memory */
} etlg_batch_view;

int32_t etlg_batch_view_get(const etlg_batch* batch, etlg_batch_view* out);
/* Wait for an ETLG_F_ASYNC batch and refresh its counts/error. */
int32_t etlg_batch_sync(etlg_ctx* ctx, etlg_batch* batch);
/* Enqueue (no synchronisation) a device-to-device copy of the batch's 64-byte
 * result header into `dst_device_8xu64`:
 *   {first_err key (~0 = none), n_events, fixed_bytes, heap_bytes,
 *    payload insert/update/delete bytes, n_frames}
 * Must be called right after the etlg_decode that produced `batch`. This is the
 * per-shard record the multi-GPU all-gather exchanges (one fixed-size header per
 * rank; rank order == LSN order). For a finished batch the copy is enqueued on the
 * context's stream; for an ETLG_F_ASYNC batch in flight it travels on a private
 * stream behind the batch's kernels (a copy between two decode kernels costs a
 * dispatch gap): call etlg_ctx_fence before work on the context's stream reads it. */
int32_t etlg_batch_header_to_device(etlg_ctx* ctx, etlg_batch* batch, void* dst_device_8xu64);
/* Makes the context's stream wait (on the device; the host does not block) for every
 * ETLG_F_ASYNC batch enqueued so far: their decode kernels — consecutive batches may
 * run on two private streams side by side — and their header copies. Device work the
 * caller enqueues on the context's stream afterwards sees their arenas and headers. */
int32_t etlg_ctx_fence(etlg_ctx* ctx);
/* Copy a device-resident (ETLG_F_OUTPUT_ON_DEVICE) batch into host memory;
 * afterwards the view holds host pointers. */
int32_t etlg_batch_download(etlg_ctx* ctx, etlg_batch* batch);
void etlg_batch_free(etlg_batch* batch);

/* ------------------------------------------------------ columnar hand-off */

/* Arrow-layout column buffers for the rows of ONE schema slot of a decoded batch,
 * built on the device from the arena (no Cell objects, no per-row host work).
 * Replaces rows_to_record_batch / build_array_for_field and the cell_to_*
 * converters of the reference's Arrow sinks
 * (crates/etl-destinations/src/iceberg/encoding.rs:34-84, :150-360). */
typedef enum etlg_arrow_kind {
  ETLG_AK_BOOLEAN = 0,      /* values bit-packed, LSB first */
  ETLG_AK_INT32 = 1,        /* I16, I32 (cell_to_i32, encoding.rs:157) */
  ETLG_AK_INT64 = 2,        /* I64, U32 (cell_to_i64, encoding.rs:164) */
  ETLG_AK_FLOAT32 = 3,
  ETLG_AK_FLOAT64 = 4,
  ETLG_AK_DATE32 = 5,       /* days since 1970-01-01 (encoding.rs:194) */
  ETLG_AK_TIME64_US = 6,    /* encoding.rs:201 */
  ETLG_AK_TIMESTAMP_US = 7, /* encoding.rs:208 */
  ETLG_AK_TIMESTAMP_US_UTC = 8, /* encoding.rs:215 */
  ETLG_AK_FIXED16 = 9,      /* uuid: FixedSizeBinary(16) */
  ETLG_AK_LARGE_UTF8 = 10,  /* i64 offsets + bytes */
  ETLG_AK_LARGE_BINARY = 11,
  ETLG_AK_TEXT_FORM = 12,   /* json / arrays: the cell's heap entry (the source text), i64 offsets + bytes; the host finishes it. A json /
                             * jsonb cell has been checked on the device to be one JSON value under serde_json's rules (codec/text.rs:
                             * 126-134): a malformed one fails the call with ETLG_E_JSON at its event, so the host's parse cannot fail (except behind a list
                             * row handed back DEFERRED, see ETLG_ROWS_PARSE_ARRAYS: then the host meets it in event order).
                             * (numeric and timetz columns are ETLG_AK_LARGE_UTF8 of their Display strings — `n.to_string()`,
                             * `t.to_string()`, cell_to_string encoding.rs:349-352 — formatted on the device) */
  ETLG_AK_LIST = 13,        /* only with ETLG_ROWS_PARSE_ARRAYS: array literals parsed on the device (parse_cell_from_postgres_text_array,
                             * codec/text.rs:228-312): i64 list offsets in `offsets`, child validity in `child_validity`, child values
                             * in `values` (child_kind layout). Elements: bool / int2 / int4 / int8 / oid / float4 / float8 / date / time /
                             * timestamp / timestamptz / uuid (fixed-width children), text and every array type without a dedicated
                             * arm (LargeUtf8 child), numeric / timetz (LargeUtf8 child of the elements' Display strings, as the sinks
                             * write them), bytea (LargeBinary child of the decoded bytes). Var-len children: `child_offsets`.
                             * json[] / jsonb[] (round 6): LargeUtf8 child of `j.to_string()` per element (ArrayCell::Json,
                             * iceberg/encoding.rs:577-585); an element of more than 256 bytes or beyond the json writer's limits
                             * (depth 16, 64 members) hands its row back (`deferred`), one that is not JSON is ETLG_E_JSON */
  /* etlg_batch_ducklake_copy only (arrow_column_kind, crates/etl-destinations/src/ducklake/encoding.rs:236-257) */
  ETLG_AK_INT16 = 14,       /* int2: 2-byte values */
  ETLG_AK_UINT64 = 15,      /* oid, widened */
  ETLG_AK_UTF8 = 16,        /* text and the Display strings of numeric / timetz: i32 offsets + bytes */
  ETLG_AK_BINARY = 17,      /* bytea: i32 offsets + bytes */
  ETLG_AK_NONE = 255        /* not handed off - no buffers (no class maps to it today) */
} etlg_arrow_kind;

typedef struct etlg_column {
  uint32_t type_class;      /* etlg_type_class of the replicated column */
  uint32_t arrow_kind;      /* etlg_arrow_kind */
  uint32_t value_bytes;     /* bytes per row in `values` (0: bit-packed or var-len) */
  uint32_t nullable;
  uint64_t null_count;      /* rows whose validity bit is 0 */
  uint64_t deferred_count;  /* rows set in `deferred` */
  const uint8_t* validity;  /* n_rows bits, LSB first, padded to 8 bytes */
  const uint8_t* deferred;  /* same shape: cells the kernels handed back ETLG_CELL_DEFERRED. In a fixed-width
                             * column they are null in `validity`; in a TEXT_FORM column their entry is the source text */
  const uint8_t* values;
  const int64_t* offsets;   /* var-len kinds: n_rows + 1 entries, else NULL. ETLG_AK_UTF8 / ETLG_AK_BINARY: the pointer is to n_rows + 1
                             * INT32 entries (Arrow's Utf8 / Binary) — read it as const int32_t* */
  uint64_t values_bytes;    /* bytes behind `values` */
  /* ETLG_AK_LIST only */
  uint32_t child_kind;      /* the element column's etlg_arrow_kind (BOOLEAN, INT32, INT64, FLOAT32/64, DATE32, TIME64_US, TIMESTAMP_US[_UTC], FIXED16,
                             * LARGE_UTF8) */
  uint32_t _pad;
  uint64_t child_count;     /* elements of all rows = offsets[n_rows] */
  uint64_t child_null_count;
  const uint8_t* child_validity; /* child_count bits */
  const int64_t* child_offsets;  /* child_kind ETLG_AK_LARGE_UTF8 (text[] and every array without a dedicated element type): child_count + 1
                                  * byte offsets into `values`, the unescaped element texts back to back */
} etlg_column;

typedef struct etlg_columns_view {
  uint64_t n_rows;
  uint32_t n_cols;          /* replicated columns of the slot, slot order */
  uint32_t on_device;       /* 1: buffer pointers are device pointers */
  const etlg_column* cols;  /* host memory */
  const uint64_t* row_event; /* n_rows: index of the event each row came from (event order) */
} etlg_columns_view;

typedef struct etlg_columns etlg_columns;

#define ETLG_ROWS_INSERT 1u  /* Insert rows */
#define ETLG_ROWS_UPDATE 2u  /* the new row of non-partial Updates */
#define ETLG_ROWS_PARSE_ARRAYS 4u /* array columns of a fixed-width element class become ETLG_AK_LIST; a malformed literal
                                   * fails the call with the reference's error (ETLG_E_ARRAY_* / the element's parse error,
                                   * frame_index = the event index), as parse_cell_from_postgres_text does at decode time — unless
                                   * a row the device hands back DEFERRED (an element of more than 40 characters, a float text its
                                   * rule does not settle) precedes the first malformed one: then the call succeeds and the
                                   * malformed rows are handed back too, so that the consumer, finishing the deferred rows in event
                                   * order, meets the first problem first */
#define ETLG_ROWS_FORMAT_JSON 8u  /* json / jsonb columns become ETLG_AK_LARGE_UTF8 of serde_json's `Value::to_string()` — what the sinks
                                   * write (`Cell::Json(j) => j.to_string()`: iceberg/encoding.rs:356, ducklake/encoding.rs:173): compact,
                                   * object members in the byte order of their decoded keys with the last of repeated keys, strings escaped
                                   * again, number literals kept (an unsigned exponent gains '+': codec/text.rs:812-815). A cell beyond what
                                   * a lane does (nesting deeper than 16, an object of more than 64 members) keeps its source text and its
                                   * bit in `deferred`, like every cell of an ETLG_AK_TEXT_FORM column; a cell that is not one JSON value
                                   * fails the call with ETLG_E_JSON as without the flag. etlg_batch_rowbinary / _protobuf always write
                                   * the Display string (and report such a cell as host_event / host_column). */

/* `batch` must be device-resident (decoded with ETLG_F_OUTPUT_ON_DEVICE, not downloaded) and finished
 * (an ETLG_F_ASYNC batch is synced first). flags: ETLG_F_OUTPUT_ON_DEVICE keeps the buffers in HBM, otherwise
 * they are copied to host memory. An unchanged-toast cell cannot occur (partial rows are not selected). */
int32_t etlg_batch_columns(etlg_ctx* ctx, etlg_batch* batch, int32_t schema_slot, uint32_t row_kinds,
                           uint32_t flags, etlg_columns** out);
int32_t etlg_columns_view_get(const etlg_columns* cols, etlg_columns_view* out);
/* Returns the buffers to the context's pool (no device synchronisation): work the caller enqueued on them must be complete. */
void etlg_columns_free(etlg_columns* cols);

/* The Iceberg sink's changelog rows for ONE schema slot of a decoded batch, as the Arrow column buffers of etlg_batch_columns plus the
 * two trailing CDC columns (crates/etl-destinations/src/iceberg/core.rs:300-416, write_table_rows :268-291): in event order, at most
 * one row per event,
 *   Insert -> the row; Update -> the full new row; Delete -> the full OLD row,
 * and behind the slot's replicated columns two non-nullable ETLG_AK_LARGE_UTF8 columns (type_class ETLG_TC_STRING, null_count 0,
 * validity all ones) of fixed-width values:
 *   cols[n_data_cols]      cdc_operation   "INSERT" | "UPDATE" | "DELETE" (IcebergOperationType Display, core.rs:77-85): offsets[i] = 6 i
 *   cols[n_data_cols + 1]  sequence_number `{commit_lsn:016x}/{tx_ordinal:016x}` of the row's event, lower-case hex (event_sequence_key()
 *                          .to_string(), crates/etl/src/event.rs:346-351): offsets[i] = 33 i
 * The events the sink refuses with SourceReplicaIdentityError (iceberg_update_row / iceberg_delete_row, core.rs:636-680) are not among
 * the rows: a partial Update, a Delete that carries only the key, a Delete without an old image. They are counted (n_host_rows) and the
 * first of them in event order is named with its reason; the other rows are still built, as in the other hand-offs. The reference fails
 * the WHOLE write_events call at the first refused event across ALL tables (the `?` at core.rs:332-350): the host takes the minimum
 * host_event over the slots it hands off and raises the error text of core.rs:642-678. Column NAMES (find_unique_column_name,
 * core.rs:685-), Relation events and Truncates stay on the host.
 * A table-copy batch (etlg_copy_decode): every row is kept, the operation is "INSERT" and the sequence number is
 * generate_sequence_number(0, 0) = "0000000000000000/0000000000000000" (event.rs:370-375).
 * opts: ETLG_ROWS_PARSE_ARRAYS | ETLG_ROWS_FORMAT_JSON, as for etlg_batch_columns; the row kinds are fixed, any other bit is
 * ETLG_InvalidArgument. Batch requirements, flags and the reports of malformed array literals / json cells (first row in event order,
 * then first column, over the rows selected here) as for etlg_batch_columns. An unchanged-toast cell cannot occur: partial rows are not
 * selected, and a Delete's full old row is decoded through convert_tuple_to_row, which accepts no unchanged-toast cell
 * (codec/event.rs:552). The result is read with etlg_columns_view_get (n_cols = the slot's columns + 2) and freed with
 * etlg_columns_free; the call synchronises with the device exactly as often as etlg_batch_columns does for the same slot and options. */
#define ETLG_ICE_PARTIAL_UPDATE 1u
#define ETLG_ICE_KEY_ONLY_DELETE 2u
#define ETLG_ICE_DELETE_WITHOUT_OLD_ROW 3u
typedef struct etlg_changelog_info {
  uint64_t n_host_rows;  /* Update / Delete events of the slot the sink refuses; they are not among the rows */
  uint64_t host_event;   /* the first of them in event order, ~0 = none */
  uint32_t host_reason;  /* ETLG_ICE_* of host_event, 0 = none */
  uint32_t n_data_cols;  /* cols[0..n_data_cols) = the slot's replicated columns; [n_data_cols] cdc_operation, [+1] sequence_number */
} etlg_changelog_info;
int32_t etlg_batch_iceberg(etlg_ctx* ctx, etlg_batch* batch, int32_t schema_slot, uint32_t opts, uint32_t flags, etlg_columns** out);
/* ETLG_InvalidArgument for an object that etlg_batch_columns built. */
int32_t etlg_columns_changelog_get(const etlg_columns* cols, etlg_changelog_info* out);

/* DuckLake's Arrow copy staging for ONE schema slot of a TABLE-COPY batch (etlg_copy_decode): the column buffers of the RecordBatch
 * prepare_copy_rows appends through the DuckDB appender (crates/etl-destinations/src/ducklake/encoding.rs:32-49,
 * copy_rows_to_arrow_record_batch :303-340) — every row of the batch, in order. Column kinds by type class (arrow_column_kind :236-257):
 *   BOOL BOOLEAN | I16 INT16 | I32 INT32 | I64 INT64 | U32 UINT64 | F32 / F64 FLOAT32 / FLOAT64 | DATE DATE32 | TIME TIME64_US |
 *   TIMESTAMP TIMESTAMP_US | TIMESTAMPTZ TIMESTAMP_US_UTC | BYTEA BINARY | STRING, NUMERIC, TIMETZ UTF8 (numeric / timetz: their
 *   Display strings, push_cell :170-171, as in etlg_batch_columns).
 * Null slots hold zero values (arrow's From<Vec<Option<T>>>), a null var-len entry is empty; validity, null_count and `nullable` (the
 * column's, for the Field) as in etlg_batch_columns. A DEFERRED cell (a float text the fast rule does not settle) is null, set in
 * `deferred` and counted in deferred_count, as there: a caller that wants none decodes with ETLG_F_FINISH_CELLS.
 * A slot with a UUID, JSON or ARRAY class column has no Arrow form (arrow_column_kinds returns None; the sink takes prepare_rows, which
 * ETLG_DL_TUPLES and the host cover): the call gives ETLG_OK and builds nothing — n_rows = 0, n_cols = 0, status ETLG_DLC_NOT_ARROW,
 * `column` = the first such column. Array types outside the value codec's table decode as ETLG_TC_STRING and cannot be told here: only
 * the caller has is_array_type, and it MUST NOT ask for the Arrow form of such a table.
 * 32-bit offsets: arrow-rs panics when a StringArray's / BinaryArray's bytes pass i32::MAX. A var-len column whose bytes exceed
 * 2^31 - 1 gives ETLG_OK, no buffers (n_rows = 0, n_cols = 0), status ETLG_DLC_OFFSETS_OVERFLOW and the first such column; the caller
 * splits the batch. (Tests lower the cap with the environment variable ETLG_DLC_OFFSET_CAP=<bytes>, read when the context is created.)
 * No conversion error exists on this path: date_days_since_epoch cannot fail (chrono's dates span about +-96 million days, which fits
 * i32) and time_micros_since_midnight cannot fail, so no error path is built for them.
 * A batch that is not a table-copy batch is ETLG_InvalidArgument (the reference uses this form for copy rows only). Batch
 * requirements and ETLG_F_OUTPUT_ON_DEVICE as for etlg_batch_columns; the call synchronises with the device exactly as often as
 * etlg_batch_columns does for the same slot. The result is read with etlg_columns_view_get and freed with etlg_columns_free. */
#define ETLG_DLC_OK 0u
#define ETLG_DLC_NOT_ARROW 1u
#define ETLG_DLC_OFFSETS_OVERFLOW 2u
typedef struct etlg_ducklake_copy_info {
  uint32_t status;  /* ETLG_DLC_* */
  uint32_t column;  /* NOT_ARROW / OFFSETS_OVERFLOW: the first column that has no Arrow form / whose bytes pass the cap; else 0 */
  uint32_t _pad[2];
} etlg_ducklake_copy_info;
int32_t etlg_batch_ducklake_copy(etlg_ctx* ctx, etlg_batch* batch, int32_t schema_slot, uint32_t flags, etlg_columns** out);
/* ETLG_InvalidArgument for any other object (etlg_batch_columns, etlg_batch_iceberg). */
int32_t etlg_columns_ducklake_get(const etlg_columns* cols, etlg_ducklake_copy_info* out);

/* ClickHouse RowBinary rows for ONE schema slot of a decoded batch, encoded on the device: what
 * cell_to_clickhouse_value + encode_to_row_binary (crates/etl-destinations/src/clickhouse/encoding.rs:58-83,
 * :188-283) and append_cdc_columns (clickhouse/core.rs:96-114) produce for the rows core.rs:1078-1127 collects:
 * Insert -> the row; Update -> the new row; Delete -> the old row, and for a Delete that carries only the key the tombstone row
 * expand_key_row builds (core.rs:1437-1472: the key cells in the primary-key columns, NULL in every other column that is nullable
 * at the source and not an array, default_cell's zero value (:1481-1517) in the rest) when the slot's replica identity is the primary
 * key or Full (ensure_clickhouse_key_identity_is_primary_key, :1404-1427) and no nullable non-key column has a type outside the value
 * codec's table (is_array_type decides NULL or empty array there; only the host knows every array type). Events the reference
 * refuses or the device does not build (a Partial update, key-only Deletes of other slots) are left out and counted in n_host_rows.
 * Columns of class numeric / timetz / time are Display strings in the reference (`n.to_string()`, encoding.rs:66-71): they are
 * formatted on the device (PgNumeric Display, crates/etl-postgres/src/numeric.rs:460-560; PgTimeTz, etl-postgres/src/time.rs:113-117,
 * 210-225); so is a json / jsonb cell (`j.to_string()`, encoding.rs:73: serde_json's Display, see ETLG_ROWS_FORMAT_JSON — a cell that
 * is not one JSON value fails the call with ETLG_E_JSON at its event, the reference's decode error, before any report of the sink's own).
 * Arrays of every element class leave as Array(Nullable(T)) (array_cell_to_clickhouse_values, encoding.rs:86-111): fixed-width values,
 * text-like elements as the unescaped text, numeric / timetz / json elements as their Display strings, bytea elements as bytes_to_hex.
 * A DEFERRED scalar cell / an array literal the device cannot take apart (malformed: the host raises the reference's decode error; a
 * numeric / timetz element of more than 40 characters, a json element of more than 256 bytes) / a json cell beyond json_display's
 * limits in a row makes the call return status ETLG_RB_NEEDS_HOST (no bytes; host_event / host_column name the first such cell). Arrays of fixed-width elements are encoded as Array(Nullable(T)). */
typedef enum etlg_ch_engine {
  ETLG_CH_MERGE_TREE = 0,           /* + cdc_operation String, cdc_lsn UInt64 */
  ETLG_CH_REPLACING_MERGE_TREE = 1  /* + _etl_version UInt128 (commit_lsn << 64 | tx_ordinal), _etl_deleted UInt8 */
} etlg_ch_engine;

#define ETLG_RB_OK 0u
#define ETLG_RB_NEEDS_HOST 3u

typedef struct etlg_rowbinary_view {
  uint64_t n_rows;
  uint64_t n_bytes;
  uint64_t n_host_rows;       /* Insert/Update/Delete events of the slot that are not among the rows */
  uint32_t status;            /* ETLG_RB_OK | ETLG_RB_NEEDS_HOST */
  uint32_t on_device;
  uint64_t host_event;        /* NEEDS_HOST: the first event (and column) the device cannot encode; ~0 = the slot's classes */
  uint32_t host_column;
  uint32_t _pad;
  const uint8_t* bytes;       /* rows back to back, event order */
  const int64_t* row_offsets; /* n_rows + 1 (the client cuts inserts at max_bytes_per_insert, client.rs:566-600) */
  const uint64_t* row_event;  /* n_rows */
} etlg_rowbinary_view;

typedef struct etlg_rowbinary etlg_rowbinary;

/* nullable_flags: one byte per destination column = the slot's replicated columns, then the engine's two CDC
 * columns (nullable_flags_from_clickhouse_columns, clickhouse/core.rs:162-209); n_flags must be n_cols + 2
 * ("ClickHouse RowBinary row width mismatch", encoding.rs:263-274, otherwise). A NULL in a non-nullable column and a
 * date outside 1900-01-01..=2299-12-31 fail the call with ETLG_ConversionError like the reference (etlg_last_error:
 * the description, frame_index = the event index). Same batch requirements as etlg_batch_columns.
 * A table-copy batch (etlg_copy_decode): every row of the slot is kept, in row order, its data columns encoded as an Insert event's
 * under the same nullable_flags rules and errors, and the CDC tail is that of append_cdc_columns(Insert, PgLsn 0, tx_ordinal 0, engine)
 * (write_table_rows_inner, clickhouse/core.rs:739-773): MergeTree String("INSERT") + UInt64 0, ReplacingMergeTree UInt128 0 + UInt8 0.
 * n_host_rows is 0. */
int32_t etlg_batch_rowbinary(etlg_ctx* ctx, etlg_batch* batch, int32_t schema_slot, const uint8_t* nullable_flags,
                             uint32_t n_flags, int32_t engine, uint32_t flags, etlg_rowbinary** out);
/* BigQuery Storage Write rows for ONE schema slot: the protobuf bytes of the BigQueryTableRows the sink builds for the slot's events
 * (crates/etl-destinations/src/bigquery/core.rs:978-1036; cell_encode_prost, bigquery/encoding.rs:120-190: field tag = column position
 * + 1, NULL cells leave nothing), every row closed by _CHANGE_TYPE and _CHANGE_SEQUENCE_NUMBER =
 * "{commit_lsn:016x}/{tx_ordinal:016x}/{ordinal:016x}" (core.rs:1405-1407):
 *   Insert -> one UPSERT row (ordinal 0);
 *   Update -> the new row as UPSERT; when the update changed the primary key — the old image's primary-key cells (key image or full
 *             old row) against the new row's, bigquery_primary_key_changed :1557-1645 — a sparse DELETE row of the OLD key goes first
 *             (ordinal 0) and the UPSERT takes ordinal 1 (:1425-1476): such an event is two consecutive rows with the same row_event;
 *   Delete -> the sparse DELETE row: the old image's primary-key cells under their column tags (bigquery_delete_row :1742-1754).
 * Events the reference refuses are left out and counted in n_host_rows (the host raises the reference's error when it meets the first):
 * a partial update, a delete without an old row, a key image or an update without an old row under a replica identity other than the
 * primary key (:1497-1555). So are updates that carry an old row when a primary-key column is of a class whose Cell equality is not
 * equality of the arena's words / bytes (float4 / float8, numeric, timetz), or a primary-key cell is DEFERRED.
 * numeric / timetz cells are their Display strings, a numeric with more than 38 decimal places fails the
 * call like validate_numeric_for_bigquery (bigquery/validation.rs:20-35: ETLG_UnsupportedValueInDestination, "Cell validation failed
 * for BigQuery compatibility", detail "Cell at index N failed validation", frame_index = the event). A json / jsonb cell is its
 * serde_json Display string (encoding.rs:173-176) behind validate_json_for_bigquery (validation.rs:47-85): an integer literal of the
 * parsed value outside u64 / i64 fails the call the same way; a cell that is not one JSON value fails it with ETLG_E_JSON. Array
 * cells (array_cell_encode_prost, encoding.rs:203-290): bool / int2 / int4 / oid / int8 / float4 / float8 / timestamptz packed; date /
 * time / timestamp / uuid, text-like, numeric, timetz and json elements one string field per element, bytea elements one bytes field;
 * an empty array nothing; a NULL element fails the call with ETLG_NullValuesNotSupportedInArrayInDestination (same description and
 * detail), a numeric element of more than 38 decimal places / a json element's integer outside u64 / i64 with
 * ETLG_UnsupportedValueInDestination (validate_elements, validation.rs:143-188). A literal the device cannot take apart (see
 * etlg_batch_rowbinary), DEFERRED cells and json cells beyond json_display's limits return ETLG_RB_NEEDS_HOST.
 * The result is an etlg_rowbinary (same view; n_rows can exceed the number of events).
 * A table-copy batch (etlg_copy_decode): one row per source row (row_event[i] = i), the cells under tags 1..n, then _CHANGE_TYPE =
 * "UPSERT" under tag n + 1 and NOTHING under n + 2 — write_table_rows appends only the change type (bigquery/core.rs:602-649; compare
 * bigquery_upsert_row :1410-1418, which pushes both). The validation rules are unchanged. */
int32_t etlg_batch_protobuf(etlg_ctx* ctx, etlg_batch* batch, int32_t schema_slot, uint32_t flags, etlg_rowbinary** out);
/* Snowflake Snowpipe Streaming rows for ONE schema slot: the NDJSON line serialize_row writes for every row the sink builds
 * (crates/etl-destinations/src/snowflake/encoding.rs:57-72; core.rs:345-438), in event order, at most one row per event, each line
 * serde_json's compact map followed by '\n':
 *   {"<col>":<value>,...,"_cdc_operation":"insert|update|delete","_cdc_sequence_number":"<commit_lsn:016x>/<tx_ordinal:016x>"}
 *   Insert -> every replicated column ("insert"); Update with a full new row -> the new row ("update"); Delete with a full old row ->
 *   every replicated column, with a key image -> the identity columns only, keyed by their names ("delete"). A partial Update and a
 *   Delete without an old row are left out and counted in n_host_rows (the host raises SourceReplicaIdentityError, :572-608).
 *   A table-copy batch (etlg_copy_decode) gives "insert" rows under the zero token 0000000000000000/0000000000000000 (:683-699).
 * col_names: the slot's replicated column names in slot order, each NUL-terminated, back to back; n_names must be the slot's n_cols
 * (ETLG_InvalidArgument otherwise). Keys and text values are escaped like serde_json (\" \\ \b \f \n \r \t, \u00xx for the other
 * bytes below 0x20, everything else raw). Values (CellSerializer :94-140): NULL null; bool; integers in decimal; float4 / float8 in
 * ryu's shortest form (serde_json serialize_f32 / _f64); numeric, date (%Y-%m-%d), time (%H:%M:%S%.f), timestamp, timestamptz
 * (%Y-%m-%d %H:%M:%S%.f+00:00), timetz, uuid (hyphenated lower case) and bytea (lower-case hex) as JSON strings; json / jsonb the value
 * itself, embedded; text-like cells JSON strings; arrays JSON arrays of the same (a NULL element is null).
 * A float that is NaN / +-inf, a numeric NaN / +-Infinity (cell or element) fails the call like Error::Encoding: ETLG_InvalidData,
 * description "Snowflake encoding error", detail "Encoding error: Snowflake does not support NaN/Infinity float values: NaN" (inf, -inf) /
 * "Encoding error: Snowflake NUMBER does not support NaN" / "... Infinity", frame_index = the event. A json cell or element that is not
 * one JSON value fails it with ETLG_E_JSON before anything else. Otherwise the first row in event order (its first column, an array's
 * first element) that fails or that the device cannot encode decides: DEFERRED cells, literals the array walkers do not take apart and
 * json beyond json_display's limits give status ETLG_RB_NEEDS_HOST (host_event / host_column). Typed array cells of a batch finished
 * with ETLG_F_FINISH_CELLS are written from their etlg_array_hdr. Flags: ETLG_F_OUTPUT_ON_DEVICE. Every row's bytes include its '\n'. */
int32_t etlg_batch_ndjson(etlg_ctx* ctx, etlg_batch* batch, int32_t schema_slot, const char* col_names, uint32_t n_names, uint32_t flags,
                          etlg_rowbinary** out);
/* DuckLake SQL literals for ONE schema slot: the text cell_to_sql_literal writes (crates/etl-destinations/src/ducklake/encoding.rs:
 * 366-612), which every row the DuckLake sink writes goes through. `what` picks the records, in event order, at most one per event per
 * call, with NO separator or terminator between them (row_offsets cut them):
 *   ETLG_DL_TUPLES      one "(lit, lit, ...)" per row the sink upserts (table_row_to_sql_literal_ref: hashed into the batch identity,
 *                       inserted as VALUES text): Insert -> the row; Update with a full new row -> the new row; a table-copy batch
 *                       (etlg_copy_decode) -> every row. A partial Update is counted in n_host_rows; Deletes give nothing. (The partial
 *                       Updates counted here are served by ETLG_DL_UPDATES.)
 *   ETLG_DL_PREDICATES  one `"col" = lit AND "col" IS NULL` per row image the sink deletes / matches by (delete_predicate_from_row,
 *                       batches.rs:1229-1316): Update / Delete -> from the old image (a full image: the cells at the identity columns'
 *                       positions; a key image: its cells), identity columns in slot order; an Update without an old image -> from the
 *                       new row's identity columns (TableMutation::Replace) unless that row is partial; a partial Update without an old
 *                       image and a Delete without one are counted in n_host_rows; Inserts give nothing. A table-copy batch -> every
 *                       row, over the PRIMARY-KEY columns (etlg_col.primary_key). A NULL key cell is `"col" IS NULL`. A slot without
 *                       identity columns: every Update / Delete is counted in n_host_rows (the host raises "DuckLake delete requires a
 *                       replica identity"); a copy batch without primary-key columns gives empty records. (The partial Updates
 *                       counted here are served by ETLG_DL_UPDATES.)
 *   ETLG_DL_UPDATES     every PARTIAL Update (a new row with unchanged-TOAST columns no old image completes), which the sink applies as
 *                       one `UPDATE ... SET <assignments> WHERE <predicate>` (ducklake/core.rs:1846-1913, batches.rs:1179-1190): TWO
 *                       consecutive records with the same row_event.
 *                       Record 2k, the SET clause: update_assignments_from_partial_row(...).join(", ") (batches.rs:1319-1399, 2125) —
 *                       `"col" = lit` for every column whose cell is not MISSING, in slot order; a NULL cell is `"col" = NULL`; the
 *                       literals are those of ETLG_DL_TUPLES.
 *                       Record 2k+1, the predicate of the mutation's delete_row, as ETLG_DL_PREDICATES writes it: from the old image (a
 *                       full image: the cells at the identity columns' positions; a key image: its cells); without an old image from
 *                       the partial new row's cells at the identity columns (key_row_from_updated_partial_row, core.rs:846-).
 *                       Counted in n_host_rows, without records (the host raises the reference's error at the first of them): a partial
 *                       Update of a slot without identity columns ("DuckLake update requires a replica identity"), one without an old
 *                       image whose identity column is MISSING ("DuckLake partial update is missing replica-identity columns") and one
 *                       with no present cell at all ("DuckLake partial update row has no assignments"). Inserts, Deletes, Updates with
 *                       a full new row and a table-copy batch give nothing and are NOT host rows for this `what`.
 *                       etlg_rowbinary_col_ends_get gives where the columns' pieces of every record end.
 * col_names: as for etlg_batch_ndjson (n_names must be the slot's n_cols, ETLG_InvalidArgument otherwise; so is an unknown `what`).
 * Names are quoted like quote_double_identifier (ducklake/sql.rs:10-12): '"' doubled, nothing else changed.
 * Values: NULL; TRUE / FALSE; integers in decimal; float8 as Rust's f64 Display (shortest digits, positional, never an exponent: 1,
 * -0, 0.1, 1e21 as 1 and 21 zeros; up to 327 bytes), float4 widened first (0.1f32 -> 0.10000000149011612), NaN / +-inf as
 * CAST('NaN' AS DOUBLE) / CAST('Infinity' AS DOUBLE) / CAST('-Infinity' AS DOUBLE) (AS FLOAT for float4) — values, not errors;
 * text-like cells, numeric and timetz Display through quote_literal; DATE '%Y-%m-%d'; TIME '%H:%M:%S%.6f';
 * TIMESTAMP '%Y-%m-%d %H:%M:%S%.6f'; TIMESTAMPTZ '...%.6f+00:00'; CAST('<hyphenated lower-case uuid>' AS UUID);
 * CAST(<quote_literal(serde_json Display)> AS JSON); from_hex('<UPPER-case hex>'); arrays [e, e, NULL] of the same ("[]" when empty),
 * from the source literal or from the etlg_array_hdr ETLG_F_FINISH_CELLS leaves.
 * quote_literal is pg_escape 0.1.1, RESTATED FROM THE CRATE'S DOCUMENTATION — its source is not vendored with the reference and the
 * reference's tests pin only the plain arm ('alice'): a ' is doubled; a text that holds a backslash has every backslash doubled and is
 * prefixed with a space and E (a\b -> " E'a\\b'" in C notation); otherwise plain '...'. The quote doubling and the backslash arm are
 * UNPINNED (one function on each side: dl_quote in rowformats.hip.h, quote_literal in tests/ducklake_literals.py).
 * Errors: a json cell or element that is not one JSON value fails the call with ETLG_E_JSON at its event before anything else; the sink
 * has no encoding error on this path. A DEFERRED scalar, an array literal the walkers do not take apart and json beyond json_display's
 * limits give status ETLG_RB_NEEDS_HOST with the first such event and column in event order; for ETLG_DL_PREDICATES only the key
 * columns are looked at; for ETLG_DL_UPDATES the SET record looks at every present column and the predicate record at its key columns,
 * and within an event the SET record's first such column is reported, else the predicate record's. Flags: ETLG_F_OUTPUT_ON_DEVICE. The result is an etlg_rowbinary (same view). */
#define ETLG_DL_TUPLES 0u
#define ETLG_DL_PREDICATES 1u
#define ETLG_DL_UPDATES 3u
int32_t etlg_batch_duckdb(etlg_ctx* ctx, etlg_batch* batch, int32_t schema_slot, int32_t what, const char* col_names, uint32_t n_names,
                          uint32_t flags, etlg_rowbinary** out);
int32_t etlg_rowbinary_view_get(const etlg_rowbinary* rb, etlg_rowbinary_view* out);
/* ETLG_DL_UPDATES only (any other object: ETLG_InvalidArgument): n_rows * n_cols u32 entries, on the host or the device like the
 * other arrays of the view, freed with the object. col_ends[r * n_cols + c] is the number of bytes of record r written once column c
 * is done; a column that contributes nothing (a MISSING cell, a column outside the key) repeats the previous value, or 0 in front.
 * Piece c of a record is (col_ends[c - 1], col_ends[c]) without its leading separator (", " / " AND "): the host rebuilds
 * Vec<String> assignments from the pieces and feeds hash_partial_table_row_ref (batches.rs:1562-1594) with (column index, literal),
 * the literal being the piece minus len(quoted name) + 3. An object without records (n_rows == 0, also one that came back as
 * ETLG_RB_NEEDS_HOST) gives ETLG_OK and a null pointer. */
int32_t etlg_rowbinary_col_ends_get(const etlg_rowbinary* rb, const uint32_t** col_ends);
void etlg_rowbinary_free(etlg_rowbinary* rb);

/* DuckLake batch identities for ONE schema slot, hashed on the device: the fingerprint of the `batch_id` every atomic batch of the sink
 * gets (build_mutation_batch_identity, crates/etl-destinations/src/ducklake/batches.rs:1402-1446; build_copy_batch_identity :1449-1464).
 * The fingerprint is BatchIdHasher (:260-289), FNV-1a-64: h = (h ^ byte) * 0x100000001b3 from 0xcbf29ce484222325, byte by byte over
 * every literal of every row of the batch — the texts etlg_batch_duckdb wrote. `tuples`, `predicates` and `updates` (may be NULL) are the
 * objects etlg_batch_duckdb returned for THIS batch and slot with ETLG_DL_TUPLES, ETLG_DL_PREDICATES and ETLG_DL_UPDATES, built with
 * ETLG_F_OUTPUT_ON_DEVICE and of status ETLG_RB_OK: their bytes are hashed where they lie, nothing is encoded again or downloaded.
 * out[i] (HOST, n_ranges entries) is the hasher's state after ranges[i].seed has absorbed the byte stream of the slot's Insert / Update /
 * Delete events with index in [first_event, end_event), in event order; events of other slots and of every other kind are skipped, an
 * empty range gives its seed. The host keeps what is cheap and serial: cutting the batch into atomic batches
 * (prepare_mutation_table_batches), the seed — the state after "mutation" or "copy" and table_name.id(), both hashed as strings — and the
 * format! of the id (build_batch_identity :1536-1553).
 * The byte stream restates Rust's Hash impls as the reference drives them through Hasher::write: a str / String is its bytes followed by
 * one 0xFF, a u64 / usize 8 little-endian bytes. Per event of a WAL batch: le64(start_lsn) le64(commit_lsn), then, with T the event's
 * ETLG_DL_TUPLES record and P its ETLG_DL_PREDICATES record:
 *   Insert                                                    "insert" FF T FF
 *   Delete                                                    "delete" FF P FF
 *   full Update with an old image (ETLG_OLD_FULL / _KEY)      "update" FF P FF T FF
 *   full Update without one (TableMutation::Replace)          "replace" FF P FF T FF
 *   partial Update (records 2k, 2k + 1 of `updates`)          "update" FF R(2k+1) FF le64(n_cols), then for every column c that is not
 *                                                             MISSING, in slot order: le64(c) lit_c FF — lit_c cut out of record 2k by
 *                                                             col_ends, minus the quoted name and " = " (hash_partial_table_row_ref,
 *                                                             :1562-1594; etlg_rowbinary_col_ends_get)
 * Per row of a table-copy batch: P FF T FF, P over the primary-key columns, no LSNs (:1458-1461).
 * col_names / n_names as for etlg_batch_duckdb (the quoted names' lengths cut the SET pieces).
 * A slot event inside a range that has no record where the table needs one — the events the reference refuses, which the three calls
 * count in n_host_rows, and a partial Update when `updates` is NULL — gives ETLG_OK with info->status ETLG_RB_NEEDS_HOST, host_event =
 * the first such event, and no fingerprint is written. ETLG_InvalidArgument: an object of another batch, slot or `what`, one on the
 * host or of status ETLG_RB_NEEDS_HOST; n_names other than the slot's column count; ranges that are not ascending and disjoint.
 * (An object names its batch by address and by a number every batch of the process gets once: an object that outlived its batch is
 * refused too, also when a later batch lies at the freed one's address.)
 * Batch requirements as for etlg_batch_columns. The call stops for the device once, at its end.
 * THE STREAM IS UNPINNED. The reference's tests (batches.rs:3290-3396) assert only that ids are equal or differ; no fingerprint is
 * written down anywhere as a number. Pinned are FNV-1a itself (the standard vectors "" cbf29ce484222325, "a" af63dc4c8601ec8c, "foobar"
 * 85944171f73967e8) and the records' bytes (the DuckLake tests). The interleaving above is restated in one function on each side —
 * fp_walk in etl_amd/csrc/fingerprint.hip, event_stream in tests/ducklake_identity.py — and a deployment that switches between
 * host-computed and device-computed ids across a restart depends on that restatement. */
typedef struct etlg_dl_range {
  uint64_t first_event; /* [first_event, end_event) in the batch's event order */
  uint64_t end_event;
  uint64_t seed;        /* the hasher's state the range starts from */
} etlg_dl_range;
typedef struct etlg_dl_fp_info {
  uint32_t status;      /* ETLG_RB_OK | ETLG_RB_NEEDS_HOST */
  uint32_t _pad;
  uint64_t host_event;  /* NEEDS_HOST: the first slot event inside a range that lacks a record; else ~0 */
} etlg_dl_fp_info;
int32_t etlg_ducklake_fingerprints(etlg_ctx* ctx, etlg_batch* batch, int32_t schema_slot, const etlg_rowbinary* tuples,
                                   const etlg_rowbinary* predicates, const etlg_rowbinary* updates, const char* col_names, uint32_t n_names,
                                   const etlg_dl_range* ranges, uint32_t n_ranges, uint64_t* out, etlg_dl_fp_info* info);

/* --------------------------------------------------------------- size hints */

/* Event::size_hint (crates/etl/src/event.rs:295-320) for every event of a batch, computed on the device from the
 * arena: what EventBatch::push adds up to decide batch cut points (replication/apply.rs:656-657, 1932-1935).
 * The estimate is built from `size_of::<T>()` of the reference's own types (data/table_row.rs:248-384), whose
 * layouts are not ABI-stable: the Rust shim fills this model once (crates/etl-gfx950/src/lib.rs).
 * What is tested: the reference holds no test that states a size hint as a number, so there is nothing to pin the FORMULA's
 * restatement to — tests/test_gpu_size_hints.py checks the device against oracle/size_hint.py, a second restatement of the same
 * reading of event.rs / table_row.rs by the same hands. That is self-consistency, not parity with the reference. */
typedef struct etlg_size_model {
  uint32_t begin_event;             /* size_of::<BeginEvent>() ... (event.rs:297-316) */
  uint32_t commit_event;
  uint32_t insert_event;
  uint32_t update_event;
  uint32_t delete_event;
  uint32_t truncate_event;
  uint32_t relation_event;
  uint32_t replicated_table_schema; /* per truncated table (event.rs:311-314) */
  uint32_t table_row;               /* size_of::<TableRow>()  (table_row.rs:249-251) */
  uint32_t cell;                    /* size_of::<Cell>(), times the row's Vec capacity: n_cols (codec/event.rs:567),
                                       n_ident for key rows (:800, :831) */
  uint32_t _reserved[2];
} etlg_size_model;

/* The event has a part only the host can size: a DEFERRED json / array / numeric cell (estimate_json_allocated_bytes /
 * estimate_array_allocated_bytes need the parsed value) or a Partial updated row (its Vec capacities depend on the
 * reserve/append sequence of codec/event.rs:636-660). The low bits hold everything else of the event. */
#define ETLG_SIZE_HINT_INCOMPLETE (1ull << 63)

/* out: n_events u64 entries; device memory when flags has ETLG_F_OUTPUT_ON_DEVICE, else host memory.
 * Same batch requirements as etlg_batch_columns. Per cell (estimate_cell_allocated_bytes, table_row.rs:276-299):
 * String -> len (str::to_owned), Bytes -> len (Vec::with_capacity(hex / 2), codec/hex.rs:21), Numeric::Value ->
 * 2 * ndigits (Vec::with_capacity(retained_groups), numeric.rs:444), everything fixed-width -> 0. */
int32_t etlg_batch_size_hints(etlg_ctx* ctx, etlg_batch* batch, const etlg_size_model* model, uint32_t flags,
                              uint64_t* out);

/* Where the apply loop cuts the event stream into write_events batches, found on the device: no hint comes back to the host.
 * The reference's rule: EventBatch::push adds event.size_hint() to a running size_hint_bytes (crates/etl/src/replication/apply.rs:656-657);
 * after every message the loop flushes when size_hint_bytes >= cached_batch_budget.current_batch_size_bytes() (:1932-1945); the flush takes
 * the batch and the next one starts at zero. Over the events [first, stop_event) of this batch:
 *     s = carry_in
 *     for i in first .. stop_event:
 *         s += hint[i]
 *         if s >= budget: emit cut i + 1 (the exclusive end of a write_events batch); s = 0
 *     carry_out = s
 * cuts_out receives the cuts, ascending event indexes. When n_cuts > cuts_cap the first cuts_cap cuts are written and n_cuts is the full
 * count: the caller resumes with first = cuts_out[cuts_cap - 1] and carry_in = 0. That is the contract, not an error. cuts_cap == 0 with
 * cuts_out == NULL only counts. With ETLG_F_OUTPUT_ON_DEVICE in `flags` cuts_out is device memory, else host memory.
 * hints == NULL: the library evaluates the hints itself (etlg_batch_size_hints' kernel) into pooled device memory; `model` is required.
 * hints != NULL: a DEVICE array of n_events entries in etlg_batch_size_hints' format; `model` may be NULL. This form is for tables with
 * json / array columns and for partial Updates: the host sizes the INCOMPLETE events, writes the completed values — bit 63 cleared —
 * into its device copy of the hints and calls again; without it every such table would come down to one call per event. The caller's
 * values are sizes of real events: like the library's, their sum over the range, plus carry_in, plus budget, stays below 2^64.
 * An event whose hint has ETLG_SIZE_HINT_INCOMPLETE stops the walk: stop_event is the first such event of [first, end) (else `end`), the
 * cuts are exact up to it, carry_out is the running sum there; the host adds that one event and resumes at stop_event + 1.
 * What only the host knows it says through the range and the carry: a forced flush after a Commit (end_batch, apply.rs:2337-2353) or at
 * the deadline ends the range there and starts the next one with carry_in = 0; a change of the budget (CachedBatchBudget refreshes at most
 * every 100 ms, runtime/batch_budget.rs:123-137) ends the range where it takes effect, and carry_out goes on as the next carry_in; the
 * sum left open by the previous decoded batch is the first range's carry_in.
 * Arguments: budget in [1, 2^62]; carry_in < budget (the reference would already have flushed otherwise); first <= end <= n_events; a
 * model or hints; anything else is ETLG_InvalidArgument. No sum can wrap: carry_in < budget <= 2^62, and a batch's hints are bounded by its
 * arena bytes plus the model's constants per column (u32 each), far below 2^62 — so the reference's saturating_add never saturates and
 * plain 64-bit adds are the rule.
 * Same batch requirements as etlg_batch_columns (device-resident, finished; an ASYNC batch is synced first).
 * The call stops for the device at most twice: once to learn stop_event and total — the host bounds the cuts by
 * min(stop_event - first, (carry_in + total) / budget), every closed batch summing to at least budget, and sizes the remaining launches
 * with that bound — and once at its end. A range that cannot hold a cut (the bound is 0, or first == end) ends at the first stop.
 * What is tested: the reference's tests state no cut position as a number; tests/batch_cuts.py restates the three lines above. */
typedef struct etlg_cuts_info {
  uint64_t n_cuts;      /* cuts the rule makes in [first, stop_event): may exceed cuts_cap */
  uint64_t stop_event;  /* first event of [first, end) whose hint has ETLG_SIZE_HINT_INCOMPLETE, else `end` */
  uint64_t carry_out;   /* size_hint_bytes of the batch left open at stop_event (behind the last cut) */
  uint64_t total;       /* sum of the hints of [first, stop_event) */
} etlg_cuts_info;

int32_t etlg_batch_cuts(etlg_ctx* ctx, etlg_batch* batch, const etlg_size_model* model, const uint64_t* hints,
                        uint64_t first, uint64_t end, uint64_t budget, uint64_t carry_in, uint32_t flags,
                        uint64_t* cuts_out, uint64_t cuts_cap, etlg_cuts_info* info);

/* rows_out[k] = the number of rows whose row_event < cuts[k] (a lower bound), for n_cuts cuts: where a hand-off object's rows are cut so
 * that every slice holds the rows of one write_events batch, without downloading row_event. row_event: the DEVICE row_event array (n_rows
 * entries, ascending) of any hand-off object — etlg_columns_view, the iceberg and ducklake-copy results, etlg_rowbinary_view of the
 * RowBinary / protobuf / NDJSON / DuckLake calls. Consecutive equal entries (BigQuery's DELETE + UPSERT pair of one event) fall on the
 * same side of a cut. `cuts` is device memory when cuts_on_device != 0, else host memory; rows_out is device memory with
 * ETLG_F_OUTPUT_ON_DEVICE in `flags`, else host memory. The call stops for the device once, at its end. */
int32_t etlg_cuts_locate(etlg_ctx* ctx, const uint64_t* cuts, uint64_t n_cuts, uint32_t cuts_on_device,
                         const uint64_t* row_event, uint64_t n_rows, uint32_t flags, uint64_t* rows_out);

/* Source payload accounting on the device: what the apply loop measures per row message and the seam's hand-off has no value for.
 * The reference builds StreamingPayloadMetadata::{insert,update,delete}(bytes) for every Insert / Update / Delete message it receives
 * (apply.rs:2459-2463, :2503-2507, :2547-2551) — bytes = the tuple value bytes of calculate_tuple_bytes (codec/event.rs:261-297), the
 * same number as etlg_batch_view.payload_bytes sums — and calls record_received() and record_row_size() on it BEFORE
 * should_apply_changes: the received side covers messages that yield no event. EventBatch::push then merges the metadata of the events
 * of one write_events batch (apply.rs:656-658) and record_processed() reports the merged value per kind once the write is acknowledged
 * (source_payload_metadata.rs:120-185): the delivered side covers events only. An operation present with 0 bytes is an observation
 * (Some(0) is not None): every sum comes with its row count, and rows[k] == 0 is the reference's None.
 *
 * buf / len / frame_offsets / nframes: the input the batch was decoded from (ETLG_F_INPUT_ON_DEVICE in `flags`: device memory). A
 * caller that decoded without a sidecar passes the offsets etlg_scan_boundaries returns. For a batch of etlg_copy_decode: the rows and
 * row_offsets; event i is row i, its bytes are row_offsets[i + 1] - row_offsets[i] (TableCopyPayloadMetadata, table_copy.rs:84), and
 * everything is reported under ETLG_PK_COPY.
 * Received side, over the frames [0, view.n_frames): info->received_bytes / received_rows per kind, and hist_out (optional, host
 * memory): hist_out[k * (n_bounds + 1) + j] = the messages of kind k with hist_bounds[j - 1] < bytes <= hist_bounds[j], the last entry
 * of each kind being the overflow bucket — Prometheus `le` buckets, not cumulated. The buckets are the exporter's, not the reference's:
 * hist_bounds is host memory, strictly ascending, n_bounds <= 64. received_bytes[0..3) equals view.payload_bytes in every case: when
 * the batch ended in an error that was raised after the failing message had recorded its metrics, that message counts here as there.
 * received_bytes[ETLG_PK_COPY] equals view.payload_bytes[0] of a table-copy batch.
 * Delivered side, over the batch's events: ev_bytes_out (optional, n_events entries) = the value bytes of each event's message, 0 for
 * Begin / Commit / Relation / Truncate; sums_out (optional, n_cuts + 1 entries) = bytes and rows per kind of the events
 * [cuts[k - 1], cuts[k]), the first range from 0, the last up to n_events. `cuts`: as etlg_batch_cuts writes them (device memory when
 * cuts_on_device != 0, else host memory), ascending, none above n_events; NULL / 0: one range. Both outputs are device memory with
 * ETLG_F_OUTPUT_ON_DEVICE in `flags`, else host memory. Sums are plain 64-bit adds: the reference merges with saturating_add, which
 * cannot differ below 2^64, and a batch holds fewer than 2^32 value bytes per message and fewer than 2^30 messages. Merging the
 * sums of several decoded batches is the caller's, and there saturating.
 * How an event finds its message: every Begin / Relation / Insert / Update / Delete / Truncate / Commit frame takes the transaction's
 * next ordinal, whether or not it yields an event (next_tx_ordinal() runs before the ownership test), and no other frame does. So the
 * frame of an event is the (r + ev_tx_ordinal)-th such frame of the batch, r being the rank of the Begin frame that opened its
 * transaction — a Begin always yields an event, so the j-th 'B' event is the j-th Begin frame — and for the events in front of the
 * batch's first Begin it is the (ev_tx_ordinal - the ordinal the batch started from)-th.
 * The call never reads outside [buf, buf + len): a frame whose offsets do not lie inside it is not looked at. An event whose frame
 * does not parse or does not carry the event's kind — other bytes than the batch was decoded from — gives ETLG_OK with info->status
 * ETLG_PM_MISMATCH and mismatch_event, and then no delivered value is to be trusted.
 * ETLG_InvalidArgument: a batch of another context, one that is not finished or not device-resident (an ASYNC batch is synced first;
 * a batch that ended in a decode error is accepted: its events are delivered); frame_offsets == NULL; nframes < view.n_frames;
 * n_bounds > 64 or bounds that are not strictly ascending; cuts that are not ascending or pass n_events.
 * The call stops for the device once, at its end. */
enum { ETLG_PK_INSERT = 0, ETLG_PK_UPDATE = 1, ETLG_PK_DELETE = 2, ETLG_PK_COPY = 3 };
#define ETLG_PM_OK 0u
#define ETLG_PM_MISMATCH 1u

typedef struct etlg_payload_sums {
  uint64_t bytes[4];  /* per ETLG_PK_* */
  uint64_t rows[4];   /* rows[k] == 0 <=> Option::None */
} etlg_payload_sums;

typedef struct etlg_payload_info {
  uint64_t received_bytes[4];  /* every row message of frames [0, view.n_frames), per ETLG_PK_* */
  uint64_t received_rows[4];
  uint64_t n_ranges;           /* n_cuts + 1 */
  int32_t status;              /* ETLG_PM_OK | ETLG_PM_MISMATCH */
  uint32_t _pad;
  uint64_t mismatch_event;     /* first event whose joined frame does not carry its kind, ~0 if none */
} etlg_payload_info;

int32_t etlg_batch_payload(etlg_ctx* ctx, etlg_batch* batch, const uint8_t* buf, size_t len, const uint32_t* frame_offsets,
                           size_t nframes, const uint64_t* cuts, uint64_t n_cuts, uint32_t cuts_on_device,
                           const uint64_t* hist_bounds, uint32_t n_bounds, uint32_t flags, uint32_t* ev_bytes_out,
                           etlg_payload_sums* sums_out, uint64_t* hist_out, etlg_payload_info* info);

/* The pass plan of a destination's write_events loop, built on the device: what a driver that holds only device hand-offs needs to run
 * the loop all five sinks share (etl-destinations: clickhouse/core.rs:1063-1164, bigquery/core.rs:956-1100, snowflake/core.rs:262-335,
 * ducklake/core.rs:1815-2060, iceberg/core.rs:300-430) without downloading ev_kind / ev_flags / ev_schema_slot / ev_table_id. One pass of
 * that loop collects Insert / Update / Delete rows per table until the next Relation or Truncate event, writes those tables, handles the
 * run of Relation events, then the run of Truncate events, and starts over while events are left.
 * Window and ranges: events [first, end), first <= end <= n_events. `cuts` (n_cuts entries; device memory when cuts_on_device != 0,
 * else host memory) are the exclusive range ends etlg_batch_cuts wrote: ascending, each in [first, end]. Every cut closes one
 * write_events range; a last range runs to `end` when the last cut is below `end`; n_cuts == 0 is one range. Equal neighbouring cuts,
 * or a cut equal to `first`, make an empty range: it is counted (in `range` and n_ranges) and has no pass — the reference's
 * `while event_iter.peek().is_some()` does nothing for it. The device checks the cuts: one outside [first, end] or below its
 * predecessor gives ETLG_OK with info->status = ETLG_OL_BAD_CUTS, info->bad_cut = the index of the first such cut, and nothing else
 * written anywhere.
 * THE PASS RULE. The class of an event is 2 for 'T', 1 for 'R' — 0 with ETLG_OL_RELATIONS_INLINE in `opts`: Iceberg's loop breaks at
 * Truncate only and meets Relation events inside the data run (iceberg/core.rs:310-312, :360) —, and 0 for everything else (B, C, I,
 * U, D). A pass starts at the first event of every non-empty range and at every event whose class is lower than its predecessor's.
 * Inside a pass the classes therefore never fall: data_end is the pass's first event of class >= 1 (the pass end if it has none) and
 * rel_end its first event of class 2 (the pass end if it has none): rows are the I / U / D events of [first_event, data_end), the
 * Relation run is [data_end, rel_end), the Truncate run [rel_end, end_event).
 * Outputs: device memory with ETLG_F_OUTPUT_ON_DEVICE in `flags`, else host memory, filled before the call returns; any of them may
 * be NULL and its part is skipped. With P = min(n_passes, passes_cap) and W = (view.n_slots + 63) / 64:
 *   passes_out[p], p < P   the pass; `range` = the index of its write_events range (empty ranges counted); trunc_first / n_trunc = its
 *                          entries of trunc_out, counted over all entries, those beyond trunc_cap included.
 *   ends_out[p], p < P     end_event again, as plain words: the shape etlg_cuts_locate takes as `cuts`, so that the passes become row
 *                          positions of any hand-off object's row_event.
 *   touched_out[p * W + s / 64], p < P   bit s % 64 is set iff pass p holds at least one I / U / D event of slot s — the keys of the
 *                          loop's `pending` map. Every word of the P passes is written, zero when no bit is set.
 *   trunc_out[k], k < min(n_trunc, trunc_cap)   one entry per {table_id, schema_slot} pair in the body of every Truncate event of the
 *                          window, in event order, then body order. Not de-duplicated: the host keeps the first entry per table_id of a
 *                          pass, as truncate_schemas.entry(id).or_insert(schema) does (clickhouse/core.rs:1148-1155). A Truncate that
 *                          names no table this worker owns has no entry.
 *   slots_out[s], s < view.n_slots   the census of the whole window per category: 0 Insert, 1 Update with a full new row, 2 Update
 *                          with ETLG_FLAG_PARTIAL, 3 Delete ETLG_OLD_FULL, 4 Delete ETLG_OLD_KEY, 5 Delete ETLG_OLD_NONE. rows[k] =
 *                          events of the category, first[k] = the lowest event index of it, ~0 when there is none. It tells which
 *                          slots to hand off at all, and the lowest event over all tables that a sink refuses, before anything is
 *                          written.
 * The caps are the caller's: n_passes and n_trunc are the full counts and may exceed them; nothing is written at or beyond a cap, and
 * the caller calls again with larger buffers. passes_cap counts passes for passes_out, ends_out and touched_out alike.
 * Same batch requirements as etlg_batch_cuts (device-resident, finished; an ASYNC batch is synced first, and one that ended in a decode
 * error gives that error).
 * ETLG_InvalidArgument: a batch that is not device-resident, a batch of etlg_copy_decode (write_table_rows has no passes), first > end
 * or end > n_events, n_cuts without cuts or above 2^38. The call stops for the device once, at its end.
 * What is tested: the reference's tests state no pass boundary as a number; tests/batch_outline.py restates the loop above. */
#define ETLG_OL_RELATIONS_INLINE 1u
#define ETLG_OL_OK 0u
#define ETLG_OL_BAD_CUTS 1u

typedef struct etlg_outline_pass {
  uint64_t first_event;
  uint64_t data_end;     /* first event of class >= 1, else end_event */
  uint64_t rel_end;      /* first event of class 2, else end_event */
  uint64_t end_event;    /* exclusive */
  uint64_t range;        /* index of the write_events range */
  uint64_t trunc_first;  /* first entry of trunc_out */
  uint64_t n_trunc;
} etlg_outline_pass;

typedef struct etlg_outline_trunc {
  uint32_t table_id;
  uint32_t schema_slot;
  uint64_t event;
} etlg_outline_trunc;

typedef struct etlg_outline_slot {
  uint64_t rows[6];
  uint64_t first[6];     /* ~0: none */
} etlg_outline_slot;

typedef struct etlg_outline_info {
  uint64_t n_passes;     /* may exceed passes_cap */
  uint64_t n_trunc;      /* may exceed trunc_cap */
  uint64_t n_relations;  /* 'R' events of the window */
  uint64_t n_rows;       /* I / U / D events of the window */
  uint64_t n_ranges;     /* write_events ranges, empty ones included */
  uint64_t bad_cut;      /* ETLG_OL_BAD_CUTS: index of the first bad cut */
  uint32_t status;       /* ETLG_OL_OK | ETLG_OL_BAD_CUTS */
  uint32_t _pad;
} etlg_outline_info;

int32_t etlg_batch_outline(etlg_ctx* ctx, etlg_batch* batch, uint64_t first, uint64_t end, const uint64_t* cuts, uint64_t n_cuts,
                           uint32_t cuts_on_device, uint32_t opts, uint32_t flags, etlg_outline_pass* passes_out, uint64_t* ends_out,
                           uint64_t* touched_out, uint64_t passes_cap, etlg_outline_trunc* trunc_out, uint64_t trunc_cap,
                           etlg_outline_slot* slots_out, etlg_outline_info* info);

/* The DuckLake sink's atomic batches of ONE schema slot, cut on the device: the step between etlg_batch_outline and
 * etlg_ducklake_fingerprints — the replay filter (retain_mutations_after_sequence_key, etl-destinations ducklake/batches.rs:932-946), the
 * cut into atomic batches with their identity fields (prepare_mutation_table_batches :727-758, push_prepared_mutation_batch :1091-1125)
 * and the grouping of a batch's mutations into the DuckDB operations the sink executes (prepare_table_mutations :1128-1226) — without
 * downloading ev_kind / ev_flags / ev_schema_slot / ev_start_lsn / ev_commit_lsn / ev_tx_ordinal.
 * Windows: `passes` (n_passes entries; device memory when passes_on_device != 0, else host memory) are the passes etlg_batch_outline
 * wrote, of which only [first_event, data_end) is read: one window is one segment of the reference, the rows write_events_inner
 * (ducklake/core.rs:1815-1947) collects per table before a Relation or Truncate. Windows ascend and do not overlap; an empty window is
 * allowed.
 * MEMBERS of a window: its Insert / Update / Delete events with ev_schema_slot == schema_slot. Category (ETLG_DLP_CAT_*): Insert;
 * UPDATE_FULL = Update with ETLG_OLD_FULL / _KEY and a full new row; REPLACE = Update with ETLG_OLD_NONE and a full new row;
 * UPDATE_PARTIAL = Update with ETLG_FLAG_PARTIAL, any old image; DELETE = Delete.
 * REFUSED members (before the replay filter, as in the reference): an Update / Delete of a slot with n_ident == 0
 * (ETLG_DLP_R_UPDATE_IDENTITY "DuckLake update requires a replica identity", ETLG_DLP_R_DELETE_IDENTITY "DuckLake delete requires a
 * replica identity"; core.rs:371-392), else a Delete with ETLG_OLD_NONE (ETLG_DLP_R_DELETE_NO_OLD "DuckLake delete requires an old row
 * image", :1919-1929).
 * REPLAY FILTER: with has_watermark != 0 a member is retained iff (ev_commit_lsn, ev_tx_ordinal) > (wm_commit_lsn, wm_tx_ordinal),
 * lexicographically (compare_sequence_keys :1012-1015); otherwise every member is retained.
 * ATOMIC BATCHES: per window the retained members in event order, in consecutive groups of 16 (CDC_MUTATION_BATCH_SIZE, :79); the last
 * group of a window may be shorter; no group spans two windows.
 * OPERATIONS of a group, in member order: a maximal run of INSERTs is one UPSERT op of n rows; a maximal run of DELETEs one DELETE op
 * of n predicates, origin "delete"; every UPDATE_FULL a DELETE op (origin "update", 1 predicate) then an UPSERT op of 1 row; every
 * REPLACE the same with origin "replace"; every UPDATE_PARTIAL one UPDATE op. An Insert directly behind an Update's own UPSERT op
 * starts a new UPSERT op (the reference does not merge them, :3168-3233). A group has at most 32 ops.
 * `tuples` / `predicates` / `updates`: the objects etlg_batch_duckdb built for this batch and slot, checked as
 * etlg_ducklake_fingerprints checks them (ETLG_InvalidArgument otherwise); each may be NULL.
 * Outputs: device memory with ETLG_F_OUTPUT_ON_DEVICE in `flags`, else host memory; any may be NULL and its part is skipped.
 *   ranges_out[b], b < min(n_batches, batches_cap)    {first_event, end_event, seed}: what etlg_ducklake_fingerprints takes as `ranges`.
 *   batches_out[b], same b                            the group; op_first / n_ops index ops_out, counted over all ops, those beyond
 *                                                     ops_cap included.
 *   ops_out[k], k < min(n_ops, ops_cap)               the op. rec_first is the index of its first record in the object of its kind — an
 *                                                     UPSERT op's in `tuples`, a DELETE op's in `predicates`, an UPDATE op's in `updates`
 *                                                     (its SET record 2k; 2k + 1 is its predicate) —, the lower bound of first_event in
 *                                                     that object's row_event; the op's n records follow it without a gap. ~0 when the
 *                                                     object is NULL.
 * info gives the full n_batches, n_ops, n_members, n_retained and n_dropped; nothing is written at or beyond a cap, caps of 0 only count.
 * info->status, the first that applies; for every status but ETLG_DLP_OK NO output array is touched and the counts are 0:
 *   ETLG_DLP_BAD_PASSES  a window with first_event > data_end, data_end > n_events, or first_event below its predecessor's data_end;
 *                        info->bad_pass = the lowest such index.
 *   ETLG_DLP_REFUSED     info->event = the lowest refused member inside a window, info->reason = ETLG_DLP_R_*. The reference fails the
 *                        whole write_events at the first such event over all tables: the host takes the minimum over the slots it plans.
 *   ETLG_DLP_NOT_PREFIX  info->event = the lowest dropped member that follows a retained member of its window. Keys ascend in a
 *                        replication stream, so this should not occur; a range [first_event, end_event) would otherwise cover an event
 *                        the fingerprint must not absorb.
 *   ETLG_DLP_NEEDS_HOST  info->event = the lowest retained member whose record is missing from an object that was given (the events the
 *                        hand-off calls counted in n_host_rows). A NULL object is no error; a partial Update with updates == NULL is
 *                        reported by etlg_ducklake_fingerprints.
 * ETLG_InvalidArgument: a batch of etlg_copy_decode (prepare_copy_table_batch makes one batch of all rows), a batch that is not
 * device-resident (an ASYNC batch is synced first; one that ended in a decode error gives that error), an unknown slot, n_passes > 0
 * without passes, n_passes or n_events above 2^38. The call stops for the device once, at its end.
 * What is tested: tests/golden/ducklake_plan_kats.json transcribes the reference's own vectors (batches.rs:2893-3272);
 * tests/ducklake_plan.py restates the three loops. */
#define ETLG_DLP_OK 0u
#define ETLG_DLP_BAD_PASSES 1u
#define ETLG_DLP_REFUSED 2u
#define ETLG_DLP_NOT_PREFIX 3u
#define ETLG_DLP_NEEDS_HOST 4u
#define ETLG_DLP_R_UPDATE_IDENTITY 1u
#define ETLG_DLP_R_DELETE_IDENTITY 2u
#define ETLG_DLP_R_DELETE_NO_OLD 3u
#define ETLG_DLP_CAT_INSERT 0u
#define ETLG_DLP_CAT_UPDATE_FULL 1u
#define ETLG_DLP_CAT_REPLACE 2u
#define ETLG_DLP_CAT_UPDATE_PARTIAL 3u
#define ETLG_DLP_CAT_DELETE 4u
#define ETLG_DLP_OP_UPSERT 0u
#define ETLG_DLP_OP_DELETE 1u
#define ETLG_DLP_OP_UPDATE 2u
#define ETLG_DLP_ORIGIN_NONE 0u
#define ETLG_DLP_ORIGIN_DELETE 1u
#define ETLG_DLP_ORIGIN_UPDATE 2u
#define ETLG_DLP_ORIGIN_REPLACE 3u

typedef struct etlg_dl_batch {
  uint64_t first_event;       /* the first member */
  uint64_t end_event;         /* the last member + 1 */
  uint64_t first_start_lsn;   /* the first member's ev_start_lsn */
  uint64_t last_commit_lsn;   /* the last member's ev_commit_lsn: with last_tx_ordinal the last sequence key */
  uint64_t first_commit_lsn;  /* with first_tx_ordinal the first sequence key */
  uint64_t first_tx_ordinal;
  uint64_t last_tx_ordinal;
  uint64_t window;            /* index into `passes` */
  uint64_t op_first;          /* first entry of ops_out */
  uint32_t n_members;         /* 1 .. 16 */
  uint32_t n_ops;             /* 1 .. 32 */
  uint32_t n_cat[5];          /* members per ETLG_DLP_CAT_* */
  uint32_t _pad;
} etlg_dl_batch;

typedef struct etlg_dl_op {
  uint32_t kind;              /* ETLG_DLP_OP_* */
  uint32_t origin;            /* ETLG_DLP_ORIGIN_*: of a DELETE op */
  uint64_t first_event;       /* the op's first member */
  uint64_t n;                 /* rows / predicates; 1 for UPDATE */
  uint64_t rec_first;         /* ~0: the object is NULL */
} etlg_dl_op;

typedef struct etlg_dl_plan_info {
  uint64_t n_batches;         /* may exceed batches_cap */
  uint64_t n_ops;             /* may exceed ops_cap */
  uint64_t n_members;
  uint64_t n_retained;
  uint64_t n_dropped;         /* n_members - n_retained */
  uint64_t event;             /* REFUSED / NOT_PREFIX / NEEDS_HOST: the lowest such event */
  uint64_t bad_pass;          /* BAD_PASSES: the lowest such window */
  uint32_t status;            /* ETLG_DLP_* */
  uint32_t reason;            /* REFUSED: ETLG_DLP_R_* */
} etlg_dl_plan_info;

int32_t etlg_ducklake_plan(etlg_ctx* ctx, etlg_batch* batch, int32_t schema_slot, const etlg_outline_pass* passes, uint64_t n_passes,
                           uint32_t passes_on_device, uint32_t has_watermark, uint64_t wm_commit_lsn, uint64_t wm_tx_ordinal, uint64_t seed,
                           const etlg_rowbinary* tuples, const etlg_rowbinary* predicates, const etlg_rowbinary* updates, uint32_t flags,
                           etlg_dl_range* ranges_out, etlg_dl_batch* batches_out, uint64_t batches_cap, etlg_dl_op* ops_out,
                           uint64_t ops_cap, etlg_dl_plan_info* info);

/* The Snowflake sink's row batches of ONE schema slot, planned on the device: the step between etlg_batch_ndjson and the sink's
 * requests — what the three encode_* functions (etl-destinations snowflake/core.rs:345-438) and RowBatchBuilder::push_row
 * (snowflake/streaming/batch.rs:150-189) decide per row — without downloading row_offsets / row_event / ev_kind / ev_flags /
 * ev_schema_slot / ev_commit_lsn / ev_tx_ordinal. The zstd stream, the split into a new request at 3.8 MB of compressed output and
 * the 4 MB check stay the host's; the plan tells it where to look: once per segment of about flush_bytes, not once per row.
 * Windows: `passes` as in etlg_ducklake_plan — only [first_event, data_end) of each is read; windows ascend, do not overlap and may be
 * empty. One window is the rows accumulate_data_events (core.rs:279-303) gives one table's fresh RowBatchBuilder before a Relation or
 * Truncate.
 * MEMBERS of a window: its Insert / Update / Delete events with ev_schema_slot == schema_slot.
 * `ndjson`: the object etlg_batch_ndjson built for this batch and slot; required, device-resident (ETLG_F_OUTPUT_ON_DEVICE), of status
 * ETLG_RB_OK or ETLG_RB_NEEDS_HOST; anything else — NULL, a host-resident object, another call's, batch's or slot's object — is
 * ETLG_InvalidArgument.
 * FILTER: with has_committed != 0 a member is retained iff (ev_commit_lsn, ev_tx_ordinal) > (c_commit_lsn, c_tx_ordinal),
 * lexicographically: the channel has committed an offset iff committed_offset >= offset (streaming/channel.rs:175-177), and the tokens
 * `{commit_lsn:016x}/{tx_ordinal:016x}` (streaming/offset_token.rs:21-23) order as the pairs do. Otherwise every member is retained.
 * FAILING members, in the reference's order: an Update with ETLG_FLAG_PARTIAL fails whether or not it is retained
 * (ETLG_SFP_R_PARTIAL_UPDATE: snowflake_update_row :572-588 runs before the offset test in encode_update :372-394); a RETAINED Delete
 * with ETLG_OLD_NONE fails (ETLG_SFP_R_DELETE_NO_OLD: encode_delete :396-438 tests the offset first, then snowflake_delete_row
 * :591-608); a retained member whose NDJSON row is longer than max_row_bytes fails (ETLG_SFP_R_ROW_TOO_LARGE: strictly longer, as
 * batch.rs:160; info->row_bytes is its length, '\n' included, for the reference's message).
 * SEGMENTS: per window, s = 0, and for its retained rows in order, len = the row's bytes with its '\n':
 *     if s + len >= flush_bytes: a segment starts at this row with flush_before = 1; s = 0
 *     (the window's first retained row starts a segment in any case; its flush_before is 1 only if the line above fired)
 *     s += len
 * — push_row's `input_since_flush + len >= MAX_UNFLUSHED_BYTES` (batch.rs:166-180). Per segment the host does one flush when
 * flush_before != 0, with first_row_bytes added to compressed_size() for the split (batch.rs:175), one write_all of
 * bytes[byte_first, byte_end) of `ndjson` — a segment's rows are consecutive rows of it — and one extend of the offset range by the
 * two tokens. No segment spans two windows. flush_bytes must lie in [1, 2^32] and max_row_bytes be >= 1; the reference's values are
 * the two constants below.
 * A table-copy batch (etlg_copy_decode; core.rs:683-701 uses the same builder with the zero token): n_passes == 0 with passes == NULL
 * means one window over all rows, has_committed must be 0 (ETLG_InvalidArgument otherwise), every key is (0, 0), and first_event /
 * last_event are row indexes.
 * Outputs: device memory with ETLG_F_OUTPUT_ON_DEVICE in `flags`, else host memory; each may be NULL and is then skipped.
 *   segs_out[k], k < min(n_segs, segs_cap)   the segment; nothing is written at or beyond the cap, segs_cap == 0 only counts,
 *                                            info->n_segs is the full count.
 *   windows_out[w], every pass               seg_first / n_segs count all segments, those beyond segs_cap included; first_row /
 *                                            end_row are the window's retained rows in `ndjson` (a window without one has
 *                                            first_row == end_row == the rows of `ndjson` in front of data_end).
 * info->status, the first that applies; for every status but ETLG_SFP_OK NO output array is touched and the counts are 0:
 *   ETLG_SFP_BAD_PASSES  as ETLG_DLP_BAD_PASSES; info->bad_pass = the lowest such index.
 *   ETLG_SFP_FAILED      info->event = the lowest failing member inside a window, whatever its reason; info->reason = ETLG_SFP_R_*;
 *                        info->row_bytes for ROW_TOO_LARGE. The reference fails the whole call at the first such event over all
 *                        tables: the host takes the minimum over the slots it plans.
 *   ETLG_SFP_NOT_PREFIX  info->event = the lowest dropped member that follows a retained member of its window (offsets ascend in a
 *                        replication stream, so this should not occur; a segment's byte range would otherwise cover a dropped row).
 *   ETLG_SFP_NEEDS_HOST  `ndjson` has status ETLG_RB_NEEDS_HOST: info->event = its host_event; or a retained member that does not
 *                        fail has no row in `ndjson`: info->event = the lowest such member.
 * ETLG_InvalidArgument also: an unknown slot, a batch that is not device-resident (an ASYNC batch is synced first; one that ended in
 * a decode error gives that error), n_passes > 0 without passes, flush_bytes or max_row_bytes out of range, n_passes or n_events above
 * 2^38, and an `ndjson` of 2^32 - 16 rows or more (the jump tables index rows with 32 bits, as etlg_batch_cuts' do events).
 * A stated difference from the reference: etlg_batch_ndjson runs before any filter, so an encoding error (NaN, Infinity) fails it even
 * in a row this call's filter would drop, where the reference never encodes that row.
 * The call stops for the device once, at its end: the jump tables and the segment bound are sized from the object's n_rows and
 * n_bytes, which the host holds.
 * What is tested: the reference's tests state no flush position as a number (batch.rs:272-373 assert row counts, offsets and the
 * oversize error); tests/snowflake_plan.py restates encode_* and push_row as one sequential loop and
 * tests/test_gpu_snowflake_plan.py compares every field with it. */
#define ETLG_SF_MAX_UNFLUSHED_BYTES 131072ull /* MAX_UNFLUSHED_BYTES, batch.rs:26 */
#define ETLG_SF_MAX_ROW_BYTES 2097152ull      /* MAX_UNCOMPRESSED_ROW_BYTES, batch.rs:31 */
#define ETLG_SFP_OK 0u
#define ETLG_SFP_BAD_PASSES 1u
#define ETLG_SFP_FAILED 2u
#define ETLG_SFP_NOT_PREFIX 3u
#define ETLG_SFP_NEEDS_HOST 4u
#define ETLG_SFP_R_PARTIAL_UPDATE 1u
#define ETLG_SFP_R_DELETE_NO_OLD 2u
#define ETLG_SFP_R_ROW_TOO_LARGE 3u

typedef struct etlg_sf_segment {
  uint64_t window;            /* index into `passes` */
  uint64_t first_row;         /* rows [first_row, end_row) of `ndjson` */
  uint64_t end_row;
  uint64_t first_event;       /* the first row's event */
  uint64_t last_event;        /* the last row's event */
  uint64_t byte_first;        /* bytes [byte_first, byte_end) of `ndjson` */
  uint64_t byte_end;
  uint64_t first_row_bytes;   /* what the host adds to compressed_size() at batch.rs:175 */
  uint64_t first_commit_lsn;  /* with first_tx_ordinal the first token of OffsetRange */
  uint64_t first_tx_ordinal;
  uint64_t last_commit_lsn;   /* with last_tx_ordinal the last token */
  uint64_t last_tx_ordinal;
  uint32_t flush_before;      /* 1: the encoder is flushed (and the split decided) before this segment's first row */
  uint32_t _pad;
} etlg_sf_segment;

typedef struct etlg_sf_window {
  uint64_t seg_first;         /* first entry of segs_out */
  uint64_t n_segs;
  uint64_t first_row;         /* the retained rows [first_row, end_row) of `ndjson` */
  uint64_t end_row;
  uint64_t n_members;
  uint64_t n_retained;
  uint64_t n_bytes;           /* bytes of the retained rows */
} etlg_sf_window;

typedef struct etlg_sf_plan_info {
  uint64_t n_segs;            /* may exceed segs_cap */
  uint64_t n_members;
  uint64_t n_retained;
  uint64_t n_dropped;         /* n_members - n_retained */
  uint64_t n_rows;            /* rows in segments (== n_retained) */
  uint64_t n_bytes;           /* their bytes */
  uint64_t event;             /* FAILED / NOT_PREFIX / NEEDS_HOST: the event; else ~0 */
  uint64_t row_bytes;         /* FAILED with ETLG_SFP_R_ROW_TOO_LARGE: the row's length */
  uint64_t bad_pass;          /* BAD_PASSES: the lowest such window; else ~0 */
  uint32_t status;            /* ETLG_SFP_* */
  uint32_t reason;            /* FAILED: ETLG_SFP_R_* */
} etlg_sf_plan_info;

int32_t etlg_snowflake_plan(etlg_ctx* ctx, etlg_batch* batch, int32_t schema_slot, const etlg_outline_pass* passes, uint64_t n_passes,
                            uint32_t passes_on_device, uint32_t has_committed, uint64_t c_commit_lsn, uint64_t c_tx_ordinal,
                            const etlg_rowbinary* ndjson, uint64_t flush_bytes, uint64_t max_row_bytes, uint32_t flags,
                            etlg_sf_segment* segs_out, uint64_t segs_cap, etlg_sf_window* windows_out, etlg_sf_plan_info* info);

/* The ClickHouse sink's INSERT statements of ONE schema slot, cut on the device: the step between etlg_batch_rowbinary and the sink's
 * requests — where write_events_inner (etl-destinations clickhouse/core.rs:1063-1225) refuses an event and where insert_rows
 * (clickhouse/client.rs:565-649) opens and commits each statement — without downloading row_offsets / row_event / ev_kind / ev_flags /
 * ev_schema_slot. Shaped after etlg_snowflake_plan above.
 * Windows: `passes` as in etlg_snowflake_plan — only [first_event, data_end) of each is read; windows ascend, do not overlap and may be
 * empty. One window is the rows one pass of write_events_inner gathers for one table until a Relation or Truncate (core.rs:1066-1136)
 * and flush_pending_rows (:1172-1225) hands to one insert_rows call.
 * MEMBERS of a window: its Insert / Update / Delete events with ev_schema_slot == schema_slot. The sink has no replay filter: every
 * member is retained.
 * `rowbinary`: the object etlg_batch_rowbinary built for this batch and slot; required, device-resident (ETLG_F_OUTPUT_ON_DEVICE), of
 * status ETLG_RB_OK or ETLG_RB_NEEDS_HOST; anything else — NULL, a host-resident object, a protobuf, NDJSON or DuckLake object, another
 * batch's or slot's object — is ETLG_InvalidArgument. The ENGINE is the one the object was built for; it is not an argument.
 * FAILING members, raised at the event, in event order, before the pass is flushed; per event the reference's order of tests:
 *   ETLG_CHP_R_PARTIAL_UPDATE   an Update with ETLG_FLAG_PARTIAL, both engines (clickhouse_update_row :1364-1375);
 *   ETLG_CHP_R_UPDATE_IDENTITY  a full Update under ETLG_CH_REPLACING_MERGE_TREE on a slot whose replica identity is neither PrimaryKey
 *                               nor Full (:1377-1379, ensure_clickhouse_key_identity_is_primary_key :1404-1427);
 *   ETLG_CHP_R_DELETE_NO_OLD    a Delete with ETLG_OLD_NONE, both engines (clickhouse_delete_old_row :1385-1400);
 *   ETLG_CHP_R_KEY_WIDTH        a Delete with ETLG_OLD_KEY on a slot whose identity column count differs from its primary-key column
 *                               count, both engines (expand_key_row :1437-1450 tests the width first);
 *   ETLG_CHP_R_KEY_IDENTITY     a Delete with ETLG_OLD_KEY, widths agree, identity neither PrimaryKey nor Full, both engines (:1452).
 * STATEMENTS: per window, over its rows in order (every member has one row), insert_rows' loop (client.rs:578-600):
 *     while rows remain: a statement opens; bytes = 0; while bytes < max_bytes_per_insert and rows remain: take a row, bytes += its
 *     RowBinary length; the statement is committed
 * — a statement closes behind the first row that brings its bytes to max_bytes_per_insert or more, never spans two windows, and the
 * last one of a window may be short. Per statement the host does one INSERT of bytes[byte_first, byte_end) of `rowbinary` — its rows are
 * consecutive rows of the object — and records end_row - first_row and byte_end - byte_first (ETL_CLICKHOUSE_INSERT_ROWS / _BYTES);
 * per window with a statement it records n_stmts (ETL_CLICKHOUSE_STATEMENTS_PER_BATCH). max_bytes_per_insert must lie in [1, 2^63]:
 * with 0 the reference's loop never ends. The reference's default is the constant below.
 * A table-copy batch (etlg_copy_decode; write_table_rows_inner :739-773 calls the same insert_rows with the same budget): n_passes == 0
 * with passes == NULL means one window over all rows, first_event / last_event are row indexes, and no reason can apply.
 * Outputs: device memory with ETLG_F_OUTPUT_ON_DEVICE in `flags`, else host memory; each may be NULL and is then skipped.
 *   stmts_out[k], k < min(n_stmts, stmts_cap)   the statement; nothing is written at or beyond the cap, stmts_cap == 0 only counts,
 *                                               info->n_stmts is the full count.
 *   windows_out[w], every pass                  stmt_first / n_stmts count all statements, those beyond stmts_cap included; a window
 *                                               without a member has first_row == end_row == the rows of `rowbinary` in front of
 *                                               data_end.
 * info->status, the first that applies; for every status but ETLG_CHP_OK NO output array is touched and the counts are 0:
 *   ETLG_CHP_BAD_PASSES  as ETLG_SFP_BAD_PASSES; info->bad_pass = the lowest such index.
 *   ETLG_CHP_FAILED      info->event = the lowest failing member inside a window, whatever its reason; info->reason = ETLG_CHP_R_*;
 *                        info->fail_pass = the window that holds it. The reference has written the passes in front of that window
 *                        when it raises the error: the host plans again with passes[0, fail_pass) alone. It fails the whole call at
 *                        the first such event over all tables: the host takes the minimum over the slots it plans.
 *   ETLG_CHP_NEEDS_HOST  `rowbinary` has status ETLG_RB_NEEDS_HOST: info->event = its host_event (fail_pass stays ~0); or a member
 *                        that does not fail has no row in `rowbinary` — a key-only Delete of a slot whose tombstone only the host
 *                        builds (a nullable non-key column of a type whose array-ness the host alone knows): info->event = the lowest
 *                        such member, info->fail_pass its window.
 * ETLG_InvalidArgument also: an unknown slot, a batch that is not device-resident (an ASYNC batch is synced first; one that ended in
 * a decode error gives that error), n_passes > 0 without passes, max_bytes_per_insert out of range, n_passes or n_events above 2^38,
 * and a `rowbinary` of 2^32 - 16 rows or more (the jump tables index rows with 32 bits).
 * A stated difference from the reference: etlg_batch_rowbinary encodes the whole slot first, so its own errors (a NULL in a
 * non-nullable column, a date out of range, ETLG_E_JSON) come before a refusal that the reference would have met earlier in event order.
 * The call stops for the device once, at its end: the jump tables and the statement bound are sized from the object's n_rows and
 * n_bytes and from max_bytes_per_insert, which the host holds.
 * What is tested: the reference's tests state no statement boundary as a number; tests/clickhouse_plan.py restates the refusals and
 * insert_rows' loop as one sequential loop and tests/test_gpu_clickhouse_plan.py compares every field with it. */
#define ETLG_CH_MAX_BYTES_PER_INSERT 67108864ull /* DEFAULT_MAX_BYTES_PER_INSERT, core.rs:234 */
#define ETLG_CHP_OK 0u
#define ETLG_CHP_BAD_PASSES 1u
#define ETLG_CHP_FAILED 2u
#define ETLG_CHP_NEEDS_HOST 3u
#define ETLG_CHP_R_PARTIAL_UPDATE 1u
#define ETLG_CHP_R_UPDATE_IDENTITY 2u
#define ETLG_CHP_R_DELETE_NO_OLD 3u
#define ETLG_CHP_R_KEY_WIDTH 4u
#define ETLG_CHP_R_KEY_IDENTITY 5u

typedef struct etlg_ch_statement {
  uint64_t window;            /* index into `passes` */
  uint64_t first_row;         /* rows [first_row, end_row) of `rowbinary`: consecutive */
  uint64_t end_row;
  uint64_t first_event;       /* the first row's event */
  uint64_t last_event;        /* the last row's event */
  uint64_t byte_first;        /* bytes [byte_first, byte_end) of `rowbinary`: one write of one range */
  uint64_t byte_end;
} etlg_ch_statement;

typedef struct etlg_ch_window {
  uint64_t stmt_first;        /* first entry of stmts_out */
  uint64_t n_stmts;           /* ETL_CLICKHOUSE_STATEMENTS_PER_BATCH (recorded when > 0) */
  uint64_t first_row;         /* the member rows [first_row, end_row) of `rowbinary` */
  uint64_t end_row;
  uint64_t n_members;
  uint64_t n_bytes;           /* bytes of the member rows */
} etlg_ch_window;

typedef struct etlg_ch_plan_info {
  uint64_t n_stmts;           /* may exceed stmts_cap */
  uint64_t n_members;
  uint64_t n_rows;            /* rows in statements (== n_members) */
  uint64_t n_bytes;           /* their bytes */
  uint64_t event;             /* FAILED / NEEDS_HOST: the event; else ~0 */
  uint64_t bad_pass;          /* BAD_PASSES: the lowest such window; else ~0 */
  uint64_t fail_pass;         /* FAILED, NEEDS_HOST for a member without a row: the window that holds `event`; else ~0 */
  uint32_t status;            /* ETLG_CHP_* */
  uint32_t reason;            /* FAILED: ETLG_CHP_R_* */
} etlg_ch_plan_info;

int32_t etlg_clickhouse_plan(etlg_ctx* ctx, etlg_batch* batch, int32_t schema_slot, const etlg_outline_pass* passes, uint64_t n_passes,
                             uint32_t passes_on_device, const etlg_rowbinary* rowbinary, uint64_t max_bytes_per_insert, uint32_t flags,
                             etlg_ch_statement* stmts_out, uint64_t stmts_cap, etlg_ch_window* windows_out, etlg_ch_plan_info* info);

/* The BigQuery sink's append requests of ONE schema slot, planned on the device: the step between etlg_batch_protobuf and the sink's
 * requests — where write_events (etl-destinations bigquery/core.rs:956-1069) refuses an event and which rows form each
 * create_append_request — without downloading row_offsets / row_event / ev_kind / ev_flags / ev_schema_slot. Shaped after
 * etlg_clickhouse_plan above.
 * Windows: `passes` as in etlg_clickhouse_plan — only [first_event, data_end) of each is read; windows ascend, do not overlap and may
 * be empty. One window is what one turn of write_events' outer loop gathers for one table until a Relation or Truncate
 * (core.rs:959-1040).
 * MEMBERS of a window: its Insert / Update / Delete events with ev_schema_slot == schema_slot. The sink has no replay filter: every
 * member is retained.
 * `protobuf`: the object etlg_batch_protobuf built for this batch and slot; required, device-resident (ETLG_F_OUTPUT_ON_DEVICE), of
 * status ETLG_RB_OK or ETLG_RB_NEEDS_HOST; anything else — NULL, a host-resident object, a RowBinary, NDJSON or DuckLake object,
 * another batch's or slot's object — is ETLG_InvalidArgument.
 * FAILING members, raised at the event, in event order; per event the reference's order of tests, so an event has one reason:
 *   ETLG_BQP_R_PARTIAL_UPDATE          an Update with ETLG_FLAG_PARTIAL (bigquery_update_new_row :1478-1494, called at :1000 before the
 *                                      old image is looked at);
 *   ETLG_BQP_R_UPDATE_NO_OLD_IDENTITY  a full Update with ETLG_OLD_NONE on a slot whose replica identity is not PrimaryKey (:1439-1442,
 *                                      ensure_bigquery_update_without_old_row_can_skip_delete :1516-1534);
 *   ETLG_BQP_R_KEY_WIDTH               an Update or Delete with ETLG_OLD_KEY on a slot whose identity column count differs from its
 *                                      primary-key column count (:1599-1614 Update, :1680-1694 Delete: the width is tested first);
 *   ETLG_BQP_R_KEY_IDENTITY            an Update or Delete with ETLG_OLD_KEY, widths agree, identity not PrimaryKey (:1616, :1696,
 *                                      ensure_bigquery_key_image_matches_primary_key :1537-1554);
 *   ETLG_BQP_R_DELETE_NO_OLD           a Delete with ETLG_OLD_NONE (bigquery_delete_old_row :1497-1512).
 * The host picks the reference's description from reason and event kind (the two key-image errors are worded per kind).
 * REQUESTS, a WAL batch: per window with at least one member exactly one — the create_append_request of that table in that turn
 * (:1043-1064). Its rows are the rows of `protobuf` whose row_event lies in [first_event, data_end): consecutive rows, found by two
 * lower bounds in row_event. An Update that changed the primary key is TWO rows of one event (:1445-1474), so end_row - first_row may
 * exceed n_members; it is what ETL_BQ_APPEND_BATCHES_BATCH_SIZE records (:1053). The entry's index in reqs_out is the request_index.
 * max_batch_bytes is ignored on this path. The client crate's own split of one request into gRPC messages is not in the reference,
 * is not restated here and is out of scope.
 * REQUESTS, a table-copy batch (etlg_copy_decode; write_table_rows :602-649): n_passes == 0 with passes == NULL, one window over all
 * rows (passes on such a batch are ETLG_InvalidArgument: the split is of the whole call's rows). With R = n_rows of the object,
 * calculate_target_batches_for_table_copy (:1760-1784) and split_table_rows (:1790-1827):
 *     est = the length of row 0 — the object's rows lie back to back without framing, a row's length is encoded_len() of the row —;
 *     rows_per_batch = est ? max_batch_bytes / est : R;   target = rows_per_batch ? ceil(R / rows_per_batch) : 1   (R == 0: 0);
 *     one request of all rows if R <= 1, target == 1 or R <= target; otherwise opt = ceil(R / target), nsub = ceil(R / opt),
 *     q = R / nsub, r = R % nsub, and request i < nsub holds q + (i < r) rows from row i * q + min(i, r). R == 0 gives no request.
 * max_batch_bytes — the client crate's MAX_BATCH_SIZE_BYTES, whose value the reference does not state: an argument without a default
 * macro — must lie in [1, 2^63] for a copy batch. est is read on the device. first_event / last_event are row indexes, n_members is
 * the request's row count, `window` is 0, and no reason can apply.
 * Outputs: device memory with ETLG_F_OUTPUT_ON_DEVICE in `flags`, else host memory; each may be NULL and is then skipped.
 *   reqs_out[k], k < min(n_reqs, reqs_cap)   the request; nothing is written at or beyond the cap, reqs_cap == 0 only counts,
 *                                            info->n_reqs is the full count.
 *   windows_out[w], every pass (one entry on a copy batch)   req_first / n_reqs count all requests, those beyond reqs_cap included; a
 *                                            window without a member has first_row == end_row == the rows of `protobuf` in front of
 *                                            data_end.
 * info->status, the first that applies; for every status but ETLG_BQP_OK NO output array is touched and the counts are 0:
 *   ETLG_BQP_BAD_PASSES  as ETLG_CHP_BAD_PASSES; info->bad_pass = the lowest such index.
 *   ETLG_BQP_FAILED      info->event = the lowest failing member inside a window, whatever its reason; info->reason = ETLG_BQP_R_*;
 *                        info->fail_pass = the window that holds it. The reference has written the passes in front of that window
 *                        when it raises the error: the host plans again with passes[0, fail_pass) alone. It fails the whole call at
 *                        the first such event over all tables: the host takes the minimum over the slots it plans.
 *   ETLG_BQP_NEEDS_HOST  `protobuf` has status ETLG_RB_NEEDS_HOST: info->event = its host_event (fail_pass stays ~0); or a member
 *                        that does not fail has no row in `protobuf` — an Update with an old image whose primary key the device does
 *                        not compare (a float / numeric / timetz key class, a DEFERRED key cell): info->event = the lowest such
 *                        member, info->fail_pass its window.
 * ETLG_InvalidArgument also: an unknown slot, a batch that is not device-resident (an ASYNC batch is synced first; one that ended in
 * a decode error gives that error), n_passes > 0 without passes, n_passes or n_events above 2^38.
 * A stated difference from the reference: etlg_batch_protobuf encodes the whole slot first, so its own errors (a numeric of more than
 * 38 decimal places, a NULL array element, ETLG_E_JSON) come before a refusal that the reference would have met earlier in event order.
 * The call stops for the device once, at its end.
 * What is tested: tests/golden/bigquery_split_kats.py holds the reference's split_table_rows_* and calculate_target_batches_* vectors
 * (core.rs:2277-2419); tests/bigquery_plan.py restates the refusals, the request per window and the two copy functions, and
 * tests/test_gpu_bigquery_plan.py compares every field with it. */
#define ETLG_BQP_OK 0u
#define ETLG_BQP_BAD_PASSES 1u
#define ETLG_BQP_FAILED 2u
#define ETLG_BQP_NEEDS_HOST 3u
#define ETLG_BQP_R_PARTIAL_UPDATE 1u
#define ETLG_BQP_R_UPDATE_NO_OLD_IDENTITY 2u
#define ETLG_BQP_R_KEY_WIDTH 3u
#define ETLG_BQP_R_KEY_IDENTITY 4u
#define ETLG_BQP_R_DELETE_NO_OLD 5u

typedef struct etlg_bq_request {
  uint64_t window;            /* index into `passes`; 0 on a table-copy batch */
  uint64_t first_row;         /* rows [first_row, end_row) of `protobuf`: consecutive */
  uint64_t end_row;
  uint64_t first_event;       /* the first row's event */
  uint64_t last_event;        /* the last row's event */
  uint64_t byte_first;        /* bytes [byte_first, byte_end) of `protobuf` */
  uint64_t byte_end;
  uint64_t n_members;         /* the window's members; end_row - first_row - n_members of them are two rows */
} etlg_bq_request;

typedef struct etlg_bq_window {
  uint64_t req_first;         /* first entry of reqs_out */
  uint64_t n_reqs;            /* 0 or 1; a table-copy batch: all */
  uint64_t first_row;         /* the member rows [first_row, end_row) of `protobuf` */
  uint64_t end_row;
  uint64_t n_members;
  uint64_t n_two_row;         /* members of two rows: end_row - first_row - n_members */
  uint64_t n_bytes;           /* bytes of the member rows */
} etlg_bq_window;

typedef struct etlg_bq_plan_info {
  uint64_t n_reqs;            /* may exceed reqs_cap */
  uint64_t n_members;
  uint64_t n_rows;            /* rows in requests (n_members + n_two_row) */
  uint64_t n_two_row;
  uint64_t n_bytes;           /* their bytes */
  uint64_t est_row_bytes;     /* a table-copy batch: the length of row 0; else 0 */
  uint64_t target_batches;    /* a table-copy batch: calculate_target_batches_for_table_copy; else 0 */
  uint64_t event;             /* FAILED / NEEDS_HOST: the event; else ~0 */
  uint64_t bad_pass;          /* BAD_PASSES: the lowest such window; else ~0 */
  uint64_t fail_pass;         /* FAILED, NEEDS_HOST for a member without a row: the window that holds `event`; else ~0 */
  uint32_t status;            /* ETLG_BQP_* */
  uint32_t reason;            /* FAILED: ETLG_BQP_R_* */
} etlg_bq_plan_info;

int32_t etlg_bigquery_plan(etlg_ctx* ctx, etlg_batch* batch, int32_t schema_slot, const etlg_outline_pass* passes, uint64_t n_passes,
                           uint32_t passes_on_device, const etlg_rowbinary* protobuf, uint64_t max_batch_bytes, uint32_t flags,
                           etlg_bq_request* reqs_out, uint64_t reqs_cap, etlg_bq_window* windows_out, etlg_bq_plan_info* info);

/* The Iceberg sink's writes of ONE schema slot, planned on the device: the step between etlg_batch_iceberg and the sink's insert_rows
 * calls — where write_events (etl-destinations iceberg/core.rs:300-440) refuses an event, which rows of the changelog object form each
 * insert_rows call, and what a slice of every Arrow column of the object over those rows needs — without downloading row_event /
 * ev_kind / ev_flags / ev_schema_slot / ev_table_id, nor any validity bitmap or offsets array of the object. Shaped after
 * etlg_bigquery_plan above.
 * Windows: `passes` are the passes of etlg_batch_outline taken WITH ETLG_OL_RELATIONS_INLINE: Iceberg's inner loop breaks at Truncate
 * only (core.rs:310-312) and meets Relation events inside the data run (:360). Only [first_event, data_end) of each is read; windows
 * ascend, do not overlap and may be empty. The call cannot tell which option the outline was built with: passes taken without it are
 * narrower windows (they end at every Relation), which plan more writes than the reference makes, and nothing here reports that.
 * MEMBERS of a window: its Insert / Update / Delete events with ev_schema_slot == schema_slot.
 * `changelog`: the object etlg_batch_iceberg built for this batch and slot; required, device-resident (ETLG_F_OUTPUT_ON_DEVICE).
 * Anything else — NULL, a host-resident object, an object of etlg_batch_columns or etlg_batch_ducklake_copy, another batch's or slot's
 * object — is ETLG_InvalidArgument.
 * FAILING members, raised at the event, in event order; one test applies per event kind, so an event has one reason (the numbers of
 * etlg_changelog_info.host_reason):
 *   ETLG_ICE_PARTIAL_UPDATE          an Update with ETLG_FLAG_PARTIAL (iceberg_update_row, core.rs:636-652);
 *   ETLG_ICE_KEY_ONLY_DELETE         a Delete with ETLG_OLD_KEY (iceberg_delete_row, :661);
 *   ETLG_ICE_DELETE_WITHOUT_OLD_ROW  a Delete with ETLG_OLD_NONE (:670). pgoutput sends no Delete without an old image: this reason is
 *                                    reachable in the model (tests/iceberg_plan.py) alone.
 * The changelog object holds no row for a refused event, by design.
 * WRITES, a WAL batch: per window with at least one member exactly one — the insert_rows of that table in that turn (:395-409). Its
 * rows are the rows of `changelog` whose row_event lies in [first_event, data_end): consecutive rows, found by two lower bounds in
 * row_event. One event is one row, so end_row - first_row == n_members.
 * THE TABLE KEY. The loop groups rows in a HashMap<TableId, (schema, rows)> with the first schema seen for the table (:304-307,
 * :324-327): per TABLE, not per schema slot. A window that holds Insert / Update / Delete events of this slot's table_id (the context's,
 * as etlg_ctx_slots reports it) under ANOTHER slot is one the reference encodes under one schema, or refuses at the Relation between
 * them (:360-382). The planner does not decide this. Every window with a member reports other_slot_event: the lowest Insert / Update /
 * Delete event in [first_event, data_end) whose ev_table_id is the slot's table and whose ev_schema_slot is another slot, ~0 if there
 * is none; a window without a member of this slot reports ~0 (the table's entry of that turn is the other slot's alone, and the
 * plan of that slot covers it). info->n_mixed counts the windows that have one.
 * SLICES. For every write k < min(n_writes, writes_cap) and every column c of the object — the data columns and the two CDC columns,
 * n_cols = etlg_columns_view.n_cols — slices_out[k * n_cols + c] describes rows [first_row, end_row) of that column as an Arrow slice:
 *   null_count         zero bits of `validity` in the row range;
 *   deferred_count     set bits of `deferred` in the row range;
 *   byte_first/_end    the range of `values` the slice owns: row * value_bytes for a fixed-width kind; the bit positions first_row,
 *                      end_row for ETLG_AK_BOOLEAN; offsets[first_row], offsets[end_row] for LARGE_UTF8 / LARGE_BINARY / TEXT_FORM; for
 *                      ETLG_AK_LIST the child range times the element width, the child bit positions for a BOOLEAN child, and
 *                      child_offsets[child_first], child_offsets[child_end] for a var-len child (both 0 when the column has no child
 *                      element: there are no child offsets then);
 *   child_first/_end   ETLG_AK_LIST: offsets[first_row], offsets[end_row]; otherwise 0;
 *   child_null_count   ETLG_AK_LIST: zero bits of child_validity in [child_first, child_end); otherwise 0.
 * Over writes that cover all rows of the object the null_count / deferred_count / child_null_count of a column's slices sum to the
 * column's own counts. A bitmap whose column reports a count of 0 is not read.
 * A table-copy batch (etlg_copy_decode; write_table_rows, core.rs:268-291): n_passes == 0 with passes == NULL (passes on such a batch are
 * ETLG_InvalidArgument), one window over all rows and one write when the object has a row (!table_rows.is_empty()). No refusal can
 * apply; first_event / last_event are row indexes, n_members the row count, other_slot_event ~0.
 * Outputs: device memory with ETLG_F_OUTPUT_ON_DEVICE in `flags`, else host memory; each may be NULL and is then skipped.
 *   writes_out[k], k < min(n_writes, writes_cap)   the write; nothing is written at or beyond the cap (slices: writes_cap * n_cols),
 *                                                  writes_cap == 0 only counts, info->n_writes is the full count.
 *   windows_out[w], every pass (one entry on a copy batch)   write_first / n_writes count all writes, those beyond writes_cap
 *                                                  included; a window without a member has first_row == end_row == the rows of
 *                                                  `changelog` in front of data_end.
 * info->status, the first that applies; for every status but ETLG_ICP_OK NO output array is touched and the counts are 0:
 *   ETLG_ICP_BAD_PASSES  as ETLG_CHP_BAD_PASSES; info->bad_pass = the lowest such index.
 *   ETLG_ICP_FAILED      info->event = the lowest failing member inside a window, whatever its reason; info->reason = ETLG_ICE_*;
 *                        info->fail_pass = the window that holds it. The reference raises the error while it gathers that pass, so
 *                        the passes in front of it are written: the host plans again with passes[0, fail_pass) alone. It fails the
 *                        whole call at the first such event over all tables: the host takes the minimum over the slots it plans.
 *   ETLG_ICP_NEEDS_HOST  a member that does not fail has no row in `changelog`: info->event = the lowest such member, info->fail_pass
 *                        its window. etlg_batch_iceberg selects every Insert, full Update and full-old-row Delete of the slot, and the
 *                        call takes no other object, so this status is reachable in the model alone, not through this ABI; the
 *                        kernels keep the test so that a row is never read for an event that has none.
 * ETLG_InvalidArgument also: an unknown slot, a batch that is not device-resident (an ASYNC batch is synced first; one that ended in
 * a decode error gives that error), n_passes > 0 without passes, n_passes or n_events above 2^38, more than 2^38 slices to write.
 * Stated differences from the reference: etlg_batch_iceberg builds the whole slot first, so its own errors (a malformed array literal,
 * ETLG_E_JSON) come before a refusal that the reference would have met earlier in event order. Column names, the catalog calls, the
 * Relation metadata check against the store and Parquet encoding are not restated here.
 * The call stops for the device once, at its end.
 * What is tested: tests/golden/iceberg_plan_kats.py holds the outcomes of the reference's iceberg_update_row_* / iceberg_delete_row_*
 * unit tests (core.rs:794-840); tests/iceberg_plan.py restates the refusals, the write per window, other_slot_event and the slice
 * arithmetic, and tests/test_gpu_iceberg_plan.py compares every field of every output with it. */
#define ETLG_ICP_OK 0u
#define ETLG_ICP_BAD_PASSES 1u
#define ETLG_ICP_FAILED 2u
#define ETLG_ICP_NEEDS_HOST 3u

typedef struct etlg_ice_write {
  uint64_t window;            /* index into `passes`; 0 on a table-copy batch */
  uint64_t first_row;         /* rows [first_row, end_row) of `changelog`: consecutive */
  uint64_t end_row;
  uint64_t first_event;       /* the first row's event */
  uint64_t last_event;        /* the last row's event */
  uint64_t n_members;         /* == end_row - first_row */
  uint64_t other_slot_event;  /* the window's; ~0 none */
} etlg_ice_write;

typedef struct etlg_ice_window {
  uint64_t write_first;       /* first entry of writes_out */
  uint64_t n_writes;          /* 0 or 1 */
  uint64_t first_row;         /* the member rows [first_row, end_row) of `changelog` */
  uint64_t end_row;
  uint64_t n_members;
  uint64_t other_slot_event;  /* the lowest Insert / Update / Delete of the slot's table under another slot in the window; ~0 none */
} etlg_ice_window;

typedef struct etlg_ice_slice {
  uint64_t null_count;
  uint64_t deferred_count;
  uint64_t byte_first;        /* of `values`: bytes, or bit positions where the values are bit-packed */
  uint64_t byte_end;
  uint64_t child_first;       /* ETLG_AK_LIST: the child elements [child_first, child_end); else 0 */
  uint64_t child_end;
  uint64_t child_null_count;
} etlg_ice_slice;

typedef struct etlg_ice_plan_info {
  uint64_t n_writes;          /* may exceed writes_cap */
  uint64_t n_members;
  uint64_t n_rows;            /* rows in writes (== n_members) */
  uint64_t n_mixed;           /* windows with an other_slot_event */
  uint64_t event;             /* FAILED / NEEDS_HOST: the event; else ~0 */
  uint64_t bad_pass;          /* BAD_PASSES: the lowest such window; else ~0 */
  uint64_t fail_pass;         /* FAILED / NEEDS_HOST: the window that holds `event`; else ~0 */
  uint32_t status;            /* ETLG_ICP_* */
  uint32_t reason;            /* FAILED: ETLG_ICE_* */
} etlg_ice_plan_info;

int32_t etlg_iceberg_plan(etlg_ctx* ctx, etlg_batch* batch, int32_t schema_slot, const etlg_outline_pass* passes, uint64_t n_passes,
                          uint32_t passes_on_device, const etlg_columns* changelog, uint32_t flags, etlg_ice_write* writes_out,
                          uint64_t writes_cap, etlg_ice_slice* slices_out, etlg_ice_window* windows_out, etlg_ice_plan_info* info);

/* Schema slots known to the context (also reachable from every batch view). */
int32_t etlg_ctx_slots(const etlg_ctx* ctx, uint32_t* n_slots,
                       const etlg_slot_desc** slots);

/* ------------------------------------------------------------- measurement */

/* HIP-event timing of the kernels launched by etlg_decode, each on the stream
 * it is launched on (bench.py's roofline leg). enable = 1: as the chain runs —
 * consecutive ETLG_F_ASYNC batches side by side on two decode streams, so their
 * durations overlap; enable = 2: the chain kept on one stream, i.e. every
 * kernel timed alone; 0: off (resets the counters). */
typedef struct etlg_kernel_stat {
  const char* name;
  uint64_t launches;
  double total_ms;
} etlg_kernel_stat;

int32_t etlg_ctx_profile(etlg_ctx* ctx, int32_t enable);
int32_t etlg_ctx_profile_read(etlg_ctx* ctx, etlg_kernel_stat* out,
                              uint32_t cap, uint32_t* n);

#ifdef __cplusplus
}
#endif
#endif /* ETLG_H */
