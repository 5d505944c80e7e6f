// Structures shared between the host control plane (host.cpp) and the gfx950
// kernels (kernels.hip). Plain data, no pointers into host memory.
#pragma once
#include <stdint.h>

namespace etlg {

// Frame classes written by k_classify (pgoutput tag, or the XLogData/keepalive
// envelope). 0 = malformed frame (wire-level error).
enum : uint8_t { FT_BAD = 0 };

// One replicated column of a schema slot (mirrors etlg_slot_col).
struct DevCol {
  uint8_t cls;       // etlg_type_class
  uint8_t nullable;
  uint8_t identity;
  uint8_t key_col;   // (k_rows) the column whose key_index is THIS record's index: cell j of a dense key tuple decodes against column key_col of record j
  uint16_t off_full; // byte offset inside a full-layout row
  uint16_t off_key;  // byte offset inside a key-layout row
  uint16_t key_index;
  uint16_t hr;       // (k_rows) heap rank: bits 0..7 among the columns of a full row whose class can reach the heap, bits 8..15 among the identity
                     // columns in key_index order; 0xFF = the class never reaches the heap
};

// A ReplicatedTableSchema instance (reference: crates/etl/src/schema.rs:380-441).
struct DevSlot {
  uint32_t n_cols, n_ident;
  uint32_t row_full, row_key;  // bytes, multiples of 4
  uint32_t st_full, st_key;    // state bytes at the head of a row
  uint32_t cols_base;          // index of the first DevCol
  uint32_t has_var;            // != 0: some column may produce a heap entry (var-len / numeric / deferrable class). For slots of
                               // up to 16 columns, bit k: column k may; bit 16 + k: ... and how many bytes depends on the text
                               // (numeric, float, date / time, bytea), not on its length alone. Wider slots: all ones.
  uint32_t key_masks;          // the same two masks for a dense key tuple: bit j = the identity column with key_index j
  uint32_t ident_mask;         // bit k: column k is an identity column (<= 16 columns)
  uint32_t host_id;            // the schema slot id the arenas name (etlg_slot_desc index). The device table holds only the slots a frame
                               // of the batch can decode against, in ascending id order: DevTable.init_slot / DevEpoch.slot /
                               // DecParams.copy_slot index THIS table, and what reaches ev_slot / Truncate bodies is host_id
};

// Per-table side input for one batch: ownership state
// (apply.rs:2844-2850) + the shared-table-cache timeline
// (table_cache.rs:53-154) as a list of epochs keyed by frame index.
struct DevTable {
  uint32_t table_id;
  uint32_t state_kind;  // etlg_table_state_kind
  uint64_t state_lsn;
  uint32_t init_kind;   // cache entry at batch start: 0 none, 1 WaitingForRelation, 2 Ready
  int32_t init_slot;
  uint32_t ep_begin, ep_end;  // range in the DevEpoch array
};

struct DevEpoch {
  uint32_t frame;   // frame index of the R / M message that caused the change
  uint32_t kind;    // 1 WaitingForRelation, 2 Ready
  int32_t slot;
  uint32_t emit;    // R frames: 1 if the RelationEvent is emitted (owned)
};

// Control frame descriptor handed to the host control plane.
struct CtrlFrame {
  uint32_t frame;
  uint32_t tag;        // 'R' | 'M'
  uint32_t in_txn;
  uint32_t stage_off;  // where k_ctrl_list put a copy of the frame's bytes in DecParams.ctrl_stage; ~0: it did not fit, fetch [o0, o1) of the input
  uint64_t final_lsn;
  uint32_t o0, o1;     // byte range of the frame in the input
};

// Result block (device -> host, one small copy per batch).
struct DevResult {
  unsigned long long first_err;  // min over (frame << 16 | rank << 8 | code); ~0 = none
  uint64_t n_events, fixed_bytes, heap_bytes;
  uint64_t payload[3];
  uint64_t n_frames;             // frames consumed
  uint32_t out_in_txn, n_ctrl;
  uint64_t out_final_lsn, out_next_ord;
  uint32_t fused_fail, ctrl_bytes;  // ctrl_bytes: bytes of R / M frames k_ctrl_list gathered into DecParams.ctrl_stage (4-byte granules). fused_fail: single-pass result not usable: 1 a look-back spin gave up (never expected), 2 the fixed-width plan did not
                                 // cover the batch (plan.hip), 4 a schema too wide for k_cells, 8 the ASYNC predecessor of this batch failed
  unsigned long long dbg_t[12];  // ETLG_FUSED_DBG&8: summed shader-clock cycles per phase (lane 0 of every tile)
  // fused kernel: payload byte counters sharded by tile id so that no single address
  // sees more than ntiles/32 atomics; the host folds them into payload[] after the sync
  unsigned long long pay_shard[32][3];
  // plan.hip: set (release) by the batch's last tile once out_in_txn / out_final_lsn / out_next_ord above are written: a batch that runs
  // beside this one on the second stream (DecParams.flags bit 4) polls it before it reads them
  uint32_t carry_ready;
  uint32_t copy_span;   // k_copy_cells: offs[nrows] - offs[0], the bytes of the rows (TableCopyPayloadMetadata) — travels with the result block instead of two 4-byte copies
};

// Side arguments of the fused single-pass kernel (fused.hip).
struct FusedParams {
  unsigned long long* d_txn;   // [ntiles]  st:2 | seg:30 | mark:32
  unsigned long long* d_outa;  // [ntiles]  st:2 | events:30 | heap dwords:32
  unsigned long long* d_outb;  // [ntiles]  st:2 | fixed dwords:62
  uint32_t* ticket;
  uint32_t ntiles;
  uint32_t lds_bytes;          // staging capacity per tile (dynamic LDS)
  uint32_t in_aligned;         // input pointer is 16-byte aligned
  uint32_t blk;                // frames per tile (256 or 64)
  uint32_t dbg;                // ablation bits (profiling only): 1 no LDS staging, 2 skip writes, 4 skip look-back, 8 phase timers
  uint32_t seq_lookback;       // 1: ownership needs the transaction's final_lsn (a table is in SyncDone state)
  uint32_t side_bytes;         // LDS bytes reserved for a copy of the side-input tables (0 = read them from global)
  uint32_t maxc;               // k_cells: widest schema slot of the batch (columns)
  uint32_t clear_words;        // 64-bit words of d_clear this launch zeroes (the descriptor buffer of the NEXT batch)
  unsigned long long* d_clear;
  uint32_t copy_rel;           // k_copy_cells: the table id the rows' Insert events carry
  uint32_t rows_maxh_old;      // k_rows: most heap-class IDENTITY columns in one slot (rows of the heap-cell table for key / old images)
  uint32_t rows_maxh;          // k_rows: most heap-class columns in one slot (rows for new images)
};

constexpr unsigned long long kNoErr = ~0ull;
// DevResult.fused_fail bits, by name for the host (the kernels write the literals)
constexpr uint32_t kFailLookback = 1u;     // a look-back spin gave up (never expected)
constexpr uint32_t kFailPlanGaveUp = 2u;   // the fixed-width plan did not cover the batch (plan.hip)
constexpr uint32_t kFailTooWide = 4u;      // a schema too wide for k_cells
constexpr uint32_t kFailNotRun = 8u;       // the ASYNC predecessor of this batch failed: this one did not run
constexpr uint32_t kFailRowsBack = 16u;    // k_rows handed the batch back (bits 8 and up: why; 1 = a tile beyond its LDS window, DevResult.dbg_t[11] holds what it needed)
constexpr uint32_t kFailScanCount = 32u;   // decoded behind its boundary scan and the count read on the device was not usable (plan.hip)
// DecParams.flags bits, likewise
constexpr uint32_t kDecNoControl = 1u;     // bit 0: NO_CONTROL asserted
constexpr uint32_t kDecCopyRows = 2u;      // bit 1: table-copy rows
constexpr uint32_t kDecLateCarry = 16u;    // bit 4: `carry` belongs to a batch that may still be running on the other stream
constexpr uint32_t kDecCtlPrePass = 32u;   // bit 5: the pre-pass of a pipelined control batch (the carried state comes from `carry`, kernels.hip)
constexpr uint32_t kDecCheckCells = 64u;   // bit 6: ETLG_F_CHECK_CELLS
constexpr uint32_t kDecAblations = 0xF00u; // bits 8-11: profiling ablations (ETLG_FUSED_DBG)
constexpr int kBlock = 256;  // frames per workgroup (one lane per frame)

// error stage ranks: for one frame the lowest rank wins, mirroring the order
// in which the reference detects them (wire parse -> transaction state ->
// ownership/schema lookup -> event decode).
enum : uint32_t { RK_WIRE = 0, RK_TXN = 1, RK_SCHEMA = 2, RK_DECODE = 3, RK_COPY_SHAPE = 4 };

struct DecParams {
  const uint8_t* in;
  const uint32_t* offs;  // nframes + 1
  uint32_t nframes;
  uint32_t nblocks;
  uint64_t in_len;
  // carried transaction state (apply.rs:942-963)
  uint32_t in_txn;
  uint32_t worker_kind, sync_table;
  // bits 8-11 (0x100 no row stores, 0x200 no header stores, 0x400 no row decode, 0x800 uniform waves only) are
  // profiling ablations set from ETLG_FUSED_DBG; results are wrong with any of them
  uint32_t flags;        // bit0: NO_CONTROL asserted; bit1: table-copy rows (synthetic Insert frames: no ownership
                         // check, NULL allowed in every column — table_row.rs:199-201); bit4: `carry` belongs to a batch that may still
                         // be running on the other stream: poll its carry_ready before reading it (plan.hip only)
  uint64_t final_lsn, next_ord;
  uint32_t host_err_frame;  // frames >= this are ignored (host control plane failed there)
  uint32_t n_tables;
  uint32_t n_epochs, n_slots, n_cols;  // sizes of the side-input arrays
  int32_t copy_slot;     // flags bit1 (table-copy rows): the schema slot every row decodes against
  // side inputs
  const DevTable* tables;
  const DevEpoch* epochs;
  const DevSlot* slots;
  const DevCol* cols;   // ETLG_F_CHECK_CELLS: the n_cols records are followed by n_cols bytes, the element class of every array column
                        // (etlg_array_elem_class; 0 otherwise) — chk_elem_table(), values.hip.h. The structure itself did not grow: the
                        // argument blocks of the single-pass kernels are laid out as before
  // per-frame scratch
  uint8_t* f_tag;
  uint8_t* f_emit;
  uint32_t* f_fixed;  // bytes
  uint32_t* f_heap;   // bytes
  // per-block aggregates / prefixes
  uint32_t* blk_cnt;      // ordinal consumers per block -> exclusive prefix
  uint32_t* blk_last;     // max over ((idx+1)<<1|isBegin) -> exclusive running max
  uint32_t* blk_ev;       // events per block -> exclusive prefix
  uint64_t* blk_fixed;    // bytes
  uint64_t* blk_heap;
  uint64_t* blk_payload;  // 3 per block
  CtrlFrame* ctrl;        // compacted control frames
  uint32_t ctrl_cap;
  uint32_t ctrl_stage_cap;  // bytes of ctrl_stage
  uint8_t* ctrl_stage;    // the control frames' bytes, gathered so that the host fetches them with one copy
  // outputs
  uint8_t* ev_kind; uint8_t* ev_flags;
  uint32_t* ev_table; uint32_t* ev_slot;
  uint64_t* ev_start; uint64_t* ev_commit; uint64_t* ev_ord; uint64_t* ev_body;
  uint8_t* fixed; uint8_t* heap;
  uint64_t fixed_cap, heap_cap;
  DevResult* res;
  // ETLG_F_ASYNC chains batches on the device: when set, the carried transaction state (in_txn / final_lsn / next_ord above)
  // is read from the result block of the batch issued just before this one on the same stream, not from these host values
  const DevResult* carry;
  // ETLG_F_ASYNC without a sidecar, fixed-width plan (round 6): the record-boundary scan of THIS batch is still in flight when the decode is
  // enqueued behind it. `nframes` above is then an upper bound the grids were sized by; the kernels read the count the scan left on the
  // device — words [0] frames, [1] flags, [2] tiles that guessed wrong (either non-zero: the scan did not hold) — and take it for nframes (plan.hip, plan_frames_from_device)
  const uint32_t* nframes_dev;
};

// The fixed-width decode plan (plan.hip): the eligible tables of a batch, sorted by rel_id, and their columns.
struct PlanTab {
  uint32_t rel_id;
  uint32_t slot;        // schema slot id
  uint32_t n_cols;
  uint32_t row_dwords;  // full-layout row block, dwords
  uint32_t cols_base;   // index of the table's first column word
  uint32_t key_dwords;  // key-layout row block, dwords; 0: the plan does not take this table's Deletes (no identity column)
  uint32_t n_ident;
  uint32_t keys_base;   // index of the table's first key word (n_cols of them, behind the column words)
};
// one word per column: cls | nullable << 8 | off_full << 16
// one key word per column (Deletes by key, round 6): identity | key_index << 8 | off_key (dwords) << 24

struct PlanParams {
  unsigned long long* desc;    // look-back words (plan.hip): desc[ntiles] | gdesc[ceil(ntiles / 64)] | dlsn[ntiles]
  unsigned long long* d_clear; // descriptor buffer of the NEXT batch, zeroed by this launch
  uint32_t clear_words;
  uint32_t ntiles;             // tiles of 64 frames (one wave each)
  uint32_t lds_bytes;          // dynamic LDS per tile: the staging window [0, rows_off) + the tile's image of the fixed arena (64 rows)
  uint32_t rows_off;
  uint32_t n_tabs;
  const PlanTab* tabs;
  const uint32_t* cols;
  uint32_t dbg;                // ETLG_PLAN_DBG. bit 0: no LDS staging (tests: the in-place reader). Profiling ablations, results are WRONG:
                               // bit 1 stop after staging, bit 2 stop after the message heads, bit 3 no cell decode / row stores, bit 4 no event header stores
                               // bit 5: phase clocks into DevResult.dbg_t; bit 9: one tile per wave (k_plan) even when two would do
  uint32_t max_row_dw;         // dwords of the widest planned row (k_plan2 / k_plan3 keep a row of up to 6 / 8 dwords in registers)
  // Tile prefixes from the sidecar pre-pass (k_plan_pre, plan.hip), or null: the decode kernel then runs the look-back itself.
  // pre[2 * tile] = {last Begin / Commit mark before the tile : 30 | fixed-arena dwords before it : 32}, pre[2 * tile + 1] = LSN of the
  // Begin that is open when the tile starts — what plan_resolve2 would hand the tile.
  const unsigned long long* pre;
  unsigned long long* pre_out; // ... as the pre-pass writes it
  uint32_t* pre_ticket;        // the pre-pass's arrival counter (zero between launches)
  uint32_t pre_tag;            // 1..3, changes with every use of a buffer: the status of this launch's group words
  uint32_t pre_row_dw;         // the row dwords every planned table shares (the pre-pass prices a frame without reading it)
  uint32_t pre_key_dw;         // ... and the key-row dwords they share, with
  uint32_t pre_key_below;      // the length below which a frame that is no Begin / Commit is priced as a Delete by key: the shortest row frame any
                               // planned table can send (38 + 6 per NOT NULL column + 1 per nullable one). 0: every such frame is a row (Deletes give the batch up)
  uint32_t pre_key_max;        // the longest Delete by key the pre-pass still recognises: a frame of pre_key_below .. pre_key_max bytes has its tag byte read
                               // (like the frames of a Begin's / Commit's length) and is priced as a key row when that is 'D'
};

// ---- columnar hand-off (columns.hip, rowformats.hip, finish.hip)
// The vocabulary the host (host_handoff.inc) and the kernels share. The fields that hold these stay uint32_t.
enum : uint32_t { FMT_ROWBINARY = 0, FMT_PROTOBUF = 1, FMT_NDJSON = 2, FMT_DUCKLAKE = 3 };   // RbJob.format: the sink's row format
// ColSel.kinds bits: inserts, new rows of non-partial updates, full old rows of deletes, key rows of deletes
enum : uint32_t { SEL_INSERT = 1u, SEL_UPDATE_NEW = 2u, SEL_DELETE_OLD = 4u, SEL_DELETE_KEY = 8u };
// ColSel.dl (dl_selection, host_handoff.inc): the tuples the sink upserts, the predicates it deletes / matches by over the identity columns,
// over the primary-key columns (a table-copy batch: every row), the partial Updates. DL_SEL_NONE: not a DuckLake call. RbJob.dl_what holds the
// same fact one lower (dl_row_what): with one numbering in both fields the code bytes of the six DuckLake kernels moved
enum : uint32_t { DL_SEL_NONE = 0, DL_SEL_TUPLES = 1, DL_SEL_PRED_IDENT = 2, DL_SEL_PRED_PK = 3, DL_SEL_UPDATES = 4 };
enum : uint32_t { DL_ROW_TUPLES = 0, DL_ROW_PRED_IDENT = 1, DL_ROW_PRED_PK = 2, DL_ROW_UPDATES = 3 }; constexpr uint32_t dl_row_what(uint32_t sel) { return sel - DL_SEL_TUPLES; }
enum : uint32_t { DLS_NOTHING = 0, DLS_ROW = 1, DLS_HOST = 2, DLS_TWO_ROWS = 3 };   // dl_selected (columns.hip): what an event becomes
// A row's error code (rb_row / pb_row / nd_row / dl_row return column << 8 | code). RB_E_BQ_NUMERIC_SCALE: the json integer rule's too. ND_E_*: Error::Encoding of Snowflake
enum : uint32_t { RB_E_NULL = 1, RB_E_DATE_RANGE = 2, RB_E_HOST_CELL = 3, RB_E_BQ_NUMERIC_SCALE = 4, RB_E_JSON = 5, RB_E_BQ_ARRAY_NULL = 6,
                  ND_E_FLOAT_NAN = 7, ND_E_FLOAT_INF = 8, ND_E_FLOAT_NINF = 9, ND_E_NUM_NAN = 10, ND_E_NUM_INF = 11, ND_E_FIRST = ND_E_FLOAT_NAN, ND_E_LAST = ND_E_NUM_INF };
// The report word: rank | row << 24 | column << 8 | code, folded with atomicMin. A json cell that is not JSON ranks first (the reference's
// decode fails before a sink sees a row), then a date out of range and every report of the other formats, then RowBinary's other reports
constexpr unsigned long long kRbRankDecode = 0ull, kRbRankEarly = 1ull << 61, kRbRankLate = 1ull << 62;
struct RbReport { uint64_t row; uint32_t col, code; };
constexpr unsigned long long rb_report_pack(unsigned long long rank, uint64_t row, uint32_t col_code) { return rank | (unsigned long long)((row << 24) | col_code); }
constexpr RbReport rb_report_unpack(unsigned long long w) { return RbReport{(w & ~(kRbRankEarly | kRbRankLate)) >> 24, (uint32_t)((w >> 8) & 0xFFFF), (uint32_t)(w & 0xFF)}; }
// ColJob.err of a list column is min over (row << 8 | code): this code marks a row handed back DEFERRED, not malformed (k_arr_count)
constexpr uint32_t kArrHandBack = 0xFFu;
struct ColSel {            // which events are rows of the hand-off
  const uint8_t* ev_kind; const uint8_t* ev_flags; const uint32_t* ev_slot; const uint64_t* ev_body;
  uint64_t n_events;
  uint32_t slot, kinds;    // kinds: SEL_* bits
  unsigned long long* host_rows;  // optional: I/U/D events of the slot the selection leaves out (partial updates, key-only deletes)
  uint32_t row_full, row_key;
  uint32_t* blk;           // per-block counts -> exclusive prefix; blk[nblocks] = total
  uint32_t nblocks;
  uint64_t* row_event; uint64_t* row_base;   // outputs of k_col_rows
  // BigQuery rows (pb != 0; bigquery/core.rs:978-1036): an event becomes 0, 1 or 2 rows, and a row's base carries what it is in its
  // top bits (kPbDelete: the sparse DELETE row of an old image; kPbKey: that image has the key layout; kPbSecond: sequence ordinal 1)
  uint32_t pb, n_cols;
  uint32_t identity_pk;    // the slot's replica identity is the primary key
  uint32_t pk_comparable;  // every primary-key column is of a class whose Cell equality is equality of the arena's words / bytes
  const uint8_t* fixed; const uint8_t* heap;
  const uint32_t* cols;    // per replicated column: cls | .. | off_full << 16 (RbJob.cols)
  const uint32_t* kcols;   // identity | source nullable << 1 | primary key << 2 | key_index << 8 | off_key << 16 (RbJob.kcols)
  // DuckLake rows (dl: DL_SEL_*; ducklake/core.rs:1824-1945, batches.rs:1128-1226): a predicate row's base carries kPbKey when the image has
  // the key layout. DL_SEL_UPDATES: two rows per event, the SET clause of the partial new row, then the predicate of the old image — without
  // one, of the new row itself (kPbSecond marks the predicate row). That arm reads the new row's cell states through fixed / kcols /
  // n_cols above.
  // dl_ident: the slot has identity columns (without them every predicate candidate of a WAL batch stays with the host)
  uint32_t dl, dl_ident;
  // Iceberg changelog (etlg_batch_iceberg; kinds: inserts, new rows, old rows): the Update / Delete events of the slot the sink refuses are counted in ice[0],
  // and ice[3] takes the minimum of (event << 8 | ETLG_ICE_*) over them, in the counting launch (k_col_count). Null: not asked for
  unsigned long long* ice;
};
constexpr unsigned long long kPbDelete = 1ull << 63, kPbKey = 1ull << 62, kPbSecond = 1ull << 61, kPbBase = (1ull << 61) - 1;

// the kernels' private column kinds, behind the public ETLG_AK_* numbers (include/etlg.h): formatted string columns (columns.hip AK_*_STR)
constexpr uint32_t kAkNumericStr = 64, kAkTimetzStr = 65, kAkJsonStr = 66;
struct ColJob {
  const uint8_t* fixed; const uint8_t* heap; const uint64_t* row_base;
  uint64_t n_rows;
  uint32_t col_index, off_full, cls, kind;
  unsigned long long* validity; unsigned long long* deferred; uint8_t* values;
  unsigned long long* null_count; unsigned long long* deferred_count;
  uint32_t* lens; const int64_t* offsets;   // var-len
  // list columns (array literals parsed on the device): element class, child validity words, child null counter, first error
  uint32_t elem_cls;
  uint32_t off32;            // a job of etlg_batch_ducklake_copy: a var-len column's `offsets` is int32 entries (Utf8 / Binary), not int64, and the fixed-width launch has the Int16 arm
  uint32_t* child_validity; unsigned long long* child_nulls; unsigned long long* err;
  uint32_t* child_lens; const int64_t* child_offsets;   // lists of strings: byte length / start of every element
};

struct CdcJob {            // the two trailing CDC columns of an Iceberg changelog batch (k_col_cdc): cdc_operation, sequence_number
  const uint64_t* row_event; const uint8_t* ev_kind; const uint64_t* ev_commit; const uint64_t* ev_ord;
  uint64_t n_rows;
  uint32_t zero_token;     // a table-copy batch: every sequence number is generate_sequence_number(0, 0)
  uint32_t nb_seq, nb_op;  // workgroups of the launch that write sequence / operation bytes (4096 each); the rest write offsets and bitmaps
  uint32_t _pad;
  uint8_t* op_values; uint8_t* seq_values;   // 6 / 33 bytes per row; 16-byte aligned, sized up to a multiple of 16 (whole uint4 stores)
  int64_t* op_offsets; int64_t* seq_offsets; // n_rows + 1 each
  unsigned long long* op_validity; unsigned long long* seq_validity; unsigned long long* op_deferred; unsigned long long* seq_deferred;
};

// A schema slot and a replicated column as the finish pass reads them (slot_table, host_handoff.inc). cols_base: the slot's first ColRec; fin_base / n_fin: its part of FinJob.fin.
// k_size_hints keeps the narrower packing it had, HintSlotRec / HintColRec, cut from the same table: with the wide records it fell outside the parent's span on cfg3
struct SlotRec { uint32_t n_cols, n_ident, row_full, row_key, cols_base, fin_base, n_fin; };
struct ColRec {
  uint32_t kind, offs, key_index;   // kind: cls | identity << 8 | elem_cls << 16; offs: off_full | off_key << 16
  constexpr uint32_t cls() const { return kind & 0xFFu; } constexpr uint32_t elem_cls() const { return (kind >> 16) & 0xFFu; }
  constexpr bool identity() const { return ((kind >> 8) & 1u) != 0; }
  constexpr uint32_t off_full() const { return offs & 0xFFFFu; } constexpr uint32_t off_key() const { return offs >> 16; }
};
struct HintSlotRec { uint32_t n_cols, n_ident, row_full, row_key, cols_base; };
struct HintColRec {   // kind: cls | identity << 8 | off_full << 16
  uint32_t kind, off_key;
  constexpr uint32_t cls() const { return kind & 0xFFu; } constexpr bool identity() const { return ((kind >> 8) & 1u) != 0; } constexpr uint32_t off_full() const { return kind >> 16; }
};
struct HintJob {           // Event::size_hint per event (k_size_hints)
  const uint8_t* ev_kind; const uint8_t* ev_flags; const uint32_t* ev_table; const uint32_t* ev_slot; const uint64_t* ev_body;
  const uint8_t* fixed; const uint8_t* heap;
  uint64_t n_events;
  const HintSlotRec* slots; const HintColRec* cols;
  uint32_t n_slots;
  uint32_t m_begin, m_commit, m_insert, m_update, m_delete, m_truncate, m_relation, m_rts, m_row, m_cell;
  unsigned long long* out;
};

struct CutJob {            // write_events cut points (etlg_batch_cuts: k_cut_* in finish.hip); k, a, e below are LOCAL indexes, event - first
  const unsigned long long* hints;   // the batch's hints, n_events entries (k_size_hints' format)
  uint64_t first, n;                 // the range [first, first + n)
  uint64_t budget, carry_in;
  uint32_t tile, n_tiles;            // events per scan tile; ceil(n / tile)
  unsigned long long* tsum;          // per tile: the sum of its hints; after k_cut_scan the sum of the tiles before it
  unsigned long long* tinc;          // per tile: the first local index with ETLG_SIZE_HINT_INCOMPLETE, ~0 none
  unsigned long long* q;             // n + 1 entries: q[0] = 0, q[k + 1] = the hints of [first, first + k] summed
  unsigned long long* hdr;           // [0] L = stop_event - first, [1] total = q[L], [2] n_cuts, [3] carry_out, [4] the first cut (local)
  uint32_t* jump;                    // levels x (L + 2): level k maps the start a of a batch to the start 2^k cuts on; L + 1 = no such cut
  uint64_t L;                        // (the host has read hdr[0] by the time it launches the kernels that take it from here)
  uint32_t levels;
  unsigned long long* cuts; uint64_t cuts_cap;
};

// The write_events pass plan (etlg_batch_outline: k_ol_* in finish.hip). k below is a LOCAL index, event - first. The host has set the
// scratch parts up: bitmap, crow, touched and hdr zero; bad, cfirst, de and re all ones. Nothing leaves the scratch before k_ol_fix, and
// no kernel behind k_ol_mark writes anything once *bad names a cut.
enum : uint32_t { OL_H_PASSES = 0, OL_H_TRUNC = 1, OL_H_REL = 2, OL_H_ROWS = 3, OL_H_RANGES = 4, OL_H_WORDS = 5 };
constexpr uint32_t kOlLdsSlots = 64;   // distinct slots a tile's census aggregates in LDS; the rest goes to global atomics one by one
struct OutlineJob {
  const uint8_t* ev_kind; const uint8_t* ev_flags; const uint32_t* ev_slot; const uint32_t* ev_table; const uint64_t* ev_body; const uint8_t* fixed;
  uint64_t first, n;                  // the window [first, first + n)
  const unsigned long long* cuts; uint64_t n_cuts;
  uint32_t inline_rel;                // ETLG_OL_RELATIONS_INLINE: 'R' is class 0
  uint32_t n_slots, W;                // slots the census covers; touched words per pass
  uint32_t tile, n_tiles;             // events per tile; ceil(n / tile)
  unsigned long long* hdr;            // OL_H_*
  unsigned long long* bad;            // the lowest index of a bad cut, ~0 none
  uint32_t* bitmap;                   // bit k: a write_events range starts at local event k (n / 32 + 1 words)
  unsigned long long* tsum;           // per tile: pass starts, truncate entries, Relations, rows; after k_ol_scan those in front of the tile
  unsigned long long* crow; unsigned long long* cfirst;   // the census, n_slots x 6 each
  unsigned long long* de; unsigned long long* re;   // per written pass: data_end / rel_end where a lane raised the class, else ~0 (null without passes_out)
  unsigned long long* tf;             // passes_cap + 1: truncate entries in front of the pass (null without passes_out)
  unsigned long long* touched;        // passes_cap x W, k_ol_fix copies the written passes out (null without touched_out)
  unsigned long long* passes_out; unsigned long long* ends_out; unsigned long long* touched_out; uint64_t passes_cap;   // 7 words per pass
  unsigned long long* trunc_out; uint64_t trunc_cap;                                                                    // 2 words per entry
  unsigned long long* slots_out;      // 12 words per slot
};

// The DuckLake atomic-batch plan (etlg_ducklake_plan: k_dlp_* in finish.hip). hdr: the four counts start as zeros, the four status
// words — the lowest bad pass, the lowest refused event * 4 + its reason, the lowest not-prefix event, the lowest event without a record —
// as all ones. No kernel behind the one that sets a status word writes an output once one of them is set.
enum : uint32_t { DLP_H_MEMBERS = 0, DLP_H_RETAINED = 1, DLP_H_BATCHES = 2, DLP_H_OPS = 3, DLP_H_BAD = 4, DLP_H_REFUSED = 5, DLP_H_NOTPREFIX = 6, DLP_H_NEEDSHOST = 7, DLP_H_WORDS = 8 };
constexpr uint32_t kDlpGroup = 16;        // CDC_MUTATION_BATCH_SIZE (ducklake/batches.rs:79)
constexpr uint32_t kDlpBatchWords = 13;   // etlg_dl_batch
constexpr uint32_t kDlpOpWords = 4;       // etlg_dl_op
struct DlpRecs { const unsigned long long* row_event; uint64_t n_rows; uint32_t given, _pad; };   // one etlg_batch_duckdb object's row_event
struct DlpJob {
  const uint8_t* ev_kind; const uint8_t* ev_flags; const uint32_t* ev_slot; const uint64_t* ev_start; const uint64_t* ev_commit; const uint64_t* ev_ord;
  uint64_t n_events;
  const unsigned long long* passes; uint64_t n_passes;   // etlg_outline_pass: 7 words, the window is words 0 and 1
  uint32_t slot, no_ident;            // no_ident: the slot has no identity column, every Update / Delete is refused
  uint32_t has_wm, tile, n_tiles, _pad;
  uint64_t wm_lsn, wm_ord, seed;
  DlpRecs t, p, u;                    // ETLG_DL_TUPLES / _PREDICATES / _UPDATES
  unsigned long long* hdr;            // DLP_H_*
  unsigned long long* tsum;           // per tile: members, retained; after k_dlp_scan those in front of the tile
  uint8_t* code;                      // per event: 1 member | 2 retained | category << 2
  unsigned long long* rpre;           // n_events + 1: retained members in front of the event
  uint32_t* glens; const int64_t* gpre;   // per pass: its groups, and (n_passes + 1) the groups in front of it
  unsigned long long* dense;          // the retained members' events, in order
  unsigned long long* gstart;         // per group, and one more: where its members begin in `dense`
  unsigned long long* mpos;           // per retained member: its record in tuples (updates: the SET record), its record in predicates; ~0 none
  uint32_t* oplens; const int64_t* opre;  // per group (n_events entries, 0 behind the last group): its ops, and the ops in front of it
  unsigned long long* ranges_out; unsigned long long* batches_out; uint64_t batches_cap;   // 3 and kDlpBatchWords words per group
  unsigned long long* ops_out; uint64_t ops_cap;                                           // kDlpOpWords words per op
};

// The Snowflake row-batch plan (etlg_snowflake_plan: k_sfp_* in finish.hip). hdr: four counts and the ROW_TOO_LARGE length start as
// zeros, the four status words — the lowest bad pass, the lowest failing event * 4 + its reason, the lowest not-prefix event, the lowest
// retained event without a row — as all ones. No kernel behind the one that sets a status word writes an output once one of them is set.
enum : uint32_t { SFP_H_MEMBERS = 0, SFP_H_RETAINED = 1, SFP_H_SEGS = 2, SFP_H_BYTES = 3, SFP_H_BAD = 4, SFP_H_FAILED = 5, SFP_H_NOTPREFIX = 6, SFP_H_NEEDSHOST = 7,
                  SFP_H_ROWBYTES = 8, SFP_H_WORDS = 16 };
constexpr uint32_t kSfpSegWords = 13;     // etlg_sf_segment
constexpr uint32_t kSfpWinWords = 7;      // etlg_sf_window
struct SfpJob {
  const uint8_t* ev_kind; const uint8_t* ev_flags; const uint32_t* ev_slot; const uint64_t* ev_commit; const uint64_t* ev_ord;
  uint64_t n_events;
  const unsigned long long* passes; uint64_t n_passes;   // etlg_outline_pass: 7 words, the window is words 0 and 1
  const unsigned long long* row_event; const unsigned long long* q;   // the NDJSON object: n_rows events, n_rows + 1 offsets (the prefix sums of the row lengths)
  uint64_t n_rows;
  uint32_t slot, has_c, zero_keys, tile, n_tiles, levels;   // zero_keys: a table-copy batch, every key is (0, 0)
  uint64_t c_lsn, c_ord, flush, max_row;
  unsigned long long* hdr;            // SFP_H_*
  unsigned long long* tsum;           // per tile: members, retained; after k_sfp_scan those in front of the tile
  uint8_t* code;                      // per event: 1 member | 2 retained
  unsigned long long* pre;            // 2 x (n_events + 1): members and retained members in front of the event
  unsigned long long* wrow;           // per window: first_row, end_row
  uint32_t* slens; const int64_t* spre;   // per window: its segments, and (n_passes + 1) the segments in front of it
  uint32_t* jump;                     // levels x (n_rows + 2): next^(2^k) of every row; n_rows + 1 is the end
  unsigned long long* segs_out; uint64_t segs_cap; unsigned long long* windows_out;
};

// The ClickHouse statement plan (etlg_clickhouse_plan: k_chp_* in finish.hip). hdr: three counts start as zeros, the three status words
// — the lowest bad pass, the lowest failing event * 8 + its reason, the lowest member that does not fail and has no row — as all ones;
// the two windows that hold the events of the latter two are written by k_chp_scan. No kernel behind the one that sets a status word
// writes an output once one of them is set.
enum : uint32_t { CHP_H_MEMBERS = 0, CHP_H_STMTS = 1, CHP_H_BYTES = 2, CHP_H_BAD = 4, CHP_H_FAILED = 5, CHP_H_NEEDSHOST = 6, CHP_H_FAILPASS = 8, CHP_H_NOROWPASS = 9,
                  CHP_H_WORDS = 16 };
constexpr uint32_t kChpStmtWords = 7;     // etlg_ch_statement
constexpr uint32_t kChpWinWords = 6;      // etlg_ch_window
struct ChpJob {
  const uint8_t* ev_kind; const uint8_t* ev_flags; const uint32_t* ev_slot;
  uint64_t n_events;
  const unsigned long long* passes; uint64_t n_passes;   // etlg_outline_pass: 7 words, the window is words 0 and 1
  const unsigned long long* row_event; const unsigned long long* q;   // the RowBinary object: n_rows events, n_rows + 1 offsets (the prefix sums of the row lengths)
  uint64_t n_rows;
  uint32_t slot, tile, n_tiles, levels;
  uint32_t rows;                      // the object has rows (status ETLG_RB_OK); 0: only the statuses in front of NEEDS_HOST are worked out
  uint32_t replacing, ident_ok, width_ok;   // the object's engine is ReplacingMergeTree; the slot's identity is PrimaryKey or Full; it has as many identity as primary-key columns
  uint64_t budget;                    // max_bytes_per_insert
  unsigned long long* hdr;            // CHP_H_*
  unsigned long long* tsum;           // per tile: members; after k_chp_scan those in front of the tile
  uint8_t* code;                      // per event: 1 member
  unsigned long long* pre;            // n_events + 1: members in front of the event
  unsigned long long* wrow;           // per window: first_row, end_row
  uint32_t* slens; const int64_t* spre;   // per window: its statements, and (n_passes + 1) the statements in front of it
  uint32_t* jump;                     // levels x (n_rows + 2): next^(2^k) of every row; n_rows + 1 is the end
  unsigned long long* stmts_out; uint64_t stmts_cap; unsigned long long* windows_out;
};

// The BigQuery request plan (etlg_bigquery_plan: k_bqp_* in finish.hip). hdr as ChpJob's — counts that start as zeros, the three status
// words (the lowest bad pass, the lowest failing event * 8 + its reason, the lowest member that does not fail and has no row) as all
// ones, the two windows of the latter two events written by k_bqp_scan — with the counts an event of two rows adds and the two figures
// of a table-copy batch. The words the kernels share with the ClickHouse plan (plan_* in finish.hip) keep ChpJob's names and numbers.
enum : uint32_t { BQP_H_MEMBERS = 0, BQP_H_REQS = 1, BQP_H_BYTES = 2, BQP_H_ROWS = 3, BQP_H_BAD = 4, BQP_H_FAILED = 5, BQP_H_NEEDSHOST = 6, BQP_H_FAILPASS = 8,
                  BQP_H_NOROWPASS = 9, BQP_H_TWOROW = 10, BQP_H_EST = 11, BQP_H_TARGET = 12, BQP_H_WORDS = 16 };
static_assert((uint32_t)BQP_H_BAD == (uint32_t)CHP_H_BAD && (uint32_t)BQP_H_FAILED == (uint32_t)CHP_H_FAILED && (uint32_t)BQP_H_NEEDSHOST == (uint32_t)CHP_H_NEEDSHOST,
              "chp_mark / chp_write in finish.hip serve both jobs");
constexpr uint32_t kBqpReqWords = 8;      // etlg_bq_request
constexpr uint32_t kBqpWinWords = 7;      // etlg_bq_window
struct BqpJob {
  const uint8_t* ev_kind; const uint8_t* ev_flags; const uint32_t* ev_slot;
  uint64_t n_events;
  const unsigned long long* passes; uint64_t n_passes;   // etlg_outline_pass: 7 words, the window is words 0 and 1
  const unsigned long long* row_event; const unsigned long long* q;   // the protobuf object: n_rows events (an event may own two consecutive rows), n_rows + 1 offsets
  uint64_t n_rows;
  uint32_t slot, tile, n_tiles;
  uint32_t rows;                      // the object has rows (status ETLG_RB_OK); 0: only the statuses in front of NEEDS_HOST are worked out
  uint32_t ident_pk, width_ok;        // the slot's identity is PrimaryKey; it has as many identity as primary-key columns
  uint64_t budget;                    // max_batch_bytes (a table-copy batch only)
  unsigned long long* hdr;            // BQP_H_*
  unsigned long long* tsum;           // per tile: members; after k_bqp_scan those in front of the tile
  uint8_t* code;                      // per event: 1 member
  unsigned long long* pre;            // n_events + 1: members in front of the event
  unsigned long long* wrow;           // per window: first_row, end_row
  uint32_t* slens; const int64_t* spre;   // per window: 1 when it has a request, and (n_passes + 1) the requests in front of it
  unsigned long long* reqs_out; uint64_t reqs_cap; unsigned long long* windows_out;
};

// The Iceberg write plan (etlg_iceberg_plan: k_icp_* in finish.hip). hdr as BqpJob's: counts that start as zeros, the three status
// words as all ones, the two windows of the failing event and of the member without a row written by k_icp_scan. Two things are new.
// The event side keeps a second prefix, of the events of the slot's TABLE under another slot (bit 1 of the code byte). The bitmap side
// counts bits in row ranges of the changelog object's bitmaps: every bitmap that can hold a counted bit — a validity with nulls, a
// `deferred` with deferred cells, a child validity with null elements — is a run of 64-bit words in ONE word space (`base`: where its
// words start there), and bpre is the running count of set bits in front of every word of that space.
enum : uint32_t { ICP_H_MEMBERS = 0, ICP_H_WRITES = 1, ICP_H_MIXED = 2, ICP_H_ROWS = 3, ICP_H_BAD = 4, ICP_H_FAILED = 5, ICP_H_NEEDSHOST = 6, ICP_H_FAILPASS = 8,
                  ICP_H_NOROWPASS = 9, ICP_H_WORDS = 16 };
static_assert((uint32_t)ICP_H_BAD == (uint32_t)CHP_H_BAD && (uint32_t)ICP_H_FAILED == (uint32_t)CHP_H_FAILED && (uint32_t)ICP_H_NEEDSHOST == (uint32_t)CHP_H_NEEDSHOST,
              "chp_mark / chp_write in finish.hip serve this job too");
constexpr uint32_t kIcpWriteWords = 7;    // etlg_ice_write
constexpr uint32_t kIcpWinWords = 6;      // etlg_ice_window
constexpr uint32_t kIcpSliceWords = 7;    // etlg_ice_slice
constexpr uint32_t kIcpNoBitmap = ~0u;
struct IcpBitmap { const unsigned long long* words; uint64_t base; };   // a scanned bitmap: its words (8-byte aligned) and where they start in the word space
struct IcpCol {                       // a column of the object, as k_icp_slices reads it
  const long long* offsets;           // var-len kinds and lists: n_rows + 1
  const long long* child_offsets;     // a list with a var-len child: child_count + 1
  uint64_t child_count;
  uint32_t kind, child_kind;          // etlg_arrow_kind
  uint32_t width, child_width;        // bytes of a fixed-width value / list element; 0: bit-packed or var-len
  uint32_t bm_valid, bm_deferred, bm_child, pad_;   // index into `bitmaps`; kIcpNoBitmap: the count is 0 without a read
};
struct IcpJob {
  const uint8_t* ev_kind; const uint8_t* ev_flags; const uint32_t* ev_slot; const uint32_t* ev_table;
  uint64_t n_events;
  const unsigned long long* passes; uint64_t n_passes;   // etlg_outline_pass: 7 words, the window is words 0 and 1
  const unsigned long long* row_event;                   // the changelog object: n_rows events, one row per event
  uint64_t n_rows;
  uint32_t slot, table_id, tile, n_tiles;
  uint32_t n_cols, n_bitmaps;
  const IcpCol* cols; const IcpBitmap* bitmaps;          // n_cols; n_bitmaps, and one more whose base is the word space's end
  uint64_t n_words; uint32_t wtile, n_wtiles;            // the word space, the words per tile of its scan, its tiles
  unsigned long long* hdr;            // ICP_H_*
  unsigned long long* tsum;           // per tile: members; after k_icp_scan those in front of the tile
  unsigned long long* fsum;           // per tile: events of the table under another slot; after k_icp_scan those in front of the tile
  unsigned long long* bsum;           // per word tile: set bits; after k_icp_scan those in front of the tile
  uint8_t* code;                      // per event: 1 member | 2 an Insert / Update / Delete of the table under another slot
  unsigned long long* pre;            // n_events + 1: members in front of the event
  unsigned long long* fpre;           // n_events + 1: events of the table under another slot in front of the event
  unsigned long long* bpre;           // n_words + 1: set bits in front of the word
  unsigned long long* wrow;           // per window: first_row, end_row, other_slot_event
  uint32_t* slens; const int64_t* spre;   // per window: 1 when it has a write, and (n_passes + 1) the writes in front of it
  unsigned long long* writes_out; uint64_t writes_cap; unsigned long long* slices_out; unsigned long long* windows_out;
};

// Source payload accounting (etlg_batch_payload). The frame side (k_payf_* in kernels.hip) measures every row message and lists the
// frames that take a transaction ordinal; the event side (k_paye_* in finish.hip) joins every event to its frame through that list and
// sums the ranges. Channels: 0 Insert, 1 Update, 2 Delete; a table-copy batch has channel 0 alone and reports it as ETLG_PK_COPY.
constexpr uint32_t kPayBad = 0xFFFFFFFFu;   // fbytes of a row message that does not parse, or of a copy row whose offsets do not hold
constexpr uint32_t kPayBuckets = 65;        // 64 bounds at the most, and the overflow bucket
enum : uint32_t { PAY_H_BYTES = 0, PAY_H_ROWS = 4, PAY_H_COUNTS = 8, PAY_H_MISMATCH = 9, PAY_H_BAD_CUTS = 10, PAY_H_WORDS = 11 };
struct PayJob {
  const uint8_t* in; const uint32_t* offs; const uint8_t* f_tag; uint64_t in_len;   // the input the batch was decoded from, and k_classify's tags
  uint32_t n_frames;         // frames the batch consumed (view.n_frames): the ordinals and the Begins are counted over them
  uint32_t n_recv;           // frames the received side measures: n_frames, + 1 when the failing frame had recorded its metrics
  uint32_t copy;             // table-copy batch: frame f is row f, its bytes offs[f + 1] - offs[f]
  uint32_t tile, n_tiles;    // frames per tile; ceil(n_recv / tile)
  const unsigned long long* bounds; uint32_t n_bounds;
  uint32_t* fbytes;          // per frame of [0, n_recv): the value bytes of a row message, 0 for any other frame, or kPayBad
  unsigned long long* tcnt;  // per tile: ordinal-taking frames | Begin frames << 32; after k_payf_scan the counts in front of the tile
  uint32_t* r2f;             // rank among the ordinal-taking frames -> frame
  uint32_t* brank;           // j-th Begin frame -> its rank
  unsigned long long* hdr;   // PAY_H_*: received bytes[4], rows[4]; ordinal-taking frames | Begin frames << 32; first mismatching event; bad cuts
  unsigned long long* hist;  // 4 x (n_bounds + 1) counts
  const uint8_t* ev_kind; const unsigned long long* ev_ord; uint64_t n_events;
  uint64_t entry_ord;        // the transaction ordinal the batch started from (events in front of its first Begin)
  uint32_t etile, n_etiles;  // events per tile; ceil(n_events / etile)
  unsigned long long* etb;   // per event tile: its 'B' events; after k_paye_scan those in front of it
  uint32_t* ev_bytes;        // per event: the value bytes of its message
  unsigned long long* tsum;  // per event tile: bytes[3], rows[3] of the channels; after k_paye_sums those in front of it (null: no range sums)
  unsigned long long* pb; uint32_t* pr;   // 3 x (n_events + 1) prefix sums of the channels' bytes and rows
  const unsigned long long* cuts; uint64_t n_cuts;
  unsigned long long* sums;  // n_cuts + 1 x etlg_payload_sums
};

struct FinJob {            // the finish pass (k_fin_count / k_fin_fill, finish.hip)
  const uint8_t* ev_kind; const uint8_t* ev_flags; const uint32_t* ev_slot; const uint64_t* ev_body;
  uint8_t* fixed; uint8_t* heap;
  uint64_t n_events;
  const SlotRec* slots; const ColRec* cols;   // per host slot, per column
  const uint32_t* fin;     // the finishable columns of every slot (indexes into the slot's columns)
  uint32_t n_slots, maxfin, what;
  uint32_t* lens; const int64_t* offsets;
  uint32_t* counts;        // elements of every array the count pass sized (the fill pass lays the entry out without another walk)
  uint64_t heap_base;      // where the appended entries start
  unsigned long long* stats;   // [0] deferred cells examined, [1] arrays typed, [2] floats settled, [3] left deferred
};

struct RbJob {             // ClickHouse RowBinary rows (k_rb_rows)
  const uint8_t* fixed; const uint8_t* heap; const uint64_t* row_event; const uint64_t* row_base;
  const uint8_t* ev_kind; const uint64_t* ev_commit; const uint64_t* ev_ord;
  uint64_t n_rows;
  uint32_t n_cols, engine;         // engine: 0 MergeTree, 1 ReplacingMergeTree
  uint32_t cdc_nullable;           // bit 0 / 1: the first / second trailing CDC column is Nullable() in the destination
  uint32_t format;                 // FMT_*: ClickHouse RowBinary, BigQuery protobuf (prost wire format), Snowflake NDJSON, DuckLake SQL literals
  const uint32_t* cols;            // per replicated column: cls | nullable << 8 | off_full << 16
  const uint32_t* kcols;           // per replicated column, for key images: identity | source nullable << 1 | primary key << 2 | key_index << 8 | off_key << 16
  const uint8_t* ev_flags;
  uint32_t* lens; const int64_t* offsets; uint8_t* out;
  unsigned long long* err;         // min over failing cells of rb_report_pack(); ~0 = none
  uint32_t has_json;               // the table has a json / jsonb column: the kernels that carry json_display
  uint32_t qparts, parts;          // the counting pass notes where the row's qparts pieces begin (4; 2 / 1 for narrow tables); the byte pass writes a row with parts lanes (1, 2, 4 <= qparts)
  uint32_t* part_off;              // [(qparts - 1) x n_rows]: where pieces 1 .. of a row begin, in bytes from the row's start
  // FMT_NDJSON (nd_row): the escaped `"name":` key of every column (key_off: n_cols + 1 byte offsets into keys), and
  // whether the batch is a table copy (every row's sequence number is the zero token)
  const uint8_t* nd_keys; const uint32_t* nd_key_off;
  uint32_t nd_zero_token;
  // FMT_ROWBINARY / FMT_PROTOBUF on a table-copy batch (etlg_copy_decode): the tail of a copied row, not of a CDC row — RowBinary: the CDC columns of
  // (Insert, commit_lsn 0, tx_ordinal 0) (clickhouse/core.rs:739-773); protobuf: _CHANGE_TYPE alone, no _CHANGE_SEQUENCE_NUMBER field
  // (bigquery/core.rs:602-649). Uniform over the launch: the counting pass and the byte pass read the same word
  uint32_t copy_tail;
  // FMT_DUCKLAKE (dl_row): nd_keys are the quoted identifiers; dl_what is DL_ROW_*. DL_ROW_UPDATES: a row whose base carries
  // kPbSecond is a predicate over the identity columns, any other row the SET clause `"c" = lit, ...` of the cells that are not MISSING
  uint32_t dl_what, _pad;
  // col_ends (DL_ROW_UPDATES, else null): [n_rows x n_cols] bytes of a record written once a column is done, from the counting pass
  uint32_t* col_ends;
};

struct FpRecs {            // the device-resident arrays of one etlg_batch_duckdb result
  const uint64_t* row_event; const int64_t* row_offsets; const uint8_t* bytes; uint64_t n_rows;
};
struct FpJob {             // DuckLake batch identities (fingerprint.hip)
  const uint8_t* ev_kind; const uint8_t* ev_flags; const uint32_t* ev_slot; const uint64_t* ev_start; const uint64_t* ev_commit;
  uint64_t n_events;
  uint32_t slot, copy;             // copy: a table-copy batch (`P FF T FF` per row, no LSNs)
  uint32_t n_cols, n_ranges;
  FpRecs t, p, u;                  // ETLG_DL_TUPLES / _PREDICATES / _UPDATES (u.n_rows == 0 when the caller has none)
  const uint32_t* u_ends;          // col_ends of the updates [u.n_rows x n_cols]
  const uint32_t* name_len;        // per column: len(quoted name) + 3, what a SET piece holds in front of its literal
  const uint64_t* ranges;          // n_ranges x {first_event, end_event, seed}
  uint32_t* plan;                  // per event: what it hashes (FP_*) and its records' indexes {tag, t, p, u}
  uint32_t* lens; const int64_t* offs;   // per event: bytes of its stream; their exclusive scan (n_events + 1)
  uint8_t* stream;                 // the byte stream of every slot event of the batch, back to back
  uint64_t* bounds;                // n_ranges x {begin, end} in stream bytes
  uint8_t* perm;                   // per piece: the low-byte permutation (256 bytes)
  uint8_t* lin;                    // per piece: the low byte it is entered with
  uint64_t* maps;                  // per piece: {P^n, C}
  unsigned long long* result;      // [0] the first event inside a range that lacks a record (~0 none), [1 + i] fingerprint of range i
  uint32_t n_chunks;               // an upper bound of the stream's chunks (the launches' grids)
};


}  // namespace etlg
