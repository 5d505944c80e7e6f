// The pgoutput frame and transaction machinery of the decode kernels (kernels.hip, copy.hip and, through lookback.hip.h, the
// single-pass kernels): error records and the carried transaction state, the transaction scans, frame geometry, the side-table
// lookups, the message walkers, the row writers and the per-frame passes (structure, sizing, transaction check, write). The
// hand-off kernels do not include this header: they start from decoded arenas.
//
// Reference sections restated here (paths relative to the supabase/etl checkout):
//   wire grammar (A0)          postgres-replication 0.6.7 / PostgreSQL protocol docs
//   payload accounting (A3)    crates/etl/src/postgres/codec/event.rs:261-297
//   tuple -> row (A4/A5)       crates/etl/src/postgres/codec/event.rs:554-587, 938-983
//   update/delete (A11/A12)    crates/etl/src/postgres/codec/event.rs:437-527, 605-923
//   ownership / cache (A2/A14) crates/etl/src/replication/apply.rs:2836-2867, 3514-3519, 3705-3734
#pragma once
#include "values.hip.h"

namespace etlg {

DEV void record_error(const DecParams& p, uint32_t frame, uint32_t rank, uint32_t code) {
  unsigned long long key = ((unsigned long long)frame << 16) | ((unsigned long long)rank << 8) | code;
  atomicMin(&p.res->first_err, key);
}

// ETLG_F_ASYNC batches are chained on the device: the transaction state a batch starts from is what the batch before it
// left in its result block (stream order), not what the host knew when it enqueued this one.
// Returns false when that batch did not produce a result (an error, a plan that did not hold, a predecessor that failed in turn):
// this one must not run either — the host decodes both again, in order, when they are synced (DevResult.fused_fail bit 3).
// (bit 1 alone — a fixed-width plan that gave its batch up over a shape it does not cover — is not a reason to stop: that kernel has
// published the three words from the Begin / Commit frames it read. The host keeps this batch's result only if the second attempt at
// that batch leaves the same words: finish_batch, `spare`; otherwise this batch is decoded again as it always was.)
// The rule on its own, for a kernel that fetches the block's words itself (plan.hip: with everything else its prologue loads).
DEV bool carry_usable(uint32_t fused_fail, unsigned long long first_err) { return (fused_fail & ~2u) == 0 && first_err == kNoErr; }
DEV bool load_carry(DecParams& p) {
  if (!p.carry) return true;
  const bool ok = carry_usable(p.carry->fused_fail, p.carry->first_err);
  p.in_txn = p.carry->out_in_txn; p.final_lsn = p.carry->out_final_lsn; p.next_ord = p.carry->out_next_ord;
  if (!ok && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&p.res->fused_fail, 8u);
  return ok;
}

// device slot index -> the slot id the arenas name (DevSlot.host_id); negative values (lookup failures) pass through
DEV uint32_t slot_host_id(const DecParams& p, int sl) { return sl >= 0 ? p.slots[sl].host_id : (uint32_t)sl; }

// ------------------------------------------------------------- transaction scans
// Exclusive sum scan of three u32 values at once (one LDS exchange, two barriers).
// lds: 3 * nwaves words. tot[k] = workgroup totals.
DEV void block_scan3_excl(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t* lds, uint32_t tot[3]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (int)(blockDim.x >> 6);
  const uint32_t ia = wave_scan_add(a), ib = wave_scan_add(b), ic = wave_scan_add(c);
  if (lane == 63) { lds[3 * wave] = ia; lds[3 * wave + 1] = ib; lds[3 * wave + 2] = ic; }
  __syncthreads();
  uint32_t pa = 0, pb = 0, pc = 0, ta = 0, tb = 0, tc = 0;
  for (int w = 0; w < nw; w++) {
    const uint32_t xa = lds[3 * w], xb = lds[3 * w + 1], xc = lds[3 * w + 2];
    if (w < wave) { pa += xa; pb += xb; pc += xc; }
    ta += xa; tb += xb; tc += xc;
  }
  __syncthreads();
  a = pa + ia - a; b = pb + ib - b; c = pc + ic - c;
  tot[0] = ta; tot[1] = tb; tot[2] = tc;
}

// Transaction scan: inclusive segmented count + EXCLUSIVE running max in one exchange.
// lds: 2 * nwaves words.
DEV void block_scan_txn(uint32_t cnt, uint32_t mark, uint32_t* lds, uint32_t& seg_incl, uint32_t& mark_excl,
                        uint32_t& tot_cnt, uint32_t& tot_mark) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (int)(blockDim.x >> 6);
  const uint32_t ic = wave_scan_incl(cnt, [](uint32_t a, uint32_t b) { return seg_combine(a, b); }, 0u);
  const uint32_t im = wave_scan_max(mark);
  // exclusive running max: the previous lane's inclusive value (wave_shr:1, 0 into lane 0)
  uint32_t pm = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)im, 0x138, 0xF, 0xF, false);
  if (lane == 63) { lds[2 * wave] = ic; lds[2 * wave + 1] = im; }
  __syncthreads();
  uint32_t pc = 0, pmx = 0, tcn = 0, tmx = 0;
  for (int w = 0; w < nw; w++) {
    const uint32_t xc = lds[2 * w], xm = lds[2 * w + 1];
    if (w < wave) { pc = seg_combine(pc, xc); pmx = pmx > xm ? pmx : xm; }
    tcn = seg_combine(tcn, xc); tmx = tmx > xm ? tmx : xm;
  }
  __syncthreads();
  seg_incl = seg_combine(pc, ic);
  mark_excl = pmx > pm ? pmx : pm;
  tot_cnt = tcn; tot_mark = tmx;
}

// --------------------------------------------------------- frame geometry
// CopyData := 'd' Int32-BE(len incl. itself) payload
// payload  := 'w' u64 wal_start u64 wal_end i64 ts <pgoutput msg> | 'k' u64 i64 u8
constexpr uint32_t kHdr = 5;        // 'd' + length
constexpr uint32_t kTagOff = 30;    // offset of the pgoutput tag inside the frame
constexpr uint32_t kBodyOff = 31;   // first byte after the tag

DEV bool consumes_ordinal(uint32_t tag) {  // apply.rs:2284-2292, 2339, 2377, 2457, 2501, 2545, 2587
  return tag == 'B' || tag == 'C' || tag == 'R' || tag == 'I' || tag == 'U' || tag == 'D' || tag == 'T';
}

// ------------------------------------------------------- side-input lookups
DEV int find_table(const DecParams& p, uint32_t table_id) {
  int lo = 0, hi = (int)p.n_tables - 1;
  while (lo <= hi) {
    int mid = (lo + hi) >> 1;
    uint32_t v = p.tables[mid].table_id;
    if (v == table_id) return mid;
    if (v < table_id) lo = mid + 1; else hi = mid - 1;
  }
  return -1;
}

// should_apply_changes: apply.rs:2626-2639 -> 2836-2867 / 3514-3519
DEV bool should_apply(const DecParams& p, int ti, uint32_t table_id, uint64_t remote_final_lsn) {
  if (p.worker_kind == ETLG_WORKER_TABLE_SYNC) return p.sync_table == table_id;
  if (ti < 0) return false;
  const DevTable& t = p.tables[ti];
  if (t.state_kind == ETLG_TS_READY) return true;
  if (t.state_kind == ETLG_TS_SYNC_DONE) return t.state_lsn <= remote_final_lsn;
  return false;
}

// get_replicated_table_schema (apply.rs:3705-3734) at stream position `f`:
// the shared-table-cache entry in force just before frame f.
// returns slot >= 0, or -ETLG_E_MISSING_SHARED_STATE / -ETLG_E_WAITING_RELATION
DEV int cache_slot_before(const DecParams& p, int ti, uint32_t f) {
  if (ti < 0) return -(int)ETLG_E_MISSING_SHARED_STATE;
  const DevTable& t = p.tables[ti];
  uint32_t kind = t.init_kind;
  int slot = t.init_slot;
  // epochs are few (one per R / DDL message of this table in the batch)
  uint32_t lo = t.ep_begin, hi = t.ep_end;  // first epoch with frame >= f
  while (lo < hi) {
    uint32_t mid = (lo + hi) >> 1;
    if (p.epochs[mid].frame < f) lo = mid + 1; else hi = mid;
  }
  if (lo > t.ep_begin) { kind = p.epochs[lo - 1].kind; slot = p.epochs[lo - 1].slot; }
  if (kind == 0) return -(int)ETLG_E_MISSING_SHARED_STATE;
  if (kind == 1) return -(int)ETLG_E_WAITING_RELATION;
  return slot;
}

// The epoch created by the R message at frame f itself (nullptr if the host did not
// process it, e.g. because it lies behind the host's own error frame).
DEV const DevEpoch* epoch_at(const DecParams& p, int ti, uint32_t f) {
  if (ti < 0) return nullptr;
  const DevTable& t = p.tables[ti];
  uint32_t lo = t.ep_begin, hi = t.ep_end;
  while (lo < hi) {
    uint32_t mid = (lo + hi) >> 1;
    if (p.epochs[mid].frame < f) lo = mid + 1; else hi = mid;
  }
  if (lo < t.ep_end && p.epochs[lo].frame == f && p.epochs[lo].kind == 2) return &p.epochs[lo];
  return nullptr;
}

// ---------------------------------------------------------- message shapes
// Tuple := i16 ncols, ncols x { 'n' | 'u' | 't' i32 len bytes | 'b' i32 len bytes }
// Structural walk: bounds, tags, value bytes (calculate_tuple_bytes, codec/event.rs:261-271).
DEV bool walk_tuple(const u8*& c, const u8* e, uint32_t& ncols, uint32_t& vbytes, bool over = false) {
  if (e - c < 2) return false;
  const uint32_t n = ld_be16(c);
  c += 2;
  if (n & 0x8000u) return false;  // negative count
  ncols = n;
  for (uint32_t i = 0; i < n; i++) {
    if (c >= e) return false;
    // cell tag and length in one load where the bytes may be over-read (LDS-staged tiles)
    uint64_t head = 0;
    if (over) __builtin_memcpy(&head, c, 8);
    const uint32_t t = over ? (uint32_t)head & 0xFFu : (uint32_t)*c;
    c++;
    if (t == 'n' || t == 'u') continue;
    if (t != 't' && t != 'b') return false;
    if (e - c < 4) return false;
    const uint32_t len = over ? __builtin_bswap32((uint32_t)(head >> 8)) : ld_be32(c);
    c += 4;
    if ((len & 0x80000000u) || (uint64_t)(e - c) < len) return false;
    vbytes += len;
    c += len;
  }
  return true;
}

struct RowMsg {
  uint32_t rel_id;
  const u8* old_t;   // at the i16 column count of the old/key tuple (nullptr if none)
  const u8* new_t;   // likewise for the new tuple (nullptr for D)
  uint32_t old_kind; // ETLG_OLD_*
  uint32_t old_n, new_n;
  uint32_t vbytes;   // payload bytes (A3)
};

// I := u32 rel 'N' Tuple ; U := u32 rel ['K'|'O' Tuple] 'N' Tuple ; D := u32 rel ('K'|'O') Tuple
DEV bool parse_row_msg(uint32_t tag, const u8* b, const u8* e, RowMsg& m, bool over = false) {
  if (e - b < 5) return false;
  m.rel_id = ld_be32(b);
  const u8* c = b + 4;
  m.old_t = nullptr; m.new_t = nullptr; m.old_kind = ETLG_OLD_NONE; m.old_n = m.new_n = 0; m.vbytes = 0;
  uint32_t t = *c++;
  if (tag == 'I') {
    if (t != 'N') return false;
    m.new_t = c;
    return walk_tuple(c, e, m.new_n, m.vbytes, over);
  }
  if (tag == 'U') {
    if (t == 'K' || t == 'O') {
      m.old_kind = t == 'K' ? ETLG_OLD_KEY : ETLG_OLD_FULL;
      m.old_t = c;
      if (!walk_tuple(c, e, m.old_n, m.vbytes, over)) return false;
      if (c >= e) return false;
      t = *c++;
    }
    if (t != 'N') return false;
    m.new_t = c;
    return walk_tuple(c, e, m.new_n, m.vbytes, over);
  }
  // 'D'
  if (t != 'K' && t != 'O') return false;
  m.old_kind = t == 'K' ? ETLG_OLD_KEY : ETLG_OLD_FULL;
  m.old_t = c;
  return walk_tuple(c, e, m.old_n, m.vbytes, over);
}

DEV bool has_cstr(const u8*& c, const u8* e) {
  while (c < e) if (*c++ == 0) return true;
  return false;
}

// Cell iterator over a structurally valid tuple.
struct CellIt {
  const u8* c;
  DEV void begin(const u8* tuple) { c = tuple + 2; }
  DEV uint32_t next(const u8*& data, uint32_t& len) {
    const uint32_t t = *c++;
    data = nullptr; len = 0;
    if (t == 't' || t == 'b') { len = ld_be32(c); c += 4; data = c; c += len; }
    return t;
  }
};

// ---------------------------------------------------------------- k_size
// Heap bytes of one tuple decoded against `n` schema columns.
//   mode 0: full row (convert_tuple_to_row); mode 1: dense key tuple;
//   mode 2: full-width key tuple (non-identity positions skipped unread);
//   mode 3: update new tuple (u cells never allocate: alias or Missing)
template <uint32_t VAR = 0>
DEV uint32_t tuple_heap_bytes(const DecParams& p, const DevSlot& s, const u8* tuple, uint32_t ncells, int mode, bool over = false) {
  if (!s.has_var) return 0;  // fixed-width schema: no cell can reach the heap
  const DevCol* cols = p.cols + s.cols_base;
  CellIt it; it.begin(tuple);
  uint32_t h = 0, next_ident = 0;
  for (uint32_t i = 0; i < ncells; i++) {
    const u8* d; uint32_t len;
    const uint32_t t = it.next(d, len);
    uint32_t ci;
    if (mode == 1) {
      // i-th identity column
      ci = 0xFFFFFFFFu;
      for (uint32_t c = 0, k = 0; c < s.n_cols; c++) if (cols[c].identity) { if (k == i) { ci = c; break; } k++; }
      if (ci == 0xFFFFFFFFu) break;
    } else {
      if (i >= s.n_cols) break;
      ci = i;
      if (mode == 2) { if (!cols[ci].identity) continue; next_ident++; }
    }
    if (t == 't') h += cell_heap_bytes<VAR>(cols[ci].cls, d, len, over);
  }
  (void)next_ident;
  return h;
}

// ---------------------------------------------------------------- k_write
// One row image out of one tuple. `mode`:
//   ROW_FULL    convert_tuple_to_row (codec/event.rs:554-587), full layout
//   ROW_KEY     normalize_key_tuple_to_row (codec/event.rs:795-923), key layout (dense or full-width tuple)
//   ROW_UPDATE  convert_update_tuple_to_updated_table_row + OldRowResolver (codec/event.rs:605-791):
//               'u' cells alias the aligned old value (Cell::clone) or become MISSING (Partial)
// A single body (one inlined copy of the value codec) serves all three.
enum : uint32_t { ROW_FULL = 0, ROW_KEY = 1, ROW_UPDATE = 2 };

// CHECK (ETLG_F_CHECK_CELLS, the multi-pass kernels only: kernels.hip): a json / jsonb / array cell is validated where it is deferred,
// behind its UTF-8 check, with the code parse_cell_from_postgres_text would raise (cell_text_error, cellparse.hip.h). A compile-time
// choice: the single-pass kernels instantiate CHECK = false and carry no trace of it.
template <bool CHECK = false, uint32_t VAR = 0>
DEV uint32_t write_row(const DecParams& p, const DevSlot& s, uint32_t mode, const u8* tuple, uint32_t ncells, u8* row,
                       uint32_t old_kind, const u8* old_row, uint32_t& hcur, bool& partial, bool over = false) {
  bool dense = false;
  if (mode == ROW_KEY) {
    if (s.n_ident == 0) return ETLG_E_KEY_MISSING_COLS;
    dense = ncells == s.n_ident;
    if (!dense && ncells != s.n_cols) return ETLG_E_KEY_SHAPE;
  } else if (ncells != s.n_cols) {
    return ETLG_E_TUPLE_WIDTH;
  }
  const DevCol* cols = p.cols + s.cols_base;
  StateAcc sa{(uint32_t*)row};
  CellIt it; it.begin(tuple);
  uint32_t ci = 0;  // schema column cursor (dense key tuples walk identity columns only)
  const uint32_t n_out = mode == ROW_KEY ? s.n_ident : s.n_cols;
  // A decoded old row always has exactly n_cols (Full) / n_ident (Key) cells, so the
  // resolver's width checks (codec/event.rs:700-710, 730-740, 772-785) cannot fire here.
  for (uint32_t i = 0; i < ncells; i++) {
    const u8* d; uint32_t len;
    const uint32_t t = it.next(d, len);
    if (mode == ROW_KEY) {
      if (dense) { while (ci < s.n_cols && !cols[ci].identity) ci++; }
      else { ci = i; if (!cols[ci].identity) continue; }  // full-width key tuple: other positions are skipped unread
    } else {
      ci = i;
    }
    const DevCol col = cols[ci];
    const uint32_t k = mode == ROW_KEY ? col.key_index : i;  // output cell index
    uint32_t* slot = (uint32_t*)(row + (mode == ROW_KEY ? col.off_key : col.off_full));
    uint32_t st = ETLG_CELL_NULL;
    if (t == 'n') {  // convert_tuple_data_to_cell, codec/event.rs:945-961
      if (!col.nullable && !(p.flags & 2u)) return ETLG_E_REQUIRED_NULL;
      slot_zero(slot, col.cls);
    } else if (t == 'u') {
      if (mode == ROW_FULL) return ETLG_E_FULL_ROW_MISSING;
      if (mode == ROW_KEY) return ETLG_E_KEY_MISSING_VALUE;
      const bool from_full = old_kind == ETLG_OLD_FULL;
      const bool from_key = old_kind == ETLG_OLD_KEY && col.identity;
      if (from_full || from_key) {  // Cell::clone of the aligned old value: alias its slot
        const uint32_t oi = from_full ? i : col.key_index;
        const uint32_t* src = (const uint32_t*)(old_row + (from_full ? col.off_full : col.off_key));
        const uint32_t nw = slot_bytes(col.cls) >> 2;
        for (uint32_t w = 0; w < nw; w++) slot[w] = src[w];
        st = get_state(old_row, oi);
      } else {
        slot_zero(slot, col.cls);
        st = ETLG_CELL_MISSING;
        partial = true;
      }
    } else if (t == 't') {
      const uint32_t err = decode_text_cell<true, VAR>(col.cls, d, len, slot, p.heap, hcur, st, over);
      if (err) return err;
      if constexpr (CHECK) {
        if (class_always_deferred(col.cls)) {
          const uint32_t ce = cell_text_error(col.cls, chk_elem_table(p)[s.cols_base + ci], d, len);
          if (ce && ce < 0x100u) return ce;   // (0x100, ARR_HOST: a lane cannot decide — the cell stays DEFERRED, include/etlg.h)
        }
      }
    } else {
      return ETLG_E_BINARY_FORMAT;
    }
    sa.put(k, st, k + 1 == n_out);
    if (mode == ROW_KEY && dense) ci++;
  }
  return 0;
}

// convert_tuple_to_row for a wave whose active lanes ALL decode an INSERT of the same
// schema slot with the same column count (the common case). `slot_u` / `n` are wave-uniform
// (SGPRs): the column descriptors come through the scalar cache, the loop trip count and
// the per-column class dispatch are scalar branches, and only the data-dependent work
// (cell tag, length, characters) stays per lane. `pg` must hold GLOBAL side-table pointers.
template <uint32_t VAR = 0>
DEV uint32_t write_full_row_uniform(const DecParams& pg, uint32_t slot_u, const u8* tuple, uint32_t n, u8* row,
                                    uint32_t& hcur, bool over) {
  // The descriptors are read as whole dwords through constant-address-space pointers: the address is wave-uniform
  // and the memory is never written by a kernel, so these are s_load (scalar cache, results in SGPRs). As byte /
  // halfword fields of a plain global struct they compiled to global_load_ubyte / _ushort + s_waitcnt vmcnt(0) +
  // v_readfirstlane — one dependent vector-memory round trip per column (gfx950 has no sub-dword scalar loads).
  const ETLG_CONST_AS uint32_t* sw = (const ETLG_CONST_AS uint32_t*)(uintptr_t)(pg.slots + slot_u);
  static_assert(sizeof(DevSlot) == 44 && sizeof(DevCol) == 12, "descriptor words below");
  if (n != sw[0]) return ETLG_E_TUPLE_WIDTH;                      // DevSlot.n_cols
  const ETLG_CONST_AS uint32_t* cw = (const ETLG_CONST_AS uint32_t*)(uintptr_t)(pg.cols + sw[6]);  // DevSlot.cols_base
  struct { uint32_t cls, nullable, off_full; } col;
  const u8* c = tuple + 2;
  uint32_t acc = 0;
  uint32_t* stw = (uint32_t*)row;
  for (uint32_t i = 0; i < n; i++) {
    { const uint32_t w0 = cw[3 * i], w1 = cw[3 * i + 1]; col.cls = w0 & 0xFFu; col.nullable = (w0 >> 8) & 0xFFu; col.off_full = w1 & 0xFFFFu; }
    const uint32_t cls = col.cls;
    uint32_t* slot = (uint32_t*)(row + col.off_full);  // always the arena: a pointer that may also name private memory turns every row store into a flat store
    uint64_t head = 0;
    if (over) __builtin_memcpy(&head, c, 8);  // tag + length in one load
    const uint32_t t = over ? (uint32_t)head & 0xFFu : (uint32_t)*c;
    c++;
    uint32_t st = ETLG_CELL_NULL;
    if (t == 't') {
      const uint32_t len = over ? __builtin_bswap32((uint32_t)(head >> 8)) : ld_be32(c);
      c += 4;
      const uint32_t err = decode_text_cell<true, VAR>(cls, c, len, slot, pg.heap, hcur, st, over);
      if (err) return err;
      c += len;
    } else if (t == 'n') {
      if (!col.nullable && !(pg.flags & 2u)) return ETLG_E_REQUIRED_NULL;
      slot_zero(slot, cls);
    } else if (t == 'u') {
      return ETLG_E_FULL_ROW_MISSING;
    } else {
      return ETLG_E_BINARY_FORMAT;
    }
    acc |= st << (2 * (i & 15));
    if (((i & 15) == 15 || i + 1 == n) && !(pg.flags & 0x100u)) { stw[i >> 4] = acc; acc = 0; }
  }
  return 0;
}

// ------------------------------------------------------------ per-frame passes
// Transaction context of one frame (state BEFORE the frame is applied).
struct TxnCtx {
  bool in_txn;         // remote_final_lsn.is_some()
  uint64_t final_lsn;  // valid when in_txn
  uint64_t ord;        // ordinal this frame takes if it consumes one
};

struct FrameView {
  uint32_t f;     // frame index in the batch
  uint32_t tag;   // pgoutput tag ('k' keepalive, FT_BAD malformed)
  const u8* fr;   // first byte of the CopyData frame ('d')
  const u8* e;    // one past its last byte
};

// Structural validation of the whole message (what the third-party parser does
// before the reference sees it). For I/U/D fills `m`. Returns false on a wire error.
DEV bool frame_structure(const FrameView& v, RowMsg& m, bool over = false) {
  const u8* b = v.fr + kBodyOff;
  const u8* e = v.e;
  switch (v.tag) {
    case FT_BAD: return false;
    case 'O': { const u8* c = b + 8; return e - b >= 9 && has_cstr(c, e); }              // u64 lsn, cstr name
    case 'Y': { const u8* c = b + 4; return e - b >= 6 && has_cstr(c, e) && has_cstr(c, e); }  // u32 oid, cstr, cstr
    case 'R': return e - b >= 4;  // the rest of R is validated by the host control plane
    case 'I': case 'U': case 'D': return parse_row_msg(v.tag, b, e, m, over);
    case 'T': {  // i32 nrel, i8 options, nrel x u32
      if (e - b < 5) return false;
      const uint32_t nrel = ld_be32(b);
      return !(nrel & 0x80000000u) && (uint64_t)(e - b - 5) / 4 >= nrel;
    }
    default: return true;  // 'k', 'B', 'C' were length-checked by classify; 'M' is the host's
  }
}

// Transaction state machine + ownership + exact output sizes of one frame
// (apply.rs:2279-2617, 2836-2867). `wire_ok`/`m` come from frame_structure.
// check_txn = false: the transaction context is not known yet (fused kernel, early
// sizing); the frame is sized as if inside a transaction and txn_check_frame runs later.
template <uint32_t VAR = 0>
DEV void size_frame(const DecParams& p, const FrameView& v, const TxnCtx& tx, bool wire_ok, const RowMsg& m,
                    uint32_t& emit, uint32_t& fixed, uint32_t& heap, uint64_t pay[3], int& row_slot,
                    bool check_txn = true, bool over = false) {
  const uint32_t f = v.f, tag = v.tag;
  const u8* b = v.fr + kBodyOff;
  emit = 0; fixed = 0; heap = 0;
  if (!wire_ok) { record_error(p, f, RK_WIRE, ETLG_E_WIRE); return; }
  switch (tag) {
    case 'B': emit = 1; fixed = 8; break;
    case 'C':
      if (check_txn && !tx.in_txn) record_error(p, f, RK_TXN, ETLG_E_TXN_STATE);
      else if (check_txn && ld_be64(b + 1) != tx.final_lsn) record_error(p, f, RK_TXN, ETLG_E_COMMIT_LSN);
      else { emit = 1; fixed = 16; }
      break;
    case 'M':
      if (p.flags & 1u) record_error(p, f, RK_WIRE, ETLG_E_CTRL_HINT);
      break;  // host control plane (apply.rs:2160-2276)
    case 'R': {  // handle_relation_message: the event is emitted here, the schema work is the host's
      if (p.flags & 1u) { record_error(p, f, RK_WIRE, ETLG_E_CTRL_HINT); break; }
      if (check_txn && !tx.in_txn) { record_error(p, f, RK_TXN, ETLG_E_TXN_STATE); break; }
      const uint32_t rel = ld_be32(b);
      const DevEpoch* ep = epoch_at(p, find_table(p, rel), f);
      if (ep && ep->emit) emit = 1;
      break;
    }
    case 'I': case 'U': case 'D': {
      if (check_txn && !tx.in_txn) { record_error(p, f, RK_TXN, ETLG_E_TXN_STATE); break; }
      pay[tag == 'I' ? 0 : tag == 'U' ? 1 : 2] = m.vbytes;  // metrics precede the ownership check
      int slot;
      if (p.flags & 2u) slot = p.copy_slot;  // table-copy rows: the caller named the schema
      else {
        const int ti = find_table(p, m.rel_id);
        if (!should_apply(p, ti, m.rel_id, tx.final_lsn)) break;
        slot = cache_slot_before(p, ti, f);
        if (slot < 0) { record_error(p, f, RK_SCHEMA, (uint32_t)(-slot)); break; }
      }
      const DevSlot& s = p.slots[slot];
      row_slot = slot;
      emit = 1;
      for (uint32_t img = (tag == 'I' || m.old_kind == ETLG_OLD_NONE) ? 1u : 0u; img < (tag == 'D' ? 1u : 2u); img++) {
        const bool is_new = img == 1;
        int mode;
        if (is_new) { fixed += s.row_full; mode = tag == 'U' ? 3 : 0; }
        else if (m.old_kind == ETLG_OLD_FULL) { fixed += s.row_full; mode = 0; }
        else { fixed += s.row_key; mode = m.old_n == s.n_ident ? 1 : m.old_n == s.n_cols ? 2 : -1; }
        if (mode >= 0) heap += tuple_heap_bytes<VAR>(p, s, is_new ? m.new_t : m.old_t, is_new ? m.new_n : m.old_n, mode, over);
      }
      break;
    }
    case 'T': {
      if (check_txn && !tx.in_txn) { record_error(p, f, RK_TXN, ETLG_E_TXN_STATE); break; }
      const uint32_t nrel = ld_be32(b);
      uint32_t owned = 0;
      for (uint32_t i = 0; i < nrel; i++) {
        const uint32_t rel = ld_be32(b + 5 + 4 * i);
        const int ti = find_table(p, rel);
        if (!should_apply(p, ti, rel, tx.final_lsn)) continue;
        const int slot = cache_slot_before(p, ti, f);
        if (slot < 0) { record_error(p, f, RK_SCHEMA, (uint32_t)(-slot)); owned = 0; break; }
        owned++;
      }
      if (owned) { emit = 1; fixed = 8 * owned; }
      break;
    }
    default: break;  // 'k', 'O', 'Y'
  }
}

// The transaction-state checks of size_frame for a frame that was sized early.
DEV void txn_check_frame(const DecParams& p, const FrameView& v, const TxnCtx& tx) {
  const uint32_t tag = v.tag;
  if (tag == 'C') {
    if (!tx.in_txn) record_error(p, v.f, RK_TXN, ETLG_E_TXN_STATE);
    else if (ld_be64(v.fr + kBodyOff + 1) != tx.final_lsn) record_error(p, v.f, RK_TXN, ETLG_E_COMMIT_LSN);
  } else if (tag == 'R' || tag == 'I' || tag == 'U' || tag == 'D' || tag == 'T') {
    if (!tx.in_txn) record_error(p, v.f, RK_TXN, ETLG_E_TXN_STATE);
  }
}

// Decodes one emitting frame into the arena at (ev_idx, fx_off, hp_off).
// `pu` (optional): the same parameters with GLOBAL side-table pointers, enabling the
// wave-uniform INSERT path; `over`: the frame bytes may be over-read by up to 7 bytes.
template <bool CHECK = false, uint32_t VAR = 0>
DEV void write_frame(const DecParams& p, const FrameView& v, const TxnCtx& tx, const RowMsg& m, int row_slot,
                     uint64_t ev_idx, uint64_t fx_off, uint64_t hp_off, const DecParams* pu = nullptr, bool over = false) {
  const uint32_t f = v.f, tag = v.tag;
  const u8* fr = v.fr;
  const u8* b = fr + kBodyOff;
  u8* body = p.fixed + fx_off;
  uint32_t flags = 0, table = 0, slot_id = 0;
  uint64_t commit_lsn = tx.final_lsn;
  switch (tag) {
    case 'B':  // parse_event_from_begin_message, codec/event.rs:303-316
      commit_lsn = ld_be64(b);
      st64((uint32_t*)body, ld_be64(b + 8));
      table = ld_be32(b + 16);
      break;
    case 'C':  // parse_event_from_commit_message, codec/event.rs:322-336
      flags = b[0];
      commit_lsn = ld_be64(b + 1);
      st64((uint32_t*)body, ld_be64(b + 9));
      st64((uint32_t*)body + 2, ld_be64(b + 17));
      break;
    case 'R': {
      table = ld_be32(b);
      const DevEpoch* ep = epoch_at(p, find_table(p, table), f);
      slot_id = ep ? slot_host_id(p, ep->slot) : 0;
      break;
    }
    case 'T': {  // parse_event_from_truncate_message, codec/event.rs:533-547
      const uint32_t nrel = ld_be32(b);
      flags = b[4];
      uint32_t k = 0;
      for (uint32_t i = 0; i < nrel; i++) {
        const uint32_t rel = ld_be32(b + 5 + 4 * i);
        const int ti = find_table(p, rel);
        if (!should_apply(p, ti, rel, tx.final_lsn)) continue;
        const int sl = cache_slot_before(p, ti, f);
        ((uint32_t*)body)[2 * k] = rel; ((uint32_t*)body)[2 * k + 1] = slot_host_id(p, sl);
        k++;
      }
      table = k;
      break;
    }
    default: {  // I / U / D
      table = m.rel_id;
      const int sl = row_slot >= 0 ? row_slot : cache_slot_before(p, find_table(p, m.rel_id), f);
      slot_id = slot_host_id(p, sl);
      uint32_t hcur = (uint32_t)hp_off;
      uint32_t err = 0;
      bool partial = false;
      const uint32_t sl_u = __builtin_amdgcn_readfirstlane((uint32_t)sl);
      const uint32_t n_u = __builtin_amdgcn_readfirstlane(m.new_n);
      if (p.flags & 0x400u) { /* profiling ablation: no row decode at all */ }
      else if (p.flags & 0x800u) { if (pu && __all(tag == 'I' && (uint32_t)sl == sl_u && m.new_n == n_u)) err = write_full_row_uniform<VAR>(*pu, sl_u, m.new_t, n_u, body, hcur, over); /* ablation: uniform waves only */ }
      else if (pu && __all(tag == 'I' && (uint32_t)sl == sl_u && m.new_n == n_u)) {
        err = write_full_row_uniform<VAR>(*pu, sl_u, m.new_t, n_u, body, hcur, over);
      } else {
        const DevSlot& s = p.slots[sl];
        const uint32_t old_sz = m.old_kind == ETLG_OLD_FULL ? s.row_full : m.old_kind == ETLG_OLD_KEY ? s.row_key : 0;
        if (tag != 'I') flags = m.old_kind;
        // image 0 = old / key tuple (U, D), image 1 = new tuple (I, U): one call site for both
        for (uint32_t img = (tag == 'I' || m.old_kind == ETLG_OLD_NONE) ? 1u : 0u; img < (tag == 'D' ? 1u : 2u) && !err; img++) {
          const bool is_new = img == 1;
          const uint32_t mode = is_new ? (tag == 'U' ? (uint32_t)ROW_UPDATE : (uint32_t)ROW_FULL)
                                       : (m.old_kind == ETLG_OLD_KEY ? (uint32_t)ROW_KEY : (uint32_t)ROW_FULL);
          err = write_row<CHECK, VAR>(p, s, mode, is_new ? m.new_t : m.old_t, is_new ? m.new_n : m.old_n,
                          is_new ? body + old_sz : body, m.old_kind, body, hcur, partial, over);
        }
      }
      if (partial) flags |= ETLG_FLAG_PARTIAL;
      if (err) { record_error(p, f, RK_DECODE, err); return; }
      break;
    }
  }
  if (p.flags & 0x200u) return;  // profiling ablation (no header stores)
  p.ev_kind[ev_idx] = (u8)tag;
  p.ev_flags[ev_idx] = (u8)flags;
  p.ev_table[ev_idx] = table;
  p.ev_slot[ev_idx] = slot_id;
  p.ev_start[ev_idx] = ld_be64(fr + 6);  // wal_start (apply.rs:2039)
  p.ev_commit[ev_idx] = commit_lsn;
  p.ev_ord[ev_idx] = tx.ord;
  p.ev_body[ev_idx] = fx_off;
}

// classify from a frame pointer (LDS or global) + its sidecar extent
DEV uint32_t classify_ptr(const u8* fr, uint32_t flen) {
  if (flen < kHdr + 1 || fr[0] != 'd' || ld_be32(fr + 1) + 1u != flen) return FT_BAD;
  const uint32_t outer = fr[5];
  if (outer == 'k') return flen >= kHdr + 18 ? 'k' : FT_BAD;
  if (outer != 'w' || flen < kBodyOff) return FT_BAD;
  const uint32_t tag = fr[kTagOff];
  switch (tag) {
    case 'B': return flen >= kBodyOff + 20 ? tag : FT_BAD;  // u64 final_lsn, i64 ts, u32 xid
    case 'C': return flen >= kBodyOff + 25 ? tag : FT_BAD;  // i8 flags, u64, u64, i64
    case 'O': case 'Y': case 'R': case 'M': case 'I': case 'U': case 'D': case 'T': return tag;
    default: return FT_BAD;
  }
}

DEV uint32_t classify_frame(const DecParams& p, uint32_t f) {
  const uint32_t o0 = p.offs[f], o1 = p.offs[f + 1];
  if (o1 <= o0 || o1 > p.in_len) return FT_BAD;
  return classify_ptr(p.in + o0, o1 - o0);
}

}  // namespace etlg
