// Columnar hand-off on the device: the rows of ONE schema slot out of a decoded batch, as Arrow-layout
// column buffers — validity bitmap + values (+ 64-bit offsets for var-len columns) — built by kernels over the arena that
// is already in HBM. Replaces the per-Cell builders of the reference's sinks (rows_to_record_batch / build_array_for_field,
// crates/etl-destinations/src/iceberg/encoding.rs:34-84; cell_to_* converters :150-360) with one strided gather per column:
//
//   Bool -> Boolean (bit-packed) | I16, I32 -> Int32 | I64, U32 -> Int64 (cell_to_i32 / cell_to_i64, :157-171)
//   F32 -> Float32 | F64 -> Float64 | Date -> Date32 (days since 1970-01-01, :194) | Time -> Time64(us) (:201)
//   Timestamp -> Timestamp(us) (:208) | TimestampTz -> Timestamp(us, UTC) (:215) | Uuid -> FixedSizeBinary(16)
//   String -> LargeUtf8 | Bytes -> LargeBinary | numeric / json / arrays -> their heap entries (LargeBinary, the host finishes them)
//
// A cell the decode kernels handed back DEFERRED is null in `validity` and set in the column's `deferred` bitmap: the consumer
// finishes it from the arena (row_event names the event). Integer / byte work, HBM-bound: no MFMA.
#include "handoff.hip.h"

namespace etlg {

DEV bool col_selected(const ColSel& s, uint64_t i, uint64_t& base) {
  if (i >= s.n_events || s.ev_slot[i] != s.slot) return false;
  const uint32_t k = s.ev_kind[i], fl = s.ev_flags[i];
  base = s.ev_body[i];
  if (k == 'I') return (s.kinds & SEL_INSERT) != 0;
  if (k == 'U' && (s.kinds & SEL_UPDATE_NEW) && !(fl & ETLG_FLAG_PARTIAL)) {
    const uint32_t ok = fl & 3u;
    base += ok == ETLG_OLD_FULL ? s.row_full : ok == ETLG_OLD_KEY ? s.row_key : 0u;
    return true;
  }
  if (k == 'D' && (s.kinds & SEL_DELETE_OLD) && (fl & 3u) == ETLG_OLD_FULL) return true;
  if (k == 'D' && (s.kinds & SEL_DELETE_KEY) && (fl & 3u) == ETLG_OLD_KEY) return true;   // the key row: RowBinary expands it into the tombstone (rb_row)
  return false;
}

// ---- BigQuery: which rows an event becomes (bigquery/core.rs:978-1036, 1425-1476, 1557-1645)
// Did the update change the primary key (bigquery_primary_key_changed)? 0 no, 1 yes, 2 a cell the device does not compare.
DEV uint32_t pb_pk_changed(const ColSel& s, uint64_t oldb, uint64_t newb, bool key) {
  for (uint32_t i = 0; i < s.n_cols; i++) {
    const uint32_t kc = s.kcols[i];
    if (!(kc & 4u)) continue;
    const uint32_t cd = s.cols[i], cls = cd & 0xFFu;
    const uint32_t oi = key ? (kc >> 8) & 0xFFu : i, ooff = key ? kc >> 16 : cd >> 16;
    const uint32_t so = (s.fixed[oldb + oi / 4] >> (2 * (oi % 4))) & 3u, sn = (s.fixed[newb + i / 4] >> (2 * (i % 4))) & 3u;
    if ((so != ETLG_CELL_NULL && so != ETLG_CELL_VALUE) || (sn != ETLG_CELL_NULL && sn != ETLG_CELL_VALUE)) return 2;
    if (so != sn) return 1;
    if (so == ETLG_CELL_NULL) continue;
    const u8* a = s.fixed + oldb + ooff; const u8* b = s.fixed + newb + (cd >> 16);
    if (cls == ETLG_TC_STRING || cls == ETLG_TC_BYTEA) {
      const uint32_t la = *(const uint32_t*)(a + 4), lb = *(const uint32_t*)(b + 4);
      if (la != lb) return 1;
      const u8* ha = s.heap + *(const uint32_t*)a; const u8* hb = s.heap + *(const uint32_t*)b;
      for (uint32_t k = 0; k < la; k++) if (ha[k] != hb[k]) return 1;
    } else {
      const uint32_t nw = slot_bytes(cls) >> 2;
      for (uint32_t w = 0; w < nw; w++) if (((const uint32_t*)a)[w] != ((const uint32_t*)b)[w]) return 1;
    }
  }
  return 0;
}
// -> number of rows (0: the event stays with the host — the reference refuses it, or the device cannot decide), their bases
DEV uint32_t pb_selected(const ColSel& s, uint64_t i, unsigned long long* bases) {
  if (i >= s.n_events || s.ev_slot[i] != s.slot) return 0;
  const uint32_t k = s.ev_kind[i], fl = s.ev_flags[i], ok = fl & 3u;
  const uint64_t base = s.ev_body[i];
  if (k == 'I') { bases[0] = base; return 1; }
  if (k == 'D') {  // bigquery_delete_row: the old image's primary-key cells (a key image only under primary-key identity, :1540-1555)
    if (ok == ETLG_OLD_FULL) { bases[0] = base | kPbDelete; return 1; }
    if (ok == ETLG_OLD_KEY && s.identity_pk) { bases[0] = base | kPbDelete | kPbKey; return 1; }
    return 0;
  }
  if (k != 'U' || (fl & ETLG_FLAG_PARTIAL)) return 0;   // bigquery_update_new_row refuses partial rows (:1478-1494)
  const uint64_t newb = base + (ok == ETLG_OLD_FULL ? s.row_full : ok == ETLG_OLD_KEY ? s.row_key : 0u);
  if (ok == ETLG_OLD_NONE) {  // ensure_bigquery_update_without_old_row_can_skip_delete (:1515-1536)
    if (!s.identity_pk) return 0;
    bases[0] = newb; return 1;
  }
  if ((ok == ETLG_OLD_KEY && !s.identity_pk) || !s.pk_comparable) return 0;
  const uint32_t ch = pb_pk_changed(s, base, newb, ok == ETLG_OLD_KEY);
  if (ch == 2) return 0;
  if (ch == 1) {  // the old key goes first, the new row follows with the next ordinal (:1446-1474)
    bases[0] = base | kPbDelete | (ok == ETLG_OLD_KEY ? kPbKey : 0ull);
    bases[1] = newb | kPbSecond;
    return 2;
  }
  bases[0] = newb;
  return 1;
}

// ---- DuckLake: what an event becomes for the tuples (DL_SEL_TUPLES), for the predicates (DL_SEL_PRED_IDENT; DL_SEL_PRED_PK: a table-copy
// batch, every row) and for the partial Updates (DL_SEL_UPDATES):
// DLS_NOTHING, DLS_ROW (bases[0]: the image, | kPbKey when it has the key layout), DLS_HOST: an event the host has to take (n_host_rows),
// DLS_TWO_ROWS (DL_SEL_UPDATES only).
// Insert -> a tuple; Update -> the new row's tuple unless it is partial, and the predicate of the old image — without one, of the
// new row's identity columns (TableMutation::Replace) unless that row is partial (key_row_from_updated_partial_row); Delete -> the
// predicate of the old image, which it must carry ("DuckLake delete requires an old row image").
// DL_SEL_UPDATES, a partial Update only (ducklake/core.rs:1846-1913, batches.rs:1179-1190): the SET clause of the partial new row (bases[0]) and
// the predicate of the mutation's delete_row (bases[1], | kPbSecond): the old image, else the partial row's own identity cells. The
// host takes the event when the slot has no identity columns, when no old image came and an identity cell is MISSING (core.rs:896-905)
// and when no cell is present at all (batches.rs:1337).
DEV uint32_t dl_selected(const ColSel& s, uint64_t i, unsigned long long* bases) {
  if (i >= s.n_events || s.ev_slot[i] != s.slot) return DLS_NOTHING;
  const uint32_t k = s.ev_kind[i], fl = s.ev_flags[i], ok = fl & 3u;
  const bool partial = (fl & ETLG_FLAG_PARTIAL) != 0;
  unsigned long long& base = bases[0];
  base = s.ev_body[i];
  if (s.dl == DL_SEL_UPDATES) {
    if (k != 'U' || !partial) return DLS_NOTHING;
    if (!s.dl_ident) return DLS_HOST;   // "DuckLake update requires a replica identity"
    const uint64_t oldb = base, newb = oldb + (ok == ETLG_OLD_FULL ? s.row_full : ok == ETLG_OLD_KEY ? s.row_key : 0u);
    bool any = false, key_missing = false;
    for (uint32_t c = 0; c < s.n_cols; c++) {
      const uint32_t st = (s.fixed[newb + c / 4] >> (2 * (c % 4))) & 3u;
      if (st != ETLG_CELL_MISSING) any = true;
      else if (s.kcols[c] & 1u) key_missing = true;
    }
    if (!any || (ok == ETLG_OLD_NONE && key_missing)) return DLS_HOST;
    bases[0] = newb;
    bases[1] = (ok == ETLG_OLD_NONE ? newb : ok == ETLG_OLD_KEY ? oldb | kPbKey : oldb) | kPbSecond;
    return DLS_TWO_ROWS;
  }
  if (k == 'I') return s.dl != DL_SEL_PRED_IDENT ? DLS_ROW : DLS_NOTHING;
  if (k != 'U' && k != 'D') return DLS_NOTHING;
  if (s.dl == DL_SEL_TUPLES) {
    if (k == 'D') return DLS_NOTHING;
    if (partial) return DLS_HOST;
    base += ok == ETLG_OLD_FULL ? s.row_full : ok == ETLG_OLD_KEY ? s.row_key : 0u;
    return DLS_ROW;
  }
  if (!s.dl_ident) return DLS_HOST;   // "DuckLake delete requires a replica identity"
  if (ok == ETLG_OLD_FULL) return DLS_ROW;
  if (ok == ETLG_OLD_KEY) { base |= kPbKey; return DLS_ROW; }
  return k == 'U' && !partial ? DLS_ROW : DLS_HOST;
}
DEV uint32_t dl_rows(uint32_t dls) { return dls == DLS_ROW ? 1u : dls == DLS_TWO_ROWS ? 2u : 0u; }

// Iceberg changelog: why the sink refuses a row event of the slot that col_selected (inserts, new rows, old rows) left out (iceberg_update_row / iceberg_delete_row,
// crates/etl-destinations/src/iceberg/core.rs:636-680); 0: not a row event of the slot
DEV uint32_t ice_refused(const ColSel& s, uint64_t i) {
  if (i >= s.n_events || s.ev_slot[i] != s.slot) return 0u;
  const uint32_t k = s.ev_kind[i], fl = s.ev_flags[i];
  if (k == 'U') return (fl & ETLG_FLAG_PARTIAL) ? ETLG_ICE_PARTIAL_UPDATE : 0u;
  if (k == 'D') return (fl & 3u) == ETLG_OLD_FULL ? 0u : (fl & 3u) == ETLG_OLD_KEY ? ETLG_ICE_KEY_ONLY_DELETE : ETLG_ICE_DELETE_WITHOUT_OLD_ROW;
  return 0u;
}

__global__ __launch_bounds__(256) void k_col_count(ColSel s) {
  __shared__ uint32_t lds[8];
  uint64_t base;
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  unsigned long long pbb[2];
  const uint32_t dls = s.dl ? dl_selected(s, i, pbb) : (uint32_t)DLS_NOTHING;
  const uint32_t sel = s.dl ? dl_rows(dls) : s.pb ? pb_selected(s, i, pbb) : col_selected(s, i, base) ? 1u : 0u;
  if (s.host_rows) {  // row events of the slot that are not handed off
    bool left = dls == DLS_HOST;
    if (!s.dl && !sel && i < s.n_events && s.ev_slot[i] == s.slot) { const uint32_t k = s.ev_kind[i]; left = k == 'I' || k == 'U' || k == 'D'; }
    const unsigned long long m = __ballot(left);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(s.host_rows, (unsigned long long)__builtin_popcountll(m));
  }
  if (s.ice) {  // the refused events of the slot: their count, and the first of them with its reason (the lanes of a wave hold ascending events)
    const uint32_t why = sel ? 0u : ice_refused(s, i);
    const unsigned long long m = __ballot(why != 0u);
    if (m && (threadIdx.x & 63) == (uint32_t)__builtin_ctzll(m)) {
      atomicAdd(s.ice, (unsigned long long)__builtin_popcountll(m));
      atomicMin(s.ice + 3, (unsigned long long)((i << 8) | why));
    }
  }
  uint32_t tot;
  block_scan_incl<0>(sel, lds, &tot);
  if (threadIdx.x == 0) s.blk[blockIdx.x] = tot;
}

// exclusive scan of n u32 counts in place (single workgroup, chunks of 256); total at [n]
__global__ __launch_bounds__(256) void k_col_scan(uint32_t* v, uint32_t n) {
  __shared__ uint32_t lds[8];
  uint32_t run = 0;
  for (uint32_t b0 = 0; b0 < n; b0 += 256) {
    const uint32_t i = b0 + threadIdx.x;
    const uint32_t x = i < n ? v[i] : 0u;
    uint32_t tot;
    const uint32_t inc = block_scan_incl<0>(x, lds, &tot);
    if (i < n) v[i] = run + inc - x;
    run += tot;
  }
  if (threadIdx.x == 0) v[n] = run;
}

__global__ __launch_bounds__(256) void k_col_rows(ColSel s) {
  __shared__ uint32_t lds[8];
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint64_t base = 0;
  unsigned long long pbb[2] = {0, 0};
  const uint32_t sel = s.dl ? dl_rows(dl_selected(s, i, pbb)) : s.pb ? pb_selected(s, i, pbb) : col_selected(s, i, base) ? 1u : 0u;
  const uint32_t inc = block_scan_incl<0>(sel, lds, nullptr);
  if (sel) {
    const uint32_t r = s.blk[blockIdx.x] + inc - sel;
    s.row_event[r] = i; s.row_base[r] = (s.pb || s.dl) ? pbb[0] : base;
    if (sel == 2) { s.row_event[r + 1] = i; s.row_base[r + 1] = pbb[1]; }
  }
}

// ---- Iceberg changelog: the two trailing CDC columns of every row (iceberg/core.rs:62-85, 268-291), both non-nullable LargeUtf8 of a
// fixed width: cdc_operation "INSERT" | "UPDATE" | "DELETE" (6 bytes), sequence_number `{commit_lsn:016x}/{tx_ordinal:016x}` (33 bytes;
// crates/etl/src/event.rs:346-351). Every output is a function of its byte position, so the launch is cut by bytes, not by rows: a
// workgroup writes 4096 consecutive bytes of one value stream, a lane one aligned 16-byte piece of it (a uint4 store, consecutive lanes
// to consecutive addresses; the piece that holds the stream's end is filled with zeros — the buffers are sized up to 16). The rows a
// workgroup's bytes belong to (<= 126 / 684) are gathered once into LDS through row_event, which ascends: near-coalesced loads. The
// remaining workgroups write the offsets (8-byte stores, lane-linear) and the bitmaps (validity all ones, deferred all zeros).
constexpr uint32_t kCdcSeq = 33, kCdcOp = 6, kCdcTile = 4096;
__global__ __launch_bounds__(256) void k_col_cdc(CdcJob j) {
  __shared__ unsigned long long s_lsn[kCdcTile / kCdcSeq + 2], s_ord[kCdcTile / kCdcSeq + 2];
  __shared__ uint8_t s_kind[kCdcTile / kCdcOp + 2];
  uint32_t bx = blockIdx.x;
  const uint64_t n = j.n_rows;
  if (bx < j.nb_seq + j.nb_op) {
    const bool seq = bx < j.nb_seq;
    const uint32_t w = seq ? kCdcSeq : kCdcOp;
    if (!seq) bx -= j.nb_seq;
    const uint64_t b0 = (uint64_t)bx * kCdcTile, total = n * w, r0 = b0 / w;
    const uint64_t rl = (b0 + kCdcTile - 1) / w;
    const uint32_t nr = (uint32_t)((rl < n ? rl : n - 1) - r0 + 1);
    for (uint32_t t = threadIdx.x; t < nr; t += 256) {
      const uint64_t ev = j.row_event[r0 + t];
      if (seq) { s_lsn[t] = j.zero_token ? 0ull : j.ev_commit[ev]; s_ord[t] = j.zero_token ? 0ull : j.ev_ord[ev]; }
      else s_kind[t] = j.ev_kind[ev];
    }
    __syncthreads();
    const uint64_t p0 = b0 + (uint64_t)threadIdx.x * 16;
    if (p0 >= total) return;
    uint32_t lr = (uint32_t)(p0 / w - r0), k = (uint32_t)(p0 % w);
    uint32_t out[4] = {0u, 0u, 0u, 0u};
    for (uint32_t q = 0; q < 16; q++) {
      uint32_t ch = 0u;
      if (p0 + q < total) {
        if (seq) {
          const unsigned long long v = k < 16u ? s_lsn[lr] : s_ord[lr];
          const uint32_t nib = (uint32_t)(v >> ((((k < 16u ? 15u : 32u) - k) * 4u) & 63u)) & 15u;   // digit k of the LSN, digit k - 17 of the ordinal (k == 16 is the '/')
          ch = k == 16u ? (uint32_t)'/' : nib < 10u ? '0' + nib : 'a' + (nib - 10u);
        } else {
          const uint32_t kd = s_kind[lr];
          const unsigned long long word = kd == 'U' ? 0x455441445055ull : kd == 'D' ? 0x4554454c4544ull : 0x545245534e49ull;   // "UPDATE" / "DELETE" / "INSERT", first byte lowest
          ch = (uint32_t)(word >> (8u * k)) & 0xFFu;
        }
      }
      out[q >> 2] |= ch << (8u * (q & 3u));
      if (++k == w) { k = 0u; lr++; }
    }
    *(uint4*)((seq ? j.seq_values : j.op_values) + p0) = make_uint4(out[0], out[1], out[2], out[3]);
    return;
  }
  bx -= j.nb_seq + j.nb_op;
  const uint64_t t = (uint64_t)bx * 256 + threadIdx.x;
  if (t <= n) { j.op_offsets[t] = (int64_t)(t * kCdcOp); j.seq_offsets[t] = (int64_t)(t * kCdcSeq); }
  if (t < (n + 63) / 64) {
    const unsigned long long m = (t == n / 64) ? (1ull << (n & 63)) - 1ull : ~0ull;   // (t == n / 64 only when n is no multiple of 64)
    j.op_validity[t] = m; j.seq_validity[t] = m; j.op_deferred[t] = 0ull; j.seq_deferred[t] = 0ull;
  }
}

enum : uint32_t { AK_BOOL = 0, AK_I32 = 1, AK_I64 = 2, AK_F32 = 3, AK_F64 = 4, AK_DATE32 = 5, AK_TIME64 = 6, AK_TS = 7, AK_TSTZ = 8, AK_FIXED16 = 9,
                  AK_UTF8 = 10, AK_BINARY = 11, AK_TEXT_FORM = 12, AK_I16 = 14 /* ETLG_AK_INT16 (etlg_batch_ducklake_copy) */,
                  AK_NUMERIC_STR = kAkNumericStr, AK_TIMETZ_STR = kAkTimetzStr, AK_JSON_STR = kAkJsonStr, AK_NONE = 255 };   // 64 / 65 / 66: internal (dev_types.h kAkNumericStr ..; ColPlan.fmt), never the caller's: a string column to it

// One thread per row: state, value, validity / deferred words through wave ballots.
// (DLC: etlg_batch_ducklake_copy's launch, which alone has the 2-byte arm — an instantiation of its own, so that the kernels behind
// etlg_batch_columns / etlg_batch_iceberg compile from the text they had)
template <bool DLC = false>
DEV void col_fixed_body(const ColJob& j, uint32_t bx) {
  const uint64_t r = (uint64_t)bx * 256 + threadIdx.x;
  const bool live = r < j.n_rows;
  uint32_t st = ETLG_CELL_NULL;
  const u8* slot = nullptr;
  if (live) { const uint64_t b = j.row_base[r]; st = col_state(j, b); slot = j.fixed + b + j.off_full; }
  const bool valid = live && st == ETLG_CELL_VALUE, defer = live && st == ETLG_CELL_DEFERRED;
  const unsigned long long vm = __ballot(valid), dm = __ballot(defer), lm = __ballot(live);
  if ((threadIdx.x & 63) == 0 && lm) {
    j.validity[r >> 6] = vm; j.deferred[r >> 6] = dm;
    const uint32_t nulls = (uint32_t)__builtin_popcountll(lm & ~vm), nd = (uint32_t)__builtin_popcountll(dm);
    if (nulls) atomicAdd(j.null_count, (unsigned long long)nulls);
    if (nd) atomicAdd(j.deferred_count, (unsigned long long)nd);
  }
  if (j.kind == AK_BOOL) {  // values are bit-packed like the validity
    const unsigned long long bits = __ballot(valid && ld32a(slot) != 0);
    if ((threadIdx.x & 63) == 0 && lm) ((unsigned long long*)j.values)[r >> 6] = bits;
    return;
  }
  if (!live) return;
  uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
  if constexpr (DLC) {   // Int16 (ducklake/encoding.rs:236-257): the low half of the 4-byte slot (nothing behind it is read); a null slot holds 0
    if (j.kind == AK_I16) { ((uint16_t*)j.values)[r] = valid ? (uint16_t)ld32a(slot) : (uint16_t)0; return; }
  }
  if (valid) { w0 = ld32a(slot); if (j.kind != AK_I32 && j.kind != AK_F32 && j.kind != AK_DATE32) w1 = ld32a(slot + 4); }
  switch (j.kind) {
    case AK_I32: case AK_F32: ((uint32_t*)j.values)[r] = w0; break;
    case AK_DATE32: ((int32_t*)j.values)[r] = valid ? (int32_t)w0 - kCeDays1970 : 0; break;
    case AK_I64: {  // I64 as is; U32 widens (cell_to_i64)
      const uint64_t v = j.cls == ETLG_TC_U32 ? (uint64_t)w0 : ((uint64_t)w1 << 32) | w0;
      ((uint64_t*)j.values)[r] = v; break;
    }
    case AK_F64: ((uint64_t*)j.values)[r] = ((uint64_t)w1 << 32) | w0; break;
    case AK_TIME64: ((int64_t*)j.values)[r] = valid ? (int64_t)w0 * 1000000 + (int64_t)(w1 / 1000u) : 0; break;
    case AK_TS: case AK_TSTZ: {
      if (valid) w2 = ld32a(slot + 8);
      const int64_t days = (int64_t)(int32_t)w0 - kCeDays1970;
      ((int64_t*)j.values)[r] = valid ? (days * 86400 + (int64_t)w1) * 1000000 + (int64_t)(w2 / 1000u) : 0; break;
    }
    case AK_FIXED16: {
      if (valid) { w2 = ld32a(slot + 8); w3 = ld32a(slot + 12); }
      ((uint4*)j.values)[r] = make_uint4(w0, w1, w2, w3); break;
    }
    default: break;
  }
}

// Several columns of one hand-off in ONE launch (blockIdx.y = column): a cfg3 batch's Arrow columns were ~30 launches of 3-30 us each,
// and a third of the call was the gaps between them. The jobs travel in the kernel's argument block (a ColJob is 152 bytes, the
// block holds 4 KB): tables of more columns take several packs.
constexpr int kPack = 20;
struct ColPack { ColJob j[kPack]; unsigned long long* blk[kPack]; int64_t* offs[kPack]; unsigned long long* tot[kPack]; };   // tot: where the column's byte total goes (one read-back for all)
__global__ __launch_bounds__(256) void k_col_fixed_pack(ColPack p) { col_fixed_body(p.j[blockIdx.y], blockIdx.x); }
__global__ __launch_bounds__(256) void k_col_fixed_pack_dlc(ColPack p) { col_fixed_body<true>(p.j[blockIdx.y], blockIdx.x); }


// var-len columns, pass 1: validity / deferred words + the byte length of every row's entry
// (blk: the block's sum of lengths, for the offsets scan — a launch of its own, k_col_len_blocks, for the callers that have no such pass)
// JS: the launch has a json column that leaves as its Display string (a kernel of its own: json_display's registers would cost every
// other table two waves per SIMD)
template <bool JS>
DEV void col_lens_body(const ColJob& j, unsigned long long* blk, uint32_t bx, uint64_t* lds_sum) {
  const uint64_t r = (uint64_t)bx * 256 + threadIdx.x;
  const bool live = r < j.n_rows;
  uint32_t st = ETLG_CELL_NULL, len = 0;
  if (live) {
    const uint64_t b = j.row_base[r];
    st = col_state(j, b);
    // text-form columns hand over DEFERRED entries too (their heap entry is the source text)
    const bool text_form = j.kind == AK_TEXT_FORM || j.kind == AK_JSON_STR;
    const bool has = st == ETLG_CELL_VALUE || (text_form && st == ETLG_CELL_DEFERRED);
    bool json_ok = true;
    if (has && j.cls == ETLG_TC_JSON) {   // "JSON deserialization failed" for the first malformed cell in event order (codec/text.rs:126-134)
      const u8* slot = j.fixed + b + j.off_full;
      json_ok = json_valid(j.heap + ld32a(slot), ld32a(slot + 4));
      if (!json_ok) atomicMin(j.err, (unsigned long long)((r << 8) | ETLG_E_JSON));
    }
    if (has) {
      const u8* slot = j.fixed + b + j.off_full;
      len = j.kind == AK_NUMERIC_STR ? numeric_str_len(j.heap + ld32a(slot)) : j.kind == AK_TIMETZ_STR ? timetz_str_len(slot) : ld32a(slot + 4);
      if (JS && j.kind == AK_JSON_STR && json_ok) {   // the Display string where a lane writes it, the source text handed back DEFERRED where not
        JsCount c;
        if (json_display(c, j.heap + ld32a(slot), len, false) == JD_OK) { len = c.n; st = ETLG_CELL_VALUE; }
      }
    }
    j.lens[r] = len;
  }
  const bool valid = live && (st == ETLG_CELL_VALUE || ((j.kind == AK_TEXT_FORM || j.kind == AK_JSON_STR) && st == ETLG_CELL_DEFERRED));
  const bool defer = live && st == ETLG_CELL_DEFERRED;
  const unsigned long long vm = __ballot(valid), dm = __ballot(defer), lm = __ballot(live);
  if ((threadIdx.x & 63) == 0 && lm) {
    j.validity[r >> 6] = vm; j.deferred[r >> 6] = dm;
    const uint32_t nulls = (uint32_t)__builtin_popcountll(lm & ~vm), nd = (uint32_t)__builtin_popcountll(dm);
    if (nulls) atomicAdd(j.null_count, (unsigned long long)nulls);
    if (nd) atomicAdd(j.deferred_count, (unsigned long long)nd);
  }
  const uint64_t t = block_sum64(len, lds_sum);
  if (threadIdx.x == 0) blk[bx] = t;
}
template <bool JS>
__global__ __launch_bounds__(256) void k_col_lens_pack(ColPack p) {
  __shared__ uint64_t lds_sum[4];
  col_lens_body<JS>(p.j[blockIdx.y], p.blk[blockIdx.y], blockIdx.x, lds_sum);
}

// lens (u32) -> offsets (i64), three steps like k_col_count / k_col_scan / k_col_rows
__global__ __launch_bounds__(256) void k_col_len_blocks(const uint32_t* lens, uint64_t n, unsigned long long* blk) {
  __shared__ uint64_t lds[4];
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t t = block_sum64(i < n ? lens[i] : 0u, lds);
  if (threadIdx.x == 0) blk[blockIdx.x] = t;
}
DEV void col_len_scan_body(unsigned long long* blk, uint32_t n, uint64_t* lds) {
  const uint64_t total = carry_scan64(blk, n, 1, lds);
  if (threadIdx.x == 0) blk[n] = total;
}
__global__ __launch_bounds__(256) void k_col_len_scan(unsigned long long* blk, uint32_t n) {
  __shared__ uint64_t lds[4];
  col_len_scan_body(blk, n, lds);
}
__global__ __launch_bounds__(256) void k_col_len_scan_pack(ColPack p, uint32_t n) {   // one workgroup per column
  __shared__ uint64_t lds[4];
  col_len_scan_body(p.blk[blockIdx.x], n, lds);
}
// (O: int64_t, or int32_t for the Utf8 / Binary columns of etlg_batch_ducklake_copy — the host refuses a column whose total passes
// 2^31 - 1 before anyone reads its offsets, so the narrowing is exact wherever it is looked at)
template <class O = int64_t>
DEV void col_offsets_body(const uint32_t* lens, uint64_t n, const unsigned long long* blk, O* offsets, uint32_t bx, uint64_t* lds, unsigned long long* tot = nullptr) {
  const uint64_t i = (uint64_t)bx * 256 + threadIdx.x;
  const uint64_t ex = block_scan_excl64(i < n ? lens[i] : 0u, lds, nullptr);
  if (i < n) offsets[i] = (O)(blk[bx] + ex);
  if (i == n - 1) { offsets[n] = (O)(blk[bx] + ex + lens[i]); if (tot) *tot = blk[bx] + ex + lens[i]; }
}
__global__ __launch_bounds__(256) void k_col_offsets(const uint32_t* lens, uint64_t n, const unsigned long long* blk, int64_t* offsets, unsigned long long* tot = nullptr) {
  __shared__ uint64_t lds[4];
  col_offsets_body(lens, n, blk, offsets, blockIdx.x, lds, tot);
}
template <class O>
__global__ __launch_bounds__(256) void k_col_offsets_pack(ColPack p) {
  __shared__ uint64_t lds[4];
  const ColJob& j = p.j[blockIdx.y];
  col_offsets_body(j.lens, j.n_rows, p.blk[blockIdx.y], (O*)p.offs[blockIdx.y], blockIdx.x, lds, p.tot[blockIdx.y]);
}

// var-len columns, pass 2: one wave per 64 rows; the wave moves one row at a time, 4 bytes per lane per step where both ends
// allow it (heap entries start 4-byte aligned; the destination is wherever the previous row ended)
template <class O = int64_t>
DEV void col_copy_body(const ColJob& j, uint32_t bx) {
  // A wave takes 64 consecutive rows (their bytes are consecutive in `values`): eight lanes per row, eight rows at a time, eight bytes
  // per lane and step. (One row at a time with a byte per lane was a load and a store instruction per row of up to 64 bytes: 44 us per
  // text column of a cfg3 batch, profiles/r04q.)
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t r0 = ((uint64_t)bx * 4 + (threadIdx.x >> 6)) * 64;
  if (r0 >= j.n_rows) return;
  const uint64_t r = r0 + lane;
  uint32_t len = 0, src = 0; int64_t dst = 0;
  if (r < j.n_rows) { len = j.lens[r]; dst = ((const O*)j.offsets)[r]; if (len) src = ld32a(j.fixed + j.row_base[r] + j.off_full); }
  const uint32_t sub = lane & 7u, grp = lane >> 3;
  for (uint32_t it = 0; it < 8; it++) {
    const int k = (int)(it * 8u + grp);
    const uint32_t l_k = (uint32_t)__shfl((int)len, k, 64);
    const uint32_t s_k = (uint32_t)__shfl((int)src, k, 64);
    const uint64_t d_k = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)((uint64_t)dst >> 32), k, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)dst, k, 64);
    const u8* sp = j.heap + s_k;
    u8* dp = j.values + d_k;
    for (uint32_t b = sub * 8u; b < l_k; b += 64u) {
      if (b + 8u <= l_k) { uint64_t v; __builtin_memcpy(&v, sp + b, 8); __builtin_memcpy(dp + b, &v, 8); }
      else for (uint32_t t = b; t < l_k; t++) dp[t] = sp[t];
    }
  }
}

// formatted string columns (numeric, timetz), pass 2: one thread per row writes its Display string at its offset
template <bool JS, class O = int64_t>
DEV void col_fmt_body(const ColJob& j, uint32_t bx) {
  const uint64_t r = (uint64_t)bx * 256 + threadIdx.x;
  if (r >= j.n_rows || !j.lens[r]) return;
  const u8* slot = j.fixed + j.row_base[r] + j.off_full;
  // through the row formats' writer: eight bytes per store (a store per byte was a write request per byte and lane). For json the byte
  // writer did worse than that: its instantiation faulted on the MI355X — a store address with its low or high half replaced — while
  // the same function under a bounds-checked byte writer, under RbWrite in k_rb_rows and on the emulator was right
  // (profiles/r05x_json_arrow_fault.txt; not pursued further).
  RbWrite w(j.values + ((const O*)j.offsets)[r]);
  if (j.kind == AK_NUMERIC_STR) numeric_str(w, j.heap + ld32a(slot));
  else if (j.kind == AK_TIMETZ_STR) timetz_str(w, slot);
  else if (JS) {   // json: the Display string, or (the rows pass 1 marked DEFERRED) the source text as it is
    const u8* t = j.heap + ld32a(slot);
    if ((j.deferred[r >> 6] >> (r & 63)) & 1ull) w.bytes(t, j.lens[r]);
    else (void)json_display(w, t, ld32a(slot + 4), false);
  }
  w.finish();
}
// pass 2 of several var-len columns in one launch: a column is copied or formatted by what it is (uniform per blockIdx.y)
template <bool JS, class O = int64_t>
__global__ __launch_bounds__(256) void k_col_var2_pack(ColPack p) {
  const ColJob& j = p.j[blockIdx.y];
  if (j.kind == AK_NUMERIC_STR || j.kind == AK_TIMETZ_STR || j.kind == AK_JSON_STR) col_fmt_body<JS, O>(j, blockIdx.x); else col_copy_body<O>(j, blockIdx.x);
}


DEV bool arr_text(const ColJob& j, uint64_t r, const u8*& s, uint32_t& n, uint32_t& st) {
  const uint64_t b = j.row_base[r];
  st = col_state(j, b);
  if (st != ETLG_CELL_VALUE && st != ETLG_CELL_DEFERRED) return false;
  const u8* slot = j.fixed + b + j.off_full;
  s = j.heap + ld32a(slot); n = ld32a(slot + 4);
  return true;
}

// json[] / jsonb[] as a list of `j.to_string()` strings (ArrayCell::Json, iceberg/encoding.rs:577, 964): the literal's elements one by
// one (json_arr_check, handoff.hip.h) — checked as ONE JSON value (an element that is not is the reference's decode error,
// codec/text.rs:126-134, like a scalar json cell), sized. An element of more than kJsonElemMax bytes or beyond json_display's limits
// (depth 16, 64 members) hands the row back (ARR_HOST).
DEV uint32_t arr_json_check(const u8* s, uint32_t n, uint32_t& cnt) {
  u8 tmp[kJsonElemMax];
  JsonArrFacts f;
  if (const uint32_t e = json_arr_check<true>(s, n, tmp, cnt, f)) return e;
  // of an element too long to look at and one that is not JSON, the first in element order decides (an element too long to look at may
  // not be JSON at all: the row is the host's before anything behind it)
  if (f.too_long && !f.bad_first) return ARR_HOST;
  if (f.bad_json) return ETLG_E_JSON;
  return f.limit ? (uint32_t)ARR_HOST : 0u;
}

__global__ __launch_bounds__(256) void k_arr_count(ColJob j) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = r < j.n_rows;
  bool valid = false, defer = false;
  if (live) {
    const u8* s; uint32_t n, st, cnt = 0;
    if (arr_text(j, r, s, n, st)) {
      auto none = [](uint32_t) -> u8* { return nullptr; };
      auto skip = [](uint32_t, bool, const uint32_t*, const u8*) {};
      const uint32_t e = j.elem_cls == ETLG_TC_JSON ? arr_json_check(s, n, cnt)
                       : (j.elem_cls == ETLG_TC_STRING || j.elem_cls == ETLG_TC_BYTEA) ? arr_walk<true>(s, n, j.elem_cls, cnt, skip, none) : arr_walk<false>(s, n, j.elem_cls, cnt, skip, none);
      // A row handed back (ARR_HOST) is the host's to finish, and it may turn out to be the batch's first malformed literal. So the call
      // only fails for a malformed row when no handed-back row precedes it (the host compares the two minima: code kArrHandBack marks a
      // hand-back); otherwise the malformed rows are handed back as well, and the consumer — finishing deferred rows in event
      // order — meets the first problem first, like parse_cell_from_postgres_text at decode time.
      if (e == ARR_HOST) { defer = true; cnt = 0; atomicMin(j.err, (unsigned long long)((r << 8) | kArrHandBack)); }
      else if (e) { atomicMin(j.err, (unsigned long long)((r << 8) | e)); cnt = 0; defer = true; }
      else valid = true;
    }
    j.lens[r] = cnt;
  }
  const unsigned long long vm = __ballot(valid), dm = __ballot(defer), lm = __ballot(live);
  if ((threadIdx.x & 63) == 0 && lm) {
    j.validity[r >> 6] = vm; j.deferred[r >> 6] = dm;
    const uint32_t nulls = (uint32_t)__builtin_popcountll(lm & ~vm), nd = (uint32_t)__builtin_popcountll(dm);
    if (nulls) atomicAdd(j.null_count, (unsigned long long)nulls);
    if (nd) atomicAdd(j.deferred_count, (unsigned long long)nd);
  }
}

__global__ __launch_bounds__(256) void k_arr_fill(ColJob j) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= j.n_rows || !j.lens[r]) return;
  const u8* s; uint32_t n, st, cnt;
  if (!arr_text(j, r, s, n, st)) return;
  const uint64_t o = (uint64_t)j.offsets[r];
  uint32_t nulls = 0;
  if (j.elem_cls == ETLG_TC_JSON) {
    // pass A (values not set): the Display length and validity of every element; pass B: the characters
    u8 tmp[kJsonElemMax];
    if (!j.values) {
      json_arr_visit(s, n, tmp, [&](uint32_t k, bool is_null, const u8* t, uint32_t tn) {
        const uint64_t e = o + k;
        uint32_t len = 0;
        if (!is_null) {
          JsCount c;
          (void)json_display(c, t, tn, false);
          len = c.n;
          atomicOr(&j.child_validity[e >> 5], 1u << (e & 31));
        } else nulls++;
        j.child_lens[e] = len;
      });
      if (nulls) atomicAdd(j.child_nulls, (unsigned long long)nulls);
    } else {
      json_arr_visit(s, n, tmp, [&](uint32_t k, bool is_null, const u8* t, uint32_t tn) {
        if (is_null) return;
        RbWrite sw(j.values + j.child_offsets[o + k]);
        (void)json_display(sw, t, tn, false);
        sw.finish();
      });
    }
    return;
  }
  if (j.elem_cls == ETLG_TC_NUMERIC || j.elem_cls == ETLG_TC_TIMETZ) {
    // ArrayCell::Numeric / TimeTz are lists of their Display strings in the sinks (iceberg/encoding.rs:902-945: `n.to_string()`,
    // `t.to_string()`): pass A their lengths, pass B the characters. The element's value is what decode_text_cell left in the
    // walker's scratch (a numeric heap entry) or in its slot words (timetz).
    const bool num = j.elem_cls == ETLG_TC_NUMERIC;
    if (!j.values) {
      (void)arr_walk<false>(s, n, j.elem_cls, cnt, [&](uint32_t k, bool is_null, const uint32_t* w, const u8* scratch) {
        const uint64_t e = o + k;
        j.child_lens[e] = is_null ? 0u : num ? numeric_str_len(scratch + w[0]) : timetz_str_len((const u8*)w);
        if (is_null) nulls++; else atomicOr(&j.child_validity[e >> 5], 1u << (e & 31));
      }, [](uint32_t) -> u8* { return nullptr; });
      if (nulls) atomicAdd(j.child_nulls, (unsigned long long)nulls);
    } else {
      (void)arr_walk<false>(s, n, j.elem_cls, cnt, [&](uint32_t k, bool is_null, const uint32_t* w, const u8* scratch) {
        if (is_null) return;
        RbWrite sw(j.values + j.child_offsets[o + k]);
        if (num) numeric_str(sw, scratch + w[0]); else timetz_str(sw, (const u8*)w);
        sw.finish();
      }, [](uint32_t) -> u8* { return nullptr; });
    }
    return;
  }
  if (j.elem_cls == ETLG_TC_STRING || j.elem_cls == ETLG_TC_BYTEA) {
    // pass A (child_lens set, values not): the byte length and validity of every element; pass B (values set): the bytes
    if (!j.values) {
      (void)arr_walk<true>(s, n, j.elem_cls, cnt, [&](uint32_t k, bool is_null, const uint32_t* w, const u8*) {
        const uint64_t e = o + k;
        j.child_lens[e] = w[0];
        if (is_null) nulls++; else atomicOr(&j.child_validity[e >> 5], 1u << (e & 31));
      }, [](uint32_t) -> u8* { return nullptr; });
      if (nulls) atomicAdd(j.child_nulls, (unsigned long long)nulls);
    } else {
      (void)arr_walk<true>(s, n, j.elem_cls, cnt, [](uint32_t, bool, const uint32_t*, const u8*) {},
                           [&](uint32_t k) -> u8* { return k < j.lens[r] ? j.values + j.child_offsets[o + k] : nullptr; });
    }
    return;
  }
  (void)arr_walk<false>(s, n, j.elem_cls, cnt, [&](uint32_t k, bool is_null, const uint32_t* w, const u8*) {
    const uint64_t e = o + k;
    if (is_null) { nulls++; }
    else atomicOr(&j.child_validity[e >> 5], 1u << (e & 31));
    switch (j.kind) {   // child layout: the same conversions as col_fixed_body
      case AK_BOOL: if (!is_null && w[0]) atomicOr(&((uint32_t*)j.values)[e >> 5], 1u << (e & 31)); break;
      case AK_I32: case AK_F32: ((uint32_t*)j.values)[e] = w[0]; break;
      case AK_DATE32: ((int32_t*)j.values)[e] = is_null ? 0 : (int32_t)w[0] - kCeDays1970; break;
      case AK_TIME64: ((int64_t*)j.values)[e] = is_null ? 0 : (int64_t)w[0] * 1000000 + (int64_t)(w[1] / 1000u); break;
      case AK_TS: case AK_TSTZ:
        ((int64_t*)j.values)[e] = is_null ? 0 : (((int64_t)(int32_t)w[0] - kCeDays1970) * 86400 + (int64_t)w[1]) * 1000000 + (int64_t)(w[2] / 1000u); break;
      case AK_FIXED16: ((uint4*)j.values)[e] = make_uint4(w[0], w[1], w[2], w[3]); break;
      default: ((uint64_t*)j.values)[e] = j.elem_cls == ETLG_TC_U32 ? (uint64_t)w[0] : ((uint64_t)w[1] << 32) | w[0]; break;   // I64, U32, F64
    }
  }, [](uint32_t) -> u8* { return nullptr; });
  if (nulls) atomicAdd(j.child_nulls, (unsigned long long)nulls);
}

}  // namespace etlg

extern "C" {

using namespace etlg;

void etlg_k_col_select(const ColSel* selv, hipStream_t st) {
  const ColSel s = *selv;
  if (!s.nblocks) return;
  hipLaunchKernelGGL(k_col_count, dim3(s.nblocks), dim3(256), 0, st, s);
  hipLaunchKernelGGL(k_col_scan, dim3(1), dim3(256), 0, st, s.blk, s.nblocks);
  hipLaunchKernelGGL(k_col_rows, dim3(s.nblocks), dim3(256), 0, st, s);
}

// both CDC columns of a changelog batch in one launch (the job's nb_seq / nb_op are filled in here)
void etlg_k_col_cdc(const CdcJob* jv, hipStream_t st) {
  CdcJob j = *jv;
  if (!j.n_rows) return;
  j.nb_seq = (uint32_t)((j.n_rows * kCdcSeq + kCdcTile - 1) / kCdcTile);
  j.nb_op = (uint32_t)((j.n_rows * kCdcOp + kCdcTile - 1) / kCdcTile);
  hipLaunchKernelGGL(k_col_cdc, dim3(j.nb_seq + j.nb_op + (uint32_t)((j.n_rows + 256) / 256)), dim3(256), 0, st, j);
}

// Packed forms (jobs: n <= etlg_k_col_pack_max() ColJob records of ONE hand-off, all with the same n_rows): every fixed-width column /
// pass 1 of every var-len column (lens -> block sums -> offsets; blk[i] / offs[i]: the column's scan scratch and offsets) / pass 2.
uint32_t etlg_k_col_pack_max(void) { return kPack; }
static void fill_pack(ColPack& p, const ColJob* jobs, uint32_t n, unsigned long long* const* blk, int64_t* const* offs, unsigned long long* const* tot = nullptr) {
  for (uint32_t i = 0; i < n; i++) { p.j[i] = jobs[i]; p.blk[i] = blk ? blk[i] : nullptr; p.offs[i] = offs ? offs[i] : nullptr; p.tot[i] = tot ? tot[i] : nullptr; }
}
void etlg_k_col_fixed_pack(const ColJob* j, uint32_t n, hipStream_t st) {
  if (!n || !j[0].n_rows) return;
  ColPack p; fill_pack(p, j, n, nullptr, nullptr);
  const dim3 grid((uint32_t)((j[0].n_rows + 255) / 256), n);
  if (j[0].off32) hipLaunchKernelGGL(k_col_fixed_pack_dlc, grid, dim3(256), 0, st, p); else hipLaunchKernelGGL(k_col_fixed_pack, grid, dim3(256), 0, st, p);
}
void etlg_k_col_var_pack(const ColJob* j, uint32_t n, unsigned long long* const* blk, int64_t* const* offs, unsigned long long* const* tot, int step, hipStream_t st) {
  if (!n || !j[0].n_rows) return;
  const uint32_t nb = (uint32_t)((j[0].n_rows + 255) / 256);
  ColPack p; fill_pack(p, j, n, blk, offs, tot);
  bool js = false;
  for (uint32_t i = 0; i < n; i++) js |= j[i].kind == AK_JSON_STR;
  const bool o32 = j[0].off32 != 0;   // (one hand-off, one offset width: etlg_batch_ducklake_copy, whose tables have no json column)
  if (step == 0) {
    if (js) hipLaunchKernelGGL(k_col_lens_pack<true>, dim3(nb, n), dim3(256), 0, st, p); else hipLaunchKernelGGL(k_col_lens_pack<false>, dim3(nb, n), dim3(256), 0, st, p);
    hipLaunchKernelGGL(k_col_len_scan_pack, dim3(n), dim3(256), 0, st, p, nb);
    if (o32) hipLaunchKernelGGL(k_col_offsets_pack<int32_t>, dim3(nb, n), dim3(256), 0, st, p); else hipLaunchKernelGGL(k_col_offsets_pack<int64_t>, dim3(nb, n), dim3(256), 0, st, p);
  } else if (o32) {
    hipLaunchKernelGGL((k_col_var2_pack<false, int32_t>), dim3(nb, n), dim3(256), 0, st, p);
  } else {
    if (js) hipLaunchKernelGGL(k_col_var2_pack<true>, dim3(nb, n), dim3(256), 0, st, p); else hipLaunchKernelGGL(k_col_var2_pack<false>, dim3(nb, n), dim3(256), 0, st, p);
  }
}

// block sums of n lens (blk[b]: the sum of lens[256 b ..], left by the caller's own kernel: k_rb_lens) + lens -> offsets (i64,
// n + 1 entries); blk: (ceil(n / 256) + 1) x u64; tot: where the total goes as well, or null
void etlg_k_scan_blocks(const uint32_t* lens, uint64_t n, unsigned long long* blk, int64_t* offsets, unsigned long long* tot, hipStream_t st) {
  if (!n) return;
  const uint32_t nb = (uint32_t)((n + 255) / 256);
  hipLaunchKernelGGL(k_col_len_scan, dim3(1), dim3(256), 0, st, blk, nb);
  hipLaunchKernelGGL(k_col_offsets, dim3(nb), dim3(256), 0, st, lens, n, (const unsigned long long*)blk, offsets, tot);
}

// the same for a caller that has only the lens: blk is scratch
void etlg_k_scan_lens(const uint32_t* lens, uint64_t n, unsigned long long* blk, int64_t* offsets, hipStream_t st) {
  if (!n) return;
  const uint32_t nb = (uint32_t)((n + 255) / 256);
  hipLaunchKernelGGL(k_col_len_blocks, dim3(nb), dim3(256), 0, st, lens, n, blk);
  etlg_k_scan_blocks(lens, n, blk, offsets, nullptr, st);
}

// list columns: step 0 = element counts + list offsets, step 1 = child values / validity
void etlg_k_col_list(const ColJob* jv, unsigned long long* blk, int64_t* offsets, int step, hipStream_t st) {
  const ColJob j = *jv;
  if (!j.n_rows) return;
  const uint32_t nb = (uint32_t)((j.n_rows + 255) / 256);
  if (step == 0) {
    hipLaunchKernelGGL(k_arr_count, dim3(nb), dim3(256), 0, st, j);
    etlg_k_scan_lens(j.lens, j.n_rows, blk, offsets, st);
  } else {
    hipLaunchKernelGGL(k_arr_fill, dim3(nb), dim3(256), 0, st, j);
  }
}

}  // extern "C"
