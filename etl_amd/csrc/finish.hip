// Event::size_hint of every event of a batch (etlg_batch_size_hints) and the finish pass (etlg_batch_finish_cells): both read the arena
// of a decoded, device-resident batch; the finish pass also writes it. Integer / byte work: no MFMA.
#include "handoff.hip.h"
#include "float_slow.h"

extern "C" void etlg_k_scan_lens(const uint32_t* lens, uint64_t n, unsigned long long* blk, int64_t* offsets, hipStream_t st);   // columns.hip

namespace etlg {

// ---- Event::size_hint (crates/etl/src/event.rs:295-320; data/table_row.rs:248-299)
DEV uint64_t hint_row(const HintJob& j, const HintSlotRec& sl, uint64_t base, bool key, bool& incomplete) {
  uint64_t total = (uint64_t)j.m_row + (uint64_t)(key ? sl.n_ident : sl.n_cols) * j.m_cell;   // TableRow + Vec<Cell> capacity
  uint32_t k = 0;
  for (uint32_t i = 0; i < sl.n_cols; i++) {
    const HintColRec& cd = j.cols[sl.cols_base + i];
    const uint32_t cls = cd.cls();
    if (key && !cd.identity()) continue;
    const uint32_t pos = key ? k : i, off = key ? cd.off_key : cd.off_full();
    k++;
    const uint32_t st = (j.fixed[base + pos / 4] >> (2 * (pos % 4))) & 3u;
    if (st == ETLG_CELL_NULL) continue;
    if (st == ETLG_CELL_MISSING) { incomplete = true; continue; }
    const bool text_form = cls == ETLG_TC_JSON || cls == ETLG_TC_ARRAY || cls == ETLG_TC_NUMERIC;
    if (st == ETLG_CELL_DEFERRED) { if (text_form) incomplete = true; continue; }   // a deferred fixed-width cell owns no heap
    const u8* slot = j.fixed + base + off;
    if (cls == ETLG_TC_STRING || cls == ETLG_TC_BYTEA) total += ld32a(slot + 4);
    else if (cls == ETLG_TC_NUMERIC) { const u8* h = j.heap + ld32a(slot); if (h[0] == ETLG_NUM_VALUE) total += 2u * (uint32_t)(h[6] | (h[7] << 8)); }
    else if (cls == ETLG_TC_JSON || cls == ETLG_TC_ARRAY) incomplete = true;
  }
  return total;
}

__global__ __launch_bounds__(256) void k_size_hints(HintJob j) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= j.n_events) return;
  const uint32_t kind = j.ev_kind[i], fl = j.ev_flags[i];
  uint64_t v = 0;
  bool inc = false;
  if (kind == 'B') v = j.m_begin;
  else if (kind == 'C') v = j.m_commit;
  else if (kind == 'R') v = j.m_relation;
  else if (kind == 'T') v = (uint64_t)j.m_truncate + (uint64_t)j.ev_table[i] * j.m_rts;
  else if (kind == 'I' || kind == 'U' || kind == 'D') {
    const uint32_t s = j.ev_slot[i];
    if (s >= j.n_slots) { inc = true; }
    else {
      const HintSlotRec& sl = j.slots[s];
      uint64_t base = j.ev_body[i];
      v = kind == 'I' ? j.m_insert : kind == 'U' ? j.m_update : j.m_delete;
      if (kind != 'I') {
        const uint32_t ok = fl & 3u;
        if (ok) { v += hint_row(j, sl, base, ok == ETLG_OLD_KEY, inc); base += ok == ETLG_OLD_KEY ? sl.row_key : sl.row_full; }
      }
      if (kind != 'D') {
        if (fl & ETLG_FLAG_PARTIAL) inc = true;
        v += hint_row(j, sl, base, false, inc);
      }
    }
  }
  j.out[i] = v | (inc ? (1ull << 63) : 0ull);
}

// ---- write_events cut points (etlg_batch_cuts, include/etlg.h): the apply loop's rule — EventBatch::push adds the event's hint to
// size_hint_bytes (crates/etl/src/replication/apply.rs:656-657), the loop flushes once size_hint_bytes >= the budget (:1932-1945) and the
// next batch starts at zero — is a prefix sum that resets, and the reset is not associative. It decomposes: with q the plain prefix sums
// of the hints, the batch that STARTS at a ends at the smallest e > a with q[e] - q[a] >= budget, whatever came before a. So the cuts are
// the orbit of the first cut under a -> next(a), and the p-th orbit element is reached through the jump levels next^(2^k) named by the
// bits of p. Launches, none of which exchanges a word between its workgroups: tile sums + first INCOMPLETE per tile (k_cut_tiles), their
// scan by one workgroup (k_cut_scan), q (k_cut_write); the host reads L and total and sizes the rest: next by binary search in q
// (k_cut_next), one squaring per level (k_cut_level), the count and the carry by one thread (k_cut_count), the cuts (k_cut_emit).
constexpr unsigned long long kHintMask = ~(1ull << 63);
constexpr unsigned long long kNone64 = ~0ull;

DEV uint64_t block_min64(uint64_t v, uint64_t* lds) {  // returns the workgroup minimum
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { const uint64_t t = __shfl_xor(v, d, 64); v = t < v ? t : v; }
  if (lane == 0) lds[wave] = v;
  __syncthreads();
  uint64_t m = lds[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); w++) m = lds[w] < m ? lds[w] : m;
  __syncthreads();
  return m;
}

__global__ __launch_bounds__(256) void k_cut_tiles(CutJob j) {
  __shared__ uint64_t lds[4];
  const uint64_t k0 = (uint64_t)blockIdx.x * j.tile;
  if (k0 >= j.n) return;
  const uint64_t k1 = k0 + j.tile < j.n ? k0 + j.tile : j.n;
  uint64_t sum = 0, inc = kNone64;
  for (uint64_t k = k0 + threadIdx.x; k < k1; k += 256) {
    const uint64_t h = j.hints[j.first + k];
    sum += h & kHintMask;
    if ((h >> 63) && k < inc) inc = k;
  }
  sum = block_sum64(sum, lds);
  inc = block_min64(inc, lds);
  if (threadIdx.x == 0) { j.tsum[blockIdx.x] = sum; j.tinc[blockIdx.x] = inc; }
}

// one workgroup: the tile sums become the sums in front of each tile, the tiles' first INCOMPLETE events their minimum
__global__ __launch_bounds__(256) void k_cut_scan(CutJob j) {
  __shared__ uint64_t lds[4];
  (void)carry_scan64(j.tsum, j.n_tiles, 1, lds);
  uint64_t inc = kNone64;
  for (uint32_t t = threadIdx.x; t < j.n_tiles; t += 256) { const uint64_t ti = j.tinc[t]; inc = ti < inc ? ti : inc; }
  inc = block_min64(inc, lds);
  if (threadIdx.x == 0) { j.hdr[0] = inc < j.n ? inc : j.n; j.hdr[1] = 0; j.q[0] = 0; }   // (hdr[1]: k_cut_write, when L > 0)
}

__global__ __launch_bounds__(256) void k_cut_write(CutJob j) {
  __shared__ uint64_t lds[4];
  const uint64_t k0 = (uint64_t)blockIdx.x * j.tile;
  if (k0 >= j.n) return;
  const uint64_t k1 = k0 + j.tile < j.n ? k0 + j.tile : j.n, L = j.hdr[0];
  uint64_t carry = j.tsum[blockIdx.x];
  for (uint64_t kb = k0; kb < k1; kb += 256) {   // (uniform trip count: every lane takes part in every scan)
    const uint64_t k = kb + threadIdx.x;
    const bool on = k < k1;
    const uint64_t v = on ? j.hints[j.first + k] & kHintMask : 0;
    uint64_t tot;
    const uint64_t inc = carry + block_scan_excl64(v, lds, &tot) + v;
    if (on) { j.q[k + 1] = inc; if (k + 1 == L) j.hdr[1] = inc; }
    carry += tot;
  }
}

// the smallest e in [lo, hi] with q[e] >= want; hi + 1 when there is none (q is ascending)
DEV uint64_t cut_lower_bound(const unsigned long long* q, uint64_t lo, uint64_t hi, uint64_t want) {
  uint64_t end = hi + 1;
  while (lo < end) { const uint64_t mid = lo + ((end - lo) >> 1); if (q[mid] >= want) end = mid; else lo = mid + 1; }
  return lo;
}

__global__ __launch_bounds__(256) void k_cut_next(CutJob j) {
  const uint64_t a = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (a > j.L + 1) return;
  j.jump[a] = a >= j.L ? (uint32_t)(j.L + 1) : (uint32_t)cut_lower_bound(j.q, a + 1, j.L, j.q[a] + j.budget);
}

__global__ __launch_bounds__(256) void k_cut_level(const uint32_t* src, uint32_t* dst, uint64_t n) {
  const uint64_t a = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (a < n) dst[a] = src[src[a]];
}

__global__ __launch_bounds__(64) void k_cut_count(CutJob j) {
  if (threadIdx.x) return;
  const uint64_t L = j.L, W = L + 2;
  // the first batch opens with carry_in (< budget, so the subtraction does not wrap)
  uint64_t pos = cut_lower_bound(j.q, 1, L, j.budget - j.carry_in), n = 0;
  j.hdr[4] = pos;
  if (pos <= L) {
    n = 1;
    for (uint32_t k = j.levels; k-- > 0;) { const uint64_t nx = j.jump[(uint64_t)k * W + pos]; if (nx <= L) { pos = nx; n += 1ull << k; } }
  }
  j.hdr[2] = n;
  j.hdr[3] = n ? j.q[L] - j.q[pos] : j.carry_in + j.q[L];
}

__global__ __launch_bounds__(256) void k_cut_emit(CutJob j) {
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= j.hdr[2] || p >= j.cuts_cap) return;
  const uint64_t W = j.L + 2;
  uint64_t pos = j.hdr[4];
  for (uint32_t k = 0; k < j.levels; k++) if ((p >> k) & 1u) pos = j.jump[(uint64_t)k * W + pos];
  j.cuts[p] = j.first + pos;
}

// etlg_cuts_locate: per cut the number of rows whose event lies in front of it (row_event is ascending; equal entries stay together)
__global__ __launch_bounds__(256) void k_cuts_locate(const unsigned long long* cuts, uint64_t n_cuts, const unsigned long long* row_event, uint64_t n_rows,
                                                     unsigned long long* rows_out) {
  const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n_cuts) return;
  rows_out[k] = n_rows ? cut_lower_bound(row_event, 0, n_rows - 1, cuts[k]) : 0;
}

// ---- the write_events pass plan (etlg_batch_outline, include/etlg.h: the pass rule is stated there). The sequential loop of the sinks —
// rows until a Relation or Truncate, the Relation run, the Truncate run, again — becomes a flag per event: a pass starts where a
// write_events range starts (a bitmap of the cuts, k_ol_mark) and where the class falls against the event before, which global memory
// holds, so no tile needs a carry. Launches, none of which exchanges a word between its workgroups: the cuts checked and marked
// (k_ol_mark), per tile the starts, truncate entries, Relations and rows plus the slot census (k_ol_tiles), their scan by one workgroup
// (k_ol_scan), a pass index and a truncate position per event (k_ol_write), a thread per written pass for what no single event knows
// (k_ol_fix). The caps are the caller's, so nothing is read back in between; every output is written from scratch by k_ol_write and
// k_ol_fix, which do nothing once a cut is bad. Every loop runs to a launch parameter: tile / 256 chunks, 64 table entries, log2(n_cuts)
// steps of a search, W words, at most trunc_cap entries of a body.
constexpr uint32_t kOlFree = ~0u;
constexpr uint32_t kOlTouchWords = 16;          // touched words of the pass a tile continues that k_ol_write gathers in LDS (1 024 slots)
constexpr uint64_t kOlLow = (1ull << 48) - 1;  // a chunk's truncate entries (256 x u32) ride below its starts in one scanned word

DEV uint32_t ol_class(uint32_t kind, uint32_t inline_rel) { return kind == 'T' ? 2u : (kind == 'R' && !inline_rel) ? 1u : 0u; }
DEV bool ol_is_row(uint32_t kind) { return kind == 'I' || kind == 'U' || kind == 'D'; }
DEV uint32_t ol_category(uint32_t kind, uint32_t fl) {
  if (kind == 'I') return 0u;
  if (kind == 'U') return (fl & ETLG_FLAG_PARTIAL) ? 2u : 1u;
  const uint32_t ok = fl & 3u;
  return ok == ETLG_OLD_FULL ? 3u : ok == ETLG_OLD_KEY ? 4u : 5u;
}

// local event k < n: its kind and class, whether a pass starts at it, and the class it follows inside its pass (0 at a start)
struct OlEvent { uint32_t kind, cls, after; bool start; };
DEV OlEvent ol_event(const OutlineJob& j, uint64_t k) {
  OlEvent e;
  e.kind = j.ev_kind[j.first + k];
  e.cls = ol_class(e.kind, j.inline_rel);
  e.after = k ? ol_class(j.ev_kind[j.first + k - 1], j.inline_rel) : 0u;   // (ev_kind[first - 1] is never read)
  e.start = k == 0 || ((j.bitmap[k >> 5] >> (k & 31)) & 1u) || e.cls < e.after;
  if (e.start) e.after = 0u;
  return e;
}

__global__ __launch_bounds__(256) void k_ol_mark(OutlineJob j) {
  const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= j.n_cuts) return;
  const uint64_t c = j.cuts[k], end = j.first + j.n;
  if (c < j.first || c > end || (k && c < j.cuts[k - 1])) { atomicMin(j.bad, (unsigned long long)k); return; }
  if (c < end) atomicOr(&j.bitmap[(c - j.first) >> 5], 1u << ((c - j.first) & 31));
  if (k + 1 == j.n_cuts) j.hdr[OL_H_RANGES] = j.n_cuts + (c < end ? 1u : 0u);   // a last range runs to `end`
}

// The tile's slot table: kOlLdsSlots keys, claimed by atomicMin alone. A lane walks from its slot's home and leaves the smaller key in
// every entry it meets, carrying the larger one on; entries are never freed, so whoever looks a slot up later walks from the same home
// until it meets the slot or a free entry. With more distinct slots than entries the largest keys fall off the end and are counted in
// global memory directly. A claim MOVES keys that were placed before it, and the counters belong to positions: so the tile claims the
// slots of ALL its events first, and counts, behind a barrier, in a table that no longer changes.
DEV void ol_claim(uint32_t* keys, uint32_t s) {
  uint32_t cur = s, pos = s % kOlLdsSlots;
  for (uint32_t t = 0; t < kOlLdsSlots; t++) {
    const uint32_t old = atomicMin(&keys[pos], cur);
    if (old == kOlFree || old == cur) return;
    if (old > cur) cur = old;
    pos = (pos + 1) % kOlLdsSlots;
  }
}
DEV uint32_t ol_find(const uint32_t* keys, uint32_t s) {
  uint32_t pos = s % kOlLdsSlots;
  for (uint32_t t = 0; t < kOlLdsSlots; t++) {
    const uint32_t k = keys[pos];
    if (k == s) return pos;
    if (k == kOlFree) break;
    pos = (pos + 1) % kOlLdsSlots;
  }
  return kOlLdsSlots;
}

// A lane's part in the census: its event is a row of slot s (< n_slots) and category cat; `mine`: the lane claims and counts — every
// row lane, or the first lane alone (cnt = 64) of a wave whose 64 events are rows of one slot and category, which is every wave of a
// single-table stream. Holds wave collectives: every lane of the workgroup calls it, `on` or not.
struct OlRow { uint32_t s, cat, cnt; bool mine; };
DEV OlRow ol_row(const OutlineJob& j, uint64_t k, bool on, uint32_t kind) {
  OlRow r{0, 0, 1, false};
  bool row = false;
  if (on && ol_is_row(kind)) {
    r.s = j.ev_slot[j.first + k];
    r.cat = ol_category(kind, j.ev_flags[j.first + k]);
    row = r.s < j.n_slots;
  }
  const uint32_t key = row ? r.s * 8u + r.cat : kOlFree, key0 = __shfl(key, 0, 64);
  const bool uni = __all(key == key0) && key0 != kOlFree;
  r.mine = row && (!uni || (threadIdx.x & 63) == 0);
  if (uni) r.cnt = 64;
  return r;
}

__global__ __launch_bounds__(256) void k_ol_tiles(OutlineJob j) {
  __shared__ uint64_t lds[4];
  __shared__ uint32_t keys[kOlLdsSlots], rows[kOlLdsSlots * 6];
  __shared__ unsigned long long firsts[kOlLdsSlots * 6];
  const uint64_t k0 = (uint64_t)blockIdx.x * j.tile;
  if (k0 >= j.n) return;
  const uint64_t k1 = k0 + j.tile < j.n ? k0 + j.tile : j.n;
  if (threadIdx.x < kOlLdsSlots) keys[threadIdx.x] = kOlFree;
  for (uint32_t t = threadIdx.x; t < kOlLdsSlots * 6; t += 256) { rows[t] = 0; firsts[t] = kNone64; }
  __syncthreads();
  uint64_t starts = 0, truncs = 0, rels = 0, nrows = 0;
  for (uint64_t kb = k0; kb < k1; kb += 256) {   // the tile's sums, and every slot claimed (uniform trip count: every lane takes part in every collective)
    const uint64_t k = kb + threadIdx.x;
    const bool on = k < k1;
    uint32_t kind = 0;
    if (on) {
      const OlEvent e = ol_event(j, k);
      kind = e.kind;
      starts += e.start;
      rels += e.kind == 'R';
      nrows += ol_is_row(e.kind);
      if (e.kind == 'T') truncs += j.ev_table[j.first + k];
    }
    const OlRow r = ol_row(j, k, on, kind);
    if (r.mine) ol_claim(keys, r.s);
  }
  __syncthreads();
  for (uint64_t kb = k0; kb < k1; kb += 256) {   // the census, in the table as it now stands
    const uint64_t k = kb + threadIdx.x;
    const bool on = k < k1;
    const OlRow r = ol_row(j, k, on, on ? (uint32_t)j.ev_kind[j.first + k] : 0u);
    if (!r.mine) continue;
    const uint32_t at = ol_find(keys, r.s);
    if (at < kOlLdsSlots) { atomicAdd(&rows[at * 6 + r.cat], r.cnt); atomicMin(&firsts[at * 6 + r.cat], (unsigned long long)(j.first + k)); }
    else { atomicAdd(&j.crow[(uint64_t)r.s * 6 + r.cat], (unsigned long long)r.cnt); atomicMin(&j.cfirst[(uint64_t)r.s * 6 + r.cat], (unsigned long long)(j.first + k)); }
  }
  __syncthreads();
  if (threadIdx.x < kOlLdsSlots && keys[threadIdx.x] != kOlFree) {   // one global atomic per slot and category of the tile
    const uint64_t s = keys[threadIdx.x];
    for (uint32_t c = 0; c < 6; c++) {
      const uint32_t r = rows[threadIdx.x * 6 + c];
      if (r) { atomicAdd(&j.crow[s * 6 + c], (unsigned long long)r); atomicMin(&j.cfirst[s * 6 + c], firsts[threadIdx.x * 6 + c]); }
    }
  }
  starts = block_sum64(starts, lds); truncs = block_sum64(truncs, lds); rels = block_sum64(rels, lds); nrows = block_sum64(nrows, lds);
  if (threadIdx.x == 0) { unsigned long long* t = j.tsum + 4 * (uint64_t)blockIdx.x; t[0] = starts; t[1] = truncs; t[2] = rels; t[3] = nrows; }
}

// one workgroup: each of the four sums per tile becomes the sum in front of the tile; the totals are the call's counts
__global__ __launch_bounds__(256) void k_ol_scan(OutlineJob j) {
  __shared__ uint64_t lds[4];
  if (*j.bad != kNone64) return;
  for (uint32_t k = 0; k < 4; k++) {
    const uint64_t tot = carry_scan64(j.tsum + k, j.n_tiles, 4, lds);
    if (threadIdx.x == 0) j.hdr[k] = tot;   // OL_H_PASSES, _TRUNC, _REL, _ROWS
  }
}

// the number of cuts <= ev: the index of the write_events range that holds event ev
DEV uint64_t ol_range_of(const unsigned long long* cuts, uint64_t n_cuts, uint64_t ev) {
  uint64_t lo = 0, hi = n_cuts;
  while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if (cuts[mid] <= ev) lo = mid + 1; else hi = mid; }
  return lo;
}

__global__ __launch_bounds__(256) void k_ol_write(OutlineJob j) {
  __shared__ uint64_t lds[4];
  if (*j.bad != kNone64) return;
  const uint64_t k0 = (uint64_t)blockIdx.x * j.tile;
  if (k0 >= j.n) return;
  const uint64_t k1 = k0 + j.tile < j.n ? k0 + j.tile : j.n;
  const int lane = threadIdx.x & 63;
  uint64_t carry_p = j.tsum[4 * (uint64_t)blockIdx.x], carry_t = j.tsum[4 * (uint64_t)blockIdx.x + 1];
  // The pass in progress where the tile begins (~0, which no event has, in front of the window's first tile) may span thousands of tiles
  // — one range of a single-table stream is one pass —, and every tile would send its bits to the same words: the tile gathers the
  // first kOlTouchWords words of that pass in LDS and ends with one atomicOr per word. Passes that start inside the tile go direct.
  __shared__ unsigned long long tw[kOlTouchWords];
  const uint64_t p_in = carry_p - 1;
  if (threadIdx.x < kOlTouchWords) tw[threadIdx.x] = 0;
  __syncthreads();
  for (uint64_t kb = k0; kb < k1; kb += 256) {   // (uniform trip count: every lane takes part in every scan)
    const uint64_t k = kb + threadIdx.x, i = j.first + k;
    const bool on = k < k1;
    OlEvent e{0, 0, 0, false};
    if (on) e = ol_event(j, k);
    const uint64_t tcnt = on && e.kind == 'T' ? j.ev_table[i] : 0ull, v = ((uint64_t)e.start << 48) | tcnt;
    uint64_t tot;
    const uint64_t ex = block_scan_excl64(v, lds, &tot);
    // the event's pass (the window's first event is a start, so every event has one) and its first truncate entry
    const uint64_t p = carry_p + (ex >> 48) + e.start - 1, tpos = carry_t + (ex & kOlLow);
    carry_p += tot >> 48; carry_t += tot & kOlLow;
    if (on && e.start) {
      if (j.passes_out && p < j.passes_cap) { j.passes_out[7 * p] = i; j.passes_out[7 * p + 4] = ol_range_of(j.cuts, j.n_cuts, i); }
      if (j.tf && p <= j.passes_cap) j.tf[p] = tpos;
      if (p >= 1 && p - 1 < j.passes_cap) {   // the pass before ends here
        if (j.passes_out) j.passes_out[7 * (p - 1) + 3] = i;
        if (j.ends_out) j.ends_out[p - 1] = i;
      }
    }
    if (on && j.de && p < j.passes_cap && e.cls > e.after) {   // the class rises: the data run ends, the Truncate run begins
      if (e.after == 0) j.de[p] = i;
      if (e.cls == 2) j.re[p] = i;
    }
    if (on && e.kind == 'T' && j.trunc_out && tpos < j.trunc_cap) {
      const uint64_t room = j.trunc_cap - tpos, cnt = tcnt < room ? tcnt : room;
      const u8* body = j.fixed + j.ev_body[i];
      for (uint64_t t = 0; t < cnt; t++) {
        j.trunc_out[2 * (tpos + t)] = (uint64_t)ld32a(body + 8 * t) | ((uint64_t)ld32a(body + 8 * t + 4) << 32);   // table_id, schema_slot
        j.trunc_out[2 * (tpos + t) + 1] = i;
      }
    }
    // touched: neighbouring lanes with the same (pass, word) fold their bits into the first of them, which issues the one atomicOr
    uint32_t s = 0;
    bool row = on && j.touched && p < j.passes_cap && ol_is_row(e.kind);
    if (row) { s = j.ev_slot[i]; row = s < j.n_slots; }
    const uint64_t key = row ? p * j.W + (s >> 6) : kNone64;
    uint64_t bits = row ? 1ull << (s & 63) : 0ull;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint64_t ok = __shfl(key, (lane + d) & 63, 64), ob = __shfl(bits, (lane + d) & 63, 64);
      if (lane + d < 64 && ok == key) bits |= ob;
    }
    const uint64_t before = __shfl_up(key, 1, 64);
    if (row && (lane == 0 || before != key)) {
      if (p == p_in && (s >> 6) < kOlTouchWords) atomicOr(&tw[s >> 6], (unsigned long long)bits);
      else atomicOr(&j.touched[key], (unsigned long long)bits);
    }
  }
  __syncthreads();
  if (threadIdx.x < kOlTouchWords && tw[threadIdx.x]) atomicOr(&j.touched[p_in * j.W + threadIdx.x], tw[threadIdx.x]);   // (set bits: a row of p_in, p_in < passes_cap)
}

// a thread per written pass: what no event of the pass knows — the ends no lane set, the last pass's end, the truncate entries' count —
// and the copy of its touched words; the grid's first threads also copy the census out
__global__ __launch_bounds__(256) void k_ol_fix(OutlineJob j) {
  if (*j.bad != kNone64) return;
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t np = j.hdr[OL_H_PASSES], nt = j.hdr[OL_H_TRUNC], P = np < j.passes_cap ? np : j.passes_cap, end = j.first + j.n;
  if (t < P) {
    const bool last = t + 1 == np;
    if (j.passes_out) {
      unsigned long long* po = j.passes_out + 7 * t;
      const uint64_t pe = last ? end : po[3], d = j.de[t], r = j.re[t], tf = j.tf[t];
      po[1] = d == kNone64 ? pe : d; po[2] = r == kNone64 ? pe : r; po[3] = pe;
      po[5] = tf; po[6] = (last ? nt : j.tf[t + 1]) - tf;
    }
    if (j.ends_out && last) j.ends_out[t] = end;
    if (j.touched_out) for (uint32_t w = 0; w < j.W; w++) j.touched_out[t * j.W + w] = j.touched[t * j.W + w];
  }
  if (j.slots_out && t < (uint64_t)j.n_slots * 12) {
    const uint64_t s = t / 12, c = t % 12;
    j.slots_out[t] = c < 6 ? j.crow[s * 6 + c] : j.cfirst[s * 6 + c - 6];
  }
}

// ---- the DuckLake atomic-batch plan (etlg_ducklake_plan, include/etlg.h: the rule is stated there). Replay filter, the cut into groups
// of 16 and the grouping into operations are a selection, a rank that restarts at every window and run boundaries inside a group: with
// rpre[i] the retained members in front of event i, a member's rank in its window w is rpre[i] - rpre[first_event of w], the groups of w
// are ceil(retained of w / 16), and the retained members in event order are one dense list that the groups cut without a gap — a group
// is the stretch between two neighbouring starts of that list. Launches, none of which exchanges a word between its workgroups: the
// windows checked (k_dlp_mark), per tile the members and the retained ones plus a code byte per event (k_dlp_tiles), their scan by one
// workgroup (k_dlp_scan), rpre (k_dlp_write), the groups per window (k_dlp_pass) and their scan (etlg_k_scan_lens), per member its place
// in the dense list, its group's start and its records (k_dlp_members), per group its fields and the count of its ops (k_dlp_groups),
// their scan, and the ops (k_dlp_ops). The caps are the caller's, so nothing is read back in between; the outputs are written from
// scratch by the last two kernels, which do nothing once a status word is set. Every loop runs to a launch parameter: tile / 256
// chunks, log2(n_passes) and log2(records) steps of a search, 16 members.
DEV bool dlp_any_status(const DlpJob& j) {
  return j.hdr[DLP_H_BAD] != kNone64 || j.hdr[DLP_H_REFUSED] != kNone64 || j.hdr[DLP_H_NOTPREFIX] != kNone64 || j.hdr[DLP_H_NEEDSHOST] != kNone64;
}
// the window that can hold event i: the last one that starts at or in front of it (every earlier one has ended by then); ~0 none
DEV uint64_t dlp_window(const DlpJob& j, uint64_t i) {
  uint64_t lo = 0, hi = j.n_passes;
  while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if (j.passes[7 * mid] <= i) lo = mid + 1; else hi = mid; }
  if (!lo || i >= j.passes[7 * (lo - 1) + 1]) return kNone64;
  return lo - 1;
}
// event i as the code byte of a member inside a window, 0 otherwise; *refused: the reason the sink refuses it, 0 none
DEV uint32_t dlp_code(const DlpJob& j, uint64_t i, uint32_t* refused) {
  *refused = 0;
  const uint32_t kind = j.ev_kind[i];
  if (!ol_is_row(kind) || j.ev_slot[i] != j.slot || dlp_window(j, i) == kNone64) return 0u;
  const uint32_t fl = j.ev_flags[i], old = fl & 3u;
  uint32_t cat = ETLG_DLP_CAT_INSERT;
  if (kind == 'U') {
    cat = (fl & ETLG_FLAG_PARTIAL) ? ETLG_DLP_CAT_UPDATE_PARTIAL : old == ETLG_OLD_NONE ? ETLG_DLP_CAT_REPLACE : ETLG_DLP_CAT_UPDATE_FULL;
    if (j.no_ident) *refused = ETLG_DLP_R_UPDATE_IDENTITY;
  } else if (kind == 'D') {
    cat = ETLG_DLP_CAT_DELETE;
    if (j.no_ident) *refused = ETLG_DLP_R_DELETE_IDENTITY;
    else if (old == ETLG_OLD_NONE) *refused = ETLG_DLP_R_DELETE_NO_OLD;
  }
  const uint64_t lsn = j.ev_commit[i];
  const bool keep = !j.has_wm || lsn > j.wm_lsn || (lsn == j.wm_lsn && j.ev_ord[i] > j.wm_ord);   // compare_sequence_keys: lexicographic
  return 1u | (keep ? 2u : 0u) | (cat << 2);
}

__global__ __launch_bounds__(256) void k_dlp_mark(DlpJob j) {
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= j.n_passes) return;
  const uint64_t fe = j.passes[7 * p], de = j.passes[7 * p + 1];
  if (fe > de || de > j.n_events || (p && fe < j.passes[7 * (p - 1) + 1])) atomicMin(&j.hdr[DLP_H_BAD], (unsigned long long)p);
}

__global__ __launch_bounds__(256) void k_dlp_tiles(DlpJob j) {
  __shared__ uint64_t lds[4];
  if (j.hdr[DLP_H_BAD] != kNone64) return;
  const uint64_t k0 = (uint64_t)blockIdx.x * j.tile;
  if (k0 >= j.n_events) return;
  const uint64_t k1 = k0 + j.tile < j.n_events ? k0 + j.tile : j.n_events;
  uint64_t members = 0, kept = 0, refused = kNone64;
  for (uint64_t i = k0 + threadIdx.x; i < k1; i += 256) {
    uint32_t why;
    const uint32_t code = dlp_code(j, i, &why);
    j.code[i] = (uint8_t)code;
    members += code & 1u;
    kept += (code >> 1) & 1u;
    if (why && i * 4 + why < refused) refused = i * 4 + why;
  }
  members = block_sum64(members, lds); kept = block_sum64(kept, lds); refused = block_min64(refused, lds);
  if (threadIdx.x == 0) {
    j.tsum[2 * (uint64_t)blockIdx.x] = members; j.tsum[2 * (uint64_t)blockIdx.x + 1] = kept;
    if (refused != kNone64) atomicMin(&j.hdr[DLP_H_REFUSED], (unsigned long long)refused);
  }
}

// one workgroup: both sums per tile become the sums in front of the tile; the totals are the call's counts
__global__ __launch_bounds__(256) void k_dlp_scan(DlpJob j) {
  __shared__ uint64_t lds[4];
  if (j.hdr[DLP_H_BAD] != kNone64) return;
  const uint64_t members = carry_scan64(j.tsum, j.n_tiles, 2, lds), kept = carry_scan64(j.tsum + 1, j.n_tiles, 2, lds);
  if (threadIdx.x == 0) { j.hdr[DLP_H_MEMBERS] = members; j.hdr[DLP_H_RETAINED] = kept; j.rpre[j.n_events] = kept; }
}

__global__ __launch_bounds__(256) void k_dlp_write(DlpJob j) {
  __shared__ uint64_t lds[4];
  if (j.hdr[DLP_H_BAD] != kNone64) return;
  const uint64_t k0 = (uint64_t)blockIdx.x * j.tile;
  if (k0 >= j.n_events) return;
  const uint64_t k1 = k0 + j.tile < j.n_events ? k0 + j.tile : j.n_events;
  uint64_t carry = j.tsum[2 * (uint64_t)blockIdx.x + 1];
  for (uint64_t kb = k0; kb < k1; kb += 256) {   // (uniform trip count: every lane takes part in every scan)
    const uint64_t i = kb + threadIdx.x;
    const bool on = i < k1;
    uint64_t tot;
    const uint64_t ex = block_scan_excl64(on ? (j.code[i] >> 1) & 1u : 0u, lds, &tot);
    if (on) j.rpre[i] = carry + ex;
    carry += tot;
  }
}

// a thread per window: its groups (the windows were checked: data_end <= n_events)
__global__ __launch_bounds__(256) void k_dlp_pass(DlpJob j) {
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= j.n_passes || j.hdr[DLP_H_BAD] != kNone64) return;
  const uint64_t kept = j.rpre[j.passes[7 * p + 1]] - j.rpre[j.passes[7 * p]];
  j.glens[p] = (uint32_t)((kept + kDlpGroup - 1) / kDlpGroup);
}

// the record of event i in an object: its lower bound in row_event when that entry is the event's, ~0 when the event has none
DEV uint64_t dlp_record(const DlpRecs& r, uint64_t i) {
  if (!r.n_rows) return kNone64;
  const uint64_t at = cut_lower_bound(r.row_event, 0, r.n_rows - 1, i);
  return at < r.n_rows && r.row_event[at] == i ? at : kNone64;
}

// a thread per event: a retained member takes its place in the dense list, opens its group when its rank in the window is a multiple
// of 16, and finds its records; a dropped member behind a retained one of its window is the not-prefix case
__global__ __launch_bounds__(256) void k_dlp_members(DlpJob j) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= j.n_events || j.hdr[DLP_H_BAD] != kNone64) return;
  if (i == 0) j.gstart[j.gpre[j.n_passes]] = j.rpre[j.n_events];   // the end of the last group
  const uint32_t code = j.code[i];
  if (!(code & 1u)) return;
  const uint64_t w = dlp_window(j, i), m = j.rpre[i], rank = m - j.rpre[j.passes[7 * w]];
  if (!(code & 2u)) { if (rank) atomicMin(&j.hdr[DLP_H_NOTPREFIX], (unsigned long long)i); return; }
  j.dense[m] = i;
  if (rank % kDlpGroup == 0) j.gstart[(uint64_t)j.gpre[w] + rank / kDlpGroup] = m;
  const uint32_t cat = code >> 2;
  uint64_t a = kNone64, b = kNone64;
  bool missing = false;
  if (cat == ETLG_DLP_CAT_UPDATE_PARTIAL) {
    if (j.u.given) { a = dlp_record(j.u, i); missing = a == kNone64; }
  } else {
    if (cat != ETLG_DLP_CAT_DELETE && j.t.given) { a = dlp_record(j.t, i); missing = a == kNone64; }
    if (cat != ETLG_DLP_CAT_INSERT && j.p.given) { b = dlp_record(j.p, i); missing = missing || b == kNone64; }
  }
  j.mpos[2 * m] = a; j.mpos[2 * m + 1] = b;
  if (missing) atomicMin(&j.hdr[DLP_H_NEEDSHOST], (unsigned long long)i);
}

// a thread per group: its fields but op_first, its range for etlg_ducklake_fingerprints, and the count of its ops — a maximal run of
// Inserts or of Deletes is one op, a full Update or a Replace two, a partial Update one (prepare_table_mutations)
__global__ __launch_bounds__(256) void k_dlp_groups(DlpJob j) {
  const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= j.n_events || dlp_any_status(j)) return;
  if (g >= (uint64_t)j.gpre[j.n_passes]) { j.oplens[g] = 0; return; }
  const uint64_t m0 = j.gstart[g], cnt = j.gstart[g + 1] - m0, first = j.dense[m0], last = j.dense[m0 + cnt - 1];
  uint32_t cats[5] = {0, 0, 0, 0, 0}, ops = 0, before = ~0u;
#pragma unroll
  for (uint32_t k = 0; k < kDlpGroup; k++) {
    if (k >= cnt) break;
    const uint32_t cat = j.code[j.dense[m0 + k]] >> 2;
#pragma unroll
    for (uint32_t c = 0; c < 5; c++) cats[c] += cat == c;
    if (cat == ETLG_DLP_CAT_INSERT || cat == ETLG_DLP_CAT_DELETE) ops += cat != before;
    else ops += cat == ETLG_DLP_CAT_UPDATE_PARTIAL ? 1u : 2u;
    before = cat;
  }
  j.oplens[g] = ops;
  if (g >= j.batches_cap) return;
  if (j.ranges_out) { j.ranges_out[3 * g] = first; j.ranges_out[3 * g + 1] = last + 1; j.ranges_out[3 * g + 2] = j.seed; }
  if (j.batches_out) {
    unsigned long long* o = j.batches_out + kDlpBatchWords * g;
    o[0] = first; o[1] = last + 1; o[2] = j.ev_start[first]; o[3] = j.ev_commit[last];
    o[4] = j.ev_commit[first]; o[5] = j.ev_ord[first]; o[6] = j.ev_ord[last]; o[7] = dlp_window(j, first);
    o[9] = cnt | ((uint64_t)ops << 32);
    o[10] = cats[0] | ((uint64_t)cats[1] << 32); o[11] = cats[2] | ((uint64_t)cats[3] << 32); o[12] = cats[4];
  }
}

DEV void dlp_emit(const DlpJob& j, uint64_t k, uint32_t kind, uint32_t origin, uint64_t first, uint64_t n, uint64_t rec) {
  if (!j.ops_out || k >= j.ops_cap) return;
  unsigned long long* o = j.ops_out + kDlpOpWords * k;
  o[0] = kind | ((uint64_t)origin << 32); o[1] = first; o[2] = n; o[3] = rec;
}

// a thread per group: op_first, and its ops behind those of the groups in front; the grid's first thread leaves the two counts
__global__ __launch_bounds__(256) void k_dlp_ops(DlpJob j) {
  const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= j.n_events || dlp_any_status(j)) return;
  const uint64_t G = (uint64_t)j.gpre[j.n_passes];
  if (g == 0) { j.hdr[DLP_H_BATCHES] = G; j.hdr[DLP_H_OPS] = (uint64_t)j.opre[j.n_events]; }
  if (g >= G) return;
  const uint64_t m0 = j.gstart[g], cnt = j.gstart[g + 1] - m0;
  uint64_t k = (uint64_t)j.opre[g];
  if (j.batches_out && g < j.batches_cap) j.batches_out[kDlpBatchWords * g + 8] = k;
  if (!j.ops_out || k >= j.ops_cap) return;
  uint64_t run_first = 0, run_n = 0, run_rec = 0;
  uint32_t run_cat = ~0u;
  for (uint32_t t = 0; t <= kDlpGroup; t++) {   // one step past the last member closes the run in progress
    const bool on = t < cnt;
    const uint64_t i = on ? j.dense[m0 + t] : 0;
    const uint32_t cat = on ? j.code[i] >> 2 : ~0u;
    if (run_n && cat != run_cat) {
      const bool ins = run_cat == ETLG_DLP_CAT_INSERT;
      dlp_emit(j, k++, ins ? ETLG_DLP_OP_UPSERT : ETLG_DLP_OP_DELETE, ins ? ETLG_DLP_ORIGIN_NONE : ETLG_DLP_ORIGIN_DELETE, run_first, run_n, run_rec);
      run_n = 0;
    }
    if (!on) break;
    const uint64_t a = j.mpos[2 * (m0 + t)], b = j.mpos[2 * (m0 + t) + 1];
    if (cat == ETLG_DLP_CAT_INSERT || cat == ETLG_DLP_CAT_DELETE) {
      if (!run_n) { run_first = i; run_cat = cat; run_rec = cat == ETLG_DLP_CAT_INSERT ? a : b; }
      run_n++;
    } else if (cat == ETLG_DLP_CAT_UPDATE_PARTIAL) {
      dlp_emit(j, k++, ETLG_DLP_OP_UPDATE, ETLG_DLP_ORIGIN_NONE, i, 1, a);
    } else {
      dlp_emit(j, k++, ETLG_DLP_OP_DELETE, cat == ETLG_DLP_CAT_UPDATE_FULL ? ETLG_DLP_ORIGIN_UPDATE : ETLG_DLP_ORIGIN_REPLACE, i, 1, b);
      dlp_emit(j, k++, ETLG_DLP_OP_UPSERT, ETLG_DLP_ORIGIN_NONE, i, 1, a);
    }
  }
}

// ---- the Snowflake row-batch plan (etlg_snowflake_plan, include/etlg.h: the rule is stated there). What encode_insert / _update /
// _delete and RowBatchBuilder::push_row decide per row is a selection, three refusals and a byte counter that resets at every flush;
// like the apply loop's budget rule above, the reset is not associative, and it decomposes the same way: the NDJSON object's
// row_offsets q ARE the prefix sums of the row lengths, and the segment that STARTS at row a of a window whose retained rows end at
// win_end ends at next(a) = min(win_end, max(a + 1, the smallest e with q[e + 1] - q[a] >= flush)), whatever came before a. A window's
// segments are the orbit of its first retained row under next, cut where it reaches win_end, and the p-th is reached through the jump
// levels next^(2^k) named by the bits of p. With no status set the retained members of a window are a suffix of its members and each
// has a row, so they are the last `retained` rows in front of the lower bound of data_end in row_event. Launches, none of which
// exchanges a word between its workgroups: the windows checked (k_sfp_mark), per tile the members and the retained ones, a code byte per
// event and the lowest failing event and event without a row (k_sfp_tiles), the scan by one workgroup (k_sfp_scan), both prefixes per
// event (k_sfp_write), the not-prefix test (k_sfp_members), next per row (k_sfp_next), a squaring per level (k_cut_level), per window
// its rows and the count of its segments through the levels (k_sfp_pass), their scan (etlg_k_scan_lens), the windows (k_sfp_windows)
// and the segments (k_sfp_emit). The host sizes the levels and the emit grid from the object's n_rows and n_bytes — two neighbouring
// segments of a window hold at least `flush` bytes — so nothing is read back in between. Every loop runs to a launch parameter: tile /
// 256 chunks, log2(n_passes) and log2(n_rows) steps of a search, `levels` jumps.
DEV bool sfp_any_status(const SfpJob& j) {
  return j.hdr[SFP_H_BAD] != kNone64 || j.hdr[SFP_H_FAILED] != kNone64 || j.hdr[SFP_H_NOTPREFIX] != kNone64 || j.hdr[SFP_H_NEEDSHOST] != kNone64;
}
// the window that can hold event i: the last one that starts at or in front of it (every earlier one has ended by then); ~0 none
DEV uint64_t sfp_window(const SfpJob& j, uint64_t i) {
  uint64_t lo = 0, hi = j.n_passes;
  while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if (j.passes[7 * mid] <= i) lo = mid + 1; else hi = mid; }
  if (!lo || i >= j.passes[7 * (lo - 1) + 1]) return kNone64;
  return lo - 1;
}
// the rows of the object whose event lies in front of event i
DEV uint64_t sfp_rows_before(const SfpJob& j, uint64_t i) { return j.n_rows ? cut_lower_bound(j.row_event, 0, j.n_rows - 1, i) : 0; }

__global__ __launch_bounds__(256) void k_sfp_mark(SfpJob j) {
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= j.n_passes) return;
  const uint64_t fe = j.passes[7 * p], de = j.passes[7 * p + 1];
  if (fe > de || de > j.n_events || (p && fe < j.passes[7 * (p - 1) + 1])) atomicMin(&j.hdr[SFP_H_BAD], (unsigned long long)p);
}

// a code byte per event, the tile's members and retained members, and the two minima: the lowest failing event (with its reason in the
// low bits) and the lowest retained, non-failing member without a row. row_event == null: the object has no rows to look at (NEEDS_HOST)
__global__ __launch_bounds__(256) void k_sfp_tiles(SfpJob j) {
  __shared__ uint64_t lds[4];
  if (j.hdr[SFP_H_BAD] != kNone64) return;
  const uint64_t k0 = (uint64_t)blockIdx.x * j.tile;
  if (k0 >= j.n_events) return;
  const uint64_t k1 = k0 + j.tile < j.n_events ? k0 + j.tile : j.n_events;
  uint64_t members = 0, kept = 0, failed = kNone64, norow = kNone64;
  for (uint64_t i = k0 + threadIdx.x; i < k1; i += 256) {
    const uint32_t kind = j.ev_kind[i];
    uint32_t code = 0, why = 0;
    if (ol_is_row(kind) && j.ev_slot[i] == j.slot && sfp_window(j, i) != kNone64) {
      const uint32_t fl = j.ev_flags[i];
      const uint64_t lsn = j.zero_keys ? 0 : j.ev_commit[i], ord = j.zero_keys ? 0 : j.ev_ord[i];
      const bool keep = !j.has_c || lsn > j.c_lsn || (lsn == j.c_lsn && ord > j.c_ord);   // committed_offset >= offset drops it
      code = 1u | (keep ? 2u : 0u);
      if (kind == 'U' && (fl & ETLG_FLAG_PARTIAL)) why = ETLG_SFP_R_PARTIAL_UPDATE;          // refused in front of the filter
      else if (keep && kind == 'D' && (fl & 3u) == ETLG_OLD_NONE) why = ETLG_SFP_R_DELETE_NO_OLD;
      else if (keep && j.row_event) {
        const uint64_t r = sfp_rows_before(j, i);
        if (r >= j.n_rows || j.row_event[r] != i) { if (i < norow) norow = i; }
        else if (j.q[r + 1] - j.q[r] > j.max_row) why = ETLG_SFP_R_ROW_TOO_LARGE;
      }
    }
    j.code[i] = (uint8_t)code;
    members += code & 1u;
    kept += (code >> 1) & 1u;
    if (why && i * 4 + why < failed) failed = i * 4 + why;
  }
  members = block_sum64(members, lds); kept = block_sum64(kept, lds); failed = block_min64(failed, lds); norow = block_min64(norow, lds);
  if (threadIdx.x == 0) {
    j.tsum[2 * (uint64_t)blockIdx.x] = members; j.tsum[2 * (uint64_t)blockIdx.x + 1] = kept;
    if (failed != kNone64) atomicMin(&j.hdr[SFP_H_FAILED], (unsigned long long)failed);
    if (norow != kNone64) atomicMin(&j.hdr[SFP_H_NEEDSHOST], (unsigned long long)norow);
  }
}

// one workgroup: both sums per tile become the sums in front of the tile; the totals are the call's counts; the length of the row
// that is too large, for the reference's message
__global__ __launch_bounds__(256) void k_sfp_scan(SfpJob j) {
  __shared__ uint64_t lds[4];
  if (j.hdr[SFP_H_BAD] != kNone64) return;
  const uint64_t members = carry_scan64(j.tsum, j.n_tiles, 2, lds), kept = carry_scan64(j.tsum + 1, j.n_tiles, 2, lds);
  if (threadIdx.x == 0) {
    j.hdr[SFP_H_MEMBERS] = members; j.hdr[SFP_H_RETAINED] = kept; j.pre[2 * j.n_events] = members; j.pre[2 * j.n_events + 1] = kept;
    const uint64_t failed = j.hdr[SFP_H_FAILED];
    if (failed != kNone64 && (failed & 3u) == ETLG_SFP_R_ROW_TOO_LARGE) { const uint64_t r = sfp_rows_before(j, failed >> 2); j.hdr[SFP_H_ROWBYTES] = j.q[r + 1] - j.q[r]; }
  }
}

__global__ __launch_bounds__(256) void k_sfp_write(SfpJob j) {
  __shared__ uint64_t lds[4];
  if (j.hdr[SFP_H_BAD] != kNone64) return;
  const uint64_t k0 = (uint64_t)blockIdx.x * j.tile;
  if (k0 >= j.n_events) return;
  const uint64_t k1 = k0 + j.tile < j.n_events ? k0 + j.tile : j.n_events;
  uint64_t cm = j.tsum[2 * (uint64_t)blockIdx.x], cr = j.tsum[2 * (uint64_t)blockIdx.x + 1];
  for (uint64_t kb = k0; kb < k1; kb += 256) {   // (uniform trip count: every lane takes part in every scan)
    const uint64_t i = kb + threadIdx.x;
    const bool on = i < k1;
    const uint32_t code = on ? j.code[i] : 0u;
    uint64_t tot;   // members in the high half, retained members in the low half: a chunk has at most 256 of each
    const uint64_t ex = block_scan_excl64(((uint64_t)(code & 1u) << 32) | ((code >> 1) & 1u), lds, &tot);
    if (on) { j.pre[2 * i] = cm + (ex >> 32); j.pre[2 * i + 1] = cr + (ex & 0xFFFFFFFFull); }
    cm += tot >> 32; cr += tot & 0xFFFFFFFFull;
  }
}

// a thread per event: a dropped member behind a retained one of its window is the not-prefix case
__global__ __launch_bounds__(256) void k_sfp_members(SfpJob j) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= j.n_events || j.hdr[SFP_H_BAD] != kNone64) return;
  if ((j.code[i] & 3u) != 1u) return;
  const uint64_t w = sfp_window(j, i);
  if (j.pre[2 * i + 1] != j.pre[2 * j.passes[7 * w] + 1]) atomicMin(&j.hdr[SFP_H_NOTPREFIX], (unsigned long long)i);
}

// a thread per row, and two more: where the segment that starts at the row ends. Rows n_rows and n_rows + 1 are the end of every orbit.
__global__ __launch_bounds__(256) void k_sfp_next(SfpJob j) {
  const uint64_t a = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (a > j.n_rows + 1) return;   // (no status test: the squarings behind this launch index with what it writes, which is a row or the end whatever the passes hold)
  uint64_t nx = j.n_rows + 1;
  if (a < j.n_rows && j.row_event) {
    nx = a + 1;
    const uint64_t w = sfp_window(j, j.row_event[a]);
    if (w != kNone64) {
      const uint64_t win_end = sfp_rows_before(j, j.passes[7 * w + 1]);                   // > a: the row's event lies in front of data_end
      const uint64_t k = cut_lower_bound(j.q, a + 1, j.n_rows, j.q[a] + j.flush);         // q[k] - q[a] >= flush first holds at k (n_rows + 1: never)
      if (k - 1 > nx) nx = k - 1;
      if (win_end < nx) nx = win_end;
    }
  }
  j.jump[a] = (uint32_t)nx;
}

// a thread per window: its retained rows and the count of its segments; a workgroup's bytes go into the call's total in one add
__global__ __launch_bounds__(256) void k_sfp_pass(SfpJob j) {
  __shared__ uint64_t lds[4];
  if (sfp_any_status(j)) return;
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint64_t bytes = 0;
  if (p < j.n_passes) {
    const uint64_t fe = j.passes[7 * p], de = j.passes[7 * p + 1], kept = j.pre[2 * de + 1] - j.pre[2 * fe + 1];
    const uint64_t end_row = sfp_rows_before(j, de), first_row = end_row - kept, W = j.n_rows + 2;
    uint64_t n = 0;
    if (kept) {
      uint64_t pos = first_row;
      n = 1;
      for (uint32_t k = j.levels; k-- > 0;) { const uint64_t nx = j.jump[(uint64_t)k * W + pos]; if (nx < end_row) { pos = nx; n += 1ull << k; } }
      bytes = j.q[end_row] - j.q[first_row];
    }
    j.wrow[2 * p] = first_row; j.wrow[2 * p + 1] = end_row;
    j.slens[p] = (uint32_t)n;
  }
  bytes = block_sum64(bytes, lds);
  if (threadIdx.x == 0 && bytes) atomicAdd(&j.hdr[SFP_H_BYTES], (unsigned long long)bytes);
}

// a thread per window: its entry; the grid's first thread leaves the count of all segments
__global__ __launch_bounds__(256) void k_sfp_windows(SfpJob j) {
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= j.n_passes || sfp_any_status(j)) return;
  if (p == 0) j.hdr[SFP_H_SEGS] = (uint64_t)j.spre[j.n_passes];
  if (!j.windows_out) return;
  const uint64_t fe = j.passes[7 * p], de = j.passes[7 * p + 1], first_row = j.wrow[2 * p], end_row = j.wrow[2 * p + 1];
  unsigned long long* o = j.windows_out + kSfpWinWords * p;
  o[0] = (uint64_t)j.spre[p]; o[1] = j.slens[p]; o[2] = first_row; o[3] = end_row;
  o[4] = j.pre[2 * de] - j.pre[2 * fe]; o[5] = j.pre[2 * de + 1] - j.pre[2 * fe + 1];
  o[6] = end_row > first_row ? j.q[end_row] - j.q[first_row] : 0;
}

// a thread per segment that can be written: its window by a search in the windows' offsets (of equal offsets the last: the windows in
// front of it are empty), its first row through the levels named by the bits of its index in the window
__global__ __launch_bounds__(256) void k_sfp_emit(SfpJob j) {
  const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= j.segs_cap || sfp_any_status(j) || s >= (uint64_t)j.spre[j.n_passes]) return;
  uint64_t lo = 0, hi = j.n_passes;
  while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if ((uint64_t)j.spre[mid] <= s) lo = mid + 1; else hi = mid; }
  const uint64_t w = lo - 1, p = s - (uint64_t)j.spre[w], W = j.n_rows + 2;
  uint64_t pos = j.wrow[2 * w];
  for (uint32_t k = 0; k < j.levels; k++) if ((p >> k) & 1u) pos = j.jump[(uint64_t)k * W + pos];
  const uint64_t end = j.jump[pos], first = j.row_event[pos], last = j.row_event[end - 1], len0 = j.q[pos + 1] - j.q[pos];
  unsigned long long* o = j.segs_out + kSfpSegWords * s;
  o[0] = w; o[1] = pos; o[2] = end; o[3] = first; o[4] = last; o[5] = j.q[pos]; o[6] = j.q[end]; o[7] = len0;
  o[8] = j.zero_keys ? 0 : j.ev_commit[first]; o[9] = j.zero_keys ? 0 : j.ev_ord[first];
  o[10] = j.zero_keys ? 0 : j.ev_commit[last]; o[11] = j.zero_keys ? 0 : j.ev_ord[last];
  o[12] = (p || len0 >= j.flush) ? 1u : 0u;
}

// ---- the ClickHouse statement plan (etlg_clickhouse_plan, include/etlg.h: the rule is stated there). What write_events_inner refuses is
// a test per event; what insert_rows cuts is a byte counter that restarts with every statement, and it decomposes as the two rules
// above do: the RowBinary object's row_offsets q ARE the prefix sums of the row lengths, and the statement that STARTS at row a of a
// window whose rows end at win_end ends at next(a) = min(win_end, the smallest e > a with q[e] - q[a] >= budget), whatever came before
// a. A window's statements are the orbit of its first row under next, cut where it reaches win_end, and the p-th is reached through the
// jump levels next^(2^k) named by the bits of p. With no status set every member of a window has a row and the object holds no other
// row of the window's events, so the window's rows are the last `members` rows in front of the lower bound of data_end in row_event.
// Launches, none of which exchanges a word between its workgroups: the windows checked (k_chp_mark), per tile the members, a code byte
// per event and the lowest failing event and member without a row (k_chp_tiles), the scan by one workgroup and the windows of those two
// events (k_chp_scan), the prefix per event (k_chp_write), next per row (k_chp_next), a squaring per level (k_cut_level), per window its
// rows and the count of its statements through the levels (k_chp_pass), their scan (etlg_k_scan_lens), the windows (k_chp_windows) and
// the statements (k_chp_emit). The host sizes the levels and the emit grid from the object's n_rows and n_bytes — every statement of a
// window but its last holds at least `budget` bytes — so nothing is read back in between. Every loop runs to a launch parameter: tile /
// 256 chunks, log2(n_passes) and log2(n_rows) steps of a search, `levels` jumps.
DEV bool chp_any_status(const ChpJob& j) { return j.hdr[CHP_H_BAD] != kNone64 || j.hdr[CHP_H_FAILED] != kNone64 || j.hdr[CHP_H_NEEDSHOST] != kNone64; }
// the window that can hold event i: the last one that starts at or in front of it (every earlier one has ended by then); ~0 none
template <class J> DEV uint64_t chp_window(const J& j, uint64_t i) {   // (J: ChpJob, BqpJob)
  uint64_t lo = 0, hi = j.n_passes;
  while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if (j.passes[7 * mid] <= i) lo = mid + 1; else hi = mid; }
  if (!lo || i >= j.passes[7 * (lo - 1) + 1]) return kNone64;
  return lo - 1;
}
// the rows of the object whose event lies in front of event i
template <class J> DEV uint64_t chp_rows_before(const J& j, uint64_t i) { return j.n_rows ? cut_lower_bound(j.row_event, 0, j.n_rows - 1, i) : 0; }

// a thread per window: the lowest one that descends, overlaps its predecessor or ends past the events
template <class J> DEV void chp_mark(const J& j) {
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= j.n_passes) return;
  const uint64_t fe = j.passes[7 * p], de = j.passes[7 * p + 1];
  if (fe > de || de > j.n_events || (p && fe < j.passes[7 * (p - 1) + 1])) atomicMin(&j.hdr[CHP_H_BAD], (unsigned long long)p);
}
__global__ __launch_bounds__(256) void k_chp_mark(ChpJob j) { chp_mark(j); }

// a code byte per event, the tile's members, and the two minima: the lowest failing event (with its reason in the low bits; the tests
// run in the reference's order, so an event has one reason) and the lowest member that does not fail and has no row. rows == 0: the
// object's status is NEEDS_HOST, it has no rows to look at (n_rows == 0 with rows != 0 is an object that is merely empty)
__global__ __launch_bounds__(256) void k_chp_tiles(ChpJob j) {
  __shared__ uint64_t lds[4];
  if (j.hdr[CHP_H_BAD] != kNone64) return;
  const uint64_t k0 = (uint64_t)blockIdx.x * j.tile;
  if (k0 >= j.n_events) return;
  const uint64_t k1 = k0 + j.tile < j.n_events ? k0 + j.tile : j.n_events;
  uint64_t members = 0, failed = kNone64, norow = kNone64;
  for (uint64_t i = k0 + threadIdx.x; i < k1; i += 256) {
    const uint32_t kind = j.ev_kind[i];
    uint32_t code = 0, why = 0;
    if (ol_is_row(kind) && j.ev_slot[i] == j.slot && chp_window(j, i) != kNone64) {
      const uint32_t fl = j.ev_flags[i], old = fl & 3u;
      code = 1u;
      if (kind == 'U') {
        if (fl & ETLG_FLAG_PARTIAL) why = ETLG_CHP_R_PARTIAL_UPDATE;
        else if (j.replacing && !j.ident_ok) why = ETLG_CHP_R_UPDATE_IDENTITY;
      } else if (kind == 'D') {
        if (old == ETLG_OLD_NONE) why = ETLG_CHP_R_DELETE_NO_OLD;
        else if (old == ETLG_OLD_KEY) why = !j.width_ok ? ETLG_CHP_R_KEY_WIDTH : !j.ident_ok ? ETLG_CHP_R_KEY_IDENTITY : 0u;
      }
      if (!why && j.rows) {
        const uint64_t r = chp_rows_before(j, i);
        if (r >= j.n_rows || j.row_event[r] != i) { if (i < norow) norow = i; }
      }
    }
    j.code[i] = (uint8_t)code;
    members += code;
    if (why && i * 8 + why < failed) failed = i * 8 + why;
  }
  members = block_sum64(members, lds); failed = block_min64(failed, lds); norow = block_min64(norow, lds);
  if (threadIdx.x == 0) {
    j.tsum[blockIdx.x] = members;
    if (failed != kNone64) atomicMin(&j.hdr[CHP_H_FAILED], (unsigned long long)failed);
    if (norow != kNone64) atomicMin(&j.hdr[CHP_H_NEEDSHOST], (unsigned long long)norow);
  }
}

// one workgroup: the sums per tile become the sums in front of the tile; the total is the call's count; the windows that hold the
// failing event and the member without a row, for the host that plans again with the passes in front
__global__ __launch_bounds__(256) void k_chp_scan(ChpJob j) {
  __shared__ uint64_t lds[4];
  if (j.hdr[CHP_H_BAD] != kNone64) return;
  const uint64_t members = carry_scan64(j.tsum, j.n_tiles, 1, lds);
  if (threadIdx.x == 0) {
    j.hdr[CHP_H_MEMBERS] = members; j.pre[j.n_events] = members;
    const uint64_t failed = j.hdr[CHP_H_FAILED], norow = j.hdr[CHP_H_NEEDSHOST];
    if (failed != kNone64) j.hdr[CHP_H_FAILPASS] = chp_window(j, failed >> 3);
    if (norow != kNone64) j.hdr[CHP_H_NOROWPASS] = chp_window(j, norow);
  }
}

// the members in front of every event of a tile, from the code bytes and the tile's carry
// (bit: which bit of the code byte is counted, with the tile carries `tsum` and the prefix `pre` that belong to it)
template <class J> DEV void chp_write_bit(const J& j, uint64_t* lds, uint32_t bit, const unsigned long long* tsum, unsigned long long* pre) {
  if (j.hdr[CHP_H_BAD] != kNone64) return;
  const uint64_t k0 = (uint64_t)blockIdx.x * j.tile;
  if (k0 >= j.n_events) return;
  const uint64_t k1 = k0 + j.tile < j.n_events ? k0 + j.tile : j.n_events;
  uint64_t carry = tsum[blockIdx.x];
  for (uint64_t kb = k0; kb < k1; kb += 256) {   // (uniform trip count: every lane takes part in every scan)
    const uint64_t i = kb + threadIdx.x;
    const bool on = i < k1;
    uint64_t tot;
    const uint64_t ex = block_scan_excl64(on ? (j.code[i] >> bit) & 1u : 0u, lds, &tot);
    if (on) pre[i] = carry + ex;
    carry += tot;
  }
}
template <class J> DEV void chp_write(const J& j, uint64_t* lds) { chp_write_bit(j, lds, 0u, j.tsum, j.pre); }
__global__ __launch_bounds__(256) void k_chp_write(ChpJob j) {
  __shared__ uint64_t lds[4];
  chp_write(j, lds);
}

// a thread per row, and two more: where the statement that starts at the row ends. Rows n_rows and n_rows + 1 are the end of every orbit.
__global__ __launch_bounds__(256) void k_chp_next(ChpJob j) {
  const uint64_t a = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (a > j.n_rows + 1) return;   // (no status test: the squarings behind this launch index with what it writes, which is a row or the end whatever the passes hold)
  uint64_t nx = j.n_rows + 1;
  if (a < j.n_rows) {
    nx = a + 1;
    const uint64_t w = chp_window(j, j.row_event[a]);
    if (w != kNone64) {
      const uint64_t win_end = chp_rows_before(j, j.passes[7 * w + 1]);                   // > a: the row's event lies in front of data_end
      nx = cut_lower_bound(j.q, a + 1, j.n_rows, j.q[a] + j.budget);                      // q[nx] - q[a] >= budget first holds at nx (n_rows + 1: never); the sum stays below 2^64
      if (win_end < nx) nx = win_end;
    }
  }
  j.jump[a] = (uint32_t)nx;
}

// a thread per window: its rows and the count of its statements; a workgroup's bytes go into the call's total in one add
__global__ __launch_bounds__(256) void k_chp_pass(ChpJob j) {
  __shared__ uint64_t lds[4];
  if (chp_any_status(j)) return;
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint64_t bytes = 0;
  if (p < j.n_passes) {
    const uint64_t fe = j.passes[7 * p], de = j.passes[7 * p + 1], members = j.pre[de] - j.pre[fe];
    const uint64_t end_row = chp_rows_before(j, de), first_row = end_row - members, W = j.n_rows + 2;
    uint64_t n = 0;
    if (members) {
      uint64_t pos = first_row;
      n = 1;
      for (uint32_t k = j.levels; k-- > 0;) { const uint64_t nx = j.jump[(uint64_t)k * W + pos]; if (nx < end_row) { pos = nx; n += 1ull << k; } }
      bytes = j.q[end_row] - j.q[first_row];
    }
    j.wrow[2 * p] = first_row; j.wrow[2 * p + 1] = end_row;
    j.slens[p] = (uint32_t)n;
  }
  bytes = block_sum64(bytes, lds);
  if (threadIdx.x == 0 && bytes) atomicAdd(&j.hdr[CHP_H_BYTES], (unsigned long long)bytes);
}

// a thread per window: its entry; the grid's first thread leaves the count of all statements
__global__ __launch_bounds__(256) void k_chp_windows(ChpJob j) {
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= j.n_passes || chp_any_status(j)) return;
  if (p == 0) j.hdr[CHP_H_STMTS] = (uint64_t)j.spre[j.n_passes];
  if (!j.windows_out) return;
  const uint64_t fe = j.passes[7 * p], de = j.passes[7 * p + 1], first_row = j.wrow[2 * p], end_row = j.wrow[2 * p + 1];
  unsigned long long* o = j.windows_out + kChpWinWords * p;
  o[0] = (uint64_t)j.spre[p]; o[1] = j.slens[p]; o[2] = first_row; o[3] = end_row;
  o[4] = j.pre[de] - j.pre[fe];
  o[5] = end_row > first_row ? j.q[end_row] - j.q[first_row] : 0;
}

// a thread per statement that can be written: its window by a search in the windows' offsets (of equal offsets the last: the windows in
// front of it are empty), its first row through the levels named by the bits of its index in the window
__global__ __launch_bounds__(256) void k_chp_emit(ChpJob j) {
  const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= j.stmts_cap || chp_any_status(j) || s >= (uint64_t)j.spre[j.n_passes]) return;
  uint64_t lo = 0, hi = j.n_passes;
  while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if ((uint64_t)j.spre[mid] <= s) lo = mid + 1; else hi = mid; }
  const uint64_t w = lo - 1, p = s - (uint64_t)j.spre[w], W = j.n_rows + 2;
  uint64_t pos = j.wrow[2 * w];
  for (uint32_t k = 0; k < j.levels; k++) if ((p >> k) & 1u) pos = j.jump[(uint64_t)k * W + pos];
  const uint64_t end = j.jump[pos];
  unsigned long long* o = j.stmts_out + kChpStmtWords * s;
  o[0] = w; o[1] = pos; o[2] = end; o[3] = j.row_event[pos]; o[4] = j.row_event[end - 1]; o[5] = j.q[pos]; o[6] = j.q[end];
}

// ---- the BigQuery request plan (etlg_bigquery_plan, include/etlg.h: the rule is stated there). What write_events refuses is a test per
// event; a window with a member is one append request of all its rows, so there is no byte counter to restart and no jump level. What
// differs from the ClickHouse plan above: an Update that changes the primary key is TWO rows of one event, so a window's rows are not
// its last `members` rows — both ends come from a lower bound in row_event (of first_event and of data_end), which takes both rows of
// an event wherever the window begins or ends. Launches, none of which exchanges a word between its workgroups: the windows checked
// (k_bqp_mark), per tile the members, a code byte per event and the lowest failing event and member without a row (k_bqp_tiles), the
// scan by one workgroup and the windows of those two events (k_bqp_scan), the prefix per event (k_bqp_write), per window its rows, its
// bytes and whether it has a request (k_bqp_pass), the scan of those 0 / 1 lengths (etlg_k_scan_lens), the windows (k_bqp_windows) and
// the requests (k_bqp_emit). A table-copy batch is k_bqp_copy alone. Every loop runs to a launch parameter: tile / 256 chunks,
// log2(n_passes) and log2(n_rows) steps of a search.
DEV bool bqp_any_status(const BqpJob& j) { return j.hdr[BQP_H_BAD] != kNone64 || j.hdr[BQP_H_FAILED] != kNone64 || j.hdr[BQP_H_NEEDSHOST] != kNone64; }

__global__ __launch_bounds__(256) void k_bqp_mark(BqpJob j) { chp_mark(j); }

// as k_chp_tiles, with this sink's refusals: the tests of one event in the reference's order (bigquery/core.rs:997-1034), so an event
// has one reason. rows == 0: the object's status is NEEDS_HOST, it has no rows to look at
__global__ __launch_bounds__(256) void k_bqp_tiles(BqpJob j) {
  __shared__ uint64_t lds[4];
  if (j.hdr[BQP_H_BAD] != kNone64) return;
  const uint64_t k0 = (uint64_t)blockIdx.x * j.tile;
  if (k0 >= j.n_events) return;
  const uint64_t k1 = k0 + j.tile < j.n_events ? k0 + j.tile : j.n_events;
  uint64_t members = 0, failed = kNone64, norow = kNone64;
  for (uint64_t i = k0 + threadIdx.x; i < k1; i += 256) {
    const uint32_t kind = j.ev_kind[i];
    uint32_t code = 0, why = 0;
    if (ol_is_row(kind) && j.ev_slot[i] == j.slot && chp_window(j, i) != kNone64) {
      const uint32_t fl = j.ev_flags[i], old = fl & 3u;
      code = 1u;
      if (kind == 'U' && (fl & ETLG_FLAG_PARTIAL)) why = ETLG_BQP_R_PARTIAL_UPDATE;                   // bigquery_update_new_row comes before the old image is looked at
      else if (kind == 'U' && old == ETLG_OLD_NONE) why = j.ident_pk ? 0u : ETLG_BQP_R_UPDATE_NO_OLD_IDENTITY;
      else if (kind == 'D' && old == ETLG_OLD_NONE) why = ETLG_BQP_R_DELETE_NO_OLD;
      else if (kind != 'I' && old == ETLG_OLD_KEY) why = !j.width_ok ? ETLG_BQP_R_KEY_WIDTH : !j.ident_pk ? ETLG_BQP_R_KEY_IDENTITY : 0u;   // the width before the identity
      if (!why && j.rows) {
        const uint64_t r = chp_rows_before(j, i);
        if (r >= j.n_rows || j.row_event[r] != i) { if (i < norow) norow = i; }
      }
    }
    j.code[i] = (uint8_t)code;
    members += code;
    if (why && i * 8 + why < failed) failed = i * 8 + why;
  }
  members = block_sum64(members, lds); failed = block_min64(failed, lds); norow = block_min64(norow, lds);
  if (threadIdx.x == 0) {
    j.tsum[blockIdx.x] = members;
    if (failed != kNone64) atomicMin(&j.hdr[BQP_H_FAILED], (unsigned long long)failed);
    if (norow != kNone64) atomicMin(&j.hdr[BQP_H_NEEDSHOST], (unsigned long long)norow);
  }
}

// one workgroup, as k_chp_scan: the sums in front of every tile, the total, the windows of the failing event and of the member without a row
__global__ __launch_bounds__(256) void k_bqp_scan(BqpJob j) {
  __shared__ uint64_t lds[4];
  if (j.hdr[BQP_H_BAD] != kNone64) return;
  const uint64_t members = carry_scan64(j.tsum, j.n_tiles, 1, lds);
  if (threadIdx.x == 0) {
    j.hdr[BQP_H_MEMBERS] = members; j.pre[j.n_events] = members;
    const uint64_t failed = j.hdr[BQP_H_FAILED], norow = j.hdr[BQP_H_NEEDSHOST];
    if (failed != kNone64) j.hdr[BQP_H_FAILPASS] = chp_window(j, failed >> 3);
    if (norow != kNone64) j.hdr[BQP_H_NOROWPASS] = chp_window(j, norow);
  }
}

__global__ __launch_bounds__(256) void k_bqp_write(BqpJob j) {
  __shared__ uint64_t lds[4];
  chp_write(j, lds);
}

// a thread per window: its rows by two lower bounds — never end_row - members: an event of two rows would push first_row into the window
// in front —, a 0 / 1 length for its request; a workgroup's bytes, rows and second rows go into the call's totals in one add each
__global__ __launch_bounds__(256) void k_bqp_pass(BqpJob j) {
  __shared__ uint64_t lds[4];
  if (bqp_any_status(j)) return;
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint64_t bytes = 0, rows = 0, two = 0;
  if (p < j.n_passes) {
    const uint64_t fe = j.passes[7 * p], de = j.passes[7 * p + 1], members = j.pre[de] - j.pre[fe];
    const uint64_t first_row = chp_rows_before(j, fe), end_row = chp_rows_before(j, de);
    if (members) { rows = end_row - first_row; two = rows - members; bytes = j.q[end_row] - j.q[first_row]; }   // (no status: every member has a row, the object no other row of these events)
    j.wrow[2 * p] = first_row; j.wrow[2 * p + 1] = end_row;
    j.slens[p] = members ? 1u : 0u;
  }
  bytes = block_sum64(bytes, lds); rows = block_sum64(rows, lds); two = block_sum64(two, lds);
  if (threadIdx.x == 0 && rows) {
    atomicAdd(&j.hdr[BQP_H_BYTES], (unsigned long long)bytes); atomicAdd(&j.hdr[BQP_H_ROWS], (unsigned long long)rows);
    if (two) atomicAdd(&j.hdr[BQP_H_TWOROW], (unsigned long long)two);
  }
}

// a thread per window: its entry; the grid's first thread leaves the count of all requests
__global__ __launch_bounds__(256) void k_bqp_windows(BqpJob j) {
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= j.n_passes || bqp_any_status(j)) return;
  if (p == 0) j.hdr[BQP_H_REQS] = (uint64_t)j.spre[j.n_passes];
  if (!j.windows_out) return;
  const uint64_t fe = j.passes[7 * p], de = j.passes[7 * p + 1], first_row = j.wrow[2 * p], end_row = j.wrow[2 * p + 1], members = j.pre[de] - j.pre[fe];
  unsigned long long* o = j.windows_out + kBqpWinWords * p;
  o[0] = (uint64_t)j.spre[p]; o[1] = j.slens[p]; o[2] = first_row; o[3] = end_row; o[4] = members;
  o[5] = members ? end_row - first_row - members : 0;
  o[6] = members ? j.q[end_row] - j.q[first_row] : 0;
}

// a thread per request that can be written: its window by a search in the windows' offsets (of equal offsets the last: the windows in
// front of it have no request)
__global__ __launch_bounds__(256) void k_bqp_emit(BqpJob j) {
  const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= j.reqs_cap || bqp_any_status(j) || s >= (uint64_t)j.spre[j.n_passes]) return;
  uint64_t lo = 0, hi = j.n_passes;
  while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if ((uint64_t)j.spre[mid] <= s) lo = mid + 1; else hi = mid; }
  const uint64_t w = lo - 1, first_row = j.wrow[2 * w], end_row = j.wrow[2 * w + 1];
  unsigned long long* o = j.reqs_out + kBqpReqWords * s;
  o[0] = w; o[1] = first_row; o[2] = end_row; o[3] = j.row_event[first_row]; o[4] = j.row_event[end_row - 1]; o[5] = j.q[first_row]; o[6] = j.q[end_row];
  o[7] = j.pre[j.passes[7 * w + 1]] - j.pre[j.passes[7 * w]];
}

// a table-copy batch: calculate_target_batches_for_table_copy (bigquery/core.rs:1760-1784) and split_table_rows (:1790-1827) in closed
// form, a thread per request that can be written; the grid's first thread leaves the counts and the one window. n_rows == 0: no request
__global__ __launch_bounds__(256) void k_bqp_copy(BqpJob j) {
  const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x, R = j.n_rows;
  const uint64_t est = R ? j.q[1] - j.q[0] : 0;                       // encoded_len() of the first row alone
  const uint64_t per = est ? j.budget / est : R;                      // MAX_BATCH_SIZE_BYTES.checked_div(estimated_row_size).unwrap_or(total_rows)
  const uint64_t target = !R ? 0 : per ? (R + per - 1) / per : 1;
  uint64_t nsub = R ? 1 : 0, each = R, extra = 0;
  if (!(R <= 1 || target == 1 || R <= target)) {
    const uint64_t opt = (R + target - 1) / target;                   // > 0: R > target > 1
    nsub = (R + opt - 1) / opt; each = R / nsub; extra = R % nsub;
  }
  if (s == 0) {
    const uint64_t bytes = R ? j.q[R] - j.q[0] : 0;
    j.hdr[BQP_H_REQS] = nsub; j.hdr[BQP_H_MEMBERS] = R; j.hdr[BQP_H_ROWS] = R; j.hdr[BQP_H_BYTES] = bytes; j.hdr[BQP_H_EST] = est; j.hdr[BQP_H_TARGET] = target;
    if (j.windows_out) { unsigned long long* o = j.windows_out; o[0] = 0; o[1] = nsub; o[2] = 0; o[3] = R; o[4] = R; o[5] = 0; o[6] = bytes; }
  }
  if (s >= j.reqs_cap || s >= nsub) return;
  const uint64_t first_row = s * each + (s < extra ? s : extra), end_row = first_row + each + (s < extra ? 1 : 0);
  unsigned long long* o = j.reqs_out + kBqpReqWords * s;
  o[0] = 0; o[1] = first_row; o[2] = end_row; o[3] = j.row_event[first_row]; o[4] = j.row_event[end_row - 1]; o[5] = j.q[first_row]; o[6] = j.q[end_row];
  o[7] = end_row - first_row;
}

// ---- the Iceberg write plan (etlg_iceberg_plan, include/etlg.h: the rule is stated there). The event side is the BigQuery plan's with
// this sink's three refusals (one test per event kind) and one event per row; it keeps a second prefix, of the Insert / Update / Delete
// events of the slot's TABLE under another slot, so that a window's first such event is a lower bound in it. The bitmap side is what no
// other plan has: every write is a slice of every column of the changelog object, and a slice wants the bits of a row range counted.
// Windows go from one row to the whole object, so no thread walks a range: the words of every bitmap that can hold a counted bit lie in
// one word space, bpre is the running popcount in front of every word of it, and a range's count is two reads of bpre and the two masked
// words at its ends (icp_ones). Launches, none of which exchanges a word between its workgroups: the windows checked (k_icp_mark), per
// event tile the members, the other-slot events, a code byte per event and the two minima, per word tile the set bits (k_icp_tiles),
// the three scans by one workgroup and the windows of the two minima (k_icp_scan), the three prefixes (k_icp_write), per window its
// rows, its other-slot event and whether it has a write (k_icp_pass), the scan of those 0 / 1 lengths (etlg_k_scan_lens), the windows
// (k_icp_windows), and a thread per write and column for the slices with one more per write for its entry (k_icp_emit). A table-copy
// batch has no event side: the word tiles, their scan and prefix, and k_icp_emit, whose first thread leaves the counts and the one
// window. Every loop runs to a launch parameter: tile / 256 and wtile / 256 chunks, log2 steps of a search in n_passes, n_rows,
// n_events or n_bitmaps.
DEV bool icp_any_status(const IcpJob& j) { return j.hdr[ICP_H_BAD] != kNone64 || j.hdr[ICP_H_FAILED] != kNone64 || j.hdr[ICP_H_NEEDSHOST] != kNone64; }
// word g of the word space: of the last bitmap that starts at or in front of it (the bases ascend strictly; g < n_words)
DEV uint64_t icp_word(const IcpJob& j, uint64_t g) {
  uint32_t lo = 0, hi = j.n_bitmaps;
  while (hi - lo > 1) { const uint32_t mid = lo + ((hi - lo) >> 1); if (j.bitmaps[mid].base <= g) lo = mid; else hi = mid; }
  return j.bitmaps[lo].words[g - j.bitmaps[lo].base];
}
// set bits of bitmap b in the bit range [lo, hi), lo <= hi <= its bits: whole words through bpre, the two edge words masked. A word is
// read only where the range cuts it, so nothing at or behind the bitmap's last word is touched when hi ends on a word
DEV uint64_t icp_ones(const IcpJob& j, uint32_t b, uint64_t lo, uint64_t hi) {
  const IcpBitmap m = j.bitmaps[b];
  uint64_t n = j.bpre[m.base + (hi >> 6)] - j.bpre[m.base + (lo >> 6)];
  if (lo & 63) n -= (uint64_t)__builtin_popcountll(m.words[lo >> 6] & ((1ull << (lo & 63)) - 1));
  if (hi & 63) n += (uint64_t)__builtin_popcountll(m.words[hi >> 6] & ((1ull << (hi & 63)) - 1));
  return n;
}

__global__ __launch_bounds__(256) void k_icp_mark(IcpJob j) { chp_mark(j); }

// the first n_tiles workgroups, as k_bqp_tiles with this sink's refusals (iceberg_update_row core.rs:636-652, iceberg_delete_row
// :655-680: one test per event kind, so an event has one reason) and bit 1 of the code byte: an Insert / Update / Delete of the slot's
// table under another slot, in a window or not. The workgroups behind them: the set bits of a tile of the word space
__global__ __launch_bounds__(256) void k_icp_tiles(IcpJob j) {
  __shared__ uint64_t lds[4];
  if (blockIdx.x >= j.n_tiles) {
    const uint64_t t = blockIdx.x - j.n_tiles, g0 = t * j.wtile, g1 = g0 + j.wtile < j.n_words ? g0 + j.wtile : j.n_words;
    uint64_t ones = 0;
    for (uint64_t g = g0 + threadIdx.x; g < g1; g += 256) ones += (uint64_t)__builtin_popcountll(icp_word(j, g));
    ones = block_sum64(ones, lds);
    if (threadIdx.x == 0) j.bsum[t] = ones;
    return;
  }
  if (j.hdr[ICP_H_BAD] != kNone64) return;
  const uint64_t k0 = (uint64_t)blockIdx.x * j.tile;
  if (k0 >= j.n_events) return;
  const uint64_t k1 = k0 + j.tile < j.n_events ? k0 + j.tile : j.n_events;
  uint64_t members = 0, foreign = 0, failed = kNone64, norow = kNone64;
  for (uint64_t i = k0 + threadIdx.x; i < k1; i += 256) {
    const uint32_t kind = j.ev_kind[i];
    uint32_t code = 0, why = 0;
    if (ol_is_row(kind)) {
      if (j.ev_slot[i] != j.slot) code = j.ev_table[i] == j.table_id ? 2u : 0u;
      else if (chp_window(j, i) != kNone64) {
        const uint32_t fl = j.ev_flags[i], old = fl & 3u;
        code = 1u;
        if (kind == 'U') why = (fl & ETLG_FLAG_PARTIAL) ? ETLG_ICE_PARTIAL_UPDATE : 0u;
        else if (kind == 'D') why = old == ETLG_OLD_KEY ? ETLG_ICE_KEY_ONLY_DELETE : old == ETLG_OLD_NONE ? ETLG_ICE_DELETE_WITHOUT_OLD_ROW : 0u;
        if (!why) {
          const uint64_t r = chp_rows_before(j, i);
          if (r >= j.n_rows || j.row_event[r] != i) { if (i < norow) norow = i; }
        }
      }
    }
    j.code[i] = (uint8_t)code;
    members += code & 1u; foreign += code >> 1;
    if (why && i * 8 + why < failed) failed = i * 8 + why;
  }
  members = block_sum64(members, lds); foreign = block_sum64(foreign, lds); failed = block_min64(failed, lds); norow = block_min64(norow, lds);
  if (threadIdx.x == 0) {
    j.tsum[blockIdx.x] = members; j.fsum[blockIdx.x] = foreign;
    if (failed != kNone64) atomicMin(&j.hdr[ICP_H_FAILED], (unsigned long long)failed);
    if (norow != kNone64) atomicMin(&j.hdr[ICP_H_NEEDSHOST], (unsigned long long)norow);
  }
}

// one workgroup, as k_bqp_scan, over three rows of tile sums: the word tiles' first (it does not depend on the passes), then the members
// and the other-slot events
__global__ __launch_bounds__(256) void k_icp_scan(IcpJob j) {
  __shared__ uint64_t lds[4];
  const uint64_t ones = carry_scan64(j.bsum, j.n_wtiles, 1, lds);
  if (threadIdx.x == 0) j.bpre[j.n_words] = ones;
  if (!j.n_tiles || j.hdr[ICP_H_BAD] != kNone64) return;
  const uint64_t members = carry_scan64(j.tsum, j.n_tiles, 1, lds), foreign = carry_scan64(j.fsum, j.n_tiles, 1, lds);
  if (threadIdx.x == 0) {
    j.hdr[ICP_H_MEMBERS] = members; j.pre[j.n_events] = members; j.fpre[j.n_events] = foreign;
    const uint64_t failed = j.hdr[ICP_H_FAILED], norow = j.hdr[ICP_H_NEEDSHOST];
    if (failed != kNone64) j.hdr[ICP_H_FAILPASS] = chp_window(j, failed >> 3);
    if (norow != kNone64) j.hdr[ICP_H_NOROWPASS] = chp_window(j, norow);
  }
}

// the first n_tiles workgroups: both prefixes per event of a tile; the workgroups behind them: the set bits in front of every word of a
// tile of the word space
__global__ __launch_bounds__(256) void k_icp_write(IcpJob j) {
  __shared__ uint64_t lds[4];
  if (blockIdx.x < j.n_tiles) { chp_write_bit(j, lds, 0u, j.tsum, j.pre); chp_write_bit(j, lds, 1u, j.fsum, j.fpre); return; }
  const uint64_t t = blockIdx.x - j.n_tiles, g0 = t * j.wtile, g1 = g0 + j.wtile < j.n_words ? g0 + j.wtile : j.n_words;
  uint64_t carry = j.bsum[t];
  for (uint64_t gb = g0; gb < g1; gb += 256) {   // (uniform trip count: every lane takes part in every scan)
    const uint64_t g = gb + threadIdx.x;
    const bool on = g < g1;
    uint64_t tot;
    const uint64_t ex = block_scan_excl64(on ? (uint64_t)__builtin_popcountll(icp_word(j, g)) : 0ull, lds, &tot);
    if (on) j.bpre[g] = carry + ex;
    carry += tot;
  }
}

// a thread per window: its rows by two lower bounds in row_event, its first other-slot event by one in fpre, a 0 / 1 length for its
// write; a workgroup's rows and mixed windows go into the call's totals in one add each
__global__ __launch_bounds__(256) void k_icp_pass(IcpJob j) {
  __shared__ uint64_t lds[4];
  if (icp_any_status(j)) return;
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint64_t rows = 0, mixed = 0;
  if (p < j.n_passes) {
    const uint64_t fe = j.passes[7 * p], de = j.passes[7 * p + 1], members = j.pre[de] - j.pre[fe];
    const uint64_t first_row = chp_rows_before(j, fe), end_row = chp_rows_before(j, de);
    // a window with a member: fpre[e] > fpre[fe] first holds at e = the event + 1 (fe < e <= de: fpre[de] is such an entry)
    const uint64_t other = members && j.fpre[de] != j.fpre[fe] ? cut_lower_bound(j.fpre, fe + 1, de, j.fpre[fe] + 1) - 1 : kNone64;
    if (members) rows = end_row - first_row;   // (no status: every member has a row, the object no other row of these events)
    mixed = other != kNone64 ? 1u : 0u;
    j.wrow[3 * p] = first_row; j.wrow[3 * p + 1] = end_row; j.wrow[3 * p + 2] = other;
    j.slens[p] = members ? 1u : 0u;
  }
  rows = block_sum64(rows, lds); mixed = block_sum64(mixed, lds);
  if (threadIdx.x == 0) {
    if (rows) atomicAdd(&j.hdr[ICP_H_ROWS], (unsigned long long)rows);
    if (mixed) atomicAdd(&j.hdr[ICP_H_MIXED], (unsigned long long)mixed);
  }
}

// a thread per window: its entry; the grid's first thread leaves the count of all writes
__global__ __launch_bounds__(256) void k_icp_windows(IcpJob j) {
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= j.n_passes || icp_any_status(j)) return;
  if (p == 0) j.hdr[ICP_H_WRITES] = (uint64_t)j.spre[j.n_passes];
  if (!j.windows_out) return;
  unsigned long long* o = j.windows_out + kIcpWinWords * p;
  o[0] = (uint64_t)j.spre[p]; o[1] = j.slens[p]; o[2] = j.wrow[3 * p]; o[3] = j.wrow[3 * p + 1]; o[4] = j.pre[j.passes[7 * p + 1]] - j.pre[j.passes[7 * p]];
  o[5] = j.wrow[3 * p + 2];
}

// the slice of column c over rows [r0, r1) of the object (r0 < r1 <= n_rows)
DEV void icp_slice(const IcpJob& j, uint32_t c, uint64_t r0, uint64_t r1, unsigned long long* o) {
  const IcpCol k = j.cols[c];
  uint64_t b0 = 0, b1 = 0, c0 = 0, c1 = 0, cn = 0;
  if (k.kind == ETLG_AK_LIST) {
    c0 = (uint64_t)k.offsets[r0]; c1 = (uint64_t)k.offsets[r1];
    if (k.child_width) { b0 = c0 * k.child_width; b1 = c1 * k.child_width; }
    else if (k.child_kind == ETLG_AK_BOOLEAN) { b0 = c0; b1 = c1; }
    else if (k.child_count) { b0 = (uint64_t)k.child_offsets[c0]; b1 = (uint64_t)k.child_offsets[c1]; }   // (no child elements: no child offsets to read)
    if (k.bm_child != kIcpNoBitmap) cn = (c1 - c0) - icp_ones(j, k.bm_child, c0, c1);
  } else if (k.width) { b0 = r0 * k.width; b1 = r1 * k.width; }
  else if (k.kind == ETLG_AK_BOOLEAN) { b0 = r0; b1 = r1; }
  else { b0 = (uint64_t)k.offsets[r0]; b1 = (uint64_t)k.offsets[r1]; }
  o[0] = k.bm_valid != kIcpNoBitmap ? (r1 - r0) - icp_ones(j, k.bm_valid, r0, r1) : 0;
  o[1] = k.bm_deferred != kIcpNoBitmap ? icp_ones(j, k.bm_deferred, r0, r1) : 0;
  o[2] = b0; o[3] = b1; o[4] = c0; o[5] = c1; o[6] = cn;
}

// n_cols + 1 threads per write that can be written: a slice per column, and the write's entry. The write's window comes from a search
// in the windows' offsets (of equal offsets the last: the windows in front of it have no write). A table-copy batch (n_passes == 0) has
// one window over all rows and one write when the object has a row; the grid's first thread leaves its counts and its window
__global__ __launch_bounds__(256) void k_icp_emit(IcpJob j) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x, per = (uint64_t)j.n_cols + 1, s = t / per;
  const uint32_t c = (uint32_t)(t % per);
  const bool copy = j.n_passes == 0;
  if (!copy && icp_any_status(j)) return;
  const uint64_t n_writes = copy ? (j.n_rows ? 1u : 0u) : (uint64_t)j.spre[j.n_passes];
  if (copy && t == 0) {
    j.hdr[ICP_H_WRITES] = n_writes; j.hdr[ICP_H_MEMBERS] = j.n_rows; j.hdr[ICP_H_ROWS] = j.n_rows;
    if (j.windows_out) { unsigned long long* o = j.windows_out; o[0] = 0; o[1] = n_writes; o[2] = 0; o[3] = j.n_rows; o[4] = j.n_rows; o[5] = kNone64; }
  }
  if (s >= j.writes_cap || s >= n_writes) return;
  uint64_t w = 0, first_row = 0, end_row = j.n_rows, members = j.n_rows, other = kNone64;
  if (!copy) {
    uint64_t lo = 0, hi = j.n_passes;
    while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if ((uint64_t)j.spre[mid] <= s) lo = mid + 1; else hi = mid; }
    w = lo - 1; first_row = j.wrow[3 * w]; end_row = j.wrow[3 * w + 1]; other = j.wrow[3 * w + 2];
    members = j.pre[j.passes[7 * w + 1]] - j.pre[j.passes[7 * w]];
  }
  if (c < j.n_cols) { if (j.slices_out) icp_slice(j, c, first_row, end_row, j.slices_out + kIcpSliceWords * (s * j.n_cols + c)); return; }
  if (!j.writes_out) return;
  unsigned long long* o = j.writes_out + kIcpWriteWords * s;
  o[0] = w; o[1] = first_row; o[2] = end_row; o[3] = j.row_event[first_row]; o[4] = j.row_event[end_row - 1]; o[5] = members; o[6] = other;
}

// ---- source payload accounting, event side (etlg_batch_payload, include/etlg.h): what EventBatch::push merges for the events of one
// write_events batch (apply.rs:656-658) and record_processed reports. The arena no longer has a message's value bytes (integers, floats
// and temporals are decoded), so every event is joined to its frame: the frame side (kernels.hip) has listed the frames that take a
// transaction ordinal (rank -> frame) and the rank of every Begin frame. A Begin always yields an event, so the j-th 'B' event is the
// j-th Begin frame, and the frame of an event is the (rank of its Begin + ev_tx_ordinal)-th listed frame; in front of the batch's first
// Begin it is the (ev_tx_ordinal - entry ordinal)-th. The joined frame must carry the event's kind: anything else is a MISMATCH (the
// caller passed other bytes than the batch was decoded from). Launches, none of which exchanges a word between its workgroups: 'B'
// events per tile (k_paye_tiles), their scan by one workgroup (k_paye_scan), the join, ev_bytes and the channels' sums per tile
// (k_paye_join), those scanned (k_paye_sums), the prefix sums of bytes and rows per channel (k_paye_prefix), a lane per range
// (k_paye_ranges). Sums are plain 64-bit adds: a batch's value bytes are below 2^32 per frame and 2^30 frames, far from 2^64.
DEV uint32_t pay_channel(uint32_t kind) { return kind == 'I' ? 0u : kind == 'U' ? 1u : kind == 'D' ? 2u : 3u; }

__global__ __launch_bounds__(256) void k_paye_tiles(PayJob j) {
  __shared__ uint64_t lds[4];
  const uint64_t i0 = (uint64_t)blockIdx.x * j.etile, i1 = i0 + j.etile < j.n_events ? i0 + j.etile : j.n_events;
  uint64_t n = 0;
  for (uint64_t i = i0 + threadIdx.x; i < i1; i += 256) n += j.ev_kind[i] == 'B';
  n = block_sum64(n, lds);
  if (threadIdx.x == 0) j.etb[blockIdx.x] = n;
}

__global__ __launch_bounds__(256) void k_paye_scan(PayJob j) {
  __shared__ uint64_t lds[4];
  (void)carry_scan64(j.etb, j.n_etiles, 1, lds);
}

__global__ __launch_bounds__(256) void k_paye_join(PayJob j) {
  __shared__ uint64_t lds[4];
  const uint64_t i0 = (uint64_t)blockIdx.x * j.etile, i1 = i0 + j.etile < j.n_events ? i0 + j.etile : j.n_events;
  const uint64_t n_cons = j.hdr[PAY_H_COUNTS] & 0xFFFFFFFFull, n_begin = j.hdr[PAY_H_COUNTS] >> 32;
  uint64_t carry = j.copy ? 0 : j.etb[blockIdx.x], sb[3] = {0, 0, 0}, sr[3] = {0, 0, 0};
  for (uint64_t ib = i0; ib < i1; ib += 256) {   // (uniform trip count: every lane takes part in every scan)
    const uint64_t i = ib + threadIdx.x;
    const bool on = i < i1;
    const uint32_t kind = on ? j.ev_kind[i] : 0;
    uint64_t begins = 0;   // 'B' events up to and including this one
    if (!j.copy) {
      const uint64_t v = kind == 'B';
      uint64_t tot;
      begins = carry + block_scan_excl64(v, lds, &tot) + v;
      carry += tot;
    }
    if (on) {
      uint32_t ch = 3, bytes = kPayBad;
      if (j.copy) {   // event i is row i
        ch = 0;
        if (i < j.n_frames) bytes = j.fbytes[i];
      } else {
        const uint64_t ord = j.ev_ord[i];
        uint64_t rank = ~0ull;
        if (begins) { if (begins <= n_begin) rank = (uint64_t)j.brank[begins - 1] + ord; }
        else if (ord >= j.entry_ord) rank = ord - j.entry_ord;
        if (rank < n_cons) {
          const uint32_t f = j.r2f[rank];
          if (j.f_tag[f] == kind) { ch = pay_channel(kind); bytes = j.fbytes[f]; }   // (0 for B / C / R / T, kPayBad for a row message that does not parse)
        }
      }
      if (bytes == kPayBad) { atomicMin(&j.hdr[PAY_H_MISMATCH], (unsigned long long)i); bytes = 0; ch = 3; }
      j.ev_bytes[i] = bytes;
      if (ch < 3) { sb[ch] += bytes; sr[ch] += 1; }
    }
  }
  if (!j.tsum) return;
  for (int k = 0; k < 3; k++) { sb[k] = block_sum64(sb[k], lds); sr[k] = block_sum64(sr[k], lds); }
  if (threadIdx.x == 0) for (int k = 0; k < 3; k++) { j.tsum[6 * (uint64_t)blockIdx.x + k] = sb[k]; j.tsum[6 * (uint64_t)blockIdx.x + 3 + k] = sr[k]; }
}

// one workgroup: each of the six sums per tile becomes the sum in front of the tile
__global__ __launch_bounds__(256) void k_paye_sums(PayJob j) {
  __shared__ uint64_t lds[4];
  for (uint32_t k = 0; k < 6; k++) (void)carry_scan64(j.tsum + k, j.n_etiles, 6, lds);
  if (threadIdx.x < 3) { j.pb[(uint64_t)threadIdx.x * (j.n_events + 1)] = 0; j.pr[(uint64_t)threadIdx.x * (j.n_events + 1)] = 0; }
}

// pb[c][i + 1], pr[c][i + 1] = bytes and rows of channel c over the events [0, i]. One scan per channel: a chunk of 256 events holds
// less than 2^40 bytes, so the rows ride above bit 40 of the same word; the carries are kept apart.
__global__ __launch_bounds__(256) void k_paye_prefix(PayJob j) {
  __shared__ uint64_t lds[4];
  const uint64_t i0 = (uint64_t)blockIdx.x * j.etile, i1 = i0 + j.etile < j.n_events ? i0 + j.etile : j.n_events, W = j.n_events + 1;
  constexpr uint64_t kLow = (1ull << 40) - 1;
  uint64_t cb[3], cr[3];
  for (int k = 0; k < 3; k++) { cb[k] = j.tsum[6 * (uint64_t)blockIdx.x + k]; cr[k] = j.tsum[6 * (uint64_t)blockIdx.x + 3 + k]; }
  for (uint64_t ib = i0; ib < i1; ib += 256) {
    const uint64_t i = ib + threadIdx.x;
    const bool on = i < i1;
    // (an event that did not join counts here with 0 bytes and not in k_paye_join: the call reports MISMATCH and no sum is to be trusted)
    const uint32_t ch = !on ? 3u : j.copy ? 0u : pay_channel(j.ev_kind[i]);
    const uint64_t bytes = on ? j.ev_bytes[i] : 0;
    for (uint32_t k = 0; k < 3; k++) {
      const uint64_t v = ch == k ? (1ull << 40) | bytes : 0;
      uint64_t tot;
      const uint64_t inc = block_scan_excl64(v, lds, &tot) + v;
      if (on) { j.pb[k * W + i + 1] = cb[k] + (inc & kLow); j.pr[k * W + i + 1] = (uint32_t)(cr[k] + (inc >> 40)); }
      cb[k] += tot & kLow; cr[k] += tot >> 40;
    }
  }
}

// range k = the events [cuts[k - 1], cuts[k]), the first from 0, the last up to n_events. Cuts that descend or pass n_events read
// nothing: the range is zero and the call is refused.
__global__ __launch_bounds__(256) void k_paye_ranges(PayJob j) {
  const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (k > j.n_cuts) return;
  const uint64_t lo = k ? j.cuts[k - 1] : 0, hi = k < j.n_cuts ? j.cuts[k] : j.n_events, W = j.n_events + 1;
  unsigned long long* out = j.sums + 8 * k;
  for (int c = 0; c < 8; c++) out[c] = 0;
  if (lo > hi || hi > j.n_events) { j.hdr[PAY_H_BAD_CUTS] = 1; return; }
  for (uint32_t c = 0; c < 3; c++) {
    const uint32_t kind = j.copy ? (uint32_t)ETLG_PK_COPY : c;
    if (j.copy && c) break;
    out[kind] = j.pb[c * W + hi] - j.pb[c * W + lo];
    out[4 + kind] = j.pr[c * W + hi] - j.pr[c * W + lo];
  }
}

// ---- the finish pass (etlg_batch_finish_cells, include/etlg.h): cells a decode left ETLG_CELL_DEFERRED are settled in the arena itself.
// Array literals (parse_cell_from_postgres_text_array, crates/etl/src/postgres/codec/text.rs:163-312) become typed heap entries — header,
// validity bits, element slots or end offsets + bytes (include/etlg.h: etlg_array_hdr) — appended behind the batch's heap; float texts the
// fast rule could not decide get their exactly rounded bits (float_slow.h). One thread per (event, row image, finishable column); a cell
// the device does not settle (a malformed literal, a json element, a numeric element of more than 40 characters) stays DEFERRED for the
// host, exactly as before. Two walks of the text like k_arr_count / k_arr_fill: sizes -> exclusive scan -> entries.
enum : uint32_t { FIN_ARRAYS = 1u, FIN_FLOATS = 2u };

struct FinCell { bool on; uint32_t cls, elem; u8* slot; uint32_t* stw; uint32_t stsh; };
DEV FinCell fin_cell(const FinJob& j, uint64_t t) {
  FinCell c{false, 0, 0, nullptr, nullptr, 0};
  const uint32_t K = 2u * j.maxfin;
  const uint64_t ev = t / K;
  const uint32_t r = (uint32_t)(t % K), img = r / j.maxfin, q = r % j.maxfin;
  if (ev >= j.n_events) return c;
  const uint32_t kind = j.ev_kind[ev];
  if (!(kind == 'I' || kind == 'U' || kind == 'D')) return c;
  const uint32_t s = j.ev_slot[ev];
  if (s >= j.n_slots) return c;
  const SlotRec& sl = j.slots[s];
  if (q >= sl.n_fin) return c;
  const uint32_t col = j.fin[sl.fin_base + q];
  const ColRec& cd = j.cols[sl.cols_base + col];
  const uint32_t ok = kind == 'I' ? 0u : (uint32_t)j.ev_flags[ev] & 3u;
  uint64_t base = j.ev_body[ev];
  uint32_t pos = col, off = cd.off_full();
  if (img == 0) {
    if (ok == ETLG_OLD_NONE) return c;
    if (ok == ETLG_OLD_KEY) { if (!cd.identity()) return c; pos = cd.key_index; off = cd.off_key(); }
  } else {
    if (kind == 'D') return c;
    base += ok == ETLG_OLD_KEY ? sl.row_key : ok == ETLG_OLD_FULL ? sl.row_full : 0u;
  }
  u8* stb = j.fixed + base + pos / 4;
  const uint32_t st = (*stb >> (2 * (pos % 4))) & 3u;
  if (st != ETLG_CELL_DEFERRED) return c;
  c.on = true; c.cls = cd.cls(); c.elem = cd.elem_cls();
  c.slot = j.fixed + base + off;
  c.stw = (uint32_t*)((uintptr_t)stb & ~(uintptr_t)3);
  c.stsh = 8u * (uint32_t)((uintptr_t)stb & 3u) + 2u * (pos % 4);
  return c;
}
DEV bool fin_elem_fixed(uint32_t e) { return e == ETLG_TC_BOOL || e == ETLG_TC_I16 || e == ETLG_TC_I32 || e == ETLG_TC_I64 || e == ETLG_TC_U32 || e == ETLG_TC_F32 || e == ETLG_TC_F64 ||
                                             e == ETLG_TC_DATE || e == ETLG_TC_TIME || e == ETLG_TC_TIMETZ || e == ETLG_TC_TIMESTAMP || e == ETLG_TC_TIMESTAMPTZ || e == ETLG_TC_UUID; }
DEV bool fin_elem_var(uint32_t e) { return e == ETLG_TC_STRING || e == ETLG_TC_BYTEA || e == ETLG_TC_NUMERIC; }

// bytes of the typed entry of one array literal, 0 = not settled here
DEV uint32_t fin_array_bytes(const u8* s, uint32_t n, uint32_t elem, bool exact, uint32_t& cnt) {
  cnt = 0;
  uint64_t data = 0;
  auto none = [](uint32_t) -> u8* { return nullptr; };
  uint32_t e;
  if (fin_elem_fixed(elem)) e = arr_walk<false>(s, n, elem, cnt, [](uint32_t, bool, const uint32_t*, const u8*) {}, none, exact);
  else if (elem == ETLG_TC_NUMERIC) e = arr_walk<false>(s, n, elem, cnt, [&](uint32_t, bool is_null, const uint32_t* w, const u8*) { if (!is_null) data += pad4(w[1]); }, none);
  else if (fin_elem_var(elem)) e = arr_walk<true>(s, n, elem, cnt, [&](uint32_t, bool, const uint32_t* w, const u8*) { data += w[0]; }, none);
  else return 0;
  if (e) return 0;
  const uint64_t tot = 8ull + 4ull * ((cnt + 31u) >> 5) + (fin_elem_fixed(elem) ? (uint64_t)cnt * slot_bytes(elem) : 4ull * cnt + ((data + 3ull) & ~3ull));
  return tot > 0x7FFFFFF0ull ? 0u : (uint32_t)tot;
}

// Thread u of the grid takes cell t = event * K + row, with u = row * n_events + event: the lanes of a wave hold the SAME column of
// consecutive events (one element class, one code path: with t = u every lane of a wave decoded another class, 31 paths one after the
// other — 7.2 ms for the fill of a 30 MB type-matrix batch), while sizes and entries stay in (event, image, column) order.
DEV uint64_t fin_thread_cell(const FinJob& j, uint64_t u) {
  const uint64_t K = 2ull * j.maxfin;
  return (u % j.n_events) * K + u / j.n_events;
}

__global__ __launch_bounds__(256) void k_fin_count(FinJob j) {
  const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= j.n_events * 2ull * j.maxfin) return;
  const uint64_t t = fin_thread_cell(j, u);
  const FinCell c = fin_cell(j, t);
  uint32_t len = 0;
  uint32_t cnt = 0;
  if (c.on && c.cls == ETLG_TC_ARRAY && (j.what & FIN_ARRAYS)) len = fin_array_bytes(j.heap + ld32a(c.slot), ld32a(c.slot + 4), c.elem, (j.what & FIN_FLOATS) != 0, cnt);
  j.lens[t] = len;
  if (len) j.counts[t] = cnt;
}

DEV void fin_tally(const FinJob& j, bool seen, bool arr, bool flt, bool left) {   // one atomic per wave and counter
  const unsigned long long ms = __ballot(seen), ma = __ballot(arr), mf = __ballot(flt), ml = __ballot(left);
  if ((threadIdx.x & 63u) == 0) {
    if (ms) atomicAdd(&j.stats[0], (unsigned long long)__builtin_popcountll(ms));
    if (ma) atomicAdd(&j.stats[1], (unsigned long long)__builtin_popcountll(ma));
    if (mf) atomicAdd(&j.stats[2], (unsigned long long)__builtin_popcountll(mf));
    if (ml) atomicAdd(&j.stats[3], (unsigned long long)__builtin_popcountll(ml));
  }
}

__global__ __launch_bounds__(256) void k_fin_fill(FinJob j) {
  const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const bool in_grid = u < j.n_events * 2ull * j.maxfin;
  const uint64_t t = in_grid ? fin_thread_cell(j, u) : 0;
  FinCell c{false, 0, 0, nullptr, nullptr, 0};
  if (in_grid) c = fin_cell(j, t);
  bool settled = false, was_arr = false, was_flt = false;
  if (c.on) {
  const u8* s = j.heap + ld32a(c.slot);
  const uint32_t n = ld32a(c.slot + 4);
  if ((c.cls == ETLG_TC_F32 || c.cls == ETLG_TC_F64) && (j.what & FIN_FLOATS)) {
    // (the decode validated the grammar: only texts parse_float_fast calls inconclusive are DEFERRED)
    const uint64_t bits = parse_float_exact_t([&](uint32_t i) { return (uint32_t)s[i]; }, n, c.cls == ETLG_TC_F32);
    ((uint32_t*)c.slot)[0] = (uint32_t)bits; ((uint32_t*)c.slot)[1] = (uint32_t)(bits >> 32);
    settled = true; was_flt = true;
  } else if (c.cls == ETLG_TC_ARRAY && (j.what & FIN_ARRAYS) && j.lens && j.lens[t]) {
    const uint32_t bytes = j.lens[t], elem = c.elem;
    const uint64_t at = j.heap_base + (uint64_t)j.offsets[t];
    uint32_t* const e32 = (uint32_t*)(j.heap + at);
    uint32_t cnt = j.counts[t];   // (from the count pass: the header and the validity words come before the elements)
    auto none = [](uint32_t) -> u8* { return nullptr; };
    const bool fixed = fin_elem_fixed(elem), exact = (j.what & FIN_FLOATS) != 0;
    const uint32_t total = cnt, vw = (total + 31u) >> 5, sb = fixed ? slot_bytes(elem) : 0u;
    e32[0] = total; e32[1] = elem | (sb << 8);
    for (uint32_t i = 0; i < vw; i++) e32[2 + i] = 0;
    uint32_t* const valid = e32 + 2;
    if (fixed) {
      uint32_t* const vals = e32 + 2 + vw;
      (void)arr_walk<false>(s, n, elem, cnt, [&](uint32_t k, bool is_null, const uint32_t* w, const u8*) {
        uint32_t* d = vals + (size_t)k * (sb >> 2);
        for (uint32_t q = 0; q < (sb >> 2); q++) d[q] = is_null ? 0u : w[q];
        if (!is_null) valid[k >> 5] |= 1u << (k & 31u);
      }, none, exact);
    } else {
      uint32_t* const ends = e32 + 2 + vw;
      u8* const data = (u8*)(ends + total);
      uint32_t run = 0;
      if (elem == ETLG_TC_NUMERIC) {
        (void)arr_walk<false>(s, n, elem, cnt, [&](uint32_t k, bool is_null, const uint32_t* w, const u8* scratch) {
          if (!is_null) {
            const uint32_t nb = pad4(w[1]);
            heap_copy(data + run, scratch + w[0], w[1]);
            run += nb;
            valid[k >> 5] |= 1u << (k & 31u);
          }
          ends[k] = run;
        }, none);
      } else {
        // text / bytea elements: their bytes leave as the walk unescapes them; element k starts where element k - 1 ended
        uint32_t lens_run = 0;
        (void)arr_walk<true>(s, n, elem, cnt, [&](uint32_t k, bool is_null, const uint32_t* w, const u8*) {
          lens_run += w[0];
          ends[k] = lens_run;
          if (!is_null) valid[k >> 5] |= 1u << (k & 31u);
        }, [&](uint32_t) -> u8* { return data + lens_run; });
        run = lens_run;
        while (run & 3u) data[run++] = 0;
      }
    }
    ((uint32_t*)c.slot)[0] = (uint32_t)at; ((uint32_t*)c.slot)[1] = bytes;
    settled = true; was_arr = true;
  }
  if (settled) atomicAnd(c.stw, ~(3u << c.stsh));   // DEFERRED (3) -> VALUE (0); the other cells of the row share the word
  }
  fin_tally(j, c.on, was_arr, was_flt, c.on && !settled);
}

}  // namespace etlg

extern "C" {

using namespace etlg;

void etlg_k_size_hints(const HintJob* jv, hipStream_t st) {
  const HintJob j = *jv;
  if (j.n_events) hipLaunchKernelGGL(k_size_hints, dim3((uint32_t)((j.n_events + 255) / 256)), dim3(256), 0, st, j);
}

// etlg_batch_cuts: step 0 = q, L and total (grids from n and the tile), step 1 = the jump levels, the count and the cuts (grids from L
// and from the host's bound of the cuts, min(cuts_cap, L, (carry_in + total) / budget); threads past the device's count exit)
void etlg_k_cuts(const CutJob* jv, int step, uint64_t emit_bound, hipStream_t st) {
  const CutJob j = *jv;
  if (step == 0) {
    if (j.n_tiles) hipLaunchKernelGGL(k_cut_tiles, dim3(j.n_tiles), dim3(256), 0, st, j);
    hipLaunchKernelGGL(k_cut_scan, dim3(1), dim3(256), 0, st, j);
    if (j.n_tiles) hipLaunchKernelGGL(k_cut_write, dim3(j.n_tiles), dim3(256), 0, st, j);
    return;
  }
  const uint64_t W = j.L + 2;
  const uint32_t nb = (uint32_t)((W + 255) / 256);
  hipLaunchKernelGGL(k_cut_next, dim3(nb), dim3(256), 0, st, j);
  for (uint32_t k = 1; k < j.levels; k++) hipLaunchKernelGGL(k_cut_level, dim3(nb), dim3(256), 0, st, j.jump + (uint64_t)(k - 1) * W, j.jump + (uint64_t)k * W, W);
  hipLaunchKernelGGL(k_cut_count, dim3(1), dim3(64), 0, st, j);
  if (emit_bound) hipLaunchKernelGGL(k_cut_emit, dim3((uint32_t)((emit_bound + 255) / 256)), dim3(256), 0, st, j);
}

// etlg_batch_outline: every launch in one piece (the grids come from n, the tile, n_cuts and the caller's caps; threads past the device's
// counts exit). passes_cap is the host's bound of the passes that can be written, min(the caller's cap, n)
void etlg_k_outline(const OutlineJob* jv, hipStream_t st) {
  const OutlineJob j = *jv;
  if (j.n_cuts) hipLaunchKernelGGL(k_ol_mark, dim3((uint32_t)((j.n_cuts + 255) / 256)), dim3(256), 0, st, j);
  if (j.n_tiles) hipLaunchKernelGGL(k_ol_tiles, dim3(j.n_tiles), dim3(256), 0, st, j);
  hipLaunchKernelGGL(k_ol_scan, dim3(1), dim3(256), 0, st, j);
  if (j.n_tiles) hipLaunchKernelGGL(k_ol_write, dim3(j.n_tiles), dim3(256), 0, st, j);
  const uint64_t census = j.slots_out ? (uint64_t)j.n_slots * 12 : 0, fix = j.passes_cap > census ? j.passes_cap : census;
  if (fix) hipLaunchKernelGGL(k_ol_fix, dim3((uint32_t)((fix + 255) / 256)), dim3(256), 0, st, j);
}

// etlg_ducklake_plan: every launch in one piece (the grids come from n_events, the tile and n_passes, both > 0; threads past the
// device's counts exit). gblk / oblk: the block sums of the two offset scans ((ceil(n / 256) + 1) words each)
void etlg_k_ducklake_plan(const DlpJob* jv, unsigned long long* gblk, unsigned long long* oblk, hipStream_t st) {
  const DlpJob j = *jv;
  const dim3 per_pass((uint32_t)((j.n_passes + 255) / 256)), per_event((uint32_t)((j.n_events + 255) / 256));
  hipLaunchKernelGGL(k_dlp_mark, per_pass, dim3(256), 0, st, j);
  hipLaunchKernelGGL(k_dlp_tiles, dim3(j.n_tiles), dim3(256), 0, st, j);
  hipLaunchKernelGGL(k_dlp_scan, dim3(1), dim3(256), 0, st, j);
  hipLaunchKernelGGL(k_dlp_write, dim3(j.n_tiles), dim3(256), 0, st, j);
  hipLaunchKernelGGL(k_dlp_pass, per_pass, dim3(256), 0, st, j);
  etlg_k_scan_lens(j.glens, j.n_passes, gblk, (int64_t*)j.gpre, st);
  hipLaunchKernelGGL(k_dlp_members, per_event, dim3(256), 0, st, j);
  hipLaunchKernelGGL(k_dlp_groups, per_event, dim3(256), 0, st, j);
  etlg_k_scan_lens(j.oplens, j.n_events, oblk, (int64_t*)j.opre, st);
  hipLaunchKernelGGL(k_dlp_ops, per_event, dim3(256), 0, st, j);
}

// etlg_snowflake_plan: every launch in one piece (the grids come from n_events, the tile, n_passes — all > 0 —, n_rows and the host's
// bound on the segments that can be written; threads past the device's counts exit). rows == false: the object has no rows (its
// status is NEEDS_HOST), only the statuses in front of that one are worked out. sblk: the block sums of the offset scan
void etlg_k_snowflake_plan(const SfpJob* jv, unsigned long long* sblk, uint64_t emit_bound, bool rows, hipStream_t st) {
  const SfpJob j = *jv;
  const dim3 per_pass((uint32_t)((j.n_passes + 255) / 256)), per_event((uint32_t)((j.n_events + 255) / 256));
  hipLaunchKernelGGL(k_sfp_mark, per_pass, dim3(256), 0, st, j);
  hipLaunchKernelGGL(k_sfp_tiles, dim3(j.n_tiles), dim3(256), 0, st, j);
  hipLaunchKernelGGL(k_sfp_scan, dim3(1), dim3(256), 0, st, j);
  hipLaunchKernelGGL(k_sfp_write, dim3(j.n_tiles), dim3(256), 0, st, j);
  hipLaunchKernelGGL(k_sfp_members, per_event, dim3(256), 0, st, j);
  if (!rows) return;
  const uint64_t W = j.n_rows + 2;
  const uint32_t nb = (uint32_t)((W + 255) / 256);
  hipLaunchKernelGGL(k_sfp_next, dim3(nb), dim3(256), 0, st, j);
  for (uint32_t k = 1; k < j.levels; k++) hipLaunchKernelGGL(k_cut_level, dim3(nb), dim3(256), 0, st, j.jump + (uint64_t)(k - 1) * W, j.jump + (uint64_t)k * W, W);
  hipLaunchKernelGGL(k_sfp_pass, per_pass, dim3(256), 0, st, j);
  etlg_k_scan_lens(j.slens, j.n_passes, sblk, (int64_t*)j.spre, st);
  hipLaunchKernelGGL(k_sfp_windows, per_pass, dim3(256), 0, st, j);
  if (emit_bound) hipLaunchKernelGGL(k_sfp_emit, dim3((uint32_t)((emit_bound + 255) / 256)), dim3(256), 0, st, j);
}

// etlg_clickhouse_plan: every launch in one piece (the grids come from n_events, the tile, n_passes — all > 0 —, n_rows and the host's
// bound on the statements that can be written; threads past the device's counts exit). j.rows == 0: the object has no rows (its
// status is NEEDS_HOST), only the statuses in front of that one are worked out. sblk: the block sums of the offset scan
void etlg_k_clickhouse_plan(const ChpJob* jv, unsigned long long* sblk, uint64_t emit_bound, hipStream_t st) {
  const ChpJob j = *jv;
  const dim3 per_pass((uint32_t)((j.n_passes + 255) / 256));
  hipLaunchKernelGGL(k_chp_mark, per_pass, dim3(256), 0, st, j);
  hipLaunchKernelGGL(k_chp_tiles, dim3(j.n_tiles), dim3(256), 0, st, j);
  hipLaunchKernelGGL(k_chp_scan, dim3(1), dim3(256), 0, st, j);
  if (!j.rows) return;
  hipLaunchKernelGGL(k_chp_write, dim3(j.n_tiles), dim3(256), 0, st, j);
  const uint64_t W = j.n_rows + 2;
  const uint32_t nb = (uint32_t)((W + 255) / 256);
  hipLaunchKernelGGL(k_chp_next, dim3(nb), dim3(256), 0, st, j);
  for (uint32_t k = 1; k < j.levels; k++) hipLaunchKernelGGL(k_cut_level, dim3(nb), dim3(256), 0, st, j.jump + (uint64_t)(k - 1) * W, j.jump + (uint64_t)k * W, W);
  hipLaunchKernelGGL(k_chp_pass, per_pass, dim3(256), 0, st, j);
  etlg_k_scan_lens(j.slens, j.n_passes, sblk, (int64_t*)j.spre, st);
  hipLaunchKernelGGL(k_chp_windows, per_pass, dim3(256), 0, st, j);
  if (emit_bound) hipLaunchKernelGGL(k_chp_emit, dim3((uint32_t)((emit_bound + 255) / 256)), dim3(256), 0, st, j);
}

// etlg_bigquery_plan: every launch in one piece. copy: a table-copy batch, k_bqp_copy alone over max(1, emit_bound) threads (its first
// thread leaves the counts). Else the grids come from n_events, the tile and n_passes — all > 0 — and the host's bound on the requests
// that can be written; j.rows == 0: the object has no rows, only the statuses in front of NEEDS_HOST are worked out
void etlg_k_bigquery_plan(const BqpJob* jv, unsigned long long* sblk, uint64_t emit_bound, bool copy, hipStream_t st) {
  const BqpJob j = *jv;
  if (copy) { hipLaunchKernelGGL(k_bqp_copy, dim3((uint32_t)(((emit_bound ? emit_bound : 1) + 255) / 256)), dim3(256), 0, st, j); return; }
  const dim3 per_pass((uint32_t)((j.n_passes + 255) / 256));
  hipLaunchKernelGGL(k_bqp_mark, per_pass, dim3(256), 0, st, j);
  hipLaunchKernelGGL(k_bqp_tiles, dim3(j.n_tiles), dim3(256), 0, st, j);
  hipLaunchKernelGGL(k_bqp_scan, dim3(1), dim3(256), 0, st, j);
  if (!j.rows) return;
  hipLaunchKernelGGL(k_bqp_write, dim3(j.n_tiles), dim3(256), 0, st, j);
  hipLaunchKernelGGL(k_bqp_pass, per_pass, dim3(256), 0, st, j);
  etlg_k_scan_lens(j.slens, j.n_passes, sblk, (int64_t*)j.spre, st);
  hipLaunchKernelGGL(k_bqp_windows, per_pass, dim3(256), 0, st, j);
  if (emit_bound) hipLaunchKernelGGL(k_bqp_emit, dim3((uint32_t)((emit_bound + 255) / 256)), dim3(256), 0, st, j);
}

// etlg_iceberg_plan: every launch in one piece. The word tiles ride behind the event tiles in k_icp_tiles and k_icp_write (a table-copy
// batch has no event tile: n_tiles == 0, n_passes == 0, and k_icp_emit runs max(1, emit_bound) threads, of which the first leaves the
// counts). emit_bound: (n_cols + 1) threads per write that can be written
void etlg_k_iceberg_plan(const IcpJob* jv, unsigned long long* sblk, uint64_t emit_bound, hipStream_t st) {
  const IcpJob j = *jv;
  const bool copy = j.n_passes == 0;
  const dim3 per_pass((uint32_t)((j.n_passes + 255) / 256)), tiles(j.n_tiles + j.n_wtiles);
  if (!copy) hipLaunchKernelGGL(k_icp_mark, per_pass, dim3(256), 0, st, j);
  if (tiles.x) hipLaunchKernelGGL(k_icp_tiles, tiles, dim3(256), 0, st, j);
  hipLaunchKernelGGL(k_icp_scan, dim3(1), dim3(256), 0, st, j);
  if (tiles.x) hipLaunchKernelGGL(k_icp_write, tiles, dim3(256), 0, st, j);
  if (!copy) {
    hipLaunchKernelGGL(k_icp_pass, per_pass, dim3(256), 0, st, j);
    etlg_k_scan_lens(j.slens, j.n_passes, sblk, (int64_t*)j.spre, st);
    hipLaunchKernelGGL(k_icp_windows, per_pass, dim3(256), 0, st, j);
  } else if (!emit_bound) emit_bound = 1;
  if (emit_bound) hipLaunchKernelGGL(k_icp_emit, dim3((uint32_t)((emit_bound + 255) / 256)), dim3(256), 0, st, j);
}

// etlg_batch_payload, event side, behind the frame side on the same stream (hdr[PAY_H_COUNTS], r2f, brank, fbytes); tsum == null: the
// join alone (ev_bytes and the mismatch), no range sums
void etlg_k_payload_events(const PayJob* jv, hipStream_t st) {
  const PayJob j = *jv;
  if (j.n_etiles) {
    if (!j.copy) {
      hipLaunchKernelGGL(k_paye_tiles, dim3(j.n_etiles), dim3(256), 0, st, j);
      hipLaunchKernelGGL(k_paye_scan, dim3(1), dim3(256), 0, st, j);
    }
    hipLaunchKernelGGL(k_paye_join, dim3(j.n_etiles), dim3(256), 0, st, j);
  }
  if (!j.tsum) return;
  hipLaunchKernelGGL(k_paye_sums, dim3(1), dim3(256), 0, st, j);
  if (j.n_etiles) hipLaunchKernelGGL(k_paye_prefix, dim3(j.n_etiles), dim3(256), 0, st, j);
  hipLaunchKernelGGL(k_paye_ranges, dim3((uint32_t)((j.n_cuts + 1 + 255) / 256)), dim3(256), 0, st, j);
}

void etlg_k_cuts_locate(const unsigned long long* cuts, uint64_t n_cuts, const unsigned long long* row_event, uint64_t n_rows, unsigned long long* rows_out,
                        hipStream_t st) {
  if (n_cuts) hipLaunchKernelGGL(k_cuts_locate, dim3((uint32_t)((n_cuts + 255) / 256)), dim3(256), 0, st, cuts, n_cuts, row_event, n_rows, rows_out);
}

// the finish pass: step 0 = entry sizes of every (event, image, finishable column) + their exclusive scan (blk: (ceil(n / 256) + 1) x u64
// scratch, offsets: n + 1 x i64), step 1 = the entries, the slots and the cell states
void etlg_k_finish(const FinJob* jv, unsigned long long* blk, int64_t* offsets, int step, hipStream_t st) {
  const FinJob j = *jv;
  const uint64_t n = j.n_events * 2ull * j.maxfin;
  if (!n) return;
  const uint32_t nb = (uint32_t)((n + 255) / 256);
  if (step == 0) {
    hipLaunchKernelGGL(k_fin_count, dim3(nb), dim3(256), 0, st, j);
    etlg_k_scan_lens(j.lens, n, blk, offsets, st);
  } else hipLaunchKernelGGL(k_fin_fill, dim3(nb), dim3(256), 0, st, j);
}
uint32_t etlg_k_finish_job_bytes(void) { return (uint32_t)sizeof(FinJob); }

}  // extern "C"
