// ETLG_F_CHECK_CELLS, the single-pass half (include/etlg.h): k_chk_cells runs on the batch's decode stream directly
// behind the single-pass decode kernel and in front of the copy of the result block. It walks the DEFERRED json / jsonb / array cells of
// the arena that kernel just wrote and answers one question — does this batch hold a cell the reference's decode rejects
// (parse_cell_from_postgres_text, crates/etl/src/postgres/codec/text.rs:126-134, 163-312)? If so it puts a key into the batch's
// DevResult::first_err, and finish_batch (host_orchestrate.inc) decodes the batch again with the multi-pass kernels, whose k_write_chk
// (kernels.hip) raises the error at its frame in the reference's order and whose k_finalize cuts there. The key is a hint, never the
// answer: over-reporting costs a second attempt that comes back clean, under-reporting would lose an error — so every cell the
// multi-pass check would fail must fail here too (both call cell_text_error, cellparse.hip.h).
//
// No host stop: the event count is read from the result block on the device, the grid is sized from the frame count the host has (a
// frame emits at most one event). Thread u takes (row image, column) u / n_events of event u % n_events, as the finish pass arranges
// its cells (fin_thread_cell, finish.hip): the lanes of a wave hold ONE column of consecutive events — one class, one code path.
// One ballot and at most one atomic per wave. Integer / byte work, no MFMA.
#include "cellparse.hip.h"

namespace etlg {

__global__ __launch_bounds__(256) void k_chk_cells(DecParams p, uint32_t maxc, uint32_t ev_bound) {
  const DevResult* r = p.res;
  // (a first attempt that already failed is decoded again whatever this kernel finds; its arena may be incomplete)
  const bool usable = r->first_err == kNoErr && !r->fused_fail;
  const uint64_t ne = !usable ? 0ull : r->n_events < ev_bound ? r->n_events : ev_bound;
  const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = ne && u < ne * 2ull * maxc;   // (every lane reaches the ballot below)
  const uint64_t ev = live ? u % ne : 0;
  const uint32_t q = live ? (uint32_t)(u / ne) : 0u, img = q / maxc, col = q % maxc;
  uint32_t code = 0;
  do {
    if (!live) break;
    const uint32_t kind = p.ev_kind[ev];
    if (!(kind == 'I' || kind == 'U' || kind == 'D')) break;
    const uint32_t hs = p.ev_slot[ev];
    uint32_t lo = 0, hi = p.n_slots;   // the device table holds the live slots in ascending host id order
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (p.slots[mid].host_id < hs) lo = mid + 1; else hi = mid; }
    if (lo >= p.n_slots || p.slots[lo].host_id != hs) break;
    const DevSlot& s = p.slots[lo];
    if (col >= s.n_cols || s.cols_base + col >= p.n_cols) break;
    const DevCol dc = p.cols[s.cols_base + col];
    if (!class_always_deferred(dc.cls)) break;
    const uint32_t ok = kind == 'I' ? 0u : (uint32_t)p.ev_flags[ev] & 3u;
    uint64_t base = p.ev_body[ev];
    uint32_t pos = col, off = dc.off_full, row = s.row_full;
    if (img == 0) {   // the old image (Update / Delete): full or key layout
      if (ok == ETLG_OLD_NONE) break;
      if (ok == ETLG_OLD_KEY) { if (!dc.identity) break; pos = dc.key_index; off = dc.off_key; row = s.row_key; }
    } else {
      if (kind == 'D') break;
      base += ok == ETLG_OLD_KEY ? s.row_key : ok == ETLG_OLD_FULL ? s.row_full : 0u;
    }
    if (base + row > p.fixed_cap || off + 8u > row) break;
    const u8* rowp = p.fixed + base;
    if (get_state(rowp, pos) != ETLG_CELL_DEFERRED) break;   // NULL, MISSING, or settled already
    const uint32_t* slot = (const uint32_t*)(rowp + off);
    const uint64_t at = slot[0], n = slot[1];
    if (at + n > p.heap_cap) break;
    const uint32_t e = cell_text_error(dc.cls, chk_elem_table(p)[s.cols_base + col], p.heap + at, (uint32_t)n);
    if (e && e < ARR_HOST) code = e;
  } while (false);
  const unsigned long long m = __ballot(code != 0);
  if (m && (threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(m))
    atomicMin(&p.res->first_err, ((unsigned long long)ev << 16) | ((unsigned long long)RK_DECODE << 8) | code);
}

}  // namespace etlg

extern "C" void etlg_k_launch_chk_cells(const etlg::DecParams* p, uint32_t maxc, uint32_t ev_bound, hipStream_t s) {
  const uint64_t n = (uint64_t)ev_bound * 2ull * maxc;
  if (!n) return;
  hipLaunchKernelGGL(etlg::k_chk_cells, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, *p, maxc, ev_bound);
}
