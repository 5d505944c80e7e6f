// What the decode decides before it touches the device: the output capacities, the bound of a batch decoded behind its boundary scan, the
// geometry of the fixed-width plan's launch, the generic kernel choice, k_rows' tile choice, the staging window of k_fused / k_cells /
// k_copy_cells, the side set's layout and the plan's summary. Plain C++, no HIP and no context: tests/native/decode_plan_check.cpp includes
// this header alone and compares every figure with the expressions it replaced. The host (host_orchestrate.inc,
// host_decode.inc) passes in what it gets from the kernel launchers, as values or as a callable.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/etlg.h"
#include "dev_types.h"
#include "scratch_layout.h"

namespace decode_plan {
using namespace etlg;

constexpr uint64_t kLdsCu = 160 * 1024;       // LDS of a CU
constexpr uint64_t kLdsWindowMax = 150 * 1024;   // the most a workgroup asks for

// ---- setup_outputs: one event per frame; rows bounded by the widest slot; truncate bodies by 2x frame bytes; heap by 2.5x input
struct OutCaps { size_t evcap; uint64_t fixed_cap, heap_cap; };
inline OutCaps out_caps(uint32_t nf, uint64_t blen, uint32_t max_row_bytes) {
  return {(size_t)nf + 16, (uint64_t)nf * max_row_bytes + 2 * blen + 64, std::min<uint64_t>(0xFFFFFFF0ull, blen * 5 / 2 + 64)};
}

// ---- a batch decoded behind its boundary scan. The estimate: this batch's bytes at the bytes per frame of the last scanned batch of the
// stream; the bound its grids are sized by: a quarter above it, within what the offsets buffer holds
struct ScanBound { size_t offs_cap; uint64_t nf_est, bound; };
inline ScanBound scan_bound(size_t len, uint64_t last_nf, uint64_t last_len) {
  ScanBound o{};
  o.offs_cap = len / 24 + 1024;
  o.nf_est = last_len ? std::max<uint64_t>(1, (uint64_t)((unsigned __int128)len * last_nf / last_len)) : 0;
  o.bound = std::min<uint64_t>(o.offs_cap, o.nf_est + o.nf_est / 4 + 4096);
  return o;
}

inline uint64_t avg_frame(uint64_t len, uint64_t nf) { return (len + nf - 1) / nf; }

// ---- the fixed-width plan's launch (plan.hip). rows_off: the staging window (a tile read in place parks 64 x 32-byte bodies there); rows
// of up to 8 dwords wait for the look-back inside their own frame's staged head, wider tables get a region of 64 rows behind the window.
// per: descriptor pairs, {agg, lsn}[ntiles] | {agg, lsn}[ngroups] — the look-back's groups are 64 tiles, the pre-pass's are what plan.hip
// makes them (pre_group_log). dbytes: a look-back buffer. pbytes: a pre-pass buffer, ticket (a fixed place, whatever the batch's size: it
// must read zero) | {prefix inside the group}[ntiles] | {group prefix}[ngroups]
struct PlanGeom { uint32_t ntiles, rows_off, lds_bytes, max_row_dw; size_t per, dbytes, pbytes; };
inline PlanGeom plan_geom(uint32_t nf, uint64_t avg, uint32_t margin_pct, uint32_t plan_max_row, uint32_t pre_group_log) {
  PlanGeom g{};
  g.ntiles = (nf + 63) / 64;
  uint64_t cap = 64 * avg * (100 + (uint64_t)margin_pct) / 100 + 128;
  cap = std::min<uint64_t>((cap + 127) & ~127ull, 48 * 1024);
  g.rows_off = (uint32_t)std::max<uint64_t>(cap, 2048 + 64);
  g.lds_bytes = g.rows_off + (plan_max_row > 32 ? (uint32_t)(64ull * plan_max_row + 64) : 0u);
  g.max_row_dw = (plan_max_row + 3) / 4;
  const size_t gtiles = std::min<size_t>(64, (size_t)1 << pre_group_log);
  g.per = 2 * ((size_t)g.ntiles + ((size_t)g.ntiles + gtiles - 1) / gtiles);
  g.dbytes = g.per * 8 + 64;
  g.pbytes = (64 + g.per * 8 + 255) & ~(size_t)255;
  return g;
}
// The pre-pass buffers rotate: use number `useq` takes buffer useq mod nbufs; its tag differs from the tag of that buffer's last two uses,
// so a stale group word is never taken for this launch's
struct PreSlot { uint32_t slot, tag; };
inline PreSlot pre_slot(uint32_t useq, uint32_t nbufs) { return {useq % nbufs, 1u + (useq / nbufs) % 3u}; }

// ---- the generic single-pass kernels. The side tables ride in LDS when they fit 32 KiB (0: they do not, or ETLG_FUSED_DBG bit 4)
inline uint32_t side_lds_bytes(uint32_t n_tables, uint32_t n_epochs, uint32_t n_slots, uint32_t n_cols, bool off) {
  const uint64_t side = (uint64_t)n_tables * sizeof(DevTable) + (uint64_t)n_epochs * sizeof(DevEpoch) + (uint64_t)n_slots * sizeof(DevSlot) + (uint64_t)n_cols * sizeof(DevCol);
  return (side <= 32768 && !off) ? (uint32_t)((side + 15) & ~15ull) : 0u;
}
// 0 k_fused / 256 frames per tile, one lane per frame (narrow frames); 1 k_fused / 64; 2 k_cells, 64 frames per tile with the waves spread
// over the columns (wide frames; any_var: a table the batch may carry has TEXT / NUMERIC / ... columns, one lane per frame crawls on those)
inline int generic_kernel(uint64_t avg, bool any_var, bool cells_ok, int forced, bool direct) {
  int kernel = (avg <= 192 && !(any_var && cells_ok && avg > 96)) ? 0 : (cells_ok ? 2 : 1);
  if (forced >= 0 && forced <= 2) kernel = forced == 2 && !cells_ok ? 1 : forced;
  return direct ? 2 : kernel;
}

// ---- k_rows: frames per tile x tiles per CU, the pair that keeps the most FRAMES in flight on a CU (a tile is a chain of latencies: what a
// CU delivers is frames in flight / a tile's time) — 64 frames at four tiles when that fits; 56 or 48 frames when eight fewer lanes buy a
// fourth tile; 16-frame tiles for 1.5 KB frames. The window then takes what its share of the LDS leaves. LDS is handed out in granules: a
// workgroup's static + dynamic bytes are rounded up, so the budget per workgroup is rounded DOWN. cf_forced: ETLG_ROWS_CF, 8 .. 64, a
// multiple of 8. max_wgs: what the register file allows. table_bytes(maxh_old, maxh, widest, cf): the kernel's tables for a tile of cf
struct RowsIn { uint64_t avg; uint32_t maxrow, maxh, maxh_old, widest, side_bytes; uint64_t stat, rows_win_min; uint32_t cf_forced; uint64_t max_wgs; };
struct RowsChoice { bool taken; uint32_t cf; uint64_t need, tabb, wgs; uint32_t lds_bytes; };
inline uint64_t rows_budget(uint64_t wgs) { return (kLdsCu / wgs / 1280) * 1280; }
template <class TableBytes>
RowsChoice rows_choice(const RowsIn& in, TableBytes table_bytes) {
  auto need_of = [&](uint32_t f, uint64_t& tb) {
    tb = table_bytes(in.maxh_old, in.maxh, in.widest, f);
    return in.stat + in.side_bytes + tb + std::max<uint64_t>((uint64_t)f * in.avg * 9 / 8 + 1024, in.rows_win_min * f / 64 + 64);
  };
  auto wgs_of = [&](uint64_t nd) { uint64_t w = 0; for (uint64_t k = 1; k <= in.max_wgs; k++) if (nd <= rows_budget(k)) w = k; return w; };
  RowsChoice o{};
  o.cf = 64;
  const uint32_t cf_forced = in.cf_forced;
  uint64_t best = 0;
  for (uint32_t f = 64; f >= 16; f -= 8) {
    if (cf_forced >= 8 && cf_forced <= 64 && !(cf_forced & 7u) && f != cf_forced && cf_forced >= 16) continue;
    uint64_t tb;
    const uint64_t nd = need_of(f, tb);
    if ((uint64_t)f * in.maxrow > 0x3FFFFull || nd > kLdsWindowMax) continue;
    const uint64_t w = wgs_of(nd);
    const uint64_t score = (uint64_t)f * w / (w == 1 ? 2 : 1);   // (one tile per CU is four waves on 256 lanes of SIMD: last resort)
    if (score >= best && score) { best = score; o.cf = f; }      // (a tie goes to the smaller tile: more waves per CU)
  }
  if (cf_forced >= 8 && cf_forced < 16 && !(cf_forced & 7u)) o.cf = cf_forced;
  o.need = need_of(o.cf, o.tabb);
  o.taken = !(o.need > kLdsWindowMax || (uint64_t)o.cf * in.maxrow > 0x3FFFFull);   // (a tile's piece of the fixed arena is addressed by 16-bit dword offsets)
  if (!o.taken) return o;
  o.wgs = std::max<uint64_t>(1, wgs_of(o.need));
  o.lds_bytes = (uint32_t)std::min<uint64_t>((rows_budget(o.wgs) - in.stat) & ~15ull, kLdsWindowMax);
  return o;
}

// ---- the LDS window per tile of k_fused / k_cells / k_copy_cells: the average tile plus a margin (margin_pct: ETLG_LDS_MARGIN_PCT, < 0
// not set); a tile that does not fit reads the input in place. k_cells: its tables beside the window, at least its floor; the rows -> arena
// kernel sizes its own (copy_lds(window)). LDS decides how many workgroups share a CU (the register file allows four): the window takes
// whatever the allocation can grow by without losing one, so fewer tiles overflow it. stat: the kernel's static LDS
template <class CopyLds>
uint32_t generic_window(int kernel, uint64_t avg, int margin_pct, bool direct, uint32_t side_bytes, uint64_t cells_tables, uint64_t cells_floor, uint64_t stat, CopyLds copy_lds) {
  const uint64_t blk = kernel == 0 ? 256u : 64u;
  uint64_t cap = kernel == 1 ? blk * avg * 5 / 4 + 2048 : blk * avg * 9 / 8 + 1024;
  if (margin_pct >= 0) cap = blk * avg * (100 + (uint64_t)margin_pct) / 100 + 1024;
  cap = (cap + 255) & ~255ull;
  if (kernel == 2) {
    cap = direct ? copy_lds((uint32_t)cap) : std::max<uint64_t>(cap + cells_tables, cells_floor);
    const uint64_t wgs = std::max<uint64_t>(1, std::min<uint64_t>(4, kLdsCu / (cap + side_bytes + stat)));
    cap = std::max<uint64_t>(cap, (kLdsCu / wgs - 512 - stat - side_bytes) & ~255ull);
  }
  return (uint32_t)std::min<uint64_t>(cap + side_bytes, kLdsWindowMax);
}

// ---- one uploaded copy of the side inputs: tables | epochs | slots | columns, one element-class byte per column behind the records | plan
// tables | plan column words, 16 bytes of slack behind every part
struct SideLayout { size_t tables, epochs, slots, cols, elems, ptabs, pcols, total; };
inline SideLayout side_layout(size_t n_tables, size_t n_epochs, size_t n_slots, size_t n_cols, size_t n_ptabs, size_t n_pcols) {
  ScratchLayout l; SideLayout o{};
  o.tables = l.take(n_tables * sizeof(DevTable) + 16); o.epochs = l.take(n_epochs * sizeof(DevEpoch) + 16); o.slots = l.take(n_slots * sizeof(DevSlot) + 16);
  o.cols = l.take(n_cols * (sizeof(DevCol) + 1) + 16); o.elems = o.cols + n_cols * sizeof(DevCol);
  o.ptabs = l.take(n_ptabs * sizeof(PlanTab) + 16); o.pcols = l.take(n_pcols * 4 + 16);
  o.total = l.total();
  return o;
}

// ---- what the host keeps of the plan tables it uploaded. max_row: bytes of the widest planned row (at least 16). uniform_dw /
// uniform_key_dw: the row / key-row dwords shared by every planned table, 0 when they differ — the sidecar pre-pass prices a row without
// knowing its table, and a Delete by key by its length too: shorter than any row frame of any planned table (key_below), no longer than the
// longest key in canonical form (key_max). covers_all: every table state the batch can meet is covered by the plan — a table that is not
// eligible but owned (a TEXT column, say) would fail every batch that carries its rows
struct PlanSummary { uint32_t n_tabs, max_row, uniform_dw, uniform_key_dw, key_below, key_max; bool covers_all; };
inline PlanSummary plan_summary(const std::vector<PlanTab>& pt, const std::vector<uint32_t>& pc, const std::vector<DevTable>& tv) {
  PlanSummary o{};
  o.n_tabs = (uint32_t)pt.size();
  o.max_row = 16;
  for (auto& e : pt) o.max_row = std::max<uint32_t>(o.max_row, e.row_dwords * 4);
  o.uniform_dw = pt.empty() ? 0u : pt[0].row_dwords;
  for (auto& e : pt) if (e.row_dwords != o.uniform_dw) o.uniform_dw = 0;
  o.uniform_key_dw = pt.empty() ? 0u : pt[0].key_dwords;
  o.key_below = ~0u; o.key_max = 0;
  for (auto& e : pt) {
    if (e.key_dwords != o.uniform_key_dw) o.uniform_key_dw = 0;
    uint32_t shortest = 38;   // CopyData + XLogData head, tag, relation id, 'N', column count
    for (uint32_t k = 0; k < e.n_cols; k++) shortest += ((pc[e.cols_base + k] >> 8) & 1u) ? 1u : 6u;   // 'n', or 't' len:4 and one character
    o.key_below = std::min(o.key_below, shortest);
    uint32_t longest = 38;
    for (uint32_t k = 0; k < e.n_cols; k++) {
      const uint32_t cls = pc[e.cols_base + k] & 0xFFu;
      longest += (pc[e.keys_base + k] & 1u) ? 5u + (cls == ETLG_TC_BOOL ? 1u : cls == ETLG_TC_I16 ? 6u : cls == ETLG_TC_I32 ? 11u : cls == ETLG_TC_U32 ? 10u : 20u) : 1u;
    }
    o.key_max = std::max(o.key_max, longest);
  }
  if (!o.uniform_key_dw || pt.empty()) { o.key_below = 0; o.key_max = 0; }
  o.covers_all = !pt.empty();
  for (const DevTable& t : tv) if (t.state_kind != ETLG_TS_ABSENT && t.state_kind != ETLG_TS_OTHER) {
    bool found = false;
    for (auto& e : pt) if (e.rel_id == t.table_id) found = true;
    if (!found) o.covers_all = false;
  }
  return o;
}

}  // namespace decode_plan
