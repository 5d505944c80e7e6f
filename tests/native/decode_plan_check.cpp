// Stand-alone check of etl_amd/csrc/decode_plan.h (tests/test_decode_plan.py builds it with the address and undefined-behaviour sanitizers;
// the header is included alone). Every figure the header hands to the decode's host layer against the expression it replaced: the old_*
// functions below are the bodies of enqueue_single, build_side_inputs, setup_outputs and etlg_decode as they stood before the cut, with
// their locals as parameters — nothing expected is obtained from the header. The grid crosses every threshold those expressions have. The
// side set's parts are also checked on their own: at multiples of 64, disjoint, inside the total.
#include "decode_plan.h"

#include <cstdio>

using namespace etlg;

static int bad = 0;
static unsigned long long cases = 0;
#define CHECK(cond) do { if (!(cond)) { bad++; std::printf("FAILED line %d: %s\n", __LINE__, #cond); } } while (0)
#define CHECK_EQ(a, b) do { const unsigned long long a_ = (unsigned long long)(a), b_ = (unsigned long long)(b); cases++; \
    if (a_ != b_) { if (bad++ < 40) std::printf("FAILED line %d: %s = %llu, expected %llu\n", __LINE__, #a, a_, b_); } } while (0)

// what the kernel launchers answer, as this program plays them (any function of the arguments does: both sides get the same one)
static uint32_t table_bytes(uint32_t maxh_old, uint32_t maxh, uint32_t widest, uint32_t f) { return f * (maxh + maxh_old) * 8 + widest * 16 + 256; }
static uint32_t cells_table_bytes(uint32_t maxc) { return maxc * 96 + 128; }
static uint32_t cells_lds_floor(uint32_t maxc) { return maxc * 1024 + 4096; }
static uint32_t cells_static_lds(uint32_t maxc) { return maxc > 16 ? 6144 : 3072; }
static uint32_t copy_cells_static_lds(uint32_t maxc) { return maxc > 16 ? 7168 : 3584; }
static uint32_t copy_cells_lds(uint32_t maxc, uint32_t window) { return window + maxc * 160 + 512; }

// ---- the plan launch (enqueue_single, level 0)
struct OldPlan { uint32_t ntiles, rows_off, lds_bytes, max_row_dw; size_t per, dbytes, pbytes; };
static OldPlan old_plan(uint32_t nf, uint64_t avg, uint32_t plan_margin_pct, uint32_t plan_max_row, uint32_t group_log) {
  OldPlan q{};
  q.ntiles = (nf + 63) / 64;
  uint64_t cap = 64 * avg * (100 + (uint64_t)plan_margin_pct) / 100 + 128;
  cap = std::min<uint64_t>((cap + 127) & ~127ull, 48 * 1024);
  q.rows_off = (uint32_t)std::max<uint64_t>(cap, 2048 + 64);
  q.lds_bytes = q.rows_off + (plan_max_row > 32 ? (uint32_t)(64ull * plan_max_row + 64) : 0u);
  q.max_row_dw = (plan_max_row + 3) / 4;
  const size_t gtiles = std::min<size_t>(64, (size_t)1 << group_log);
  const size_t per = 2 * ((size_t)q.ntiles + ((size_t)q.ntiles + gtiles - 1) / gtiles);
  q.per = per;
  q.dbytes = per * 8 + 64;
  q.pbytes = (64 + per * 8 + 255) & ~(size_t)255;
  return q;
}
static void check_plan() {
  const uint64_t avgs[] = {1, 96, 97, 192, 193, 730, 740, 800, 5000};   // 740 x 64 x 1.04 reaches the 48 KiB clamp
  const uint32_t nfs[] = {1, 63, 64, 65, 4096, 4097, (1u << 29) - 3};
  bool clamped = false, floored = false;
  for (uint64_t avg : avgs) for (uint32_t nf : nfs) for (uint32_t row : {32u, 33u, 512u}) for (uint32_t margin : {0u, 4u}) for (uint32_t glog : {4u, 6u, 8u}) {
    const OldPlan o = old_plan(nf, avg, margin, row, glog);
    const decode_plan::PlanGeom g = decode_plan::plan_geom(nf, avg, margin, row, glog);
    CHECK_EQ(g.ntiles, o.ntiles); CHECK_EQ(g.rows_off, o.rows_off); CHECK_EQ(g.lds_bytes, o.lds_bytes); CHECK_EQ(g.max_row_dw, o.max_row_dw);
    CHECK_EQ(g.per, o.per); CHECK_EQ(g.dbytes, o.dbytes); CHECK_EQ(g.pbytes, o.pbytes);
    clamped |= o.rows_off == 48 * 1024; floored |= o.rows_off == 2048 + 64;
  }
  CHECK(clamped); CHECK(floored);
  for (uint32_t useq = 0; useq < 14; useq++) {   // more than a lap of the four buffers, and of the three tags
    const uint32_t NB = 4;
    const uint32_t slot = useq % NB, tag = 1u + (useq / NB) % 3u;
    const decode_plan::PreSlot ps = decode_plan::pre_slot(useq, NB);
    CHECK_EQ(ps.slot, slot); CHECK_EQ(ps.tag, tag);
    if (useq >= NB) CHECK(ps.tag != decode_plan::pre_slot(useq - NB, NB).tag);
    if (useq >= 2 * NB) CHECK(ps.tag != decode_plan::pre_slot(useq - 2 * NB, NB).tag);
  }
}

// ---- side_bytes and the generic kernel choice
static uint32_t old_side_bytes(uint32_t n_tables, uint32_t n_epochs, uint32_t n_slots, uint32_t n_cols, uint32_t fused_dbg) {
  const uint64_t side = (uint64_t)n_tables * sizeof(DevTable) + (uint64_t)n_epochs * sizeof(DevEpoch) +
                        (uint64_t)n_slots * sizeof(DevSlot) + (uint64_t)n_cols * sizeof(DevCol);
  return (side <= 32768 && !(fused_dbg & 16)) ? (uint32_t)((side + 15) & ~15ull) : 0u;
}
static int old_kernel(uint64_t avg, bool any_var, bool cells_ok, int fused_kernel, bool direct) {
  int kernel = (avg <= 192 && !(any_var && cells_ok && avg > 96)) ? 0 : (cells_ok ? 2 : 1);  // 0 fused/256, 1 fused/64, 2 cells
  if (fused_kernel >= 0 && fused_kernel <= 2) kernel = fused_kernel == 2 && !cells_ok ? 1 : fused_kernel;
  if (direct) kernel = 2;
  return kernel;
}
static void check_choice() {
  for (uint32_t nt : {0u, 1u, 40u, 2000u}) for (uint32_t ne : {0u, 1u, 300u}) for (uint32_t ns : {0u, 1u, 64u}) for (uint32_t nc : {0u, 1u, 900u, 5000u}) for (uint32_t dbg : {0u, 16u, 8u})
    CHECK_EQ(decode_plan::side_lds_bytes(nt, ne, ns, nc, (dbg & 16) != 0), old_side_bytes(nt, ne, ns, nc, dbg));
  {  // the edge of the 32 KiB: one table more than fits
    const uint32_t fit = 32768 / sizeof(DevTable);
    CHECK(decode_plan::side_lds_bytes(fit, 0, 0, 0, false) != 0); CHECK_EQ(decode_plan::side_lds_bytes(fit + 1, 0, 0, 0, false), old_side_bytes(fit + 1, 0, 0, 0, 0));
  }
  for (uint64_t avg : {1ull, 96ull, 97ull, 192ull, 193ull, 5000ull}) for (int any_var = 0; any_var < 2; any_var++) for (int cells_ok = 0; cells_ok < 2; cells_ok++)
    for (int forced : {-1, 0, 1, 2, 3, 4}) for (int direct = 0; direct < 2; direct++)
      CHECK_EQ(decode_plan::generic_kernel(avg, any_var, cells_ok, forced, direct), old_kernel(avg, any_var, cells_ok, forced, direct));
}

// ---- k_rows' tile choice
struct OldRows { bool ok; uint32_t cf; uint64_t need, tabb, wgs; uint32_t lds_bytes; };
static OldRows old_rows(uint64_t avg, uint32_t maxrow, uint32_t maxh, uint32_t maxh_old, uint32_t widest, uint32_t side_bytes, uint64_t stat, uint64_t rows_win_min,
                        uint32_t rows_cf, uint64_t max_wgs) {
  OldRows r{};
  bool ok = true;
  auto budget = [](uint64_t wgs) { return ((160 * 1024) / wgs / 1280) * 1280; };
  uint32_t cf = 64;
  uint64_t need = 0, tabb = 0;
  const uint32_t cf_forced = rows_cf;   // (ETLG_ROWS_CF, experiments / tests: 8 .. 64, a multiple of 8)
  auto need_of = [&](uint32_t f, uint64_t& tb) {
    tb = table_bytes(maxh_old, maxh, widest, f);
    return stat + side_bytes + tb + std::max<uint64_t>((uint64_t)f * avg * 9 / 8 + 1024, rows_win_min * f / 64 + 64);
  };
  auto wgs_of = [&](uint64_t nd) { uint64_t w = 0; for (uint64_t k = 1; k <= max_wgs; k++) if (nd <= budget(k)) w = k; return w; };
  {
    uint64_t best = 0;
    for (uint32_t f = 64; f >= 16; f -= 8) {
      if (cf_forced >= 8 && cf_forced <= 64 && !(cf_forced & 7u) && f != cf_forced && cf_forced >= 16) continue;
      uint64_t tb;
      const uint64_t nd = need_of(f, tb);
      if ((uint64_t)f * maxrow > 0x3FFFFull || nd > 150 * 1024) continue;
      const uint64_t w = wgs_of(nd);
      const uint64_t score = (uint64_t)f * w / (w == 1 ? 2 : 1);   // (one tile per CU is four waves on 256 lanes of SIMD: last resort)
      if (score >= best && score) { best = score; cf = f; }        // (a tie goes to the smaller tile: more waves per CU)
    }
    if (cf_forced >= 8 && cf_forced < 16 && !(cf_forced & 7u)) cf = cf_forced;
    need = need_of(cf, tabb);
  }
  r.cf = cf; r.need = need; r.tabb = tabb;
  if (need > 150 * 1024 || (uint64_t)cf * maxrow > 0x3FFFFull) ok = false;   // (a tile's piece of the fixed arena is addressed by 16-bit dword offsets)
  else {
    const uint64_t wgs = std::max<uint64_t>(1, wgs_of(need));
    const uint64_t tot = (budget(wgs) - stat) & ~15ull;
    r.lds_bytes = (uint32_t)std::min<uint64_t>(tot, 150 * 1024);
    r.wgs = wgs;
  }
  r.ok = ok;
  return r;
}
static void check_rows() {
  const uint64_t avgs[] = {1, 96, 97, 192, 193, 500, 1500, 3000, 20000};   // 20000: every tile size needs more than 150 KiB
  const uint32_t maxrows[] = {16, 4095, 4096, 4097, 5461, 5462, 16383, 16384, 70000};   // cf x maxrow crosses 0x3FFFF at 64, 48 and 16 frames
  unsigned taken = 0, refused_need = 0, refused_row = 0, cfs_seen = 0;
  for (uint64_t avg : avgs) for (uint32_t maxrow : maxrows) for (uint32_t cf_forced : {0u, 7u, 8u, 16u, 24u, 64u}) for (uint64_t win_min : {0ull, 90000ull, 400000ull})
    for (uint32_t side : {0u, 32768u}) for (uint32_t maxh : {1u, 12u}) for (uint32_t widest : {1u, 64u}) for (uint64_t max_wgs : {2ull, 4ull, 8ull}) {
      const uint32_t maxh_old = maxh / 3;
      const uint64_t stat = 2048;
      const OldRows o = old_rows(avg, maxrow, maxh, maxh_old, widest, side, stat, win_min, cf_forced, max_wgs);
      const decode_plan::RowsChoice r = decode_plan::rows_choice(decode_plan::RowsIn{avg, maxrow, maxh, maxh_old, widest, side, stat, win_min, cf_forced, max_wgs}, table_bytes);
      CHECK_EQ(r.taken, o.ok); CHECK_EQ(r.cf, o.cf); CHECK_EQ(r.need, o.need); CHECK_EQ(r.tabb, o.tabb);
      if (o.ok) { CHECK_EQ(r.wgs, o.wgs); CHECK_EQ(r.lds_bytes, o.lds_bytes); taken++; cfs_seen |= 1u << (o.cf / 8); }
      else if (o.need > 150 * 1024) refused_need++;
      else refused_row++;
    }
  CHECK(taken > 100); CHECK(refused_need > 0); CHECK(refused_row > 0);
  CHECK((cfs_seen & (1u << 8)) && (cfs_seen & (1u << 2)) && (cfs_seen & (1u << 1)));   // 64-frame, 16-frame and the forced 8-frame tiles all occur
}

// ---- the k_fused / k_cells / k_copy_cells window
static uint32_t old_window(int kernel, uint64_t avg, int lds_margin_pct, bool direct, uint32_t widest, uint32_t side_bytes) {
  const bool use_cells = kernel == 2;
  const uint32_t blk = kernel == 0 ? 256u : 64u;
  uint64_t cap = kernel == 1 ? (uint64_t)blk * avg * 5 / 4 + 2048 : (uint64_t)blk * avg * 9 / 8 + 1024;
  if (lds_margin_pct >= 0) cap = (uint64_t)blk * avg * (100 + (uint64_t)lds_margin_pct) / 100 + 1024;   // (ETLG_LDS_MARGIN_PCT)
  cap = (cap + 255) & ~255ull;
  if (use_cells) {
    cap = direct ? copy_cells_lds(widest, (uint32_t)cap) : std::max<uint64_t>(cap + cells_table_bytes(widest), cells_lds_floor(widest));
    const uint64_t stat = direct ? copy_cells_static_lds(widest) : cells_static_lds(widest);
    const uint64_t wgs = std::max<uint64_t>(1, std::min<uint64_t>(4, (160 * 1024) / (cap + side_bytes + stat)));
    cap = std::max<uint64_t>(cap, ((160 * 1024) / wgs - 512 - stat - side_bytes) & ~255ull);
  }
  cap = std::min<uint64_t>(cap + side_bytes, 150 * 1024);
  return (uint32_t)cap;
}
static void check_window() {
  bool clamped = false, grown = false;
  for (int kernel : {0, 1, 2}) for (uint64_t avg : {1ull, 96ull, 97ull, 192ull, 193ull, 400ull, 600ull, 1800ull, 3000ull}) for (int margin : {-1, 0, 25}) for (int direct = 0; direct < 2; direct++)
    for (uint32_t widest : {1u, 16u, 17u, 32u}) for (uint32_t side : {0u, 4096u, 32768u}) {
      if (direct && kernel != 2) continue;   // (table-copy rows decoded in place always take the rows -> arena kernel)
      const bool cells = kernel == 2;
      const uint64_t stat = !cells ? 0 : direct ? copy_cells_static_lds(widest) : cells_static_lds(widest);
      const uint32_t got = decode_plan::generic_window(kernel, avg, margin, direct, side, cells && !direct ? cells_table_bytes(widest) : 0, cells && !direct ? cells_lds_floor(widest) : 0, stat,
                                                       [&](uint32_t window) { return copy_cells_lds(widest, window); });
      const uint32_t want = old_window(kernel, avg, margin, direct, widest, side);
      CHECK_EQ(got, want);
      clamped |= want == 150 * 1024;
      grown |= cells && want < 150 * 1024 && want > ((256 * avg * 9 / 8 + 1024 + 255) & ~255ull) + side + 40000;
    }
  CHECK(clamped); CHECK(grown);
}

// ---- the side set's layout
struct Part { size_t at, len; };
static void check_parts(const std::vector<Part>& parts, size_t total) {
  for (size_t i = 0; i < parts.size(); i++) {
    CHECK(parts[i].at % 64 == 0);
    CHECK(parts[i].at + parts[i].len <= total);
    for (size_t k = i + 1; k < parts.size(); k++) CHECK(parts[i].at + parts[i].len <= parts[k].at || parts[k].at + parts[k].len <= parts[i].at);
  }
}
static void check_side_layout() {
  const size_t counts[] = {0, 1, 7, 1000};
  for (size_t nt : counts) for (size_t ne : counts) for (size_t ns : counts) for (size_t nc : counts) for (size_t npt : counts) for (size_t npc : counts) {
    // the chain build_side_inputs added by hand
    const size_t o_tables = 0;
    const size_t o_epochs = al64(nt * sizeof(DevTable) + 16);
    const size_t o_slots = o_epochs + al64(ne * sizeof(DevEpoch) + 16);
    const size_t o_cols = o_slots + al64(ns * sizeof(DevSlot) + 16);
    const size_t o_ptabs = o_cols + al64(nc * (sizeof(DevCol) + 1) + 16);   // (the records, then one element-class byte per record)
    const size_t o_pcols = o_ptabs + al64(npt * sizeof(PlanTab) + 16);
    const size_t total = o_pcols + al64(npc * 4 + 16);
    const decode_plan::SideLayout l = decode_plan::side_layout(nt, ne, ns, nc, npt, npc);
    CHECK_EQ(l.tables, o_tables); CHECK_EQ(l.epochs, o_epochs); CHECK_EQ(l.slots, o_slots); CHECK_EQ(l.cols, o_cols); CHECK_EQ(l.elems, o_cols + nc * sizeof(DevCol));
    CHECK_EQ(l.ptabs, o_ptabs); CHECK_EQ(l.pcols, o_pcols); CHECK_EQ(l.total, total);
    check_parts({{l.tables, nt * sizeof(DevTable)}, {l.epochs, ne * sizeof(DevEpoch)}, {l.slots, ns * sizeof(DevSlot)}, {l.cols, nc * (sizeof(DevCol) + 1)},
                 {l.ptabs, npt * sizeof(PlanTab)}, {l.pcols, npc * 4}}, l.total);
    CHECK(l.elems + nc <= l.ptabs);   // the element-class bytes sit behind the column records, in front of the next part
  }
}

// ---- the plan's summary over the built tables
struct OldSummary { uint32_t n_plan_tabs, plan_max_row, plan_uniform_dw, plan_uniform_key_dw, plan_key_below, plan_key_max; bool plan_covers_all; };
static OldSummary old_summary(const std::vector<PlanTab>& pt, const std::vector<uint32_t>& pc, const std::vector<DevTable>& tv) {
  OldSummary c_{}; OldSummary* c = &c_;
  c->n_plan_tabs = (uint32_t)pt.size();
  c->plan_max_row = 16;
  for (auto& e : pt) c->plan_max_row = std::max<uint32_t>(c->plan_max_row, e.row_dwords * 4);
  c->plan_uniform_dw = pt.empty() ? 0u : pt[0].row_dwords;   // the sidecar pre-pass prices a row without knowing its table
  for (auto& e : pt) if (e.row_dwords != c->plan_uniform_dw) c->plan_uniform_dw = 0;
  c->plan_uniform_key_dw = pt.empty() ? 0u : pt[0].key_dwords;
  c->plan_key_below = ~0u; c->plan_key_max = 0;
  for (auto& e : pt) {
    if (e.key_dwords != c->plan_uniform_key_dw) c->plan_uniform_key_dw = 0;
    uint32_t shortest = 38;   // CopyData + XLogData head, tag, relation id, 'N', column count
    for (uint32_t k = 0; k < e.n_cols; k++) shortest += ((pc[e.cols_base + k] >> 8) & 1u) ? 1u : 6u;   // 'n', or 't' len:4 and one character
    c->plan_key_below = std::min(c->plan_key_below, shortest);
    uint32_t longest = 38;
    for (uint32_t k = 0; k < e.n_cols; k++) {
      const uint32_t cls = pc[e.cols_base + k] & 0xFFu;
      longest += (pc[e.keys_base + k] & 1u) ? 5u + (cls == ETLG_TC_BOOL ? 1u : cls == ETLG_TC_I16 ? 6u : cls == ETLG_TC_I32 ? 11u : cls == ETLG_TC_U32 ? 10u : 20u) : 1u;
    }
    c->plan_key_max = std::max(c->plan_key_max, longest);
  }
  if (!c->plan_uniform_key_dw || pt.empty()) { c->plan_key_below = 0; c->plan_key_max = 0; }
  c->plan_covers_all = !pt.empty();
  for (const DevTable& t : tv) if (t.state_kind != ETLG_TS_ABSENT && t.state_kind != ETLG_TS_OTHER) {
    bool found = false;
    for (auto& e : pt) if (e.rel_id == t.table_id) found = true;
    if (!found) c->plan_covers_all = false;
  }
  return c_;
}
// a planned table of `classes` (bit 8 of a class: nullable, bit 9: identity) appended to pt / pc the way build_side_inputs does
static void add_table(std::vector<PlanTab>& pt, std::vector<uint32_t>& pc, uint32_t rel_id, uint32_t row_dwords, uint32_t key_dwords, const std::vector<uint32_t>& classes) {
  PlanTab e{};
  e.rel_id = rel_id; e.slot = rel_id & 7; e.n_cols = (uint32_t)classes.size(); e.row_dwords = row_dwords; e.key_dwords = key_dwords;
  e.cols_base = (uint32_t)pc.size();
  for (size_t k = 0; k < classes.size(); k++) pc.push_back((classes[k] & 0xFFu) | (((classes[k] >> 8) & 1u) << 8) | ((uint32_t)(8 + 8 * k) << 16));
  e.keys_base = (uint32_t)pc.size();
  uint32_t ki = 0;
  for (size_t k = 0; k < classes.size(); k++) { const bool id = (classes[k] >> 9) & 1u; pc.push_back(id ? (1u | (ki << 8) | ((uint32_t)(1 + 2 * ki) << 24)) : 0u); ki += id; e.n_ident += id; }
  pt.push_back(e);
}
static void check_summary() {
  const uint32_t N = 1u << 8, ID = 1u << 9;
  const std::vector<uint32_t> five_int4 = {ETLG_TC_I32 | ID, ETLG_TC_I32, ETLG_TC_I32 | N, ETLG_TC_I32, ETLG_TC_I32 | N};
  const std::vector<uint32_t> mixed = {ETLG_TC_I64 | ID, ETLG_TC_BOOL | ID, ETLG_TC_I16 | N, ETLG_TC_U32, ETLG_TC_I64 | N, ETLG_TC_BOOL};
  auto table = [](uint32_t id, uint32_t state) { DevTable t{}; t.table_id = id; t.state_kind = state; return t; };
  struct Case { const char* what; std::vector<PlanTab> pt; std::vector<uint32_t> pc; std::vector<DevTable> tv; };
  std::vector<Case> cases_;
  cases_.push_back({"none", {}, {}, {}});
  cases_.push_back({"none, one table owned", {}, {}, {table(5, ETLG_TS_READY)}});
  { Case k{"one", {}, {}, {table(5, ETLG_TS_READY)}}; add_table(k.pt, k.pc, 5, 8, 2, five_int4); cases_.push_back(k); }
  { Case k{"one without a key", {}, {}, {table(5, ETLG_TS_READY)}}; add_table(k.pt, k.pc, 5, 8, 0, {ETLG_TC_I32, ETLG_TC_I32 | N}); cases_.push_back(k); }
  { Case k{"two equal", {}, {}, {table(5, ETLG_TS_READY), table(6, ETLG_TS_READY), table(9, ETLG_TS_ABSENT), table(10, ETLG_TS_OTHER)}};
    add_table(k.pt, k.pc, 5, 8, 2, five_int4); add_table(k.pt, k.pc, 6, 8, 2, mixed); cases_.push_back(k); }
  { Case k{"two, row_dwords differ", {}, {}, {table(5, ETLG_TS_READY), table(6, ETLG_TS_READY)}};
    add_table(k.pt, k.pc, 5, 8, 2, five_int4); add_table(k.pt, k.pc, 6, 130, 2, mixed); cases_.push_back(k); }
  { Case k{"two, key_dwords differ", {}, {}, {table(5, ETLG_TS_READY), table(6, ETLG_TS_READY)}};
    add_table(k.pt, k.pc, 5, 8, 2, five_int4); add_table(k.pt, k.pc, 6, 8, 4, mixed); cases_.push_back(k); }
  { Case k{"two, a third table owned and not planned", {}, {}, {table(5, ETLG_TS_READY), table(6, ETLG_TS_READY), table(7, ETLG_TS_SYNC_DONE)}};
    add_table(k.pt, k.pc, 5, 8, 2, five_int4); add_table(k.pt, k.pc, 6, 8, 2, mixed); cases_.push_back(k); }
  unsigned covered = 0, uniform = 0, keyed = 0;
  for (const Case& k : cases_) {
    const OldSummary o = old_summary(k.pt, k.pc, k.tv);
    const decode_plan::PlanSummary s = decode_plan::plan_summary(k.pt, k.pc, k.tv);
    CHECK_EQ(s.n_tabs, o.n_plan_tabs); CHECK_EQ(s.max_row, o.plan_max_row); CHECK_EQ(s.uniform_dw, o.plan_uniform_dw); CHECK_EQ(s.uniform_key_dw, o.plan_uniform_key_dw);
    CHECK_EQ(s.key_below, o.plan_key_below); CHECK_EQ(s.key_max, o.plan_key_max); CHECK_EQ(s.covers_all, o.plan_covers_all);
    covered += o.plan_covers_all; uniform += o.plan_uniform_dw != 0; keyed += o.plan_key_max != 0;
  }
  CHECK(covered >= 4 && covered < cases_.size()); CHECK(uniform >= 4 && uniform < cases_.size()); CHECK(keyed >= 2 && keyed < cases_.size());
}

// ---- the chained scan's estimate and bound, the output capacities
static void check_scan_and_outputs() {
  const size_t lens[] = {0, 1, 23, 24, 4096, 64u << 20, (size_t)1 << 31, 0xFFFFFFEFull};
  const uint64_t last_nfs[] = {0, 1, 1000, 1u << 20, (1u << 30) - 1};
  const uint64_t last_lens[] = {0, 1, 24000, 64u << 20, 0xFFFFFFEFull};
  for (size_t len : lens) for (uint64_t scan_last_nf : last_nfs) for (uint64_t scan_last_len : last_lens) {
    const size_t offs_cap = len / 24 + 1024;
    const uint64_t nf_est = scan_last_len ? std::max<uint64_t>(1, (uint64_t)((unsigned __int128)len * scan_last_nf / scan_last_len)) : 0;
    const uint64_t bound = std::min<uint64_t>(offs_cap, nf_est + nf_est / 4 + 4096);
    const decode_plan::ScanBound sb = decode_plan::scan_bound(len, scan_last_nf, scan_last_len);
    CHECK_EQ(sb.offs_cap, offs_cap); CHECK_EQ(sb.nf_est, nf_est); CHECK_EQ(sb.bound, bound);
  }
  for (uint32_t nf : {0u, 1u, 63u, 64u, 65u, (1u << 29) - 3, (1u << 30) - 1}) for (uint64_t blen : {0ull, 1ull, 4096ull, 1ull << 31, 0xFFFFFFEFull, 3ull << 32}) for (uint32_t max_row : {16u, 1040u, 131072u}) {
    const size_t evcap = (size_t)nf + 16;
    const uint64_t fixed_cap = (uint64_t)nf * max_row + 2 * blen + 64;
    const uint64_t heap_cap = std::min<uint64_t>(0xFFFFFFF0ull, blen * 5 / 2 + 64);
    const decode_plan::OutCaps oc = decode_plan::out_caps(nf, blen, max_row);
    CHECK_EQ(oc.evcap, evcap); CHECK_EQ(oc.fixed_cap, fixed_cap); CHECK_EQ(oc.heap_cap, heap_cap);
  }
  for (uint64_t len : {1ull, 100ull, 64ull << 20}) for (uint64_t nf : {1ull, 63ull, 64ull, 65ull, (1ull << 29) - 3}) CHECK_EQ(decode_plan::avg_frame(len, nf), (len + nf - 1) / nf);
}

int main() {
  check_plan();
  check_choice();
  check_rows();
  check_window();
  check_side_layout();
  check_summary();
  check_scan_and_outputs();
  std::printf("comparisons %llu\nmismatches %d\n", cases, bad);
  return bad ? 1 : 0;
}
