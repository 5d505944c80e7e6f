// How the hand-off calls carve a scratch block: a running offset that hands out 64-byte aligned parts (parts that overlap would be a GPU fault, so no
// caller adds offsets by hand), and the two layouts with the most links. Plain C++, no HIP: tests/native/scratch_layout_check.cpp includes this header alone.
#pragma once
#include <cstddef>
#include <cstdint>

inline size_t al64(size_t x) { return (x + 63) & ~(size_t)63; }   // the parts of a shared block start at multiples of 64 bytes

struct ScratchLayout {
  size_t off;
  explicit ScratchLayout(size_t first = 0) : off(al64(first)) {}   // `first`: the bytes of the part at offset 0
  size_t take(size_t bytes) { const size_t at = off; off += al64(bytes); return at; }   // the next part: where it starts. take(0) takes nothing
  size_t skip(size_t bytes) { const size_t at = off; off += bytes; return at; }         // the few links that are not al64 (a fixed 64-byte record)
  size_t total() const { return off; }   // (the callers allocate 64 bytes of slack behind it)
};

// etlg_batch_cuts, the block of its first stop: hdr (5 words) | tsum | tinc (a word per tile) | q (n + 1 words) | the hints of the whole
// batch when the library evaluates them itself (own_hints; `hints` is then where k_size_hints writes)
struct CutsLayout { size_t hdr, tsum, tinc, q, hints, total; };
inline CutsLayout cuts_layout(uint64_t n, uint64_t n_tiles, uint64_t n_events, bool own_hints) {
  ScratchLayout l; CutsLayout o{};
  o.hdr = l.take(5 * 8); o.tsum = l.take(n_tiles * 8); o.tinc = l.take(n_tiles * 8); o.q = l.take((n + 1) * 8);
  o.hints = own_hints ? l.take(n_events * 8) : l.total();
  o.total = l.total();
  return o;
}

// etlg_batch_outline, its one block. What starts as zeros lies together ([zero_at, ones_at): the range-start bitmap, the census' rows, the
// touched words of the passes that can be written, hdr), then what starts as all ones ([ones_at, ones_end): bad, the census' firsts, de,
// re), then what is written before it is read (tsum, tf), a host caller's cuts, and the staging of a host caller's outputs in one piece
// ([stage_at, total): passes | ends | touched | truncates | slots). hdr and bad are neighbours: one read-back of 72 bytes brings both.
// P: the passes that can be written, min(passes_cap, n); T: the truncate entries that can be; a part nobody asked for takes nothing.
struct OutlineLayout { size_t zero_at, bitmap, crow, touched, hdr, ones_at, bad, cfirst, de, re, ones_end, tsum, tf, cuts, stage_at, s_passes, s_ends, s_touched, s_trunc, s_slots, total; };
inline OutlineLayout outline_layout(uint64_t n, uint64_t n_tiles, uint64_t n_slots, uint64_t W, uint64_t P, uint64_t T, uint64_t n_cuts, bool want_passes, bool want_ends,
                                    bool want_touched, bool want_slots, bool cuts_here, bool stage) {
  ScratchLayout l; OutlineLayout o{};
  o.zero_at = o.bitmap = l.take((n / 32 + 1) * 4); o.crow = l.take(n_slots * 48); o.touched = l.take(want_touched ? P * W * 8 : 0); o.hdr = l.take(64);
  o.ones_at = o.bad = l.take(64); o.cfirst = l.take(n_slots * 48); o.de = l.take(want_passes ? P * 8 : 0); o.re = l.take(want_passes ? P * 8 : 0);
  o.ones_end = l.total();
  o.tsum = l.take(n_tiles * 32); o.tf = l.take(want_passes ? (P + 1) * 8 : 0); o.cuts = l.take(cuts_here ? n_cuts * 8 : 0);
  o.stage_at = l.total();
  o.s_passes = l.take(stage && want_passes ? P * 56 : 0); o.s_ends = l.take(stage && want_ends ? P * 8 : 0); o.s_touched = l.take(stage && want_touched ? P * W * 8 : 0);
  o.s_trunc = l.take(stage ? T * 16 : 0); o.s_slots = l.take(stage && want_slots ? n_slots * 96 : 0);
  o.total = l.total();
  return o;
}

// etlg_ducklake_plan, its one block: hdr (4 words of zeros, then 4 of all ones) | what is written before it is read — the tile sums, a
// code byte and rpre per event, the groups per window with their scan, the dense list, the groups' starts, two record positions per
// member, the ops per group with their scan — | a host caller's passes | the staging of a host caller's outputs in one piece
// ([stage_at, total): ranges | batches | ops). B, K: the groups and ops that can be written; a part nobody asked for takes nothing.
struct DlpLayout { size_t hdr, tsum, code, rpre, glens, gblk, gpre, dense, gstart, mpos, oplens, oblk, opre, passes, stage_at, s_ranges, s_batches, s_ops, total; };
inline DlpLayout dlp_layout(uint64_t n, uint64_t n_tiles, uint64_t n_passes, uint64_t B, uint64_t K, bool want_ranges, bool want_batches, bool passes_here, bool stage) {
  ScratchLayout l; DlpLayout o{};
  o.hdr = l.take(64); o.tsum = l.take(n_tiles * 16); o.code = l.take(n); o.rpre = l.take((n + 1) * 8);
  o.glens = l.take(n_passes * 4); o.gblk = l.take((n_passes / 256 + 2) * 8); o.gpre = l.take((n_passes + 1) * 8);
  o.dense = l.take(n * 8); o.gstart = l.take((n + 1) * 8); o.mpos = l.take(n * 16);
  o.oplens = l.take(n * 4); o.oblk = l.take((n / 256 + 2) * 8); o.opre = l.take((n + 1) * 8);
  o.passes = l.take(passes_here ? n_passes * 56 : 0);
  o.stage_at = l.total();
  o.s_ranges = l.take(stage && want_ranges ? B * 24 : 0); o.s_batches = l.take(stage && want_batches ? B * 104 : 0); o.s_ops = l.take(stage ? K * 32 : 0);
  o.total = l.total();
  return o;
}

// etlg_snowflake_plan, its one block: hdr (4 words of zeros, 4 of all ones, 8 of zeros) | what is written before it is read — the tile
// sums, a code byte and two prefixes per event, two rows and the segments per window with their scan, the jump levels over the rows —
// | a host caller's passes | the staging of a host caller's outputs in one piece ([stage_at, total): segments | windows). E: the
// segments that can be written; a part nobody asked for takes nothing.
struct SfpLayout { size_t hdr, tsum, code, pre, wrow, slens, sblk, spre, jump, passes, stage_at, s_segs, s_wins, total; };
inline SfpLayout sfp_layout(uint64_t n, uint64_t n_tiles, uint64_t n_passes, uint64_t n_rows, uint32_t levels, uint64_t E, bool want_wins, bool passes_here, bool stage) {
  ScratchLayout l; SfpLayout o{};
  o.hdr = l.take(128); o.tsum = l.take(n_tiles * 16); o.code = l.take(n); o.pre = l.take((n + 1) * 16);
  o.wrow = l.take(n_passes * 16); o.slens = l.take(n_passes * 4); o.sblk = l.take((n_passes / 256 + 2) * 8); o.spre = l.take((n_passes + 1) * 8);
  o.jump = l.take((size_t)levels * (n_rows + 2) * 4);
  o.passes = l.take(passes_here ? n_passes * 56 : 0);
  o.stage_at = l.total();
  o.s_segs = l.take(stage ? E * 104 : 0); o.s_wins = l.take(stage && want_wins ? n_passes * 56 : 0);
  o.total = l.total();
  return o;
}

// etlg_clickhouse_plan, its one block: hdr (4 words of zeros, 4 of all ones, 8 of zeros) | what is written before it is read — the tile
// sums, a code byte and a prefix per event, two rows and the statements per window with their scan, the jump levels over the rows —
// | a host caller's passes | the staging of a host caller's outputs in one piece ([stage_at, total): statements | windows). E: the
// statements that can be written; a part nobody asked for takes nothing.
struct ChpLayout { size_t hdr, tsum, code, pre, wrow, slens, sblk, spre, jump, passes, stage_at, s_stmts, s_wins, total; };
inline ChpLayout chp_layout(uint64_t n, uint64_t n_tiles, uint64_t n_passes, uint64_t n_rows, uint32_t levels, uint64_t E, bool want_wins, bool passes_here, bool stage) {
  ScratchLayout l; ChpLayout o{};
  o.hdr = l.take(128); o.tsum = l.take(n_tiles * 8); o.code = l.take(n); o.pre = l.take((n + 1) * 8);
  o.wrow = l.take(n_passes * 16); o.slens = l.take(n_passes * 4); o.sblk = l.take((n_passes / 256 + 2) * 8); o.spre = l.take((n_passes + 1) * 8);
  o.jump = l.take((size_t)levels * (n_rows + 2) * 4);
  o.passes = l.take(passes_here ? n_passes * 56 : 0);
  o.stage_at = l.total();
  o.s_stmts = l.take(stage ? E * 56 : 0); o.s_wins = l.take(stage && want_wins ? n_passes * 48 : 0);
  o.total = l.total();
  return o;
}

// etlg_bigquery_plan, its one block, as ChpLayout without the jump levels: hdr (4 words of zeros, 4 of all ones, 8 of zeros) | the tile
// sums, a code byte and a prefix per event, two rows and a 0 / 1 request per window with their scan | a host caller's passes | the
// staging of a host caller's outputs in one piece ([stage_at, total): requests | windows). E: the requests that can be written; n_win:
// the window entries (one on a table-copy batch, which takes none of the per-event parts: n == 0).
struct BqpLayout { size_t hdr, tsum, code, pre, wrow, slens, sblk, spre, passes, stage_at, s_reqs, s_wins, total; };
inline BqpLayout bqp_layout(uint64_t n, uint64_t n_tiles, uint64_t n_passes, uint64_t n_win, uint64_t E, bool want_wins, bool passes_here, bool stage) {
  ScratchLayout l; BqpLayout o{};
  o.hdr = l.take(128); o.tsum = l.take(n_tiles * 8); o.code = l.take(n); o.pre = l.take(n ? (n + 1) * 8 : 0);
  o.wrow = l.take(n_passes * 16); o.slens = l.take(n_passes * 4); o.sblk = l.take((n_passes / 256 + 2) * 8); o.spre = l.take((n_passes + 1) * 8);
  o.passes = l.take(passes_here ? n_passes * 56 : 0);
  o.stage_at = l.total();
  o.s_reqs = l.take(stage ? E * 64 : 0); o.s_wins = l.take(stage && want_wins ? n_win * 56 : 0);
  o.total = l.total();
  return o;
}

// etlg_iceberg_plan, its one block, as BqpLayout with the second prefix and the bitmap side: hdr (4 words of zeros, 4 of all ones, 8 of
// zeros) | the tile sums of members and of other-slot events, a code byte and two prefixes per event, three words and a 0 / 1 write per
// window with their scan | the word space's tile sums and its prefix (W words: W + 1 entries) | what the host uploads in one piece
// ([up_at, stage_at): the column records, the bitmap records with their closing entry, a host caller's passes) | the staging of a host
// caller's outputs in one piece ([stage_at, total): writes | slices | windows). E: the writes that can be written; n_win: the window
// entries (one on a table-copy batch, which takes none of the per-event parts: n == 0).
struct IcpLayout { size_t hdr, tsum, fsum, code, pre, fpre, wrow, slens, sblk, spre, bsum, bpre, up_at, cols, bitmaps, passes, stage_at, s_writes, s_slices, s_wins, total; };
inline IcpLayout icp_layout(uint64_t n, uint64_t n_tiles, uint64_t n_passes, uint64_t n_win, uint64_t E, uint64_t n_cols, uint64_t n_bitmaps, uint64_t W, uint64_t n_wtiles,
                            bool want_writes, bool want_slices, bool want_wins, bool passes_here, bool stage) {
  ScratchLayout l; IcpLayout o{};
  o.hdr = l.take(128); o.tsum = l.take(n_tiles * 8); o.fsum = l.take(n_tiles * 8); o.code = l.take(n); o.pre = l.take(n ? (n + 1) * 8 : 0); o.fpre = l.take(n ? (n + 1) * 8 : 0);
  o.wrow = l.take(n_passes * 24); o.slens = l.take(n_passes * 4); o.sblk = l.take((n_passes / 256 + 2) * 8); o.spre = l.take((n_passes + 1) * 8);
  o.bsum = l.take(n_wtiles * 8); o.bpre = l.take((W + 1) * 8);
  o.up_at = l.total();
  o.cols = l.take(n_cols * 56); o.bitmaps = l.take((n_bitmaps + 1) * 16); o.passes = l.take(passes_here ? n_passes * 56 : 0);
  o.stage_at = l.total();
  o.s_writes = l.take(stage && want_writes ? E * 56 : 0); o.s_slices = l.take(stage && want_slices ? E * n_cols * 56 : 0); o.s_wins = l.take(stage && want_wins ? n_win * 48 : 0);
  o.total = l.total();
  return o;
}

// etlg_batch_payload: hdr | hist | bounds (the three the call reads back and uploads) | the frame side | the event side. ev_bytes and sums
// live here unless they go straight to the caller's device memory; the range sums' parts exist only when sums are asked for.
struct PayLayout { size_t hdr, hist, bounds, fbytes, tcnt, r2f, brank, etb, evb, tsum, pb, pr, cuts, sums, total; };
inline PayLayout payload_layout(uint32_t hdr_words, uint32_t n_hist, uint64_t n_recv, uint64_t nf, uint64_t ne, uint32_t n_tiles, uint32_t n_etiles, uint64_t n_cuts,
                                bool evb_here, bool want_sums, bool cuts_here, bool sums_here) {
  ScratchLayout l; PayLayout o{};
  o.hdr = l.take((size_t)hdr_words * 8); o.hist = l.take((size_t)n_hist * 8); o.bounds = l.take(64 * 8);
  o.fbytes = l.take(n_recv * 4); o.tcnt = l.take((size_t)n_tiles * 8); o.r2f = l.take(nf * 4); o.brank = l.take(nf * 4); o.etb = l.take((size_t)n_etiles * 8);
  o.evb = l.take(evb_here ? ne * 4 : 0); o.tsum = l.take(want_sums ? (size_t)n_etiles * 48 : 0);
  o.pb = l.take(want_sums ? 3 * (ne + 1) * 8 : 0); o.pr = l.take(want_sums ? 3 * (ne + 1) * 4 : 0);
  o.cuts = l.take(want_sums && cuts_here ? n_cuts * 8 : 0); o.sums = l.take(want_sums && sums_here ? (n_cuts + 1) * 64 : 0);
  o.total = l.total();
  return o;
}
