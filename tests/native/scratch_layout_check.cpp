// Stand-alone check of etl_amd/csrc/scratch_layout.h (tests/test_scratch_layout.py builds it with the address and undefined-behaviour
// sanitizers): the carve hands out parts that start at multiples of 64, never descend and never overlap, a zero-byte take takes nothing,
// and the two layouts with the most links lie where the offset chains they replaced put them. The expected offsets are written out
// here, link by link, with this file's own rounding; nothing expected is obtained from the header.
#include "scratch_layout.h"

#include <cstdio>
#include <vector>

static int bad = 0;
#define CHECK(cond) do { if (!(cond)) { bad++; std::printf("FAILED line %d: %s\n", __LINE__, #cond); } } while (0)
#define CHECK_EQ(a, b) do { const unsigned long long a_ = (unsigned long long)(a), b_ = (unsigned long long)(b); \
    if (a_ != b_) { bad++; std::printf("FAILED line %d: %s = %llu, expected %llu\n", __LINE__, #a, a_, b_); } } while (0)

static size_t up64(size_t x) { return (x + 63) / 64 * 64; }

static void check_carve() {
  const size_t sizes[] = {0, 1, 63, 64, 65, 0, 4096, 7, 0, 0, 1000003, 8, 64 * 3, 0};
  ScratchLayout l;
  CHECK_EQ(l.total(), 0);
  std::vector<size_t> at, len;
  size_t prev = 0;
  for (size_t b : sizes) {
    const size_t before = l.total(), o = l.take(b);
    CHECK_EQ(o, before);                       // a part starts where the block ended
    CHECK(o % 64 == 0);
    CHECK(o >= prev);                          // never descends
    CHECK(l.total() >= o + b);                 // the part lies inside the block
    CHECK(l.total() % 64 == 0);
    CHECK(l.total() - o < b + 64);             // and costs less than 64 bytes of padding
    if (!b) CHECK_EQ(l.total(), before);       // a zero-byte take takes nothing
    at.push_back(o); len.push_back(b); prev = o;
  }
  for (size_t i = 0; i < at.size(); i++)
    for (size_t k = i + 1; k < at.size(); k++) CHECK(at[i] + len[i] <= at[k]);   // no two parts overlap
  // the raw advance: exactly the bytes asked for (a 64-byte record, the slack at a block's end), returned like take
  ScratchLayout r;
  r.take(100);
  CHECK_EQ(r.skip(64), 128);
  CHECK_EQ(r.take(8), 192);
  CHECK_EQ(r.skip(0), 256);
  CHECK_EQ(r.total(), 256);
  CHECK_EQ(al64(0), 0); CHECK_EQ(al64(1), 64); CHECK_EQ(al64(64), 64); CHECK_EQ(al64(65), 128);
}

// etlg_batch_cuts: o_tsum = al64(5 * 8), o_tinc = o_tsum + al64(n_tiles * 8), o_q = o_tinc + al64(n_tiles * 8),
// o_hints = o_q + al64((n + 1) * 8), total = o_hints + (hints ? 0 : al64(ne * 8))
static void check_cuts(unsigned long long n, unsigned long long tile, bool hints_given) {
  const unsigned long long n_tiles = (n + tile - 1) / tile, ne = n + 11;   // (the range is a part of the batch's events)
  const size_t o_tsum = up64(5 * 8), o_tinc = o_tsum + up64(n_tiles * 8), o_q = o_tinc + up64(n_tiles * 8), o_hints = o_q + up64((n + 1) * 8),
               total = o_hints + (hints_given ? 0 : up64(ne * 8));
  const CutsLayout l = cuts_layout(n, n_tiles, ne, !hints_given);
  CHECK_EQ(l.hdr, 0); CHECK_EQ(l.tsum, o_tsum); CHECK_EQ(l.tinc, o_tinc); CHECK_EQ(l.q, o_q); CHECK_EQ(l.hints, o_hints); CHECK_EQ(l.total, total);
  const size_t at[] = {l.hdr, l.tsum, l.tinc, l.q, l.hints, l.total};
  for (size_t i = 0; i < 6; i++) { CHECK(at[i] % 64 == 0); if (i) CHECK(at[i] >= at[i - 1]); }
}

// etlg_batch_payload, the chain of its fourteen links
static void check_payload(bool want_sums, bool out_dev, bool ev_bytes_out, bool cuts_on_device) {
  const unsigned long long ne = 2049, nf = 300, n_recv = 300, n_cuts = 2, n_ranges = n_cuts + 1;
  const unsigned n_bounds = 3, n_hist = 4 * (n_bounds + 1), hdr_words = 11, n_tiles = (unsigned)((n_recv + 255) / 256), n_etiles = (unsigned)((ne + 2047) / 2048);
  const size_t o_hist = up64(hdr_words * 8), o_bounds = o_hist + up64((size_t)n_hist * 8), o_fbytes = o_bounds + up64(64 * 8), o_tcnt = o_fbytes + up64(n_recv * 4),
               o_r2f = o_tcnt + up64((size_t)n_tiles * 8), o_brank = o_r2f + up64(nf * 4), o_etb = o_brank + up64(nf * 4), o_evb = o_etb + up64((size_t)n_etiles * 8),
               o_tsum = o_evb + (out_dev && ev_bytes_out ? 0 : up64(ne * 4)), o_pb = o_tsum + (want_sums ? up64((size_t)n_etiles * 48) : 0),
               o_pr = o_pb + (want_sums ? up64(3 * (ne + 1) * 8) : 0), o_cuts = o_pr + (want_sums ? up64(3 * (ne + 1) * 4) : 0),
               o_sums = o_cuts + (want_sums && !cuts_on_device ? up64(n_cuts * 8) : 0), total = o_sums + (want_sums && !out_dev ? up64(n_ranges * 64) : 0);
  const PayLayout l = payload_layout(hdr_words, n_hist, n_recv, nf, ne, n_tiles, n_etiles, n_cuts, !(out_dev && ev_bytes_out), want_sums, !cuts_on_device, !out_dev);
  CHECK_EQ(l.hdr, 0); CHECK_EQ(l.hist, o_hist); CHECK_EQ(l.bounds, o_bounds); CHECK_EQ(l.fbytes, o_fbytes); CHECK_EQ(l.tcnt, o_tcnt); CHECK_EQ(l.r2f, o_r2f);
  CHECK_EQ(l.brank, o_brank); CHECK_EQ(l.etb, o_etb); CHECK_EQ(l.evb, o_evb); CHECK_EQ(l.tsum, o_tsum); CHECK_EQ(l.pb, o_pb); CHECK_EQ(l.pr, o_pr);
  CHECK_EQ(l.cuts, o_cuts); CHECK_EQ(l.sums, o_sums); CHECK_EQ(l.total, total);
  const size_t at[] = {l.hdr, l.hist, l.bounds, l.fbytes, l.tcnt, l.r2f, l.brank, l.etb, l.evb, l.tsum, l.pb, l.pr, l.cuts, l.sums, l.total};
  for (size_t i = 0; i < 15; i++) { CHECK(at[i] % 64 == 0); if (i) CHECK(at[i] >= at[i - 1]); }
  if (want_sums && !out_dev && !cuts_on_device) CHECK_EQ(total, 64 * (2 + 2 + 8 + 19 + 1 + 19 + 19 + 1 + 129 + 2 + 769 + 385 + 1 + 3));   // the same, counted by hand in 64-byte lines
}

int main() {
  check_carve();
  for (int given = 0; given < 2; given++) { check_cuts(1, 2048, given != 0); check_cuts(2049, 2048, given != 0); check_cuts(49157, 128, given != 0); }
  for (int sums = 0; sums < 2; sums++)
    for (int m = 0; m < 8; m++) check_payload(sums != 0, (m & 1) != 0, (m & 2) != 0, (m & 4) != 0);
  std::printf("mismatches %d\n", bad);
  return bad ? 1 : 0;
}
