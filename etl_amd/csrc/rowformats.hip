// The RowBinary / protobuf and NDJSON kernels (rowformats.hip.h), and the launcher of every row format.
#include "rowformats.hip.h"

extern "C" void etlg_k_rows_ducklake(const etlg::RbJob* j, unsigned long long* blk, int64_t* offsets, unsigned long long* tot, int step, hipStream_t st);   // rowformats_dl.hip

// step 0: lengths + offsets (blk: (nblocks + 1) x u64 scratch); step 1: the bytes
extern "C" void etlg_k_rowbinary(const etlg::RbJob* jv, unsigned long long* blk, int64_t* offsets, unsigned long long* tot, int step, hipStream_t st) {
  using namespace etlg;
  const RbJob j = *jv;
  if (!j.n_rows) return;
  if (j.format == FMT_DUCKLAKE) etlg_k_rows_ducklake(&j, blk, offsets, tot, step, st);
  else if (j.format == FMT_NDJSON) rb_launch_js<NdFormat>(j, blk, offsets, tot, step, st);
  else rb_launch_js<RbPbFormat>(j, blk, offsets, tot, step, st);
}
