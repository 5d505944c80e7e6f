// The DuckLake kernels (rowformats.hip.h): tuples / predicates, and the partial Updates in instantiations of their own — sharing the
// tuples' ones cost the two older modes 2 % (profiles/duckdb_updates_probe_mi355x.txt). A source of its own for the build's sake: the
// row formats are most of its time, and the two sources compile side by side.
#include "rowformats.hip.h"

extern "C" void etlg_k_rows_ducklake(const etlg::RbJob* j, unsigned long long* blk, int64_t* offsets, unsigned long long* tot, int step, hipStream_t st) {
  using namespace etlg;
  if (j->dl_what == DL_ROW_UPDATES) rb_launch_js<DlUpdFormat>(*j, blk, offsets, tot, step, st); else rb_launch_js<DlFormat>(*j, blk, offsets, tot, step, st);
}
