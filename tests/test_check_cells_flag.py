"""ETLG_F_CHECK_CELLS has one value in the C header, the Python bindings and the Rust crate."""
import os
import re

from etl_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_value_in_header_bindings_and_crate():
    h = open(os.path.join(ROOT, "include", "etlg.h")).read()
    rs = open(os.path.join(ROOT, "crates", "etl-gfx950", "src", "ffi.rs")).read()
    mh = re.search(r"ETLG_F_CHECK_CELLS\s*=\s*1u\s*<<\s*(\d+)", h)
    mr = re.search(r"pub const ETLG_F_CHECK_CELLS: u32 = 1 << (\d+);", rs)
    assert mh and mr
    assert abi.F_CHECK_CELLS == 1 << int(mh.group(1)) == 1 << int(mr.group(1)) == 32
    flags = [abi.F_INPUT_ON_DEVICE, abi.F_OUTPUT_ON_DEVICE, abi.F_NO_CONTROL, abi.F_ASYNC, abi.F_FINISH_CELLS, abi.F_CHECK_CELLS]
    assert len(set(flags)) == len(flags)


def test_the_crate_offers_the_option_and_defaults_to_off():
    lib = open(os.path.join(ROOT, "crates", "etl-gfx950", "src", "lib.rs")).read()
    assert "pub fn set_check_cells(&mut self, on: bool)" in lib and "check_cells: false" in lib
    assert "ETLG_F_CHECK_CELLS" in lib
