"""The NDJSON kernels' float text (etl_amd/csrc/float_json.h: Ryu's shortest round-trip digits in ryu's format32 / format64 layout,
what serde_json writes for an f32 / f64) against libstdc++'s std::to_chars, through a host build of the same header: 10^7 random bit
patterns of each width, every power of two with its neighbours, the subnormal and normal extremes, and the values around every
layout threshold — zero mismatches."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_float_json_matches_to_chars(tmp_path):
    exe = str(tmp_path / "float_json_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "etl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "float_json_check.cpp"), "-o", exe])
    out = subprocess.run([exe, "10000000"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:]
    assert "mismatches 0" in out.stdout
    assert int(out.stdout.split("checked ")[1].split()[0]) > 2 * 10**7


def test_float_json_pinned_layouts(tmp_path):
    """A few texts of every layout row, written out (the table in float_json.h)."""
    src = tmp_path / "pins.cpp"
    src.write_text('#include <stdio.h>\n#include <string.h>\n#include <string>\n#include "float_json.h"\n'
                   'struct B { std::string s; void put(uint8_t c) { s.push_back((char)c); } };\n'
                   'int main() { double d[] = {0.0, -0.0, 1.5, 2.5, 1e15, 1e16, 12.34, 0.00001, 0.000001, 1.5e-7, 1.234e33, -3.0, 5e-324, 1.7976931348623157e308};\n'
                   '  for (double v : d) { uint64_t b; memcpy(&b, &v, 8); B o; etlg::float_json(o, b, false); printf("%s\\n", o.s.c_str()); }\n'
                   '  float f[] = {1.5f, 1e12f, 1e13f, 0.00001f, 0.000001f, 1e-7f, 3.4028235e38f, 1e-45f};\n'
                   '  for (float v : f) { uint32_t b; memcpy(&b, &v, 4); B o; etlg::float_json(o, b, true); printf("%s\\n", o.s.c_str()); } }\n')
    exe = str(tmp_path / "pins")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "etl_amd", "csrc"), str(src), "-o", exe])
    got = subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()
    assert got == ["0.0", "-0.0", "1.5", "2.5", "1000000000000000.0", "1e16", "12.34", "0.00001", "1e-6", "1.5e-7", "1.234e33", "-3.0",
                   "5e-324", "1.7976931348623157e308",
                   "1.5", "1000000000000.0", "1e13", "0.00001", "0.000001", "1e-7", "3.4028235e38", "1e-45"]
