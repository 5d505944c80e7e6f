"""The DuckLake literal kernels' float text (etl_amd/csrc/float_display.h: Ryu's shortest round-trip digits laid out positionally, what
Rust's f64 Display writes; a float4 widened first) against libstdc++'s std::to_chars(.., chars_format::fixed), through a host build of
the same header (tests/native/float_display_check.cpp): 10^7 random bit patterns of each width — as many as tests/test_float_json.py
runs —, every power of two of both widths with its neighbours, zeros, the subnormal extremes, DBL_MAX / FLT_MAX, the powers of ten
1e-30 .. 1e30 — zero mismatches, and the count pass's length equal to the written length on every one.

to_chars' fixed text is byte-equal to Display wherever it is the shortest positional form. For most integers of 2^53 and more
libstdc++ prints the exact integer instead (1e23 -> 99999999999999991611392, Display -> 100000000000000000000000): on those 7.6
million of the 22 million values the check is tied to to_chars by its length, by its own shortest digits (chars_format::scientific) laid
out positionally, by its leading 17 digits to within the rounding interval, and by strtod reading the text back as the same bits."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_float_display_matches_to_chars(tmp_path):
    exe = str(tmp_path / "float_display_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "etl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "float_display_check.cpp"), "-o", exe])
    out = subprocess.run([exe, "10000000"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:]
    assert "mismatches 0" in out.stdout
    assert int(out.stdout.split("checked ")[1].split()[0]) > 2 * 10**7
    assert int(out.stdout.split("longest ")[1].split()[0]) == 327       # "-0." + 323 zeros + a digit .. : what the count pass must size


def test_float_display_pinned_layouts(tmp_path):
    """A few texts of every layout row, written out (the table in float_display.h)."""
    src = tmp_path / "pins.cpp"
    src.write_text('#include <stdio.h>\n#include <string.h>\n#include <string>\n#include "float_display.h"\n'
                   'struct B { std::string s; void put(uint8_t c) { s.push_back((char)c); } };\n'
                   'int main() { double d[] = {0.0, -0.0, 1.0, 0.1, 1e21, 1e23, 12.34, 0.00001, 1.5e-7, -3.0, 5e-324, 1.7976931348623157e308};\n'
                   '  for (double v : d) { uint64_t b; memcpy(&b, &v, 8); B o; etlg::float_display(o, b); printf("%s\\n", o.s.c_str()); }\n'
                   '  float f[] = {0.1f, 1.5f, 1e-45f, 3.4028235e38f, -0.0f};\n'
                   '  for (float v : f) { uint32_t b; memcpy(&b, &v, 4); B o; etlg::float_display(o, etlg::f32_widen_bits(b)); printf("%s\\n", o.s.c_str()); } }\n')
    exe = str(tmp_path / "pins")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "etl_amd", "csrc"), str(src), "-o", exe])
    got = subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()
    assert got == ["0", "-0", "1", "0.1", "1" + "0" * 21, "1" + "0" * 23, "12.34", "0.00001", "0.00000015", "-3", "0." + "0" * 323 + "5",
                   "17976931348623157" + "0" * 292,
                   "0.10000000149011612", "1.5", "0." + "0" * 44 + "1401298464324817", "34028234663852886" + "0" * 22, "-0"]
