"""The float formatters and parsers of the kernels without a GPU: tests/test_gpu_float_text.py against the SIMT emulator build
(tests/simt/build.py) — in the default lane order, with the lanes of every workgroup shuffled between rendezvous, and with the byte pass
forced to 1, 2 and 4 lanes per row (ETLG_RB_PARTS) for the tests that do not set it themselves. TEST INFRASTRUCTURE: the emulator
build is g++'s compilation of the headers, so this run checks the populations, the references and the plumbing; the -m gpu run of
the same file on an MI355X is the check of the device compilation and stays the gate."""
import os
import subprocess
import sys

import pytest

from tests.test_simt_emulation import ROOT, _emu_env, simt_lib  # noqa: F401  (the emulator build, by import)


def test_reference_helper_stands_apart_from_the_product_headers():
    """tests/float_reference.py imports nothing of the product and opens no file; its rounding agrees with Python's own correctly rounded
    float() on random decimal texts, and every pattern's shortest text reads back as the pattern in both widths."""
    import random
    import re
    import struct
    from fractions import Fraction
    from tests import float_reference as FR
    src = open(os.path.join(ROOT, "tests", "float_reference.py")).read()
    assert not re.search(r"^\s*(from|import)\s+(etl_amd|oracle|tests|ctypes)", src, re.M) and "open(" not in src and "#include" not in src
    rng = random.Random(7)
    for _ in range(1500):
        t = "%d.%de%d" % (rng.randint(0, 10 ** rng.randint(1, 25)), rng.randint(0, 10 ** 18), rng.randint(-345, 310))
        assert FR.round_fraction(Fraction(t), False) == struct.unpack("<Q", struct.pack("<d", float(t)))[0], t
    for is32 in (False, True):
        for b in FR.population_a(is32, 1536):
            mag = b & ~(1 << (31 if is32 else 63))
            assert FR.round_fraction(FR.bits_value(mag, is32), is32) == mag
            assert not mag or FR.round_fraction(Fraction(FR.shortest_text(b, is32)), is32) == b, hex(b)
    assert FR.exact_decimal(FR.bits_value(1, True)) == "0." + "0" * 44 + str(5 ** 149) and str(5 ** 149).startswith("14012984643248170709")   # 2^-149
    assert FR.exact_decimal(Fraction(3, 8)) == "0.375" and FR.exact_decimal(Fraction(12)) == "12"
    assert FR.bump("0.125", 1) == "0.126" and FR.bump("0.125", -1) == "0.124" and FR.bump("99", 1) == "100" and FR.bump("0.09", 1) == "0.10" and FR.bump("1.00", -1) == "0.99"


@pytest.mark.parametrize("order,parts", [(None, None), ("shuffle", None), (None, "1"), (None, "2"), ("shuffle", "4")])
def test_float_text_on_the_emulator(simt_lib, order, parts):  # noqa: F811
    env = _emu_env(simt_lib, 900, order)
    env.pop("ETLG_RB_PARTS", None)
    if parts:
        env["ETLG_RB_PARTS"] = parts
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_float_text.py"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-4000:], out.stderr[-2000:])
    assert " passed" in out.stdout and "skipped" not in out.stdout
