"""Float text as the device compiles it: shortest output (float_json.h, float_display.h over ryu_table.h) and exact parsing (float_fast.h,
float_slow.h behind k_fin_fill) at scale, against references that share nothing with those headers (tests/float_reference.py: Python's
repr, numpy's unique scientific form, exact rationals) and the layouts of tests/snowflake_ndjson.py / tests/ducklake_literals.py.

Population A: ~6 000 finite bit patterns per width entered as their shortest text — every f32 exponent, every 8th f64 exponent, the
powers of ten around the layouts' thresholds, every digit count — decoded (Clinger's divide, Eisel-Lemire) and printed by every sink
under every lane split of the byte pass, staged through LDS and written directly. Population B: exact half-way points, texts only the
exact parser settles. Population C: float arrays, as literals and typed."""
import os
import struct
from fractions import Fraction

import numpy as np
import pytest

from etl_amd import abi
from tests import ducklake_literals as DL
from tests import float_reference as FR
from tests import pgwire as W
from tests import scenarios as SC
from tests.test_gpu_duckdb import _both_finished
from tests.test_gpu_duckdb import _check as _check_dl
from tests.test_gpu_ndjson import _check as _check_nd
from tests.test_gpu_rowbinary import _both, _stream

pytestmark = pytest.mark.gpu
EMU = os.environ.get("ETLG_SIMT_RUN") == "1"

N_A = 6144                           # patterns per width (24 workgroups of 256 rows); ~1 400 of them are not random fill (FR.population_a)
N_B = 400                            # base patterns per width, three texts each
N_C = 300                            # rows of two array cells
RB_LDS = 32 * 1024                   # the byte pass's LDS image (rowformats.hip.h kRbLds)


def _read(ptr, nbytes):
    if not nbytes:
        return np.zeros(0, np.uint8)
    if EMU:
        import ctypes as C
        return np.frombuffer((C.c_uint8 * nbytes).from_address(ptr), dtype=np.uint8).copy()
    return abi.device_tensor(ptr, nbytes, 0).cpu().numpy()


class _Arena:
    """A HostBatch for the _check helpers, materialised once: the reference rows are computed from the same list every time."""

    def __init__(self, hb):
        self.hb, self.slots, self._events = hb, hb.slots, None

    def materialize(self):
        if self._events is None:
            self._events = self.hb.materialize()
        return self._events


def _states(hb, ev, slot=0):
    """The state bits of every column of event ev's row."""
    base = int(hb.body_off[ev])
    return [(int(hb.fixed[base + i // 4]) >> (2 * (i % 4))) & 3 for i in range(len(hb.slots[slot].cols))]


def _bits(hb, ev, col, slot=0):
    c = hb.slots[slot].cols[col]
    at = int(hb.body_off[ev]) + c.off_full
    return struct.unpack_from("<Q" if c.type_class == abi.TC_F64 else "<I", hb.fixed, at)[0]


# ---------------------------------------------------------------------------------------------------------------- population A
A_COLS = [("id", SC.INT8, False, 1), ("x", SC.FLOAT8, True, 0), ("s", 25, True, 0), ("y", SC.FLOAT4, True, 0)]
A_NAMES = [c[0] for c in A_COLS]


@pytest.fixture(scope="module")
def pop_a():
    """The patterns in row order, the stream, and the oracle's plain decode of it (made once, never changed). Rows are ordered by the
    length of their DuckLake tuple's floats, longest first: the 64 longest rows (5e-324 prints as 326 bytes) are adjacent and lead
    workgroups whose piece outgrows the LDS image, the rows at the end are short enough for theirs to be staged."""
    from oracle import oracle
    p8, p4 = FR.population_a(False, N_A), FR.population_a(True, N_A)
    width = [len(DL.float_literal(a, False)) + len(DL.float_literal(c, True)) for a, c in zip(p8, p4)]
    order = sorted(range(N_A), key=lambda k: -width[k])
    p8, p4 = [p8[k] for k in order], [p4[k] for k in order]
    rows = [[str(i), FR.shortest_text(a, False), "s" * (7 * i % 23), FR.shortest_text(c, True)] for i, (a, c) in enumerate(zip(p8, p4))]
    buf, offs = _stream([W.insert(42, r) for r in rows] + [W.delete(42, old=r) for r in rows[::16]])
    prime = SC.simple_table(A_COLS, ident=[1] * len(A_COLS))
    o = oracle.Oracle()
    prime(o)
    rb = o.decode(buf, offs)
    assert rb.err_code == 0, rb.err_desc
    hb = rb.host_batch()
    return dict(p8=p8, p4=p4, rows=rows, buf=buf, offs=offs, prime=prime, hb=hb, arena=_Arena(hb), keep=(o, rb))


def _a_cells(hb, n):
    """(event, x state, y state, x bits, y bits) of the n Insert rows: event i + 1 is row i (Begin comes first)."""
    for i in range(n):
        st = _states(hb, i + 1)
        yield i, st[1], st[3], _bits(hb, i + 1, 1), _bits(hb, i + 1, 3)


def test_population_a_oracle_alone_is_clean(pop_a):
    """No cell is DEFERRED in the oracle's plain decode and every cell holds the pattern its text was made from; the population holds
    what the other tests rely on (every f32 exponent, the thresholds, both store paths of the byte pass at 256 rows per workgroup)."""
    hb, p8, p4 = pop_a["hb"], pop_a["p8"], pop_a["p4"]
    assert chr(hb.kind[1]) == "I" and chr(hb.kind[N_A]) == "I" and chr(hb.kind[N_A + 1]) == "D"
    bad = [(i, sx, sy, hex(bx), hex(by)) for i, sx, sy, bx, by in _a_cells(hb, N_A)
           if sx != abi.CELL_VALUE or sy != abi.CELL_VALUE or bx != p8[i] or by != p4[i]]
    assert not bad, (len(bad), bad[:5])
    assert {(b >> 23) & 0xFF for b in p4} == set(range(255))
    assert {(b >> 52) & 0x7FF for b in p8} >= set(range(0, 2047, 8)) | {0, 1, 2, 2044, 2045, 2046} | set(range(1020, 1028))
    assert {len(FR.shortest_digits(b, False)) for b in p8} == set(range(1, 18))
    assert {len(FR.shortest_digits(b, True)) for b in p4} == set(range(1, 10))
    v8, v4 = {FR.to_float(b, False) for b in p8}, {FR.to_float(b, True) for b in p4}
    assert all(float("1e%d" % k) in v8 for k in range(-8, 24))
    assert {2.0 ** 53 - 1, 2.0 ** 53, 2.0 ** 53 + 2} <= v8 and {2.0 ** 24 - 1, 2.0 ** 24, 2.0 ** 24 + 2} <= v4
    assert {0, 1 << 63, 1, (1 << 52) - 1, 1 << 52, (1 << 52) + 1} <= set(p8) and {0, 1 << 31, 1, 0x007FFFFF, 0x00800000} <= set(p4)
    # the DuckLake tuples of 256 consecutive rows: the first workgroups' pieces exceed the LDS image, the last are staged
    # (the 64 longest rows lead: `s` and `id`, which the order does not look at, add 26 bytes at the most)
    recs = DL.event_records(pop_a["arena"].materialize(), 0, A_NAMES, [1] * 4, DL.TUPLES)[0]
    assert len(recs) == N_A and max(len(r) for r in recs[:64]) >= 326 and min(len(r) for r in recs[:64]) >= max(len(r) for r in recs[64:]) - 26
    pieces = [sum(len(r) for r in recs[k:k + 256]) for k in range(0, N_A, 256)]
    assert pieces[0] > RB_LDS and pieces[-1] + 16 <= RB_LDS, pieces


def test_population_a_device_arena_holds_the_patterns(pop_a):
    """Clinger's divide and Eisel-Lemire as the device compiles them, against the target bits themselves."""
    hb, b, d = _both(pop_a["prime"], pop_a["buf"], pop_a["offs"])
    gh = b.host()
    diff = pop_a["hb"].diff(gh)
    assert not diff, diff[:6]
    bad = [(i, sx, sy, hex(bx), hex(by)) for i, sx, sy, bx, by in _a_cells(gh, N_A)
           if sx != abi.CELL_VALUE or sy != abi.CELL_VALUE or bx != pop_a["p8"][i] or by != pop_a["p4"][i]]
    assert not bad, (len(bad), bad[:5])
    assert d.debug_paths()["redone"] == 0
    b.close(); d.close()


@pytest.mark.parametrize("parts", [None, "1", "2", "4"])
def test_population_a_sinks_under_each_lane_split(pop_a, parts):
    """etlg_batch_ndjson, then etlg_batch_duckdb's tuples and predicates, host and device output, byte for byte: the counting pass and
    the byte pass of every formatter agree for every exponent and digit count, with a row's bytes written by 1, 2 and 4 lanes (the split
    falls between the two floats) and by the host's own choice."""
    from etl_amd.decoder import Decoder
    before = os.environ.get("ETLG_RB_PARTS")
    os.environ.pop("ETLG_RB_PARTS", None)
    if parts:
        os.environ["ETLG_RB_PARTS"] = parts
    try:
        d = Decoder(0)                       # (the variable is read when the context is created)
        pop_a["prime"](d)
        b = d.decode(pop_a["buf"], pop_a["offs"], flags=abi.F_OUTPUT_ON_DEVICE)
        assert b.rc == 0, b.error
        hb = pop_a["arena"]
        n_del = len(pop_a["rows"][::16])
        for on_device in (False, True):
            assert _check_nd(hb, b, A_NAMES, on_device=on_device) == N_A + n_del
        for what, n in ((abi.DL_TUPLES, N_A), (abi.DL_PREDICATES, n_del)):
            for on_device in (False, True):
                assert _check_dl(hb, b, A_NAMES, what, on_device=on_device) == n
        # one known answer read off the device without the layout helpers: the smallest subnormal, positionally and as ryu lays it out
        k = pop_a["p8"].index(1)
        r = b.duckdb(0, A_NAMES, what=abi.DL_TUPLES, on_device=True)
        o = _read(r.view.row_offsets, 8 * (N_A + 1)).view(np.int64)
        assert _read(r.view.bytes, int(r.view.n_bytes))[int(o[k]):int(o[k + 1])].tobytes().startswith(b"(%d, 0." % k + b"0" * 323 + b"5, '")
        r.close()
        r = b.ndjson(0, A_NAMES, on_device=True)
        o = _read(r.view.row_offsets, 8 * (N_A + 1)).view(np.int64)
        assert _read(r.view.bytes, int(r.view.n_bytes))[int(o[k]):int(o[k + 1])].tobytes().startswith(b'{"id":%d,"x":5e-324,"s":"' % k)
        r.close()
        b.close(); d.close()
    finally:
        os.environ.pop("ETLG_RB_PARTS", None)
        if before is not None:
            os.environ["ETLG_RB_PARTS"] = before


# ---------------------------------------------------------------------------------------------------------------- population B
B_COLS = [("id", SC.INT8, False, 1), ("x", SC.FLOAT8, True, 0), ("y", SC.FLOAT4, True, 0)]
B_NAMES = [c[0] for c in B_COLS]


def test_population_b_half_way_texts_through_the_exact_parser():
    """The exact half-way point between a float and its successor, one digit below and one above, for 400 patterns per width over every
    exponent: the fast rule leaves most of them DEFERRED, k_fin_fill's 768-digit decimal settles them, ties to even."""
    t8, t4 = FR.population_b(False, N_B), FR.population_b(True, N_B)
    n = len(t8)
    assert n == len(t4) == 3 * N_B and max(len(t) for t, _ in t8) > 1000 and max(len(t) for t, _ in t4) > 140
    for t, want in t8:                       # the reference against Python's own correctly rounded parse
        assert want == struct.unpack("<Q", struct.pack("<d", float(t)))[0], t
    # ties go to even: the half-way text itself reads as the even neighbour, the bumped ones as the lower and the upper
    for pop, is32 in ((t8, False), (t4, True)):
        for k in range(0, n, 3):
            half, lo, hi = pop[k][1], pop[k + 1][1], pop[k + 2][1]
            assert hi == lo + 1 and half in (lo, hi) and half % 2 == 0, pop[k][0]
            assert FR.bits_value(lo, is32) < Fraction(pop[k][0]) < FR.bits_value(hi, is32)
    buf, offs = _stream([W.insert(42, [str(i), a[0], c[0]]) for i, (a, c) in enumerate(zip(t8, t4))])
    prime = SC.simple_table(B_COLS)
    hb, b, d = _both(prime, buf, offs)
    # ---- the oracle alone
    deferred = [_states(hb, i + 1)[1:] for i in range(n)]
    n8, n4 = sum(s[0] == abi.CELL_DEFERRED for s in deferred), sum(s[1] == abi.CELL_DEFERRED for s in deferred)
    assert n8 >= 600 and n4 >= 600, (n8, n4)
    hf, bf, df = _both_finished(prime, buf, offs, True)
    bad = [(i, hex(_bits(hf, i + 1, 1)), hex(t8[i][1]), hex(_bits(hf, i + 1, 2)), hex(t4[i][1])) for i in range(n)
           if _states(hf, i + 1)[1:] != [abi.CELL_VALUE] * 2 or _bits(hf, i + 1, 1) != t8[i][1] or _bits(hf, i + 1, 2) != t4[i][1]]
    assert not bad, (len(bad), bad[:5])
    # ---- the device: the same cells DEFERRED by a plain decode ...
    gh = b.host()
    assert [_states(gh, i + 1)[1:] for i in range(n)] == deferred
    diff = hb.diff(gh)
    assert not diff, diff[:6]
    # ... none with the finish pass (the sinks first: they want the batch on the device), and every cell the reference's bits
    assert _check_nd(hf, bf, B_NAMES) == n
    assert _check_dl(hf, bf, B_NAMES, abi.DL_TUPLES, on_device=True) == n
    gf = bf.host()
    bad = [(i, _states(gf, i + 1), hex(_bits(gf, i + 1, 1)), hex(t8[i][1]), hex(_bits(gf, i + 1, 2)), hex(t4[i][1])) for i in range(n)
           if _states(gf, i + 1)[1:] != [abi.CELL_VALUE] * 2 or _bits(gf, i + 1, 1) != t8[i][1] or _bits(gf, i + 1, 2) != t4[i][1]]
    assert not bad, (len(bad), bad[:5])
    diff = hf.diff(gf)
    assert not diff, diff[:6]
    for x in (b, d, bf, df):
        x.close()


# ---------------------------------------------------------------------------------------------------------------- population C
C_COLS = [("id", SC.INT8, False, 1), ("a8", 1022, True, 0), ("a4", 1021, True, 0)]
C_NAMES = [c[0] for c in C_COLS]


@pytest.mark.parametrize("finish", [False, True], ids=["text_array", "typed_array"])
def test_population_c_float_arrays(finish):
    """float8[] / float4[] cells of 0..12 elements over population A's texts, NULLs and quoted elements among them: printed from the
    literal (the sink parses every element) and from the typed entry the finish pass leaves, whose elements are the patterns' bits."""
    p8, p4 = FR.population_a(False, 1536), FR.population_a(True, 1536)
    lits = FR.population_c(N_C, p8, p4)
    assert max(len(w) for _, w, _, _ in lits) == 12 and min(len(w) for _, w, _, _ in lits) == 0 and any('"' in a for a, _, _, _ in lits)
    buf, offs = _stream([W.insert(42, [str(i), a8, a4]) for i, (a8, _, a4, _) in enumerate(lits)])
    hb, b, d = _both_finished(SC.simple_table(C_COLS), buf, offs, finish)
    assert _check_nd(hb, b, C_NAMES) == N_C and _check_nd(hb, b, C_NAMES, on_device=True) == N_C
    assert _check_dl(hb, b, C_NAMES, abi.DL_TUPLES) == N_C and _check_dl(hb, b, C_NAMES, abi.DL_TUPLES, on_device=True) == N_C
    gh = b.host()
    diff = hb.diff(gh)
    assert not diff, diff[:6]
    rows = [e["row"] for e in gh.materialize() if e["kind"] == "I"]
    for (a8, w8, a4, w4), row in zip(lits, rows):
        if not finish:
            assert row[1] == ("Deferred", 1022, a8.encode()) and row[2] == ("Deferred", 1021, a4.encode())
            continue
        for cell, name, want in ((row[1], "F64", w8), (row[2], "F32", w4)):
            assert cell == ("Array", name, [("Null",) if w is None else (name, w) for w in want]), (a8, a4)
    b.close(); d.close()
