"""Table-copy batches for the ClickHouse, BigQuery and DuckLake sinks, through the C ABI, host and device output, byte for byte against
the host model tests/table_copy_sinks.py (built from materialize(), pinned to the reference by tests/test_table_copy_sink_kats.py):

  etlg_batch_rowbinary / etlg_batch_protobuf on a copy batch (rowformats.hip.h, RbJob.copy_tail): every row kept, the CDC tail of
    (Insert, commit_lsn 0, tx_ordinal 0) / the single trailing _CHANGE_TYPE field, under 1, 2 and 4 lanes per row with rows that take the
    staged LDS image and rows that take the direct path, both ClickHouse engines, the errors at their row;
  etlg_batch_ducklake_copy (columns.hip: the 2-byte store, the int32 offsets): kinds, values, zeroed null slots, int32 offsets, deferred
    floats, the NOT_ARROW and OFFSETS_OVERFLOW reports, argument errors, an ASYNC batch; every buffer against etlg_batch_columns(INSERT) on
    the same batch; one batch of 200 003 rows checked vectorised.

Row counts 1, 63, 64, 65, 150, 257 and 1 000: no multiple of 64 / 256, both sides of the wave and workgroup seams."""
import ctypes as C
import os

import numpy as np
import pytest

from etl_amd import abi
from tests import pgwire as W
from tests import scenarios as SC
from tests import table_copy_sinks as TC
from tests.test_gpu_iceberg import _read
from tests.test_gpu_rowbinary import NUMERICS, TIMETZS

pytestmark = pytest.mark.gpu
EMU = os.environ.get("ETLG_SIMT_RUN") == "1"
ASYNC = abi.F_ASYNC | abi.F_OUTPUT_ON_DEVICE
ROW_COUNTS = [1, 63, 64, 65, 150, 257, 1000]
ALL = list(SC.ALLTYPES)
ARROW_COLS = [c for c in ALL if c[0] not in ("u", "j", "arr")]          # what arrow_column_kinds accepts
ESCAPES = "tab\there\nline\\back\rcr\x08bs\x0cff\x0bvt é中 end"          # every COPY escape in a text
FLOATS_SLOW = ["0.1000000000000000055511151231257827021181583404541015625", "3.141592653589793238462643383279",
               "50537618.817359292015891086651596749e82", "107896223265412489690691363e88", "28879636596541978310003766487.741e-212"]


def _esc(v):
    """A cell's text as COPY's text format writes it (None / W.NULL: the NULL marker)."""
    if v is None or v is W.NULL:
        return "\\N"
    for a, b in (("\\", "\\\\"), ("\t", "\\t"), ("\n", "\\n"), ("\r", "\\r"), ("\x08", "\\b"), ("\x0c", "\\f"), ("\x0b", "\\v")):
        v = v.replace(a, b)
    return v


def _lines(rows):
    lines = [("\t".join(_esc(v) for v in r) + "\n").encode() for r in rows]
    return np.frombuffer(b"".join(lines), dtype=np.uint8), np.cumsum([0] + [len(x) for x in lines]).astype(np.uint32)


def _copy(cols, rows, flags=abi.F_OUTPUT_ON_DEVICE, model=True):
    """The rows as a table-copy batch on the oracle and on the device -> (materialised rows | None, host batch | None, batch, decoder)."""
    from etl_amd.decoder import Decoder
    from oracle import oracle
    buf, offs = _lines(rows)
    pk = [1 if c[3] else 0 for c in cols]
    d = Decoder(0)
    d.schema_put(42, 0, cols)
    sd = d.table_ready(42, 0, [1] * len(cols), pk)
    gb = d.copy_decode(sd, buf, offs, flags=flags)
    assert gb.rc == 0, gb.error
    if not model:
        return None, None, gb, d
    o = oracle.Oracle()
    o.schema_put(42, 0, cols)
    rb = o.copy_decode(o.table_ready(42, 0, [1] * len(cols), pk), buf, offs)
    assert rb.err_code == 0, rb.err_desc
    hb = rb.host_batch()
    cells = TC.copy_rows(hb.materialize(), 0)
    assert len(cells) == len(rows)
    return cells, hb, gb, d


NUMERICS_BQ = [x for x in NUMERICS if x not in ("1e-40", "-7e-100")]     # BigQuery refuses more than 38 decimal places (validation.rs:20-35)


def _alltypes(i, cols, wide_dates=True, bigquery=False):
    """Row i of the all-types table restricted to `cols`: the edge values first, then a cycle through the value lists. bigquery: rows that
    sink accepts — no NULL array element, no numeric of more than 38 decimal places."""
    names = [c[0] for c in cols]
    nums = NUMERICS_BQ if bigquery else NUMERICS
    if i == 0:
        r = SC.alltypes_row()
    elif i == 1:
        r = SC.alltypes_row(id="2", b="f", i2="-32768", i4="-2147483648", o="4294967295", d="0001-01-01" if wide_dates else "1900-01-01", t="00:00:00",
                            ts="1969-12-31 23:59:59.5", tstz="2026-01-02 03:04:05+02", f8="1e300", f4="-0.5", s="", by="\\x", j="[]", arr="{}")
    elif i == 2:
        r = SC.alltypes_row(id="-9223372036854775808", i2="32767", d="9999-12-31" if wide_dates else "2299-12-31", t="23:59:59.12", s="x" * 300,
                            by="\\x" + "ab" * 200, f8="-Infinity", f4="Infinity", o="0")
    elif i == 3:
        r = [("4" if c[0] == "id" else W.NULL) for c in ALL]                                       # a whole-NULL row (the key aside)
    elif i == 4:
        r = SC.alltypes_row(id="5", s=ESCAPES, i2="0", f8="0", f4="-0")
    else:
        r = SC.alltypes_row(id=str(10 + i), s="y" * (i * 13 % 200), t=f"01:02:{i % 60:02}.{i:06}", n=nums[i % len(nums)], tz=TIMETZS[i % len(TIMETZS)],
                            i2=str((i * 7919) % 65536 - 32768), o=str((i * 2654435761) % (1 << 32)), b="tf"[i % 2], by="\\x" + "%02x" % (i % 256) * (i % 9),
                            j='{"k":%d,"a":[1,2,{"z":null}]}' % i, arr="{%d,NULL}" % i)
        if i % 11 == 5:                                                                            # NULLs in every nullable column, one at a time
            k = (i // 11) % (len(ALL) - 1) + 1
            r[k] = W.NULL
    full = dict(zip([c[0] for c in ALL], r))
    if bigquery and full["arr"] is not W.NULL:
        full["arr"] = full["arr"].replace("NULL", "7")
    return [full[n] for n in names]


# ---------------------------------------------------------------- RowBinary and protobuf

def _rows_object(r, dev):
    n = r.n_rows
    offs = _read(r.view.row_offsets, 8 * (n + 1), dev).view(np.int64)
    data = _read(r.view.bytes, int(r.view.n_bytes), dev).tobytes()
    ev = _read(r.view.row_event, 8 * n, dev).view(np.uint64)
    return offs, data, ev


def _check_rows(r, want, dev):
    assert r.status == abi.RB_OK and r.n_rows == len(want) and int(r.view.n_host_rows) == 0 and r.view.on_device == (1 if dev else 0)
    offs, data, ev = _rows_object(r, dev)
    assert np.array_equal(ev, np.arange(len(want), dtype=np.uint64))                               # one row per source row
    lens = np.array([len(x) for x in want], dtype=np.int64)
    assert offs[0] == 0 and np.array_equal(np.diff(offs), lens), int(np.flatnonzero(np.diff(offs) != lens)[0])
    if data != b"".join(want):
        bad = [k for k in range(len(want)) if data[int(offs[k]):int(offs[k + 1])] != want[k]][0]
        raise AssertionError((bad, data[int(offs[bad]):int(offs[bad + 1])], want[bad]))
    r.close()


def _check_row_formats(cells, gb, nullable, engines=(abi.CH_MERGE_TREE, abi.CH_REPLACING_MERGE_TREE), protobuf=True):
    for dev in (False, True):
        for engine in engines:
            for cdc in ([0, 0], [1, 1]):
                if cdc[0] and (dev or engine == abi.CH_MERGE_TREE):
                    continue
                _check_rows(gb.rowbinary(0, nullable + cdc, engine, on_device=dev), TC.rowbinary_rows(cells, nullable + cdc, engine), dev)
        if protobuf:
            _check_rows(gb.protobuf(0, on_device=dev), TC.protobuf_rows(cells), dev)


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_row_formats_on_the_alltypes_table(n):
    """All of SC.ALLTYPES (json and array cells included). RowBinary takes dates of 1900..2299 only, so its batch has those at the
    edges and protobuf's has 0001-01-01 and 9999-12-31; the wider dates fail the RowBinary call at their row like a CDC batch's."""
    from etl_amd.decoder import EtlError
    nullable = [1 if c[2] else 0 for c in ALL]
    cells, hb, gb, d = _copy(ALL, [_alltypes(i, ALL, wide_dates=False) for i in range(n)])
    _check_row_formats(cells, gb, nullable, protobuf=False)
    gb.close(); d.close()
    cells, hb, gb, d = _copy(ALL, [_alltypes(i, ALL, bigquery=True) for i in range(n)])
    for dev in (False, True):
        _check_rows(gb.protobuf(0, on_device=dev), TC.protobuf_rows(cells), dev)
    if n > 1:
        with pytest.raises(EtlError) as ei:
            gb.rowbinary(0, nullable + [0, 0])
        assert ei.value.description == "Date out of ClickHouse Date32 range" and ei.value.frame_index == 1
    gb.close(); d.close()


SMALL = [("id", SC.INT8, False, 1), ("a", SC.INT4, True, 0), ("s", 25, True, 0), ("b", SC.BOOL, True, 0)]     # rows of about 30 bytes
BIG = [("id", SC.INT8, False, 1), ("s", 25, True, 0), ("n", SC.NUMERIC, True, 0), ("t", 25, True, 0), ("ts", SC.TIMESTAMPTZ, True, 0),
       ("by", SC.BYTEA, True, 0)]                                                                              # rows of about 500 bytes


@pytest.mark.parametrize("parts", [1, 2, 4])
@pytest.mark.parametrize("size", ["small", "big"])
def test_row_formats_under_every_split_of_a_row(parts, size, monkeypatch):
    """ETLG_RB_PARTS lanes per row: the counting pass and the byte pass must agree on the shorter tail wherever a lane starts in the
    middle of a row. 257 rows: two workgroups at every split; small rows go through the staged LDS image, 500-byte rows directly."""
    monkeypatch.setenv("ETLG_RB_PARTS", str(parts))
    if size == "small":
        cols = SMALL
        rows = [[str(i), W.NULL if i % 7 == 3 else str(i * 3 - 50), W.NULL if i % 5 == 1 else "t%d" % i, W.NULL if i % 3 == 2 else "tf"[i % 2]] for i in range(257)]
    else:
        cols = BIG
        rows = [[str(i), "s" * (180 + i % 90), NUMERICS_BQ[i % len(NUMERICS_BQ)], W.NULL if i % 6 == 2 else ESCAPES * 2 + "x" * (i % 60),
                 "2026-01-02 03:04:05.%06d+00" % i, "\\x" + "c3" * (40 + i % 50)] for i in range(257)]
    cells, hb, gb, d = _copy(cols, rows)
    want = TC.protobuf_rows(cells)
    avg = sum(len(x) for x in want) / len(want)
    assert (avg < 40) if size == "small" else (400 < avg < 600), avg
    _check_row_formats(cells, gb, [1 if c[2] else 0 for c in cols])
    gb.close(); d.close()


def test_replacing_merge_tree_version_of_every_copied_row_is_zero():
    """Must fail without the copy tail: the virtual transaction's ordinals count up from 0, so row 1 and later carried a version."""
    cells, hb, gb, d = _copy(SMALL, [[str(i), str(i), "x", "t"] for i in range(65)])
    r = gb.rowbinary(0, [0, 1, 1, 1, 0, 0], abi.CH_REPLACING_MERGE_TREE)
    offs, data = r.row_offsets(), r.bytes().tobytes()
    for k in range(65):
        assert data[int(offs[k + 1]) - 17:int(offs[k + 1])] == bytes(17), k                       # UInt128 0 + UInt8 0
    r.close()
    r = gb.rowbinary(0, [0, 1, 1, 1, 0, 0], abi.CH_MERGE_TREE)
    offs, data = r.row_offsets(), r.bytes().tobytes()
    assert all(data[int(offs[k + 1]) - 15:int(offs[k + 1])] == b"\x06INSERT" + bytes(8) for k in range(65))
    r.close(); gb.close(); d.close()


def test_protobuf_copy_row_ends_with_the_upsert_field():
    """Must fail without the copy tail: a copied row has no _CHANGE_SEQUENCE_NUMBER field, so n_bytes is smaller than the CDC form's by
    that field — tag n + 2, length 50."""
    from oracle import protobuf as PB
    n = 65
    cells, hb, gb, d = _copy(SMALL, [[str(i), str(i), "x", "t"] for i in range(n)])
    r = gb.protobuf(0)
    offs, data = r.row_offsets(), r.bytes().tobytes()
    tail = PB.ld(len(SMALL) + 1, b"UPSERT")
    assert all(data[int(offs[k]):int(offs[k + 1])].endswith(tail) for k in range(n))
    cdc_bytes = sum(len(x) for x in TC.protobuf_rows(cells)) + n * len(PB.ld(len(SMALL) + 2, b"0" * 50))
    assert int(r.view.n_bytes) == cdc_bytes - n * 52
    r.close(); gb.close(); d.close()


def test_row_format_errors_at_their_row():
    from etl_amd.decoder import EtlError
    cols = [("id", SC.INT8, False, 1), ("s", 25, True, 0), ("n", SC.NUMERIC, True, 0), ("j", SC.JSONB, True, 0)]
    rows = [[str(i), "t%d" % i, "1.5", '{"a":%d}' % i] for i in range(150)]
    bad_null, bad_scale, bad_json = 70, 131, 140
    rows[bad_null][1] = W.NULL
    rows[bad_scale][2] = "0." + "0" * 38 + "1"                                                     # 39 decimal places
    cells, hb, gb, d = _copy(cols, rows)
    with pytest.raises(EtlError) as ei:                                                            # NULL in a non-nullable destination column
        gb.rowbinary(0, [0, 0, 1, 1, 0, 0])
    assert (ei.value.kind, ei.value.description, ei.value.frame_index) == (abi.ConversionError, "NULL value for non-nullable ClickHouse column", bad_null)
    with pytest.raises(EtlError) as ei:
        gb.rowbinary(0, [0, 1, 1, 1, 0])
    assert ei.value.description == "ClickHouse RowBinary row width mismatch"
    with pytest.raises(EtlError) as ei:                                                            # numeric scale > 38
        gb.protobuf(0)
    assert (ei.value.kind, ei.value.detail, ei.value.frame_index) == (abi.UnsupportedValueInDestination, "Cell at index 2 failed validation", bad_scale)
    _check_rows(gb.rowbinary(0, [0, 1, 1, 1, 0, 0]), TC.rowbinary_rows(cells, [0, 1, 1, 1, 0, 0], 0), False)   # (ClickHouse takes that numeric)
    gb.close(); d.close()
    rows[bad_json][3] = "{bad"                                                                     # not JSON: the decode error, before everything else
    cells, hb, gb, d = _copy(cols, rows, model=False)
    for call in (lambda: gb.rowbinary(0, [0, 0, 1, 1, 0, 0]), lambda: gb.protobuf(0)):
        with pytest.raises(EtlError) as ei:
            call()
        assert (ei.value.code, ei.value.description, ei.value.frame_index) == (abi.E_JSON, "JSON deserialization failed", bad_json)
    gb.close(); d.close()


# ---------------------------------------------------------------- the Arrow form

def _padded_bits(bits):
    n = len(bits)
    out = np.zeros((n + 63) // 64 * 8, np.uint8)
    packed = np.packbits(np.asarray(bits, bool), bitorder="little")
    out[:len(packed)] = packed
    return out


def _check_arrow(cells, type_classes, nullable, c, dev):
    n = len(cells)
    kinds, cols = TC.arrow_columns(cells, type_classes)
    assert (int(c.ducklake.status), c.n_rows, c.view.n_cols, c.view.on_device) == (abi.DLC_OK, n, len(kinds), 1 if dev else 0)
    assert np.array_equal(_read(c.view.row_event, 8 * n, dev).view(np.uint64), np.arange(n, dtype=np.uint64))
    bm = (n + 63) // 64 * 8
    for i, (kind, m) in enumerate(zip(kinds, cols)):
        k = c.column(i)
        col_cells = [r[i] for r in cells]
        width = 0 if kind in TC.VAR or kind == abi.AK_BOOLEAN else TC.FIXED[kind][0]
        assert (k.type_class, k.arrow_kind, k.value_bytes, k.nullable) == (type_classes[i], kind, width, nullable[i]), i
        valid, deferred = m[0], TC.deferred_bits(col_cells)
        assert (int(k.null_count), int(k.deferred_count)) == (int((~valid).sum()), int(deferred.sum())), i
        assert np.array_equal(_read(k.validity, bm, dev), _padded_bits(valid)), i
        assert np.array_equal(_read(k.deferred, bm, dev), _padded_bits(deferred)), i
        if kind in TC.VAR:
            offs = _read(k.offsets, 4 * (n + 1), dev).view(np.int32)                               # int32 offsets
            assert offs[0] == 0 and int(offs[n]) == int(k.values_bytes) == len(m[2]), i
            assert np.array_equal(offs, m[1]), (i, int(np.flatnonzero(offs != m[1])[0]))
            assert _read(k.values, int(k.values_bytes), dev).tobytes() == m[2], i
        elif kind == abi.AK_BOOLEAN:
            assert not k.offsets and int(k.values_bytes) == bm
            assert np.array_equal(_read(k.values, bm, dev), _padded_bits(m[1])), i                 # bit-packed
        else:
            assert not k.offsets and int(k.values_bytes) == n * width
            got = _read(k.values, n * width, dev).view(TC.FIXED[kind][1])
            assert np.array_equal(got, m[1]), (i, int(np.flatnonzero(got != m[1])[0]))             # null slots are zero


def _arrow_both(cells, hb, gb):
    tcs, nullable = [c.type_class for c in hb.slots[0].cols], [c.nullable for c in hb.slots[0].cols]
    for dev in (False, True):
        c = gb.ducklake_copy(0, on_device=dev)
        _check_arrow(cells, tcs, nullable, c, dev)
        c.close()


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_arrow_form_of_the_alltypes_table(n):
    cells, hb, gb, d = _copy(ARROW_COLS, [_alltypes(i, ARROW_COLS) for i in range(n)])
    _arrow_both(cells, hb, gb)
    c = gb.ducklake_copy(0)
    names = [x[0] for x in ARROW_COLS]
    want = {"id": (abi.AK_INT64, 8), "b": (abi.AK_BOOLEAN, 0), "i2": (abi.AK_INT16, 2), "i4": (abi.AK_INT32, 4), "o": (abi.AK_UINT64, 8),
            "n": (abi.AK_UTF8, 0), "by": (abi.AK_BINARY, 0), "d": (abi.AK_DATE32, 4), "t": (abi.AK_TIME64_US, 8), "tz": (abi.AK_UTF8, 0),
            "ts": (abi.AK_TIMESTAMP_US, 8), "tstz": (abi.AK_TIMESTAMP_US_UTC, 8), "f8": (abi.AK_FLOAT64, 8), "f4": (abi.AK_FLOAT32, 4), "s": (abi.AK_UTF8, 0)}
    assert [(c.column(i).arrow_kind, c.column(i).value_bytes) for i in range(len(names))] == [want[x] for x in names]
    if n >= 63:
        i2 = c.host_arrays(names.index("i2"))[2].view(np.int16)
        oid = c.host_arrays(names.index("o"))[2].view(np.uint64)
        dates = c.host_arrays(names.index("d"))[2].view(np.int32)
        assert (int(i2[1]), int(i2[2]), int(i2[3])) == (-32768, 32767, 0) and (int(oid[1]), int(oid[3])) == (4294967295, 0)
        assert (int(dates[1]), int(dates[2])) == (-719162, 2932896)                                # 0001-01-01, 9999-12-31
    c.close(); gb.close(); d.close()


def test_deferred_floats_without_and_with_finish_cells():
    cols = [("id", SC.INT8, False, 1), ("x", SC.FLOAT8, True, 0), ("y", SC.FLOAT4, True, 0)]
    rows = [[str(i), FLOATS_SLOW[i % len(FLOATS_SLOW)] if i % 3 else "2.5", "1.5"] for i in range(150)]
    cells, hb, gb, d = _copy(cols, rows)
    _arrow_both(cells, hb, gb)
    c = gb.ducklake_copy(0)
    assert int(c.column(1).deferred_count) > 0 and int(c.column(1).deferred_count) == int(c.column(1).null_count)
    c.close(); gb.close(); d.close()
    _, _, gb, d = _copy(cols, rows, flags=abi.F_OUTPUT_ON_DEVICE | abi.F_FINISH_CELLS, model=False)
    c = gb.ducklake_copy(0)
    assert [int(c.column(i).deferred_count) for i in range(3)] == [0, 0, 0] and [int(c.column(i).null_count) for i in range(3)] == [0, 0, 0]
    assert np.array_equal(c.host_arrays(1)[2].view(np.float64), np.array([float(r[1]) for r in rows]))         # (Python's float() rounds correctly)
    assert not c.host_arrays(1)[1].any()
    c.close(); gb.close(); d.close()


@pytest.mark.parametrize("what", ["uuid", "json", "array"])
def test_a_table_without_an_arrow_form(what):
    oid = {"uuid": SC.UUID, "json": 114, "array": SC.INT4_A}[what]
    text = {"uuid": "123e4567-e89b-12d3-a456-426614174000", "json": '{"id":1}', "array": "{1,NULL}"}[what]
    cols = [("id", SC.INT4, False, 1), ("s", 25, True, 0), ("v", oid, True, 0), ("w", SC.JSONB, True, 0)]
    _, _, gb, d = _copy(cols, [[str(i), "x", text, "[]"] for i in range(65)], model=False)
    for dev in (False, True):
        c = gb.ducklake_copy(0, on_device=dev)
        assert (int(c.ducklake.status), int(c.ducklake.column), c.n_rows, c.view.n_cols) == (abi.DLC_NOT_ARROW, 2, 0, 0)
        c.close()
    gb.close(); d.close()


def test_offsets_overflow_under_a_lowered_cap(monkeypatch):
    cols = [("id", SC.INT4, False, 1), ("a", 25, True, 0), ("t", 25, True, 0)]
    rows = [[str(i), "ab", "%040d" % i] for i in range(257)]                                       # 257 x 40 = 10 280 bytes in column 2
    monkeypatch.setenv("ETLG_DLC_OFFSET_CAP", "4096")
    cells, hb, gb, d = _copy(cols, rows)
    for dev in (False, True):
        c = gb.ducklake_copy(0, on_device=dev)
        assert (int(c.ducklake.status), int(c.ducklake.column), c.n_rows, c.view.n_cols) == (abi.DLC_OFFSETS_OVERFLOW, 2, 0, 0)
        c.close()
    gb.close(); d.close()
    monkeypatch.setenv("ETLG_DLC_OFFSET_CAP", str(257 * 40 + 1))                                   # one byte under the cap: the columns
    cells, hb, gb, d = _copy(cols, rows)
    _arrow_both(cells, hb, gb)
    gb.close(); d.close()
    monkeypatch.setenv("ETLG_DLC_OFFSET_CAP", str(257 * 40 - 1))                                   # one byte over
    _, _, gb, d = _copy(cols, rows, model=False)
    c = gb.ducklake_copy(0)
    assert (int(c.ducklake.status), int(c.ducklake.column)) == (abi.DLC_OFFSETS_OVERFLOW, 2)
    c.close(); gb.close(); d.close()


def test_arguments_and_other_objects():
    from etl_amd.decoder import EtlError
    from tests.test_gpu_rowbinary import _both, _stream
    buf, offs = _stream([W.insert(42, ["1", "x"])])
    hb, b, d = _both(SC.simple_table(SC.COLS2), buf, offs)                                         # a WAL batch
    with pytest.raises(EtlError) as ei:
        b.ducklake_copy(0)
    assert ei.value.kind == abi.InvalidArgument
    out = C.c_void_p()
    assert d.L.etlg_batch_ducklake_copy(d.h, b.h, 0, 0, C.byref(out)) == abi.InvalidArgument and not out
    plain = b.columns(0)
    info = abi.DuckLakeCopyInfo()
    assert d.L.etlg_columns_ducklake_get(plain.h, C.byref(info)) == abi.InvalidArgument           # an etlg_batch_columns object
    ice = b.iceberg(0)
    assert d.L.etlg_columns_ducklake_get(ice.h, C.byref(info)) == abi.InvalidArgument
    assert d.L.etlg_columns_ducklake_get(None, C.byref(info)) == abi.InvalidArgument
    plain.close(); ice.close(); b.close(); d.close()
    cells, hb, gb, d = _copy(SMALL, [["1", "2", "x", "t"]])
    c = gb.ducklake_copy(0)
    assert d.L.etlg_columns_ducklake_get(c.h, None) == abi.InvalidArgument
    assert d.L.etlg_columns_ducklake_get(c.h, C.byref(info)) == abi.OK and info.status == abi.DLC_OK
    assert d.L.etlg_columns_changelog_get(c.h, C.byref(abi.ChangelogInfo())) == abi.InvalidArgument
    with pytest.raises(Exception):
        gb.ducklake_copy(7)                                                                        # no such slot
    c.close()
    gb.host()                                                                                      # downloaded: the arena left the device
    with pytest.raises(EtlError) as ei:
        gb.ducklake_copy(0)
    assert ei.value.kind == abi.InvalidState
    gb.close(); d.close()


def test_async_copy_batch():
    rows = [_alltypes(i, ARROW_COLS) for i in range(150)]
    cells, hb, gb, d = _copy(ARROW_COLS, rows, flags=ASYNC)                                        # (the call syncs the pending batch itself)
    _arrow_both(cells, hb, gb)
    gb.close(); d.close()
    cells, hb, gb, d = _copy(SMALL, [[str(i), str(i), "x", "t"] for i in range(150)], flags=ASYNC)
    _check_rows(gb.rowbinary(0, [0, 1, 1, 1, 0, 0], abi.CH_REPLACING_MERGE_TREE), TC.rowbinary_rows(cells, [0, 1, 1, 1, 0, 0], 1), False)
    gb.close(); d.close()


@pytest.mark.parametrize("n", [65, 257])
def test_against_etlg_batch_columns_on_the_same_batch(n):
    """Every column whose kind did not change is buffer-equal; a Utf8 / Binary column has the same bytes and its int32 offsets equal the
    int64 ones; int2 / oid columns hold the same numbers; and etlg_batch_columns gives afterwards what it gave before."""
    cells, hb, gb, d = _copy(ARROW_COLS, [_alltypes(i, ARROW_COLS) for i in range(n)])

    def buffers(c):
        out = [c.row_event().tobytes()]
        for i in range(len(ARROW_COLS)):
            k = c.column(i)
            v, df, vals, offsets = c.host_arrays(i)
            out.append((k.type_class, k.arrow_kind, k.value_bytes, k.nullable, int(k.null_count), int(k.deferred_count), int(k.values_bytes),
                        v.tobytes(), df.tobytes(), vals.tobytes(), None if offsets is None else offsets.tobytes()))
        return out
    before = gb.columns(0)
    want = buffers(before)
    dl = gb.ducklake_copy(0)
    got = buffers(dl)
    assert got[0] == want[0]
    changed = {abi.AK_INT16: abi.AK_INT32, abi.AK_UINT64: abi.AK_INT64, abi.AK_UTF8: abi.AK_LARGE_UTF8, abi.AK_BINARY: abi.AK_LARGE_BINARY}
    seen = set()
    for i in range(len(ARROW_COLS)):
        g, w = got[i + 1], want[i + 1]
        if g[1] not in changed:
            assert g == w, i
            continue
        seen.add(g[1])
        assert w[1] == changed[g[1]] and (g[0], g[3], g[4], g[5], g[7], g[8]) == (w[0], w[3], w[4], w[5], w[7], w[8]), i
        if g[1] in TC.VAR:
            assert g[6] == w[6] and g[9] == w[9], i
            assert np.array_equal(np.frombuffer(g[10], np.int32).astype(np.int64), np.frombuffer(w[10], np.int64)), i
        elif g[1] == abi.AK_INT16:
            assert np.array_equal(np.frombuffer(g[9], np.int16).astype(np.int32), np.frombuffer(w[9], np.int32)), i
        else:
            assert np.array_equal(np.frombuffer(g[9], np.uint64), np.frombuffer(w[9], np.int64).view(np.uint64)), i
    assert seen == set(changed)
    after = gb.columns(0)
    assert buffers(after) == want and after.ducklake is None
    for c in (before, dl, after):
        c.close()
    gb.close(); d.close()


def test_full_size_batch():
    """200 003 copied rows (the emulator runs the same kernels over fewer): every buffer of the Arrow form and the protobuf / RowBinary
    tails, checked vectorised in numpy."""
    n = 3001 if EMU else 200_003
    cols = [("id", SC.INT4, False, 1), ("t", 25, True, 0), ("n", SC.NUMERIC, True, 0), ("i2", SC.INT2, True, 0), ("o", SC.OID, True, 0),
            ("by", SC.BYTEA, True, 0)]
    idx = np.arange(n)
    i2 = (idx * 7919 % 65536 - 32768).astype(np.int64)
    oid = (idx.astype(np.uint64) * np.uint64(2654435761)) % np.uint64(1 << 32)
    i2l, oidl = i2.tolist(), oid.tolist()
    texts = [b"text-%d" % i if i % 9 else None for i in range(n)]
    nums = [b"%d.%02d" % (i, i % 100) for i in range(n)]
    lines = [b"%d\t%s\t%s\t%d\t%d\t\\\\x%s\n" % (i, texts[i] if texts[i] is not None else b"\\N", nums[i], i2l[i], oidl[i], b"%02x" % (i % 256) * (i % 5)) for i in range(n)]
    buf = np.frombuffer(b"".join(lines), dtype=np.uint8)
    offs = np.cumsum([0] + [len(x) for x in lines]).astype(np.uint32)
    from etl_amd.decoder import Decoder
    d = Decoder(0)
    d.schema_put(42, 0, cols)
    sd = d.table_ready(42, 0, [1] * len(cols), [1, 0, 0, 0, 0, 0])
    gb = d.copy_decode(sd, buf, offs, flags=abi.F_OUTPUT_ON_DEVICE)
    assert gb.rc == 0, gb.error
    c = gb.ducklake_copy(0)
    assert c.n_rows == n and n % 64 != 0 and n % 256 != 0 and int(c.ducklake.status) == abi.DLC_OK
    assert [c.column(i).arrow_kind for i in range(6)] == [abi.AK_INT32, abi.AK_UTF8, abi.AK_UTF8, abi.AK_INT16, abi.AK_UINT64, abi.AK_BINARY]
    assert np.array_equal(c.row_event(), idx.astype(np.uint64))
    assert np.array_equal(c.host_arrays(0)[2].view(np.int32), idx.astype(np.int32))
    assert np.array_equal(c.host_arrays(3)[2].view(np.int16), i2.astype(np.int16))
    assert np.array_equal(c.host_arrays(4)[2].view(np.uint64), oid)
    ones = _padded_bits(np.ones(n, bool))
    for i, parts in ((1, [t or b"" for t in texts]), (2, nums), (5, [bytes([k % 256]) * (k % 5) for k in range(n)])):
        v, df, vals, o = c.host_arrays(i)
        want_o = np.zeros(n + 1, np.int64)
        np.cumsum([len(p) for p in parts], out=want_o[1:])
        assert o.dtype == np.int32 and np.array_equal(o, want_o.astype(np.int32)) and int(c.column(i).values_bytes) == int(want_o[n])
        assert vals.tobytes() == b"".join(parts)
        assert np.array_equal(v, _padded_bits(idx % 9 != 0) if i == 1 else ones) and not df.any()
    assert int(c.column(1).null_count) == int((idx % 9 == 0).sum())
    c.close()
    # the two row formats' tails on the same batch: 17 zero bytes / the UPSERT field and nothing behind it
    r = gb.rowbinary(0, [0, 1, 1, 1, 1, 1, 0, 0], abi.CH_REPLACING_MERGE_TREE)
    o, data = r.row_offsets(), r.bytes()
    assert r.n_rows == n and np.array_equal(r.row_event(), idx.astype(np.uint64))
    ends = o[1:, None] - np.arange(17, 0, -1)[None, :]
    assert not data[ends].any()
    assert np.array_equal(data[o[:-1, None] + np.arange(4)[None, :]].copy().view(np.int32).ravel(), idx.astype(np.int32))      # the id opens every row
    r.close()
    r = gb.protobuf(0)
    o, data = r.row_offsets(), r.bytes()
    tail = np.frombuffer(bytes([(7 << 3) | 2, 6]) + b"UPSERT", np.uint8)
    ends = o[1:, None] - np.arange(8, 0, -1)[None, :]
    assert r.n_rows == n and np.array_equal(data[ends], np.broadcast_to(tail, (n, 8)))
    r.close(); gb.close(); d.close()
