"""tests/table_copy_sinks.py — the host model tests/test_gpu_copy_sinks.py holds the device to — against the reference's own vectors
(tests/golden/ducklake_copy_kats.py, transcribed with their file:line): the DuckLake kind table row by row, the reference's tests of
prepare_copy_rows, ClickHouse's zero LSN / ordinal and BigQuery's single trailing field. CPU only."""
import numpy as np

from etl_amd import abi
from oracle import oracle
from oracle import protobuf as PB
from oracle import rowbinary as RB
from tests import table_copy_sinks as TC
from tests.golden import ducklake_copy_kats as K

KIND_OF = {"Bool": abi.AK_BOOLEAN, "I16": abi.AK_INT16, "I32": abi.AK_INT32, "I64": abi.AK_INT64, "U64": abi.AK_UINT64, "F32": abi.AK_FLOAT32,
           "F64": abi.AK_FLOAT64, "Utf8": abi.AK_UTF8, "Date32": abi.AK_DATE32, "Time64Microsecond": abi.AK_TIME64_US,
           "TimestampMicrosecond": abi.AK_TIMESTAMP_US, "TimestampTzMicrosecond": abi.AK_TIMESTAMP_US_UTC, "Binary": abi.AK_BINARY}
DATA_TYPE_OF = {"Int32": abi.AK_INT32, "Utf8": abi.AK_UTF8, "Timestamp(us)": abi.AK_TIMESTAMP_US}


# the value codec's class of every oid of the kind table (include/etlg.h etlg_type_class_of_oid), stated here so that the test needs no library
CLASS_OF_OID = {16: abi.TC_BOOL, 21: abi.TC_I16, 23: abi.TC_I32, 20: abi.TC_I64, 26: abi.TC_U32, 700: abi.TC_F32, 701: abi.TC_F64,
                1082: abi.TC_DATE, 1083: abi.TC_TIME, 1114: abi.TC_TIMESTAMP, 1184: abi.TC_TIMESTAMPTZ, 17: abi.TC_BYTEA, 2950: abi.TC_UUID,
                114: abi.TC_JSON, 3802: abi.TC_JSON, 25: abi.TC_STRING, 1043: abi.TC_STRING, 1700: abi.TC_NUMERIC, 1266: abi.TC_TIMETZ,
                1007: abi.TC_ARRAY, 1009: abi.TC_ARRAY}


def test_the_kind_table_row_by_row():
    assert len(K.KIND_TABLE) == 21
    for line, name, oid, kind in K.KIND_TABLE:
        kinds, bad = TC.arrow_kinds([CLASS_OF_OID[oid]])
        if kind is None:
            assert kinds is None and bad == 0, (line, name)
        else:
            assert kinds == [KIND_OF[kind]] and bad is None, (line, name)
            dt, width, obits = K.DATA_TYPES[kind]
            if width is not None:
                assert TC.FIXED[kinds[0]][0] == width, (line, name)
            if obits is not None:
                assert kinds[0] in TC.VAR and obits == 32
    assert set(KIND_OF) == set(K.DATA_TYPES)
    assert {"Int16", "UInt64", "Utf8", "Binary"} <= {v[0] for v in K.DATA_TYPES.values()}          # not Int32 / Int64 / LargeUtf8 / LargeBinary


def _decode_copy(cols, rows):
    """The oracle's table-copy decode of `rows` (texts, None = NULL) -> materialised cells per row."""
    o = oracle.Oracle()
    o.schema_put(42, 0, [(n, oid, nullable, 1 if i == 0 else 0) for i, (n, oid, nullable) in enumerate(cols)])
    slot = o.table_ready(42, 0, [1] * len(cols), [1] + [0] * (len(cols) - 1))
    lines = [("\t".join("\\N" if v is None else v for v in r) + "\n").encode() for r in rows]
    buf = np.frombuffer(b"".join(lines), dtype=np.uint8)
    offs = np.cumsum([0] + [len(x) for x in lines]).astype(np.uint32)
    rb = o.copy_decode(slot, buf, offs)
    assert rb.err_code == 0, rb.err_desc
    hb = rb.host_batch()
    return hb, TC.copy_rows(hb.materialize(), 0)


def test_the_references_arrow_table():
    t = K.ARROW_TABLE
    hb, rows = _decode_copy(t["cols"], t["rows"])
    kinds, cols = TC.arrow_columns(rows, [c.type_class for c in hb.slots[0].cols])
    assert len(rows) == t["num_rows"] and len(cols) == t["num_columns"]
    assert kinds == [DATA_TYPE_OF[d] for d in t["data_types"]]
    v, vals = cols[0]
    assert v.all() and vals.dtype == np.int32 and vals.tolist() == t["values"][0]
    v, offs, data = cols[1]
    assert v.tolist() == [True, False] and offs.dtype == np.int32 and offs.tolist() == [0, 5, 5] and data == b"alice"
    v, vals = cols[2]
    assert v.tolist() == [True, False] and vals.dtype == np.int64 and vals.tolist() == [t["values"][2][0], 0]      # the null slot is zero


def test_the_fallbacks():
    for lines, cols, bad_col, _payload in K.FALLBACKS:
        kinds, bad = TC.arrow_kinds([CLASS_OF_OID[oid] for _, oid, _ in cols])
        assert kinds is None and bad == bad_col, lines


def test_clickhouse_copy_tail_is_insert_with_zero_lsn_and_ordinal():
    k = K.CLICKHOUSE_COPY_CDC
    assert (k["operation"], k["commit_lsn"], k["tx_ordinal"]) == ("INSERT", 0, 0)
    hb, rows = _decode_copy([("id", 20, False), ("s", 25, True)], [["1", "x"], ["2", None], ["3", "y"]])
    for engine, tail in ((RB.MERGE_TREE, k["merge_tree"]), (RB.REPLACING_MERGE_TREE, k["replacing_merge_tree"])):
        assert RB.cdc_columns("I", 0, 0, engine) == tail
        out = TC.rowbinary_rows(rows, [0, 1, 0, 0], engine)
        assert len(out) == 3 and all(r.endswith(tail) for r in out)
        assert out[1] == RB.row(rows[1], [0, 1]) + tail and out[1][:9] == (2).to_bytes(8, "little") + b"\x01"
        # Nullable() CDC columns take their marker bytes, as for CDC rows
        marked = TC.rowbinary_rows(rows, [0, 1, 1, 1], engine)
        assert all(len(m) == len(r) + 2 for m, r in zip(marked, out))


def test_bigquery_copy_row_has_one_trailing_field():
    k = K.BIGQUERY_COPY_TRAILING
    assert k["cells"] == [TC.UPSERT.decode()]
    hb, rows = _decode_copy([("id", 20, False), ("s", 25, True)], [["1", "x"], ["2", None]])
    out = TC.protobuf_rows(rows)
    n = 2
    trailing = PB.ld(n + 1, b"UPSERT")
    assert out[0] == PB.cell(rows[0][0], 1) + PB.cell(rows[0][1], 2) + trailing
    assert out[1] == PB.cell(rows[1][0], 1) + trailing                       # Cell::Null leaves nothing
    ev = [e for e in hb.materialize() if e["kind"] == "I"]
    cdc = PB.upsert_row(ev[0], ev[0]["row"], 0)                              # the CDC form: both fields
    assert cdc.startswith(out[0]) and len(cdc) - len(out[0]) == len(PB.ld(n + 2, b"0" * 50))
    assert PB.key(n + 2, 2) not in out[0][-len(trailing):]
