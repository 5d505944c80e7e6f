"""TEST INFRASTRUCTURE — a small host model of what the ClickHouse, BigQuery and DuckLake sinks write for a TABLE-COPY batch
(write_table_rows), built from `HostBatch.materialize()` — the reference's value model — and not from arena offsets. Pinned to the
reference's own vectors by tests/test_table_copy_sink_kats.py; tests/test_gpu_copy_sinks.py holds etlg_batch_rowbinary /
etlg_batch_protobuf on a copy batch and etlg_batch_ducklake_copy against it.

  ClickHouse (write_table_rows_inner, crates/etl-destinations/src/clickhouse/core.rs:739-773): every row's cells as for an Insert,
    then append_cdc_columns(Insert, PgLsn 0, tx_ordinal 0, engine).
  BigQuery (write_table_rows, bigquery/core.rs:602-649): every row's cells under tags 1..n, then _CHANGE_TYPE = "UPSERT" under n + 1 —
    and no _CHANGE_SEQUENCE_NUMBER field (compare bigquery_upsert_row :1410-1418, which pushes both).
  DuckLake (prepare_copy_rows, ducklake/encoding.rs:32-49): for a table arrow_column_kinds (:229-257) accepts, an Arrow RecordBatch
    (copy_rows_to_arrow_record_batch :303-340) — Int16 for int2, UInt64 for oid, Utf8 / Binary with 32-bit offsets, null slots zero
    (arrow's From<Vec<Option<T>>>).

An Arrow column of the model is (validity bool[n], values) with values a numpy array of the kind's dtype (Boolean: bool[n], to be
bit-packed by the reader), or (validity, int32 offsets[n + 1], bytes) for Utf8 / Binary."""
import numpy as np

from etl_amd import abi
from oracle import display as D
from oracle import protobuf as PB
from oracle import rowbinary as RB

CE_DAYS_1970 = 719163
UPSERT = b"UPSERT"                                   # BigQueryOperationType::Upsert (bigquery/core.rs:611-614)

# arrow_column_kind (ducklake/encoding.rs:236-257) by type class; a class that is not here has no Arrow form (`None`)
ARROW_KINDS = {
    abi.TC_BOOL: abi.AK_BOOLEAN, abi.TC_I16: abi.AK_INT16, abi.TC_I32: abi.AK_INT32, abi.TC_I64: abi.AK_INT64, abi.TC_U32: abi.AK_UINT64,
    abi.TC_F32: abi.AK_FLOAT32, abi.TC_F64: abi.AK_FLOAT64, abi.TC_DATE: abi.AK_DATE32, abi.TC_TIME: abi.AK_TIME64_US,
    abi.TC_TIMESTAMP: abi.AK_TIMESTAMP_US, abi.TC_TIMESTAMPTZ: abi.AK_TIMESTAMP_US_UTC, abi.TC_BYTEA: abi.AK_BINARY,
    abi.TC_STRING: abi.AK_UTF8, abi.TC_NUMERIC: abi.AK_UTF8, abi.TC_TIMETZ: abi.AK_UTF8,
}
NOT_ARROW = (abi.TC_UUID, abi.TC_JSON, abi.TC_ARRAY)
# (bytes per value, numpy dtype) of the fixed-width kinds; Boolean is bit-packed
FIXED = {abi.AK_INT16: (2, np.int16), abi.AK_INT32: (4, np.int32), abi.AK_INT64: (8, np.int64), abi.AK_UINT64: (8, np.uint64),
         abi.AK_FLOAT32: (4, np.uint32), abi.AK_FLOAT64: (8, np.uint64), abi.AK_DATE32: (4, np.int32), abi.AK_TIME64_US: (8, np.int64),
         abi.AK_TIMESTAMP_US: (8, np.int64), abi.AK_TIMESTAMP_US_UTC: (8, np.int64)}
VAR = (abi.AK_UTF8, abi.AK_BINARY)


def copy_rows(events, slot_index):
    """The cells of every row of a materialised table-copy batch, in row order (every event of it is an Insert)."""
    return [e["row"] for e in events if e["kind"] == "I" and e.get("schema_slot") == slot_index]


def rowbinary_rows(rows, nullable_flags, engine):
    """RowBinary bytes per copied row; nullable_flags: the data columns' and then the two CDC columns' (rb_encode_nullable)."""
    n = len(nullable_flags) - 2
    tail = RB.cdc_columns("I", 0, 0, engine)
    if engine == RB.MERGE_TREE:                       # String, UInt64
        op, lsn = tail[:7], tail[7:]
    else:                                             # UInt128, UInt8
        op, lsn = tail[:16], tail[16:]
    tail = (b"\x00" if nullable_flags[n] else b"") + op + (b"\x00" if nullable_flags[n + 1] else b"") + lsn
    return [RB.row(cells, list(nullable_flags[:n])) + tail for cells in rows]


def protobuf_rows(rows):
    """protobuf bytes per copied row: the cells under tags 1..n, then the single trailing field."""
    return [b"".join(PB.cell(c, i + 1) for i, c in enumerate(cells)) + PB.ld(len(cells) + 1, UPSERT) for cells in rows]


def arrow_kinds(type_classes):
    """(kinds, None) — or (None, index of the first column without an Arrow form): arrow_column_kinds."""
    for i, tc in enumerate(type_classes):
        if tc in NOT_ARROW:
            return None, i
    return [ARROW_KINDS[tc] for tc in type_classes], None


def _string(c):
    k = c[0]
    if k == "Numeric":
        return D.numeric_string(*c[1:]).encode()
    if k == "TimeTz":
        return D.timetz_string(*c[1:]).encode()
    assert k in ("String", "Bytes"), c
    return bytes(c[1])


def _fixed(c):
    k = c[0]
    if k in ("Bool", "I16", "I32", "I64", "U32", "F32", "F64"):     # (floats: materialize() keeps the bits)
        return int(c[1])
    if k == "Date":
        return c[1] - CE_DAYS_1970
    if k == "Time":
        return c[1] * 1_000_000 + c[2] // 1000
    if k in ("Timestamp", "TimestampTz"):
        return ((c[1] - CE_DAYS_1970) * 86400 + c[2]) * 1_000_000 + c[3] // 1000
    raise AssertionError(c)


def arrow_column(cells, kind):
    """One column's cells -> (validity, values) / (validity, offsets, bytes); a Deferred cell is null (and set in `deferred` by the device)."""
    valid = np.array([c[0] not in ("Null", "Deferred") for c in cells], dtype=bool)
    if kind in VAR:
        parts = [_string(c) if ok else b"" for c, ok in zip(cells, valid)]
        offs = np.zeros(len(cells) + 1, dtype=np.int64)
        np.cumsum([len(p) for p in parts], out=offs[1:])
        assert int(offs[-1]) <= 2**31 - 1
        return valid, offs.astype(np.int32), b"".join(parts)
    if kind == abi.AK_BOOLEAN:
        return valid, np.array([bool(c[1]) if ok else False for c, ok in zip(cells, valid)], dtype=bool)
    vals = [_fixed(c) if ok else 0 for c, ok in zip(cells, valid)]
    dt = FIXED[kind][1]
    if dt in (np.int16, np.int32, np.int64):
        return valid, np.array(vals, dtype=np.int64).astype(dt)
    return valid, np.array(vals, dtype=np.uint64).astype(dt)


def deferred_bits(cells):
    return np.array([c[0] == "Deferred" for c in cells], dtype=bool)


def arrow_columns(rows, type_classes):
    """(kinds, [column model]) for an eligible table."""
    kinds, bad = arrow_kinds(type_classes)
    assert bad is None
    return kinds, [arrow_column([r[i] for r in rows], k) for i, k in enumerate(kinds)]
