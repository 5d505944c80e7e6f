"""Known answers for the sinks' table-copy rows, transcribed as data from the reference (crates/etl-destinations/src): the kind table
of DuckLake's Arrow copy staging, the reference's own tests of prepare_copy_rows, and what ClickHouse and BigQuery append to a copied
row. tests/test_table_copy_sink_kats.py holds the model tests/table_copy_sinks.py to them. Cells are the Postgres texts that decode to
the reference's `Cell` literals (None = NULL), as in tests/golden/arrow_kats.py."""

# ducklake/encoding.rs:236-257 arrow_column_kind, row by row: (line, PgType, type oid, ArrowColumnKind | None);
# :237-239 is_array_type comes first (any array type: None); :255 `_ => Utf8` (here: text, varchar, numeric, timetz)
KIND_TABLE = [
    (242, "BOOL", 16, "Bool"), (243, "INT2", 21, "I16"), (244, "INT4", 23, "I32"), (245, "INT8", 20, "I64"), (246, "OID", 26, "U64"),
    (247, "FLOAT4", 700, "F32"), (248, "FLOAT8", 701, "F64"), (249, "DATE", 1082, "Date32"), (250, "TIME", 1083, "Time64Microsecond"),
    (251, "TIMESTAMP", 1114, "TimestampMicrosecond"), (252, "TIMESTAMPTZ", 1184, "TimestampTzMicrosecond"), (253, "BYTEA", 17, "Binary"),
    (254, "UUID", 2950, None), (254, "JSON", 114, None), (254, "JSONB", 3802, None),
    (255, "TEXT", 25, "Utf8"), (255, "VARCHAR", 1043, "Utf8"), (255, "NUMERIC", 1700, "Utf8"), (255, "TIMETZ", 1266, "Utf8"),
    (237, "INT4_ARRAY", 1007, None), (237, "TEXT_ARRAY", 1009, None),
]
# ducklake/encoding.rs:87-105 ArrowColumnKind::data_type: kind -> (Arrow DataType, bytes per value | None for bit-packed / var-len,
# bits per offset | None)
DATA_TYPES = {
    "Bool": ("Boolean", None, None), "I16": ("Int16", 2, None), "I32": ("Int32", 4, None), "I64": ("Int64", 8, None), "U64": ("UInt64", 8, None),
    "F32": ("Float32", 4, None), "F64": ("Float64", 8, None), "Utf8": ("Utf8", None, 32), "Date32": ("Date32", 4, None),
    "Time64Microsecond": ("Time64(us)", 8, None), "TimestampMicrosecond": ("Timestamp(us)", 8, None),
    "TimestampTzMicrosecond": ("Timestamp(us,+00:00)", 8, None), "Binary": ("Binary", None, 32),
}

# ducklake/encoding.rs:787-824 prepare_copy_rows_uses_arrow_for_supported_columns, the same table at batches.rs:2520-2548
# (staging_load_rows_appends_arrow_record_batch): columns (name, oid, nullable), rows, the data types it asserts, rows x columns
ARROW_TABLE = {
    "lines": "encoding.rs:787-824, batches.rs:2520-2548",
    "cols": [("id", 23, False), ("name", 25, True), ("created_at", 1114, True)],
    "rows": [["1", "alice", "2026-01-02 03:04:05"], ["2", None, None]],
    "data_types": ["Int32", "Utf8", "Timestamp(us)"],
    "num_rows": 2, "num_columns": 3,
    # not asserted by the reference's test — arrow's layout of those values: NaiveDate(2026, 1, 2) 03:04:05 in microseconds
    "values": [[1, 2], [b"alice", None], [1767323045000000, None]],
}
# :827-847 prepare_copy_rows_falls_back_for_array_columns (SqlLiterals "(1, [1, NULL])"), :850-870 ..._for_cast_sensitive_columns (Appender)
FALLBACKS = [
    ("encoding.rs:827-847", [("id", 23, False), ("tags", 1007, True)], 1, "SqlLiterals"),
    ("encoding.rs:850-870", [("payload", 114, False)], 0, "Appender"),
]

# clickhouse/core.rs:755-759: "Initial-copy rows are tagged as INSERT with LSN 0 / tx_ordinal 0";
# append_cdc_columns(&mut values, CdcOperation::Insert, PgLsn::from(0), 0, engine)
CLICKHOUSE_COPY_CDC = {"lines": "clickhouse/core.rs:755-759", "operation": "INSERT", "commit_lsn": 0, "tx_ordinal": 0,
                       # core.rs:96-114 append_cdc_columns: MergeTree String(op) + UInt64(lsn); ReplacingMergeTree UInt128(lsn << 64 | ordinal) + UInt8(deleted)
                       "merge_tree": b"\x06INSERT" + bytes(8), "replacing_merge_tree": bytes(16) + b"\x00"}
# bigquery/core.rs:611-614: `table_row.values_mut().push(BigQueryOperationType::Upsert.into_cell())` — one trailing cell, nothing else
BIGQUERY_COPY_TRAILING = {"lines": "bigquery/core.rs:611-614", "cells": ["UPSERT"]}
