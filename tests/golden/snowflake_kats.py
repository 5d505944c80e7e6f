"""The Snowflake sink's own test vectors, transcribed from the reference (crates/etl-destinations/src/snowflake/...). Values are
compared as parsed JSON, the way the reference's tests compare them (serde_json::Value equality). Data only."""

# encoding.rs:311-350 cell_serialization_ok: (cell, expected JSON value as text). Cells in materialize() form; "2026-04-29" is chrono
# day 739735 from CE; 10:30:00.123456 = 37800 s + 123456000 ns.
CELL_OK = [
    (("Null",), "null"),
    (("Bool", True), "true"),
    (("Bool", False), "false"),
    (("String", b"hello"), '"hello"'),
    (("I16", 42), "42"),
    (("I32", 2147483647), "2147483647"),
    (("U32", 4294967295), "4294967295"),
    (("I64", 9223372036854775807), "9223372036854775807"),
    (("F32", 0x3FC00000), "1.5"),                      # F32(1.5) -> json!(1.5f64)
    (("F64", 0x4004000000000000), "2.5"),
    (("Numeric", 0, 0, 0, 0, ()), '"0"'),              # PgNumeric::default().to_string()
    (("Date", 739735), '"2026-04-29"'),
    (("Time", 37800, 123456000), '"10:30:00.123456"'),
    (("Timestamp", 739735, 37800, 123456000), '"2026-04-29 10:30:00.123456"'),
    (("TimestampTz", 739735, 37800, 0), '"2026-04-29 10:30:00+00:00"'),
    (("Uuid", bytes(16)), '"00000000-0000-0000-0000-000000000000"'),
    (("Deferred", 3802, b'{"key": [1, 2, 3]}'), '{"key":[1,2,3]}'),
    (("Bytes", bytes([0xDE, 0xAD, 0xBE, 0xEF])), '"deadbeef"'),
]

# encoding.rs:353-371 rejects_non_finite: every one of these cells fails (the detail is Error::Encoding's Display, error.rs:25-26)
REJECTED = [
    (("F64", 0x7FF8000000000000), "Encoding error: Snowflake does not support NaN/Infinity float values: NaN"),
    (("F64", 0x7FF0000000000000), "Encoding error: Snowflake does not support NaN/Infinity float values: inf"),
    (("F64", 0xFFF0000000000000), "Encoding error: Snowflake does not support NaN/Infinity float values: -inf"),
    (("F32", 0x7FC00000), "Encoding error: Snowflake does not support NaN/Infinity float values: NaN"),
    (("F32", 0x7F800000), "Encoding error: Snowflake does not support NaN/Infinity float values: inf"),
    (("F32", 0xFF800000), "Encoding error: Snowflake does not support NaN/Infinity float values: -inf"),
    (("Numeric", 1, 0, 0, 0, ()), "Encoding error: Snowflake NUMBER does not support NaN"),
    (("Numeric", 2, 0, 0, 0, ()), "Encoding error: Snowflake NUMBER does not support Infinity"),
    (("Numeric", 3, 0, 0, 0, ()), "Encoding error: Snowflake NUMBER does not support Infinity"),
]

# encoding.rs:373-408 array_serialization_ok: (array type oid, literal, expected JSON value as text)
ARRAY_OK = [
    (1007, b"{1,NULL,3}", "[1, null, 3]"),
    (1007, b"{}", "[]"),
    (1000, b"{t,NULL}", "[true, null]"),
    (1009, b"{a,NULL}", '["a", null]'),
    (1001, b'{"\\\\xff",NULL}', '["ff", null]'),
    (2951, b"{00000000-0000-0000-0000-000000000000}", '["00000000-0000-0000-0000-000000000000"]'),
    (3807, b"{1,NULL}", "[1, null]"),
    (1022, b"{1.5,NULL,2.5}", "[1.5, null, 2.5]"),
    (1182, b"{2026-04-29,NULL}", '["2026-04-29", null]'),
]

# encoding.rs:410-421 array_rejects_non_finite
ARRAY_REJECTED = [
    (1022, b"{NaN}", "Encoding error: Snowflake does not support NaN/Infinity float values: NaN"),
    (1021, b"{Infinity}", "Encoding error: Snowflake does not support NaN/Infinity float values: inf"),
    (1231, b"{NaN}", "Encoding error: Snowflake NUMBER does not support NaN"),
]

# encoding.rs:423-434 multi_column_row: columns id, name; I32(1), String("hello"); CdcMeta(Insert, "0")
MULTI_COLUMN = (["id", "name"], [("I32", 1), ("String", b"hello")], "insert", "0", {"id": 1, "name": "hello"})
# encoding.rs:436-461 multi_row_ndjson: two rows of column id, one line each
MULTI_ROW = (["id"], [[("I32", 1)], [("I32", 2)]], "insert", "0", [{"id": 1}, {"id": 2}])
# encoding.rs:463-478 cdc_columns
CDC = (["id", "name"], [("I32", 1), ("String", b"Alice")], "insert", "0000/0000",
       {"id": 1, "name": "Alice", "_cdc_operation": "insert", "_cdc_sequence_number": "0000/0000"})

# streaming/offset_token.rs:16-23: zero() and new(commit_lsn, tx_ordinal) = "{:016x}/{:016x}"
OFFSET_ZERO = "0000000000000000/0000000000000000"
OFFSET_NEW = [((0, 0), "0000000000000000/0000000000000000"), ((0x16B3748, 7), "00000000016b3748/0000000000000007"),
              ((2**64 - 1, 2**64 - 1), "ffffffffffffffff/ffffffffffffffff")]

# core.rs:897-960: which row an update / delete becomes. (event kind, image kind) -> "new" | "old" | "key" | None (the host raises
# SourceReplicaIdentityError)
ROW_CHOICES = [(("U", "Full"), "new"), (("U", "Partial"), None), (("D", "Full"), "old"), (("D", "Key"), "key"), (("D", "None"), None)]
