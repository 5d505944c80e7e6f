"""The DuckLake sink's own vectors (tests/golden/ducklake_kats.py, transcribed from ducklake/encoding.rs, sql.rs and batches.rs) against
the CPU restatement tests/ducklake_literals.py, byte for byte as the reference's tests compare them (String equality); the
restatement's remaining rules (float Display, six-digit fractions, CASTs) pinned on hand-written cases; and quote_literal's UNPINNED
arms in a test of their own (test_quote_literal_unpinned_arms), so that a correction of the restated pg_escape rule is one edit there
and one in the kernel."""
import datetime as dt
import struct

import pytest

from tests import ducklake_literals as DL
from tests.golden import ducklake_kats as K


@pytest.mark.parametrize("oid,lit,want", K.ARRAYS)
def test_array_cell_to_sql_literal_preserves_nulls(oid, lit, want):
    assert DL.literal(("Deferred", oid, lit)) == want


@pytest.mark.parametrize("cells,want", K.TUPLES)
def test_rows_with_arrays_as_sql_literals(cells, want):
    assert DL.tuple_literal(cells) == want
    ev = [{"kind": "I", "schema_slot": 0, "row": cells}]
    assert DL.event_records(ev, 0, ["id", "tags"], [1, 0], DL.TUPLES) == ([want], [0], 0)
    assert DL.event_records(ev, 0, ["id", "tags"], [1, 0], DL.TUPLES, copy=True, primary_key=[1, 0]) == ([want], [0], 0)
    assert DL.event_records(ev, 0, ["id", "tags"], [1, 0], DL.PREDICATES) == ([], [], 0)
    assert DL.event_records(ev, 0, ["id", "tags"], [1, 0], DL.PREDICATES, copy=True, primary_key=[1, 0]) == ([b'"id" = 1'], [0], 0)
    assert DL.event_records(ev, 0, ["id", "tags"], [1, 0], DL.PREDICATES, copy=True, primary_key=[0, 0]) == ([b""], [0], 0)


@pytest.mark.parametrize("name,want", K.IDENTIFIERS)
def test_quote_identifier(name, want):
    assert DL.quote_identifier(name) == want


@pytest.mark.parametrize("names,ident,row,want", K.PREDICATES)
def test_delete_predicate_from_row(names, ident, row, want):
    for ev in ({"kind": "D", "schema_slot": 0, "old_kind": "Full", "old_row": row},
               {"kind": "U", "schema_slot": 0, "partial": False, "old_kind": "Full", "old_row": row, "row": row},
               {"kind": "U", "schema_slot": 0, "partial": False, "old_kind": "None", "row": row},
               {"kind": "D", "schema_slot": 0, "old_kind": "Key", "old_row": [c for c, f in zip(row, ident) if f]}):
        assert DL.event_records([ev], 0, names, ident, DL.PREDICATES) == ([want], [0], 0)


def test_missing_replica_identity_is_left_to_the_host():
    names, ident, ev = K.NO_IDENTITY
    assert DL.event_records([ev], 0, names, ident, DL.PREDICATES) == ([], [], 1)


@pytest.mark.parametrize("names,ident,events,want", K.MUTATIONS)
def test_prepare_table_mutations_predicates(names, ident, events, want):
    assert DL.event_records(events, 0, names, ident, DL.PREDICATES) == (want, list(range(len(events))), 0)


def test_text_predicate_shape():
    name, cell, want = K.TEXT_PREDICATE
    assert DL.predicate([name], [cell]) == want


def test_row_choices():
    full, key = [("I32", 1), ("String", b"alice")], [("I32", 1)]
    names, ident = ["id", "name"], [1, 0]

    def both(e):
        return tuple(DL.event_records([dict(e, schema_slot=0)], 0, names, ident, w) for w in (DL.TUPLES, DL.PREDICATES))
    t, p = b"(1, 'alice')", b'"id" = 1'
    assert both({"kind": "I", "row": full}) == (([t], [0], 0), ([], [], 0))
    assert both({"kind": "U", "partial": False, "old_kind": "Full", "old_row": full, "row": full}) == (([t], [0], 0), ([p], [0], 0))
    assert both({"kind": "U", "partial": False, "old_kind": "Key", "old_row": key, "row": full}) == (([t], [0], 0), ([p], [0], 0))
    assert both({"kind": "U", "partial": False, "old_kind": "None", "row": full}) == (([t], [0], 0), ([p], [0], 0))
    assert both({"kind": "U", "partial": True, "old_kind": "Key", "old_row": key, "row": full}) == (([], [], 1), ([p], [0], 0))
    assert both({"kind": "U", "partial": True, "old_kind": "None", "row": full}) == (([], [], 1), ([], [], 1))
    assert both({"kind": "D", "old_kind": "Full", "old_row": full}) == (([], [], 0), ([p], [0], 0))
    assert both({"kind": "D", "old_kind": "Key", "old_row": key}) == (([], [], 0), ([p], [0], 0))
    assert both({"kind": "D", "old_kind": "None"}) == (([], [], 0), ([], [], 1))
    assert DL.predicate(["id", "name"], [("Null",), ("String", b"x")]) == b'"id" IS NULL AND "name" = \'x\''


def test_quote_literal_plain_arm_is_pinned():
    assert DL.quote_literal("alice") == b"'alice'"                       # batches.rs:2687
    assert DL.quote_literal('{"a":1}') == b"'{\"a\":1}'"                # encoding.rs:766
    assert DL.quote_literal("") == b"''" and DL.quote_literal("é日本") == "'é日本'".encode()


def test_quote_literal_unpinned_arms():
    """pg_escape 0.1.1 as its documentation states it — NOT pinned by any reference vector; the device twin is dl_quote."""
    assert DL.quote_literal("O'Reilly") == b"'O''Reilly'"
    assert DL.quote_literal("a\\b") == b" E'a\\\\b'"
    assert DL.quote_literal("'\\'") == b" E'''\\\\'''"
    assert DL.literal(("Deferred", 114, b'{"k": "a\\"b"}')) == b" E'{\"k\":\"a\\\\\"b\"}'".join([b"CAST(", b" AS JSON)"])


def test_scalar_literals():
    def f64(v):
        return DL.float_literal(struct.unpack("<Q", struct.pack("<d", v))[0], False).decode()

    def f32(v):
        return DL.float_literal(struct.unpack("<I", struct.pack("<f", v))[0], True).decode()
    assert [f64(v) for v in (0.0, -0.0, 1.0, 0.1, 1e21, 1e15, 1e16, 12.34, 1.5e-7, -2.5, 1e23)] == \
        ["0", "-0", "1", "0.1", "1" + "0" * 21, "1" + "0" * 15, "1" + "0" * 16, "12.34", "0.00000015", "-2.5", "1" + "0" * 23]
    assert f64(5e-324) == "0." + "0" * 323 + "5" and len(f64(-5e-324)) == 327
    assert f64(1.7976931348623157e308) == "17976931348623157" + "0" * 292
    assert f32(0.1) == "0.10000000149011612" and f32(1.5) == "1.5" and f32(1e-45) == "0." + "0" * 44 + "1401298464324817"
    assert f64(float("nan")) == "CAST('NaN' AS DOUBLE)" and f64(float("inf")) == "CAST('Infinity' AS DOUBLE)" and f64(float("-inf")) == "CAST('-Infinity' AS DOUBLE)"
    assert f32(float("nan")) == "CAST('NaN' AS FLOAT)" and f32(float("inf")) == "CAST('Infinity' AS FLOAT)" and f32(float("-inf")) == "CAST('-Infinity' AS FLOAT)"
    day = dt.date(2026, 4, 29).toordinal()
    assert DL.literal(("Null",)) == b"NULL" and DL.literal(("Bool", True)) == b"TRUE" and DL.literal(("Bool", False)) == b"FALSE"
    assert DL.literal(("I64", -9223372036854775808)) == b"-9223372036854775808" and DL.literal(("U32", 4294967295)) == b"4294967295"
    assert DL.literal(("Date", day)) == b"DATE '2026-04-29'"
    assert DL.literal(("Time", 37800, 0)) == b"TIME '10:30:00.000000'" and DL.literal(("Time", 37800, 123456000)) == b"TIME '10:30:00.123456'"
    assert DL.literal(("Timestamp", day, 37800, 500000000)) == b"TIMESTAMP '2026-04-29 10:30:00.500000'"
    assert DL.literal(("TimestampTz", day, 37800, 0)) == b"TIMESTAMPTZ '2026-04-29 10:30:00.000000+00:00'"
    assert DL.literal(("Uuid", bytes(range(16)))) == b"CAST('00010203-0405-0607-0809-0a0b0c0d0e0f' AS UUID)"
    assert DL.literal(("Bytes", bytes([0xDE, 0xAD, 0xBE, 0xEF]))) == b"from_hex('DEADBEEF')"
    assert DL.literal(("Numeric", 0, 0, 0, 0, ())) == b"'0'"
    assert DL.literal(("Deferred", 1007, b"{}")) == b"[]" and DL.literal(("Deferred", 1009, b'{a,"b\'c",NULL}')) == b"['a', 'b''c', NULL]"
    assert DL.literal(("Deferred", 1001, b'{"\\\\xdeadBEEF",NULL}')) == b"[from_hex('DEADBEEF'), NULL]"
