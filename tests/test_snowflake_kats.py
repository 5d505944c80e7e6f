"""The Snowflake sink's own vectors (tests/golden/snowflake_kats.py, transcribed from snowflake/encoding.rs, offset_token.rs and
core.rs) against the CPU restatement tests/snowflake_ndjson.py, compared as parsed JSON values the way the reference compares them;
and the restatement's byte rules (escaping, float layout) pinned on hand-written cases."""
import datetime as dt
import json

import pytest

from tests import snowflake_ndjson as SN
from tests.golden import snowflake_kats as K


def test_kat_dates_are_chrono_days():
    assert dt.date(2026, 4, 29).toordinal() == 739735


@pytest.mark.parametrize("cell,want", K.CELL_OK)
def test_cell_serialization_ok(cell, want):
    line = SN.line(["v"], [cell], "insert", "0")
    assert json.loads(line)["v"] == json.loads(want)
    assert line.endswith(b"\n") and line.count(b"\n") == 1


@pytest.mark.parametrize("cell,detail", K.REJECTED)
def test_rejects_non_finite(cell, detail):
    with pytest.raises(SN.EncodingError) as ei:
        SN.line(["v"], [cell], "insert", "0")
    assert str(ei.value) == detail


@pytest.mark.parametrize("oid,lit,want", K.ARRAY_OK)
def test_array_serialization_ok(oid, lit, want):
    assert json.loads(SN.line(["v"], [("Deferred", oid, lit)], "insert", "0"))["v"] == json.loads(want)


@pytest.mark.parametrize("oid,lit,detail", K.ARRAY_REJECTED)
def test_array_rejects_non_finite(oid, lit, detail):
    with pytest.raises(SN.EncodingError) as ei:
        SN.line(["v"], [("Deferred", oid, lit)], "insert", "0")
    assert str(ei.value) == detail


def test_multi_column_row_multi_row_ndjson_and_cdc_columns():
    names, cells, op, seq, want = K.MULTI_COLUMN
    got = json.loads(SN.line(names, cells, op, seq))
    assert all(got[k] == v for k, v in want.items())
    names, rows, op, seq, want = K.MULTI_ROW
    text = b"".join(SN.line(names, r, op, seq) for r in rows)
    lines = text.rstrip(b"\n").split(b"\n")
    assert len(lines) == 2 and [json.loads(x)["id"] for x in lines] == [w["id"] for w in want]
    names, cells, op, seq, want = K.CDC
    assert json.loads(SN.line(names, cells, op, seq)) == want


def test_offset_token():
    assert SN.ZERO_TOKEN == K.OFFSET_ZERO
    for (lsn, ord_), want in K.OFFSET_NEW:
        ev = [{"kind": "I", "schema_slot": 0, "commit_lsn": lsn, "tx_ordinal": ord_, "row": [("I32", 1)]}]
        rows, idx, host = SN.event_rows(ev, 0, ["id"], [1])
        assert json.loads(rows[0])["_cdc_sequence_number"] == want
        rows, _, _ = SN.event_rows(ev, 0, ["id"], [1], copy=True)
        assert json.loads(rows[0])["_cdc_sequence_number"] == K.OFFSET_ZERO


def test_update_and_delete_row_choices():
    full, key = [("I32", 1), ("String", b"alice")], [("I32", 1)]
    for (kind, image), want in K.ROW_CHOICES:
        e = {"kind": kind, "schema_slot": 0, "commit_lsn": 5, "tx_ordinal": 1}
        if kind == "U":
            e.update(partial=image == "Partial", old_kind="None", row=full)
        else:
            e.update(old_kind=image)
            if image != "None":
                e["old_row"] = full if image == "Full" else key
        rows, idx, host = SN.event_rows([e], 0, ["id", "name"], [1, 0])
        if want is None:
            assert rows == [] and host == 1
            continue
        got = json.loads(rows[0])
        assert got["_cdc_operation"] == ("update" if kind == "U" else "delete")
        assert {k: v for k, v in got.items() if not k.startswith("_cdc")} == ({"id": 1} if want == "key" else {"id": 1, "name": "alice"})


def test_escaping_and_float_layout_rules():
    assert SN.jstr(bytes(range(0x20))) == (b'"\\u0000\\u0001\\u0002\\u0003\\u0004\\u0005\\u0006\\u0007\\b\\t\\n\\u000b\\f\\r\\u000e\\u000f'
                                         b'\\u0010\\u0011\\u0012\\u0013\\u0014\\u0015\\u0016\\u0017\\u0018\\u0019\\u001a\\u001b\\u001c\\u001d\\u001e\\u001f"')
    assert SN.jstr('a"b\\c\x7f é') == b'"a\\"b\\\\c\x7f' + " é".encode() + b'"'
    import struct

    def f64(v):
        return SN.float_text(struct.unpack("<Q", struct.pack("<d", v))[0], False).decode()

    def f32(v):
        return SN.float_text(struct.unpack("<I", struct.pack("<f", v))[0], True).decode()
    assert [f64(v) for v in (0.0, -0.0, 1e15, 1e16, 12.34, 1e-5, 1e-6, 1.5e-7, 1.234e33, -2.5, 5e-324)] == \
        ["0.0", "-0.0", "1000000000000000.0", "1e16", "12.34", "0.00001", "1e-6", "1.5e-7", "1.234e33", "-2.5", "5e-324"]
    assert [f32(v) for v in (1e12, 1e13, 1e-5, 1e-6, 1e-7, 3.4028235e38)] == ["1000000000000.0", "1e13", "0.00001", "0.000001", "1e-7", "3.4028235e38"]
