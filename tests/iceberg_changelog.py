"""TEST INFRASTRUCTURE — a small host model of the Iceberg sink's changelog rows (crates/etl-destinations/src/iceberg/core.rs:300-416,
write_table_rows :268-291), built from `HostBatch.materialize()` — the reference's value model — and not from arena offsets. Pinned to
the reference's own vectors by tests/test_iceberg_kats.py; tests/test_gpu_iceberg.py holds etlg_batch_iceberg against it.

  Insert -> the row | Update -> the full new row | Delete -> the full OLD row (core.rs:300-416)
  + cdc_operation "INSERT" | "UPDATE" | "DELETE" (IcebergOperationType Display, :77-85)
  + sequence_number = event_sequence_key().to_string() = `{commit_lsn:016x}/{tx_ordinal:016x}` (crates/etl/src/event.rs:346-351);
    generate_sequence_number(0, 0) for table-copy rows (:370-375)
  a partial Update, a key-only Delete, a Delete without an old image: SourceReplicaIdentityError (iceberg_update_row /
  iceberg_delete_row, :636-680) — here counted, the first one named.

A row's values are Python values per the cell_to_* converters (iceberg/encoding.rs:150-360): None, bool, int (Int32 / Int64; Date32 days
since 1970-01-01; Time64 / Timestamp microseconds), float bit patterns as int ("nan" for any NaN), 16 uuid bytes, bytes for strings /
binary / Display strings (numeric, timetz, formatted json) / the source text of a text-form cell, lists of those for parsed arrays."""
from etl_amd import abi
from oracle import arrays as OA
from oracle import display as D
from oracle import json_display as J
from oracle.rowbinary import ARRAY_OIDS, NeedsHost, array_elements

PARTIAL_UPDATE, KEY_ONLY_DELETE, DELETE_WITHOUT_OLD_ROW = 1, 2, 3      # ETLG_ICE_* (include/etlg.h)
NO_EVENT = (1 << 64) - 1
OPS = {"I": b"INSERT", "U": b"UPDATE", "D": b"DELETE"}                 # core.rs:77-85
COPY_SEQUENCE = b"0000000000000000/0000000000000000"                   # generate_sequence_number(0, 0)
CE_DAYS_1970 = 719163
# the three refusals' descriptions (core.rs:642-678), by reason
DESCRIPTIONS = {PARTIAL_UPDATE: "Iceberg update requires a full new row image",
                KEY_ONLY_DELETE: "Iceberg delete requires a full old row image",
                DELETE_WITHOUT_OLD_ROW: "Iceberg delete requires an old row image"}


def sequence_number(commit_lsn, tx_ordinal):
    """EventSequenceKey Display (event.rs:346-351)."""
    return b"%016x/%016x" % (commit_lsn, tx_ordinal)


def choose(e):
    """(row cells | None, refusal reason) of one row event — iceberg_update_row / iceberg_delete_row."""
    k = e["kind"]
    if k == "I":
        return e["row"], 0
    if k == "U":
        return (None, PARTIAL_UPDATE) if e.get("partial") else (e["row"], 0)
    if e.get("old_kind") == "Full":
        return e["old_row"], 0
    return None, KEY_ONLY_DELETE if e.get("old_kind") == "Key" else DELETE_WITHOUT_OLD_ROW


def _float(bits, is32):
    nan = (bits & 0x7F800000) == 0x7F800000 and bits & 0x7FFFFF if is32 else (bits & (0x7FF << 52)) == (0x7FF << 52) and bits & ((1 << 52) - 1)
    return "nan" if nan else bits


def scalar(c):
    """One materialize() cell of a settled class -> its Arrow value."""
    k = c[0]
    if k in ("Null", "Missing"):
        return None
    if k in ("Bool", "I16", "I32", "I64", "U32"):
        return c[1]
    if k in ("F32", "F64"):
        return _float(c[1], k == "F32")
    if k == "Date":
        return c[1] - CE_DAYS_1970
    if k == "Time":
        return c[1] * 1_000_000 + c[2] // 1000
    if k in ("Timestamp", "TimestampTz"):
        return ((c[1] - CE_DAYS_1970) * 86400 + c[2]) * 1_000_000 + c[3] // 1000
    if k == "TimeTz":
        return D.timetz_string(*c[1:]).encode()
    if k == "Numeric":
        return D.numeric_string(*c[1:]).encode()
    if k in ("Uuid", "Bytes", "String"):
        return bytes(c[1])
    raise AssertionError(c)


def _float_cells(type_oid, text):
    from tests.snowflake_ndjson import _float_elements
    return _float_elements(type_oid, text)


def parsed_array(type_oid, text):
    """An array literal as the list the device builds (ETLG_ROWS_PARSE_ARRAYS), or NeedsHost where it hands the row back."""
    text = bytes(text)
    if type_oid in ARRAY_OIDS:
        if any(e is not None and len(e) > OA.ELEM_MAX for e in OA.split_literal(type_oid, text)):
            raise NeedsHost("an element of more than 40 characters")
        cells = _float_cells(type_oid, text) if type_oid in (1021, 1022) else array_elements(type_oid, text)
        return [scalar(c) for c in cells]
    return [e for e, _ in OA.elements(type_oid, text)]


def value(c, col, parse_arrays=False, format_json=False):
    """One cell of a replicated column -> its value in the hand-off's column."""
    if c[0] != "Deferred":
        return scalar(c)
    text = bytes(c[2])
    if col.type_class == abi.TC_JSON:
        return J.display(text) if format_json and J.device_limits_ok(text) else text
    if col.type_class == abi.TC_ARRAY:
        if not parse_arrays:
            return text
        try:
            return parsed_array(col.type_oid, text)
        except NeedsHost:
            return None                                   # the row is handed back: null, set in `deferred`
    return None                                           # a settled class handed back DEFERRED: null in the column, set in `deferred`


def changelog(events, slot_index, cols, copy=False, parse_arrays=False, format_json=False):
    """(rows, ops, sequence strings, row_event, n_host_rows, first refused event | NO_EVENT, its reason | 0) for the rows of schema slot
    `slot_index`; `cols`: the slot's columns (type_class, type_oid), e.g. HostBatch.slots[slot_index].cols."""
    rows, ops, seqs, idx = [], [], [], []
    n_host, first, why = 0, NO_EVENT, 0
    for i, e in enumerate(events):
        if e["kind"] not in "IUD" or e.get("schema_slot") != slot_index:
            continue
        cells, reason = choose(e)
        if reason:
            n_host += 1
            if first == NO_EVENT:
                first, why = i, reason
            continue
        rows.append([value(c, col, parse_arrays, format_json) for c, col in zip(cells, cols)])
        ops.append(OPS["I" if copy else e["kind"]])
        seqs.append(COPY_SEQUENCE if copy else sequence_number(e["commit_lsn"], e["tx_ordinal"]))
        idx.append(i)
    return rows, ops, seqs, idx, n_host, first, why
