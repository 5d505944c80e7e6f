"""TEST INFRASTRUCTURE — CPU restatement of the reference's DuckLake SQL literal grammar and of the rows etlg_batch_duckdb builds
from it, for the parity tests of the device path (etl_amd/csrc/rowformats.hip.h, dl_row). Never imported by the product path.

Follows crates/etl-destinations/src/ducklake/encoding.rs: table_row_to_sql_literal_ref :366-369 (`(` cells joined by `, ` `)`),
cell_to_sql_literal :387-419, array_cell_to_sql_literal :470-585 (`[e, e, NULL]`), float_literal :588-612, encode_hex :615-617;
ducklake/sql.rs:10-12 (quote_double_identifier); ducklake/batches.rs: delete_predicate_from_row :1229-1316 (`"col" = lit` / `"col" IS
NULL` over the identity columns, joined by ` AND `), prepare_table_mutations :1128-1226 and ducklake/core.rs:1824-1945 (what an event
becomes: Insert -> upsert; Update with an old image -> delete by it + upsert of a full new row / UPDATE by it for a partial one; Update
without one -> Replace from the new row's identity columns, a partial one through key_row_from_updated_partial_row on the host; Delete
-> by its old image, which it must have), delete_predicate_from_copy_row :1477-1510 (copied rows: over the primary key).

Crates that are NOT under the reference, restated from their published behaviour:
  * Rust's f64 Display (`value.to_string()`): the shortest round-trip digits laid out positionally, never an exponent, no trailing
    ".0": 1, -0, 0.1, 1e21 -> 1 and 21 zeros, 5e-324 -> "0." + 323 zeros + "5". The digits come from Python's repr. A float4 is
    widened first (`f as f64`): 0.1f32 -> 0.10000000149011612.
  * chrono's %.6f: always six fraction digits; %:z of a DateTime<Utc>: +00:00.
  * pg_escape 0.1.1 quote_literal — RESTATED FROM THE CRATE'S DOCUMENTATION, its source is not on hand and the reference's tests pin
    only the plain arm ('alice', '{"a":1}'). See quote_literal() below: the quote doubling and the backslash arm are UNPINNED.
Display strings come from oracle/display.py, json values from oracle/json_display.py, array literals from oracle/arrays.py.

Works on the per-cell tuples of etl_amd.view.HostBatch.materialize()."""
import datetime as dt
import struct
from decimal import Decimal

from oracle import arrays
from oracle import json_display as J
from oracle.display import numeric_string, timetz_string
from oracle.rowbinary import ARRAY_OIDS, NeedsHost, array_elements
from tests.snowflake_ndjson import _float_elements   # float4[] / float8[] literals -> element cells with NaN kept (shared with the NDJSON restatement)

TUPLES, PREDICATES = 0, 1


def quote_literal(b):
    """pg_escape 0.1.1 `quote_literal`, over bytes. UNPINNED beyond the plain arm — restated from the crate's documentation: a `'` is
    doubled; if the text holds a backslash, every backslash is doubled and the literal is prefixed with a space and `E`
    (a\\b -> " E'a\\\\b'"); otherwise plain '...'. The device twin is dl_quote (rowformats.hip.h): a correction is one edit on each side."""
    if isinstance(b, str):
        b = b.encode()
    b = bytes(b)
    body = b.replace(b"'", b"''").replace(b"\\", b"\\\\")
    return (b" E'" if b"\\" in b else b"'") + body + b"'"


def quote_identifier(name):
    """quote_double_identifier (ducklake/sql.rs:10-12): '"' doubled, nothing else changed."""
    if isinstance(name, str):
        name = name.encode()
    return b'"' + bytes(name).replace(b'"', b'""') + b'"'


def float_display(v):
    """Rust's Display of a finite f64."""
    neg = struct.pack("<d", v)[7] >> 7
    s = "-" if neg else ""
    if v == 0:
        return s + "0"
    t = Decimal(repr(abs(v))).normalize().as_tuple()
    digits, e = "".join(map(str, t.digits)), t.exponent
    n = len(digits)
    kk = n + e
    if e >= 0:
        return s + digits + "0" * e
    if kk > 0:
        return s + digits[:kk] + "." + digits[kk:]
    return s + "0." + "0" * -kk + digits


def float_literal(bits, is32):
    """float_literal (:588-612) of F32(bits) / F64(bits): the f32 is widened first."""
    v = struct.unpack("<f", struct.pack("<I", bits))[0] if is32 else struct.unpack("<d", struct.pack("<Q", bits))[0]
    ty = "FLOAT" if is32 else "DOUBLE"
    if v != v:
        return f"CAST('NaN' AS {ty})".encode()
    if v in (float("inf"), float("-inf")):
        return f"CAST('{'-' if v < 0 else ''}Infinity' AS {ty})".encode()
    return float_display(v).encode()


def date_string(days_ce):
    d = dt.date.fromordinal(days_ce)
    return f"{d.year:04}-{d.month:02}-{d.day:02}"


def time6(secs, nanos):
    """%H:%M:%S%.6f (a leap second is nanos >= 10^9 on second 59, printed as :60)."""
    leap = 1 if nanos >= 10**9 else 0
    nanos -= leap * 10**9
    return f"{secs // 3600:02}:{secs // 60 % 60:02}:{secs % 60 + leap:02}.{nanos // 1000:06}"


def _json(text):
    try:
        J.parse(text)
    except ValueError:
        raise arrays.JsonDecodeError(text) from None
    if not J.device_limits_ok(text):
        raise NeedsHost("json beyond json_display's limits")
    return b"CAST(" + quote_literal(J.display(text)) + b" AS JSON)"


def literal(c):
    """cell_to_sql_literal for a materialize() cell -> bytes. Raises NeedsHost, arrays.JsonDecodeError."""
    k = c[0]
    if k == "Null":
        return b"NULL"
    if k == "Bool":
        return b"TRUE" if c[1] else b"FALSE"
    if k in ("I16", "I32", "I64", "U32"):
        return str(c[1]).encode()
    if k in ("F32", "F64"):
        return float_literal(c[1], k == "F32")
    if k == "Numeric":
        return quote_literal(numeric_string(*c[1:]))
    if k == "Date":
        return b"DATE '" + date_string(c[1]).encode() + b"'"
    if k == "Time":
        return b"TIME '" + time6(c[1], c[2]).encode() + b"'"
    if k == "Timestamp":
        return b"TIMESTAMP '" + (date_string(c[1]) + " " + time6(c[2], c[3])).encode() + b"'"
    if k == "TimestampTz":
        return b"TIMESTAMPTZ '" + (date_string(c[1]) + " " + time6(c[2], c[3]) + "+00:00").encode() + b"'"
    if k == "TimeTz":
        return quote_literal(timetz_string(*c[1:]))
    if k == "Uuid":
        h = c[1].hex()
        return b"CAST(" + quote_literal(f"{h[:8]}-{h[8:12]}-{h[12:16]}-{h[16:20]}-{h[20:]}") + b" AS UUID)"
    if k == "Bytes":
        return b"from_hex('" + bytes(c[1]).hex().upper().encode() + b"')"
    if k == "String":
        return quote_literal(c[1])
    if k == "Array":                                   # a typed array (ETLG_F_FINISH_CELLS)
        return b"[" + b", ".join(literal(x) for x in c[2]) + b"]"
    if k == "Deferred" and c[1] in (114, 3802):
        return _json(c[2])
    if k == "Deferred":
        return array_literal(c[1], bytes(c[2]))
    raise NeedsHost(k)


def array_literal(type_oid, text):
    """array_cell_to_sql_literal for an array cell that is still its source literal."""
    def lst(items):
        return b"[" + b", ".join(items) + b"]"
    if type_oid in arrays.JSON_ARRAY_OIDS:
        els = arrays.split_literal(type_oid, text)
        if any(e is not None and (len(e) > arrays.JSON_ELEM_MAX or not J.device_limits_ok(e)) for e in els):
            raise NeedsHost("a json element beyond the device's limits")
        return lst(b"NULL" if e is None else b"CAST(" + quote_literal(J.display(e)) + b" AS JSON)" for e in els)
    if type_oid in (1021, 1022):
        return lst(literal(e) for e in _float_elements(type_oid, text))
    if type_oid in ARRAY_OIDS:
        return lst(literal(e) for e in array_elements(type_oid, text))
    if type_oid == arrays.BYTEA_A:
        return lst(b"NULL" if e is None else b"from_hex('" + e.hex().upper().encode() + b"')" for e, _ in arrays.elements(type_oid, text))
    if type_oid in arrays.VAR_ARRAY_OIDS or arrays.is_string_array(type_oid, text):   # text-like, numeric, timetz: quote_literal of the Display
        return lst(b"NULL" if e is None else quote_literal(e) for e, _ in arrays.elements(type_oid, text))
    raise NeedsHost(type_oid)


def tuple_literal(cells):
    """table_row_to_sql_literal_ref."""
    return b"(" + b", ".join(literal(c) for c in cells) + b")"


def predicate(key_names, key_cells):
    """delete_predicate_from_row's text over (identity column, value) pairs; no pairs -> the empty string."""
    return b" AND ".join(quote_identifier(n) + (b" IS NULL" if c[0] == "Null" else b" = " + literal(c)) for n, c in zip(key_names, key_cells))


class Failure(Exception):
    """The batch's first problem: kind 'json' | 'host', the event, the column (host)."""

    def __init__(self, kind, event, column=None):
        super().__init__(kind, event, column)
        self.kind, self.event, self.column = kind, event, column


def choose(e, what, has_identity, copy=False):
    """What event `e` becomes for `what`: None (nothing), "host" (counted in n_host_rows), or (image, layout) with image "row" /
    "old_row" and layout "full" / "key"."""
    k = e["kind"]
    if k == "I":
        return ("row", "full") if what == TUPLES or copy else None
    if what == TUPLES:
        if k == "D":
            return None
        return "host" if e["partial"] else ("row", "full")
    if not has_identity:
        return "host"
    if e["old_kind"] == "Full":
        return ("old_row", "full")
    if e["old_kind"] == "Key":
        return ("old_row", "key")
    if k == "U" and not e["partial"]:
        return ("row", "full")                      # TableMutation::Replace
    return "host"


def event_records(events, slot_index, names, identity, what, copy=False, primary_key=None):
    """(records, event index of every record, events left to the host), or raises Failure: a json cell that is not JSON first (the
    reference's decode error), else the first record in event order the device hands back (its first column). `identity` /
    `primary_key`: 0 / 1 per column; a table-copy batch's predicates are over the primary-key columns."""
    recs, idx, host, fails = [], [], 0, []
    keyflags = primary_key if copy else identity
    key_cols = [i for i, f in enumerate(keyflags or []) if f]
    for i, e in enumerate(events):
        if e["kind"] not in "IUD" or e.get("schema_slot") != slot_index:
            continue
        ch = choose(e, what, bool(key_cols), copy)
        if ch is None:
            continue
        if ch == "host":
            host += 1
            continue
        cells = e[ch[0]]
        if what == TUPLES:
            look = list(enumerate(cells))
        elif ch[1] == "key":
            look = list(zip(key_cols, cells))
        else:
            look = [(c, cells[c]) for c in key_cols]
        first = None
        for col, c in look:
            try:
                literal(c)
            except arrays.JsonDecodeError:
                first = Failure("json", i)
                break
            except NeedsHost:
                first = first or Failure("host", i, col)
        if first:
            fails.append(first)
            continue
        recs.append(tuple_literal(cells) if what == TUPLES else predicate([names[c] for c, _ in look], [c for _, c in look]))
        idx.append(i)
    js = [f for f in fails if f.kind == "json"]
    if js or fails:
        raise (js or fails)[0]
    return recs, idx, host
