"""TEST INFRASTRUCTURE — CPU restatement of the reference's Snowflake row encoder, for the parity tests of etlg_batch_ndjson
(etl_amd/csrc/rowformats.hip.h, nd_row). Never imported by the product path.

Follows crates/etl-destinations/src/snowflake/encoding.rs: serialize_row :57-72 (serde_json's compact map + '\\n'), RowSerializer
:82-92 (the columns, then _cdc_operation / _cdc_sequence_number), CellSerializer :94-140 and ArrayCellSerializer :186-224 (what every
Cell becomes), reject_non_finite :142-149 and serialize_pg_numeric :151-163 (the errors); snowflake/core.rs:345-438 and
snowflake_update_row / snowflake_delete_row :572-608 (which row an event becomes; key images keyed by the identity columns);
core.rs:683-699 (table-copy rows: insert under OffsetToken::zero); streaming/offset_token.rs:21-23 (the sequence number); error.rs:25-26,
52 (Error::Encoding's Display and kind).

serde_json and ryu are crates.io dependencies that are NOT under the reference; their published behaviour, restated:
  * strings: '"' and '\\\\' escaped, 0x08 0x0C \\n \\r \\t as \\b \\f \\n \\r \\t, other bytes below 0x20 as \\u00xx (lower-case hex),
    everything else raw (0x7F, all of UTF-8, U+2028 / U+2029 included);
  * f32 / f64 (serialize_f32 / serialize_f64 -> ryu's format32 / format64): the shortest round-trip digits d (n of them) with value
    d x 10^e, kk = n + e: e >= 0 and kk <= 16 -> digits, e zeros, ".0"; 0 < kk <= 16 -> a '.' after kk digits; -5 < kk <= 0 ->
    "0." + -kk zeros + digits; otherwise "De<kk-1>" / "D.DDDe<kk-1>" (f32: 13 and -6 < kk); zero "0.0", negative zero "-0.0".
    The digits come from Python's repr (f64, shortest round trip) and numpy's format_float_scientific(unique=True) (f32);
  * the error of a serializer's Error::custom displays as its message alone.
Display strings come from oracle/display.py, json values from oracle/json_display.py, array literals from oracle/arrays.py.

Works on the per-cell tuples of etl_amd.view.HostBatch.materialize()."""
import datetime as dt
import struct
from decimal import Decimal

from oracle import arrays
from oracle import json_display as J
from oracle.display import numeric_string, time_string, timetz_string
from oracle.rowbinary import ARRAY_OIDS, NeedsHost, array_elements

ZERO_TOKEN = "0000000000000000/0000000000000000"


class EncodingError(Exception):
    """Error::Encoding (snowflake/error.rs:25-26): kind InvalidData, description 'Snowflake encoding error', detail = str(self)."""


_ESC = {0x22: b'\\"', 0x5C: b"\\\\", 0x08: b"\\b", 0x0C: b"\\f", 0x0A: b"\\n", 0x0D: b"\\r", 0x09: b"\\t"}


def jstr(b):
    """serde_json's format_escaped_str over bytes."""
    if isinstance(b, str):
        b = b.encode()
    out = bytearray(b'"')
    for c in bytes(b):
        out += _ESC.get(c) or (b"\\u00%02x" % c if c < 0x20 else bytes([c]))
    return bytes(out) + b'"'


def layout(neg, digits, e, is32):
    """ryu pretty/mod.rs: the digits d (no leading / trailing zeros) with value d x 10^e."""
    n = len(digits)
    kk = n + e
    hi, lo = (13, -6) if is32 else (16, -5)
    s = "-" if neg else ""
    if e >= 0 and kk <= hi:
        return s + digits + "0" * e + ".0"
    if 0 < kk <= hi:
        return s + digits[:kk] + "." + digits[kk:]
    if lo < kk <= 0:
        return s + "0." + "0" * -kk + digits
    return s + digits[0] + ("." + digits[1:] if n > 1 else "") + "e" + str(kk - 1)


def _digits(text):
    t = Decimal(text).normalize().as_tuple()
    return "".join(map(str, t.digits)), t.exponent


def float_text(bits, is32):
    import numpy as np
    if is32:
        v = struct.unpack("<f", struct.pack("<I", bits))[0]
        neg = bool(bits >> 31)
    else:
        v = struct.unpack("<d", struct.pack("<Q", bits))[0]
        neg = bool(bits >> 63)
    if v != v:
        raise EncodingError("Encoding error: Snowflake does not support NaN/Infinity float values: NaN")
    if v in (float("inf"), float("-inf")):
        raise EncodingError("Encoding error: Snowflake does not support NaN/Infinity float values: " + ("-inf" if v < 0 else "inf"))
    if v == 0:
        return ("-0.0" if neg else "0.0").encode()
    d, e = _digits(np.format_float_scientific(np.float32(abs(v)), unique=True) if is32 else repr(abs(v)))
    return layout(neg, d, e, is32).encode()


def date_string(days_ce):
    d = dt.date.fromordinal(days_ce)
    return f"{d.year:04}-{d.month:02}-{d.day:02}"


def numeric(kind, sign, weight, scale, digits):
    if kind == 1:
        raise EncodingError("Encoding error: Snowflake NUMBER does not support NaN")
    if kind in (2, 3):
        raise EncodingError("Encoding error: Snowflake NUMBER does not support Infinity")
    return jstr(numeric_string(kind, sign, weight, scale, digits))


def value(c):
    """CellSerializer for a materialize() cell -> bytes. Raises EncodingError, NeedsHost, arrays.JsonDecodeError."""
    k = c[0]
    if k == "Null":
        return b"null"
    if k == "Bool":
        return b"true" if c[1] else b"false"
    if k in ("I16", "I32", "I64", "U32"):
        return str(c[1]).encode()
    if k in ("F32", "F64"):
        return float_text(c[1], k == "F32")
    if k == "Numeric":
        return numeric(*c[1:])
    if k == "Date":
        return jstr(date_string(c[1]))
    if k == "Time":
        return jstr(time_string(c[1], c[2]))
    if k == "Timestamp":
        return jstr(date_string(c[1]) + " " + time_string(c[2], c[3]))
    if k == "TimestampTz":
        return jstr(date_string(c[1]) + " " + time_string(c[2], c[3]) + "+00:00")
    if k == "TimeTz":
        return jstr(timetz_string(*c[1:]))
    if k == "Uuid":
        h = c[1].hex()
        return jstr(f"{h[:8]}-{h[8:12]}-{h[12:16]}-{h[16:20]}-{h[20:]}")
    if k == "Bytes":
        return jstr(bytes(c[1]).hex())
    if k == "String":
        return jstr(c[1])
    if k == "Array":                                   # a typed array (ETLG_F_FINISH_CELLS)
        return b"[" + b",".join(value(x) for x in c[2]) + b"]"
    if k == "Deferred" and c[1] in (114, 3802):        # Cell::Json: the Value itself
        try:
            J.parse(c[2])
        except ValueError:
            raise arrays.JsonDecodeError(c[2]) from None
        if not J.device_limits_ok(c[2]):
            raise NeedsHost("json beyond json_display's limits")
        return J.display(c[2])
    if k == "Deferred":
        return array_value(c[1], bytes(c[2]))
    raise NeedsHost(k)


def _float_elements(type_oid, text):
    """array_elements with NaN elements kept (the C++ oracle's repr has no bits for them)."""
    from oracle import oracle
    r = oracle.parse_text_cell(type_oid, text)
    if not r.startswith("Array["):
        raise NeedsHost(r)
    out = []
    for e in ([] if r == "Array[]" else r[6:-1].split(",")):
        if e == "NULL":
            out.append(("Null",))
        else:
            k, _, v = e.partition("(")
            v = v[:-1]
            out.append((k, (0x7FC00000 if k == "F32" else 0x7FF8000000000000) if v == "NaN" else int(v, 16)))
    return out


def array_value(type_oid, text):
    """ArrayCellSerializer for an array cell that is still its literal."""
    if type_oid in arrays.JSON_ARRAY_OIDS:
        els = arrays.split_literal(type_oid, text)
        if any(e is not None and (len(e) > arrays.JSON_ELEM_MAX or not J.device_limits_ok(e)) for e in els):
            raise NeedsHost("a json element beyond the device's limits")
        return b"[" + b",".join(b"null" if e is None else J.display(e) for e in els) + b"]"
    if type_oid in (1021, 1022):
        return b"[" + b",".join(value(e) for e in _float_elements(type_oid, text)) + b"]"
    if type_oid in ARRAY_OIDS:
        return b"[" + b",".join(value(e) for e in array_elements(type_oid, text)) + b"]"
    if type_oid == arrays.NUMERIC_A:
        out = []
        for e, _ in arrays.elements(type_oid, text):
            if e == b"NaN":
                raise EncodingError("Encoding error: Snowflake NUMBER does not support NaN")
            if e in (b"Infinity", b"-Infinity"):
                raise EncodingError("Encoding error: Snowflake NUMBER does not support Infinity")
            out.append(b"null" if e is None else jstr(e))
        return b"[" + b",".join(out) + b"]"
    if type_oid == arrays.BYTEA_A:
        return b"[" + b",".join(b"null" if e is None else jstr(e.hex()) for e, _ in arrays.elements(type_oid, text)) + b"]"
    if type_oid in arrays.VAR_ARRAY_OIDS or arrays.is_string_array(type_oid, text):   # text-like, timetz
        return b"[" + b",".join(b"null" if e is None else jstr(e) for e, _ in arrays.elements(type_oid, text)) + b"]"
    raise NeedsHost(type_oid)


def line(names, cells, op, seq):
    parts = [b"{"]
    for n, c in zip(names, cells):
        parts += [jstr(n), b":", value(c), b","]
    parts.append(b'"_cdc_operation":"' + op.encode() + b'","_cdc_sequence_number":"' + seq.encode() + b'"}\n')
    return b"".join(parts)


class Failure(Exception):
    """The batch's first problem: kind 'json' | 'encoding' | 'host', the event, the column (host), the detail (encoding)."""

    def __init__(self, kind, event, column=None, detail=None):
        super().__init__(kind, event, column, detail)
        self.kind, self.event, self.column, self.detail = kind, event, column, detail


def event_rows(events, slot_index, names, identity, copy=False):
    """(row bytes, event index of every row, events of the slot left to the host), or raises Failure: a json cell that is not JSON
    first (the reference's decode error), else the first row in event order that fails or that the device hands back (its first
    column). `identity`: 0 / 1 per column (the key image's columns, identity_column_schemas)."""
    rows, idx, host, fails = [], [], 0, []
    id_names = [n for n, f in zip(names, identity) if f]
    for i, e in enumerate(events):
        if e["kind"] not in "IUD" or e.get("schema_slot") != slot_index:
            continue
        if e["kind"] == "I":
            cols, cells, op = names, e["row"], "insert"
        elif e["kind"] == "U":
            if e["partial"]:
                host += 1
                continue
            cols, cells, op = names, e["row"], "update"
        else:
            if e["old_kind"] == "None":
                host += 1
                continue
            cols, cells, op = (names, e["old_row"], "delete") if e["old_kind"] == "Full" else (id_names, e["old_row"], "delete")
        seq = ZERO_TOKEN if copy else f"{e['commit_lsn']:016x}/{e['tx_ordinal']:016x}"
        first = None
        for n, c in zip(cols, cells):
            col = names.index(n)
            try:
                value(c)
            except arrays.JsonDecodeError:
                first = Failure("json", i)
                break
            except EncodingError as x:
                first = first or Failure("encoding", i, col, str(x))
            except NeedsHost:
                first = first or Failure("host", i, col)
        if first:
            fails.append(first)
            continue
        rows.append(line(cols, cells, op, seq)); idx.append(i)
    js = [f for f in fails if f.kind == "json"]
    if js or fails:
        raise (js or fails)[0]
    return rows, idx, host
