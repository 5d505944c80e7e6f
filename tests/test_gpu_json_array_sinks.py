"""One jsonb[] column through every hand-off that walks a json[] literal — etlg_batch_columns (ETLG_ROWS_PARSE_ARRAYS |
ETLG_ROWS_FORMAT_JSON), etlg_batch_iceberg, etlg_batch_rowbinary, etlg_batch_protobuf, etlg_batch_ndjson and etlg_batch_duckdb (tuples) —
with the same literals: an empty array, a NULL element, an element of exactly 256 unescaped bytes (its literal form is longer) and one
of 257, nesting of 16 and 17, an object of 64 and 65 members, an element that is not JSON, an integer beyond BigQuery's precision rule.
Every problem row once as its batch's only problem and once behind another problem in an earlier row, so that each sink's ranking of the
two is seen. The expectations are the per-sink restatements (oracle/rowbinary.py, oracle/protobuf.py, oracle/json_display.py,
tests/snowflake_ndjson.py, tests/ducklake_literals.py, oracle/arrays.py); what they leave open — which of two rows a batch reports — is
the rule the sinks share: an element that is not JSON is the reference's decode error and comes before everything a sink reports, else
the first row in event order; the Arrow lists fail for it only when no handed-back row precedes it (the consumer, finishing the
deferred rows in event order, meets the first problem first), else they hand that row back as well."""
import numpy as np
import pytest

from etl_amd import abi
from etl_amd.decoder import EtlError
from tests import pgwire as W
from tests import scenarios as SC
from tests.test_gpu_iceberg import _bits, _column
from tests.test_gpu_rowbinary import _both, _stream

pytestmark = pytest.mark.gpu

OID = 3807                                                                   # jsonb[]
COLS = [("id", SC.INT4, False, 1), ("ja", OID, True, 0)]
NAMES = ["id", "ja"]
RB_FLAGS = [0, 1, 0, 0]


def q(js):   # a JSON text as a quoted array element (Postgres escapes the quotes and the backslashes)
    return '"' + js.replace("\\", "\\\\").replace('"', '\\"') + '"'


def lit(*els):
    return "{" + ",".join("NULL" if e is None else q(e) for e in els) + "}"


def jstring(n):   # a JSON string of exactly n bytes with quotes and backslashes inside
    s = '"' + '\\"\\\\' * 10 + "x" * (n - 42) + '"'
    assert len(s) == n and len(q(s)) > n
    return s


def obj(n):
    return "{" + ",".join(f'"k{i:02}":{n - i}' for i in range(n)) + "}"


GOOD = [lit(), lit(jstring(256), '{"b":1,"a":[2,"x"]}'), lit("[" * 16 + "]" * 16), lit(obj(64)), lit("1", "true", "-0")]
PROBLEMS = {"null": lit('"a"', None, "2"), "long": lit("1", jstring(257)), "deep": lit("[" * 17 + "]" * 17), "wide": lit(obj(65)),
            "notjson": lit("[1]", "{"), "bigint": lit('{"n":18446744073709551616}')}
BEHIND = {"null": "long", "long": "notjson", "deep": "bigint", "wide": "null", "notjson": "long", "bigint": "deep"}   # problem -> the problem of an earlier row
CASES = [(None, None)] + [(p, None) for p in PROBLEMS] + [(p, e) for p, e in BEHIND.items()]


def _batch(problem, earlier):
    lits = GOOD[:3] + ([PROBLEMS[earlier]] if earlier else []) + GOOD[3:4] + ([PROBLEMS[problem]] if problem else []) + GOOD[4:]
    buf, offs = _stream([W.insert(42, [str(i + 1), t]) for i, t in enumerate(lits)])
    return _both(SC.simple_table(COLS), buf, offs)


def _first(ev, one):
    """The batch's report: `one(event)` -> the event's rows or raises; ("json", event) before everything, else the first failing row."""
    from oracle import arrays as OA
    from oracle import rowbinary as RB
    rows, fails = [], []
    for i, e in enumerate(ev):
        if e["kind"] != "I":
            continue
        try:
            rows += one(e)
        except OA.JsonDecodeError:
            fails.append(("json", i, None))
        except RB.NeedsHost:
            fails.append(("host", i, None))
        except Exception as x:   # noqa: BLE001  (the sink's own report: its class and text are compared below)
            fails.append(("sink", i, x))
    js = [f for f in fails if f[0] == "json"]
    return rows, (js or fails or [None])[0]


def _row_format(call, rows, fail, n_events):
    if fail is None:
        r = call()
        assert r.status == abi.RB_OK and r.n_rows == len(rows) == n_events and r.bytes().tobytes() == b"".join(rows)
        r.close()
    elif fail[0] == "host":
        r = call()
        assert r.status == abi.RB_NEEDS_HOST and (int(r.view.host_event), r.view.host_column) == (fail[1], 1)
        r.close()
    else:
        with pytest.raises(EtlError) as ei:
            call()
        assert ei.value.frame_index == fail[1]
        if fail[0] == "json":
            assert ei.value.code == abi.E_JSON and ei.value.description == "JSON deserialization failed"
        else:
            assert ei.value.kind == getattr(abi, type(fail[2]).__name__) and ei.value.detail == str(fail[2])


@pytest.mark.parametrize("problem,earlier", CASES)
def test_json_array_literals_through_every_sink(problem, earlier):
    from oracle import arrays as OA
    from oracle import protobuf as PB
    from oracle import rowbinary as RB
    from tests import ducklake_literals as DL
    from tests import snowflake_ndjson as SN
    hb, b, d = _batch(problem, earlier)
    ev = hb.materialize()
    ins = [i for i, e in enumerate(ev) if e["kind"] == "I"]
    n = len(ins)
    assert n < 50 and n == 5 + (problem is not None) + (earlier is not None)
    types = [c.type_class for c in hb.slots[0].cols]

    # ---- the row formats
    rows, fail = _first(ev, lambda e: RB.encode_events([e], 0, types, RB_FLAGS, abi.CH_MERGE_TREE, "PrimaryKey", None)[0])
    _row_format(lambda: b.rowbinary(0, RB_FLAGS, abi.CH_MERGE_TREE), rows, fail, n)
    rows, fail = _first(ev, lambda e: PB.event_rows([e], 0, COLS, "PrimaryKey")[0])
    _row_format(lambda: b.protobuf(0), rows, fail, n)
    for mod, one, call in ((SN, lambda: SN.event_rows(ev, 0, NAMES, [1, 0])[0], lambda: b.ndjson(0, NAMES)),
                           (DL, lambda: DL.event_records(ev, 0, NAMES, [1, 0], DL.TUPLES)[0], lambda: b.duckdb(0, NAMES, what=abi.DL_TUPLES))):
        try:
            rows, fail = one(), None
        except mod.Failure as f:
            assert f.kind in ("json", "host")
            rows, fail = [], (f.kind, f.event, None)
        _row_format(call, rows, fail, n)
    if problem in ("long", "deep", "wide", "notjson"):          # (the restatements do see the problem: no sink lets these rows through)
        assert fail is not None

    # ---- the Arrow lists: the elements' Display strings, a row beyond a lane's limits null and set in `deferred`
    want = []
    for i in ins:
        try:
            want.append([e for e, _ in OA.elements(OID, bytes(ev[i]["row"][1][2]))])
        except OA.NeedsHost:
            want.append("host")
        except OA.JsonDecodeError:
            want.append("json")
    first = {k: want.index(k) if k in want else n for k in ("host", "json")}
    for call, deferred in ((lambda: b.columns(0, parse_arrays=True, format_json=True), lambda c: np.unpackbits(c.host_arrays(1)[1], bitorder="little")[:n].astype(bool)),
                           (lambda: b.iceberg(0, parse_arrays=True, format_json=True), lambda c: _bits(c.column(1).deferred, n, False))):
        if first["json"] < first["host"]:
            with pytest.raises(EtlError) as ei:
                call()
            assert ei.value.code == abi.E_JSON and ei.value.frame_index == ins[first["json"]]
            continue
        c = call()
        assert c.n_rows == n and c.column(1).arrow_kind == abi.AK_LIST
        assert _column(c, 1) == [None if isinstance(w, str) else w for w in want]
        assert list(deferred(c)) == [isinstance(w, str) for w in want]
        c.close()
    b.close(); d.close()


MIXED = {"bad_then_long": lit("{", jstring(257)), "long_then_bad": lit(jstring(257), "{")}


@pytest.mark.parametrize("name", list(MIXED))
def test_a_too_long_and_a_malformed_element_in_one_literal(name):
    """An element that is not JSON and an element too long for a lane to look at in ONE literal. The restatements do not rank the two
    (they ask the reference's parser first, which fails on the malformed element: the error the host raises once the row is its own).
    The device's rule, written down here: a lane never looks at an element of more than 256 bytes — it may not be JSON either — so in
    the row formats the cell is the host's whichever of the two comes first; the Arrow lists take the first of the two in element
    order: the malformed element first is the decode error at its event, the long one first hands the row back."""
    lits = [GOOD[0], MIXED[name], GOOD[4]]
    buf, offs = _stream([W.insert(42, [str(i + 1), t]) for i, t in enumerate(lits)])
    hb, b, d = _both(SC.simple_table(COLS), buf, offs)
    ins = [i for i, e in enumerate(hb.materialize()) if e["kind"] == "I"]
    for call in (lambda: b.rowbinary(0, RB_FLAGS, abi.CH_MERGE_TREE), lambda: b.protobuf(0), lambda: b.ndjson(0, NAMES),
                 lambda: b.duckdb(0, NAMES, what=abi.DL_TUPLES)):
        r = call()
        assert r.status == abi.RB_NEEDS_HOST and (int(r.view.host_event), r.view.host_column) == (ins[1], 1)
        r.close()
    for call, deferred in ((lambda: b.columns(0, parse_arrays=True, format_json=True), lambda c: np.unpackbits(c.host_arrays(1)[1], bitorder="little")[:3].astype(bool)),
                           (lambda: b.iceberg(0, parse_arrays=True, format_json=True), lambda c: _bits(c.column(1).deferred, 3, False))):
        if name == "bad_then_long":
            with pytest.raises(EtlError) as ei:
                call()
            assert ei.value.code == abi.E_JSON and ei.value.frame_index == ins[1]
            continue
        c = call()
        assert _column(c, 1) == [[], None, [b"1", b"true", b"0"]] and list(deferred(c)) == [False, True, False]
        c.close()
    b.close(); d.close()
