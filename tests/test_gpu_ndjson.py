"""Device-side Snowflake NDJSON rows (etlg_batch_ndjson, etl_amd/csrc/rowformats.hip.h nd_row) byte for byte against tests/snowflake_ndjson.py
(restatement of crates/etl-destinations/src/snowflake/encoding.rs:57-280 and core.rs:345-438, 572-608, 683-699): every scalar class and
NULLs, serde_json's escapes in cells and column names, ryu's float layouts, the sink's encoding errors, arrays of every element class,
the update / delete row choices under each replica identity, DEFERRED cells, table-copy batches, typed arrays, synthetic streams."""
import json
import os

import numpy as np
import pytest

from etl_amd import abi, synth
from tests import pgwire as W
from tests import scenarios as SC
from tests import snowflake_ndjson as SN
from tests.test_gpu_rowbinary import NUMERICS, RB_COLS, TIMETZS, VAR_ARRAY_LITS, _both, _row, _stream

pytestmark = pytest.mark.gpu
EMU = os.environ.get("ETLG_SIMT_RUN") == "1"


def _read(ptr, nbytes):
    if not nbytes:
        return np.zeros(0, np.uint8)
    if EMU:
        import ctypes as C
        return np.frombuffer((C.c_uint8 * nbytes).from_address(ptr), dtype=np.uint8).copy()
    return abi.device_tensor(ptr, nbytes, 0).cpu().numpy()


def _check(hb, b, names, on_device=False, copy=False, slot=0):
    ident = [c.identity for c in hb.slots[slot].cols]
    rows, idx, host = SN.event_rows(hb.materialize(), slot, names, ident, copy=copy)
    r = b.ndjson(slot, names, on_device=on_device)
    assert r.status == abi.RB_OK and r.n_rows == len(rows) and int(r.view.n_host_rows) == host
    if on_device:
        assert r.view.on_device == 1
        ev = _read(r.view.row_event, 8 * len(rows)).view(np.uint64)
        offs = _read(r.view.row_offsets, 8 * (len(rows) + 1)).view(np.int64)
        got = _read(r.view.bytes, int(r.view.n_bytes)).tobytes()
    else:
        ev, offs = r.row_event(), r.row_offsets()
        got = r.bytes().tobytes() if rows else b""
    assert np.array_equal(ev, np.array(idx, dtype=np.uint64))
    assert np.array_equal(np.diff(offs), np.array([len(x) for x in rows], dtype=np.int64))
    want = b"".join(rows)
    if got != want:
        for k, x in enumerate(rows):
            g = got[int(offs[k]):int(offs[k + 1])]
            assert g == x, (k, g[:400], x[:400])
    for ln in got.split(b"\n")[:-1]:
        json.loads(ln)
    r.close()
    return len(rows)


def _fails(b, names):
    from etl_amd.decoder import EtlError
    with pytest.raises(EtlError) as ei:
        b.ndjson(0, names)
    return ei.value


ALL = RB_COLS + [("j", SC.JSONB, True, 0)]


def _allrow(**kw):
    j = kw.pop("j", '{"b": [1, 2.5e3, "x\\ty"], "a": null}')
    return _row(**kw) + [j]


@pytest.mark.parametrize("on_device", [False, True])
def test_every_scalar_class_and_nulls(on_device):
    names = [c[0] for c in ALL]
    rows = [_allrow(), _allrow(id="2", b="f", i2="-7", i4="-2147483648", o="4294967295", d="0001-01-01", t="00:00:00",
                               ts="1969-12-31 23:59:59.5", tstz="2026-01-02 03:04:05+02", f8="1e300", f4="-0.5", s="", by="\\x", j="[]"),
            _allrow(id="-9223372036854775808", d="9999-12-31", t="23:59:59.12", ts="2026-01-02 03:04:05", s="x" * 300, by="\\x" + "ab" * 200),
            [("4" if n == "id" else W.NULL) for n in names]]
    ok_num = [t for t in NUMERICS if t.strip().lower() not in ("nan", "infinity", "-infinity", "inf")]
    rows += [_allrow(id=str(10 + i), s="y" * (i * 13 % 200), t=f"01:02:{i % 60:02}.{i:06}", n=ok_num[i % len(ok_num)], tz=TIMETZS[i % len(TIMETZS)])
             for i in range(130)]
    buf, offs = _stream([W.insert(42, r) for r in rows])
    hb, b, d = _both(SC.simple_table(ALL), buf, offs)
    assert _check(hb, b, names, on_device) == len(rows)
    b.close(); d.close()


def test_escapes_in_cells_and_column_names():
    texts = ['a"b', "back\\slash", "\b\f\n\r\t", "\x01\x1f\x0b", "\x7f", "é日本   ", "/slash", "x" * 15 + '"' + "y" * 20,
             "z" * 33, "".join(chr(c) for c in range(1, 128)), "q" * 16 + "\n", "\x00"[1:]]
    names = ['i"d', "s\\t\n\x01é"]
    cols = [(names[0], SC.INT8, False, 1), (names[1], 25, True, 0)]
    buf, offs = _stream([W.insert(42, [str(i), t]) for i, t in enumerate(texts)])
    hb, b, d = _both(SC.simple_table(cols), buf, offs)
    assert _check(hb, b, names) == len(texts)
    r = b.ndjson(0, names)
    first = r.bytes().tobytes()[:int(r.row_offsets()[1])]
    assert first.startswith(b'{"i\\"d":0,"s\\\\t\\n\\u0001\xc3\xa9":"a\\"b",')
    r.close(); b.close(); d.close()


def test_float_layouts():
    f8 = ["0", "-0", "1e15", "1e16", "999999999999999.9", "9999999999999998", "12.34", "0.0001", "0.00001", "1e-6", "1.5e-7", "1.234e33",
          "4.9e-324", "2.2250738585072014e-308", "1.7976931348623157e308", "-2.5", "123456789012345678", "0.1", "1e22", "5e-5"]
    f4 = ["0", "-0", "1e12", "1e13", "9999999", "0.00001", "1e-6", "1e-7", "1.5", "3.4028235e38", "1e-45", "1.17549435e-38", "-3.25",
          "16777216", "0.3", "1e10", "7e-6", "123456.7", "8e-7", "2"]
    cols = [("id", SC.INT8, False, 1), ("x", SC.FLOAT8, True, 0), ("y", 700, True, 0)]
    buf, offs = _stream([W.insert(42, [str(i), a, c]) for i, (a, c) in enumerate(zip(f8, f4))])
    hb, b, d = _both(SC.simple_table(cols), buf, offs)
    assert _check(hb, b, ["id", "x", "y"]) == len(f8)
    r = b.ndjson(0, ["id", "x", "y"])
    lines = r.bytes().tobytes().split(b"\n")
    assert b'"x":1000000000000000.0,' in lines[2] and b'"x":1e16,' in lines[3] and b'"x":-0.0,"y":-0.0,' in lines[1]
    assert b'"x":5e-324,' in lines[12] and b'"y":1e13,' in lines[3] and b'"y":0.000001,' in lines[6] and b'"y":1e-7,' in lines[7]
    r.close(); b.close(); d.close()


@pytest.mark.parametrize("cls,text,detail", [
    (SC.FLOAT8, "NaN", "Snowflake does not support NaN/Infinity float values: NaN"),
    (SC.FLOAT8, "Infinity", "Snowflake does not support NaN/Infinity float values: inf"),
    (SC.FLOAT8, "-Infinity", "Snowflake does not support NaN/Infinity float values: -inf"),
    (700, "NaN", "Snowflake does not support NaN/Infinity float values: NaN"),
    (700, "-inf", "Snowflake does not support NaN/Infinity float values: -inf"),
    (SC.NUMERIC, "NaN", "Snowflake NUMBER does not support NaN"),
    (SC.NUMERIC, "Infinity", "Snowflake NUMBER does not support Infinity"),
    (SC.NUMERIC, "-Infinity", "Snowflake NUMBER does not support Infinity"),
    (1022, "{1.5,NaN}", "Snowflake does not support NaN/Infinity float values: NaN"),
    (1021, "{inf}", "Snowflake does not support NaN/Infinity float values: inf"),
    (1231, "{1,NaN}", "Snowflake NUMBER does not support NaN")])
def test_encoding_errors(cls, text, detail):
    cols = [("id", SC.INT8, False, 1), ("v", cls, True, 0)]
    ok = "{}" if cls in (1022, 1021, 1231) else "1"
    buf, offs = _stream([W.insert(42, ["1", ok]), W.insert(42, ["2", text]), W.insert(42, ["3", text])])
    hb, b, d = _both(SC.simple_table(cols), buf, offs)
    with pytest.raises(SN.Failure) as fi:
        SN.event_rows(hb.materialize(), 0, ["id", "v"], [1, 0])
    e = _fails(b, ["id", "v"])
    assert e.kind == abi.InvalidData and e.description == "Snowflake encoding error" and e.detail == "Encoding error: " + detail
    assert e.frame_index == fi.value.event == 2 and fi.value.detail == e.detail
    b.close(); d.close()


def test_invalid_json_beats_every_other_problem():
    cols = [("id", SC.INT8, False, 1), ("f", SC.FLOAT8, True, 0), ("j", 114, True, 0)]
    buf, offs = _stream([W.insert(42, ["1", "NaN", "{}"]), W.insert(42, ["2", "1", "{bad"]), W.insert(42, ["3", "1", "[1,"])])
    hb, b, d = _both(SC.simple_table(cols), buf, offs)
    e = _fails(b, ["id", "f", "j"])
    assert e.code == abi.E_JSON and e.frame_index == 2
    b.close(); d.close()
    cols = [("id", SC.INT8, False, 1), ("j", 3807, True, 0)]       # a json[] element
    buf, offs = _stream([W.insert(42, ["1", '{"1","[2"}'])])
    hb, b, d = _both(SC.simple_table(cols), buf, offs)
    assert _fails(b, ["id", "j"]).code == abi.E_JSON
    b.close(); d.close()


ARRAYS = {"bool": 1000, "int2": 1005, "int4": 1007, "int8": 1016, "oid": 1028, "float4": 1021, "float8": 1022,
          "date": 1182, "time": 1183, "timestamp": 1115, "timestamptz": 1185, "uuid": 2951}


def test_arrays_of_every_element_class():
    lits = {"bool": ["{t,f,NULL}", "{}"], "int2": ["{1,-2,32767,NULL}", "{-32768}"], "int4": ["{1,NULL,3}", "[0:2]={7,8,9}"],
            "int8": ["{9223372036854775807,-9223372036854775808,0}", "{NULL}"], "oid": ["{0,4294967295}", "{}"],
            "float4": ["{1.5,-0.25,3e10,1e-7,NULL}", "{0,-0}"], "float8": ["{1.5,-2.25e-300,1e300,1e16,NULL}", "{0.1}"],
            "date": ["{2026-01-02,NULL,0001-01-01}", "{}"], "time": ["{12:30:45.123456,00:00:00}", "{NULL}"],
            "timestamp": ['{"2026-01-02 03:04:05.123456",NULL}', "{}"], "timestamptz": ['{"2026-01-02 05:04:05.000001+02",NULL}', "{}"],
            "uuid": ["{123e4567-e89b-12d3-a456-426614174000,NULL}", "{}"]}
    names = sorted(ARRAYS)
    cols = [("id", SC.INT8, False, 1)] + [(n, ARRAYS[n], True, 0) for n in names]
    rows = [[str(k)] + [lits[n][k] for n in names] for k in range(2)] + [["2"] + [W.NULL] * len(names)]
    buf, offs = _stream([W.insert(42, r) for r in rows])
    hb, b, d = _both(SC.simple_table(cols), buf, offs)
    assert _check(hb, b, ["id"] + names) == len(rows)
    b.close(); d.close()
    onames = sorted(VAR_ARRAY_LITS)                                 # text-like / numeric / timetz / bytea elements
    okv = {o: [t for t in VAR_ARRAY_LITS[o] if not (o == 1231 and ("NaN" in t or "Inf" in t))] for o in onames}
    vcols = [("id", SC.INT8, False, 1)] + [(f"a{o}", o, True, 0) for o in onames] + [("ja", 3807, True, 0)]
    jl = ['{"{\\"k\\": [1, 2]}",NULL,"3","\\"s\\\\u0001\\""}', "{}", '{null,true}']
    nr = max(len(v) for v in okv.values())
    vrows = [[str(k)] + [okv[o][k % len(okv[o])] for o in onames] + [jl[k % 3]] for k in range(nr)] + [[str(nr)] + [W.NULL] * (len(onames) + 1)]
    buf, offs = _stream([W.insert(42, r) for r in vrows])
    hb, b, d = _both(SC.simple_table(vcols), buf, offs)
    assert _check(hb, b, [c[0] for c in vcols]) == len(vrows)
    b.close(); d.close()


@pytest.mark.parametrize("ident_name", ["Default", "Full", "Index"])
def test_updates_and_deletes_under_each_identity(ident_name):
    cols = [("a", SC.INT4, True, 0), ("k1", SC.INT8, False, 1), ("s", 25, True, 0), ("k2", 25, False, 1)]
    ident = {"Default": [0, 1, 0, 1], "Full": [1, 1, 1, 1], "Index": [0, 0, 1, 1]}[ident_name]
    msgs = []
    for i in range(60):
        row = [str(i), str(i), "t%d" % i, "k%d" % i]
        msgs.append(W.insert(42, row))
        key = [W.NULL if not f else v for f, v in zip(ident, row)]
        m = i % 6
        if m == 0:
            msgs.append(W.update(42, [str(i + 1), str(i), "u", "k%d" % i]))                         # no old image
        elif m == 1:
            msgs.append(W.update(42, [str(i + 1), str(i), "u", "k%d" % i], old=row) if ident_name == "Full" else W.update(42, [str(i + 1), str(i), "u", "k%d" % i], key=key))
        elif m == 2:
            msgs.append(W.update(42, [str(i), str(i), W.TOAST, "k%d" % i]))                         # partial (unchanged toast): host
        elif m == 3:
            msgs.append(W.delete(42, old=row))
        elif m == 4:
            msgs.append(W.delete(42, old=row) if ident_name == "Full" else W.delete(42, key=key))
        else:
            msgs.append(W.delete(42, key=key) if ident_name != "Full" else W.delete(42, old=row))
    buf, offs = _stream(msgs)
    hb, b, d = _both(SC.simple_table(cols, ident=ident), buf, offs)
    n = _check(hb, b, [c[0] for c in cols])
    assert n == 60 + 10 * 5 and b.ndjson(0, [c[0] for c in cols]).view.n_host_rows == 10
    b.close(); d.close()


def test_deferred_cells_and_ranking_between_rows():
    cols = [("id", SC.INT8, False, 1), ("x", SC.FLOAT8, True, 0), ("n", SC.NUMERIC, True, 0)]
    deferred = "50537618.817359292015891086651596749e82"            # a float text the fast rule leaves DEFERRED
    buf, offs = _stream([W.insert(42, ["1", "1.5", "1"]), W.insert(42, ["2", deferred, "NaN"]), W.insert(42, ["3", "NaN", "1"])])
    hb, b, d = _both(SC.simple_table(cols), buf, offs)
    r = b.ndjson(0, ["id", "x", "n"])                               # row 2: the DEFERRED column comes first
    assert r.status == abi.RB_NEEDS_HOST and (int(r.view.host_event), r.view.host_column) == (2, 1)
    r.close(); b.close(); d.close()
    buf, offs = _stream([W.insert(42, ["1", "NaN", "1"]), W.insert(42, ["2", deferred, "1"])])   # an earlier row's error wins
    hb, b, d = _both(SC.simple_table(cols), buf, offs)
    e = _fails(b, ["id", "x", "n"])
    assert e.frame_index == 1 and e.detail.endswith("float values: NaN")
    b.close(); d.close()
    buf, offs = _stream([W.insert(42, ["1", "1", "1"]), W.insert(42, ["2", "2", "NaN"]), W.insert(42, ["3", deferred, "1"])])
    hb, b, d = _both(SC.simple_table(cols), buf, offs)
    e = _fails(b, ["id", "x", "n"])
    assert e.frame_index == 2 and e.detail == "Encoding error: Snowflake NUMBER does not support NaN"
    b.close(); d.close()
    cols = [("id", SC.INT8, False, 1), ("a", 1007, True, 0)]         # a literal the walker does not take apart: handed back
    buf, offs = _stream([W.insert(42, ["1", "{1,2}"]), W.insert(42, ["2", "{1,x}"])])
    hb, b, d = _both(SC.simple_table(cols), buf, offs)
    r = b.ndjson(0, ["id", "a"])
    assert r.status == abi.RB_NEEDS_HOST and (int(r.view.host_event), r.view.host_column) == (2, 1)
    r.close(); b.close(); d.close()


def test_name_count_must_match():
    from etl_amd.decoder import EtlError
    buf, offs = _stream([W.insert(42, ["1", "x"])])
    hb, b, d = _both(SC.simple_table([("id", SC.INT8, False, 1), ("s", 25, True, 0)]), buf, offs)
    with pytest.raises(EtlError) as ei:
        b.ndjson(0, ["id"])
    assert ei.value.kind == abi.InvalidArgument
    b.close(); d.close()


def test_table_copy_batch_has_the_zero_token():
    from etl_amd.decoder import Decoder
    from oracle import oracle
    cols = [("id", SC.INT8, False, 1), ("s", 25, True, 0), ("f", SC.FLOAT8, True, 0)]
    rows = [b"%d\ttext %d\\twith tab\t%s\n" % (i, i, b"1.5" if i % 2 else b"\\N") for i in range(50)]
    o, d = oracle.Oracle(), Decoder(0)
    for t in (o, d):
        t.schema_put(42, 0, cols)
    so = o.table_ready(42, 0, [1] * len(cols), [1 if c[3] else 0 for c in cols])
    sd = d.table_ready(42, 0, [1] * len(cols), [1 if c[3] else 0 for c in cols])
    buf = np.frombuffer(b"".join(rows), dtype=np.uint8)
    offs = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint32)
    rb, gb = o.copy_decode(so, buf, offs), d.copy_decode(sd, buf, offs, flags=abi.F_OUTPUT_ON_DEVICE)
    assert gb.rc == 0 and rb.err_code == 0
    hb = rb.host_batch()
    assert _check(hb, gb, [c[0] for c in cols], copy=True) == 50
    r = gb.ndjson(0, [c[0] for c in cols])
    assert all(json.loads(x)["_cdc_sequence_number"] == SN.ZERO_TOKEN and json.loads(x)["_cdc_operation"] == "insert"
               for x in r.bytes().tobytes().split(b"\n")[:-1])
    r.close(); gb.close(); d.close()


@pytest.mark.parametrize("finish", [False, True])
def test_type_matrix_table(finish):
    from etl_amd.decoder import Decoder
    from oracle import oracle
    o, d = oracle.Oracle(), Decoder(0)
    buf, offs = synth.type_matrix_stream(40 if EMU else 300, mix=True)
    synth.type_matrix_register(o)
    synth.type_matrix_register(d)
    rb = o.decode(buf, offs)
    assert rb.err_code == 0
    if finish:
        rb.finish()
    gb = d.decode(buf, offs, flags=abi.F_NO_CONTROL | abi.F_OUTPUT_ON_DEVICE | (abi.F_FINISH_CELLS if finish else 0))
    assert gb.rc == 0, gb.error
    names = [c[0] for c in synth.TYPE_MATRIX_COLS]
    hb = rb.host_batch()
    try:
        want = SN.event_rows(hb.materialize(), 0, names, [c.identity for c in hb.slots[0].cols])
    except SN.Failure as f:
        r = gb.ndjson(0, names)
        assert f.kind == "host" and r.status == abi.RB_NEEDS_HOST and (int(r.view.host_event), r.view.host_column) == (f.event, f.column)
        r.close()
    else:
        assert _check(hb, gb, names) == len(want[0]) > 0
    gb.close(); d.close()


@pytest.mark.parametrize("mk,cap", [(synth.cfg2, 64 << 20), (synth.cfg3, 8 << 20), (synth.cfg5, 8 << 20)])
def test_synthetic_streams(mk, cap):
    w = mk()
    buf, offs = w.fill((96 << 10) if EMU else cap)
    hb, b, d = _both(w.register, buf, offs)
    n = 0
    for slot, sl in enumerate(hb.slots):
        t = [t for t in w.tables if t["rel_id"] == sl.table_id][0]
        names = [c[0] for c in w.schema_cols(t)]
        if len(names) == len(sl.cols):
            n += _check(hb, b, names, slot=slot)
    assert n > 100
    b.close(); d.close()
