"""Device-side DuckLake SQL literals (etlg_batch_duckdb, etl_amd/csrc/rowformats.hip.h dl_row) byte for byte against tests/ducklake_literals.py
(restatement of crates/etl-destinations/src/ducklake/encoding.rs:366-612, batches.rs:1128-1316, 1477-1510 and core.rs:1824-1945), for
both `what` values, host and device output: every scalar class and NULLs, quote_literal's arms in cells and quote_identifier in column
names, Rust's float Display including the 300-byte texts, arrays of every element class as literals and typed, the update / delete
choices under each replica identity, the events left to the host (all but the Delete without an old image, which pgoutput cannot
say: that row of the table is checked on the restatement alone), NULL key cells, hand-backs, table-copy batches, synthetic streams.
Every parity case asserts status == ETLG_RB_OK; only the explicit hand-back cases expect ETLG_RB_NEEDS_HOST."""
import os

import numpy as np
import pytest

from etl_amd import abi, synth
from tests import ducklake_literals as DL
from tests import pgwire as W
from tests import scenarios as SC
from tests.test_gpu_rowbinary import NUMERICS, RB_COLS, TIMETZS, VAR_ARRAY_LITS, _both, _row, _stream

pytestmark = pytest.mark.gpu
EMU = os.environ.get("ETLG_SIMT_RUN") == "1"
WHATS = [abi.DL_TUPLES, abi.DL_PREDICATES]


def _read(ptr, nbytes):
    if not nbytes:
        return np.zeros(0, np.uint8)
    if EMU:
        import ctypes as C
        return np.frombuffer((C.c_uint8 * nbytes).from_address(ptr), dtype=np.uint8).copy()
    return abi.device_tensor(ptr, nbytes, 0).cpu().numpy()


def _check(hb, b, names, what, on_device=False, copy=False, slot=0, pk=None):
    ident = [c.identity for c in hb.slots[slot].cols]
    recs, idx, host = DL.event_records(hb.materialize(), slot, names, ident, what, copy=copy, primary_key=pk)
    r = b.duckdb(slot, names, what=what, on_device=on_device)
    assert r.status == abi.RB_OK, (r.status, int(r.view.host_event), r.view.host_column)
    assert r.n_rows == len(recs) and int(r.view.n_host_rows) == host, (r.n_rows, len(recs), int(r.view.n_host_rows), host)
    want = b"".join(recs)
    if on_device:
        assert r.view.on_device == 1
        ev = _read(r.view.row_event, 8 * len(recs)).view(np.uint64)
        offs = _read(r.view.row_offsets, 8 * (len(recs) + 1)).view(np.int64)
        got = _read(r.view.bytes, int(r.view.n_bytes)).tobytes()
    else:
        ev, offs = r.row_event(), r.row_offsets()
        got = r.bytes().tobytes() if want else b""
    assert np.array_equal(ev, np.array(idx, dtype=np.uint64))
    assert np.array_equal(np.diff(offs), np.array([len(x) for x in recs], dtype=np.int64))
    if got != want:
        for k, x in enumerate(recs):
            g = got[int(offs[k]):int(offs[k + 1])]
            assert g == x, (k, g[:400], x[:400])
    assert got == want
    r.close()
    return len(recs)


def _check_both(hb, b, names, **kw):
    return [_check(hb, b, names, w, on_device=od, **kw) for w in WHATS for od in (False, True)][::2]


ALL = RB_COLS + [("j", SC.JSONB, True, 0)]


def _allrow(**kw):
    j = kw.pop("j", '{"b": [1, 2.5e3, "x\\ty"], "a": null}')
    return _row(**kw) + [j]


@pytest.mark.parametrize("on_device", [False, True])
def test_every_scalar_class_and_nulls(on_device):
    names = [c[0] for c in ALL]
    rows = [_allrow(), _allrow(id="2", b="f", i2="-7", i4="-2147483648", o="4294967295", d="0001-01-01", t="00:00:00",
                               ts="1969-12-31 23:59:59.5", tstz="2026-01-02 03:04:05+02", f8="1e300", f4="-0.5", s="", by="\\x", j="[]"),
            _allrow(id="-9223372036854775808", d="9999-12-31", t="23:59:59.12", ts="2026-01-02 03:04:05", s="x" * 300, by="\\x" + "ab" * 200,
                    j='{"q": "it\'s", "e": "a\\"b"}'),
            [("4" if n == "id" else W.NULL) for n in names]]
    rows += [_allrow(id=str(10 + i), s="y" * (i * 13 % 200), t=f"01:02:{i % 60:02}.{i:06}", n=NUMERICS[i % len(NUMERICS)], tz=TIMETZS[i % len(TIMETZS)])
             for i in range(130)]
    # every column is an identity column here, so the predicates run every class and the NULLs (IS NULL) too
    msgs = [W.insert(42, r) for r in rows] + [W.delete(42, old=r) for r in rows]
    buf, offs = _stream(msgs)
    hb, b, d = _both(SC.simple_table(ALL, ident=[1] * len(ALL)), buf, offs)
    assert _check(hb, b, names, abi.DL_TUPLES, on_device) == len(rows)
    assert _check(hb, b, names, abi.DL_PREDICATES, on_device) == len(rows)
    r = b.duckdb(0, names, what=abi.DL_PREDICATES)
    last = r.bytes().tobytes()[int(r.row_offsets()[3]):int(r.row_offsets()[4])]
    assert last.startswith(b'"id" = 4 AND "') and last.count(b" IS NULL") == len(names) - 1
    r.close(); b.close(); d.close()


def test_quotes_backslashes_and_multibyte_text_in_cells_and_column_names():
    texts = ["it's", "back\\slash", "'\\'", "''", "\\", "plain", "é日本   ", "x" * 15 + "'" + "y" * 20, "z" * 33, "w" * 7 + "\\" + "v" * 40 + "'",
             "".join(chr(c) for c in range(1, 128)), "q" * 16 + "'", "", "a\"b", "\b\f\n\r\t"]
    names = ['i"d', "s\\t'\n\x01é", '""']
    cols = [(names[0], SC.INT8, False, 1), (names[1], 25, True, 1), (names[2], 114, True, 0)]
    js = ['{"k": "a\\"b"}', '"it\'s"', '"\\\\"', "[1, 2]"]
    msgs = [W.insert(42, [str(i), t, js[i % 4]]) for i, t in enumerate(texts)] + [W.delete(42, key=[str(i), t, W.NULL]) for i, t in enumerate(texts)]
    buf, offs = _stream(msgs)
    hb, b, d = _both(SC.simple_table(cols, ident=[1, 1, 0]), buf, offs)
    assert _check_both(hb, b, names) == [len(texts)] * 2
    r = b.duckdb(0, names)
    o = r.row_offsets()
    got = r.bytes().tobytes()
    assert got[:int(o[1])] == b"(0, 'it''s', CAST( E'{\"k\":\"a\\\\\"b\"}' AS JSON))"
    assert got[int(o[1]):int(o[2])] == b"(1,  E'back\\\\slash', CAST('\"it''s\"' AS JSON))"
    r.close()
    r = b.duckdb(0, names, what=abi.DL_PREDICATES)
    assert r.bytes().tobytes()[:int(r.row_offsets()[1])] == b'"i""d" = 0 AND "s\\t\'\n\x01\xc3\xa9" = \'it\'\'s\''
    r.close(); b.close(); d.close()


def test_float_layouts():
    f8 = ["0", "-0", "1", "0.1", "1e21", "1e22", "1e23", "4.9e-324", "-4.9e-324", "2.2250738585072014e-308", "1.7976931348623157e308",
          "-1.7976931348623157e308", "12.34", "1e-7", "1.5e-7", "123456789012345678", "1e15", "1e16", "NaN", "Infinity", "-Infinity", "5e-5", "-2.5"]
    f4 = ["0", "-0", "0.1", "1.5", "1e-45", "3.4028235e38", "-3.4028235e38", "1.17549435e-38", "16777216", "0.3", "1e10", "7e-6", "NaN",
          "Infinity", "-Infinity", "-inf", "123456.7", "8e-7", "2", "1e12", "1e13", "-3.25", "1e-7"]
    cols = [("id", SC.INT8, False, 1), ("x", SC.FLOAT8, True, 1), ("y", 700, True, 1)]
    msgs = [W.insert(42, [str(i), a, c]) for i, (a, c) in enumerate(zip(f8, f4))]
    msgs += [W.delete(42, key=[str(i), a, c]) for i, (a, c) in enumerate(zip(f8, f4))]
    buf, offs = _stream(msgs)
    hb, b, d = _both(SC.simple_table(cols, ident=[1, 1, 1]), buf, offs)
    assert _check_both(hb, b, ["id", "x", "y"]) == [len(f8)] * 2
    r = b.duckdb(0, ["id", "x", "y"])
    o = r.row_offsets()
    recs = [r.bytes().tobytes()[int(o[k]):int(o[k + 1])] for k in range(len(f8))]
    assert recs[1] == b"(1, -0, -0)" and recs[2] == b"(2, 1, 0.10000000149011612)" and recs[4].startswith(b"(4, 1" + b"0" * 21 + b", 0." + b"0" * 44 + b"14")
    assert recs[7].startswith(b"(7, 0." + b"0" * 323 + b"5, ") and recs[8].startswith(b"(8, -0." + b"0" * 323 + b"5, ")
    assert recs[10].startswith(b"(10, 17976931348623157" + b"0" * 292 + b", ")
    assert recs[18] == b"(18, CAST('NaN' AS DOUBLE), 2)" and recs[12] == b"(12, 12.34, CAST('NaN' AS FLOAT))"
    assert recs[19].startswith(b"(19, CAST('Infinity' AS DOUBLE), ") and recs[14].endswith(b", CAST('-Infinity' AS FLOAT))") and recs[13].endswith(b", CAST('Infinity' AS FLOAT))")
    r.close(); b.close(); d.close()


def test_invalid_json_beats_a_deferred_cell_in_an_earlier_row():
    from etl_amd.decoder import EtlError
    deferred = "50537618.817359292015891086651596749e82"            # a float text the fast rule leaves DEFERRED
    cols = [("id", SC.INT8, False, 1), ("f", SC.FLOAT8, True, 0), ("j", 114, True, 0)]
    buf, offs = _stream([W.insert(42, ["1", deferred, "{}"]), W.insert(42, ["2", "1", "{bad"]), W.insert(42, ["3", "1", "[1,"])])
    hb, b, d = _both(SC.simple_table(cols), buf, offs)
    with pytest.raises(DL.Failure) as fi:
        DL.event_records(hb.materialize(), 0, ["id", "f", "j"], [1, 0, 0], DL.TUPLES)
    assert (fi.value.kind, fi.value.event) == ("json", 2)
    with pytest.raises(EtlError) as ei:
        b.duckdb(0, ["id", "f", "j"])
    assert ei.value.code == abi.E_JSON and ei.value.frame_index == 2
    r = b.duckdb(0, ["id", "f", "j"], what=abi.DL_PREDICATES)      # Inserts give no predicates: nothing is looked at
    assert r.status == abi.RB_OK and r.n_rows == 0 and r.view.n_host_rows == 0
    r.close(); b.close(); d.close()
    cols = [("id", SC.INT8, False, 1), ("j", 3807, True, 0)]       # a json[] element
    buf, offs = _stream([W.insert(42, ["1", '{"1","[2"}'])])
    hb, b, d = _both(SC.simple_table(cols), buf, offs)
    with pytest.raises(EtlError) as ei:
        b.duckdb(0, ["id", "j"])
    assert ei.value.code == abi.E_JSON
    b.close(); d.close()


ARRAYS = {"bool": 1000, "int2": 1005, "int4": 1007, "int8": 1016, "oid": 1028, "float4": 1021, "float8": 1022,
          "date": 1182, "time": 1183, "timestamp": 1115, "timestamptz": 1185, "uuid": 2951}


def _both_finished(prime, buf, offs, finish):
    """_both, with the batch run through the finish pass on both sides (typed arrays: etlg_array_hdr) when `finish`."""
    if not finish:
        return _both(prime, buf, offs)
    from etl_amd.decoder import Decoder
    from oracle import oracle
    o, d = oracle.Oracle(), Decoder(0)
    prime(o)
    prime(d)
    rb = o.decode(buf, offs)
    assert rb.err_code == 0, rb.err_desc
    rb.finish()
    b = d.decode(buf, offs, flags=abi.F_OUTPUT_ON_DEVICE | abi.F_FINISH_CELLS)
    assert b.rc == 0, b.error
    return rb.host_batch(), b, d


@pytest.mark.parametrize("finish", [False, True])
def test_arrays_of_every_element_class(finish):
    """As source literals, and typed by the finish pass (ETLG_F_FINISH_CELLS): the same quote / backslash strings reach dl_quote from
    dl_array's unescaped characters and from dl_typed_array's contiguous bytes."""
    lits = {"bool": ["{t,f,NULL}", "{}"], "int2": ["{1,-2,32767,NULL}", "{-32768}"], "int4": ["{1,NULL,3}", "[0:2]={7,8,9}"],
            "int8": ["{9223372036854775807,-9223372036854775808,0}", "{NULL}"], "oid": ["{0,4294967295}", "{}"],
            "float4": ["{1.5,-0.25,3e10,1e-7,NULL,NaN,inf}", "{0,-0}"], "float8": ["{1.5,-2.25e-300,1e300,1e16,NULL,NaN,-Infinity}", "{0.1}"],
            "date": ["{2026-01-02,NULL,0001-01-01}", "{}"], "time": ["{12:30:45.123456,00:00:00}", "{NULL}"],
            "timestamp": ['{"2026-01-02 03:04:05.123456",NULL}', "{}"], "timestamptz": ['{"2026-01-02 05:04:05.000001+02",NULL}', "{}"],
            "uuid": ["{123e4567-e89b-12d3-a456-426614174000,NULL}", "{}"]}
    names = sorted(ARRAYS)
    cols = [("id", SC.INT8, False, 1)] + [(n, ARRAYS[n], True, 0) for n in names]
    rows = [[str(k)] + [lits[n][k] for n in names] for k in range(2)] + [["2"] + [W.NULL] * len(names)]
    buf, offs = _stream([W.insert(42, r) for r in rows] + [W.delete(42, old=r) for r in rows])
    hb, b, d = _both_finished(SC.simple_table(cols, ident=[1] * len(cols)), buf, offs, finish)
    if finish:
        assert any(c[0] == "Array" for e in hb.materialize() if e["kind"] == "I" for c in e["row"])
    assert _check_both(hb, b, ["id"] + names) == [len(rows)] * 2
    b.close(); d.close()
    onames = sorted(VAR_ARRAY_LITS)                                 # text-like / numeric / timetz / bytea elements, json[]
    vcols = [("id", SC.INT8, False, 1)] + [(f"a{o}", o, True, 0) for o in onames] + [("ja", 3807, True, 0)]
    jl = ['{"{\\"k\\": [1, 2]}",NULL,"3","\\"s\\\\u0001\\"","\\"it\'s\\""}', "{}", '{null,true,"\\"a\\\\\\\\b\\""}']
    lits = dict(VAR_ARRAY_LITS)
    lits[1009] = lits[1009] + ['{"it\'s","a\\\\b",\'}', '{"\\\\","\'\\\\\'"}']
    nr = max(len(v) for v in lits.values())
    vrows = [[str(k)] + [lits[o][k % len(lits[o])] for o in onames] + [jl[k % 3]] for k in range(nr)] + [[str(nr)] + [W.NULL] * (len(onames) + 1)]
    buf, offs = _stream([W.insert(42, r) for r in vrows] + [W.delete(42, old=r) for r in vrows])
    hb, b, d = _both_finished(SC.simple_table(vcols, ident=[1] * len(vcols)), buf, offs, finish)
    if finish:
        assert any(c[0] == "Array" and any(x[0] == "String" and b"\\" in x[1] for x in c[2]) for e in hb.materialize() if e["kind"] == "I" for c in e["row"])
    assert _check_both(hb, b, [c[0] for c in vcols]) == [len(vrows)] * 2
    b.close(); d.close()


@pytest.mark.parametrize("ident_name", ["Default", "Full", "Index"])
def test_updates_and_deletes_under_each_identity(ident_name):
    cols = [("a", SC.INT4, True, 0), ("k1", SC.INT8, False, 1), ("s", 25, True, 0), ("k2", 25, True, 1)]
    ident = {"Default": [0, 1, 0, 1], "Full": [1, 1, 1, 1], "Index": [0, 0, 1, 1]}[ident_name]
    msgs = []
    for i in range(60):
        k2 = W.NULL if i % 7 == 3 else "k'%d" % i                                                   # a NULL key cell -> IS NULL
        row = [str(i), str(i), "t%d" % i, k2]
        new = [str(i + 1), str(i), "u", k2]
        msgs.append(W.insert(42, row))
        key = [W.NULL if not f else v for f, v in zip(ident, row)]
        m = i % 8
        if m == 0:
            msgs.append(W.update(42, new))                                                          # no old image: Replace
        elif m == 1:
            msgs.append(W.update(42, new, old=row) if ident_name == "Full" else W.update(42, new, key=key))
        elif m == 2:
            msgs.append(W.update(42, [str(i), str(i), W.TOAST, k2]))                                # partial, no old image: host for both
        elif m == 3:
            msgs.append(W.delete(42, old=row))
        elif m == 4:
            msgs.append(W.delete(42, old=row) if ident_name == "Full" else W.delete(42, key=key))
        elif m == 5:
            msgs.append(W.update(42, [str(i), str(i), W.TOAST, k2], old=row) if ident_name == "Full" else W.update(42, [str(i), str(i), W.TOAST, k2], key=key))   # partial with an old image
        elif m == 6:
            msgs.append(W.update(42, new, old=row))
        else:
            msgs.append(W.delete(42, key=key) if ident_name != "Full" else W.delete(42, old=row))
    buf, offs = _stream(msgs)
    hb, b, d = _both(SC.simple_table(cols, ident=ident), buf, offs)
    names = [c[0] for c in cols]
    nt, np_ = _check_both(hb, b, names)
    n0, n1, n2, n3, n4, n5, n6, n7 = [len(range(k, 60, 8)) for k in range(8)]
    # (m == 5: the unchanged-toast column `s` is in the old image under Full and Index, so the decode completes the new row from it)
    full5 = n5 if ident_name != "Default" else 0
    assert nt == 60 + n0 + n1 + n6 + full5 and np_ == n0 + n1 + n3 + n4 + n5 + n6 + n7
    rt, rp = b.duckdb(0, names), b.duckdb(0, names, what=abi.DL_PREDICATES)
    assert rt.view.n_host_rows == n2 + n5 - full5 and rp.view.n_host_rows == n2
    assert b" IS NULL" in rp.bytes().tobytes()
    rt.close(); rp.close(); b.close(); d.close()


def test_events_without_an_old_image_and_slots_without_identity():
    cols = [("id", SC.INT8, False, 1), ("s", 25, True, 0)]
    # (pgoutput has no Delete without an image — the wire format cannot say it; that row of the table is covered by the restatement's
    # own test, tests/test_ducklake_kats.py test_row_choices)
    msgs = [W.insert(42, ["1", "a"]), W.update(42, ["1", "b"]), W.update(42, ["1", W.TOAST]), W.delete(42, old=["1", "a"])]
    buf, offs = _stream(msgs)
    hb, b, d = _both(SC.simple_table(cols), buf, offs)
    recs, idx, host = DL.event_records(hb.materialize(), 0, ["id", "s"], [1, 0], DL.PREDICATES)
    assert (recs, host) == ([b'"id" = 1', b'"id" = 1'], 1)
    assert DL.event_records(hb.materialize(), 0, ["id", "s"], [1, 0], DL.TUPLES)[2] == 1
    assert _check_both(hb, b, ["id", "s"]) == [2, 2]
    b.close(); d.close()
    hb, b, d = _both(SC.simple_table(cols, ident=[0, 0]), buf, offs)      # no identity columns: every candidate stays with the host
    recs, idx, host = DL.event_records(hb.materialize(), 0, ["id", "s"], [0, 0], DL.PREDICATES)
    assert (recs, host) == ([], 3)
    assert _check_both(hb, b, ["id", "s"]) == [2, 0]
    b.close(); d.close()


def test_hand_backs_name_the_event_and_column_and_predicates_look_at_key_columns_only():
    deferred = "50537618.817359292015891086651596749e82"
    cols = [("id", SC.INT8, False, 1), ("x", SC.FLOAT8, True, 0), ("j", 114, True, 0)]
    deep = "[" * 17 + "]" * 17                                         # json beyond json_display's limits
    msgs = [W.insert(42, ["1", "1.5", "{}"]), W.insert(42, ["2", "1", deep]), W.insert(42, ["3", deferred, deep]),
            W.delete(42, old=["3", deferred, deep])]
    buf, offs = _stream(msgs)
    hb, b, d = _both(SC.simple_table(cols), buf, offs)
    with pytest.raises(DL.Failure) as fi:
        DL.event_records(hb.materialize(), 0, ["id", "x", "j"], [1, 0, 0], DL.TUPLES)
    r = b.duckdb(0, ["id", "x", "j"])
    assert r.status == abi.RB_NEEDS_HOST and (int(r.view.host_event), r.view.host_column) == (fi.value.event, fi.value.column) == (2, 2)
    r.close()
    assert _check(hb, b, ["id", "x", "j"], abi.DL_PREDICATES) == 1     # the key column is fine: "id" = 3
    b.close(); d.close()
    hb, b, d = _both(SC.simple_table(cols, ident=[1, 1, 0]), buf, offs)  # ... and handed back when the DEFERRED cell is a key cell
    with pytest.raises(DL.Failure) as fi:
        DL.event_records(hb.materialize(), 0, ["id", "x", "j"], [1, 1, 0], DL.PREDICATES)
    r = b.duckdb(0, ["id", "x", "j"], what=abi.DL_PREDICATES)
    assert r.status == abi.RB_NEEDS_HOST and (int(r.view.host_event), r.view.host_column) == (fi.value.event, fi.value.column) == (4, 1)
    r.close(); b.close(); d.close()
    cols = [("id", SC.INT8, False, 1), ("a", 1007, True, 0)]          # a literal the walker does not take apart
    buf, offs = _stream([W.insert(42, ["1", "{1,2}"]), W.insert(42, ["2", "{1,x}"])])
    hb, b, d = _both(SC.simple_table(cols), buf, offs)
    r = b.duckdb(0, ["id", "a"])
    assert r.status == abi.RB_NEEDS_HOST and (int(r.view.host_event), r.view.host_column) == (2, 1)
    r.close(); b.close(); d.close()


def test_name_count_must_match_and_what_must_be_known():
    from etl_amd.decoder import EtlError
    buf, offs = _stream([W.insert(42, ["1", "x"])])
    hb, b, d = _both(SC.simple_table([("id", SC.INT8, False, 1), ("s", 25, True, 0)]), buf, offs)
    for args in ((["id"], abi.DL_TUPLES), (["id", "s", "t"], abi.DL_PREDICATES), (["id", "s"], 2), (["id", "s"], -1)):
        with pytest.raises(EtlError) as ei:
            b.duckdb(0, args[0], what=args[1])
        assert ei.value.kind == abi.InvalidArgument
    b.close(); d.close()


@pytest.mark.parametrize("pk", [[1, 0, 0, 1], [0, 0, 0, 0]])
def test_table_copy_batch(pk):
    from etl_amd.decoder import Decoder
    from oracle import oracle
    cols = [("id", SC.INT8, False, pk[0]), ("s", 25, True, pk[1]), ("f", SC.FLOAT8, True, pk[2]), ("k", 25, True, pk[3])]
    rows = [b"%d\ttext %d\\twith tab and ' quote\t%s\t%s\n" % (i, i, b"1.5" if i % 2 else b"\\N", b"\\N" if i % 5 == 0 else b"k%d" % i) for i in range(50)]
    o, d = oracle.Oracle(), Decoder(0)
    for t in (o, d):
        t.schema_put(42, 0, cols)
    so = o.table_ready(42, 0, [1] * len(cols), pk)
    sd = d.table_ready(42, 0, [1] * len(cols), pk)
    buf = np.frombuffer(b"".join(rows), dtype=np.uint8)
    offs = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint32)
    rb, gb = o.copy_decode(so, buf, offs), d.copy_decode(sd, buf, offs, flags=abi.F_OUTPUT_ON_DEVICE)
    assert gb.rc == 0 and rb.err_code == 0
    hb = rb.host_batch()
    assert _check_both(hb, gb, [c[0] for c in cols], copy=True, pk=pk) == [50, 50]
    r = gb.duckdb(0, [c[0] for c in cols], what=abi.DL_PREDICATES)
    if any(pk):
        assert r.bytes().tobytes().startswith(b'"id" = 0 AND "k" IS NULL"id" = 1 AND "k" = \'k1\'')
    else:
        assert r.n_rows == 50 and r.view.n_bytes == 0               # no primary key: the reference joins nothing
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
    nt, np_ = _check_both(rb.host_batch(), gb, names)
    assert nt > 0
    gb.close(); d.close()


@pytest.mark.parametrize("mk,cap", [(synth.cfg2, 64 << 20), (synth.cfg3, 8 << 20), (synth.cfg5, 8 << 20)])
def test_synthetic_streams(mk, cap):
    w = mk()
    buf, offs = w.fill((96 << 10) if EMU else cap)
    hb, b, d = _both(w.register, buf, offs)
    n = compared = 0
    for slot, sl in enumerate(hb.slots):
        t = [t for t in w.tables if t["rel_id"] == sl.table_id][0]
        names = [c[0] for c in w.schema_cols(t)]
        if len(names) == len(sl.cols):   # (a slot of an older schema version has fewer columns than the table's current names)
            compared += 1
            for what in WHATS:
                n += _check(hb, b, names, what, slot=slot, on_device=what == abi.DL_PREDICATES)
    assert compared >= 1 and n > 100, (compared, len(hb.slots), n)
    b.close(); d.close()
