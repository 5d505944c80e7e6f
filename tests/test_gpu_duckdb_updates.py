"""Device-side DuckLake partial Updates (etlg_batch_duckdb with ETLG_DL_UPDATES, etl_amd/csrc/columns.hip dl_selected, rowformats.hip.h dl_row) against
tests/ducklake_updates.py (restatement of ducklake/core.rs:846-939, 1846-1913 and batches.rs:1179-1190, 1229-1399): the bytes of both
records of every partial Update, row_event, row_offsets, col_ends and n_host_rows, host and device output — under each identity shape,
across the 256-event workgroups of the select kernels, for tables of 1 / 3 / 7 columns written with 1, 2 and 4 lanes per row and every
pattern of leading MISSING columns, for every cell class, through the unstaged path of the byte pass, with the hand-backs and errors,
and with the two older `what` values counting the same events for the host as before.
Every parity case asserts status == ETLG_RB_OK; only the explicit hand-back cases expect ETLG_RB_NEEDS_HOST."""
import os

import numpy as np
import pytest

from etl_amd import abi
from tests import ducklake_literals as DL
from tests import ducklake_updates as DU
from tests import pgwire as W
from tests import scenarios as SC
from tests.test_gpu_duckdb import ALL, _allrow, _both_finished, _read
from tests.test_gpu_duckdb import _check as _check_old
from tests.test_gpu_rowbinary import NUMERICS, TIMETZS, VAR_ARRAY_LITS, _both, _stream

pytestmark = pytest.mark.gpu
T = W.TOAST


def _check(hb, b, names, on_device=False, slot=0):
    ident = [c.identity for c in hb.slots[slot].cols]
    recs, idx, ends, host = DU.update_records(hb.materialize(), slot, names, ident)
    r = b.duckdb(slot, names, what=abi.DL_UPDATES, on_device=on_device)
    assert r.status == abi.RB_OK, (r.status, int(r.view.host_event), r.view.host_column)
    assert r.n_rows == len(recs) and int(r.view.n_host_rows) == host, (r.n_rows, len(recs), int(r.view.n_host_rows), host)
    want, nc = b"".join(recs), len(names)
    if on_device:
        assert r.view.on_device == 1
        ev = _read(r.view.row_event, 8 * len(recs)).view(np.uint64)
        offs = _read(r.view.row_offsets, 8 * (len(recs) + 1)).view(np.int64)
        got = _read(r.view.bytes, int(r.view.n_bytes)).tobytes()
        ce = _read(r.col_ends_ptr(), 4 * len(recs) * nc).view(np.uint32).reshape(len(recs), nc)
    else:
        ev, offs, ce = r.row_event(), r.row_offsets(), r.col_ends()
        got = r.bytes().tobytes() if want else b""
    assert np.array_equal(ev, np.array(idx, dtype=np.uint64))
    assert np.array_equal(np.diff(offs), np.array([len(x) for x in recs], dtype=np.int64))
    if got != want:
        for k, x in enumerate(recs):
            g = got[int(offs[k]):int(offs[k + 1])]
            assert g == x, (k, g[:400], x[:400])
    assert got == want
    assert np.array_equal(ce, np.array(ends, dtype=np.uint32).reshape(len(recs), nc))
    r.close()
    return len(recs), host


def _check_all(hb, b, names, slot=0):
    """Both outputs of ETLG_DL_UPDATES, and the two older `what`s on the same batch: they count the partial Updates as before."""
    out = [_check(hb, b, names, on_device=od, slot=slot) for od in (False, True)]
    assert out[0] == out[1]
    for what in (abi.DL_TUPLES, abi.DL_PREDICATES):
        _check_old(hb, b, names, what, slot=slot)
    ev = [e for e in hb.materialize() if e["kind"] == "U" and e.get("schema_slot") == slot and e["partial"]]
    rt, rp = b.duckdb(slot, names, what=abi.DL_TUPLES), b.duckdb(slot, names, what=abi.DL_PREDICATES)
    has_ident = any(c.identity for c in hb.slots[slot].cols)
    assert int(rt.view.n_host_rows) == len(ev)
    if has_ident:
        assert int(rp.view.n_host_rows) == sum(1 for e in ev if e["old_kind"] == "None")
    rt.close(); rp.close()
    return out[0]


COLS5 = [("a", SC.INT4, True, 0), ("k1", SC.INT8, False, 1), ("s", 25, True, 0), ("k2", 25, True, 1), ('bi"g', 25, True, 0)]
OTHER = [("id", SC.INT8, False, 1), ("t", 25, True, 0)]


def _two_tables(ident):
    p1, p2 = SC.simple_table(COLS5, ident=ident), SC.simple_table(OTHER, table_id=43)

    def prime(t):
        p1(t)
        p2(t)
    return prime


def _mixed(ident, n=150):
    """Partial Updates of table 42 among Inserts, Deletes, full Updates and the events of table 43 (partial Updates too)."""
    msgs = []
    for i in range(n):
        k2 = W.NULL if i % 7 == 3 else "k'%d" % i                              # a NULL key cell -> IS NULL
        a = W.NULL if i % 5 == 1 else str(i)                                    # a NULL SET cell -> = NULL
        row = [str(i), str(i), "t%d" % i, k2, "big %d" % i]
        key = [W.NULL if not f else v for f, v in zip(ident, row)]
        m = i % 10
        if m == 0:
            msgs.append(W.insert(42, row))
        elif m in (1, 2, 3):
            msgs.append(W.update(42, [a, str(i), "u\\%d" % i, k2, T]))          # the ordinary Update of a table with a big column
        elif m == 4:
            msgs.append(W.update(42, [a, str(i), "v", k2, T], key=key) if any(ident) else W.update(42, [a, str(i), "v", k2, T]))
        elif m == 5:
            msgs.append(W.update(42, [a, str(i), T, T, T]))                     # an identity column (k2) sent as TOAST
        elif m == 6:
            msgs.append(W.update(42, row, old=row))
        elif m == 7:
            msgs.append(W.delete(42, old=row))
        elif m == 8:
            msgs.append(W.update(43, [str(i), T]))
        else:
            msgs.append(W.update(42, [T, str(i), T, k2, T]))                    # only the key present
    return msgs


@pytest.mark.parametrize("ident_name", ["Default", "Index", "None"])
def test_identity_shapes_among_other_events(ident_name):
    ident = {"Default": [0, 1, 0, 1, 0], "Index": [0, 0, 1, 1, 0], "None": [0, 0, 0, 0, 0]}[ident_name]
    buf, offs = _stream(_mixed(ident))
    hb, b, d = _both(_two_tables(ident), buf, offs)
    names = [c[0] for c in COLS5]
    n, host = _check_all(hb, b, names)
    part = [e for e in hb.materialize() if e["kind"] == "U" and e.get("schema_slot") == 0 and e["partial"]]
    assert len(part) >= 75
    if ident_name == "None":
        assert (n, host) == (0, len(part))                                      # "DuckLake update requires a replica identity"
    else:
        # m == 5 misses k2: without an old image the host's under both identities; m == 9 misses s: the host's under Index
        assert host == 15 * (2 if ident_name == "Index" else 1) and n == 2 * (len(part) - host)
        r = b.duckdb(0, names, what=abi.DL_UPDATES)
        got, o = r.bytes().tobytes(), r.row_offsets()
        assert b'"a" = NULL' in got and b'"k2" IS NULL' in got and b'"bi""g"' not in got and b" E'u\\\\" in got
        assert got[:int(o[2])] == (b'"a" = NULL, "k1" = 1, "s" =  E\'u\\\\1\', "k2" = \'k\'\'1\'' +
                                   (b'"k1" = 1 AND "k2" = \'k\'\'1\'' if ident_name == "Default" else b'"s" =  E\'u\\\\1\' AND "k2" = \'k\'\'1\''))
        r.close()
    assert _check_all(hb, b, ["id", "t"], slot=1) == (2 * 15, 0)               # the second table's own partial Updates
    b.close(); d.close()


def test_key_image_that_does_not_hold_the_toasted_column():
    ident = [0, 0, 1, 1, 0]
    msgs = []
    for i in range(40):
        row = [str(i), str(i), "s%d" % i, W.NULL if i % 4 == 1 else "k%d" % i, "x"]
        key = [W.NULL if not f else v for f, v in zip(ident, row)]
        msgs.append(W.update(42, [str(i + 1), str(i), "new s%d" % i, "new k", T], key=key))   # the key changes: the predicate is the OLD key
    buf, offs = _stream(msgs)
    hb, b, d = _both(SC.simple_table(COLS5, ident=ident), buf, offs)
    names = [c[0] for c in COLS5]
    assert _check_all(hb, b, names) == (80, 0)
    r = b.duckdb(0, names, what=abi.DL_UPDATES)
    got, o = r.bytes().tobytes(), r.row_offsets()
    assert got[:int(o[2])] == b'"a" = 1, "k1" = 0, "s" = \'new s0\', "k2" = \'new k\'' + b'"s" = \'s0\' AND "k2" = \'k0\''
    assert got[int(o[3]):int(o[4])] == b'"s" = \'s1\' AND "k2" IS NULL'
    assert r.col_ends()[0].tolist() == [7, 17, 33, 49, 49] and r.col_ends()[1].tolist() == [0, 0, 10, 26, 26]
    r.close(); b.close(); d.close()


@pytest.mark.parametrize("parts", [1, 2, 4])
def test_names_with_quotes_in_set_and_predicate_records(parts):
    """quote_double_identifier in both records: a name with '"' on present SET columns and on both identity columns, the bytes and the
    col_ends around them (the quoted name is longer than the name + 2), written with 1, 2 and 4 lanes per row."""
    cols = [("k", SC.INT8, False, 1), ("a", SC.INT4, True, 0), ("s", 25, True, 1), ("t", 25, True, 0), ("big", 25, True, 0)]
    names = ['k"y', 'x""', '"', "pl", 'big"']
    quoted = [b'"k""y"', b'"x"""""', b'""""', b'"pl"', b'"big"""']
    assert [DL.quote_identifier(n) for n in names] == quoted
    os.environ["ETLG_RB_PARTS"] = str(parts)
    try:
        msgs = [W.update(42, [str(i), T if i % 3 == 1 else "7", "v", W.NULL if i % 3 == 2 else "w", T]) for i in range(45)]
        buf, offs = _stream(msgs)
        hb, b, d = _both(SC.simple_table(cols, ident=[1, 0, 1, 0, 0]), buf, offs)
        assert _check_all(hb, b, names) == (90, 0)
        for od in (False, True):
            r = b.duckdb(0, names, what=abi.DL_UPDATES, on_device=od)
            if od:
                o = _read(r.view.row_offsets, 8 * 91).view(np.int64)
                got = _read(r.view.bytes, int(r.view.n_bytes)).tobytes()
                ce = _read(r.col_ends_ptr(), 4 * 90 * 5).view(np.uint32).reshape(90, 5)
            else:
                o, got, ce = r.row_offsets(), r.bytes().tobytes(), r.col_ends()
            rec = [got[int(o[k]):int(o[k + 1])] for k in range(6)]
            assert rec[0] == b'"k""y" = 0, "x""""" = 7, """" = \'v\', "pl" = \'w\'' and rec[1] == b'"k""y" = 0 AND """" = \'v\''
            assert ce[0].tolist() == [10, 23, 35, 47, 47] and ce[1].tolist() == [10, 10, 25, 25, 25]
            assert rec[2] == b'"k""y" = 1, """" = \'v\', "pl" = \'w\'' and ce[2].tolist() == [10, 10, 22, 34, 34]       # the second column MISSING
            assert rec[4] == b'"k""y" = 2, "x""""" = 7, """" = \'v\', "pl" = NULL' and ce[4].tolist() == [10, 23, 35, 48, 48]
            assert rec[3] == b'"k""y" = 1 AND """" = \'v\'' and b'"big"""' not in got
            # the literal hash_partial_table_row_ref takes: the piece minus its separator and len(quoted name) + 3
            lits = [rec[0][(int(ce[0][c - 1]) + 2 if c else 0) + len(quoted[c]) + 3:int(ce[0][c])] for c in range(4)]
            assert lits == [b"0", b"7", b"'v'", b"'w'"]
            r.close()
        b.close(); d.close()
    finally:
        os.environ.pop("ETLG_RB_PARTS", None)


def test_partial_updates_across_the_select_kernels_workgroups():
    """More than two workgroups of 256 events in the select kernels: partial Updates on both sides of every boundary (events 255 / 256 /
    511 / 512 among them), Inserts and host rows in between so that the row an event starts at is not twice its index."""
    cols = [("id", SC.INT8, False, 1), ("v", SC.INT4, True, 0), ("big", 25, True, 0)]
    msgs = []
    for i in range(640):
        if i % 97 == 13:
            msgs.append(W.insert(42, [str(i), "1", "b"]))
        elif i % 101 == 50:
            msgs.append(W.update(42, [T, str(i), T]))                           # the key is MISSING: the host's
        else:
            msgs.append(W.update(42, [str(i), W.NULL if i % 9 == 0 else str(-i), T]))
    buf, offs = _stream(msgs)
    hb, b, d = _both(SC.simple_table(cols), buf, offs)
    ev = hb.materialize()
    for k in (255, 256, 257, 511, 512, 513):
        assert ev[k]["kind"] == "U" and ev[k]["partial"]
    n, host = _check_all(hb, b, ["id", "v", "big"])
    assert host == 6 and n == 2 * (640 - 7 - 6)
    b.close(); d.close()


WIDE = [("c%d" % i, 25 if i % 2 else SC.INT4, True, 0) for i in range(6)] + [("key", SC.INT8, False, 1)]


@pytest.mark.parametrize("parts", [1, 2, 4])
def test_table_widths_and_missing_patterns(parts):
    """1 / 3 / 7 columns (the counting pass notes 1 / 2 / 4 pieces, the byte pass writes a row with up to `parts` lanes): a lane whose
    columns start behind MISSING ones only must not write the ", "."""
    os.environ["ETLG_RB_PARTS"] = str(parts)
    try:
        # one column: a partial row of it has no cell at all — the host's; with a key image the decode completes the row
        buf, offs = _stream([W.insert(42, ["1"])] + [W.update(42, [T]) for _ in range(5)] + [W.update(42, [T], key=["1"])])
        hb, b, d = _both(SC.simple_table([("id", SC.INT8, False, 1)]), buf, offs)
        assert _check_all(hb, b, ["id"]) == (0, 5)
        b.close(); d.close()
        for cols in ([("a", 25, True, 0), ("b", SC.INT4, True, 0), ("key", SC.INT8, False, 1)], WIDE,
                     [("key", SC.INT8, False, 1)] + WIDE[:6]):
            nc, kpos = len(cols), [c[0] for c in cols].index("key")
            msgs = []
            for i in range(70):
                row = [str(i) if c[1] != 25 else "t'%d" % i for c in cols]
                if i % 6 == 5:
                    row[[c for c in range(nc) if c != kpos][(i // 6) % (nc - 1)]] = W.NULL
                # MISSING: the first one, the first two, ..., all but the last; one in the middle; every second; everything but the key
                pat = i % (nc + 2)
                miss = set(range(pat + 1)) if pat < nc - 1 else {nc // 2} if pat == nc - 1 else set(range(0, nc, 2)) if pat == nc else set(range(nc))
                miss.discard(kpos)
                if pat < nc - 1 and kpos == 0:
                    miss = {c + 1 for c in range(pat + 1)} - {nc}               # key first: columns 1 .. are MISSING
                msgs.append(W.update(42, [T if c in miss else v for c, v in enumerate(row)]))
            buf, offs = _stream(msgs)
            hb, b, d = _both(SC.simple_table(cols), buf, offs)
            ev = [e for e in hb.materialize() if e["kind"] == "U"]
            only_key = [e for e in ev if sum(1 for c in e["row"] if c[0] != "Missing") == 1]
            assert only_key and all(e["partial"] for e in ev)
            if kpos:
                assert any(all(c[0] == "Missing" for c in e["row"][:nc - 1]) for e in ev)
                assert any(e["row"][0][0] == "Missing" and e["row"][1][0] != "Missing" for e in ev) and any(
                    e["row"][0][0] == e["row"][1][0] == "Missing" and (nc < 4 or e["row"][2][0] != "Missing") for e in ev)
            assert _check_all(hb, b, [c[0] for c in cols]) == (140, 0)
            b.close(); d.close()
    finally:
        os.environ.pop("ETLG_RB_PARTS", None)


@pytest.mark.parametrize("finish", [False, True])
def test_every_cell_class_in_set_columns(finish):
    cols = ALL + [('b"ig', 25, True, 0)]
    names = [c[0] for c in cols]
    rows = [_allrow(), _allrow(id="2", b="f", i2="-7", i4="-2147483648", o="4294967295", d="0001-01-01", t="00:00:00",
                               ts="1969-12-31 23:59:59.5", tstz="2026-01-02 03:04:05+02", f8="1e300", f4="-0.5", s="", by="\\x", j="[]"),
            _allrow(id="-9223372036854775808", d="9999-12-31", t="23:59:59.12", ts="2026-01-02 03:04:05", s="x" * 300, by="\\x" + "ab" * 200,
                    j='{"q": "it\'s", "e": "a\\"b"}'),
            [("4" if n == "id" else W.NULL) for n in names[:-1]]]
    rows += [_allrow(id=str(10 + i), s="y\\" * (i * 13 % 90), t=f"01:02:{i % 60:02}.{i:06}", n=NUMERICS[i % len(NUMERICS)], tz=TIMETZS[i % len(TIMETZS)],
                     f8=["NaN", "1e21", "-0", "4.9e-324"][i % 4]) for i in range(60)]
    buf, offs = _stream([W.update(42, r + [T]) for r in rows])
    hb, b, d = _both_finished(SC.simple_table(cols), buf, offs, finish)
    assert _check_all(hb, b, names) == (2 * len(rows), 0)
    r = b.duckdb(0, names, what=abi.DL_UPDATES)
    rec = r.bytes().tobytes()[int(r.row_offsets()[6]):int(r.row_offsets()[7])]
    assert rec.startswith(b'"id" = 4, "b" = NULL, ') and rec.count(b" = NULL") == len(names) - 2 and b'b""ig' not in rec
    r.close(); b.close(); d.close()
    onames = sorted(VAR_ARRAY_LITS)                                             # arrays of every var-len element class, json[], fixed-width ones
    acols = [("id", SC.INT8, False, 1)] + [(f"a{o}", o, True, 0) for o in onames] + [("ja", 3807, True, 0), ("i4a", 1007, True, 0), ("f8a", 1022, True, 0), ("big", 25, True, 0)]
    jl = ['{"{\\"k\\": [1, 2]}",NULL,"3","\\"s\\\\u0001\\"","\\"it\'s\\""}', "{}", '{null,true,"\\"a\\\\\\\\b\\""}']
    lits = dict(VAR_ARRAY_LITS)
    lits[1009] = lits[1009] + ['{"it\'s","a\\\\b",\'}', '{"\\\\","\'\\\\\'"}']
    nr = max(len(v) for v in lits.values())
    arows = [[str(k)] + [lits[o][k % len(lits[o])] for o in onames] + [jl[k % 3], ["{1,NULL,3}", "{}"][k % 2], ["{1.5,NaN,NULL,-Infinity}", "{0.1}"][k % 2]] for k in range(nr)]
    arows.append([str(nr)] + [W.NULL] * (len(acols) - 2))
    buf, offs = _stream([W.update(42, r + [T]) for r in arows])
    hb, b, d = _both_finished(SC.simple_table(acols), buf, offs, finish)
    if finish:
        assert any(c[0] == "Array" for e in hb.materialize() if e["kind"] == "U" for c in e["row"])
    assert _check_all(hb, b, [c[0] for c in acols]) == (2 * len(arows), 0)
    b.close(); d.close()


def test_records_beyond_the_lds_image_take_the_unstaged_path():
    """The records of a workgroup — 64 rows of the four-column table (four lanes per row), 128 of the three-column one (two lanes) — are
    beyond the 32 KiB image: the lanes write to global memory themselves; the last workgroup's few rows are staged."""
    cols = [("id", SC.INT8, False, 1), ("s", 25, True, 0), ("t", 25, True, 0), ("big", 25, True, 0)]
    msgs = [W.update(42, [str(i), chr(97 + i % 26) * (600 + i), ("'%d\\" % i) * 150, T]) for i in range(70)]
    cols3 = cols[:2] + cols[3:]
    for cc, mm in ((cols, msgs), (cols3, [W.update(42, [str(i), chr(97 + i % 26) * (600 + i), T]) for i in range(70)])):
        buf, offs = _stream(mm)
        hb, b, d = _both(SC.simple_table(cc), buf, offs)
        r = b.duckdb(0, [c[0] for c in cc], what=abi.DL_UPDATES)
        assert int(r.row_offsets()[128]) > 32 * 1024                            # (128 rows: the most a workgroup takes here unless one lane writes a row)
        r.close()
        assert _check_all(hb, b, [c[0] for c in cc]) == (140, 0)
        b.close(); d.close()


def test_hand_backs_and_errors():
    from etl_amd.decoder import EtlError
    deferred = "50537618.817359292015891086651596749e82"                        # a float text the fast rule leaves DEFERRED
    cols = [("id", SC.INT8, False, 1), ("f", SC.FLOAT8, True, 0), ("j", 114, True, 0), ("big", 25, True, 0)]
    names = [c[0] for c in cols]
    ok = [W.update(42, [str(i), "1.5", "{}", T]) for i in range(3)]
    buf, offs = _stream(ok + [W.update(42, ["7", deferred, "[1]", T]), W.update(42, ["8", deferred, "{}", T])])
    hb, b, d = _both(SC.simple_table(cols), buf, offs)
    with pytest.raises(DL.Failure) as fi:
        DU.update_records(hb.materialize(), 0, names, [1, 0, 0, 0])
    for od in (False, True):
        r = b.duckdb(0, names, what=abi.DL_UPDATES, on_device=od)
        assert r.status == abi.RB_NEEDS_HOST and (int(r.view.host_event), r.view.host_column) == (fi.value.event, fi.value.column) == (4, 1)
        r.close()
    b.close(); d.close()
    # a DEFERRED key cell: the SET record's column is reported, it comes first; in the predicate record alone with a key image
    buf, offs = _stream(ok + [W.update(42, ["7", deferred, "{}", T], key=["1", deferred, W.NULL, W.NULL])])
    hb, b, d = _both(SC.simple_table(cols, ident=[1, 1, 0, 0]), buf, offs)
    r = b.duckdb(0, names, what=abi.DL_UPDATES)
    assert r.status == abi.RB_NEEDS_HOST and (int(r.view.host_event), r.view.host_column) == (4, 1)
    r.close(); b.close(); d.close()
    buf, offs = _stream(ok + [W.update(42, ["7", "2.5", "{}", T], key=["1", deferred, W.NULL, W.NULL])])
    hb, b, d = _both(SC.simple_table(cols, ident=[1, 1, 0, 0]), buf, offs)
    with pytest.raises(DL.Failure) as fi:
        DU.update_records(hb.materialize(), 0, names, [1, 1, 0, 0])
    r = b.duckdb(0, names, what=abi.DL_UPDATES)
    assert r.status == abi.RB_NEEDS_HOST and (int(r.view.host_event), r.view.host_column) == (fi.value.event, fi.value.column) == (4, 1)
    r.close(); b.close(); d.close()
    # a json cell that is not one JSON value: ETLG_E_JSON at its event, before the DEFERRED cell of an earlier event
    buf, offs = _stream(ok + [W.update(42, ["7", deferred, "{}", T]), W.update(42, ["8", "1", "{bad", T]), W.update(42, ["9", "1", "[1,", T])])
    hb, b, d = _both(SC.simple_table(cols), buf, offs)
    with pytest.raises(DL.Failure) as fi:
        DU.update_records(hb.materialize(), 0, names, [1, 0, 0, 0])
    assert (fi.value.kind, fi.value.event) == ("json", 5)
    with pytest.raises(EtlError) as ei:
        b.duckdb(0, names, what=abi.DL_UPDATES)
    assert ei.value.code == abi.E_JSON and ei.value.frame_index == 5
    b.close(); d.close()
    # the same columns MISSING: neither
    buf, offs = _stream(ok + [W.update(42, ["7", T, T, T]), W.insert(42, ["8", deferred, "{}", "x"])])
    hb, b, d = _both(SC.simple_table(cols), buf, offs)
    assert _check(hb, b, names) == (8, 0)
    b.close(); d.close()


def test_degenerate_inputs():
    from etl_amd.decoder import Decoder, EtlError
    from oracle import oracle
    cols = [("id", SC.INT8, False, 1), ("s", 25, True, 0)]
    buf, offs = _stream([W.insert(42, ["1", "a"]), W.update(42, ["1", "b"]), W.delete(42, old=["1", "b"])])
    hb, b, d = _both(SC.simple_table(cols), buf, offs)
    for od in (False, True):
        assert _check(hb, b, ["id", "s"], on_device=od) == (0, 0)               # no partial Update: n_rows == 0, no host rows
    r = b.duckdb(0, ["id", "s"], what=abi.DL_UPDATES)
    assert r.view.n_bytes == 0 and r.col_ends().shape == (0, 2)
    r.close()
    for what in (abi.DL_TUPLES, abi.DL_PREDICATES):                             # the getter is ETLG_DL_UPDATES' alone
        r = b.duckdb(0, ["id", "s"], what=what)
        with pytest.raises(EtlError) as ei:
            r.col_ends_ptr()
        assert ei.value.kind == abi.InvalidArgument
        r.close()
    r = b.ndjson(0, ["id", "s"])
    with pytest.raises(EtlError):
        r.col_ends_ptr()
    r.close(); b.close(); d.close()
    rows = [b"%d\ttext %d\n" % (i, i) for i in range(50)]                       # a table-copy batch has no Updates
    o, d = oracle.Oracle(), Decoder(0)
    for t in (o, d):
        t.schema_put(42, 0, cols)
    so, sd = o.table_ready(42, 0, [1, 1], [1, 0]), d.table_ready(42, 0, [1, 1], [1, 0])
    cbuf = np.frombuffer(b"".join(rows), dtype=np.uint8)
    coffs = np.cumsum([0] + [len(x) for x in rows]).astype(np.uint32)
    rb, gb = o.copy_decode(so, cbuf, coffs), d.copy_decode(sd, cbuf, coffs, flags=abi.F_OUTPUT_ON_DEVICE)
    assert gb.rc == 0 and rb.err_code == 0
    r = gb.duckdb(0, ["id", "s"], what=abi.DL_UPDATES)
    assert r.status == abi.RB_OK and r.n_rows == 0 and r.view.n_host_rows == 0 and r.view.n_bytes == 0
    r.close(); gb.close(); d.close()
