"""Device-side Iceberg changelog batches (etlg_batch_iceberg, etl_amd/csrc/columns.hip k_col_cdc + the refusal words of the row
selection) through the C ABI against the host model tests/iceberg_changelog.py (built from materialize(), pinned to the reference by
tests/test_iceberg_kats.py): the rows' values, row_event, the two CDC columns and the refusal report, exactly; host and device output.
Every scenario of tests/scenarios.py that decodes, the update / delete choices under each replica identity, partial updates, every
scalar class with NULLs, the type-matrix table with both options, deferred cells, table-copy batches, empty / foreign / several slots,
ASYNC batches; the data columns byte for byte against etlg_batch_columns; argument and decode errors; one full-size batch."""
import ctypes as C
import os

import numpy as np
import pytest

from etl_amd import abi, synth
from tests import iceberg_changelog as IC
from tests import pgwire as W
from tests import scenarios as SC
from tests.test_gpu_rowbinary import NUMERICS, TIMETZS, _both, _stream

pytestmark = pytest.mark.gpu
EMU = os.environ.get("ETLG_SIMT_RUN") == "1"


def _read(ptr, nbytes, on_device):
    if not nbytes:
        return np.zeros(0, np.uint8)
    if not on_device or EMU:
        return np.frombuffer((C.c_uint8 * nbytes).from_address(ptr), dtype=np.uint8).copy()
    return abi.device_tensor(ptr, nbytes, 0).cpu().numpy()


def _bits(ptr, n, dev):
    return np.unpackbits(_read(ptr, (n + 63) // 64 * 8, dev), bitorder="little")[:n].astype(bool)


def _nan(v, is32):
    return IC._float(int(v), is32)


def _fixed(kind, raw, n):
    """n values of a fixed-width arrow kind out of the bytes `raw`, in the model's forms."""
    if kind == abi.AK_BOOLEAN:
        return [bool(x) for x in np.unpackbits(raw, bitorder="little")[:n]]
    if kind in (abi.AK_INT32, abi.AK_DATE32):
        return raw[:4 * n].view(np.int32).tolist()
    if kind in (abi.AK_INT64, abi.AK_TIME64_US, abi.AK_TIMESTAMP_US, abi.AK_TIMESTAMP_US_UTC):
        return raw[:8 * n].view(np.int64).tolist()
    if kind == abi.AK_FLOAT32:
        return [_nan(v, True) for v in raw[:4 * n].view(np.uint32)]
    if kind == abi.AK_FLOAT64:
        return [_nan(v, False) for v in raw[:8 * n].view(np.uint64)]
    if kind == abi.AK_FIXED16:
        return [raw[16 * k:16 * k + 16].tobytes() for k in range(n)]
    raise AssertionError(kind)


def _strings(offs, data, n):
    return [data[int(offs[k]):int(offs[k + 1])].tobytes() for k in range(n)]


def _column(cols, i):
    """Column i of a hand-off as a list of the model's values, read from its raw buffers (host or device)."""
    k, n, dev = cols.column(i), cols.n_rows, bool(cols.view.on_device)
    valid = _bits(k.validity, n, dev)
    var = (abi.AK_LARGE_UTF8, abi.AK_LARGE_BINARY, abi.AK_TEXT_FORM)
    if k.arrow_kind in var:
        offs = _read(k.offsets, 8 * (n + 1), dev).view(np.int64)
        assert offs[0] == 0 and int(offs[n]) == int(k.values_bytes)
        vals = _strings(offs, _read(k.values, int(k.values_bytes), dev), n)
    elif k.arrow_kind == abi.AK_LIST:
        offs = _read(k.offsets, 8 * (n + 1), dev).view(np.int64)
        m = int(k.child_count)
        assert int(offs[n]) == m
        cvalid = _bits(k.child_validity, m, dev)
        if k.child_kind in var:
            co = _read(k.child_offsets, 8 * (m + 1), dev).view(np.int64) if m else np.zeros(1, np.int64)
            child = _strings(co, _read(k.values, int(co[m]), dev), m)
        else:
            child = _fixed(k.child_kind, _read(k.values, int(k.values_bytes), dev), m)
        child = [v if ok else None for v, ok in zip(child, cvalid)]
        vals = [child[int(offs[r]):int(offs[r + 1])] for r in range(n)]
    else:
        vals = _fixed(k.arrow_kind, _read(k.values, int(k.values_bytes), dev), n)
    assert int(k.null_count) == int((~valid).sum())
    return [v if ok else None for v, ok in zip(vals, valid)]


def _check(hb, b, slot=0, on_device=False, copy=False, parse_arrays=False, format_json=False, events=None):
    ev = events if events is not None else hb.materialize()
    rows, ops, seqs, idx, n_host, first, why = IC.changelog(ev, slot, hb.slots[slot].cols, copy=copy, parse_arrays=parse_arrays, format_json=format_json)
    c = b.iceberg(slot, parse_arrays=parse_arrays, format_json=format_json, on_device=on_device)
    ci, n, nd = c.changelog, len(rows), len(hb.slots[slot].cols)
    assert (int(ci.n_host_rows), int(ci.host_event), int(ci.host_reason), int(ci.n_data_cols)) == (n_host, first, why, nd)
    assert c.n_rows == n and c.view.n_cols == nd + 2 and c.view.on_device == (1 if on_device else 0)
    dev = bool(on_device)
    assert np.array_equal(_read(c.view.row_event, 8 * n, dev).view(np.uint64), np.array(idx, dtype=np.uint64))
    for i in range(nd):
        got, want = _column(c, i), [r[i] for r in rows]
        if got != want:
            bad = [k for k in range(n) if got[k] != want[k]][0]
            raise AssertionError((i, bad, got[bad], want[bad]))
    for t, (want, w) in enumerate(((ops, 6), (seqs, 33))):
        k = c.column(nd + t)
        assert (k.type_class, k.arrow_kind, k.nullable, int(k.null_count), int(k.deferred_count), int(k.values_bytes)) == (abi.TC_STRING, abi.AK_LARGE_UTF8, 0, 0, 0, w * n)
        assert np.array_equal(_read(k.offsets, 8 * (n + 1), dev).view(np.int64), np.arange(n + 1, dtype=np.int64) * w)
        assert _read(k.values, w * n, dev).tobytes() == b"".join(want)
        ones, words = np.packbits(np.ones(n, bool), bitorder="little"), _read(k.validity, (n + 63) // 64 * 8, dev)
        assert np.array_equal(words[:len(ones)], ones) and not words[len(ones):].any()
        assert not _read(k.deferred, (n + 63) // 64 * 8, dev).any()
    c.close()
    return n, n_host


def _check_both(hb, b, **kw):
    ev = hb.materialize()
    r = [_check(hb, b, on_device=od, events=ev, **kw) for od in (False, True)]
    assert r[0] == r[1]
    return r[0]


def _scenarios():
    return [s for s in SC.all_scenarios()]


@pytest.mark.parametrize("sc", _scenarios(), ids=lambda s: s.name)
def test_scenarios(sc):
    """Every batch of every scenario that the oracle decodes without error, every slot of it."""
    from etl_amd.decoder import Decoder
    from oracle import oracle
    o, d = oracle.Oracle(), Decoder(0)
    for t in (o, d):
        if sc.worker:
            t.set_worker(*sc.worker)
        sc.prime(t)
    for buf, offs in sc.batches:
        a = np.frombuffer(bytes(buf), dtype=np.uint8) if not isinstance(buf, np.ndarray) else buf
        rb = o.decode(a, offs)
        b = d.decode(a, offs, flags=abi.F_OUTPUT_ON_DEVICE)
        if rb.err_code != 0:
            break
        assert b.rc == 0, b.error
        hb = rb.host_batch()
        ev = hb.materialize()
        for slot in range(len(hb.slots)):
            _check(hb, b, slot=slot, on_device=slot % 2 == 1, events=ev)
        b.close()
    d.close()


ALL = [c for c in SC.ALLTYPES]


@pytest.mark.parametrize("ident_name", ["Default", "Full", "Index"])
def test_updates_and_deletes_under_each_identity(ident_name):
    """Full old images are kept (Delete) or skipped over (Update), key images are skipped over (Update) or refused (Delete), partial
    updates are refused with or without an old image — and the first refusal is named although accepted rows stand behind it."""
    cols = [("a", SC.INT4, True, 0), ("k1", SC.INT8, False, 1), ("s", 25, True, 0), ("k2", 25, True, 1)]
    ident = {"Default": [0, 1, 0, 1], "Full": [1, 1, 1, 1], "Index": [0, 0, 1, 1]}[ident_name]
    msgs = []
    for i in range(150):
        k2 = W.NULL if i % 7 == 3 else "k'%d" % i
        row = [str(i), str(i), "t%d" % i, k2]
        new = [str(i + 1), str(i), "u" * (i % 40), k2]
        msgs.append(W.insert(42, row))
        key = [W.NULL if not f else v for f, v in zip(ident, row)]
        m = i % 8
        if m == 0:
            msgs.append(W.update(42, new))
        elif m == 1:
            msgs.append(W.update(42, new, old=row) if ident_name == "Full" else W.update(42, new, key=key))
        elif m == 2:
            msgs.append(W.update(42, [str(i), str(i), W.TOAST, k2]))
        elif m == 3:
            msgs.append(W.delete(42, old=row))
        elif m == 4:
            msgs.append(W.delete(42, old=row) if ident_name == "Full" else W.delete(42, key=key))
        elif m == 5:
            msgs.append(W.update(42, [str(i), str(i), W.TOAST, k2], old=row) if ident_name == "Full" else W.update(42, [str(i), str(i), W.TOAST, k2], key=key))
        elif m == 6:
            msgs.append(W.update(42, new, old=row))
        else:
            msgs.append(W.delete(42, key=key) if ident_name != "Full" else W.delete(42, old=row))
    buf, offs = _stream(msgs)
    hb, b, d = _both(SC.simple_table(cols, ident=ident), buf, offs)
    n, host = _check_both(hb, b)
    assert n > 150 and host > 0
    c = b.iceberg(0)
    # the first refused event is the partial update of i == 2: events 0 Begin, then two per i
    assert (int(c.changelog.host_event), int(c.changelog.host_reason)) == (6, abi.ICE_PARTIAL_UPDATE)
    c.close(); b.close(); d.close()


@pytest.mark.parametrize("first", ["partial", "key", "full_ok"])
def test_each_refusal_reason_and_its_event(first):
    cols = [("id", SC.INT8, False, 1), ("s", 25, True, 0)]
    ins = [W.insert(42, [str(i), "x%d" % i]) for i in range(70)]
    if first == "partial":
        msgs = ins + [W.update(42, ["1", W.TOAST]), W.insert(42, ["99", "y"]), W.delete(42, key=["1", W.NULL])] + ins[:5]
        want = (2, 71, abi.ICE_PARTIAL_UPDATE)
    elif first == "key":
        msgs = ins[:3] + [W.delete(42, key=["1", W.NULL])] + ins + [W.update(42, ["1", W.TOAST]), W.delete(42, key=["2", W.NULL])]
        want = (3, 4, abi.ICE_KEY_ONLY_DELETE)
    else:
        msgs = ins + [W.delete(42, old=["1", "x1"]), W.update(42, ["2", "z"], old=["2", "x2"]), W.update(42, ["3", "w"], key=["3", W.NULL])]
        want = (0, abi.NO_EVENT, 0)
    buf, offs = _stream(msgs)
    hb, b, d = _both(SC.simple_table(cols), buf, offs)
    _check_both(hb, b)
    c = b.iceberg(0)
    assert (int(c.changelog.n_host_rows), int(c.changelog.host_event), int(c.changelog.host_reason)) == want
    c.close(); b.close(); d.close()
    # (a Delete without an old image: pgoutput cannot say it — that row of the table is checked on the model, tests/test_iceberg_kats.py)


def test_every_scalar_class_and_nulls_under_full_identity():
    names = [c[0] for c in ALL]
    rows = [SC.alltypes_row(), SC.alltypes_row(id="2", b="f", i2="-7", i4="-2147483648", o="4294967295", d="0001-01-01", t="00:00:00",
                                               ts="1969-12-31 23:59:59.5", tstz="2026-01-02 03:04:05+02", f8="1e300", f4="-0.5", s="", by="\\x", j="[]", arr="{}"),
            SC.alltypes_row(id="-9223372036854775808", d="9999-12-31", t="23:59:59.12", s="x" * 300, by="\\x" + "ab" * 200, f8="NaN", f4="-Infinity"),
            [("4" if n == "id" else W.NULL) for n in names]]
    rows += [SC.alltypes_row(id=str(10 + i), s="y" * (i * 13 % 200), t=f"01:02:{i % 60:02}.{i:06}", n=NUMERICS[i % len(NUMERICS)], tz=TIMETZS[i % len(TIMETZS)])
             for i in range(130)]
    msgs = [W.insert(42, r) for r in rows]
    msgs += [W.update(42, rows[(k + 1) % len(rows)], old=r) for k, r in enumerate(rows)] + [W.delete(42, old=r) for r in rows]
    buf, offs = _stream(msgs)
    hb, b, d = _both(SC.simple_table(ALL, ident=[1] * len(ALL)), buf, offs)
    for pa, fj in ((False, False), (True, True)):
        assert _check_both(hb, b, parse_arrays=pa, format_json=fj) == (3 * len(rows), 0)
    c = b.iceberg(0)
    assert c.column(len(ALL)).values and _read(c.column(len(ALL)).values, 6, False).tobytes() == b"INSERT"
    seq = _read(c.column(len(ALL) + 1).values, 33, False).tobytes()
    assert seq == b"%016x/%016x" % (int(hb.commit_lsn[1]), int(hb.tx_ordinal[1]))
    c.close(); b.close(); d.close()


@pytest.mark.parametrize("opts", [(False, False), (True, False), (False, True), (True, True)])
def test_type_matrix_table(opts):
    from etl_amd.decoder import Decoder
    from oracle import oracle
    o, d = oracle.Oracle(), Decoder(0)
    buf, offs = synth.type_matrix_stream(40 if EMU else 300, mix=True)
    synth.type_matrix_register(o)
    synth.type_matrix_register(d)
    rb = o.decode(buf, offs)
    assert rb.err_code == 0
    gb = d.decode(buf, offs, flags=abi.F_NO_CONTROL | abi.F_OUTPUT_ON_DEVICE)
    assert gb.rc == 0, gb.error
    n, host = _check_both(rb.host_batch(), gb, parse_arrays=opts[0], format_json=opts[1])
    assert n > 0 and host > 0                                     # (the stream's Deletes carry the key only)
    if opts[0]:
        c = gb.iceberg(0, parse_arrays=True)
        names = [x[0] for x in synth.TYPE_MATRIX_COLS]
        assert [k for i, k in enumerate(names) if k.endswith("_arr") and c.column(i).arrow_kind != abi.AK_LIST] == []
        c.close()
    gb.close(); d.close()


def test_deferred_cells():
    cols3 = [("id", 20, False, True), ("x", 701, True, False), ("y", 700, True, False), ("a", 1022, True, False)]
    vals = ["1.5", "0.1000000000000000055511151231257827021181583404541015625", "NaN", "3.141592653589793238462643383279",
            "1e-320", "2.5", "1.7976931348623157e308", "4.9e-324", "50537618.817359292015891086651596749e82",
            "107896223265412489690691363e88", "28879636596541978310003766487.741e-212", "5693107746173304490483329377e264"]
    rows = [[str(i), vals[i % len(vals)], vals[(i + 3) % len(vals)], "{1.5,NULL,%d}" % i] for i in range(200)]
    msgs = [W.insert(42, r) for r in rows] + [W.delete(42, old=r) for r in rows[::3]]
    buf, offs = _stream(msgs)
    hb, b, d = _both(SC.simple_table(cols3, ident=[1, 1, 1, 1]), buf, offs)
    _check_both(hb, b)
    _check_both(hb, b, parse_arrays=True)
    c = b.iceberg(0)
    st = sum(1 for e in hb.materialize() if e["kind"] in "ID" for cell in (e.get("row") or e["old_row"])[1:2] if cell[0] == "Deferred")
    assert st > 0 and int(c.column(1).deferred_count) == st
    c.close(); b.close(); d.close()


def test_table_copy_batch():
    from etl_amd.decoder import Decoder
    from oracle import oracle
    cols = [("id", SC.INT8, False, 1), ("s", 25, True, 0), ("f", SC.FLOAT8, True, 0), ("k", 25, True, 1)]
    rows = [b"%d\ttext %d\\twith tab\t%s\t%s\n" % (i, i, b"1.5" if i % 2 else b"\\N", b"\\N" if i % 5 == 0 else b"k%d" % i) for i in range(150)]
    o, d = oracle.Oracle(), Decoder(0)
    for t in (o, d):
        t.schema_put(42, 0, cols)
    so = o.table_ready(42, 0, [1] * len(cols), [1, 0, 0, 1])
    sd = d.table_ready(42, 0, [1] * len(cols), [1, 0, 0, 1])
    buf = np.frombuffer(b"".join(rows), dtype=np.uint8)
    offs = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint32)
    rb, gb = o.copy_decode(so, buf, offs), d.copy_decode(sd, buf, offs, flags=abi.F_OUTPUT_ON_DEVICE)
    assert gb.rc == 0 and rb.err_code == 0
    assert _check_both(rb.host_batch(), gb, copy=True) == (150, 0)
    c = gb.iceberg(0)
    assert _read(c.column(5).values, 33 * 150, False).tobytes() == IC.COPY_SEQUENCE * 150
    c.close(); gb.close(); d.close()


def test_empty_foreign_and_several_slots():
    from etl_amd.decoder import Decoder, EtlError
    from oracle import oracle
    buf, offs = _stream([])
    hb, b, d = _both(SC.simple_table(SC.COLS2), buf, offs)
    assert _check_both(hb, b) == (0, 0)
    with pytest.raises(Exception):
        b.iceberg(7)                                               # no such slot
    hb2 = b.host()                                                 # downloaded: the arena left the device
    with pytest.raises(EtlError) as ei:
        b.iceberg(0)
    assert ei.value.kind == abi.InvalidState
    b.close(); d.close()
    # two tables in one batch: each slot gets its own rows, the other's events are neither rows nor refusals
    ca, cb = [("id", SC.INT8, False, 1), ("s", 25, True, 0)], [("k", SC.INT4, False, 1), ("f", SC.FLOAT8, True, 0), ("t", 25, True, 0)]
    msgs = []
    for i in range(90):
        msgs.append(W.insert(42, [str(i), "a%d" % i]))
        msgs.append(W.insert(43, [str(i), "1.5", "b%d" % i]))
        if i % 4 == 1:
            msgs.append(W.delete(43, key=[str(i), W.NULL, W.NULL]))
        if i % 5 == 2:
            msgs.append(W.update(42, [str(i), W.TOAST]))

    def prime(t):
        SC.simple_table(ca, table_id=42)(t)
        SC.simple_table(cb, table_id=43)(t)
    buf, offs = _stream(msgs)
    hb, b, d = _both(prime, buf, offs)
    assert len(hb.slots) == 2
    r0, r1 = _check_both(hb, b, slot=0), _check_both(hb, b, slot=1)
    assert r0 == (90, 18) and r1 == (90, 23)
    b.close(); d.close()


def test_async_batch():
    from etl_amd.decoder import Decoder
    from oracle import oracle
    w = synth.cfg3()
    o, d = oracle.Oracle(), Decoder(0)
    w.register(o); w.register(d)
    buf, offs = w.fill(96 << 10 if EMU else 1 << 20)
    rb = o.decode(buf, offs)
    assert rb.err_code == 0
    keep = (np.ascontiguousarray(buf), np.ascontiguousarray(offs, dtype=np.uint32))
    if EMU:
        b = d.decode_device(keep[0].ctypes.data, len(buf), keep[1].ctypes.data, len(offs) - 1, abi.F_OUTPUT_ON_DEVICE | abi.F_ASYNC)
    else:
        import torch
        tb, to = torch.from_numpy(keep[0].copy()).cuda(), torch.from_numpy(keep[1].view(np.int32).copy()).cuda()
        torch.cuda.synchronize()
        b = d.decode_device(tb.data_ptr(), tb.numel(), to.data_ptr(), len(offs) - 1, abi.F_OUTPUT_ON_DEVICE | abi.F_ASYNC)
    n, host = _check_both(rb.host_batch(), b)                      # (the call syncs the pending batch itself)
    assert n > 100 and host > 0
    b.close(); d.close()


@pytest.mark.parametrize("mk", [synth.cfg2, synth.cfg3])
def test_data_columns_equal_etlg_batch_columns_byte_for_byte(mk):
    """On a batch without Deletes every data column buffer (validity, deferred, values, offsets) equals etlg_batch_columns(INSERT |
    UPDATE); and etlg_batch_columns gives afterwards what it gave before."""
    w = synth.Workload(mk().tables, 0x1CEB, rows_per_txn=100, mix=(70, 30, 0), upd_key=20, upd_toast=10, name="no_deletes")
    buf, offs = w.fill(96 << 10 if EMU else 2 << 20)
    hb, b, d = _both(w.register, buf, offs)
    assert not (hb.kind == ord("D")).any() and (hb.kind == ord("U")).any()

    def buffers(c, ncols):
        n, out = c.n_rows, [c.row_event().tobytes()]
        for i in range(ncols):
            k = c.column(i)
            v, df, vals, offsets = c.host_arrays(i)
            out.append((k.type_class, k.arrow_kind, k.value_bytes, k.nullable, int(k.null_count), int(k.deferred_count), int(k.values_bytes),
                        v.tobytes(), df.tobytes(), vals.tobytes(), None if offsets is None else offsets.tobytes()))
        return n, out
    nc = len(hb.slots[0].cols)
    for pa, fj in ((False, False), (True, True)):
        before = b.columns(0, kinds=("I", "U"), parse_arrays=pa, format_json=fj)
        want = buffers(before, nc)
        ice = b.iceberg(0, parse_arrays=pa, format_json=fj)
        assert buffers(ice, nc) == want and want[0] > 100
        after = b.columns(0, kinds=("I", "U"), parse_arrays=pa, format_json=fj)
        assert buffers(after, nc) == want and after.view.n_cols == nc and after.changelog is None
        only_i = b.columns(0)
        assert only_i.n_rows == int(((hb.kind == ord("I")) & (hb.schema_slot == 0)).sum())
        for c in (before, ice, after, only_i):
            c.close()
    _check_both(hb, b)
    b.close(); d.close()


def test_arguments_and_plain_columns_objects():
    from etl_amd.decoder import EtlError
    buf, offs = _stream([W.insert(42, ["1", "x"])])
    hb, b, d = _both(SC.simple_table(SC.COLS2), buf, offs)
    L = d.L
    for opts in (abi.ROWS_INSERT, abi.ROWS_UPDATE, abi.ROWS_INSERT | abi.ROWS_PARSE_ARRAYS, 16, 1 << 31):
        out = C.c_void_p()
        assert L.etlg_batch_iceberg(d.h, b.h, 0, opts, 0, C.byref(out)) == abi.InvalidArgument and not out
    for opts in (0, abi.ROWS_PARSE_ARRAYS, abi.ROWS_FORMAT_JSON, abi.ROWS_PARSE_ARRAYS | abi.ROWS_FORMAT_JSON):
        out = C.c_void_p()
        assert L.etlg_batch_iceberg(d.h, b.h, 0, opts, 0, C.byref(out)) == abi.OK and out
        L.etlg_columns_free(out)
    plain = b.columns(0)
    info = abi.ChangelogInfo()
    assert L.etlg_columns_changelog_get(plain.h, C.byref(info)) == abi.InvalidArgument
    assert L.etlg_columns_changelog_get(None, C.byref(info)) == abi.InvalidArgument
    ice = b.iceberg(0)
    assert L.etlg_columns_changelog_get(ice.h, C.byref(info)) == abi.OK and info.n_data_cols == 2 and info.host_event == abi.NO_EVENT
    assert L.etlg_columns_changelog_get(ice.h, None) == abi.InvalidArgument
    plain.close(); ice.close(); b.close(); d.close()


@pytest.mark.parametrize("what", ["array", "json", "json_in_old_row"])
def test_malformed_cells_fail_like_etlg_batch_columns(what):
    """A malformed array literal / a cell that is not JSON: the same error at the same event as etlg_batch_columns — also when the cell
    stands in a Delete's old row, which etlg_batch_columns never selects."""
    from etl_amd.decoder import EtlError
    cols = [("id", SC.INT8, False, 1), ("a", 1007, True, 0), ("j", 114, True, 0)]
    good = ["1", "{1}", "{}"]
    bad = ["2", "{1,{2}}", "{}"] if what == "array" else ["2", "{1}", "{bad"]
    if what == "json_in_old_row":
        msgs = [W.insert(42, good), W.delete(42, old=bad), W.insert(42, good)]
    else:
        msgs = [W.insert(42, good), W.insert(42, bad), W.insert(42, good)]
    buf, offs = _stream(msgs)
    hb, b, d = _both(SC.simple_table(cols, ident=[1, 1, 1]), buf, offs)
    pa = what == "array"
    with pytest.raises(EtlError) as ei:
        b.iceberg(0, parse_arrays=pa)
    assert ei.value.frame_index == 2 and ei.value.code == (abi.E_JSON if not pa else ei.value.code)
    if what != "json_in_old_row":
        with pytest.raises(EtlError) as ec:
            b.columns(0, kinds=("I", "U"), parse_arrays=pa)
        assert (ec.value.kind, ec.value.code, ec.value.description, ec.value.frame_index) == (ei.value.kind, ei.value.code, ei.value.description, ei.value.frame_index)
    else:
        assert ei.value.description == "JSON deserialization failed"
        c = b.columns(0, kinds=("I", "U"))                         # the Inserts alone are fine
        assert c.n_rows == 2
        c.close()
    b.close(); d.close()


def test_full_size_batch():
    """>= 200 000 events built with tests/pgwire under REPLICA IDENTITY FULL, Insert / Update / Delete mixed over text + numeric + int
    columns, a row count that is no multiple of 64: every byte of both CDC columns, their offsets and bitmaps against the model computed
    vectorised in numpy; row_event and the int column against the event headers and the rows' ids."""
    if EMU:
        n_ev = 3001          # the emulator runs the same kernels over a smaller stream: the full size is the MI355X run's
    else:
        n_ev = 200_003
    cols = [("id", SC.INT4, False, 1), ("t", 25, True, 0), ("n", SC.NUMERIC, True, 0)]
    per_txn = 997
    s = W.Stream(lsn=0xABCDEF0123000000)
    k = 0
    while k < n_ev:
        m = min(per_txn, n_ev - k)
        final = 0xABCDEF0123400000 + 0x10000 * (k // per_txn)
        s.add(W.begin(final, ts=1, xid=5))
        for i in range(k, k + m):
            row = [str(i), "text-%d" % i if i % 9 else W.NULL, "%d.%02d" % (i, i % 100)]
            if i % 3 == 0:
                s.add(W.insert(42, row))
            elif i % 3 == 1:
                s.add(W.update(42, [str(i), "new", "1e3"], old=row))
            else:
                s.add(W.delete(42, old=row))
        s.add(W.commit(final, final + 8, ts=2, flags=0), lsn=final)
        k += m
    buf, offs = np.frombuffer(s.bytes(), dtype=np.uint8), s.offsets
    from etl_amd.decoder import Decoder
    d = Decoder(0)
    SC.simple_table(cols, ident=[1, 1, 1])(d)
    b = d.decode(buf, offs, flags=abi.F_OUTPUT_ON_DEVICE)
    assert b.rc == 0, b.error
    c = b.iceberg(0)
    n = c.n_rows
    assert n == n_ev and n % 64 != 0 and n % 256 != 0 and int(c.changelog.n_host_rows) == 0 and int(c.changelog.host_event) == abi.NO_EVENT
    rev = c.row_event().copy()
    op_v, op_o = c.host_arrays(3)[2].copy(), c.host_arrays(3)[3].copy()
    sq_v, sq_o = c.host_arrays(4)[2].copy(), c.host_arrays(4)[3].copy()
    bitmaps = [c.host_arrays(i)[j].copy() for i in (3, 4) for j in (0, 1)]
    ids = c.host_arrays(0)[2].view(np.int32).copy()
    hb = b.host()                                                  # the batch leaves the device here
    is_row = np.isin(hb.kind, np.frombuffer(b"IUD", np.uint8))
    assert np.array_equal(rev, np.flatnonzero(is_row).astype(np.uint64))
    assert np.array_equal(ids, np.arange(n, dtype=np.int32))
    assert np.array_equal(op_o, np.arange(n + 1, dtype=np.int64) * 6) and np.array_equal(sq_o, np.arange(n + 1, dtype=np.int64) * 33)
    kinds = hb.kind[is_row]
    table = np.zeros((256, 6), np.uint8)
    for ch, word in IC.OPS.items():
        table[ord(ch)] = np.frombuffer(word, np.uint8)
    assert np.array_equal(op_v.reshape(n, 6), table[kinds])
    hexd = np.frombuffer(b"0123456789abcdef", np.uint8)
    want = np.full((n, 33), ord("/"), np.uint8)
    for col0, v in ((0, hb.commit_lsn[is_row]), (17, hb.tx_ordinal[is_row])):
        shifts = (np.arange(15, -1, -1, dtype=np.uint64) * np.uint64(4))[None, :]
        want[:, col0:col0 + 16] = hexd[((v[:, None] >> shifts) & np.uint64(15)).astype(np.int64)]
    assert np.array_equal(sq_v.reshape(n, 33), want)
    assert want[0].tobytes() == IC.sequence_number(int(hb.commit_lsn[is_row][0]), int(hb.tx_ordinal[is_row][0]))
    assert len(np.unique(hb.commit_lsn[is_row])) > 1 and (hb.commit_lsn[is_row] >> np.uint64(60)).max() > 0      # every hex digit position is exercised
    ones = np.packbits(np.ones(n, bool), bitorder="little")
    for j, bm in enumerate(bitmaps):
        if j % 2 == 0:
            assert np.array_equal(bm[:len(ones)], ones) and not bm[len(ones):].any()
        else:
            assert not bm.any()
    c.close(); b.close(); d.close()
