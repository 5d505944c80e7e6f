"""ETLG_F_CHECK_CELLS (include/etlg.h): json / jsonb cells that are not one JSON value and array literals the reference rejects are
decode errors at their frame, in the reference's order, on every decode path. Expected values come from the oracle alone: its FULL mode
parses every cell while it decodes the frame (like parse_cell_from_postgres_text) and gives (code, kind, frame, events); the arena in
front of the cut is the CONTRACT oracle's on the frames before the failing one. Through the C ABI (etl_amd.Decoder)."""
import os
import random
import struct

import numpy as np
import pytest

from etl_amd import abi, synth
from tests import pgwire as W
from tests import scenarios as SC
from tests.golden import reference_kats as KATS
from tests.test_gpu_async import DevBufs

pytestmark = pytest.mark.gpu
EMU = os.environ.get("ETLG_SIMT_RUN") == "1"
CHECK = abi.F_CHECK_CELLS
_KNOBS = ("ETLG_FUSED_KERNEL", "ETLG_FORCE_MULTIPASS", "ETLG_COPY_DIRECT")
PATHS = {"default": {}, "fused256": {"ETLG_FUSED_KERNEL": "0"}, "fused64": {"ETLG_FUSED_KERNEL": "1"}, "cells": {"ETLG_FUSED_KERNEL": "2"},
         "rows": {"ETLG_FUSED_KERNEL": "4"}, "multipass": {"ETLG_FORCE_MULTIPASS": "1"}}


@pytest.fixture
def knobs():
    saved = {k: os.environ.pop(k, None) for k in _KNOBS}

    def use(env):
        for k in _KNOBS:
            os.environ.pop(k, None)
        os.environ.update(env)
    yield use
    for k in _KNOBS:
        os.environ.pop(k, None)
        if saved[k] is not None:
            os.environ[k] = saved[k]


def _expect(prime, buf, offs, worker=None):
    """(code, kind, frame, n_events, arena of the frames before the cut) from the oracle alone."""
    from oracle import oracle
    full, con, con2 = oracle.Oracle(mode=oracle.MODE_FULL), oracle.Oracle(), oracle.Oracle()
    for o in (full, con, con2):
        if worker:
            o.set_worker(*worker)
        prime(o)
    rf = full.decode(buf, offs)
    if rf.err_code:
        rc = _prefix_arena(con, con2, buf, offs, rf.err_frame)
    else:
        r = con.decode(buf, offs)
        assert r.err_code == 0
        rc = r.host_batch()
    assert rc.n_events == rf.n_events, (rc.n_events, rf.n_events)
    return (rf.err_code, rf.err_kind, rf.err_frame if rf.err_code else -1, rf.n_events), rc


def _prefix_arena(con, con2, buf, offs, f):
    """The CONTRACT oracle's arena of the frames before failing frame f. Its payload counters are those of the frames up to and
    INCLUDING f (a second CONTRACT oracle in the same state, whatever it makes of frame f itself): the reference records a row frame's
    payload metrics before it decodes the tuple (apply.rs:2459-2463), so the failing frame's bytes are counted — as after any other
    decode error."""
    r = con.decode(buf[:int(offs[f])], np.asarray(offs[:f + 1], dtype=np.uint32))
    assert r.err_code == 0
    hb = r.host_batch()
    r2 = con2.decode(buf[:int(offs[f + 1])], np.asarray(offs[:f + 2], dtype=np.uint32))
    assert r2.err_code == 0 or r2.err_frame == f
    hb.payload_bytes = tuple(r2.host_batch().payload_bytes)
    return hb


def _got(b):
    e = b.error
    return (e.code, e.kind, e.frame_index, int(b.view().n_events)) if e else (0, 0, -1, int(b.view().n_events))


def _decode(prime, buf, offs, flags, sidecar=True, device=False, worker=None):
    from etl_amd.decoder import Decoder
    d = Decoder(0)
    if worker:
        d.set_worker(*worker)
    prime(d)
    if device:
        dev = DevBufs([(buf, offs)])
        p, n, po, nf = dev.items[0]
        b = d.decode_device(p, n, po if sidecar else None, nf if sidecar else 0, flags | abi.F_INPUT_ON_DEVICE | abi.F_OUTPUT_ON_DEVICE)
        b._keep_dev = dev
    else:
        b = d.decode(buf, offs if sidecar else None, flags=flags)
    return d, b


def _same(prime, buf, offs, flags=CHECK, **kw):
    want, arena = _expect(prime, buf, offs, worker=kw.get("worker"))
    d, b = _decode(prime, buf, offs, flags, **kw)
    got = _got(b)
    print("check_cells: oracle", want, "device", got)
    assert got == want
    if want[0]:
        assert int(b.view().n_frames) == want[2]
    if not (flags & abi.F_FINISH_CELLS):
        diff = arena.diff(b.host())
        assert not diff, diff[:6]
    paths = d.debug_paths()
    b.close()
    d.close()
    return want, paths


def _np(s):
    return np.frombuffer(s.bytes(), dtype=np.uint8), np.asarray(s.offsets, dtype=np.uint32)


# ------------------------------------------------------------------ 1. reference vectors
def _kat_vectors():
    from etl_amd import native
    L = native.lib()
    out = []
    for oid, text, exp in KATS.ALL_TEXT_KATS:
        if L.etlg_type_class_of_oid(oid) in (abi.TC_JSON, abi.TC_ARRAY):
            out.append((oid, text, exp))
    return out


def test_reference_vectors_fail_at_their_frame():
    """Every json and array vector of the reference's own tests as column 2 of the second of three Inserts."""
    vecs = _kat_vectors()
    rejected = accepted = 0
    for oid, text, _exp in vecs:
        cols = [("id", SC.INT8, False, 1), ("v", oid, True, 0)]
        prime = SC.simple_table(cols)
        s = SC.txn([W.insert(42, ["1", W.NULL]), W.insert(42, ["2", text]), W.insert(42, ["3", W.NULL])])
        buf, offs = _np(s)
        want, _ = _same(prime, buf, offs)
        if want[0]:
            rejected += 1
            assert want[2] == 2 and want[3] == 2, (oid, text, want)   # Begin + one Insert
        else:
            accepted += 1
        d, b = _decode(prime, buf, offs, 0)        # the same batch without the flag: no error
        assert b.rc == 0 and int(b.view().n_events) == 5, (oid, text)
        b.close()
        d.close()
    print("check_cells: reference vectors rejected", rejected, "accepted", accepted)
    assert rejected >= 37 and accepted >= 1, (rejected, accepted)


# ------------------------------------------------------------------ 2. order
OCOLS = [("id", SC.INT8, False, 1), ("j", SC.JSONB, True, 0), ("t", SC.TEXT, True, 0), ("n", SC.INT4, True, 0), ("a", SC.INT4_A, True, 0)]
OPRIME = SC.simple_table(OCOLS)
BADJ, GOODJ = '{"a": [1, 2}', '{"a": [1, 2]}'


def _order_cases():
    ok = ["1", GOODJ, "x", "7", "{1,2}"]

    def row(**kw):
        r = list(ok)
        for k, v in kw.items():
            r[[c[0] for c in OCOLS].index(k)] = v
        return r
    cases = {
        "json_before_int": [W.insert(42, row()), W.insert(42, row(j=BADJ, n="7x"))],
        "int_before_array": [W.insert(42, row()), W.insert(42, row(n="7x", a="{1,2"))],
        "old_full_image_first": [W.insert(42, row()), W.update(42, row(n="x7"), old=row(j=BADJ))],
        "new_image_when_old_is_fine": [W.update(42, row(a="{1,{2}}"), old=row())],
        "bad_int_in_frame_before": [W.insert(42, row(n="q")), W.insert(42, row(j=BADJ))],
        "bad_int_in_frame_after": [W.insert(42, row(j=BADJ)), W.insert(42, row(n="q"))],
        "delete_full_image": [W.insert(42, row()), W.delete(42, old=row(a='{1,"2}'))],
        "toast_over_valid_old": [W.update(42, ["1", W.TOAST, "y", "8", W.TOAST], old=row())],
        "toast_without_old": [W.update(42, ["1", W.TOAST, "y", "8", "{3}"])],
        "array_element": [W.insert(42, row(a="{1,NULL,2x,{")), W.insert(42, row())],
        "null_cells": [W.insert(42, ["1", W.NULL, W.NULL, W.NULL, W.NULL]), W.insert(42, row(j="tru"))],
    }
    return {k: _np(SC.txn(v)) for k, v in cases.items()}


def _utf8_case():
    raw = b'{"k": "\xff\xfe"'   # not UTF-8 and not JSON: ETLG_E_UTF8 wins
    tup = struct.pack(">h", 5) + b"".join(b"t" + struct.pack(">i", len(c)) + c for c in [b"2", raw, b"x", b"7", b"{1}"])
    s = W.Stream(lsn=0x1000)
    s.add(W.begin(0x2000, ts=1, xid=7))
    s.add(W.insert(42, ["1", GOODJ, "x", "7", "{1}"]))
    s.add(b"I" + struct.pack(">I", 42) + b"N" + tup)
    s.add(W.commit(0x2000, 0x2008, ts=2, flags=0), lsn=0x2000)
    return _np(s)


@pytest.mark.parametrize("name", ["json_before_int", "int_before_array", "old_full_image_first", "new_image_when_old_is_fine", "bad_int_in_frame_before",
                                  "bad_int_in_frame_after", "delete_full_image", "toast_over_valid_old", "toast_without_old", "array_element", "null_cells"])
@pytest.mark.parametrize("path", sorted(PATHS))
def test_order_is_the_references(name, path, knobs):
    knobs(PATHS[path])
    buf, offs = _order_cases()[name]
    _same(OPRIME, buf, offs)


def test_the_two_orders_inside_one_row_give_different_codes():
    """(the issue's own check of the recipe: FULL says ETLG_E_JSON where CONTRACT says ETLG_E_INT)"""
    c = _order_cases()
    assert _expect(OPRIME, *c["json_before_int"])[0][0] == abi.E_JSON
    assert _expect(OPRIME, *c["int_before_array"])[0][0] == abi.E_INT
    assert _expect(OPRIME, *c["old_full_image_first"])[0][0] == abi.E_JSON
    assert _expect(OPRIME, *c["toast_over_valid_old"])[0][0] == 0


@pytest.mark.parametrize("path", sorted(PATHS))
def test_invalid_utf8_inside_a_json_cell(path, knobs):
    knobs(PATHS[path])
    buf, offs = _utf8_case()
    want, _ = _same(OPRIME, buf, offs)
    assert want[0] == abi.E_UTF8


def test_a_table_the_worker_does_not_apply_raises_nothing(knobs):
    """should_apply_changes skips the frame: the reference never parses its cells."""
    def prime(t):
        OPRIME(t)
        t.schema_put(43, 0, OCOLS, name="other")
        t.table_state(43, abi.TS_SYNC_DONE, 0x9000000)   # changes below that LSN belong to the table-sync worker
        t.table_ready(43, 0, [1] * len(OCOLS), [1, 0, 0, 0, 0])
    buf, offs = _np(SC.txn([W.insert(43, ["1", BADJ, "x", "7", "{1"]), W.insert(42, ["1", GOODJ, "x", "7", "{1}"])]))
    want, _ = _same(prime, buf, offs)
    assert want[0] == 0


# ------------------------------------------------------------------ 3. every path, sidecar, input side, finish pass
@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("sidecar", [True, False])
@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("finish", [False, True])
def test_every_path(path, sidecar, device, finish, knobs):
    knobs(PATHS[path])
    ok = ["171", GOODJ, "x", "171", "{1,2}"]
    rows = [W.insert(42, [str(i), GOODJ, "x" * (i % 50), str(i), "{%d,NULL}" % i]) for i in range(300)]
    rows[171] = W.insert(42, ["171", '[1, 2,, 3]', "x", "171", "{1}"])
    rows[250] = W.insert(42, ["250", GOODJ, "x", "zz", "{1}"])
    buf, offs = _np(SC.txn(rows))
    flags = CHECK | (abi.F_FINISH_CELLS if finish else 0)
    want, paths = _same(OPRIME, buf, offs, flags=flags, sidecar=sidecar, device=device)
    assert want[0] == abi.E_JSON and want[2] == 172
    # the same rows without the bad json cell, with the flag: the int error behind it
    rows[171] = W.insert(42, ok)
    buf, offs = _np(SC.txn(rows))
    want, _ = _same(OPRIME, buf, offs, flags=flags, sidecar=sidecar, device=device)
    assert want[0] == abi.E_INT and want[2] == 251


# ------------------------------------------------------------------ 4. type-matrix fuzz
CHECKED = None


def _checked_cols():
    global CHECKED
    if CHECKED is None:
        from etl_amd import native
        L = native.lib()
        CHECKED = [i for i, c in enumerate(synth.TYPE_MATRIX_COLS) if L.etlg_type_class_of_oid(c[1]) in (abi.TC_JSON, abi.TC_ARRAY)]
        assert len(CHECKED) >= 33, len(CHECKED)
    return CHECKED


def _mutate(rng, text):
    b = bytearray(text.encode())
    how = rng.randrange(8)
    if how >= 6:                                                          # a mutation that keeps most cells valid: one digit for another
        at = [i for i, c in enumerate(b) if 0x31 <= c <= 0x39]
        if at:
            b[rng.choice(at)] = rng.choice(b"123456789")
        return bytes(b)
    if how == 0 and len(b) > 1:
        del b[rng.randrange(1, len(b)):]                                  # truncation
    elif how == 1:
        at = [i for i, c in enumerate(b) if c in b'{}[]",:']              # a flipped structural byte
        if at:
            i = rng.choice(at)
            b[i] = rng.choice(b'{}[]",:x')
    elif how == 2:
        b.insert(rng.randrange(len(b) + 1), rng.choice(b"{}"))            # an extra brace
    elif how == 3:
        at = [i for i, c in enumerate(b) if c in b",{"]                   # a bad element
        i = rng.choice(at) + 1 if at else 0
        b[i:i] = rng.choice([b"zz,", b"1e,", b"--,", b"\\\\xg0,"])
    elif how == 4 and b'"' in b:
        i = b.find(b'"')
        b[i + 1:i + 1] = b"\\\\ud800" if b.startswith(b"{") and b"\\\"" in b else b"\\ud800"   # a lone surrogate escape (inside an array element: escaped once more)
    else:
        i = rng.randrange(len(b))
        b[i] = rng.choice(b"}{\\\"")
    return bytes(b)


def _replace_cells(frame, repl):
    """frame: one CopyData frame holding an Insert / Update; repl: {column index of the NEW tuple: bytes}. -> the frame rewritten."""
    body = bytes(frame[30:])       # pgoutput message: tag, rel, ...
    tag = body[:1]
    p = 5
    out = bytearray(body[:5])
    if tag == b"U" and body[p:p + 1] in (b"K", b"O"):
        q = p + 1
        n = struct.unpack(">h", body[q:q + 2])[0]
        q += 2
        for _ in range(n):
            k = body[q:q + 1]
            q += 1
            if k == b"t":
                q += 4 + struct.unpack(">i", body[q:q + 4])[0]
        out += body[p:q]
        p = q
    assert body[p:p + 1] == b"N", body[p:p + 1]
    out += b"N"
    p += 1
    n = struct.unpack(">h", body[p:p + 2])[0]
    out += body[p:p + 2]
    p += 2
    for i in range(n):
        k = body[p:p + 1]
        p += 1
        if k == b"t":
            ln = struct.unpack(">i", body[p:p + 4])[0]
            txt = body[p + 4:p + 4 + ln]
            p += 4 + ln
            if i in repl:
                txt = repl[i]
            out += b"t" + struct.pack(">i", len(txt)) + txt
        else:
            out += k
    assert p == len(body)
    payload = bytes(frame[5:30]) + bytes(out)
    return b"d" + struct.pack(">I", len(payload) + 4) + payload


def _fuzz_batch(seed, nrows=40):
    rng = random.Random(seed)
    buf, offs = synth.type_matrix_stream(nrows, rows_per_txn=16, mix=True)
    frames = [bytes(buf[int(offs[i]):int(offs[i + 1])]) for i in range(len(offs) - 1)]
    rowf = [i for i, f in enumerate(frames) if f[30:31] in (b"I", b"U")]
    texts = []
    for _ in range(rng.randrange(1, 4)):
        fi = rng.choice(rowf)
        col = rng.choice(_checked_cols())
        new = _mutate(rng, synth.TYPE_MATRIX[col][3])
        while _undecidable(synth.TYPE_MATRIX_COLS[col][1], new):   # (point 3 of the contract: not this test's ground)
            new = _mutate(rng, synth.TYPE_MATRIX[col][3])
        texts.append((synth.TYPE_MATRIX_COLS[col][1], new))
        frames[fi] = _replace_cells(frames[fi], {col: new})
    nb = np.frombuffer(b"".join(frames), dtype=np.uint8)
    no = np.cumsum([0] + [len(f) for f in frames]).astype(np.uint32)
    return nb, no, texts


def _undecidable(oid, text):
    """Point 3 of the contract, decided on the text alone: a non-text element of more than 40 characters / a json[] element of more
    than 256 bytes (an upper bound: the longest run between separators of the raw literal)."""
    from etl_amd import native
    L = native.lib()
    if L.etlg_type_class_of_oid(oid) != abi.TC_ARRAY:
        return False
    elem = L.etlg_array_elem_class(oid)
    longest = max(len(x) for x in text.split(b","))
    if elem == abi.TC_JSON:
        return longest > 256
    return elem not in (abi.TC_STRING, abi.TC_BYTEA) and longest > 40


FUZZ_SEEDS = list(range(1000, 1024)) if EMU else list(range(1000, 1210))


def test_type_matrix_fuzz():
    from etl_amd.decoder import Decoder
    d = Decoder(0)
    synth.type_matrix_register(d)
    failed = passed = 0
    for seed in FUZZ_SEEDS:
        buf, offs, texts = _fuzz_batch(seed)
        assert not any(_undecidable(o, t) for o, t in texts), (seed, texts)
        want, arena = _expect(synth.type_matrix_register, buf, offs)
        failed += want[0] != 0
        passed += want[0] == 0
        d.reset_stream_state()
        b = d.decode(buf, offs, flags=CHECK)
        got = _got(b)
        assert got == want, (seed, texts, got, want)
        diff = arena.diff(b.host())
        assert not diff, (seed, diff[:6])
        b.close()
    print("check_cells: fuzz batches failed", failed, "passed", passed)
    assert failed * 2 >= len(FUZZ_SEEDS) and passed * 10 >= len(FUZZ_SEEDS), (failed, passed)
    d.close()


def test_clean_type_matrix_streams_are_not_decoded_twice():
    """No over-reporting on clean data: the unmutated streams return 0 with the flag and no second attempt happens."""
    from etl_amd.decoder import Decoder
    from oracle import oracle
    d, o = Decoder(0), oracle.Oracle()
    synth.type_matrix_register(d)
    synth.type_matrix_register(o)
    for n in (40, 700):
        buf, offs = synth.type_matrix_stream(n, mix=True)
        d.reset_stream_state()
        o.reset_stream_state()
        b = d.decode(buf, offs, flags=CHECK | abi.F_NO_CONTROL)
        assert b.rc == 0
        diff = o.decode(buf, offs).host_batch().diff(b.host())
        assert not diff, diff[:6]
        b.close()
    p = d.debug_paths()
    d.close()
    assert p["redone"] == 0 and p["multipass"] == 0 and p["chain_rerun"] == 0, p


# ------------------------------------------------------------------ 5. ASYNC chain
def test_async_chain_with_a_bad_json_cell_in_the_middle():
    """Six device-input batches, a bad jsonb cell in the middle of the third: its error and cut are the FULL oracle's. The batches
    behind it are decoded again from the state the cut left — the frames of the failed batch behind the cut are not applied, so the
    oracle for them starts from that state too."""
    paths = _chain_exact(6, 2, seed=11)
    assert paths["chain_rerun"] >= 1, paths


def test_async_chain_across_a_ring_lap():
    """Forty batches, six in flight, the bad cell in batch 30: the second attempts happen after the result ring (32 blocks) has lapped."""
    paths = _chain_exact(40, 30, seed=13)
    assert paths["chain_rerun"] >= 1, paths


def _chain_exact(nparts, bad_part, seed):
    """A chain of `nparts` ASYNC device-input batches, up to six in flight, with an invalid jsonb cell in the middle of batch `bad_part`.
    The oracles see exactly what the contract says: that batch ends at its failing frame and the next one starts from the carried
    state as of that frame."""
    from etl_amd.decoder import Decoder
    from oracle import oracle
    # whole transactions per batch, so that the batch behind the cut starts with a Begin (the cut leaves a transaction open: what the
    # reference would do with the REST of that transaction is not defined — its apply loop has stopped)
    rng = random.Random(seed)
    pieces = [synth.type_matrix_stream(rng.randrange(40, 90), rows_per_txn=25, start_lsn=0x2000000 + k * 0x100000, mix=True) for k in range(nparts)]
    pb, po = pieces[bad_part]
    frames = [bytes(pb[int(po[i]):int(po[i + 1])]) for i in range(len(po) - 1)]
    at = len(frames) // 2
    while frames[at][30:31] != b"I":
        at += 1
    col = [c[0] for c in synth.TYPE_MATRIX_COLS].index("jsonb_col")
    frames[at] = _replace_cells(frames[at], {col: b'{"kind": "jsonb", }'})
    pieces[bad_part] = (np.frombuffer(b"".join(frames), dtype=np.uint8).copy(), np.cumsum([0] + [len(f) for f in frames]).astype(np.uint32))
    full, con, con2, d = oracle.Oracle(mode=oracle.MODE_FULL), oracle.Oracle(), oracle.Oracle(), Decoder(0)
    for t in (full, con, con2, d):
        synth.type_matrix_register(t)
    dev = DevBufs(pieces)
    flags = abi.F_INPUT_ON_DEVICE | abi.F_OUTPUT_ON_DEVICE | abi.F_NO_CONTROL | abi.F_ASYNC | CHECK
    inflight, done = [], 0
    for k, (p, n, pof, nf) in enumerate(dev.items):
        inflight.append(d.decode_device(p, n, pof, nf, flags))
        while len(inflight) - done > 5 or (k == len(dev.items) - 1 and done < len(inflight)):
            b = inflight[done]
            bufk, offk = pieces[done]
            rc = b.sync()
            rf = full.decode(bufk, offk)      # FULL mode carries the same transaction state as the device: it stops where the device stops
            if done == bad_part:
                assert rf.err_code == abi.E_JSON and rf.err_frame == at, (rf.err_code, rf.err_frame, at)
                arena = _prefix_arena(con, con2, bufk, offk, at)
            else:
                assert rf.err_code == 0, (done, rf.err_code, rf.err_frame)
                rcn = con.decode(bufk, offk)
                assert rcn.err_code == 0
                arena = rcn.host_batch()
                if done < bad_part:
                    con2.decode(bufk, offk)
            assert (rc != 0) == (rf.err_code != 0), (done, rc, b.error)
            assert _got(b) == (rf.err_code, rf.err_kind, rf.err_frame if rf.err_code else -1, rf.n_events), (done, _got(b))
            diff = arena.diff(b.host())
            assert not diff, f"batch {done}: {diff[:6]}"
            b.close()
            done += 1
    paths = d.debug_paths()
    d.close()
    return paths


# ------------------------------------------------------------------ 6. table copy
CCOLS = [("id", SC.INT8, False, 1), ("j", SC.JSONB, True, 0), ("a", SC.INT4_A, True, 0), ("t", SC.TEXT, True, 0)]


def _copy_rows(n, bad, what):
    rows = []
    for i in range(n):
        j, a = '{"i": %d}' % i, "{%d,NULL,7}" % i
        if i == bad:
            j, a = ('{"i": }', a) if what == "json" else (j, "{%d,{7}}" % i)
        rows.append(("%d\t%s\t%s\tr%d\n" % (i, j, a, i)).encode())
    return np.frombuffer(b"".join(rows), dtype=np.uint8), np.cumsum([0] + [len(r) for r in rows]).astype(np.uint32)


@pytest.mark.parametrize("what", ["json", "array"])
@pytest.mark.parametrize("direct", ["1", "0"])
@pytest.mark.parametrize("asyn", [False, True])
def test_table_copy_rows(what, direct, asyn, knobs):
    from etl_amd.decoder import Decoder
    from oracle import oracle
    knobs({"ETLG_COPY_DIRECT": direct})
    full, con, d = oracle.Oracle(mode=oracle.MODE_FULL), oracle.Oracle(), Decoder(0)
    slots = []
    for t in (full, con, d):
        t.schema_put(42, 0, CCOLS)
        slots.append(t.table_ready(42, 0, [1] * len(CCOLS), [1, 0, 0, 0]))
    n, bad = 500, 277
    buf, offs = _copy_rows(n, bad, what)
    rf = full.copy_decode(slots[0], buf, offs)
    assert rf.err_code == (abi.E_JSON if what == "json" else abi.E_ARRAY_MULTIDIM) and rf.err_frame == bad
    rcn = con.copy_decode(slots[1], buf[:int(offs[bad])], offs[:bad + 1])
    flags = CHECK | ((abi.F_ASYNC | abi.F_OUTPUT_ON_DEVICE) if asyn else 0)
    b = d.copy_decode(slots[2], buf, offs, flags=flags)
    if asyn:
        b.sync()   # (the frames path of a table copy may finish the batch inside the call)
    e = b.error
    assert e and (e.code, e.kind, e.frame_index) == (rf.err_code, rf.err_kind, rf.err_frame), (e, rf.err_code, rf.err_frame)
    assert int(b.view().n_events) == bad and int(b.view().n_frames) == bad
    assert b.view().payload_bytes[0] == int(offs[bad])
    diff = rcn.host_batch().diff(b.host())
    assert not diff, diff[:6]
    b.close()
    # without the flag: every row, no error; with it and clean rows: the same arena
    b = d.copy_decode(slots[2], buf, offs)
    assert b.rc == 0 and int(b.view().n_events) == n
    b.close()
    buf, offs = _copy_rows(n, -1, what)
    b = d.copy_decode(slots[2], buf, offs, flags=CHECK)
    assert b.rc == 0
    assert not con.copy_decode(slots[1], buf, offs).host_batch().diff(b.host())
    b.close()
    d.close()


# ------------------------------------------------------------------ 7. free where it cannot matter
def test_no_check_kernel_for_a_table_without_json_or_arrays():
    from etl_amd.decoder import Decoder
    from oracle import oracle
    w = synth.cfg3()
    buf, offs = w.fill(1 << 20)
    o, d = oracle.Oracle(), Decoder(0)
    w.register(o)
    w.register(d)
    d.profile(True)
    b = d.decode(buf, offs, flags=CHECK | abi.F_NO_CONTROL)
    assert b.rc == 0
    assert not o.decode(buf, offs).host_batch().diff(b.host())
    b.close()
    prof = d.profile_read()
    assert prof["k_chk_cells"][0] == 0, prof
    d.close()
    # ... and one launch per batch for a table that has such columns
    d = Decoder(0)
    synth.type_matrix_register(d)
    d.profile(True)
    buf, offs = synth.type_matrix_stream(100)
    b = d.decode(buf, offs, flags=CHECK | abi.F_NO_CONTROL)
    assert b.rc == 0
    b.close()
    b = d.decode(*synth.type_matrix_stream(100, start_lsn=0x3000000), flags=abi.F_NO_CONTROL)
    assert b.rc == 0
    b.close()
    prof = d.profile_read()
    assert prof["k_chk_cells"][0] == 1, prof
    d.close()
