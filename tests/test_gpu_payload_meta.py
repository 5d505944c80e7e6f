"""etlg_batch_payload (etl_amd/csrc/kernels.hip: k_payf_*, finish.hip: k_paye_*) against tests/payload_meta.py: the oracle walked one
frame per call (what the reference's per-message handlers measure, apply.rs:2459-2463 / :2503-2507 / :2547-2551) with range sums and
buckets in plain Python. Every case is compared exactly: received bytes and rows per kind, the histogram, ev_bytes per event, the sums of
every range — and received_bytes against the batch's own payload_bytes.
The kernels' constants: workgroups of 256 lanes, waves of 64 (frame counts on both sides of each), and the scan tiles — 256 frames and
2 048 events, or ETLG_PAY_TILE for both in a context of its own: with a tile of T the streams of T - 1 .. 3 T T + 5 frames give one tile,
two, one chunk of 256 tile counts and more than one. Under the SIMT emulator the same cases run with a tile of 8."""
import ctypes as C
import os

import numpy as np
import pytest

from etl_amd import abi, synth
from tests import payload_meta as PM
from tests import pgwire as W
from tests import scenarios as SC

pytestmark = pytest.mark.gpu
EMU = os.environ.get("ETLG_SIMT_RUN") == "1"
TILE = 8 if EMU else 128
TILE_SIZES = [TILE - 1, TILE, TILE + 1, TILE * TILE - 1, TILE * TILE, TILE * TILE + 1, 3 * TILE * TILE + 5]
BOUNDS = [0, 1, 4, 8, 16, 64, 100, 1000]


# ---------------------------------------------------------------- device memory of the test's own

def _dev_put(a):
    """array -> (owner, address) of a copy in device memory, 8 spare bytes behind it (the emulator's device memory is host memory)."""
    raw = np.frombuffer(np.ascontiguousarray(a).tobytes() + b"\0" * (8 + (-a.nbytes) % 8), dtype=np.uint8).copy()
    if EMU:
        return raw, raw.ctypes.data
    import torch
    own = torch.from_numpy(raw).cuda()
    torch.cuda.synchronize()
    return own, own.data_ptr()


def _dev_get(ptr, n, dtype):
    nb = n * np.dtype(dtype).itemsize
    if not nb:
        return np.zeros(0, dtype=dtype)
    if EMU:
        return np.frombuffer((C.c_uint8 * nb).from_address(ptr), dtype=dtype).copy()
    return abi.device_tensor(ptr, nb, 0).cpu().numpy().view(dtype)


def _decoder(tile=None):
    from etl_amd.decoder import Decoder
    before = os.environ.get("ETLG_PAY_TILE")
    if tile:
        os.environ["ETLG_PAY_TILE"] = str(tile)                            # read when the context is created
    try:
        return Decoder(0)
    finally:
        os.environ.pop("ETLG_PAY_TILE", None)
        if before is not None:
            os.environ["ETLG_PAY_TILE"] = before


def _arr(buf):
    return np.frombuffer(bytes(buf), dtype=np.uint8) if not isinstance(buf, np.ndarray) else buf


def _split(buf, offs, at):
    """The stream cut into decode calls in front of the frames `at`."""
    buf, offs, edges = _arr(buf), np.asarray(offs, dtype=np.uint32), [0] + list(at) + [len(offs) - 1]
    return [(buf[offs[a]:offs[b]], (offs[a:b + 1] - offs[a]).astype(np.uint32)) for a, b in zip(edges, edges[1:])]


# ---------------------------------------------------------------- the comparison

def _check(b, w, buf, offs, cuts=None, bounds=BOUNDS, copy=False):
    """Host input, host output: everything against the walk `w`. Returns the Payload."""
    v = b.view()
    p = b.payload(buf, offs, cuts=cuts, bounds=bounds)
    by, rows = w.received()
    assert list(p.info.received_bytes) == by and list(p.info.received_rows) == rows, (list(p.info.received_bytes), by, list(p.info.received_rows), rows)
    if copy:
        assert p.info.received_bytes[abi.PK_COPY] == v.payload_bytes[0]
    else:
        assert list(p.info.received_bytes)[:3] == list(v.payload_bytes)
    assert p.info.status == abi.PM_OK and p.info.mismatch_event == PM.U64_MAX
    assert p.info.n_ranges == (0 if cuts is None else len(cuts)) + 1
    assert np.array_equal(p.hist, PM.buckets(w.sizes(), bounds)), (p.hist.tolist(), PM.buckets(w.sizes(), bounds).tolist())
    assert int(v.n_events) == len(w.event_frames())
    assert np.array_equal(p.ev_bytes, w.ev_bytes()), (p.ev_bytes[:8], w.ev_bytes()[:8])
    want = PM.range_sums(w.ev_kinds(), w.ev_bytes(), [] if cuts is None else cuts, copy=copy)
    assert np.array_equal(p.sums, want), (p.sums[:3].tolist(), want[:3].tolist())
    return p


class _Case:
    """One stream decoded in one or more calls on a context of its own, and the walk of every call."""

    def __init__(self, prime, batches, tile=None, flags=0, expect_error=False):
        from oracle import oracle
        self.d, self.o = _decoder(tile), oracle.Oracle()
        prime(self.d); prime(self.o)
        self.batches = [(_arr(buf), np.asarray(offs, dtype=np.uint32)) for buf, offs in batches]
        self.b = [self.d.decode(buf, offs, flags=abi.F_OUTPUT_ON_DEVICE | flags) for buf, offs in self.batches]
        if flags & abi.F_ASYNC:
            for b in self.b:
                b.sync()
        self.w = [PM.Walk(self.o, buf, offs) for buf, offs in self.batches]
        for b, w in zip(self.b, self.w):
            assert bool(b.rc) == bool(w.err) and (expect_error or not b.rc), (b.rc, b.error, w.err)

    def check(self, k=0, **kw):
        return _check(self.b[k], self.w[k], *self.batches[k], **kw)

    def close(self):
        for b in self.b:
            b.close()
        self.d.close()


_CFG2 = {}


def _cfg2(n, tile=None):
    """The first n frames of one cfg2 stream: every frame is one event."""
    if not _CFG2:
        top = max(TILE_SIZES + [257]) + 2
        w = synth.cfg2()
        buf, offs = w.fill(top * 128 + (256 << 10))
        assert len(offs) - 1 >= top
        _CFG2.update(w=w, buf=buf, offs=offs)
    g = _CFG2
    return _Case(g["w"].register, [(g["buf"][:g["offs"][n]], g["offs"][:n + 1])], tile=tile)


def _stream(msgs, **kw):
    s = SC.txn(msgs, **kw)
    return np.frombuffer(s.bytes(), dtype=np.uint8), np.asarray(s.offsets, dtype=np.uint32)


COLS = [("id", SC.INT8, False, 1), ("v", SC.TEXT, True, 0)]


def _two_tables(t):
    SC.simple_table(COLS, table_id=42)(t)
    t.schema_put(43, 0, COLS)                                              # known, never owned


# ---------------------------------------------------------------- frame-count seams

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257])
def test_frame_counts_on_both_sides_of_wave_and_workgroup(n):
    c = _cfg2(n)
    c.check()
    c.check(cuts=list(range(1, n + 1)))
    c.close()


@pytest.mark.parametrize("n", TILE_SIZES)
def test_small_tile_crosses_every_level_of_the_scans(n):
    c = _cfg2(n, tile=TILE)
    c.check()
    c.check(cuts=[n // 3, n // 3, n - 1])
    c.close()


# ---------------------------------------------------------------- events != frames

def test_messages_of_a_table_that_is_not_owned_are_received_and_not_delivered():
    msgs = [W.insert(43 if i % 3 == 2 else 42, [str(i), "x" * (i % 37)]) for i in range(600)]
    c = _Case(_two_tables, [_stream(msgs)], tile=TILE)
    p = c.check(cuts=[1, 100, 101, 350])
    n_ev, n_fr = int(c.b[0].view().n_events), int(c.b[0].view().n_frames)
    assert n_fr == 602 and n_ev == 402                                     # events number fewer than frames
    assert p.info.received_rows[abi.PK_INSERT] == 600                      # the received side counts them all
    assert int(p.sums[:, 1, abi.PK_INSERT].sum()) == 400                   # the delivered side only the owned ones
    assert int(p.sums[:, 0, abi.PK_INSERT].sum()) < p.info.received_bytes[abi.PK_INSERT]
    c.close()


# ---------------------------------------------------------------- frame kinds

def _kinds_stream():
    N, U = W.NULL, W.TOAST
    cols = [("id", SC.INT8, False, 1), ("a", SC.TEXT, True, 0), ("k", SC.TEXT, False, 1), ("n", SC.NUMERIC, True, 0)]
    rel = [(1, "id", SC.INT8, -1), (0, "a", SC.TEXT, -1), (1, "k", SC.TEXT, -1), (0, "n", SC.NUMERIC, -1)]
    r = ["1", "alice", "key", "12345.678900"]
    one = [("id", SC.INT8, True, 0), ("s", SC.TEXT, True, 0)]
    msgs = [W.relation(42, "public", "t", "d", rel), W.origin(5, "o"), W.insert(42, r), W.insert(42, ["2", N, "", "NaN"]), W.type_msg(9, "p", "t"),
            W.update(42, ["1", "bob", "key", "1e10"]),                                         # no old tuple
            W.update(42, ["1", "bob", "key2", "7"], key=["1", N, "key", N]),                   # K
            W.update(42, ["1", U, "key2", "-0.5"], old=r),                                      # O, an unchanged-TOAST cell
            ("raw", W.keepalive(0x1234)), W.delete(42, key=["1", N, "key2", N]), W.delete(42, old=r),
            W.message("other", "{}"), W.insert(44, [N, ""]),                                   # the only value is the empty string
            W.insert(44, [N, N]), W.truncate([42], 0), W.truncate([4242], 0), W.insert(42, ["3", "x" * 500, "k" * 33, "0"])]

    def prime(t):
        SC.simple_table(cols, ready=False)(t)
        SC.simple_table(one, table_id=44)(t)
    return prime, msgs


def test_every_frame_kind():
    prime, msgs = _kinds_stream()
    c = _Case(prime, [_stream(msgs * 5)])
    p = c.check(cuts=[3, 40], bounds=[0, 3, 20])
    by, rows = c.w[0].received()
    assert rows == [25, 15, 10, 0]
    empty = [i for i, (k, b) in enumerate(zip(c.w[0].ev_kinds(), c.w[0].ev_bytes())) if k == 0 and b == 0]
    assert len(empty) == 10                                                # rows = 1, bytes = 0: Some(0)
    one = c.b[0].payload(*c.batches[0], cuts=[empty[0], empty[0] + 1]).sums[1]
    assert one[1, abi.PK_INSERT] == 1 and one[0, abi.PK_INSERT] == 0
    assert p.hist[abi.PK_INSERT, 0] == 10                                  # `le 0`
    c.close()


# ---------------------------------------------------------------- a transaction that spans decode calls

def _spanning():
    msgs = [W.insert(43, [str(i), "skip"]) if i in (0, 1, 2, 40, 41, 42, 43) else W.insert(42, [str(i), "v" * (i % 9)]) for i in range(120)]
    s = SC.txn(msgs, final=0x9000)
    s.add(W.begin(0xA000)); s.add(W.insert(42, ["7", "after"])); s.add(W.insert(43, ["8", "skipped"])); s.add(W.update(42, ["7", "again"]))
    s.add(W.commit(0xA000, 0xA008), lsn=0xA000)
    return np.frombuffer(s.bytes(), dtype=np.uint8), np.asarray(s.offsets, dtype=np.uint32)


@pytest.mark.parametrize("flags", [0, abi.F_ASYNC], ids=["sync", "async"])
@pytest.mark.parametrize("at", [[41], [41, 90], [10, 60]], ids=["two", "three", "three-b"])
def test_transaction_cut_into_several_decode_calls(at, flags):
    """Frame 0 is the Begin, frames 1-120 the Inserts, 121 the Commit, 122-126 a second transaction. A batch that starts at frame 41 opens
    with frames of the skipped table (Inserts 40-43); the middle batch of three has no Begin at all; the last batch's leading part ends
    in the Commit, and a new transaction follows."""
    buf, offs = _spanning()
    c = _Case(_two_tables, _split(buf, offs, at), tile=TILE, flags=flags)
    assert sum(int(b.view().n_events) for b in c.b) == 2 + 113 + 2 + 2 and len(c.b) == len(at) + 1
    for k in reversed(range(len(c.b))):                                    # (any order: every batch kept the ordinal it started from)
        ne = int(c.b[k].view().n_events)
        c.check(k, cuts=[ne // 2] if ne else None)
    c.close()


# ---------------------------------------------------------------- an error batch

def test_error_batch_delivers_the_events_in_front_of_the_error():
    msgs = [W.insert(42, [str(i), "ok"]) for i in range(300)]
    msgs[200] = W.insert(42, ["not a number", "payload"])                  # a malformed cell: the message had been measured
    c = _Case(_two_tables, [_stream(msgs)], tile=TILE, expect_error=True)
    assert c.b[0].rc != 0 and int(c.b[0].view().n_frames) == 201 and int(c.b[0].view().n_events) == 201
    p = c.check(cuts=[50])
    assert p.info.received_rows[abi.PK_INSERT] == 201 and int(p.sums[:, 1, abi.PK_INSERT].sum()) == 200
    c.close()


def test_error_in_front_of_the_metrics_is_not_received():
    s = W.Stream()
    s.add(W.begin(0x2000)); s.add(W.insert(42, ["1", "a"])); s.add(W.commit(0x2000, 0x2008), lsn=0x2000); s.add(W.insert(42, ["2", "outside"]))
    c = _Case(_two_tables, [(s.bytes(), s.offsets)], expect_error=True)
    p = c.check()
    assert c.b[0].rc != 0 and p.info.received_rows[abi.PK_INSERT] == 1
    c.close()


# ---------------------------------------------------------------- ranges

def test_ranges_from_the_cuts_the_device_left():
    from tests import batch_cuts as BC
    c = _cfg2(300, tile=TILE)
    b, w, (buf, offs) = c.b[0], c.w[0], c.batches[0]
    m, n = BC.size_model(), 300
    hints = b.size_hints(m)
    c.check(cuts=None)
    c.check(cuts=[n])                                                      # a cut equal to n_events: an empty last range
    for budget in (1, int(hints.sum()) // 3):
        want, _ = BC.cuts(hints, budget)
        own, ptr = _dev_put(np.zeros(n, dtype=np.uint64))
        _, info = b.cuts(m, budget, cap=n, on_device=ptr)
        assert int(info.n_cuts) == len(want) and (budget != 1 or want == list(range(1, n + 1)))
        p = b.payload(buf, offs, cuts=ptr, n_cuts=len(want), bounds=BOUNDS)
        assert np.array_equal(p.sums, PM.range_sums(w.ev_kinds(), w.ev_bytes(), want))
        assert budget != 1 or not p.sums[-1].any()
        del own
    c.close()


def test_bad_cuts_are_refused():
    from etl_amd.decoder import EtlError
    c = _cfg2(65)
    b, (buf, offs) = c.b[0], c.batches[0]
    for cuts in ([5, 4], [66], [1, 2, 70], [64, 63, 65]):
        with pytest.raises(EtlError) as e:
            b.payload(buf, offs, cuts=cuts)
        assert e.value.kind == abi.InvalidArgument, cuts
        own, ptr = _dev_put(np.array(cuts, dtype=np.uint64))              # the same from device memory: the device refuses, nothing is read
        with pytest.raises(EtlError) as e:
            b.payload(buf, offs, cuts=ptr, n_cuts=len(cuts))
        assert e.value.kind == abi.InvalidArgument, cuts
        del own
    c.check(cuts=[0, 0, 65, 65])
    c.close()


# ---------------------------------------------------------------- buckets

def test_buckets():
    from etl_amd.decoder import EtlError
    msgs = [W.insert(42, [str(i % 10), "x" * (i % 70)]) for i in range(200)] + [W.update(42, ["1", "y" * 7]), W.delete(42, key=["1", W.NULL])]
    c = _Case(_two_tables, [_stream(msgs)])
    sizes = sorted({b for _, b in c.w[0].sizes()})
    assert len(sizes) >= 64
    for bounds in ([], [sizes[3]], sizes[:64], [s + 1 for s in sizes[:64]], [0, 1, 2, 1 << 40, (1 << 64) - 1]):
        p = c.check(bounds=bounds)
        assert p.hist.shape == (4, len(bounds) + 1) and int(p.hist.sum()) == 202
    p = c.check(bounds=[sizes[3]])                                         # a value equal to a bound lands in that bucket
    assert p.hist[abi.PK_INSERT, 0] == sum(1 for k, b in c.w[0].sizes() if k == 0 and b <= sizes[3])
    for bounds in (list(range(65)), [1, 1], [5, 4], [0, 7, 7]):
        with pytest.raises(EtlError) as e:
            c.b[0].payload(*c.batches[0], bounds=bounds)
        assert e.value.kind == abi.InvalidArgument, bounds
    c.close()


# ---------------------------------------------------------------- table copy

class _CopyWalk:
    """The reference for copy rows is the offsets (TableCopyPayloadMetadata, table_copy.rs:84)."""

    def __init__(self, offs):
        self.lens = np.diff(np.asarray(offs, dtype=np.int64))

    def received(self):
        return [0, 0, 0, int(self.lens.sum())], [0, 0, 0, len(self.lens)]

    def sizes(self):
        return [(3, int(x)) for x in self.lens]

    def event_frames(self):
        return list(range(len(self.lens)))

    def ev_bytes(self):
        return self.lens.astype(np.uint32)

    def ev_kinds(self):
        return [3] * len(self.lens)


@pytest.mark.parametrize("n", [10, 257])
def test_table_copy_batch(n):
    rows = [("%d\t%s\n" % (i, "x" * (i * 7 % 50))).encode() for i in range(n)]
    buf = np.frombuffer(b"".join(rows), dtype=np.uint8)
    offs = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint32)
    d = _decoder(TILE)
    d.schema_put(42, 0, COLS)
    slot = d.table_ready(42, 0, [1, 1], [1, 0])
    b = d.copy_decode(slot, buf, offs, flags=abi.F_OUTPUT_ON_DEVICE)
    assert b.rc == 0, b.error
    w = _CopyWalk(offs)
    _check(b, w, buf, offs, copy=True)
    p = _check(b, w, buf, offs, cuts=[1, n // 2, n], bounds=[9, 20], copy=True)
    assert not p.sums[:, :, :3].any() and int(p.sums[:, 1, abi.PK_COPY].sum()) == n
    b.close(); d.close()


# ---------------------------------------------------------------- wrong input

def test_another_stream_of_the_same_frame_count_is_a_mismatch():
    a = [W.insert(42, [str(i), "a"]) for i in range(100)]
    other = list(a)
    other[30] = W.truncate([42], 0)                                        # takes an ordinal as well: the first event that differs is its own
    c = _Case(_two_tables, [_stream(a)])
    buf2, offs2 = _stream(other)
    p = c.b[0].payload(buf2, offs2)
    assert p.info.status == abi.PM_MISMATCH and p.info.mismatch_event == 31
    other[30] = W.origin(5, "o")                                           # takes none: every later event joins the frame behind its own
    buf3, offs3 = _stream(other)
    p = c.b[0].payload(buf3, offs3)
    assert p.info.status == abi.PM_MISMATCH and p.info.mismatch_event == 100   # (Inserts shifted onto Inserts; the last one lands on the Commit)
    c.check()
    c.close()


def test_truncated_len_and_short_frame_lists_are_refused_or_mismatch():
    from etl_amd.decoder import EtlError
    c = _cfg2(65)
    b, (buf, offs) = c.b[0], c.batches[0]
    with pytest.raises(EtlError) as e:
        b.payload(buf, offs[:-1])                                          # nframes < view.n_frames
    assert e.value.kind == abi.InvalidArgument
    with pytest.raises(EtlError) as e:
        b.payload(buf, None, nframes=65)                                   # no frame_offsets
    assert e.value.kind == abi.InvalidArgument
    cut = int(offs[40]) + 7                                                # `len` ends inside frame 40: frames 40.. lie outside [buf, buf + len)
    p = b.payload(buf[:cut], offs)
    assert p.info.status == abi.PM_MISMATCH and p.info.mismatch_event == 40
    assert p.info.received_rows[abi.PK_INSERT] == sum(1 for k, _, _ in c.w[0].frames[:40] if k == 0)   # the frames inside `len`
    c.close()


def test_batches_that_are_not_device_resident_are_refused():
    from etl_amd.decoder import Decoder, EtlError
    w = synth.cfg2()
    buf, offs = w.fill(8 << 10)
    d, d2 = Decoder(0), Decoder(0)
    w.register(d); w.register(d2)
    b = d.decode(buf, offs)                                                # host output
    with pytest.raises(EtlError) as e:
        b.payload(buf, offs)
    assert e.value.kind == abi.InvalidArgument and "etlg_batch_payload" in e.value.description
    b.close()
    b = d.decode(buf, offs, flags=abi.F_OUTPUT_ON_DEVICE)
    info = abi.PayloadInfo()
    a = np.ascontiguousarray(buf)
    o = np.ascontiguousarray(offs, dtype=np.uint32)
    rc = d2.L.etlg_batch_payload(d2.h, b.h, a.ctypes.data, len(a), o.ctypes.data, len(o) - 1, None, 0, 0, None, 0, 0, None, None, None, C.byref(info))
    assert rc == abi.InvalidArgument                                       # a batch of another context
    b.payload(buf, offs)
    b.host()                                                               # etlg_batch_download: the arena leaves the device
    with pytest.raises(EtlError) as e:
        b.payload(buf, offs)
    assert e.value.kind == abi.InvalidArgument
    b.close(); d.close(); d2.close()


# ---------------------------------------------------------------- input and output memory

def test_device_input_and_device_output_equal_host():
    msgs = [W.insert(43 if i % 5 == 4 else 42, [str(i), "x" * (i % 23)]) for i in range(400)] + [W.update(42, ["1", "u"]), W.delete(42, key=["1", W.NULL])]
    c = _Case(_two_tables, [_stream(msgs)], tile=TILE)
    b, (buf, offs) = c.b[0], c.batches[0]
    ne = int(b.view().n_events)
    cuts = [7, 200, ne]
    host = c.check(cuts=cuts)
    bown, bptr = _dev_put(buf)
    oown, optr = _dev_put(offs)
    dev_in = b.payload(bptr, optr, cuts=cuts, bounds=BOUNDS, nbytes=len(buf), nframes=len(offs) - 1)
    assert np.array_equal(dev_in.ev_bytes, host.ev_bytes) and np.array_equal(dev_in.sums, host.sums) and np.array_equal(dev_in.hist, host.hist)
    assert list(dev_in.info.received_bytes) == list(host.info.received_bytes)
    for in_dev in (False, True):
        eown, eptr = _dev_put(np.full(ne, 0xEEEEEEEE, dtype=np.uint32))
        sown, sptr = _dev_put(np.full((len(cuts) + 1) * 8, 0xEE, dtype=np.uint64))
        args = (bptr, optr) if in_dev else (buf, offs)
        kw = dict(nbytes=len(buf), nframes=len(offs) - 1) if in_dev else {}
        p = b.payload(*args, cuts=cuts, bounds=BOUNDS, on_device=(eptr, sptr), **kw)
        assert np.array_equal(p.hist, host.hist) and list(p.info.received_rows) == list(host.info.received_rows)
        ev = _dev_get(eptr, ne + 2, np.uint32)
        assert np.array_equal(ev[:ne], host.ev_bytes) and ev[ne] == 0      # nothing behind the events is written
        sm = _dev_get(sptr, (len(cuts) + 1) * 8 + 1, np.uint64)
        assert np.array_equal(sm[:-1].reshape(-1, 2, 4), host.sums) and sm[-1] == 0
        p = b.payload(*args, bounds=BOUNDS, on_device=(None, None), sums=False, **kw)        # neither output: the received side and the check
        assert p.info.status == abi.PM_OK and np.array_equal(p.hist, host.hist)
        del eown, sown
    del bown, oown
    c.close()


# ---------------------------------------------------------------- every scenario

@pytest.mark.parametrize("sc", SC.all_scenarios(), ids=repr)
def test_every_scenario_batch(sc):
    from oracle import oracle
    d, o = _decoder(TILE), oracle.Oracle()
    for t in (d, o):
        if sc.worker:
            t.set_worker(*sc.worker)
        sc.prime(t)
    for buf, given in sc.batches:
        buf = _arr(buf)
        b = d.decode(buf, given, flags=abi.F_OUTPUT_ON_DEVICE)
        offs = PM.frame_offsets(buf) if given is None else np.asarray(given, dtype=np.uint32)
        if given is None and len(offs) > 1:
            assert np.array_equal(d.scan_boundaries(buf[:offs[-1]]), offs)   # what a caller without a sidecar passes
        w = PM.Walk(o, buf, offs)
        ne = int(b.view().n_events)
        assert int(b.view().n_frames) == w.n_frames
        _check(b, w, buf, offs, cuts=[ne // 2] if ne else None)
        failed = b.rc != 0
        b.close()
        if failed:
            break
    d.close()
