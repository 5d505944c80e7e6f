"""etlg_batch_cuts / etlg_cuts_locate (etl_amd/csrc/finish.hip: k_cut_*, k_cuts_locate) against tests/batch_cuts.py, the restatement of the
apply loop's cut rule (crates/etl/src/replication/apply.rs:656-657, :1932-1935) over the hints of oracle/size_hint.py. Every case compares
the cuts, n_cuts, stop_event, carry_out and total with the model, exactly. The reference's tests state no cut position as a number, so
nothing here is pinned to a vector of its own: this is the device against the sequential rule.
The kernels' constants: workgroups of 256 events, waves of 64 (event counts on both sides of each), and the scan tile — 2 048 events, or
ETLG_CUTS_TILE in a context of its own: with a tile of T the streams of T - 1 .. 3 T T + 5 events give one tile, two, one chunk of 256 tile
sums and more than one. Budget 1 cuts behind every event (the deepest orbit: one jump level per bit of the event count); total + 1 never
cuts. Under the SIMT emulator the same cases run with a tile of 8 and shorter streams."""
import ctypes as C
import os
import random

import numpy as np
import pytest

from etl_amd import abi, synth
from tests import batch_cuts as BC
from tests import pgwire as W
from tests import scenarios as SC

pytestmark = pytest.mark.gpu
EMU = os.environ.get("ETLG_SIMT_RUN") == "1"
TILE = 8 if EMU else 128
TILE_SIZES = [TILE - 1, TILE, TILE + 1, TILE * TILE - 1, TILE * TILE, TILE * TILE + 1, 3 * TILE * TILE + 5]
INFO = ("n_cuts", "stop_event", "carry_out", "total")


# ---------------------------------------------------------------- device memory of the test's own

def _dev_put(a):
    """np.uint64 array -> (owner, address) of a copy in device memory (the emulator's device memory is host memory)."""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if EMU:
        own = np.concatenate([a, np.zeros(1, dtype=np.uint64)])
        return own, own.ctypes.data
    import torch
    own = torch.from_numpy(np.concatenate([a, np.zeros(1, dtype=np.uint64)]).view(np.int64)).cuda()
    torch.cuda.synchronize()
    return own, own.data_ptr()


def _dev_get(ptr, n):
    if not n:
        return np.zeros(0, dtype=np.uint64)
    if EMU:
        return np.frombuffer((C.c_uint8 * (8 * n)).from_address(ptr), dtype=np.uint64).copy()
    return abi.device_tensor(ptr, 8 * n, 0).cpu().numpy().view(np.uint64)


# ---------------------------------------------------------------- one decoded batch and its model hints

class _Case:
    def __init__(self, prime, buf, offs, tile=None, hints=None):
        from etl_amd.decoder import Decoder
        from oracle import oracle
        before = os.environ.get("ETLG_CUTS_TILE")
        if tile:
            os.environ["ETLG_CUTS_TILE"] = str(tile)            # read when the context is created
        try:
            self.d = Decoder(0)
        finally:
            os.environ.pop("ETLG_CUTS_TILE", None)
            if before is not None:
                os.environ["ETLG_CUTS_TILE"] = before
        prime(self.d)
        self.b = self.d.decode(buf, offs, flags=abi.F_OUTPUT_ON_DEVICE)
        assert self.b.rc == 0, self.b.error
        self.hb = None
        if hints is None:
            o = oracle.Oracle()
            prime(o)
            rb = o.decode(buf, offs)
            assert rb.err_code == 0, rb.err_desc
            self.hb = rb.host_batch()
            hints = BC.hints_of(self.hb)
        self.hints, self.n, self.m = hints, len(hints), BC.size_model()
        assert int(self.b.view().n_events) == self.n

    def check(self, budget, carry=0, first=0, end=None, dev_hints=None, want_hints=None, cap=None):
        want, wi = BC.cuts(self.hints if want_hints is None else want_hints, budget, carry, first, end)
        got, info = self.b.cuts(self.m if dev_hints is None else None, budget, carry, first, end, hints=dev_hints, cap=cap)
        gi = {k: int(getattr(info, k)) for k in INFO}
        assert gi == wi, (budget, carry, first, end, gi, wi)
        keep = want if cap is None else want[:cap]
        assert [int(x) for x in got] == keep, (budget, carry, first, end, [int(x) for x in got][:6], keep[:6])
        return want, wi

    def budgets(self, seed):
        clean = [int(h) for h in self.hints if not int(h) >> 63]
        total, rng = sum(clean), random.Random(seed)
        return [1, min(clean), max(clean), max(clean) + 1, max(1, total // 3), total, total + 1] + [rng.randrange(1, total + 2) for _ in range(5)]

    def check_budgets(self, seed=0xC075):
        for budget in self.budgets(seed):
            for carry in sorted({0, 1, budget - 1}):
                if carry < budget:
                    self.check(budget, carry)

    def close(self):
        self.b.close(); self.d.close()


_CFG2 = {}


def _cfg2(n, tile=None):
    """The first n events of one cfg2 stream (every frame of it is one event) and the matching prefix of hints computed once, for the
    longest stream of the file."""
    if not _CFG2:
        top = max(TILE_SIZES + [300]) + 2
        w = synth.cfg2()
        buf, offs = w.fill(top * 128 + (256 << 10))                        # (whole transactions of 1 000 rows)
        assert len(offs) - 1 >= top
        full = _Case(w.register, buf[:offs[top]], offs[:top + 1])
        _CFG2.update(w=w, buf=buf, offs=offs, hints=full.hints)
        full.close()
    g = _CFG2
    return _Case(g["w"].register, g["buf"][:g["offs"][n]], g["offs"][:n + 1], tile=tile, hints=g["hints"][:n])


def _stream(msgs):
    s = SC.txn(msgs)
    return np.frombuffer(s.bytes(), dtype=np.uint8), s.offsets


# ---------------------------------------------------------------- event-count seams, budgets, carries

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257])
def test_event_counts_on_both_sides_of_wave_and_workgroup(n):
    c = _cfg2(n)
    c.check_budgets()
    c.close()


@pytest.mark.parametrize("n", TILE_SIZES)
def test_small_tile_crosses_every_level_of_the_scan(n):
    c = _cfg2(n, tile=TILE)
    c.check_budgets()
    c.close()


@pytest.mark.parametrize("n", [256, 257, 300])
def test_more_tile_sums_than_one_pass_of_their_scan_takes(n):
    c = _cfg2(n, tile=1)                                                    # k_cut_scan walks the tile sums 256 at a time, carrying their sum
    total = int(c.hints.sum())
    for budget, carry in ((1, 0), (int(c.hints.max()) + 1, 1), (total // 3, total // 3 - 1), (total + 1, 0)):
        c.check(budget, carry)
    c.close()


def _every_kind():
    N, U = W.NULL, W.TOAST
    cols = [("id", SC.INT8, False, 1), ("a", SC.TEXT, True, 0), ("k", SC.TEXT, False, 1), ("n", SC.NUMERIC, True, 0), ("by", SC.BYTEA, True, 0)]
    r = ["1", "alice", "key", "12345.678900", "\\x0102ff"]
    msgs = [W.insert(42, r), W.insert(42, ["2", N, "", "NaN", N]), W.insert(42, ["3", "x" * 500, "k" * 33, "0", "\\x"]),
            W.update(42, ["1", "bob", "key", "1e10", N]),
            W.update(42, ["1", "bob", "key2", "7", N], key=["1", N, "key", N, N]),
            W.update(42, ["1", "carol", "key2", "-0.5", "\\xff"], old=r),
            W.delete(42, key=["1", N, "key2", N, N]), W.delete(42, old=r),
            W.truncate([42], 0)]
    return cols, msgs, W.update(42, ["1", U, "key2", "1", N])             # the last: unchanged toast, no old image -> partial


def test_every_event_kind_and_row_shape():
    cols, msgs, _ = _every_kind()
    c = _Case(SC.simple_table(cols), *_stream(msgs * 7))
    assert not (c.hints >> np.uint64(63)).any() and len(set(c.hints.tolist())) > 6
    c.check_budgets()
    c.close()


@pytest.fixture(scope="module")
def cfg3():
    w = synth.cfg3()
    buf, offs = w.fill((48 << 10) if EMU else (1 << 20))
    c = _Case(w.register, buf, offs, tile=TILE)
    yield c
    c.close()


def test_non_uniform_hints_of_the_mixed_stream(cfg3):
    assert cfg3.n > 100 and len(set(cfg3.hints.tolist())) > 20
    inc = np.flatnonzero(cfg3.hints >> np.uint64(63))
    end = int(inc[0]) if len(inc) else cfg3.n                              # (partial Updates of the stream are INCOMPLETE: see below)
    for budget in cfg3.budgets(3):
        for carry in sorted({0, 1, budget - 1}):
            if carry < budget:
                cfg3.check(budget, carry)
                cfg3.check(budget, carry, 0, end)


# ---------------------------------------------------------------- sub-ranges

def _complete(c):
    """The case's hints with every INCOMPLETE entry completed by a value of the test's own, and their copy in device memory."""
    h = c.hints.copy()
    inc = np.flatnonzero(h >> np.uint64(63))
    h[inc] = (h[inc] & np.uint64(BC.MASK)) + np.uint64(1000) + inc.astype(np.uint64) % np.uint64(97)
    return h, _dev_put(h)


def test_sub_ranges_on_and_next_to_tile_seams(cfg3):
    h, (own, ptr) = _complete(cfg3)
    n, T = cfg3.n, TILE
    assert n > 3 * T + 2
    total = int(h.sum())
    for budget in (1, int(h.max()), max(1, total // 50), total):
        for first, end in [(0, 0), (5, 5), (n, n), (1, n), (0, n - 1), (T, 2 * T), (T - 1, 2 * T + 1), (T + 1, 2 * T - 1), (2 * T, n), (T, T + 1),
                           (n - 1, n), (3, T), (3, T + 1)]:
            for carry in sorted({0, budget - 1}):
                want, wi = cfg3.check(budget, carry, first, end, dev_hints=ptr, want_hints=h)
                if first == end:
                    assert want == [] and wi["carry_out"] == carry and wi["stop_event"] == first
    del own


def test_two_ranges_chained_through_the_carry_equal_one(cfg3):
    h, (own, ptr) = _complete(cfg3)
    n, T = cfg3.n, TILE
    total = int(h.sum())
    for budget in (1, int(h.max()) + 1, max(1, total // 7)):
        whole, wi = cfg3.check(budget, 0, 0, n, dev_hints=ptr, want_hints=h)
        for mid in (1, T - 1, T, T + 1, n // 2, n - 1):
            a, ai = cfg3.check(budget, 0, 0, mid, dev_hints=ptr, want_hints=h)
            b, bi = cfg3.check(budget, ai["carry_out"], mid, n, dev_hints=ptr, want_hints=h)
            assert a + b == whole and bi["carry_out"] == wi["carry_out"]
    del own


# ---------------------------------------------------------------- events the host has to size

def test_incomplete_events_stop_the_walk_and_completed_hints_run_on():
    cols, msgs, partial = _every_kind()
    c = _Case(SC.simple_table(cols), *_stream(msgs * 3 + [partial] + msgs * 2 + [partial, partial] + msgs))
    inc = np.flatnonzero(c.hints >> np.uint64(63))
    assert len(inc) == 3 and inc[0] == 1 + 3 * len(msgs)
    h, (own, ptr) = _complete(c)
    total = int(h.sum())
    for budget in (1, 200, max(1, total // 4), total + 1):
        _, wi = c.check(budget)
        assert wi["stop_event"] == inc[0]
        _, wi = c.check(budget, 0, int(inc[0]))                            # INCOMPLETE at `first`: nothing is walked
        assert (wi["n_cuts"], wi["stop_event"], wi["total"]) == (0, inc[0], 0)
        _, wi = c.check(budget, 0, int(inc[0]) + 1)                        # the host adds the event and resumes behind it
        assert wi["stop_event"] == inc[1]
        _, wi = c.check(budget, 0, 0, None, dev_hints=ptr, want_hints=h)   # completed by the host: to the end
        assert wi["stop_event"] == c.n and wi["total"] == total
    del own
    c.close()


def test_json_and_array_cells_of_the_all_types_table():
    rows = [SC.alltypes_row(id="1", j=W.NULL, arr=W.NULL), SC.alltypes_row(id="2", j=W.NULL, arr=W.NULL), SC.alltypes_row(id="3", j="[1,2]", arr="{}"),
            SC.alltypes_row(id="4", j=W.NULL, arr=W.NULL), SC.alltypes_row(id="5")]
    c = _Case(SC.simple_table(SC.ALLTYPES), *_stream([W.insert(42, r) for r in rows] * 20))
    inc = np.flatnonzero(c.hints >> np.uint64(63))
    assert len(inc) == 40 and inc[0] == 3
    h, (own, ptr) = _complete(c)
    for budget in (1, int(h[1]), int(h.sum()) // 9):
        assert c.check(budget)[1]["stop_event"] == 3
        assert c.check(budget, budget - 1, 4)[1]["stop_event"] == 5
        assert c.check(budget, 0, 0, None, dev_hints=ptr, want_hints=h)[1]["stop_event"] == c.n
    del own
    c.close()


# ---------------------------------------------------------------- cuts_cap, output memory

def test_cuts_cap_and_resuming_from_the_last_written_cut(cfg3):
    h, (own, ptr) = _complete(cfg3)
    budget = max(1, int(h.sum()) // 40)
    want, wi = cfg3.check(budget, 0, 0, None, dev_hints=ptr, want_hints=h)
    k = wi["n_cuts"]
    assert k >= 20
    for cap in (0, 1, k - 1, k, k + 1):
        cfg3.check(budget, 0, 0, None, dev_hints=ptr, want_hints=h, cap=cap)
    for cap in (1, k // 2, k - 1):
        head, _ = cfg3.b.cuts(None, budget, hints=ptr, cap=cap)
        tail, ti = cfg3.b.cuts(None, budget, 0, int(head[-1]), hints=ptr)
        assert [int(x) for x in head] + [int(x) for x in tail] == want and int(ti.carry_out) == wi["carry_out"]
    # cuts_cap 0 without an output array only counts, at budget 1 as well
    got, info = cfg3.b.cuts(None, 1, hints=ptr, cap=0)
    assert len(got) == 0 and int(info.n_cuts) == cfg3.n
    del own


def test_device_output_equals_host_output(cfg3):
    h, (own, ptr) = _complete(cfg3)
    for budget in (1, max(1, int(h.sum()) // 40), int(h.sum()) + 1):
        host, hi = cfg3.b.cuts(None, budget, 5, 0, hints=ptr) if budget > 5 else cfg3.b.cuts(None, budget, hints=ptr)
        for cap in (cfg3.n, max(1, int(hi.n_cuts) // 2)):
            oown, optr = _dev_put(np.full(cap, 0xEE, dtype=np.uint64))
            _, di = cfg3.b.cuts(None, budget, 5 if budget > 5 else 0, 0, hints=ptr, cap=cap, on_device=optr)
            assert [int(getattr(di, k)) for k in INFO] == [int(getattr(hi, k)) for k in INFO]
            k = min(cap, int(hi.n_cuts))
            got = _dev_get(optr, cap + 1)
            assert np.array_equal(got[:k], host[:k]) and (got[k:cap] == 0xEE).all() and got[cap] == 0      # nothing behind the cuts is written
            del oown
    del own


# ---------------------------------------------------------------- arguments

def test_invalid_arguments(cfg3):
    from etl_amd.decoder import EtlError
    b, m, n = cfg3.b, cfg3.m, cfg3.n
    own, ptr = _dev_put(cfg3.hints)
    bad = [dict(budget=0), dict(budget=(1 << 62) + 1), dict(budget=10, carry_in=10), dict(budget=10, carry_in=11), dict(budget=10, first=5, end=4),
           dict(budget=10, end=n + 1), dict(budget=10, first=n + 1, end=n + 1)]
    for kw in bad:
        with pytest.raises(EtlError) as e:
            b.cuts(m, **kw)
        assert e.value.kind == abi.InvalidArgument, kw
    with pytest.raises(EtlError) as e:
        b.cuts(None, 10)                                                   # neither a model nor hints
    assert e.value.kind == abi.InvalidArgument
    got, info = b.cuts(m, 1 << 62, (1 << 62) - 1, 0, 0)                    # the largest budget and carry: valid
    assert len(got) == 0 and int(info.carry_out) == (1 << 62) - 1
    assert int(b.cuts(None, 1 << 62, hints=ptr, end=1)[1].n_cuts) == 0     # hints without a model: valid
    del own


def test_a_downloaded_batch_is_refused():
    from etl_amd.decoder import EtlError
    c = _cfg2(65)
    c.check(1)
    c.b.host()                                                             # etlg_batch_download: the arena leaves the device
    with pytest.raises(EtlError) as e:
        c.b.cuts(c.m, 1)
    assert e.value.kind == abi.InvalidState and "etlg_batch_cuts" in e.value.description
    c.close()


def test_a_host_resident_batch_is_refused():
    from etl_amd.decoder import Decoder, EtlError
    w = synth.cfg2()
    buf, offs = w.fill(8 << 10)
    d = Decoder(0)
    w.register(d)
    b = d.decode(buf, offs)
    assert b.rc == 0
    with pytest.raises(EtlError) as e:
        b.cuts(BC.size_model(), 1)
    assert e.value.kind == abi.InvalidState
    b.close(); d.close()


# ---------------------------------------------------------------- etlg_cuts_locate

def _locate(c, row_event_ptr, n_rows, row_event, cut_list):
    """Host cuts, device cuts and device output against the model."""
    want = BC.locate(row_event, cut_list)
    got = c.b.locate(np.array(cut_list, dtype=np.uint64), row_event_ptr, n_rows)
    assert np.array_equal(got, want), (cut_list[:5], got[:5], want[:5])
    cown, cptr = _dev_put(np.array(cut_list, dtype=np.uint64))
    assert np.array_equal(c.b.locate(cptr, row_event_ptr, n_rows, n_cuts=len(cut_list)), want)
    oown, optr = _dev_put(np.full(len(cut_list), 0xEE, dtype=np.uint64))
    c.b.locate(cptr, row_event_ptr, n_rows, n_cuts=len(cut_list), out=optr)
    back = _dev_get(optr, len(cut_list) + 1)
    assert np.array_equal(back[:-1], want) and back[-1] == 0
    del cown, oown
    return want


def _cut_lists(c, h):
    total = int(h.sum())
    for budget in (1, max(1, total // 30), total):
        yield BC.cuts(h, budget)[0]
    yield [c.n]                                                            # a cut equal to n_events: every row lies in front of it
    yield [0, 1, c.n // 2, c.n // 2, c.n]


def test_locate_on_columns_and_rowbinary(cfg3):
    h, _ = _complete(cfg3)
    cols = cfg3.b.columns(0, kinds=("I", "U"), on_device=True)
    nf = np.ones(len(cfg3.hb.slots[0].cols) + 2, dtype=np.uint8)           # every destination column Nullable, and the two CDC columns
    rb = cfg3.b.rowbinary(0, nf, on_device=True)
    for obj, n_rows, ptr in ((cols, cols.n_rows, cols.view.row_event), (rb, rb.n_rows, rb.view.row_event)):
        assert n_rows > 50
        row_event = _dev_get(ptr, n_rows)
        for cl in _cut_lists(cfg3, h):
            want = _locate(cfg3, ptr, n_rows, row_event, cl)
            assert want[-1] == n_rows if cl[-1] == cfg3.n else True
        assert len(cfg3.b.locate(np.zeros(0, dtype=np.uint64), ptr, n_rows)) == 0           # n_cuts = 0
        assert list(cfg3.b.locate(np.array([0, 7, cfg3.n], dtype=np.uint64), ptr, 0)) == [0, 0, 0]   # n_rows = 0
    cols.close(); rb.close()


def test_locate_keeps_the_two_rows_of_a_key_changing_update_together():
    cols = [("id", SC.INT8, False, 1), ("v", SC.TEXT, True, 0)]
    msgs = []
    for i in range(0, 300, 3):
        msgs += [W.insert(42, [str(i), "a"]), W.update(42, [str(i + 1), "b"], key=[str(i), W.NULL]), W.insert(42, [str(i + 2), "c"])]
    c = _Case(SC.simple_table(cols), *_stream(msgs))
    pb = c.b.protobuf(0, on_device=True)
    row_event = _dev_get(pb.view.row_event, pb.n_rows)
    assert pb.n_rows == 400 and (np.diff(row_event.astype(np.int64)) == 0).sum() == 100    # DELETE + UPSERT of one event
    for cl in list(_cut_lists(c, c.hints)) + [[int(e) for e in row_event[::7]], [int(e) + 1 for e in row_event[::5]]]:
        want = _locate(c, pb.view.row_event, pb.n_rows, row_event, cl)
        for k, cut in zip(want.tolist(), cl):                                              # no pair is split: all rows in front are of earlier events
            assert (row_event[:k] < cut).all() and (row_event[k:] >= cut).all()
    pb.close(); c.close()


def test_cuts_and_locate_on_a_table_copy_batch():
    from etl_amd.decoder import Decoder
    cols = [("id", SC.INT8, False, 1), ("v", SC.TEXT, True, 0)]
    rows = [("%d\t%s\n" % (i, "x" * (i * 7 % 50))).encode() for i in range(300)]
    buf = np.frombuffer(b"".join(rows), dtype=np.uint8)
    offs = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint32)
    d = Decoder(0)
    d.schema_put(42, 0, cols)
    slot = d.table_ready(42, 0, [1, 1], [1, 0])
    b = d.copy_decode(slot, buf, offs, flags=abi.F_OUTPUT_ON_DEVICE)
    assert b.rc == 0, b.error
    m = BC.size_model()
    hints = b.size_hints(m)
    assert len(hints) == 300
    rb = b.rowbinary(slot, np.array([0, 1, 0, 0], dtype=np.uint8), on_device=True)
    assert np.array_equal(_dev_get(rb.view.row_event, rb.n_rows), np.arange(300, dtype=np.uint64))      # row_event[i] = i
    for budget in (1, int(hints.sum()) // 11, int(hints.sum())):
        want, wi = BC.cuts(hints, budget)
        got, info = b.cuts(m, budget)
        assert [int(x) for x in got] == want and {k: int(getattr(info, k)) for k in INFO} == wi
        assert np.array_equal(b.locate(got, rb.view.row_event, rb.n_rows), got)                         # a cut is its own row position
    rb.close(); b.close(); d.close()
