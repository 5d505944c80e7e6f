"""etlg_clickhouse_plan (etl_amd/csrc/finish.hip: k_chp_*) through the C ABI against tests/clickhouse_plan.py, the restatement of the
reference's write_events_inner refusals and insert_rows' loop as one sequential loop. Every case compares every field the call writes
with the model, exactly: the info, the statements and the windows. Every output buffer is one entry longer than its cap and filled
with a poison byte first: what lies at or beyond a count or a cap, the entry behind, and everything when the status is not OK must
still hold it. Each case runs with host passes and host outputs and again with device passes and device outputs; the two give the same
bytes. The model's row lengths are those of the device-resident etlg_batch_rowbinary object, whose bytes tests/test_gpu_rowbinary.py
checks.
The kernels' constants: waves of 64, workgroups of 256, the tile (2 048 events, or ETLG_CHP_TILE in a context of its own), the chunks
of 256 tile sums k_chp_scan walks and the jump levels, one per bit of the largest statement count a window can have. Three tables share
the streams round robin, so the slot's rows lie three events apart."""
import ctypes as C
import os

import numpy as np
import pytest

from etl_amd import abi
from tests import batch_cuts as BC
from tests import clickhouse_plan as CP
from tests import pgwire as W
from tests import scenarios as SC
from tests.test_gpu_ducklake_plan import COLS3, FILL, NAMES, _dev_bytes, _dev_get, _dev_put, _msg, _prime3

pytestmark = pytest.mark.gpu
MIX = "IIUDIRIID"                                                            # no partial Update: the sink refuses those
MT, RMT = abi.CH_MERGE_TREE, abi.CH_REPLACING_MERGE_TREE
NULLABLE = {0: [0, 1, 1, 0, 0], 1: [0, 1, 0, 0], 2: [0, 1, 0, 0]}            # the destination columns + the engine's two CDC columns
KCOLS = [("id", SC.INT8, False, 1), ("k", SC.INT4, False, 0), ("j", SC.INT4, False, 0), ("s", 25, True, 0)]
KFLAGS = [0, 0, 0, 1, 0, 0]
N = W.NULL


def _stream(groups, extra=None):
    """groups: one pattern string per transaction -> (buf, offsets). extra: {letter: message, or a function of the event's number}."""
    s, i = W.Stream(lsn=0x1000), 0
    for pat in groups:
        final = s.lsn + 8 * (len(pat) + 2)
        s.add(W.begin(final, ts=1234, xid=77))
        for k in pat:
            m = extra.get(k) if extra else None
            s.add(m(i) if callable(m) else m if m is not None else _msg(k, i))
            i += 1
        s.add(W.commit(final, final + 8, ts=5678, flags=0), lsn=final)
    return np.frombuffer(s.bytes(), dtype=np.uint8), s.offsets


def _round_robin(n, mix=MIX):
    return "".join((mix[(i // 3) % len(mix)], "x", "y")[i % 3] for i in range(n))


# one table whose replica identity the case chooses: i Insert, u full Update with a key image, d key-only Delete, o Delete with the
# full old row, p partial Update
def _kmsgs(ident):
    key = lambda i: [str(i) if ident[0] else N, str(i) if ident[1] else N, str(i) if ident[2] else N, N]
    return {"i": lambda i: W.insert(42, [str(i), str(i), str(i), "s%d" % i]),
            "u": lambda i: W.update(42, [str(i), str(i), str(i), "u%d" % i], key=key(i)),
            "d": lambda i: W.delete(42, key=key(i)),
            "p": lambda i: W.update(42, [str(i), str(i), str(i), W.TOAST], key=key(i))}


class _Case:
    def __init__(self, groups=None, tile=None, slot=0, engine=MT, stream=None, prime=None, cols=None, ident=None, nullable=None, copy=None, extra=None):
        from etl_amd.decoder import Decoder
        from etl_amd.schema import infer_identity_type
        from oracle import oracle
        before = os.environ.get("ETLG_CHP_TILE")
        if tile:
            os.environ["ETLG_CHP_TILE"] = str(tile)                            # read when the context is created
        else:
            os.environ.pop("ETLG_CHP_TILE", None)
        try:
            self.d = Decoder(0)
        finally:
            os.environ.pop("ETLG_CHP_TILE", None)
            if before is not None:
                os.environ["ETLG_CHP_TILE"] = before
        o = oracle.Oracle()
        self.copy = copy is not None
        if self.copy:
            cols, rows = copy
            for t in (o, self.d):
                t.schema_put(42, 0, cols)
            so = o.table_ready(42, 0, [1] * len(cols), [1 if c[3] else 0 for c in cols])
            sd = self.d.table_ready(42, 0, [1] * len(cols), [1 if c[3] else 0 for c in cols])
            buf = np.frombuffer(b"".join(rows), dtype=np.uint8)
            offs = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint32)
            rb, self.b = o.copy_decode(so, buf, offs), self.d.copy_decode(sd, buf, offs, flags=abi.F_OUTPUT_ON_DEVICE)
        else:
            buf, offs = stream or _stream(groups, extra)
            prime = prime or (SC.simple_table(cols, ident=ident) if cols else _prime3())
            prime(self.d)
            prime(o)
            self.b = self.d.decode(buf, offs, flags=abi.F_OUTPUT_ON_DEVICE)
            rb = o.decode(buf, offs)
        assert self.b.rc == 0, self.b.error
        assert rb.err_code == 0, rb.err_desc
        self.hb = rb.host_batch()
        self.ev = CP.of_host_batch(self.hb)
        self.n, self.slot, self.engine = len(self.ev[0]), slot, engine
        self.members = [i for i in range(self.n) if self.ev[0][i] in "IUD" and int(self.ev[2][i]) == slot]
        cols = cols or (COLS3 if slot == 0 else None)
        ident = ident if ident is not None else ([1 if c[3] else 0 for c in cols] if cols else [1, 0])
        self.identity = dict(identity_type=infer_identity_type(cols, [1] * len(cols), ident) if cols else "PrimaryKey",
                             n_ident=sum(ident), n_pk=sum(1 for c in cols if c[3]) if cols else 1)
        self.nullable = nullable or NULLABLE[slot]
        self.rb = self.b.rowbinary(slot, self.nullable, engine, on_device=True)
        self.host_event = None
        if self.rb.status == abi.RB_OK:
            r = int(self.rb.n_rows)
            self.row_event = _dev_get(self.rb.view.row_event, r).tolist()
            self.offs = _dev_bytes(self.rb.view.row_offsets, 8 * (r + 1)).view(np.int64)
            self.lens = np.diff(self.offs).tolist()
            assert self.lens == [] or min(self.lens) > 0
        else:
            self.row_event, self.lens, self.host_event = None, None, int(self.rb.view.host_event)

    def model(self, windows, max_bytes=CP.MAX_BYTES_PER_INSERT):
        return CP.plan(*self.ev, self.slot, windows, self.row_event, self.lens, engine=self.engine, max_bytes=max_bytes,
                       needs_host_event=self.host_event, **self.identity)

    def raw(self, windows, max_bytes, scap, dev, skip=(), passes=True, rb=None):
        """One call with poison-filled buffers of scap statements / one entry per window and a guard entry each -> (rc, info, {name: words})."""
        nwin = len(windows) if (len(windows) or not self.copy) else 1
        words = {"statements": 7 * (scap + 1), "windows": 6 * (nwin + 1)}
        pa = np.full((len(windows), 7), FILL, dtype=np.uint64)                  # only first_event and data_end are read
        for p, (lo, hi) in enumerate(windows):
            pa[p, 0], pa[p, 1] = lo, hi
        bufs = {k: np.full(words[k], FILL, dtype=np.uint64) for k in words if k not in skip}
        owners = {k: _dev_put(a) for k, a in bufs.items()} if dev else {}
        pown = _dev_put(pa.reshape(-1)) if dev else None
        ptr = lambda k: None if k in skip else (owners[k][1] if dev else bufs[k].ctypes.data)
        pptr = None if not passes or not len(windows) else (pown[1] if dev else pa.ctypes.data)
        info = abi.ChPlanInfo()
        rc = self.d.L.etlg_clickhouse_plan(self.d.h, self.b.h, self.slot, pptr, len(windows), 1 if dev and pptr else 0, (rb or self.rb).h, max_bytes,
                                           abi.F_OUTPUT_ON_DEVICE if dev else 0, ptr("statements"), scap, ptr("windows"), C.byref(info))
        if dev:
            bufs = {k: _dev_get(owners[k][1], words[k]) for k in bufs}
        return rc, info, bufs

    def check(self, windows, max_bytes=CP.MAX_BYTES_PER_INSERT, scap=None, skip=(), model_windows=None):
        """Host and device memory against the model, field by field; returns the model."""
        m = self.model(model_windows or windows, max_bytes)
        assert m["status"] == CP.OK, m
        scap = m["info"]["n_stmts"] if scap is None else scap
        got = {}
        for dev in (False, True):
            rc, info, bufs = self.raw(windows, max_bytes, scap, dev, skip)
            assert rc == abi.OK and info.status == abi.CHP_OK, (rc, info.status, int(info.event), int(info.bad_pass), info.reason)
            gi = {k: int(getattr(info, k)) for k in CP.INFO_FIELDS}
            assert gi == m["info"], (dev, gi, m["info"])
            assert (int(info.event), int(info.bad_pass), int(info.fail_pass), info.reason) == (CP.NONE, CP.NONE, CP.NONE, 0)
            self.compare(m, bufs, scap, dev)
            got[dev] = bufs
        for k in got[False]:
            assert np.array_equal(got[False][k], got[True][k]), k              # host and device output pointers: the same bytes
        for s in m["statements"]:                                               # a statement never crosses a window
            wn = m["windows"][s["window"]]
            assert wn["first_row"] <= s["first_row"] < s["end_row"] <= wn["end_row"]
        return m

    def compare(self, m, bufs, scap, dev):
        S, P = min(scap, len(m["statements"])), len(m["windows"])
        if "statements" in bufs:
            want = np.array([[s[f] for f in CP.STMT_FIELDS] for s in m["statements"][:S]], dtype=np.uint64).reshape(S, 7)
            got = bufs["statements"][:7 * S].reshape(S, 7)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert not len(bad), (dev, int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())
            assert (bufs["statements"][7 * S:] == FILL).all(), dev
        if "windows" in bufs:
            want = np.array([[w[f] for f in CP.WIN_FIELDS] for w in m["windows"]], dtype=np.uint64).reshape(P, 6)
            got = bufs["windows"][:6 * P].reshape(P, 6)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert not len(bad), (dev, int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())
            assert (bufs["windows"][6 * P:] == FILL).all(), dev

    def status(self, windows, want, max_bytes=CP.MAX_BYTES_PER_INSERT, **fields):
        """A status other than OK, on host and device memory: every field of the info, and every output word still poison."""
        m = self.model(windows, max_bytes)
        assert m["status"] == want and all(m[k] == v for k, v in fields.items()), m
        full = (m.get("event", CP.NONE), m.get("bad_pass", CP.NONE), m.get("fail_pass", CP.NONE), m.get("reason", 0))
        for dev in (False, True):
            rc, info, bufs = self.raw(windows, max_bytes, 8, dev)
            assert rc == abi.OK and info.status == want, (dev, rc, info.status, int(info.event))
            assert (int(info.event), int(info.bad_pass), int(info.fail_pass), info.reason) == full, (dev, int(info.event), int(info.bad_pass), int(info.fail_pass), info.reason, m)
            assert all(int(getattr(info, k)) == 0 for k in CP.INFO_FIELDS), dev
            assert all((a == FILL).all() for a in bufs.values()), dev

    def close(self):
        self.rb.close(); self.b.close(); self.d.close()


def _whole(c):
    return [(0, c.n)]


def _stmt_rows(m):
    return [s["end_row"] - s["first_row"] for s in m["statements"]]


# ---------------------------------------------------------------- tiles, windows

@pytest.mark.parametrize("tile,engine", [(8, RMT), (512, MT), (None, RMT)])
def test_tiles(tile, engine):
    """6 000 events: more than a wave, a workgroup, two tiles of 2 048, and with tiles of 8 more than two chunks of 256 tile sums."""
    n = 6000
    c = _Case([_round_robin(n // 2), _round_robin(n - n // 2)], tile=tile, engine=engine)
    assert c.n > 2 * 2048 and len(c.members) == n // 3 and len(c.row_event) == len(c.members)
    b50 = 50 * int(np.mean(c.lens))                                          # statements of about 50 rows: 150 events, straddling tiles of 8
    m = c.check(_whole(c), max_bytes=b50)
    assert 30 < np.mean(_stmt_rows(m)) < 70 and len(m["statements"]) > 30
    mid = c.members[len(c.members) // 2] + 1                                    # windows that start in the middle of a tile
    t = min(tile or 2048, c.n // 4)
    wins = [(3, t + 5), (t + 5, t + 5), (t + 7, mid), (mid + 1, c.n - 2)]
    m = c.check(wins, max_bytes=b50)
    assert [w["n_stmts"] for w in m["windows"]][1] == 0 and m["windows"][3]["n_stmts"] > 5
    last = [m["statements"][w["stmt_first"] + w["n_stmts"] - 1] for w in m["windows"] if w["n_stmts"]]
    assert any(s["byte_end"] - s["byte_first"] < b50 for s in last)             # a window whose last statement is short
    m = c.check(wins, max_bytes=1)                                              # a statement per row: as many jump levels as the rows have bits
    assert m["info"]["n_stmts"] == m["info"]["n_rows"] > 1024
    c.close()
    c1 = _Case([_round_robin(n)], tile=tile, slot=1, engine=engine)             # another slot of the same stream
    c1.check([(0, c1.n // 2), (c1.n // 2, c1.n)], max_bytes=700)
    c1.close()


def test_window_shapes():
    c = _Case([_round_robin(300), _round_robin(240)])
    ms, ln = c.members, int(np.mean(c.lens))
    c.check(_whole(c), max_bytes=4 * ln)                                        # one window
    m = c.check([(i, i + 1) for i in range(c.n)], max_bytes=4 * ln)             # a window per event: every row a statement of its own
    assert m["info"]["n_stmts"] == len(ms) and _stmt_rows(m) == [1] * len(ms)
    m = c.check([(0, 10), (10, 10), (10, 40), (40, 40), (c.n, c.n)], max_bytes=2 * ln)   # empty windows, one at the very end
    assert [w["n_stmts"] > 0 for w in m["windows"]] == [True, False, True, False, False]
    assert m["windows"][4]["first_row"] == m["windows"][4]["end_row"] == len(c.row_event)
    gap = next(i for i in range(c.n - 1) if i not in ms and i + 1 not in ms)   # (Begin and a neighbour of another slot)
    m = c.check([(0, gap), (gap, gap + 2), (gap + 2, c.n)], max_bytes=3 * ln)   # a window without a member of the slot
    assert m["windows"][1]["n_members"] == 0 and m["windows"][1]["n_stmts"] == 0
    # the outline's passes over the cuts of a small budget, handed over as they are
    sm = BC.size_model()
    total = int(c.b.cuts(sm, 1 << 62, cap=0)[1].total)
    cuts, ci = c.b.cuts(sm, max(1, total // 9))
    ol = c.b.outline(cuts=cuts)
    assert ol.info.status == abi.OL_OK and len(ol.passes) >= 9
    wins = [(int(p[0]), int(p[1])) for p in ol.passes]
    m = c.check(wins, max_bytes=5 * ln)
    got = c.b.clickhouse_plan(0, ol.passes, c.rb, max_bytes_per_insert=5 * ln)
    assert got.info.status == abi.CHP_OK and len(got.statements) == m["info"]["n_stmts"] and len(got.windows) == len(wins)
    assert [[int(getattr(s, f)) for f in CP.STMT_FIELDS] for s in got.statements] == [[s[f] for f in CP.STMT_FIELDS] for s in m["statements"]]
    assert [[int(getattr(w, f)) for f in CP.WIN_FIELDS] for w in got.windows] == [[w[f] for f in CP.WIN_FIELDS] for w in m["windows"]]
    for dev in (False, True):                                                   # n_passes == 0, with and without a pointer
        for passes in (True, False):
            rc, info, bufs = c.raw([], 100, 4, dev, passes=passes)
            assert rc == abi.OK and info.status == abi.CHP_OK and all(int(getattr(info, k)) == 0 for k in CP.INFO_FIELDS)
            assert all((a == FILL).all() for a in bufs.values())
    c.close()


def test_relation_and_truncate_passes():
    """A stream whose passes end at a Relation and at a Truncate: the windows are the outline's [first_event, data_end)."""
    rel = W.relation(43, "public", "t43", "d", [(1, "id", SC.INT8, -1), (0, "t", 25, -1)])
    pat = _round_robin(60) + "T" + _round_robin(45) + "L" + _round_robin(30) + "TT" + _round_robin(30)
    c = _Case([pat], extra={"T": W.truncate([43], 0), "L": rel}, engine=RMT)
    ol = c.b.outline()
    assert ol.info.status == abi.OL_OK and len(ol.passes) >= 4 and int(ol.info.n_trunc) >= 2 and int(ol.info.n_relations) >= 1
    wins = [(int(p[0]), int(p[1])) for p in ol.passes]
    m = c.check(wins, max_bytes=3 * int(np.mean(c.lens)))
    assert sum(1 for w in m["windows"] if w["n_stmts"]) >= 4
    c.close()


# ---------------------------------------------------------------- max_bytes_per_insert

@pytest.mark.parametrize("engine", [MT, RMT])
def test_budget_values(engine):
    c = _Case([_round_robin(450), _round_robin(300)], engine=engine)
    ms = c.members
    m = c.check(_whole(c), max_bytes=1)                                         # every row its own statement
    assert _stmt_rows(m) == [1] * len(ms)
    k = len(ms) // 2
    prefix = int(c.offs[k])                                                     # the bytes of the first k rows
    assert min(c.lens) > 1
    assert _stmt_rows(c.check(_whole(c), max_bytes=prefix))[0] == k             # exactly a prefix of row lengths: the statement closes on that row
    assert _stmt_rows(c.check(_whole(c), max_bytes=prefix - 1))[0] == k         # one less: the k-th row still reaches it
    assert _stmt_rows(c.check(_whole(c), max_bytes=prefix + 1))[0] == k + 1     # one more: the statement takes one more row
    wins = [(0, ms[k]), (ms[k], c.n)]                                           # the same rule met on a window's first row
    for f in (c.lens[k], c.lens[k] - 1, c.lens[k] + 1):                         # a single row's length
        c.check(_whole(c), max_bytes=f)
        m2 = c.check(wins, max_bytes=f)
        first = m2["statements"][m2["windows"][1]["stmt_first"]]
        assert first["first_row"] == k and first["end_row"] - k == (1 if c.lens[k] >= f else 2)
    m = c.check(wins, max_bytes=sum(c.lens) + 1)                                # more than all bytes: one statement per window
    assert [w["n_stmts"] for w in m["windows"]] == [1, 1]
    m = c.check(wins)                                                           # the reference's 64 MiB
    assert [w["n_stmts"] for w in m["windows"]] == [1, 1] and m["info"]["n_bytes"] == sum(c.lens)
    c.check(wins, max_bytes=1 << 63)
    m = c.check(_whole(c), max_bytes=50 * int(np.mean(c.lens)))                 # about 50 rows per statement
    assert 30 < np.mean(_stmt_rows(m)) < 70
    c.close()


# ---------------------------------------------------------------- failing members, both engines

def test_alternative_key_updates_fail_under_replacing_merge_tree_only():
    groups, ident = ["iiuiui"], [0, 1, 0, 0]
    c = _Case(groups, cols=KCOLS, ident=ident, nullable=KFLAGS, extra=_kmsgs(ident), engine=RMT)
    assert c.identity == {"identity_type": "AlternativeKey", "n_ident": 1, "n_pk": 1}
    ms = c.members
    c.status(_whole(c), CP.FAILED, event=ms[2], reason=CP.R_UPDATE_IDENTITY, fail_pass=0)
    c.status([(0, ms[1]), (ms[1], ms[3]), (ms[3], c.n)], CP.FAILED, event=ms[2], reason=CP.R_UPDATE_IDENTITY, fail_pass=1)   # fail_pass names the window
    c.status([(0, ms[2]), (ms[2] + 1, c.n)], CP.FAILED, event=ms[4], reason=CP.R_UPDATE_IDENTITY, fail_pass=1)   # outside every window the first one does not count
    c.check([(0, ms[2]), (ms[2] + 1, ms[4])], max_bytes=1)                      # ... nor does either
    c.close()
    c = _Case(groups, cols=KCOLS, ident=ident, nullable=KFLAGS, extra=_kmsgs(ident), engine=MT)   # the same table under MergeTree: a plan
    m = c.check(_whole(c), max_bytes=2 * min(c.lens))
    assert m["info"]["n_members"] == 6 and m["info"]["n_stmts"] >= 3
    c.close()
    for full in ([1, 1, 1, 1], [1, 0, 0, 0]):                                   # Full and PrimaryKey pass under ReplacingMergeTree
        c = _Case(["iiuiui"], cols=KCOLS, ident=full, nullable=KFLAGS, engine=RMT,
                  extra=dict(_kmsgs([1, 0, 0, 0]), u=lambda i: W.update(42, [str(i)] * 3 + ["u"], old=[str(i)] * 3 + ["o"]) if full[1] else W.update(42, [str(i)] * 3 + ["u"], key=[str(i), N, N, N])))
        assert c.check(_whole(c), max_bytes=1)["info"]["n_stmts"] == 6
        c.close()


@pytest.mark.parametrize("engine", [MT, RMT])
def test_key_only_deletes(engine):
    ident = [0, 1, 0, 0]                                                        # an alternative key as wide as the primary key: the identity is refused
    c = _Case(["iidi"], cols=KCOLS, ident=ident, nullable=KFLAGS, extra=_kmsgs(ident), engine=engine)
    c.status(_whole(c), CP.FAILED, event=c.members[2], reason=CP.R_KEY_IDENTITY, fail_pass=0)
    c.check([(0, c.members[2])], max_bytes=1)
    c.close()
    ident = [0, 1, 1, 0]                                                        # ... and a wider one: the width is tested first
    c = _Case(["iidi"], cols=KCOLS, ident=ident, nullable=KFLAGS, extra=_kmsgs(ident), engine=engine)
    assert c.identity == {"identity_type": "AlternativeKey", "n_ident": 2, "n_pk": 1}
    c.status(_whole(c), CP.FAILED, event=c.members[2], reason=CP.R_KEY_WIDTH, fail_pass=0)
    c.close()
    ident = [1, 0, 0, 0]                                                        # the primary key: a tombstone row, no refusal
    c = _Case(["iidi"], cols=KCOLS, ident=ident, nullable=KFLAGS, extra=_kmsgs(ident), engine=engine)
    assert c.check(_whole(c), max_bytes=1)["info"]["n_stmts"] == 4
    c.close()


@pytest.mark.parametrize("engine", [MT, RMT])
def test_partial_update_and_the_lowest_event(engine):
    c = _Case(["IIPIxI"], engine=engine)                                       # _msg's P: a partial Update of table 42
    ms = c.members
    c.status(_whole(c), CP.FAILED, event=ms[2], reason=CP.R_PARTIAL_UPDATE, fail_pass=0)
    c.check([(0, ms[2]), (ms[2] + 1, c.n)], max_bytes=1)                        # outside every window it does not count
    c1 = _Case(["IIPIxI"], slot=1, engine=engine)                               # ... nor for another slot
    c1.check(_whole(c1))
    c.close(); c1.close()
    ident = [0, 1, 0, 0]                                                        # two failing events of different reasons: the lowest event wins
    c = _Case(["iipdi"], cols=KCOLS, ident=ident, nullable=KFLAGS, extra=_kmsgs(ident), engine=engine)
    ms = c.members
    c.status(_whole(c), CP.FAILED, event=ms[2], reason=CP.R_PARTIAL_UPDATE, fail_pass=0)
    c.status([(0, ms[2]), (ms[3], c.n)], CP.FAILED, event=ms[3], reason=CP.R_KEY_IDENTITY, fail_pass=1)
    c.close()
    c = _Case(["iidpi"], cols=KCOLS, ident=ident, nullable=KFLAGS, extra=_kmsgs(ident), engine=engine)
    ms = c.members
    c.status(_whole(c), CP.FAILED, event=ms[2], reason=CP.R_KEY_IDENTITY, fail_pass=0)
    c.status([(0, 1), (1, ms[2]), (ms[2] + 1, c.n)], CP.FAILED, event=ms[3], reason=CP.R_PARTIAL_UPDATE, fail_pass=2)
    c.close()


# ---------------------------------------------------------------- caps, NULL outputs, statuses

def test_caps_and_null_outputs():
    c = _Case([_round_robin(300)], engine=RMT)
    f = 3 * int(np.mean(c.lens))
    wins = [(0, 100), (100, 100), (101, c.n)]
    ns = c.model(wins, f)["info"]["n_stmts"]
    assert ns > 8
    for scap in (0, 1, ns - 1, ns, ns + 5):
        c.check(wins, max_bytes=f, scap=scap)                                   # the full count comes back, nothing is written past the cap
    c.check(wins, max_bytes=f, skip=("statements",))                            # any output may be NULL
    c.check(wins, max_bytes=f, skip=("windows",))
    c.check(wins, max_bytes=f, skip=("statements", "windows"))
    c.close()


def test_bad_passes():
    c = _Case([_round_robin(60)])
    c.status([(0, 10), (12, 11), (20, 30)], CP.BAD_PASSES, bad_pass=1)          # first_event > data_end
    c.status([(0, 10), (20, c.n + 1)], CP.BAD_PASSES, bad_pass=1)               # beyond n_events
    c.status([(0, 10), (9, 30), (5, 40)], CP.BAD_PASSES, bad_pass=1)            # starts below its predecessor's end; the lowest index
    c.status([(c.n + 1, c.n + 1)], CP.BAD_PASSES, bad_pass=0)
    c.status([(i, i + 1) for i in range(40)] + [(39, 41)], CP.BAD_PASSES, bad_pass=40)
    c.close()
    c = _Case(["IIPI"])                                                         # BAD_PASSES comes before FAILED
    c.status([(2, 1)], CP.BAD_PASSES, bad_pass=0)
    c.close()


def test_needs_host_for_a_tombstone_the_host_builds():
    """A nullable `money` column: its key-only Deletes have no row in the object (handoff_plan.h: only the host knows every array type)."""
    cols = [("id", SC.INT8, False, 1), ("m", 790, True, 0)]
    msgs = [W.insert(42, ["1", "$2.00"]), W.insert(42, ["2", "$3.00"]), W.delete(42, key=["1", N]), W.insert(42, ["3", N]), W.delete(42, key=["2", N])]
    s = SC.txn(msgs)
    for engine in (MT, RMT):
        c = _Case(stream=(np.frombuffer(s.bytes(), dtype=np.uint8), s.offsets), cols=cols, nullable=[0, 1, 0, 0], engine=engine)
        ms = c.members
        assert c.rb.status == abi.RB_OK and len(c.row_event) == 3 and len(ms) == 5
        c.status(_whole(c), CP.NEEDS_HOST, event=ms[2], fail_pass=0)
        c.status([(0, ms[1]), (ms[1], ms[3]), (ms[3], c.n)], CP.NEEDS_HOST, event=ms[2], fail_pass=1)
        c.status([(0, ms[2]), (ms[3], c.n)], CP.NEEDS_HOST, event=ms[4], fail_pass=1)
        m = c.check([(0, ms[2]), (ms[3], ms[4])], max_bytes=1)                  # the windows without them: a plan
        assert m["info"]["n_stmts"] == 3
        c.close()
    s = SC.txn([W.delete(42, key=["1", N]), W.delete(42, key=["2", N])])        # an object without any row
    c = _Case(stream=(np.frombuffer(s.bytes(), dtype=np.uint8), s.offsets), cols=cols, nullable=[0, 1, 0, 0])
    assert c.rb.status == abi.RB_OK and int(c.rb.n_rows) == 0
    c.status(_whole(c), CP.NEEDS_HOST, event=c.members[0], fail_pass=0)
    c.close()


def test_needs_host_object():
    """A RowBinary object that came back NEEDS_HOST for an array literal the device does not take apart: its host_event is reported,
    behind the statuses that come first."""
    cols = [("id", SC.INT8, False, 1), ("a", 1007, True, 0)]
    msgs = [W.insert(42, ["1", "{1,2}"]), W.insert(42, ["2", "{1,{2}}"]), W.insert(42, ["3", "{}"])]
    s = SC.txn(msgs)
    c = _Case(stream=(np.frombuffer(s.bytes(), dtype=np.uint8), s.offsets), cols=cols, nullable=[0, 1, 0, 0])
    assert c.rb.status == abi.RB_NEEDS_HOST and c.host_event == c.members[1]
    c.status(_whole(c), CP.NEEDS_HOST, event=c.members[1], fail_pass=CP.NONE)
    c.status([(0, c.members[1])], CP.NEEDS_HOST, event=c.members[1])            # the object has no rows, whatever the windows hold
    c.status([(2, 1)], CP.BAD_PASSES, bad_pass=0)                               # a status in front of it
    rc, info, bufs = c.raw([], 100, 4, False)
    assert rc == abi.OK and info.status == abi.CHP_NEEDS_HOST and int(info.event) == c.members[1]
    c.close()
    msgs = [W.insert(42, ["1", "{1,2}"]), W.update(42, ["2", W.TOAST], key=["2", N]), W.insert(42, ["2", "{1,{2}}"])]   # FAILED comes first
    s = SC.txn(msgs)
    c = _Case(stream=(np.frombuffer(s.bytes(), dtype=np.uint8), s.offsets), cols=cols, nullable=[0, 1, 0, 0])
    assert c.rb.status == abi.RB_NEEDS_HOST
    c.status(_whole(c), CP.FAILED, event=c.members[1], reason=CP.R_PARTIAL_UPDATE, fail_pass=0)
    c.close()


def test_table_copy_batch():
    cols = [("id", SC.INT8, False, 1), ("s", 25, True, 0), ("f", SC.FLOAT8, True, 0)]
    rows = [b"%d\ttext %d\\twith tab\t%s\n" % (i, i, b"1.5" if i % 2 else b"\\N") for i in range(700)]
    for engine in (MT, RMT):
        c = _Case(copy=(cols, rows), tile=64, cols=cols, nullable=[0, 1, 1, 0, 0], engine=engine)
        assert c.n == 700 and c.row_event == list(range(700))
        f = 20 * int(np.mean(c.lens))
        m = c.check([], max_bytes=f, model_windows=_whole(c))                   # no passes: one window over all rows
        assert len(m["statements"]) > 20 and m["statements"][3]["first_event"] == m["statements"][3]["first_row"]   # row indexes
        c.check([(0, 300), (300, 700)], max_bytes=f)
        c.check([], model_windows=_whole(c))                                    # write_table_rows' budget: the same 64 MiB
        c.close()


def test_wrong_objects_and_invalid_arguments():
    c = _Case(["IUD", "II"])
    info = abi.ChPlanInfo()
    pa = np.array([[0, c.n, 0, 0, 0, 0, 0]], dtype=np.uint64)

    def call(batch, slot=0, passes=pa.ctypes.data, n=1, rb=c.rb, max_bytes=100):
        return c.d.L.etlg_clickhouse_plan(c.d.h, batch.h, slot, passes, n, 0, rb.h if rb is not None else None, max_bytes, 0, None, 0, None, C.byref(info))

    assert call(c.b) == abi.OK and (int(info.n_members), int(info.n_rows)) == (5, 5)
    assert call(c.b, slot=7) == abi.InvalidArgument and call(c.b, slot=-1) == abi.InvalidArgument          # an unknown slot
    assert call(c.b, passes=None, n=1) == abi.InvalidArgument                                              # n_passes without passes
    assert call(c.b, max_bytes=0) == abi.InvalidArgument and call(c.b, max_bytes=(1 << 63) + 1) == abi.InvalidArgument   # 0: the reference's loop never ends
    assert call(c.b, max_bytes=1 << 63) == abi.OK and int(info.n_stmts) == 1 and call(c.b, max_bytes=1) == abi.OK and int(info.n_stmts) == 5
    assert call(c.b, rb=None) == abi.InvalidArgument                                                       # the object is required
    pb = c.b.protobuf(0, on_device=True)
    nd = c.b.ndjson(0, NAMES[0], on_device=True)
    dl = c.b.duckdb(0, NAMES[0], what=abi.DL_TUPLES, on_device=True)
    other = c.b.rowbinary(1, NULLABLE[1], on_device=True)
    host = c.b.rowbinary(0, NULLABLE[0], on_device=False)
    assert call(c.b, rb=pb) == abi.InvalidArgument                                                         # a protobuf object
    assert call(c.b, rb=nd) == abi.InvalidArgument                                                         # an NDJSON object
    assert call(c.b, rb=dl) == abi.InvalidArgument                                                         # a DuckLake object
    assert call(c.b, rb=other) == abi.InvalidArgument and call(c.b, slot=1, rb=other) == abi.OK            # another slot's
    assert call(c.b, rb=host) == abi.InvalidArgument                                                       # host-resident
    buf, offs = _stream(["IUD", "II"])
    b2 = c.d.decode(buf, offs, flags=abi.F_OUTPUT_ON_DEVICE)
    assert call(b2) == abi.InvalidArgument                                                                 # another batch's object
    b2.close()
    bh = c.d.decode(buf, offs)                                                                             # a batch that is not device-resident
    assert call(bh) == abi.InvalidArgument
    bh.close()
    ba = c.d.decode(buf, offs, flags=abi.F_OUTPUT_ON_DEVICE | abi.F_ASYNC)                                 # an ASYNC batch is synced first
    rba = ba.rowbinary(0, NULLABLE[0], on_device=True)
    assert call(ba, rb=rba) == abi.OK and int(info.n_members) == 5
    rba.close(); ba.close()
    bad = np.frombuffer(bytes(buf[:int(offs[2])]) + b"\xFF" * 24, dtype=np.uint8)                          # one that ended in a decode error gives that error
    be = c.d.decode(bad, list(offs[:3]) + [len(bad)], flags=abi.F_OUTPUT_ON_DEVICE | abi.F_ASYNC)
    assert call(be) not in (abi.OK, abi.InvalidArgument)
    be.close()
    pb.close(); nd.close(); dl.close(); other.close(); host.close()
    c.close()
