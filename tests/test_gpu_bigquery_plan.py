"""etlg_bigquery_plan (etl_amd/csrc/finish.hip: k_bqp_*) through the C ABI against tests/bigquery_plan.py, the restatement of the
reference's write_events refusals, its one append request per table and turn, and the two table-copy functions. Every case compares
every field the call writes with the model, exactly: the info, the requests and the windows. Every output buffer is one entry longer
than its cap and filled with a poison byte first: what lies at or beyond a count or a cap, the entry behind, and everything when the
status is not OK must still hold it. Each case runs with host passes and host outputs and again with device passes and device
outputs; the two give the same bytes. The model's rows — which event owns one, which two, and their lengths — are those of the
device-resident etlg_batch_protobuf object, whose bytes tests/test_gpu_protobuf.py checks.
The kernels' constants: waves of 64, workgroups of 256, the tile (2 048 events, or ETLG_BQP_TILE in a context of its own) and the
chunks of 256 tile sums k_bqp_scan walks. Three tables share the streams round robin, so the slot's members lie three events apart.
pgoutput has no Delete without an old image: ETLG_BQP_R_DELETE_NO_OLD is reachable in the model alone
(tests/test_bigquery_plan_model.py), as ETLG_CHP_R_DELETE_NO_OLD is. Of the adjacent pairs in the reference's order, an Update without
an old image cannot also carry a key image and a Delete with a key image has an old image, so the pairs one event can meet are
PARTIAL_UPDATE with each Update reason behind it and KEY_WIDTH with KEY_IDENTITY."""
import ctypes as C
import os

import numpy as np
import pytest

from etl_amd import abi
from tests import batch_cuts as BC
from tests import bigquery_plan as BP
from tests import pgwire as W
from tests import scenarios as SC
from tests.golden import bigquery_split_kats as KATS
from tests.test_gpu_ducklake_plan import COLS3, FILL, NAMES, _dev_bytes, _dev_get, _dev_put, _msg, _prime3

pytestmark = pytest.mark.gpu
N = W.NULL
# table 42 beside _msg's letters (I, U: key image and the same key, D: key image, R: no old image, P: partial): K / F an Update whose key
# image / full old image holds another key — two rows —, G a full old image and the same key, O a Delete with the full old row
MOVED = {"K": lambda i: W.update(42, [str(i + 10 ** 6), str(i), "k%d" % i], key=[str(i), N, N]),
         "F": lambda i: W.update(42, [str(i + 10 ** 6), str(i), "f%d" % i], old=[str(i), "7", "old"]),
         "G": lambda i: W.update(42, [str(i), str(i), "g%d" % i], old=[str(i), "7", "old"]),
         "O": lambda i: W.delete(42, old=[str(i), N, "gone"])}
MIX = "IUKDIFOKGRI"
KCOLS = [("id", SC.INT8, False, 1), ("k", SC.INT4, False, 0), ("j", SC.INT4, False, 0), ("s", 25, True, 0)]
PK2COLS = [("id", SC.INT8, False, 1), ("k", SC.INT4, False, 1), ("j", SC.INT4, False, 0), ("s", 25, True, 0)]   # a primary key of two columns


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


# one table whose replica identity the case chooses: i Insert, u full Update with a key image, r full Update without an old image,
# d key-only Delete, o Delete with the full old row, p partial Update with a key image, q partial Update without an old image
def _kmsgs(ident):
    key = lambda i: [str(i) if ident[0] else N, str(i) if ident[1] else N, str(i) if ident[2] else N, N]
    return {"i": lambda i: W.insert(42, [str(i), str(i), str(i), "s%d" % i]),
            "u": lambda i: W.update(42, [str(i), str(i), str(i), "u%d" % i], key=key(i)),
            "r": lambda i: W.update(42, [str(i), str(i), str(i), "r%d" % i]),
            "d": lambda i: W.delete(42, key=key(i)),
            "o": lambda i: W.delete(42, old=[str(i), str(i), str(i), "o"]),
            "p": lambda i: W.update(42, [str(i), str(i), str(i), W.TOAST], key=key(i)),
            "q": lambda i: W.update(42, [str(i), str(i), str(i), W.TOAST])}


class _Case:
    def __init__(self, groups=None, tile=None, slot=0, stream=None, prime=None, cols=None, ident=None, copy=None, extra=MOVED):
        from etl_amd.decoder import Decoder
        from etl_amd.schema import infer_identity_type
        from oracle import oracle
        before = os.environ.get("ETLG_BQP_TILE")
        if tile:
            os.environ["ETLG_BQP_TILE"] = str(tile)                            # read when the context is created
        else:
            os.environ.pop("ETLG_BQP_TILE", None)
        try:
            self.d = Decoder(0)
        finally:
            os.environ.pop("ETLG_BQP_TILE", None)
            if before is not None:
                os.environ["ETLG_BQP_TILE"] = before
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
        self.ev = BP.of_host_batch(self.hb)
        self.n, self.slot = len(self.ev[0]), slot
        self.members = [i for i in range(self.n) if self.ev[0][i] in "IUD" and int(self.ev[2][i]) == slot]
        cols = cols or (COLS3 if slot == 0 else None)
        ident = ident if ident is not None else ([1 if c[3] else 0 for c in cols] if cols else [1, 0])
        self.identity = dict(identity_type=infer_identity_type(cols, [1] * len(cols), ident) if cols else "PrimaryKey",
                             n_ident=sum(ident), n_pk=sum(1 for c in cols if c[3]) if cols else 1)
        self.pb = self.b.protobuf(slot, on_device=True)
        self.host_event = None
        if self.pb.status == abi.RB_OK:
            r = int(self.pb.n_rows)
            self.row_event = _dev_get(self.pb.view.row_event, r).tolist()
            self.offs = _dev_bytes(self.pb.view.row_offsets, 8 * (r + 1)).view(np.int64)
            self.lens = np.diff(self.offs).tolist()
            assert self.lens == [] or min(self.lens) > 0
        else:
            self.row_event, self.lens, self.host_event = None, None, int(self.pb.view.host_event)

    def model(self, windows, max_bytes=0):
        if self.copy:
            return BP.plan_copy(self.row_event, self.lens, max_bytes, needs_host_event=self.host_event)
        return BP.plan(*self.ev, self.slot, windows, self.row_event, self.lens, needs_host_event=self.host_event, **self.identity)

    def raw(self, windows, max_bytes, rcap, dev, skip=(), passes=True, pb=None):
        """One call with poison-filled buffers of rcap requests / one entry per window and a guard entry each -> (rc, info, {name: words})."""
        nwin = len(windows) if (len(windows) or not self.copy) else 1
        words = {"requests": 8 * (rcap + 1), "windows": 7 * (nwin + 1)}
        pa = np.full((len(windows), 7), FILL, dtype=np.uint64)                  # only first_event and data_end are read
        for p, (lo, hi) in enumerate(windows):
            pa[p, 0], pa[p, 1] = lo, hi
        bufs = {k: np.full(words[k], FILL, dtype=np.uint64) for k in words if k not in skip}
        owners = {k: _dev_put(a) for k, a in bufs.items()} if dev else {}
        pown = _dev_put(pa.reshape(-1)) if dev else None
        ptr = lambda k: None if k in skip else (owners[k][1] if dev else bufs[k].ctypes.data)
        pptr = None if not passes or not len(windows) else (pown[1] if dev else pa.ctypes.data)
        info = abi.BqPlanInfo()
        rc = self.d.L.etlg_bigquery_plan(self.d.h, self.b.h, self.slot, pptr, len(windows), 1 if dev and pptr else 0, (pb or self.pb).h, max_bytes,
                                         abi.F_OUTPUT_ON_DEVICE if dev else 0, ptr("requests"), rcap, ptr("windows"), C.byref(info))
        if dev:
            bufs = {k: _dev_get(owners[k][1], words[k]) for k in bufs}
        return rc, info, bufs

    def check(self, windows, max_bytes=0, rcap=None, skip=()):
        """Host and device memory against the model, field by field; returns the model."""
        m = self.model(windows, max_bytes)
        assert m["status"] == BP.OK, m
        rcap = m["info"]["n_reqs"] if rcap is None else rcap
        got = {}
        for dev in (False, True):
            rc, info, bufs = self.raw(windows, max_bytes, rcap, dev, skip)
            assert rc == abi.OK and info.status == abi.BQP_OK, (rc, info.status, int(info.event), int(info.bad_pass), info.reason)
            gi = {k: int(getattr(info, k)) for k in BP.INFO_FIELDS}
            assert gi == m["info"], (dev, gi, m["info"])
            assert (int(info.event), int(info.bad_pass), int(info.fail_pass), info.reason) == (BP.NONE, BP.NONE, BP.NONE, 0)
            self.compare(m, bufs, rcap, dev)
            got[dev] = bufs
        for k in got[False]:
            assert np.array_equal(got[False][k], got[True][k]), k              # host and device output pointers: the same bytes
        return m

    def compare(self, m, bufs, rcap, dev):
        S, P = min(rcap, len(m["requests"])), len(m["windows"])
        if "requests" in bufs:
            want = np.array([[s[f] for f in BP.REQ_FIELDS] for s in m["requests"][:S]], dtype=np.uint64).reshape(S, 8)
            got = bufs["requests"][:8 * S].reshape(S, 8)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert not len(bad), (dev, int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())
            assert (bufs["requests"][8 * S:] == FILL).all(), dev
        if "windows" in bufs:
            want = np.array([[w[f] for f in BP.WIN_FIELDS] for w in m["windows"]], dtype=np.uint64).reshape(P, 7)
            got = bufs["windows"][:7 * P].reshape(P, 7)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert not len(bad), (dev, int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())
            assert (bufs["windows"][7 * P:] == FILL).all(), dev

    def status(self, windows, want, max_bytes=0, **fields):
        """A status other than OK, on host and device memory: every field of the info, and every output word still poison."""
        m = self.model(windows, max_bytes)
        assert m["status"] == want and all(m[k] == v for k, v in fields.items()), m
        full = (m.get("event", BP.NONE), m.get("bad_pass", BP.NONE), m.get("fail_pass", BP.NONE), m.get("reason", 0))
        for dev in (False, True):
            rc, info, bufs = self.raw(windows, max_bytes, 8, dev)
            assert rc == abi.OK and info.status == want, (dev, rc, info.status, int(info.event))
            assert (int(info.event), int(info.bad_pass), int(info.fail_pass), info.reason) == full, (dev, int(info.event), int(info.bad_pass), int(info.fail_pass), info.reason, m)
            assert all(int(getattr(info, k)) == 0 for k in BP.INFO_FIELDS), dev
            assert all((a == FILL).all() for a in bufs.values()), dev

    def close(self):
        self.pb.close(); self.b.close(); self.d.close()


def _whole(c):
    return [(0, c.n)]


def _two_row_events(c):
    return [e for e in set(c.row_event) if c.row_event.count(e) == 2]


def _outline_windows(c, parts):
    sm = BC.size_model()
    total = int(c.b.cuts(sm, 1 << 62, cap=0)[1].total)
    cuts, ci = c.b.cuts(sm, max(1, total // parts))
    ol = c.b.outline(cuts=cuts)
    assert ol.info.status == abi.OL_OK and len(ol.passes) >= parts
    return ol, [(int(p[0]), int(p[1])) for p in ol.passes]


# ---------------------------------------------------------------- two-row Updates, windows

def test_two_row_updates():
    """An Update that changes the key is two rows of one event: a window that begins or ends on one gets both. first_row computed as
    end_row - members fails here: every window with such an event has more rows than members."""
    c = _Case([_round_robin(330), _round_robin(270)])
    ms = c.members
    two = _two_row_events(c)
    assert len(two) > 40 and len(c.row_event) == len(ms) + len(two) and all(c.ev[0][e] == "U" for e in two)
    m = c.check(_whole(c))                                                      # one window
    assert m["info"]["n_two_row"] == len(two) and m["info"]["n_rows"] == len(ms) + len(two) and m["info"]["n_reqs"] == 1
    m = c.check([(i, i + 1) for i in range(c.n)])                               # a window per event: a request per member, of one or two rows
    assert m["info"]["n_reqs"] == len(ms) and sorted(set(s["end_row"] - s["first_row"] for s in m["requests"])) == [1, 2]
    assert all((s["end_row"] - s["first_row"] == 2) == (s["first_event"] in two) for s in m["requests"])
    e = two[len(two) // 2]
    m = c.check([(0, e), (e, e + 1), (e + 1, c.n)])                             # a window ends in front of one, one is it, one begins behind it
    assert m["windows"][1]["end_row"] - m["windows"][1]["first_row"] == 2 and m["windows"][1]["n_members"] == 1
    m = c.check([(3, e + 1), (e + 1, e + 1), (e + 2, c.n - 1)])                 # a window ends on one: both rows are its own
    w0, w2 = m["windows"][0], m["windows"][2]
    assert c.row_event[w0["end_row"] - 1] == c.row_event[w0["end_row"] - 2] == e and w2["first_row"] == w0["end_row"]
    assert w0["n_two_row"] > 0 and w0["end_row"] - w0["first_row"] == w0["n_members"] + w0["n_two_row"]
    m = c.check([(0, 10), (10, 10), (10, 40), (40, 40), (c.n, c.n)])            # empty windows, one at the very end
    assert [w["n_reqs"] for w in m["windows"]] == [1, 0, 1, 0, 0]
    assert m["windows"][4]["first_row"] == m["windows"][4]["end_row"] == len(c.row_event)
    gap = next(i for i in range(c.n - 1) if i not in ms and i + 1 not in ms)   # (Begin and a neighbour of another slot)
    m = c.check([(0, gap), (gap, gap + 2), (gap + 2, c.n)])                     # a window without a member of the slot
    assert m["windows"][1]["n_members"] == 0 and m["windows"][1]["n_reqs"] == 0 and m["info"]["n_reqs"] == 2
    ol, wins = _outline_windows(c, 9)                                           # the outline's passes over the cuts of a small budget
    m = c.check(wins)
    got = c.b.bigquery_plan(0, ol.passes, c.pb)
    assert got.info.status == abi.BQP_OK and len(got.requests) == m["info"]["n_reqs"] and len(got.windows) == len(wins)
    assert [[int(getattr(s, f)) for f in BP.REQ_FIELDS] for s in got.requests] == [[s[f] for f in BP.REQ_FIELDS] for s in m["requests"]]
    assert [[int(getattr(w, f)) for f in BP.WIN_FIELDS] for w in got.windows] == [[w[f] for f in BP.WIN_FIELDS] for w in m["windows"]]
    for dev in (False, True):                                                   # n_passes == 0, with and without a pointer
        for passes in (True, False):
            rc, info, bufs = c.raw([], 0, 4, dev, passes=passes)
            assert rc == abi.OK and info.status == abi.BQP_OK and all(int(getattr(info, k)) == 0 for k in BP.INFO_FIELDS)
            assert all((a == FILL).all() for a in bufs.values())
    c.close()
    c1 = _Case([_round_robin(300)], slot=1)                                     # another slot of the same stream
    c1.check([(0, c1.n // 2), (c1.n // 2, c1.n)])
    c1.close()


def test_relation_and_truncate_passes():
    """A stream whose passes end at a Relation and at a Truncate: the windows are the outline's [first_event, data_end)."""
    rel = W.relation(43, "public", "t43", "d", [(1, "id", SC.INT8, -1), (0, "t", 25, -1)])
    pat = _round_robin(60) + "T" + _round_robin(45) + "L" + _round_robin(30) + "TT" + _round_robin(30)
    c = _Case([pat], extra=dict(MOVED, T=W.truncate([43], 0), L=rel))
    ol = c.b.outline()
    assert ol.info.status == abi.OL_OK and len(ol.passes) >= 4 and int(ol.info.n_trunc) >= 2 and int(ol.info.n_relations) >= 1
    m = c.check([(int(p[0]), int(p[1])) for p in ol.passes])
    assert m["info"]["n_reqs"] >= 4 and m["info"]["n_two_row"] > 0
    c.close()


# ---------------------------------------------------------------- tiles

@pytest.mark.parametrize("tile,n", [(8, 2400), (None, 2049)])
def test_tile_crossings(tile, n):
    """Tiles of 8 over 2 400 events: 300 tiles, more than one chunk of 256 tile sums in k_bqp_scan; the default tile with 2 049 events:
    a second tile of one event. Windows end on a tile's first and on its last event."""
    c = _Case([_round_robin(n // 2), _round_robin(n - 4 - n // 2)], tile=tile)   # (two transactions: four events beside the messages)
    t = tile or 2048
    assert c.n == n and (c.n + t - 1) // t > (256 if tile else 1)
    c.check(_whole(c))
    k = (c.n // t) // 2 * t if tile else t                                      # a tile's first event
    wins = [(0, t - 1), (t - 1, t), (t, k), (k, k + 1), (k + 1, k + t - 1), (k + t - 1, c.n)] if tile else [(0, t - 1), (t - 1, t), (t, t + 1), (t + 1, c.n)]
    m = c.check(wins)
    assert m["info"]["n_members"] == len(c.members)
    c.check([(i, min(i + 7, c.n)) for i in range(0, c.n, 7)])                   # windows that straddle every tile of 8
    c.close()


# ---------------------------------------------------------------- failing members

def test_each_reason_alone():
    alt = [0, 1, 0, 0]                                                          # an alternative key as wide as the primary key
    c = _Case(["iipi"], cols=KCOLS, extra=_kmsgs([1, 0, 0, 0]))                 # a partial Update under the primary key
    ms = c.members
    c.status(_whole(c), BP.FAILED, event=ms[2], reason=BP.R_PARTIAL_UPDATE, fail_pass=0)
    c.status([(0, ms[1]), (ms[1], ms[3]), (ms[3], c.n)], BP.FAILED, event=ms[2], reason=BP.R_PARTIAL_UPDATE, fail_pass=1)   # fail_pass names the window
    c.check([(0, ms[2]), (ms[2] + 1, c.n)])                                     # outside every window it does not fail the call
    c.close()
    c = _Case(["iiri"], cols=KCOLS, ident=alt, extra=_kmsgs(alt))               # a full Update without an old image
    assert c.identity == {"identity_type": "AlternativeKey", "n_ident": 1, "n_pk": 1}
    c.status(_whole(c), BP.FAILED, event=c.members[2], reason=BP.R_UPDATE_NO_OLD_IDENTITY, fail_pass=0)
    c.status([(0, 2), (2, c.members[2]), (c.members[2], c.n)], BP.FAILED, event=c.members[2], reason=BP.R_UPDATE_NO_OLD_IDENTITY, fail_pass=2)
    c.close()
    c = _Case(["iiri"], cols=KCOLS, extra=_kmsgs([1, 0, 0, 0]))                 # ... passes under the primary key
    assert c.check(_whole(c))["info"]["n_rows"] == 4
    c.close()
    for k in "ud":
        c = _Case(["ii" + k + "i"], cols=KCOLS, ident=alt, extra=_kmsgs(alt))   # a key image of another identity
        c.status(_whole(c), BP.FAILED, event=c.members[2], reason=BP.R_KEY_IDENTITY, fail_pass=0)
        c.check([(0, c.members[2])])
        c.close()
        wide = [0, 1, 1, 0]                                                     # ... of another width under the same identity type: the width alone
        c = _Case(["ii" + k + "i"], cols=KCOLS, ident=wide, extra=_kmsgs(wide))
        assert c.identity == {"identity_type": "AlternativeKey", "n_ident": 2, "n_pk": 1}
        c.status(_whole(c), BP.FAILED, event=c.members[2], reason=BP.R_KEY_WIDTH, fail_pass=0)
        c.close()
        c = _Case(["ii" + k + "oi"], cols=KCOLS, extra=_kmsgs([1, 0, 0, 0]))    # the primary key: no refusal; a full old image neither
        assert c.check(_whole(c))["info"]["n_members"] == 5
        c.close()
    c = _Case(["iioi"], cols=KCOLS, ident=alt, extra=_kmsgs(alt))               # a Delete with the full old row passes under any identity
    assert c.check(_whole(c))["info"]["n_rows"] == 4
    c.close()


def test_the_earlier_reason_wins_and_the_lowest_event():
    alt, narrow = [0, 1, 0, 0], [0, 0, 1, 0]
    c = _Case(["iiqi"], cols=KCOLS, ident=alt, extra=_kmsgs(alt))               # partial and without an old image: PARTIAL_UPDATE
    c.status(_whole(c), BP.FAILED, event=c.members[2], reason=BP.R_PARTIAL_UPDATE, fail_pass=0)
    c.close()
    c = _Case(["iipi"], cols=KCOLS, ident=alt, extra=_kmsgs(alt))               # partial with a key image of another identity: PARTIAL_UPDATE
    c.status(_whole(c), BP.FAILED, event=c.members[2], reason=BP.R_PARTIAL_UPDATE, fail_pass=0)
    c.close()
    c = _Case(["iipi"], cols=PK2COLS, ident=narrow, extra=_kmsgs(narrow))       # ... and of another width: PARTIAL_UPDATE
    c.status(_whole(c), BP.FAILED, event=c.members[2], reason=BP.R_PARTIAL_UPDATE, fail_pass=0)
    c.close()
    for k in "ud":                                                              # an alternative-index identity narrower than the primary key meets both: KEY_WIDTH
        c = _Case(["ii" + k + "i"], cols=PK2COLS, ident=narrow, extra=_kmsgs(narrow))
        assert c.identity == {"identity_type": "AlternativeKey", "n_ident": 1, "n_pk": 2}
        c.status(_whole(c), BP.FAILED, event=c.members[2], reason=BP.R_KEY_WIDTH, fail_pass=0)
        c.close()
    c = _Case(["iipdi"], cols=KCOLS, ident=alt, extra=_kmsgs(alt))              # two failing events of different reasons: the lowest event
    ms = c.members
    c.status(_whole(c), BP.FAILED, event=ms[2], reason=BP.R_PARTIAL_UPDATE, fail_pass=0)
    c.status([(0, ms[2]), (ms[3], c.n)], BP.FAILED, event=ms[3], reason=BP.R_KEY_IDENTITY, fail_pass=1)
    c.close()
    c = _Case(["iidrpi"], cols=KCOLS, ident=alt, extra=_kmsgs(alt))
    ms = c.members
    c.status(_whole(c), BP.FAILED, event=ms[2], reason=BP.R_KEY_IDENTITY, fail_pass=0)
    c.status([(0, 1), (1, ms[2]), (ms[2] + 1, c.n)], BP.FAILED, event=ms[3], reason=BP.R_UPDATE_NO_OLD_IDENTITY, fail_pass=2)
    c.status([(0, ms[2]), (ms[4], c.n)], BP.FAILED, event=ms[4], reason=BP.R_PARTIAL_UPDATE, fail_pass=1)
    c.close()
    c1 = _Case(["IIPIxI"], slot=1)                                              # a failing event of another slot does not count
    c1.check(_whole(c1))
    c1.close()


# ---------------------------------------------------------------- NEEDS_HOST, BAD_PASSES

def test_needs_host_for_a_key_the_device_does_not_compare():
    """A numeric primary key: Cell equality is not equality of the arena's words, so a full Update that carries a key image has no
    row in the object (etlg_batch_protobuf counts it in n_host_rows)."""
    cols = [("id", SC.NUMERIC, False, 1), ("s", 25, True, 0)]
    msgs = [W.insert(42, ["1.0", "a"]), W.insert(42, ["2", "b"]), W.update(42, ["1.00", "c"], key=["1.0", N]), W.insert(42, ["3", N]),
            W.update(42, ["2", "d"], key=["2", N]), W.update(42, ["3", "e"])]
    s = SC.txn(msgs)
    c = _Case(stream=(np.frombuffer(s.bytes(), dtype=np.uint8), s.offsets), cols=cols)
    ms = c.members
    assert c.pb.status == abi.RB_OK and len(c.row_event) == 4 and len(ms) == 6 and int(c.pb.view.n_host_rows) == 2
    c.status(_whole(c), BP.NEEDS_HOST, event=ms[2], fail_pass=0)
    c.status([(0, ms[1]), (ms[1], ms[3]), (ms[3], c.n)], BP.NEEDS_HOST, event=ms[2], fail_pass=1)
    c.status([(0, ms[2]), (ms[3], c.n)], BP.NEEDS_HOST, event=ms[4], fail_pass=1)
    m = c.check([(0, ms[2]), (ms[3], ms[4]), (ms[5], c.n)])                     # the windows without them: a plan
    assert m["info"]["n_reqs"] == 3 and m["info"]["n_rows"] == 4
    c.close()
    msgs = [W.insert(42, ["1.0", "a"]), W.update(42, ["1", W.TOAST], key=["1.0", N]), W.update(42, ["1.00", "c"], key=["1.0", N])]
    s = SC.txn(msgs)                                                            # a failing event in front of it wins ...
    c = _Case(stream=(np.frombuffer(s.bytes(), dtype=np.uint8), s.offsets), cols=cols)
    c.status(_whole(c), BP.FAILED, event=c.members[1], reason=BP.R_PARTIAL_UPDATE, fail_pass=0)
    c.close()
    msgs = [W.insert(42, ["1.0", "a"]), W.update(42, ["1.00", "c"], key=["1.0", N]), W.update(42, ["1", W.TOAST], key=["1.0", N])]
    s = SC.txn(msgs)                                                            # ... and so does one behind it: FAILED is the earlier status
    c = _Case(stream=(np.frombuffer(s.bytes(), dtype=np.uint8), s.offsets), cols=cols)
    c.status(_whole(c), BP.FAILED, event=c.members[2], reason=BP.R_PARTIAL_UPDATE, fail_pass=0)
    c.status([(0, c.members[2])], BP.NEEDS_HOST, event=c.members[1], fail_pass=0)
    c.close()


def test_needs_host_object():
    """A protobuf object that came back NEEDS_HOST for an array literal the device does not take apart: its host_event is reported,
    behind the statuses that come first."""
    cols = [("id", SC.INT8, False, 1), ("a", 1007, True, 0)]
    msgs = [W.insert(42, ["1", "{1,2}"]), W.insert(42, ["2", "{1,{2}}"]), W.insert(42, ["3", "{}"])]
    s = SC.txn(msgs)
    c = _Case(stream=(np.frombuffer(s.bytes(), dtype=np.uint8), s.offsets), cols=cols)
    assert c.pb.status == abi.RB_NEEDS_HOST and c.host_event == c.members[1]
    c.status(_whole(c), BP.NEEDS_HOST, event=c.members[1], fail_pass=BP.NONE)
    c.status([(0, c.members[1])], BP.NEEDS_HOST, event=c.members[1])            # the object has no rows, whatever the windows hold
    c.status([(2, 1)], BP.BAD_PASSES, bad_pass=0)                               # a status in front of it
    rc, info, bufs = c.raw([], 0, 4, False)
    assert rc == abi.OK and info.status == abi.BQP_NEEDS_HOST and int(info.event) == c.members[1]
    c.close()
    msgs = [W.insert(42, ["1", "{1,2}"]), W.update(42, ["2", W.TOAST], key=["2", N]), W.insert(42, ["2", "{1,{2}}"])]   # FAILED comes first
    s = SC.txn(msgs)
    c = _Case(stream=(np.frombuffer(s.bytes(), dtype=np.uint8), s.offsets), cols=cols)
    assert c.pb.status == abi.RB_NEEDS_HOST
    c.status(_whole(c), BP.FAILED, event=c.members[1], reason=BP.R_PARTIAL_UPDATE, fail_pass=0)
    c.close()


def test_bad_passes():
    c = _Case([_round_robin(60)])
    c.status([(0, 10), (12, 11), (20, 30)], BP.BAD_PASSES, bad_pass=1)          # first_event > data_end
    c.status([(0, 10), (20, c.n + 1)], BP.BAD_PASSES, bad_pass=1)               # beyond n_events
    c.status([(0, 10), (9, 30), (5, 40)], BP.BAD_PASSES, bad_pass=1)            # starts below its predecessor's end; the lowest index
    c.status([(c.n + 1, c.n + 1)], BP.BAD_PASSES, bad_pass=0)
    c.status([(i, i + 1) for i in range(40)] + [(39, 41)], BP.BAD_PASSES, bad_pass=40)
    c.close()
    c = _Case(["IIPI"])                                                         # BAD_PASSES comes before FAILED
    c.status([(2, 1)], BP.BAD_PASSES, bad_pass=0)
    c.close()


# ---------------------------------------------------------------- caps, NULL outputs

def test_caps_and_null_outputs():
    c = _Case([_round_robin(300)])
    wins = [(0, 40), (40, 40), (41, 100), (100, 101), (101, 200), (200, c.n)]
    nr = c.model(wins)["info"]["n_reqs"]
    assert nr >= 4
    for rcap in (0, 1, nr - 1, nr, nr + 5):
        c.check(wins, rcap=rcap)                                                # the full count comes back, nothing is written past the cap
    c.check(wins, skip=("requests",))                                           # any output may be NULL
    c.check(wins, skip=("windows",))
    c.check(wins, skip=("requests", "windows"))
    c.check(wins, max_bytes=(1 << 64) - 1)                                       # max_batch_bytes is ignored on this path
    c.close()


# ---------------------------------------------------------------- table-copy batches

COPY_COLS = [("id", SC.INT8, False, 1), ("s", 25, True, 0)]


def _copy_rows(n, first=None, text="t"):
    return [b"%d\t%s\n" % (i, (first if first is not None and i == 0 else text).encode()) for i in range(n)]


def _budget_for(R, est, target):
    """A max_batch_bytes with ceil(R / (budget // est)) == target (target <= R), or a first row longer than the budget for R + 1."""
    per = next(p for p in range(R, 0, -1) if -(-R // p) == target)
    return per * est + est - 1


def test_copy_split_vectors():
    """The split_table_rows vectors (tests/golden/bigquery_split_kats.py) through the call: rows of one length, max_batch_bytes chosen so
    that calculate_target_batches_for_table_copy gives the vector's target."""
    hit = set()
    for R in (0, 1, 2, 5, 10):
        c = _Case(copy=(COPY_COLS, _copy_rows(R, text="abc" if R < 11 else "t")), tile=64)
        assert c.n == R and c.row_event == list(range(R)) and len(set(c.lens)) <= 1
        est = c.lens[0] if R else 7
        targets = sorted(set(t for t in (1, 2, 3, 4, R) if 1 <= t <= R and any(-(-R // p) == t for p in range(1, R + 1)))) if R else [0]
        for t in targets:
            b = _budget_for(R, est, t) if R else 100
            m = c.check([], max_bytes=b)
            assert m["info"]["target_batches"] == t and m["info"]["est_row_bytes"] == (est if R else 0)
            assert [s["end_row"] - s["first_row"] for s in m["requests"]] == BP.split_table_rows(R, t)
            for name, lines, total, target, want in KATS.SPLIT_TABLE_ROWS:     # the reference's vectors of this size and target
                if (total, target) == (R, t):
                    assert [s["n_members"] for s in m["requests"]] == want, (name, lines)
                    hit.add(name)
        if R:                                                                   # a first row longer than max_batch_bytes: rows_per_batch 0, target 1 ("R + 1" cannot be
            m = c.check([], max_bytes=est - 1)                                  # reached: target <= R whenever rows_per_batch > 0), one request
            assert m["info"]["target_batches"] == 1 and m["info"]["n_reqs"] == 1
            m = c.check([], max_bytes=est)                                      # one row per batch: target R, R <= target -> one request of all rows
            assert m["info"]["target_batches"] == R and m["info"]["n_reqs"] == 1
            c.check([], max_bytes=1 << 63)
        c.close()
    # (the vectors with a target of 0 or above the row count are the model test's: calculate_target_batches never gives one for such rows)
    assert hit == {"split_table_rows_single_concurrent_stream", "split_table_rows_uneven_distribution", "split_table_rows_many_streams"}


def test_copy_estimate_is_row_zero_and_caps():
    rows = _copy_rows(1000, first="x")                                          # a first row much shorter than the others
    rows = [rows[0]] + [b"%d\t%s\n" % (i, b"y" * 40) for i in range(1, 1000)]
    c = _Case(copy=(COPY_COLS, rows), tile=64)
    est = c.lens[0]
    assert c.n == 1000 and max(c.lens) > 3 * est
    b = _budget_for(1000, est, 7)                                               # 1 000 rows, target 7: 143 x 6 + 142
    m = c.check([], max_bytes=b)
    assert m["info"]["target_batches"] == 7 and [s["n_members"] for s in m["requests"]] == [143] * 6 + [142]
    assert m["info"]["est_row_bytes"] == est and m["requests"][0]["byte_end"] - m["requests"][0]["byte_first"] > b   # the estimate is row 0's alone
    m = c.check([], max_bytes=_budget_for(1000, est, 334))                      # 334 -> opt 3 -> 334 requests: more than a workgroup of them
    assert m["info"]["n_reqs"] == 334
    for rcap in (0, 1, 6, 7, 12):
        c.check([], max_bytes=b, rcap=rcap)
    c.check([], max_bytes=b, skip=("requests",))
    c.check([], max_bytes=b, skip=("windows",))
    c.check([], max_bytes=b, skip=("requests", "windows"))
    got = c.b.bigquery_plan(0, None, c.pb, max_batch_bytes=b)
    assert got.info.status == abi.BQP_OK and len(got.requests) == 7 and len(got.windows) == 1 and int(got.windows[0].n_reqs) == 7
    info = abi.BqPlanInfo()
    call = lambda mb, p=None, n=0: c.d.L.etlg_bigquery_plan(c.d.h, c.b.h, 0, p, n, 0, c.pb.h, mb, 0, None, 0, None, C.byref(info))
    assert call(0) == abi.InvalidArgument and call((1 << 63) + 1) == abi.InvalidArgument   # max_batch_bytes out of range
    pa = np.array([[0, c.n, 0, 0, 0, 0, 0]], dtype=np.uint64)
    assert call(b, pa.ctypes.data, 1) == abi.InvalidArgument                    # a table-copy batch takes no passes
    assert call(b) == abi.OK and int(info.n_reqs) == 7
    c.close()


# ---------------------------------------------------------------- wrong objects

def test_wrong_objects_and_invalid_arguments():
    c = _Case(["IUD", "IK"])
    info = abi.BqPlanInfo()
    pa = np.array([[0, c.n, 0, 0, 0, 0, 0]], dtype=np.uint64)

    def call(batch, slot=0, passes=pa.ctypes.data, n=1, pb=c.pb, max_bytes=0):
        return c.d.L.etlg_bigquery_plan(c.d.h, batch.h, slot, passes, n, 0, pb.h if pb is not None else None, max_bytes, 0, None, 0, None, C.byref(info))

    assert call(c.b) == abi.OK and (int(info.n_members), int(info.n_rows), int(info.n_two_row), int(info.n_reqs)) == (5, 6, 1, 1)
    assert call(c.b, slot=7) == abi.InvalidArgument and call(c.b, slot=-1) == abi.InvalidArgument          # an unknown slot
    assert call(c.b, passes=None, n=1) == abi.InvalidArgument                                              # n_passes without passes
    assert call(c.b, pb=None) == abi.InvalidArgument                                                       # the object is required
    rb = c.b.rowbinary(0, [0, 1, 1, 0, 0], abi.CH_MERGE_TREE, on_device=True)
    nd = c.b.ndjson(0, NAMES[0], on_device=True)
    dl = c.b.duckdb(0, NAMES[0], what=abi.DL_TUPLES, on_device=True)
    other = c.b.protobuf(1, on_device=True)
    host = c.b.protobuf(0, on_device=False)
    assert call(c.b, pb=rb) == abi.InvalidArgument                                                         # a RowBinary object
    assert call(c.b, pb=nd) == abi.InvalidArgument                                                         # an NDJSON object
    assert call(c.b, pb=dl) == abi.InvalidArgument                                                         # a DuckLake object
    assert call(c.b, pb=other) == abi.InvalidArgument and call(c.b, slot=1, pb=other) == abi.OK            # another slot's
    assert call(c.b, pb=host) == abi.InvalidArgument                                                       # host-resident
    buf, offs = _stream(["IUD", "IK"], MOVED)
    b2 = c.d.decode(buf, offs, flags=abi.F_OUTPUT_ON_DEVICE)
    assert call(b2) == abi.InvalidArgument                                                                 # another batch's object
    b2.close()
    bh = c.d.decode(buf, offs)                                                                             # a batch that is not device-resident
    assert call(bh) == abi.InvalidArgument
    bh.close()
    ba = c.d.decode(buf, offs, flags=abi.F_OUTPUT_ON_DEVICE | abi.F_ASYNC)                                 # an ASYNC batch is synced first
    pba = ba.protobuf(0, on_device=True)
    assert call(ba, pb=pba) == abi.OK and int(info.n_members) == 5
    pba.close(); ba.close()
    rb.close(); nd.close(); dl.close(); other.close(); host.close()
    c.close()
