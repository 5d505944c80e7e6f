"""etlg_snowflake_plan (etl_amd/csrc/finish.hip: k_sfp_*) through the C ABI against tests/snowflake_plan.py, the restatement of the
reference's encode_insert / encode_update / encode_delete and RowBatchBuilder::push_row as one sequential loop. Every case compares
every field the call writes with the model, exactly: the info, the segments and the windows. Every output buffer is one entry longer
than its cap and filled with a poison byte first: what lies at or beyond a count or a cap, the entry behind, and everything when the
status is not OK must still hold it. Each case runs with host passes and host outputs and again with device passes and device
outputs; the two give the same bytes. The model's row lengths are those of the device-resident etlg_batch_ndjson object, whose bytes
tests/test_gpu_ndjson.py checks.
The kernels' constants: waves of 64, workgroups of 256, the tile (2 048 events, or ETLG_SFP_TILE in a context of its own), the chunks
of 256 tile sums k_sfp_scan walks and the jump levels, one per bit of the largest segment count a window can have. Three tables share
the streams round robin, so the slot's rows lie three events apart."""
import ctypes as C
import os

import numpy as np
import pytest

from etl_amd import abi
from tests import batch_cuts as BC
from tests import pgwire as W
from tests import scenarios as SC
from tests import snowflake_plan as SP
from tests.test_gpu_ducklake_plan import COLS3, FILL, NAMES, OTHER, _dev_bytes, _dev_get, _dev_put, _msg, _prime3

pytestmark = pytest.mark.gpu
EMU = os.environ.get("ETLG_SIMT_RUN") == "1"
MIX = "IIUDIRIID"                                                            # no partial Update: the sink refuses those
BIG = 2 * 1024 * 1024


def _message(k, i, big):
    if k == "B":                                                             # an Insert whose text cell makes a row of more than `big` bytes
        return W.insert(42, [str(i), "1", "x" * big])
    if k == "b":                                                             # the same on table 43
        return W.insert(43, [str(i), "y" * big])
    return _msg(k, i)


def _stream(groups, big=0, extra=None):
    """groups: one pattern string per transaction -> (buf, offsets); the transactions' final LSNs ascend. extra: {letter: message}."""
    s, i = W.Stream(lsn=0x1000), 0
    for pat in groups:
        final = s.lsn + 8 * (len(pat) + 2)
        s.add(W.begin(final, ts=1234, xid=77))
        for k in pat:
            s.add(extra[k] if extra and k in extra else _message(k, i, big))
            i += 1
        s.add(W.commit(final, final + 8, ts=5678, flags=0), lsn=final)
    return np.frombuffer(s.bytes(), dtype=np.uint8), s.offsets


def _round_robin(n, mix=MIX):
    return "".join((mix[(i // 3) % len(mix)], "x", "y")[i % 3] for i in range(n))


class _Case:
    def __init__(self, groups=None, tile=None, slot=0, stream=None, prime=None, names=None, big=0, copy=None, extra=None):
        from etl_amd.decoder import Decoder
        from oracle import oracle
        before = os.environ.get("ETLG_SFP_TILE")
        if tile:
            os.environ["ETLG_SFP_TILE"] = str(tile)                            # read when the context is created
        try:
            self.d = Decoder(0)
        finally:
            os.environ.pop("ETLG_SFP_TILE", None)
            if before is not None:
                os.environ["ETLG_SFP_TILE"] = before
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
            names = [c[0] for c in cols]
        else:
            buf, offs = stream or _stream(groups, big, extra)
            prime = prime or _prime3()
            prime(self.d)
            prime(o)
            self.b = self.d.decode(buf, offs, flags=abi.F_OUTPUT_ON_DEVICE)
            rb = o.decode(buf, offs)
        assert self.b.rc == 0, self.b.error
        assert rb.err_code == 0, rb.err_desc
        self.hb = rb.host_batch()
        self.ev = SP.of_host_batch(self.hb)
        self.n, self.slot, self.names = len(self.ev[0]), slot, names or NAMES[slot]
        self.members = [i for i in range(self.n) if self.ev[0][i] in "IUD" and int(self.ev[2][i]) == slot]
        self.keys = [(int(self.ev[3][i]), int(self.ev[4][i])) for i in self.members]
        self.nd = self.b.ndjson(slot, self.names, on_device=True)
        self.host_event = None
        if self.nd.status == abi.RB_OK:
            r = int(self.nd.n_rows)
            self.row_event = _dev_get(self.nd.view.row_event, r).tolist()
            self.offs = _dev_bytes(self.nd.view.row_offsets, 8 * (r + 1)).view(np.int64)
            self.lens = np.diff(self.offs).tolist()
            assert self.lens == [] or min(self.lens) > 0
        else:
            self.row_event, self.lens, self.host_event = None, None, int(self.nd.view.host_event)

    def model(self, windows, committed=None, flush=SP.MAX_UNFLUSHED_BYTES, max_row=SP.MAX_ROW_BYTES):
        return SP.plan(*self.ev, self.slot, windows, self.row_event, self.lens, committed=committed, flush_bytes=flush, max_row_bytes=max_row,
                       zero_keys=self.copy, needs_host_event=self.host_event)

    def raw(self, windows, committed, flush, max_row, scap, dev, skip=(), passes=True, nd=None):
        """One call with poison-filled buffers of scap segments / one entry per window and a guard entry each -> (rc, info, {name: words})."""
        nwin = len(windows) if (len(windows) or not self.copy) else 1
        words = {"segments": 13 * (scap + 1), "windows": 7 * (nwin + 1)}
        pa = np.full((len(windows), 7), FILL, dtype=np.uint64)                  # only first_event and data_end are read
        for p, (lo, hi) in enumerate(windows):
            pa[p, 0], pa[p, 1] = lo, hi
        bufs = {k: np.full(words[k], FILL, dtype=np.uint64) for k in words if k not in skip}
        owners = {k: _dev_put(a) for k, a in bufs.items()} if dev else {}
        pown = _dev_put(pa.reshape(-1)) if dev else None
        ptr = lambda k: None if k in skip else (owners[k][1] if dev else bufs[k].ctypes.data)
        pptr = None if not passes or not len(windows) else (pown[1] if dev else pa.ctypes.data)
        cm = (0, 0, 0) if committed is None else (1, int(committed[0]), int(committed[1]))
        info = abi.SfPlanInfo()
        rc = self.d.L.etlg_snowflake_plan(self.d.h, self.b.h, self.slot, pptr, len(windows), 1 if dev and pptr else 0, *cm, (nd or self.nd).h, flush, max_row,
                                          abi.F_OUTPUT_ON_DEVICE if dev else 0, ptr("segments"), scap, ptr("windows"), C.byref(info))
        if dev:
            bufs = {k: _dev_get(owners[k][1], words[k]) for k in bufs}
        return rc, info, bufs

    def check(self, windows, committed=None, flush=SP.MAX_UNFLUSHED_BYTES, max_row=SP.MAX_ROW_BYTES, scap=None, skip=(), model_windows=None):
        """Host and device memory against the model, field by field; returns the model."""
        m = self.model(model_windows or windows, committed, flush, max_row)
        assert m["status"] == SP.OK, m
        scap = m["info"]["n_segs"] if scap is None else scap
        got = {}
        for dev in (False, True):
            rc, info, bufs = self.raw(windows, committed, flush, max_row, scap, dev, skip)
            assert rc == abi.OK and info.status == abi.SFP_OK, (rc, info.status, int(info.event), int(info.bad_pass), info.reason)
            gi = {k: int(getattr(info, k)) for k in SP.INFO_FIELDS}
            assert gi == m["info"], (dev, gi, m["info"])
            assert (int(info.event), int(info.bad_pass), int(info.row_bytes), info.reason) == (SP.NONE, SP.NONE, 0, 0)
            self.compare(m, bufs, scap, dev)
            got[dev] = bufs
        for k in got[False]:
            assert np.array_equal(got[False][k], got[True][k]), k              # host and device output pointers: the same bytes
        return m

    def compare(self, m, bufs, scap, dev):
        S, P = min(scap, len(m["segments"])), len(m["windows"])
        if "segments" in bufs:
            want = np.array([[s[f] for f in SP.SEG_FIELDS] for s in m["segments"][:S]], dtype=np.uint64).reshape(S, 13)
            got = bufs["segments"][:13 * S].reshape(S, 13)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert not len(bad), (dev, int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())
            assert (bufs["segments"][13 * S:] == FILL).all(), dev
        if "windows" in bufs:
            want = np.array([[w[f] for f in SP.WIN_FIELDS] for w in m["windows"]], dtype=np.uint64).reshape(P, 7)
            got = bufs["windows"][:7 * P].reshape(P, 7)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert not len(bad), (dev, int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())
            assert (bufs["windows"][7 * P:] == FILL).all(), dev

    def status(self, windows, want, committed=None, flush=SP.MAX_UNFLUSHED_BYTES, max_row=SP.MAX_ROW_BYTES, **fields):
        """A status other than OK, on host and device memory: the info's fields, and every output word still poison."""
        m = self.model(windows, committed, flush, max_row)
        assert m["status"] == want and all(m[k] == v for k, v in fields.items()), m
        for dev in (False, True):
            rc, info, bufs = self.raw(windows, committed, flush, max_row, 8, dev)
            assert rc == abi.OK and info.status == want, (dev, rc, info.status, int(info.event))
            assert all(int(getattr(info, k)) == v for k, v in m.items() if k != "status"), (dev, int(info.event), int(info.bad_pass), info.reason, int(info.row_bytes), m)
            assert all(int(getattr(info, k)) == 0 for k in SP.INFO_FIELDS), dev
            assert all((a == FILL).all() for a in bufs.values()), dev

    def close(self):
        self.nd.close(); self.b.close(); self.d.close()


def _whole(c):
    return [(0, c.n)]


def _seg_rows(m):
    return [s["end_row"] - s["first_row"] for s in m["segments"]]


# ---------------------------------------------------------------- tiles, windows

@pytest.mark.parametrize("tile", [8, 64, 512, 2048])
def test_tiles(tile):
    n = 6000
    c = _Case([_round_robin(n // 2), _round_robin(n - n // 2)], tile=tile)
    assert c.n > 2 * 2048 and len(c.members) == n // 3 and len(c.row_event) == len(c.members)
    f50 = 50 * int(np.mean(c.lens))                                          # segments of about 50 rows: 150 events, straddling tiles of 8 and 64
    m = c.check(_whole(c), flush=f50)
    assert 30 < np.mean(_seg_rows(m)) < 70 and len(m["segments"]) > 30
    mid = c.members[len(c.members) // 2] + 1                                    # windows that start in the middle of a tile
    t = min(tile, c.n // 4)
    wins = [(3, t + 5), (t + 5, t + 5), (t + 7, mid), (mid + 1, c.n - 2)]
    m = c.check(wins, flush=f50)
    assert [w["n_segs"] for w in m["windows"]][1] == 0 and m["windows"][3]["n_segs"] > 5
    c.check(wins, committed=c.keys[40], flush=f50)                              # the first window's prefix is dropped
    c.check(wins, flush=1)
    c.close()
    c1 = _Case([_round_robin(n)], tile=tile, slot=1)                            # another slot of the same stream
    c1.check([(0, c1.n // 2), (c1.n // 2, c1.n)], flush=700)
    c1.close()


def test_window_shapes():
    c = _Case([_round_robin(300), _round_robin(240)])
    ms, ln = c.members, int(np.mean(c.lens))
    c.check(_whole(c), flush=4 * ln)                                            # one window
    m = c.check([(i, i + 1) for i in range(c.n)], flush=4 * ln)                 # a window per event: every row a segment of its own, never flushed
    assert m["info"]["n_segs"] == len(ms) and all(s["flush_before"] == 0 for s in m["segments"])
    m = c.check([(0, 10), (10, 10), (10, 40), (40, 40), (c.n, c.n)], flush=2 * ln)   # empty windows, one at the very end
    assert [w["n_segs"] > 0 for w in m["windows"]] == [True, False, True, False, False]
    assert m["windows"][4]["first_row"] == m["windows"][4]["end_row"] == len(c.row_event)
    gap = next(i for i in range(c.n - 1) if i not in ms and i + 1 not in ms)   # (Begin and a neighbour of another slot)
    c.check([(0, gap), (gap, gap + 2), (gap + 2, c.n)], flush=3 * ln)           # a window without a member of the slot
    # the outline's passes over the cuts of a small budget, handed over as they are
    sm = BC.size_model()
    total = int(c.b.cuts(sm, 1 << 62, cap=0)[1].total)
    cuts, ci = c.b.cuts(sm, max(1, total // 9))
    ol = c.b.outline(cuts=cuts)
    assert ol.info.status == abi.OL_OK and len(ol.passes) >= 9
    wins = [(int(p[0]), int(p[1])) for p in ol.passes]
    m = c.check(wins, flush=5 * ln)
    got = c.b.snowflake_plan(0, ol.passes, c.nd, flush_bytes=5 * ln)
    assert got.info.status == abi.SFP_OK and len(got.segments) == m["info"]["n_segs"] and len(got.windows) == len(wins)
    assert [[int(getattr(s, f)) for f in SP.SEG_FIELDS] for s in got.segments] == [[s[f] for f in SP.SEG_FIELDS] for s in m["segments"]]
    assert [[int(getattr(w, f)) for f in SP.WIN_FIELDS] for w in got.windows] == [[w[f] for f in SP.WIN_FIELDS] for w in m["windows"]]
    for dev in (False, True):                                                   # n_passes == 0, with and without a pointer
        for passes in (True, False):
            rc, info, bufs = c.raw([], None, 100, 1000, 4, dev, passes=passes)
            assert rc == abi.OK and info.status == abi.SFP_OK and all(int(getattr(info, k)) == 0 for k in SP.INFO_FIELDS)
            assert all((a == FILL).all() for a in bufs.values())
    c.close()


def test_relation_and_truncate_passes():
    """A stream whose passes end at a Relation and at a Truncate: the windows are the outline's [first_event, data_end)."""
    rel = W.relation(43, "public", "t43", "d", [(1, "id", SC.INT8, -1), (0, "t", 25, -1)])
    pat = _round_robin(60) + "T" + _round_robin(45) + "L" + _round_robin(30) + "TT" + _round_robin(30)
    c = _Case([pat], extra={"T": W.truncate([43], 0), "L": rel})
    ol = c.b.outline()
    assert ol.info.status == abi.OL_OK and len(ol.passes) >= 4 and int(ol.info.n_trunc) >= 2 and int(ol.info.n_relations) >= 1
    wins = [(int(p[0]), int(p[1])) for p in ol.passes]
    m = c.check(wins, flush=3 * int(np.mean(c.lens)))
    assert sum(1 for w in m["windows"] if w["n_segs"]) >= 4
    c.close()


# ---------------------------------------------------------------- flush_bytes

def test_flush_values():
    c = _Case([_round_robin(450), _round_robin(300)])
    ms = c.members
    m = c.check(_whole(c), flush=1)                                             # every row its own segment
    assert _seg_rows(m) == [1] * len(ms) and all(s["flush_before"] for s in m["segments"])
    k = len(ms) // 2                                                            # a row inside a window, and the same row as a window's first
    ln = c.lens[k]
    wins = [(0, ms[k]), (ms[k], c.n)]
    for f in (ln, ln - 1, ln + 1):                                              # the >= boundary met on a window's first row and inside a window
        m1, m2 = c.check(_whole(c), flush=f), c.check(wins, flush=f)
        first = m2["segments"][m2["windows"][1]["seg_first"]]
        assert first["first_row"] == k and first["flush_before"] == (1 if ln >= f else 0)
    m = c.check(_whole(c), flush=50 * int(np.mean(c.lens)))                     # about 50 rows per segment
    assert 30 < np.mean(_seg_rows(m)) < 70
    c.close()


def test_the_real_flush_threshold():
    n = 9000                                                                    # 3 000 rows of the slot
    c = _Case([_round_robin(n)])
    assert len(c.row_event) == 3000 and sum(c.lens) > 2 * SP.MAX_UNFLUSHED_BYTES
    m = c.check(_whole(c))                                                      # 131 072 and 2 MiB
    assert len(m["segments"]) >= 3 and all(s["byte_end"] - s["byte_first"] < SP.MAX_UNFLUSHED_BYTES for s in m["segments"])
    c.check([(0, c.n // 3), (c.n // 3, c.n)])
    c.close()


# ---------------------------------------------------------------- the committed offset

def test_committed_keys():
    c = _Case([_round_robin(60), _round_robin(75), _round_robin(45)])
    keys, f = c.keys, 3 * int(np.mean(c.lens))
    assert len({k[0] for k in keys}) == 3
    wins = [(0, c.n // 2), (c.n // 2, c.n)]
    for w in (_whole(c), wins):
        assert c.check(w, committed=None, flush=f)["info"]["n_dropped"] == 0
        assert c.check(w, committed=(keys[0][0] - 1, 1 << 40), flush=f)["info"]["n_dropped"] == 0          # below every key
        assert c.check(w, committed=keys[7], flush=f)["info"]["n_dropped"] == 8                            # an event's key: it is dropped
        lsn, o = keys[25]
        assert keys[26] == (lsn, o + 3)
        assert c.check(w, committed=(lsn, o + 1), flush=f)["info"]["n_dropped"] == 26                      # inside a transaction: the ordinal decides
        assert c.check(w, committed=(keys[19][0], 1 << 50), flush=f)["info"]["n_retained"] == sum(1 for k in keys if k[0] > keys[19][0])
        m = c.check(w, committed=keys[-1], flush=f)                                                        # above every key: no segment
        assert m["info"]["n_segs"] == 0 and m["info"]["n_retained"] == 0 and m["info"]["n_bytes"] == 0
        c.check(w, committed=(keys[-1][0] + 1, 0), flush=f)
    c.close()


def test_not_prefix():
    """Keys that do not ascend: a second transaction with a lower final LSN. A dropped member behind a retained one of its window."""
    s = W.Stream(lsn=0x1000)
    for final, pat in ((0x9000, "III"), (0x3000, "II")):
        s.add(W.begin(final, ts=1, xid=7))
        for i, k in enumerate(pat):
            s.add(_msg(k, i + final))
        s.add(W.commit(final, final + 8, ts=2, flags=0), lsn=final)
    c = _Case(stream=(np.frombuffer(s.bytes(), dtype=np.uint8), s.offsets))
    ms = c.members
    c.status(_whole(c), SP.NOT_PREFIX, committed=(0x3000, 5), event=ms[3])
    c.check([(0, ms[3]), (ms[3], c.n)], committed=(0x3000, 5), flush=50)        # in a window of its own the dropped run is a prefix
    c.close()


# ---------------------------------------------------------------- failing members

def test_max_row_bytes():
    c = _Case([_round_robin(45) + "B" + _round_robin(44)], big=300)             # one row longer than every other
    top = max(c.lens)
    at = c.members[c.lens.index(top)]
    assert c.lens.count(top) == 1
    c.check(_whole(c), max_row=top, flush=400)                                  # equal to the longest row: it passes
    c.status(_whole(c), SP.FAILED, max_row=top - 1, flush=400, event=at, reason=SP.R_ROW_TOO_LARGE, row_bytes=top)
    c.check([(0, at), (at + 1, c.n)], max_row=top - 1, flush=400)               # outside every window it does not fail
    c.check(_whole(c), max_row=top - 1, flush=400, committed=c.keys[c.members.index(at)])   # ... nor when the filter drops it
    c.close()


def test_a_row_of_more_than_two_mebibytes():
    c = _Case(["IIxBIxI"], big=BIG)
    at = c.members[2]
    assert max(c.lens) > SP.MAX_ROW_BYTES and c.lens[2] == max(c.lens)
    c.status(_whole(c), SP.FAILED, event=at, reason=SP.R_ROW_TOO_LARGE, row_bytes=c.lens[2])   # under the real constants
    m = c.check(_whole(c), max_row=c.lens[2])                                   # allowed, it is a segment of its own: flushed in front and behind
    assert [(s["first_row"], s["end_row"], s["flush_before"]) for s in m["segments"]] == [(0, 2, 0), (2, 3, 1), (3, 5, 1)]
    c.close()


def test_failed_ordering():
    """Event order decides, whatever the reason and whatever another slot holds."""
    c = _Case(["IIPIBI"], big=5000)                                             # a partial Update in front of an oversize row
    ms = c.members
    c.status(_whole(c), SP.FAILED, max_row=4000, event=ms[2], reason=SP.R_PARTIAL_UPDATE, row_bytes=0)
    c.status([(ms[3], c.n)], SP.FAILED, max_row=4000, event=ms[4], reason=SP.R_ROW_TOO_LARGE, row_bytes=c.lens[3])
    c.status(_whole(c), SP.FAILED, max_row=4000, committed=c.keys[3], event=ms[2], reason=SP.R_PARTIAL_UPDATE, row_bytes=0)   # a committed partial Update still fails
    c.close()
    c = _Case(["IBIPII"], big=5000)                                             # ... and behind it
    ms = c.members
    c.status(_whole(c), SP.FAILED, max_row=4000, event=ms[1], reason=SP.R_ROW_TOO_LARGE, row_bytes=c.lens[1])
    c.status(_whole(c), SP.FAILED, event=ms[3], reason=SP.R_PARTIAL_UPDATE, row_bytes=0)
    c.check([(0, ms[3]), (ms[3] + 1, c.n)], flush=100)
    c.close()
    c = _Case(["IbxIPI"], big=5000)                                             # another slot's oversize row and partial Update do not count
    c.status(_whole(c), SP.FAILED, max_row=4000, event=c.members[2], reason=SP.R_PARTIAL_UPDATE, row_bytes=0)
    c1 = _Case(["IbxIPI"], big=5000, slot=1)
    assert len(c1.members) == 2
    c1.status(_whole(c1), SP.FAILED, max_row=4000, event=c1.members[0], reason=SP.R_ROW_TOO_LARGE, row_bytes=c1.lens[0])
    c1.check(_whole(c1), flush=100)                                             # table 42's partial Update is not this slot's
    c.close(); c1.close()


# ---------------------------------------------------------------- caps, NULL outputs, statuses

def test_caps_and_null_outputs():
    c = _Case([_round_robin(300)])
    f = 3 * int(np.mean(c.lens))
    wins = [(0, 100), (100, 100), (101, c.n)]
    ns = c.model(wins, flush=f)["info"]["n_segs"]
    assert ns > 8
    for scap in (0, 1, ns - 1, ns, ns + 5):
        c.check(wins, flush=f, scap=scap)                                       # the full count comes back, nothing is written past the cap
    c.check(wins, flush=f, skip=("segments",))                                  # any output may be NULL
    c.check(wins, flush=f, skip=("windows",))
    c.check(wins, flush=f, skip=("segments", "windows"))
    c.close()


def test_bad_passes():
    c = _Case([_round_robin(60)])
    c.status([(0, 10), (12, 11), (20, 30)], SP.BAD_PASSES, bad_pass=1)          # first_event > data_end
    c.status([(0, 10), (20, c.n + 1)], SP.BAD_PASSES, bad_pass=1)               # beyond n_events
    c.status([(0, 10), (9, 30), (5, 40)], SP.BAD_PASSES, bad_pass=1)            # starts below its predecessor's end; the lowest index
    c.status([(c.n + 1, c.n + 1)], SP.BAD_PASSES, bad_pass=0)
    c.status([(i, i + 1) for i in range(40)] + [(39, 41)], SP.BAD_PASSES, bad_pass=40)
    c.close()


def test_needs_host():
    """An NDJSON object that came back NEEDS_HOST for a DEFERRED cell: its host_event is reported, behind the statuses that come first."""
    cols = [("id", SC.INT8, False, 1), ("x", SC.FLOAT8, True, 0)]
    deferred = "50537618.817359292015891086651596749e82"                     # a float text the fast rule leaves DEFERRED
    msgs = [W.insert(42, ["1", "1.5"]), W.insert(42, ["2", deferred]), W.insert(42, ["3", "2.5"])]
    s = SC.txn(msgs)
    c = _Case(stream=(np.frombuffer(s.bytes(), dtype=np.uint8), s.offsets), prime=SC.simple_table(cols), names=["id", "x"])
    assert c.nd.status == abi.RB_NEEDS_HOST and c.host_event == c.members[1]
    c.status(_whole(c), SP.NEEDS_HOST, event=c.members[1])
    c.status([(0, c.members[1])], SP.NEEDS_HOST, event=c.members[1])            # the object has no rows, whatever the windows hold
    c.status([(2, 1)], SP.BAD_PASSES, bad_pass=0)                               # a status in front of it
    rc, info, bufs = c.raw([], None, 100, 1000, 4, False)
    assert rc == abi.OK and info.status == abi.SFP_NEEDS_HOST and int(info.event) == c.members[1]
    c.close()


def test_table_copy_batch():
    cols = [("id", SC.INT8, False, 1), ("s", 25, True, 0), ("f", SC.FLOAT8, True, 0)]
    rows = [b"%d\ttext %d\\twith tab\t%s\n" % (i, i, b"1.5" if i % 2 else b"\\N") for i in range(700)]
    c = _Case(copy=(cols, rows), tile=64)
    assert c.n == 700 and c.row_event == list(range(700))
    f = 20 * int(np.mean(c.lens))
    m = c.check([], flush=f, model_windows=_whole(c))                           # no passes: one window over all rows
    assert len(m["segments"]) > 20 and all(s["first_commit_lsn"] == s["last_tx_ordinal"] == 0 for s in m["segments"])
    assert m["segments"][3]["first_event"] == m["segments"][3]["first_row"]     # row indexes
    c.check([(0, 300), (300, 700)], flush=f)
    rc, info, bufs = c.raw([], (0, 0), f, 1000, 4, False)                       # a committed offset on a table-copy batch is refused
    assert rc == abi.InvalidArgument
    c.close()


def test_wrong_objects_and_invalid_arguments():
    c = _Case(["IUD", "II"])
    info = abi.SfPlanInfo()
    pa = np.array([[0, c.n, 0, 0, 0, 0, 0]], dtype=np.uint64)

    def call(batch, slot=0, passes=pa.ctypes.data, n=1, nd=c.nd, flush=100, max_row=1000, cm=(0, 0, 0)):
        return c.d.L.etlg_snowflake_plan(c.d.h, batch.h, slot, passes, n, 0, *cm, nd.h if nd is not None else None, flush, max_row, 0, None, 0, None, C.byref(info))

    assert call(c.b) == abi.OK and (int(info.n_members), int(info.n_rows)) == (5, 5)
    assert call(c.b, slot=7) == abi.InvalidArgument and call(c.b, slot=-1) == abi.InvalidArgument          # an unknown slot
    assert call(c.b, passes=None, n=1) == abi.InvalidArgument                                              # n_passes without passes
    assert call(c.b, flush=0) == abi.InvalidArgument and call(c.b, flush=(1 << 32) + 1) == abi.InvalidArgument and call(c.b, flush=1 << 32) == abi.OK
    assert call(c.b, max_row=0) == abi.InvalidArgument
    assert call(c.b, nd=None) == abi.InvalidArgument                                                       # the object is required
    rbin = c.b.rowbinary(0, [1] * 5, on_device=True)
    assert rbin.status == abi.RB_OK and call(c.b, nd=rbin) == abi.InvalidArgument                          # a RowBinary object
    rbin.close()
    dl = c.b.duckdb(0, NAMES[0], what=abi.DL_TUPLES, on_device=True)
    other = c.b.ndjson(1, NAMES[1], on_device=True)
    host = c.b.ndjson(0, NAMES[0], on_device=False)
    assert call(c.b, nd=dl) == abi.InvalidArgument                                                         # a DuckLake object
    assert call(c.b, nd=other) == abi.InvalidArgument and call(c.b, slot=1, nd=other) == abi.OK            # another slot's
    assert call(c.b, nd=host) == abi.InvalidArgument                                                       # host-resident
    buf, offs = _stream(["IUD", "II"])
    b2 = c.d.decode(buf, offs, flags=abi.F_OUTPUT_ON_DEVICE)
    assert call(b2) == abi.InvalidArgument                                                                 # another batch's object
    b2.close()
    bh = c.d.decode(buf, offs)                                                                             # a batch that is not device-resident
    assert call(bh) == abi.InvalidArgument
    bh.close()
    ba = c.d.decode(buf, offs, flags=abi.F_OUTPUT_ON_DEVICE | abi.F_ASYNC)                                 # an ASYNC batch is synced first
    nda = ba.ndjson(0, NAMES[0], on_device=True)
    assert call(ba, nd=nda) == abi.OK and int(info.n_members) == 5
    nda.close(); ba.close()
    bad = np.frombuffer(bytes(buf[:int(offs[2])]) + b"\xFF" * 24, dtype=np.uint8)                          # one that ended in a decode error gives that error
    be = c.d.decode(bad, list(offs[:3]) + [len(bad)], flags=abi.F_OUTPUT_ON_DEVICE | abi.F_ASYNC)
    assert call(be) not in (abi.OK, abi.InvalidArgument)
    be.close()
    dl.close(); other.close(); host.close()
    c.close()
