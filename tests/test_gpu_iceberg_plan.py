"""etlg_iceberg_plan (etl_amd/csrc/finish.hip: k_icp_*) through the C ABI against tests/iceberg_plan.py, the restatement of the
reference's write_events loop for Iceberg (its three refusals, its one insert_rows per table and turn, its table key) and of the Arrow
slice of every column of the changelog object over a write's rows. Every case compares every field the call writes with the model,
exactly: the info, the writes, the windows and the slices. Every output buffer is one entry longer than its cap and filled with a
poison byte first: what lies at or beyond a count or a cap, the entry behind, and everything when the status is not OK must still hold
it. Each case runs with host passes and host outputs and again with device passes and device outputs; the two give the same bytes.
The model's columns — validity, deferred and child validity bits, offsets and child offsets — are read once per case from the
device-resident etlg_batch_iceberg object, whose contents tests/test_gpu_iceberg.py checks, and shared by every check of the case.
The kernels' constants: waves of 64, workgroups of 256, bitmap words of 64 rows, the event tile (2 048 events, or ETLG_ICP_TILE), the
word tile of the popcount scan (1 024 words, or ETLG_ICP_WORDS) and the chunks of 256 tile sums k_icp_scan walks. Three tables share
the streams round robin, so the slot's members lie three events apart.
pgoutput has no Delete without an old image and etlg_batch_iceberg leaves no accepted member without a row:
ETLG_ICE_DELETE_WITHOUT_OLD_ROW and ETLG_ICP_NEEDS_HOST are reachable in the model alone (tests/test_iceberg_plan_model.py)."""
import ctypes as C
import os

import numpy as np
import pytest

from etl_amd import abi
from tests import batch_cuts as BC
from tests import iceberg_plan as IP
from tests import pgwire as W
from tests import scenarios as SC
from tests.test_gpu_ducklake_plan import FILL, OTHER, _dev_bytes, _dev_get, _dev_put

pytestmark = pytest.mark.gpu
N = W.NULL
INT4_A, TEXT_A = 1007, 1009
# a nullable fixed-width column, a nullable text column, a bool column, a column without NULLs (its bitmap is never scanned), an int4[]
# and a text[] column with NULL elements, empty arrays and NULL arrays
ICOLS = [("id", SC.INT8, False, 1), ("v", SC.INT4, True, 0), ("s", SC.TEXT, True, 0), ("b", SC.BOOL, True, 0), ("k", SC.INT4, False, 0),
         ("ia", INT4_A, True, 0), ("ta", TEXT_A, True, 0)]
SUBSET = [(1, "id", SC.INT8, -1), (0, "v", SC.INT4, -1)]                        # a Relation of table 42 with fewer columns: another slot of the same table
MIX = "IUOIGIIU"


def _row(i, long_elem=False):
    j = i // 3                                                                  # (the slot's members lie three events apart)
    ia = N if j % 13 == 4 else "{}" if j % 4 == 0 else "{%d,NULL,3}" % i if j % 4 == 1 else "{7}"
    ta = N if j % 9 == 5 else "{}" if j % 3 == 0 else '{a,NULL,"b c"}' if j % 3 == 1 else "{NULL}"
    if long_elem and j % 17 == 6:
        ia = "{1,%s}" % ("0" * 44 + "5")                                        # an element of more than 40 characters: the cell is handed back DEFERRED
    return [str(i), N if j % 7 == 2 else str(-i), N if j % 5 == 1 else "t'%d" % i, N if j % 11 == 3 else "tf"[j % 2], str(i), ia, ta]


def _imsg(k, i, long_elem=False):
    """Table 42: I Insert, U full Update with a key image, G full Update with a full old image, O Delete with the full old row,
    P partial Update, D key-only Delete, L the Relation with fewer columns, S an Insert under that Relation; T a Truncate and M a Relation of
    table 43;
    x / y: Inserts, full Updates and full-old-row Deletes of tables 43 and 44."""
    row, key = _row(i, long_elem), [str(i)] + [N] * 6
    if k == "I":
        return W.insert(42, row)
    if k == "U":
        return W.update(42, row, key=key)
    if k == "G":
        return W.update(42, row, old=_row(i + 1))
    if k == "O":
        return W.delete(42, old=row)
    if k == "P":
        return W.update(42, row[:2] + [W.TOAST] + row[3:], key=key)
    if k == "D":
        return W.delete(42, key=key)
    if k == "L":
        return W.relation(42, "public", "t", "d", SUBSET)
    if k == "S":
        return W.insert(42, [str(i), str(i)])
    if k == "T":
        return W.truncate([43], 0)
    if k == "M":
        return W.relation(43, "public", "t43", "d", [(1, "id", SC.INT8, -1), (0, "t", SC.TEXT, -1)])
    tid, other = (43 if k == "x" else 44), [str(i), N if i % 4 == 2 else "o%d" % i]
    return W.update(tid, other, key=[str(i), N]) if i % 8 == 1 else W.delete(tid, old=other) if i % 8 == 4 else W.insert(tid, other)


def _stream(groups, long_elem=False):
    s, i = W.Stream(lsn=0x1000), 0
    for pat in groups:
        final = s.lsn + 8 * (len(pat) + 2)
        s.add(W.begin(final, ts=1234, xid=77))
        for k in pat:
            s.add(_imsg(k, i, long_elem))
            i += 1
        s.add(W.commit(final, final + 8, ts=5678, flags=0), lsn=final)
    return np.frombuffer(s.bytes(), dtype=np.uint8), s.offsets


def _round_robin(n, mix=MIX):
    return "".join((mix[(i // 3) % len(mix)], "x", "y")[i % 3] for i in range(n))


def _prime(t):
    SC.simple_table(ICOLS)(t)
    SC.simple_table(OTHER, table_id=43)(t)
    SC.simple_table(OTHER, table_id=44)(t)


def _bits(ptr, n):
    return np.unpackbits(_dev_bytes(ptr, (n + 63) // 64 * 8), bitorder="little")[:n].astype(bool)


def _model_columns(cl):
    """The columns of a device-resident changelog object as tests/iceberg_plan.py takes them: read once, shared by the case's checks."""
    n, out = int(cl.view.n_rows), []
    for i in range(int(cl.view.n_cols)):
        k = cl.column(i)
        col = {"kind": int(k.arrow_kind), "value_bytes": int(k.value_bytes), "validity": _bits(k.validity, n), "deferred": _bits(k.deferred, n),
               "null_count": int(k.null_count), "deferred_count": int(k.deferred_count), "child_null_count": int(k.child_null_count)}
        if k.offsets:
            col["offsets"] = _dev_bytes(k.offsets, 8 * (n + 1)).view(np.int64)
        if col["kind"] == abi.AK_LIST:
            m = int(k.child_count)
            col.update(child_kind=int(k.child_kind), child_count=m, child_validity=_bits(k.child_validity, m) if m else np.zeros(0, dtype=bool),
                       child_offsets=_dev_bytes(k.child_offsets, 8 * (m + 1)).view(np.int64) if m and k.child_offsets else None)
        out.append(col)
    return out


class _Case:
    def __init__(self, groups=None, tile=None, words=None, slot=0, copy=None, parse_arrays=True, long_elem=False):
        from etl_amd.decoder import Decoder
        from oracle import oracle
        knobs = {"ETLG_ICP_TILE": tile, "ETLG_ICP_WORDS": words}
        before = {k: os.environ.get(k) for k in knobs}
        for k, v in knobs.items():
            os.environ.pop(k, None)
            if v:
                os.environ[k] = str(v)                                          # read when the context is created
        try:
            self.d = Decoder(0)
        finally:
            for k, v in before.items():
                os.environ.pop(k, None)
                if v is not None:
                    os.environ[k] = v
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
            self.stream = _stream(groups, long_elem)
            _prime(self.d)
            _prime(o)
            self.b = self.d.decode(*self.stream, flags=abi.F_OUTPUT_ON_DEVICE)
            rb = o.decode(*self.stream)
        assert self.b.rc == 0, self.b.error
        assert rb.err_code == 0, rb.err_desc
        self.hb = rb.host_batch()
        self.ev = IP.of_host_batch(self.hb)
        self.n, self.slot = len(self.ev[0]), slot
        self.table_id = int(self.hb.slots[slot].table_id)
        self.members = [i for i in range(self.n) if self.ev[0][i] in "IUD" and int(self.ev[2][i]) == slot]
        self.cl = self.b.iceberg(slot, parse_arrays=parse_arrays, on_device=True)
        self.R, self.ncols = int(self.cl.view.n_rows), int(self.cl.view.n_cols)
        self.row_event = _dev_get(self.cl.view.row_event, self.R).tolist()
        self.cols = _model_columns(self.cl)

    def at(self, r):
        """The event at which row r of the object begins (the end of the events for r == n_rows): a window placed on rows."""
        return self.row_event[r] if r < self.R else self.n

    def model(self, windows):
        if self.copy:
            return IP.plan_copy(self.row_event, self.cols)
        return IP.plan(*self.ev, self.slot, self.table_id, windows, self.row_event, self.cols)

    def raw(self, windows, wcap, dev, skip=(), passes=True, cl=None, slot=None):
        """One call with poison-filled buffers of wcap writes, wcap * n_cols slices and one entry per window, and a guard entry each."""
        nwin = len(windows) if (len(windows) or not self.copy) else 1
        words = {"writes": 7 * (wcap + 1), "slices": 7 * (wcap * self.ncols + 1), "windows": 6 * (nwin + 1)}
        pa = np.full((len(windows), 7), FILL, dtype=np.uint64)                  # only first_event and data_end are read
        for p, (lo, hi) in enumerate(windows):
            pa[p, 0], pa[p, 1] = lo, hi
        bufs = {k: np.full(words[k], FILL, dtype=np.uint64) for k in words if k not in skip}
        owners = {k: _dev_put(a) for k, a in bufs.items()} if dev else {}
        pown = _dev_put(pa.reshape(-1)) if dev else None
        ptr = lambda k: None if k in skip else (owners[k][1] if dev else bufs[k].ctypes.data)
        pptr = None if not passes or not len(windows) else (pown[1] if dev else pa.ctypes.data)
        info = abi.IcePlanInfo()
        rc = self.d.L.etlg_iceberg_plan(self.d.h, self.b.h, self.slot if slot is None else slot, pptr, len(windows), 1 if dev and pptr else 0, (cl or self.cl).h,
                                        abi.F_OUTPUT_ON_DEVICE if dev else 0, ptr("writes"), wcap, ptr("slices"), ptr("windows"), C.byref(info))
        if dev:
            bufs = {k: _dev_get(owners[k][1], words[k]) for k in bufs}
        return rc, info, bufs

    def check(self, windows, wcap=None, skip=()):
        """Host and device memory against the model, field by field; returns the model."""
        m = self.model(windows)
        assert m["status"] == IP.OK, m
        wcap = m["info"]["n_writes"] if wcap is None else wcap
        got = {}
        for dev in (False, True):
            rc, info, bufs = self.raw(windows, wcap, dev, skip)
            assert rc == abi.OK and info.status == abi.ICP_OK, (rc, info.status, int(info.event), int(info.bad_pass), info.reason)
            gi = {k: int(getattr(info, k)) for k in IP.INFO_FIELDS}
            assert gi == m["info"], (dev, gi, m["info"])
            assert (int(info.event), int(info.bad_pass), int(info.fail_pass), info.reason) == (IP.NONE, IP.NONE, IP.NONE, 0)
            self.compare(m, bufs, wcap, dev)
            got[dev] = bufs
        for k in got[False]:
            assert np.array_equal(got[False][k], got[True][k]), k              # host and device output pointers: the same bytes
        return m

    def compare(self, m, bufs, wcap, dev):
        S, P, nc = min(wcap, len(m["writes"])), len(m["windows"]), self.ncols
        want = {"writes": np.array([[s[f] for f in IP.WRITE_FIELDS] for s in m["writes"][:S]], dtype=np.uint64).reshape(S, 7),
                "windows": np.array([[w[f] for f in IP.WIN_FIELDS] for w in m["windows"]], dtype=np.uint64).reshape(P, 6),
                "slices": np.array([[c[f] for f in IP.SLICE_FIELDS] for s in m["slices"][:S] for c in s], dtype=np.uint64).reshape(S * nc, 7)}
        for k, a in bufs.items():
            rows, width = want[k].shape
            got = a[:rows * width].reshape(rows, width)
            bad = np.flatnonzero((got != want[k]).any(axis=1))
            assert not len(bad), (k, dev, int(bad[0]), got[bad[0]].tolist(), want[k][bad[0]].tolist())
            assert (a[rows * width:] == FILL).all(), (k, dev)

    def status(self, windows, want, **fields):
        """A status other than OK, on host and device memory: every field of the info, and every output word still poison."""
        m = self.model(windows)
        assert m["status"] == want and all(m[k] == v for k, v in fields.items()), m
        full = (m.get("event", IP.NONE), m.get("bad_pass", IP.NONE), m.get("fail_pass", IP.NONE), m.get("reason", 0))
        for dev in (False, True):
            rc, info, bufs = self.raw(windows, 8, dev)
            assert rc == abi.OK and info.status == want, (dev, rc, info.status, int(info.event))
            assert (int(info.event), int(info.bad_pass), int(info.fail_pass), info.reason) == full, (dev, int(info.event), int(info.bad_pass), int(info.fail_pass), info.reason, m)
            assert all(int(getattr(info, k)) == 0 for k in IP.INFO_FIELDS), dev
            assert all((a == FILL).all() for a in bufs.values()), dev

    def sums(self, m):
        """Over writes that cover all rows the slices' counts sum to the columns' own."""
        assert sum(s["end_row"] - s["first_row"] for s in m["writes"]) == self.R
        for c, col in enumerate(self.cols):
            for f in ("null_count", "deferred_count", "child_null_count"):
                assert sum(s[c][f] for s in m["slices"]) == col[f], (c, f)

    def close(self):
        self.cl.close(); self.b.close(); self.d.close()


def _whole(c):
    return [(0, c.n)]


def _row_windows(c, cuts):
    """Windows that begin and end at the given rows of the object."""
    cuts = sorted(set(x for x in cuts if 0 <= x <= c.R) | {0, c.R})
    return [(c.at(a), c.at(b)) for a, b in zip(cuts, cuts[1:])]


# ---------------------------------------------------------------- objects around the word size

@pytest.mark.parametrize("rows", [1, 63, 64, 65, 128, 129])
def test_object_sizes(rows):
    c = _Case([_round_robin(3 * rows)])
    assert c.R == rows == len(c.members) and c.ncols == len(ICOLS) + 2
    kinds = [col["kind"] for col in c.cols]
    assert kinds == [abi.AK_INT64, abi.AK_INT32, abi.AK_LARGE_UTF8, abi.AK_BOOLEAN, abi.AK_INT32, abi.AK_LIST, abi.AK_LIST, abi.AK_LARGE_UTF8, abi.AK_LARGE_UTF8]
    assert c.cols[5]["child_kind"] == abi.AK_INT32 and c.cols[6]["child_kind"] == abi.AK_LARGE_UTF8
    if rows >= 63:                                                              # NULLs in every nullable column, NULL elements in both lists, none in id / k / the CDC columns
        assert all(c.cols[i]["null_count"] > 0 for i in (1, 2, 3, 5, 6)) and all(c.cols[i]["null_count"] == 0 for i in (0, 4, 7, 8))
        assert c.cols[5]["child_null_count"] > 0 and c.cols[6]["child_null_count"] > 0
    m = c.check(_whole(c))                                                      # one window over everything
    assert m["info"]["n_writes"] == 1 and m["info"]["n_rows"] == rows
    c.sums(m)
    m = c.check([(i, i + 1) for i in range(c.n)])                               # a window per event: a write of one row per member
    assert m["info"]["n_writes"] == rows and all(s["end_row"] - s["first_row"] == 1 for s in m["writes"])
    c.sums(m)
    m = c.check(_row_windows(c, [1, 5, 63, 64, 65, 70, 127, 128]))              # windows that begin and end inside a word and exactly on a word boundary
    c.sums(m)
    c.close()


def test_window_shapes_and_the_outline():
    c = _Case([_round_robin(330), _round_robin(270)], long_elem=True)
    ms = c.members
    assert c.R == len(ms) and any(col["deferred_count"] > 0 for col in c.cols)  # a deferred cell: its bitmap is scanned
    assert set(c.ev[0][e] for e in ms) == {"I", "U", "D"}                        # a full-old-row Delete and full Updates among the members
    m = c.check(_whole(c))
    c.sums(m)
    m = c.check([(0, 10), (10, 10), (10, 40), (40, 40), (c.n, c.n)])            # empty windows between non-empty ones, one at the very end
    assert [w["n_writes"] for w in m["windows"]] == [1, 0, 1, 0, 0] and m["windows"][4]["first_row"] == m["windows"][4]["end_row"] == c.R
    gap = next(i for i in range(c.n - 1) if i not in ms and i + 1 not in ms)
    m = c.check([(0, gap), (gap, gap + 2), (gap + 2, c.n)])                     # a window without a member of the slot
    assert m["windows"][1]["n_members"] == 0 and m["info"]["n_writes"] == 2
    c.sums(m)
    m = c.check(_row_windows(c, [64, 128, 130, 131]))
    c.sums(m)
    got = c.b.iceberg_plan(0, np.array([[0, c.n, 0, 0, 0, 0, 0]], dtype=np.uint64), c.cl)   # the Python layer: count, then fill
    assert got.info.status == abi.ICP_OK and len(got.writes) == 1 and len(got.slices) == 1 and len(got.slices[0]) == c.ncols and len(got.windows) == 1
    assert [[int(getattr(s, f)) for f in IP.SLICE_FIELDS] for s in got.slices[0]] == [[s[f] for f in IP.SLICE_FIELDS] for s in c.model(_whole(c))["slices"][0]]
    for dev in (False, True):                                                   # n_passes == 0, with and without a pointer
        for passes in (True, False):
            rc, info, bufs = c.raw([], 4, dev, passes=passes)
            assert rc == abi.OK and info.status == abi.ICP_OK and all(int(getattr(info, k)) == 0 for k in IP.INFO_FIELDS)
            assert all((a == FILL).all() for a in bufs.values())
    c.close()
    c1 = _Case([_round_robin(300)], slot=1)                                     # another slot of the same stream: no list column, no scanned child bitmap
    c1.sums(c1.check([(0, c1.n // 2), (c1.n // 2, c1.n)]))
    c1.close()


def test_outline_passes_with_truncates_and_inline_relations():
    """The outline's own passes, taken with ETLG_OL_RELATIONS_INLINE, over a stream with Truncates and a Relation inside a data run."""
    pat = _round_robin(60) + "T" + _round_robin(45) + "M" + _round_robin(30) + "TT" + _round_robin(30)
    c = _Case([pat])
    sm = BC.size_model()
    total = int(c.b.cuts(sm, 1 << 62, cap=0)[1].total)
    cuts, ci = c.b.cuts(sm, max(1, total // 3))
    ol = c.b.outline(cuts=cuts, relations_inline=True)
    assert ol.info.status == abi.OL_OK and len(ol.passes) >= 3 and int(ol.info.n_trunc) >= 2
    rel = c.ev[0].index("R")
    assert any(int(p[0]) < rel < int(p[1]) for p in ol.passes)                  # the Relation lies inside a window
    m = c.check([(int(p[0]), int(p[1])) for p in ol.passes])
    assert m["info"]["n_writes"] >= 3
    c.sums(m)
    got = c.b.iceberg_plan(0, ol.passes, c.cl)
    assert [[int(getattr(s, f)) for f in IP.WRITE_FIELDS] for s in got.writes] == [[s[f] for f in IP.WRITE_FIELDS] for s in m["writes"]]
    assert [[int(getattr(w, f)) for f in IP.WIN_FIELDS] for w in got.windows] == [[w[f] for f in IP.WIN_FIELDS] for w in m["windows"]]
    c.close()


# ---------------------------------------------------------------- tiles of both scans

@pytest.mark.parametrize("tile,words", [(256, 4), (None, None), (8, 1)])
def test_tile_crossings(tile, words):
    """3 600 events: with ETLG_ICP_TILE=256 and ETLG_ICP_WORDS=4 several tiles of both scans, with the default tiles a second event tile;
    with tiles of 8 events and of one word more than one chunk of 256 tile sums in k_icp_scan, for both scans."""
    mk = (lambda n: "".join(MIX[i % len(MIX)] for i in range(n))) if tile == 8 else _round_robin   # (tiles of one word: table 42 alone, three times the rows)
    c = _Case([mk(1800), mk(1796)], tile=tile, words=words, long_elem=True)
    t, wt = tile or 2048, words or 1024
    assert c.n == 3600 and c.R == (3596 if tile == 8 else 1199)
    n_words = sum((c.R + 63) // 64 for col in c.cols for f in ("null_count", "deferred_count") if col[f]) + \
        sum((col["child_count"] + 63) // 64 for col in c.cols if col.get("child_null_count") and col["kind"] == abi.AK_LIST)
    assert n_words > 100
    if tile == 8:
        assert c.n // t > 256 and n_words // wt > 256
    elif tile:
        assert c.n // t > 8 and n_words // wt > 8
    c.sums(c.check(_whole(c)))
    c.sums(c.check([(0, t - 1), (t - 1, t), (t, t + 1), (t + 1, c.n)]))         # windows that end on an event tile's last and first event
    w = 64 * wt if 64 * wt < c.R else 64                                        # rows of one word tile of the first scanned bitmap
    m = c.check(_row_windows(c, [w - 1, w, w + 1, 2 * w, 5 * w + 3, 9 * w]))     # on a word tile's boundary, and across several tiles
    c.sums(m)
    if tile != 8:
        c.sums(c.check([(i, min(i + 7, c.n)) for i in range(0, c.n, 7)]))      # windows that straddle every tile
    c.close()


# ---------------------------------------------------------------- failing members, bad passes

def test_refusals():
    c = _Case(["IIxPyIOI"])                                                     # a partial Update
    ms = c.members
    c.status(_whole(c), IP.FAILED, event=ms[2], reason=IP.PARTIAL_UPDATE, fail_pass=0)              # in the first window
    c.status([(0, ms[1]), (ms[1], ms[3]), (ms[3], c.n)], IP.FAILED, event=ms[2], reason=IP.PARTIAL_UPDATE, fail_pass=1)   # in a later one
    m = c.check([(0, ms[2]), (ms[2] + 1, c.n)])                                 # outside every window it does not fail the call
    assert m["info"]["n_members"] == len(ms) - 1 == c.R
    c.close()
    c = _Case(["IIDIGO"])                                                       # a key-only Delete; the full Update and the full-old-row Delete pass
    ms = c.members
    c.status(_whole(c), IP.FAILED, event=ms[2], reason=IP.KEY_ONLY_DELETE, fail_pass=0)
    assert c.check([(0, ms[2]), (ms[3], c.n)])["info"]["n_rows"] == 5
    c.close()
    c = _Case(["IPxDI", "IDyPI"])                                               # both in one batch: the lower event wins, whichever its reason
    ms = c.members
    c.status(_whole(c), IP.FAILED, event=ms[1], reason=IP.PARTIAL_UPDATE, fail_pass=0)
    c.status([(0, ms[1]), (ms[2], c.n)], IP.FAILED, event=ms[2], reason=IP.KEY_ONLY_DELETE, fail_pass=1)
    c.status([(ms[4], c.n)], IP.FAILED, event=ms[5], reason=IP.KEY_ONLY_DELETE, fail_pass=0)
    c.status([(0, 1), (ms[6], c.n)], IP.FAILED, event=ms[6], reason=IP.PARTIAL_UPDATE, fail_pass=1)
    c.close()
    c1 = _Case(["IIPIxDI"], slot=1)                                             # a failing event of another slot does not count
    c1.check(_whole(c1))
    c1.close()


def test_bad_passes():
    c = _Case([_round_robin(60)])
    c.status([(0, 10), (12, 11), (20, 30)], IP.BAD_PASSES, bad_pass=1)          # descending
    c.status([(0, 10), (20, c.n + 1)], IP.BAD_PASSES, bad_pass=1)               # beyond n_events
    c.status([(0, 10), (9, 30), (5, 40)], IP.BAD_PASSES, bad_pass=1)            # overlapping; the lowest index
    c.status([(i, i + 1) for i in range(40)] + [(39, 41)], IP.BAD_PASSES, bad_pass=40)
    c.close()
    c = _Case(["IIPI"])                                                         # BAD_PASSES comes before FAILED
    c.status([(2, 1)], IP.BAD_PASSES, bad_pass=0)
    c.close()


# ---------------------------------------------------------------- two slots of one table

def test_two_slots_of_one_table():
    """A Relation that changes the table's replicated columns in mid-window: the members behind it decode under another slot of the same
    table id, and the window names the first of them. With a Truncate between them they lie in separate windows."""
    c = _Case(["IxIyILSxSS"])
    assert len(c.hb.slots) == 4 and int(c.hb.slots[3].table_id) == c.table_id == 42
    other = [i for i in range(c.n) if c.ev[0][i] == "I" and int(c.ev[2][i]) == 3]
    assert len(other) == 3 and len(c.members) == 3                              # (every Insert behind the Relation is the new slot's)
    m = c.check(_whole(c))
    assert m["windows"][0]["other_slot_event"] == other[0] == m["writes"][0]["other_slot_event"] and m["info"]["n_mixed"] == 1
    m = c.check([(0, c.members[1]), (c.members[1], other[1]), (other[1], c.n)])
    assert [w["other_slot_event"] for w in m["windows"]] == [IP.NONE, other[0], IP.NONE] and m["info"]["n_mixed"] == 1
    assert [w["n_writes"] for w in m["windows"]] == [1, 1, 0]                    # a window without a member of this slot names no event
    c3 = _Case(["IxIyILSxSS"], slot=3, parse_arrays=False)                      # the mirror image: the plan of the new slot names the old slot's members
    m3 = c3.check(_whole(c3))
    assert m3["windows"][0]["other_slot_event"] == c.members[0] and m3["info"]["n_members"] == 3
    c3.close()
    c.close()
    c = _Case(["IxIyITLSxSS"])                                                  # the same with a Truncate between them: the outline's windows
    ol = c.b.outline(relations_inline=True)
    assert len(ol.passes) == 2
    m = c.check([(int(p[0]), int(p[1])) for p in ol.passes])
    assert [w["other_slot_event"] for w in m["windows"]] == [IP.NONE, IP.NONE] and m["info"]["n_mixed"] == 0 and [w["n_writes"] for w in m["windows"]] == [1, 0]
    c.close()


# ---------------------------------------------------------------- caps, NULL outputs

def test_caps_and_null_outputs():
    c = _Case([_round_robin(300)])
    wins = [(0, 40), (40, 40), (41, 100), (100, 101), (101, 200), (200, c.n)]
    nw = c.model(wins)["info"]["n_writes"]
    assert nw >= 4
    for wcap in (0, 1, nw - 1, nw, nw + 5):
        c.check(wins, wcap=wcap)                                                # the full count comes back, nothing is written past the cap
    for skip in (("writes",), ("slices",), ("windows",), ("writes", "slices"), ("writes", "slices", "windows")):
        c.check(wins, skip=skip)                                                # any output may be NULL
    c.close()


# ---------------------------------------------------------------- table-copy batches

COPY_COLS = [("id", SC.INT8, False, 1), ("s", SC.TEXT, True, 0), ("b", SC.BOOL, True, 0)]


@pytest.mark.parametrize("rows", [0, 1, 130])
def test_copy_batches(rows):
    lines = [b"%d\t%s\t%s\n" % (i, b"\\N" if i % 3 == 1 else b"t%d" % i, b"\\N" if i % 5 == 2 else b"tf"[i % 2:i % 2 + 1]) for i in range(rows)]
    c = _Case(copy=(COPY_COLS, lines), parse_arrays=False)
    assert c.R == rows and c.row_event == list(range(rows))
    m = c.check([])
    assert m["info"]["n_writes"] == (1 if rows else 0) and m["windows"][0]["end_row"] == rows
    c.sums(m)
    for wcap in (0, 1, 3):
        c.check([], wcap=wcap)
    for skip in (("writes",), ("slices",), ("windows",), ("writes", "slices", "windows")):
        c.check([], skip=skip)
    info = abi.IcePlanInfo()
    pa = np.array([[0, c.n, 0, 0, 0, 0, 0]], dtype=np.uint64)
    call = lambda p, n, cl=c.cl: c.d.L.etlg_iceberg_plan(c.d.h, c.b.h, 0, p, n, 0, cl.h, 0, None, 0, None, None, C.byref(info))
    assert call(pa.ctypes.data, 1) == abi.InvalidArgument                       # a table-copy batch takes no passes
    assert call(None, 0) == abi.OK and int(info.n_writes) == (1 if rows else 0)
    dlc = c.b.ducklake_copy(0, on_device=True)                                  # an object of etlg_batch_ducklake_copy, of this very batch and slot
    assert call(None, 0, dlc) == abi.InvalidArgument
    dlc.close()
    c.close()


# ---------------------------------------------------------------- wrong objects

def test_wrong_objects_and_invalid_arguments():
    c = _Case(["IUO", "IG"])
    info = abi.IcePlanInfo()
    pa = np.array([[0, c.n, 0, 0, 0, 0, 0]], dtype=np.uint64)

    def call(batch, slot=0, passes=pa.ctypes.data, n=1, cl=c.cl):
        return c.d.L.etlg_iceberg_plan(c.d.h, batch.h, slot, passes, n, 0, cl.h if cl is not None else None, 0, None, 0, None, None, C.byref(info))

    assert call(c.b) == abi.OK and (int(info.n_members), int(info.n_rows), int(info.n_writes)) == (5, 5, 1)
    assert call(c.b, slot=7) == abi.InvalidArgument and call(c.b, slot=-1) == abi.InvalidArgument          # an unknown slot
    assert call(c.b, passes=None, n=1) == abi.InvalidArgument                                              # n_passes without passes
    assert call(c.b, cl=None) == abi.InvalidArgument                                                       # the object is required
    plain = c.b.columns(0, kinds=("I", "U"), on_device=True, parse_arrays=True)
    other = c.b.iceberg(1, on_device=True)
    host = c.b.iceberg(0, parse_arrays=True, on_device=False)
    assert call(c.b, cl=plain) == abi.InvalidArgument                                                      # an object of etlg_batch_columns
    assert call(c.b, cl=other) == abi.InvalidArgument and call(c.b, slot=1, cl=other) == abi.OK            # another slot's
    assert call(c.b, cl=host) == abi.InvalidArgument                                                       # host-resident
    b2 = c.d.decode(*c.stream, flags=abi.F_OUTPUT_ON_DEVICE)
    assert call(b2) == abi.InvalidArgument                                                                 # another batch's object
    b2.close()
    bh = c.d.decode(*c.stream)                                                                             # a batch that is not device-resident
    assert call(bh) == abi.InvalidArgument
    bh.close()
    ba = c.d.decode(*c.stream, flags=abi.F_OUTPUT_ON_DEVICE | abi.F_ASYNC)                                 # an ASYNC batch is synced first
    cla = ba.iceberg(0, parse_arrays=True, on_device=True)
    assert call(ba, cl=cla) == abi.OK and int(info.n_members) == 5
    cla.close(); ba.close()
    buf, offs = c.stream
    bad = np.frombuffer(bytes(buf[:int(offs[2])]) + b"\xFF" * 24, dtype=np.uint8)                          # one that ended in a decode error gives that error
    be = c.d.decode(bad, list(offs[:3]) + [len(bad)], flags=abi.F_OUTPUT_ON_DEVICE | abi.F_ASYNC)
    assert call(be) not in (abi.OK, abi.InvalidArgument)
    be.close()
    plain.close(); other.close(); host.close()
    c.close()
