"""etlg_ducklake_plan (etl_amd/csrc/finish.hip: k_dlp_*) through the C ABI against tests/ducklake_plan.py, the restatement of the
reference's three loops (retain_mutations_after_sequence_key, prepare_mutation_table_batches, prepare_table_mutations). Every case
compares every field the call writes with the model, exactly: the info, the ranges, the batches and the ops. Every output buffer is
one word longer than its cap and filled with a poison byte first: what lies at or beyond a count or a cap, the word behind, and
everything when the status is not OK must still hold it. Each case runs with host passes and host outputs and again with device passes
and device outputs; the two give the same bytes.
The kernels' constants: waves of 64, workgroups of 256, groups of 16, the tile (2 048 events, or ETLG_DLP_TILE in a context of its own)
and the chunks of 256 tile sums k_dlp_scan walks. Three tables share the streams round robin, so the 16 members of a group lie about 48
events apart and straddle tiles of 8 and 64; tiles of 512 and 2 048 run the chunk loop of k_dlp_write and its carry."""
import ctypes as C
import os

import numpy as np
import pytest

from etl_amd import abi
from tests import ducklake_identity as ID
from tests import ducklake_literals as DL
from tests import ducklake_plan as DP
from tests import ducklake_updates as DU
from tests import pgwire as W
from tests import scenarios as SC

pytestmark = pytest.mark.gpu
EMU = os.environ.get("ETLG_SIMT_RUN") == "1"
FILL = 0xEEEEEEEEEEEEEEEE
T = W.TOAST
COLS3 = [("id", SC.INT8, False, 1), ("v", SC.INT4, True, 0), ("s", 25, True, 0)]
OTHER = [("id", SC.INT8, False, 1), ("t", 25, True, 0)]
NAMES = {0: ["id", "v", "s"], 1: ["id", "t"], 2: ["id", "t"]}
SEED = ID.seed("mutation", "public_t")


def _prime3(ident=None):
    def prime(t):
        SC.simple_table(COLS3, ident=ident)(t)
        SC.simple_table(OTHER, table_id=43)(t)
        SC.simple_table(OTHER, table_id=44)(t)
    return prime


def _msg(k, i):
    """One message per letter: I / D / U (full Update, key image) / R (Replace: a full Update without an old image) / P (partial Update,
    key image) / H (partial Update whose identity column is TOAST and that has no old image: no record anywhere) of table 42; x / y:
    the same mix on tables 43 and 44."""
    row = [str(i), W.NULL if i % 7 == 2 else str(-i), "t'%d" % i]
    key = [str(i), W.NULL, W.NULL]
    if k == "I":
        return W.insert(42, row)
    if k == "D":
        return W.delete(42, key=key)
    if k == "U":
        return W.update(42, row, key=key)
    if k == "R":
        return W.update(42, row)
    if k == "P":
        return W.update(42, [str(i), str(i), T], key=key)
    if k == "H":
        return W.update(42, [T, str(i), T])
    tid = 43 if k == "x" else 44
    m = i % 4
    if m == 0:
        return W.delete(tid, key=[str(i), W.NULL])
    if m == 1:
        return W.update(tid, [str(i), "u%d" % i], key=[str(i), W.NULL])
    return W.insert(tid, [str(i), "o%d" % i])


def _stream(groups):
    """groups: one pattern string per transaction -> (buf, offsets); the transactions' final LSNs ascend."""
    s, i = W.Stream(lsn=0x1000), 0
    for pat in groups:
        final = s.lsn + 8 * (len(pat) + 2)
        s.add(W.begin(final, ts=1234, xid=77))
        for k in pat:
            s.add(_msg(k, i))
            i += 1
        s.add(W.commit(final, final + 8, ts=5678, flags=0), lsn=final)
    return np.frombuffer(s.bytes(), dtype=np.uint8), s.offsets


def _round_robin(n, mix="IIUDIRPIID"):
    """n events: table 42's mix with tables 43 and 44 in between, so that slot 0's members lie three events apart."""
    return "".join((mix[(i // 3) % len(mix)], "x", "y")[i % 3] for i in range(n))


# ---------------------------------------------------------------- device memory of the test's own

def _dev_put(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if EMU:
        own = a.copy() if len(a) else np.zeros(1, dtype=np.uint64)
        return own, own.ctypes.data
    import torch
    own = torch.from_numpy((a if len(a) else np.zeros(1, dtype=np.uint64)).view(np.int64)).cuda()
    torch.cuda.synchronize()
    return own, own.data_ptr()


def _dev_bytes(ptr, n):
    if not n:
        return np.zeros(0, dtype=np.uint8)
    if EMU:
        return np.frombuffer((C.c_uint8 * n).from_address(ptr), dtype=np.uint8).copy()
    return abi.device_tensor(ptr, n, 0).cpu().numpy().view(np.uint8)


def _dev_get(ptr, n):
    return _dev_bytes(ptr, 8 * n).view(np.uint64)


# ---------------------------------------------------------------- one decoded batch, its model, and the raw call

class _Case:
    def __init__(self, groups, tile=None, slot=0, ident=None, objects="tpu", stream=None):
        from etl_amd.decoder import Decoder
        from oracle import oracle
        buf, offs = stream or _stream(groups)                                  # stream: one the test built itself
        prime = _prime3(ident)
        before = os.environ.get("ETLG_DLP_TILE")
        if tile:
            os.environ["ETLG_DLP_TILE"] = str(tile)                            # read when the context is created
        try:
            self.d = Decoder(0)
        finally:
            os.environ.pop("ETLG_DLP_TILE", None)
            if before is not None:
                os.environ["ETLG_DLP_TILE"] = before
        prime(self.d)
        self.b = self.d.decode(buf, offs, flags=abi.F_OUTPUT_ON_DEVICE)
        assert self.b.rc == 0, self.b.error
        o = oracle.Oracle()
        prime(o)
        rb = o.decode(buf, offs)
        assert rb.err_code == 0, rb.err_desc
        self.hb = rb.host_batch()
        self.ev = DP.of_host_batch(self.hb)
        self.n, self.slot, self.names = len(self.ev[0]), slot, NAMES[slot]
        self.events = self.hb.materialize()
        self.ident = [c.identity for c in self.hb.slots[slot].cols]
        self.members = [i for i in range(self.n) if self.ev[0][i] in "IUD" and int(self.ev[2][i]) == slot]
        self.objs, self.recs = {}, {}
        self.build(objects)

    def build(self, objects):
        """The device-resident objects and the model's records (strings, event per record) of those asked for."""
        args = (self.events, self.slot, self.names, self.ident)
        for o, what, dwhat in (("t", DL.TUPLES, abi.DL_TUPLES), ("p", DL.PREDICATES, abi.DL_PREDICATES), ("u", None, abi.DL_UPDATES)):
            if o not in objects:
                continue
            recs, idx = (DU.update_records(*args) if o == "u" else DL.event_records(*args, what))[:2]
            r = self.b.duckdb(self.slot, self.names, what=dwhat, on_device=True)
            assert r.status == abi.RB_OK and r.n_rows == len(recs)
            assert _dev_get(r.view.row_event, r.n_rows).tolist() == idx
            self.objs[o], self.recs[o] = r, (recs, idx)

    def model(self, windows, watermark=None, use="tpu"):
        idx = {o: (self.recs[o][1] if o in use else None) for o in "tpu"}
        return DP.plan(*self.ev, self.slot, windows, watermark=watermark, n_ident=sum(self.ident), tuples=idx["t"], predicates=idx["p"], updates=idx["u"])

    def raw(self, windows, watermark, use, bcap, ocap, dev, skip=(), seed=SEED, passes=True):
        """One call with poison-filled buffers of bcap / ocap entries and a guard word each -> (rc, info, {name: every word of its buffer})."""
        words = {"ranges": 3 * bcap, "batches": 13 * bcap, "ops": 4 * ocap}
        pa = np.full((len(windows), 7), FILL, dtype=np.uint64)                  # only first_event and data_end are read
        for p, (lo, hi) in enumerate(windows):
            pa[p, 0], pa[p, 1] = lo, hi
        bufs = {k: np.full(words[k] + 1, FILL, dtype=np.uint64) for k in words if k not in skip}
        owners = {k: _dev_put(a) for k, a in bufs.items()} if dev else {}
        pown = _dev_put(pa.reshape(-1)) if dev else None
        ptr = lambda k: None if k in skip else (owners[k][1] if dev else bufs[k].ctypes.data)
        pptr = None if not passes or (not len(windows) and not dev) else (pown[1] if dev else pa.ctypes.data)
        h = lambda o: self.objs[o].h if o in use else None
        wm = (0, 0, 0) if watermark is None else (1, int(watermark[0]), int(watermark[1]))
        info = abi.DlPlanInfo()
        rc = self.d.L.etlg_ducklake_plan(self.d.h, self.b.h, self.slot, pptr, len(windows), 1 if dev else 0, *wm, seed, h("t"), h("p"), h("u"),
                                         abi.F_OUTPUT_ON_DEVICE if dev else 0, ptr("ranges"), ptr("batches"), bcap, ptr("ops"), ocap, C.byref(info))
        if dev:
            bufs = {k: _dev_get(owners[k][1], words[k] + 1) for k in bufs}
        return rc, info, bufs

    def check(self, windows, watermark=None, use="tpu", bcap=None, ocap=None, skip=()):
        """Host and device memory against the model, field by field; returns the model."""
        m = self.model(windows, watermark, use)
        assert m["status"] == DP.OK, m
        bcap = m["info"]["n_batches"] if bcap is None else bcap
        ocap = m["info"]["n_ops"] if ocap is None else ocap
        got = {}
        for dev in (False, True):
            rc, info, bufs = self.raw(windows, watermark, use, bcap, ocap, dev, skip)
            assert rc == abi.OK and info.status == abi.DLP_OK, (rc, info.status, int(info.event), int(info.bad_pass))
            gi = {k: int(getattr(info, k)) for k in DP.INFO_FIELDS}
            assert gi == m["info"], (dev, gi, m["info"])
            self.compare(m, bufs, bcap, ocap, dev)
            got[dev] = bufs
        for k in got[False]:
            assert np.array_equal(got[False][k], got[True][k]), k              # host and device output pointers: the same bytes
        return m

    def compare(self, m, bufs, bcap, ocap, dev):
        B, K = min(bcap, len(m["batches"])), min(ocap, len(m["ops"]))
        if "ranges" in bufs:
            want = np.array([[b["first_event"], b["end_event"], SEED] for b in m["batches"][:B]], dtype=np.uint64).reshape(B, 3)
            assert np.array_equal(bufs["ranges"][:3 * B].reshape(B, 3), want), dev
            assert (bufs["ranges"][3 * B:] == FILL).all(), dev
        if "batches" in bufs:
            want = np.array([[b[f] for f in DP.BATCH_FIELDS[:9]] + [b["n_members"] | b["n_ops"] << 32, b["n_cat"][0] | b["n_cat"][1] << 32,
                                                                    b["n_cat"][2] | b["n_cat"][3] << 32, b["n_cat"][4]]
                             for b in m["batches"][:B]], dtype=np.uint64).reshape(B, 13)
            got = bufs["batches"][:13 * B].reshape(B, 13)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert not len(bad), (dev, int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())
            assert (bufs["batches"][13 * B:] == FILL).all(), dev
        if "ops" in bufs:
            want = np.array([[o["kind"] | o["origin"] << 32, o["first_event"], o["n"], o["rec_first"]] for o in m["ops"][:K]], dtype=np.uint64).reshape(K, 4)
            got = bufs["ops"][:4 * K].reshape(K, 4)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert not len(bad), (dev, int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())
            assert (bufs["ops"][4 * K:] == FILL).all(), dev

    def status(self, windows, want, watermark=None, use="tpu", **fields):
        """A status other than OK, on host and device memory: the info's fields, and every output word still poison."""
        m = self.model(windows, watermark, use)
        assert m["status"] == want and all(m[k] == v for k, v in fields.items()), m
        for dev in (False, True):
            rc, info, bufs = self.raw(windows, watermark, use, 8, 8, dev)
            assert rc == abi.OK and info.status == want, (dev, rc, info.status)
            assert all(int(getattr(info, k)) == v for k, v in fields.items()), (dev, int(info.event), int(info.bad_pass), info.reason)
            assert all(int(getattr(info, k)) == 0 for k in DP.INFO_FIELDS), dev
            assert all((a == FILL).all() for a in bufs.values()), dev

    def op_strings(self, m, bufs, use):
        """Per op the device's records cut out of the device objects by rec_first, against the model's strings of the op's members."""
        ops = bufs["ops"][:4 * len(m["ops"])].reshape(-1, 4)
        texts = {}
        for o in use:
            v = self.objs[o].view
            texts[o] = (_dev_bytes(v.bytes, int(v.n_bytes)).tobytes(), _dev_bytes(v.row_offsets, 8 * (int(v.n_rows) + 1)).view(np.int64))
        for b in m["batches"]:
            for k in range(b["op_first"], b["op_first"] + b["n_ops"]):
                mo, (kind, first, n, rec) = m["ops"][k], (int(ops[k][0]) & 0xFFFFFFFF, int(ops[k][1]), int(ops[k][2]), int(ops[k][3]))
                o = "u" if kind == DP.OP_UPDATE else "t" if kind == DP.UPSERT else "p"
                if o not in use:
                    assert rec == DP.NONE
                    continue
                at = b["members"].index(first)
                mine = b["members"][at:at + n]
                recs, idx = self.recs[o]
                want = b"".join(r for r, i in zip(recs, idx) if i in mine)
                data, offs = texts[o]
                per = 2 if o == "u" else 1
                assert data[int(offs[rec]):int(offs[rec + per * n])] == want, (k, mo)

    def close(self):
        for r in self.objs.values():
            r.close()
        self.b.close(); self.d.close()


def _whole(c):
    return [(0, c.n)]


# ---------------------------------------------------------------- the reference's vectors, as WAL

def _ops(m):
    return [[(o["kind"], o["origin"], o["n"]) for o in m["ops"][b["op_first"]:b["op_first"] + b["n_ops"]]] for b in m["batches"]]


def test_reference_vectors_as_wal():
    """batches.rs:2893-3233, with the LSNs the stream gives: the group counts and the op kinds / counts / origins the tests assert."""
    up, de = (DP.UPSERT, DP.O_NONE), (DP.OP_DELETE, DP.O_DELETE)
    for pat, want in (("II", [[up + (2,)]]), ("IDI", [[up + (1,), de + (1,), up + (1,)]]), ("DD", [[de + (2,)]]),
                      ("UU", [[(DP.OP_DELETE, DP.O_UPDATE, 1), up + (1,)] * 2]), ("D" * 17, [[de + (16,)], [de + (1,)]]),
                      ("IUI", [[up + (1,), (DP.OP_DELETE, DP.O_UPDATE, 1), up + (1,), up + (1,)]])):
        c = _Case([pat])
        m = c.check(_whole(c))
        assert _ops(m) == want, pat
        if pat == "DD":                                                         # :3041-3044, with this table's key values
            assert c.recs["p"][0] == [b'"id" = 0', b'"id" = 1']
        c.close()


def test_reference_retain_vector_as_wal():
    """:3236-3272: three Inserts of three transactions, the watermark the second one's key: one is retained."""
    c = _Case(["I", "I", "I"])
    keys = [(int(c.ev[4][i]), int(c.ev[5][i])) for i in c.members]
    m = c.check(_whole(c), watermark=keys[1])
    assert (m["info"]["n_retained"], m["info"]["n_dropped"]) == (1, 2) and m["batches"][0]["first_event"] == c.members[2]
    c.close()


# ---------------------------------------------------------------- tiles and windows

@pytest.mark.parametrize("tile", [8, 64, 512, 2048])
def test_tiles(tile):
    n = 2100 if EMU else 3000
    c = _Case([_round_robin(n // 2), _round_robin(n - n // 2)], tile=tile)
    assert c.n > 2048 and len(c.members) > 600
    c.check(_whole(c))
    mid = c.members[len(c.members) // 2] + 1                                    # windows that start in the middle of a tile
    t = min(tile, c.n // 4)
    wins = [(3, t + 5), (t + 5, t + 5), (t + 7, mid), (mid + 1, c.n - 2)]
    m = c.check(wins)
    assert any(b["n_members"] < 16 for b in m["batches"])
    assert tile > 64 or any(b["first_event"] // tile != (b["end_event"] - 1) // tile for b in m["batches"])   # a group that straddles tiles
    keys = [(int(c.ev[4][i]), int(c.ev[5][i])) for i in c.members]
    c.check(wins, watermark=keys[40])                                           # the first window's prefix is dropped
    c.close()
    c1 = _Case([_round_robin(n)], tile=tile, slot=1, objects="tp")              # another slot of the same stream
    c1.check([(0, c1.n // 2), (c1.n // 2, c1.n)], use="tp")
    c1.close()


def test_window_shapes():
    c = _Case([_round_robin(150, "IIDIU")])
    ms = c.members
    m = c.check([(0, ms[4] + 1), (ms[4] + 1, c.n)])                             # a window that ends after 5 members
    assert [b["n_members"] for b in m["batches"]][:2] == [5, 16] and m["batches"][1]["window"] == 1
    m = c.check([(i, i + 1) for i in range(c.n)])                               # a cut per event: groups of 1, as many passes as events
    assert m["info"]["n_batches"] == len(ms) and all(b["n_members"] == 1 for b in m["batches"])
    m = c.check([(0, 10), (10, 10), (10, 40), (40, 40), (c.n, c.n)])            # empty windows, one at the very end
    assert {b["window"] for b in m["batches"]} == {0, 2}
    gap = next(i for i in range(c.n - 1) if i not in ms and i + 1 not in ms)   # (Begin and a neighbour of another slot)
    m = c.check([(0, gap), (gap, gap + 2), (gap + 2, c.n)])                     # a window without a member of the slot
    assert {b["window"] for b in m["batches"]} == {0, 2}
    for dev in (False, True):                                                   # n_passes == 0, with and without a pointer
        for passes in (True, False):
            rc, info, bufs = c.raw([], None, "tpu", 4, 4, dev, passes=passes)
            assert rc == abi.OK and info.status == abi.DLP_OK and all(int(getattr(info, k)) == 0 for k in DP.INFO_FIELDS)
            assert all((a == FILL).all() for a in bufs.values())
    m = c.check(_whole(c), skip=("ranges",))                                    # any output may be NULL
    c.check(_whole(c), skip=("batches", "ops"))
    c.check(_whole(c), skip=("ranges", "batches", "ops"))
    c.close()


def test_passes_of_the_outline_call():
    """The passes etlg_batch_outline wrote, handed over as they are."""
    c = _Case([_round_robin(90), _round_robin(60)])
    ol = c.b.outline()
    assert ol.info.status == abi.OL_OK and len(ol.passes) >= 1
    wins = [(int(p[0]), int(p[1])) for p in ol.passes]
    m = c.model(wins)
    got = c.b.ducklake_plan(0, ol.passes, seed=SEED, tuples=c.objs["t"], predicates=c.objs["p"], updates=c.objs["u"])
    assert got.info.status == abi.DLP_OK and int(got.info.n_batches) == m["info"]["n_batches"] == len(got.batches)
    assert [(int(b.first_event), int(b.end_event), int(b.op_first), b.n_ops, list(b.n_cat)) for b in got.batches] == \
        [(b["first_event"], b["end_event"], b["op_first"], b["n_ops"], b["n_cat"]) for b in m["batches"]]
    assert [(o.kind, o.origin, int(o.first_event), int(o.n), int(o.rec_first)) for o in got.ops] == \
        [(o["kind"], o["origin"], o["first_event"], o["n"], o["rec_first"]) for o in m["ops"]]
    assert got.fingerprint_ranges() == [(b["first_event"], b["end_event"], SEED) for b in m["batches"]]
    c.close()


# ---------------------------------------------------------------- the replay filter

def test_watermarks():
    c = _Case([_round_robin(60), _round_robin(75), _round_robin(45)])
    keys = [(int(c.ev[4][i]), int(c.ev[5][i])) for i in c.members]
    assert len({k[0] for k in keys}) == 3
    wins = [(0, c.n // 2), (c.n // 2, c.n)]
    for w in (_whole(c), wins):
        assert c.check(w, watermark=None)["info"]["n_dropped"] == 0
        assert c.check(w, watermark=(keys[0][0] - 1, 1 << 40))["info"]["n_dropped"] == 0                # below every key
        assert c.check(w, watermark=keys[7])["info"]["n_dropped"] == 8                                  # a member's key: it is dropped
        lsn, o = keys[25]
        assert keys[26] == (lsn, o + 3)
        assert c.check(w, watermark=(lsn, o + 1))["info"]["n_dropped"] == 26                            # between two ordinals of a transaction
        assert c.check(w, watermark=(keys[19][0], 1 << 50))["info"]["n_retained"] == sum(1 for k in keys if k[0] > keys[19][0])
        m = c.check(w, watermark=(keys[-1][0], keys[-1][1]))                                            # above every key: no group
        assert m["info"]["n_batches"] == 0 and m["info"]["n_retained"] == 0
        c.check(w, watermark=(keys[-1][0] + 1, 0))
    c.close()


def test_not_prefix():
    """Keys that do not ascend: a second transaction with a lower final LSN. A dropped member behind a retained one of its window."""
    s = W.Stream(lsn=0x1000)
    for final, pat in ((0x9000, "III"), (0x3000, "II")):
        s.add(W.begin(final, ts=1, xid=7))
        for i, k in enumerate(pat):
            s.add(_msg(k, i + final))
        s.add(W.commit(final, final + 8, ts=2, flags=0), lsn=final)
    c = _Case(None, stream=(np.frombuffer(s.bytes(), dtype=np.uint8), s.offsets))
    ms = c.members
    c.status(_whole(c), DP.NOT_PREFIX, watermark=(0x3000, 5), event=ms[3])
    c.check([(0, ms[3]), (ms[3], c.n)], watermark=(0x3000, 5))                  # in a window of its own the dropped run is a prefix
    c.close()


# ---------------------------------------------------------------- op shapes, caps, record positions

@pytest.mark.parametrize("pat,n_ops", [("IDI", [3]), ("UU", [4]), ("IUI", [4]), ("R", [2]), ("P", [1]), ("U" * 16, [32]), ("I" * 40, [1, 1, 1]),
                                       ("IIDDPPRUIDDI" * 4, None)])
def test_op_shapes(pat, n_ops):
    c = _Case([pat])
    m = c.check(_whole(c))
    if n_ops:
        assert [b["n_ops"] for b in m["batches"]] == n_ops
    if pat == "R":
        assert [(o["kind"], o["origin"]) for o in m["ops"]] == [(DP.OP_DELETE, DP.O_REPLACE), (DP.UPSERT, DP.O_NONE)]
    if pat == "P":
        assert [(o["kind"], o["n"], o["rec_first"]) for o in m["ops"]] == [(DP.OP_UPDATE, 1, 0)]
    c.close()


def test_caps():
    c = _Case([_round_robin(300, "IUDIPR")])
    m = c.model(_whole(c))
    nb, no = m["info"]["n_batches"], m["info"]["n_ops"]
    assert nb > 4 and no > nb
    for bcap, ocap in ((0, 0), (1, 1), (nb - 1, no - 1), (3, no + 5), (nb + 5, 2), (nb, 0), (0, no)):
        c.check(_whole(c), bcap=bcap, ocap=ocap)                                # the full counts come back, nothing is written past a cap
    c.close()


def test_record_positions():
    c = _Case([_round_robin(240, "IIUDPRDDIP")])
    for use in ("tpu", "pu", "tu", "tp", ""):
        m = c.check(_whole(c), use=use)
        rc, info, bufs = c.raw(_whole(c), None, use, m["info"]["n_batches"], m["info"]["n_ops"], True)
        c.op_strings(m, bufs, use)
        kinds = {o["kind"]: o["rec_first"] for o in m["ops"]}
        assert all((kinds[k] == DP.NONE) == (o not in use) for k, o in ((DP.UPSERT, "t"), (DP.OP_DELETE, "p"), (DP.OP_UPDATE, "u")))
    wins = [(0, 100), (101, 200), (207, c.n)]
    m = c.check(wins, watermark=(int(c.ev[4][c.members[0]]), int(c.ev[5][c.members[9]])))
    c.op_strings(m, c.raw(wins, (int(c.ev[4][c.members[0]]), int(c.ev[5][c.members[9]])), "tpu", 99, 999, True)[2], "tpu")
    c.close()


# ---------------------------------------------------------------- the other statuses

def test_needs_host():
    """A partial Update without an old image whose identity column is TOAST: the ETLG_DL_UPDATES call left it out (n_host_rows)."""
    c = _Case(["IIPIHIIH"])
    assert int(c.objs["u"].view.n_host_rows) == 2
    ms = c.members
    c.status(_whole(c), DP.NEEDS_HOST, event=ms[4])
    c.status([(ms[5], c.n)], DP.NEEDS_HOST, event=ms[7])
    c.check(_whole(c), use="tp")                                                # a missing object is not an error
    c.check([(0, ms[4]), (ms[5], ms[7])])                                       # ... nor an event outside every window
    c.check(_whole(c), watermark=(int(c.ev[4][ms[7]]), int(c.ev[5][ms[7]])))    # ... nor one the replay filter dropped (no group left)
    c.close()


def test_refused_without_identity():
    """A table put with an empty identity mask: its Updates are refused, before the replay filter and inside a window only. pgoutput
    sends no Delete for such a table, and none without an old image: those two reasons are the model test's."""
    c = _Case(["IIRIR"], ident=[0, 0, 0], objects="t")
    ms = c.members
    c.status(_whole(c), DP.REFUSED, use="t", event=ms[2], reason=DP.R_UPDATE_IDENTITY)
    c.status([(ms[3], c.n)], DP.REFUSED, use="t", event=ms[4], reason=DP.R_UPDATE_IDENTITY)
    c.status(_whole(c), DP.REFUSED, use="t", watermark=(1 << 60, 0), event=ms[2], reason=DP.R_UPDATE_IDENTITY)
    c.check([(0, ms[2]), (ms[2] + 1, ms[4])], use="t")
    c.close()


def test_bad_passes():
    c = _Case([_round_robin(60)])
    c.status([(0, 10), (12, 11), (20, 30)], DP.BAD_PASSES, bad_pass=1)          # first_event > data_end
    c.status([(0, 10), (20, c.n + 1)], DP.BAD_PASSES, bad_pass=1)               # beyond n_events
    c.status([(0, 10), (9, 30), (5, 40)], DP.BAD_PASSES, bad_pass=1)            # starts below its predecessor's end; the lowest index
    c.status([(c.n + 1, c.n + 1)], DP.BAD_PASSES, bad_pass=0)
    c.status([(i, i + 1) for i in range(40)] + [(39, 41)], DP.BAD_PASSES, bad_pass=40)
    c.close()


def test_invalid_arguments():
    c = _Case(["IUD", "II"])
    info = abi.DlPlanInfo()
    pa = np.array([[0, c.n, 0, 0, 0, 0, 0]], dtype=np.uint64)

    def call(batch, slot=0, passes=pa.ctypes.data, n=1, t=None, p=None, u=None, d=None):
        d = d or c.d
        return d.L.etlg_ducklake_plan(d.h, batch.h, slot, passes, n, 0, 0, 0, 0, 0, t, p, u, 0, None, None, 0, None, 0, C.byref(info))

    assert call(c.b) == abi.OK and (info.n_batches, info.n_members) == (1, 5)
    assert call(c.b, slot=7) == abi.InvalidArgument and call(c.b, slot=-1) == abi.InvalidArgument          # an unknown slot
    assert call(c.b, passes=None, n=1) == abi.InvalidArgument                                              # n_passes without passes
    # objects: another slot's, another `what`, on the host
    other = c.b.duckdb(1, NAMES[1], what=abi.DL_TUPLES, on_device=True)
    host = c.b.duckdb(0, NAMES[0], what=abi.DL_TUPLES, on_device=False)
    assert call(c.b, t=other.h) == abi.InvalidArgument and call(c.b, t=host.h) == abi.InvalidArgument
    assert call(c.b, t=c.objs["p"].h) == abi.InvalidArgument and call(c.b, p=c.objs["u"].h) == abi.InvalidArgument
    assert call(c.b, u=c.objs["t"].h) == abi.InvalidArgument
    assert call(c.b, t=c.objs["t"].h, p=c.objs["p"].h, u=c.objs["u"].h) == abi.OK
    # another batch's objects
    buf, offs = _stream(["IUD", "II"])
    b2 = c.d.decode(buf, offs, flags=abi.F_OUTPUT_ON_DEVICE)
    assert call(b2, t=c.objs["t"].h) == abi.InvalidArgument and call(b2) == abi.OK
    b2.close()
    # a batch that is not device-resident
    bh = c.d.decode(buf, offs)
    assert call(bh) == abi.InvalidArgument
    bh.close()
    # a table-copy batch
    rows = b"1\t2\tx\n"
    bc = c.d.copy_decode(0, np.frombuffer(rows, dtype=np.uint8), np.array([0, len(rows)], dtype=np.uint64), flags=abi.F_OUTPUT_ON_DEVICE)
    assert bc.rc == 0, bc.error
    assert call(bc) == abi.InvalidArgument
    bc.close()
    # an ASYNC batch is synced first; one that ended in a decode error gives that error
    ba = c.d.decode(buf, offs, flags=abi.F_OUTPUT_ON_DEVICE | abi.F_ASYNC)
    assert call(ba) == abi.OK and (info.n_batches, info.n_members) == (1, 5)
    ba.close()
    bad = np.frombuffer(bytes(buf[:int(offs[2])]) + b"\xFF" * 24, dtype=np.uint8)
    be = c.d.decode(bad, list(offs[:3]) + [len(bad)], flags=abi.F_OUTPUT_ON_DEVICE | abi.F_ASYNC)
    rc = call(be)
    assert rc not in (abi.OK, abi.InvalidArgument)
    be.close()
    other.close(); host.close()
    c.close()


# ---------------------------------------------------------------- the reason the call exists

def test_ranges_feed_the_fingerprints_call():
    """ranges_out, handed unchanged to etlg_ducklake_fingerprints, gives per group the fingerprint tests/ducklake_identity.py computes
    for that group's members."""
    c = _Case([_round_robin(200, "IIUDPRDDIP"), _round_robin(130, "IPRD")])
    wins = [(0, 77), (77, 140), (150, c.n)]
    wm = (int(c.ev[4][c.members[5]]), int(c.ev[5][c.members[5]]))
    m = c.check(wins, watermark=wm)
    nb = m["info"]["n_batches"]
    rc, info, bufs = c.raw(wins, wm, "tpu", nb, 0, False)
    assert rc == abi.OK and int(info.n_batches) == nb > 5
    ranges = (abi.DlRange * nb).from_buffer_copy(bufs["ranges"][:3 * nb].tobytes())
    out = np.zeros(nb, dtype=np.uint64)
    fi = abi.DlFpInfo()
    blob = b"".join(n.encode() + b"\0" for n in c.names)
    rc = c.d.L.etlg_ducklake_fingerprints(c.d.h, c.b.h, 0, c.objs["t"].h, c.objs["p"].h, c.objs["u"].h, blob, len(c.names), C.addressof(ranges), nb,
                                          out.ctypes.data, C.byref(fi))
    assert rc == abi.OK and fi.status == abi.RB_OK
    streams = ID.batch_streams(c.events, 0, c.names, c.ident)
    want = [ID.fnv1a(b"".join(streams[i] for i in b["members"]), SEED) for b in m["batches"]]
    assert [int(x) for x in out] == want
    assert len(set(want)) == nb
    c.close()
