"""etlg_batch_outline (etl_amd/csrc/finish.hip: k_ol_*) against tests/batch_outline.py, the sequential restatement of the sinks'
write_events loop (clickhouse/core.rs:1063-1164; iceberg/core.rs:300-432 with relations_inline). Every case compares every field the call
writes with the model, exactly: the info, the passes, ends_out, the touched bits, the truncate entries and the census. Every output
buffer is one word longer than its cap and filled with a pattern first: what lies at or beyond a count or a cap, and the word behind,
must still hold it. Each case runs with host cuts and host outputs and again with device cuts and device outputs; the two give the same
bytes. The reference's tests state no pass boundary as a number, so nothing here is pinned to a vector of its own.
The kernels' constants: waves of 64, workgroups of 256, the tile (2 048 events, or ETLG_OL_TILE in a context of its own: 128 here, 8
under the SIMT emulator) and the chunks of 256 tile sums k_ol_scan walks; 64 entries of the census' LDS table; 16 touched words of a
continued pass gathered in LDS. A small tile crosses the scan's levels but is a single chunk of 256 lanes: BIG_TILES (512 .. 2 048, the
default) run the chunk loops of k_ol_tiles and k_ol_write, their carries from chunk to chunk and the slot table that lives across them."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

from etl_amd import abi, synth
from tests import batch_cuts as BC
from tests import batch_outline as BO
from tests import pgwire as W
from tests import scenarios as SC

pytestmark = pytest.mark.gpu
EMU = os.environ.get("ETLG_SIMT_RUN") == "1"
TILE = 8 if EMU else 128
TILE_SIZES = [TILE - 1, TILE, TILE + 1, TILE * TILE - 1, TILE * TILE, TILE * TILE + 1, 3 * TILE * TILE + 5]
FILL = 0xEEEEEEEEEEEEEEEE
BIG_TILES = [512, 1024, 2048]
N = W.NULL


# ---------------------------------------------------------------- device memory of the test's own

def _dev_put(a):
    """np.uint64 array -> (owner, address) of a copy in device memory (the emulator's device memory is host memory)."""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if EMU:
        own = a.copy() if len(a) else np.zeros(1, dtype=np.uint64)
        return own, own.ctypes.data
    import torch
    own = torch.from_numpy((a if len(a) else np.zeros(1, dtype=np.uint64)).view(np.int64)).cuda()
    torch.cuda.synchronize()
    return own, own.data_ptr()


def _dev_get(ptr, n):
    if not n:
        return np.zeros(0, dtype=np.uint64)
    if EMU:
        return np.frombuffer((C.c_uint8 * (8 * n)).from_address(ptr), dtype=np.uint64).copy()
    return abi.device_tensor(ptr, 8 * n, 0).cpu().numpy().view(np.uint64)


# ---------------------------------------------------------------- one decoded batch, its model, and the raw call

OUTPUTS = ("passes", "ends", "touched", "truncates", "slots")


class _Case:
    def __init__(self, prime, buf, offs, tile=TILE):
        from etl_amd.decoder import Decoder
        from oracle import oracle
        before = os.environ.get("ETLG_OL_TILE")
        os.environ["ETLG_OL_TILE"] = str(tile)                              # read when the context is created
        try:
            self.d = Decoder(0)
        finally:
            os.environ.pop("ETLG_OL_TILE", None)
            if before is not None:
                os.environ["ETLG_OL_TILE"] = before
        prime(self.d)
        self.b = self.d.decode(buf, offs, flags=abi.F_OUTPUT_ON_DEVICE)
        assert self.b.rc == 0, self.b.error
        o = oracle.Oracle()
        prime(o)
        rb = o.decode(buf, offs)
        assert rb.err_code == 0, rb.err_desc
        self.hb = rb.host_batch()
        self.ev = BO.of_host_batch(self.hb)
        self.kinds, self.n = self.ev[0], len(self.ev[0])
        v = self.b.view()
        assert int(v.n_events) == self.n
        self.ns = int(v.n_slots)
        self.W = (self.ns + 63) // 64

    def model(self, cuts=(), first=0, end=None, inline=False):
        return BO.outline(*self.ev, first=first, end=end, cuts=[int(c) for c in cuts], relations_inline=inline)

    def raw(self, cuts, first, end, inline, pcap, tcap, dev, skip=()):
        """One call with pattern-filled buffers of pcap / tcap entries and a guard word each -> (rc, info, {name: every word of its buffer}).
        dev: the cuts and the outputs are device memory. skip: outputs passed as NULL."""
        words = {"passes": 7 * pcap, "ends": pcap, "touched": self.W * pcap, "truncates": 2 * tcap, "slots": 12 * self.ns}
        cuts = np.ascontiguousarray(cuts, dtype=np.uint64)
        bufs = {k: np.full(words[k] + 1, FILL, dtype=np.uint64) for k in OUTPUTS if k not in skip}
        owners = {}
        if dev:
            owners = {k: _dev_put(a) for k, a in bufs.items()}
            owners["cuts"] = _dev_put(cuts)
        ptr = lambda k: None if k in skip else (owners[k][1] if dev else bufs[k].ctypes.data)
        cptr = None if not len(cuts) else (owners["cuts"][1] if dev else cuts.ctypes.data)
        info = abi.OutlineInfo()
        rc = self.d.L.etlg_batch_outline(self.d.h, self.b.h, first, self.n if end is None else end, cptr, len(cuts), 1 if dev else 0,
                                         abi.OL_RELATIONS_INLINE if inline else 0, abi.F_OUTPUT_ON_DEVICE if dev else 0,
                                         ptr("passes"), ptr("ends"), ptr("touched"), pcap, ptr("truncates"), tcap, ptr("slots"), C.byref(info))
        if dev:
            bufs = {k: _dev_get(owners[k][1], words[k] + 1) for k in bufs}
        return rc, info, bufs

    def check(self, cuts=(), first=0, end=None, inline=False, pcap=None, tcap=None, skip=()):
        """Host and device memory against the model, field by field; returns the model."""
        m = self.model(cuts, first, end, inline)
        assert m["status"] == BO.OK
        pcap = m["info"]["n_passes"] if pcap is None else pcap
        tcap = m["info"]["n_trunc"] if tcap is None else tcap
        got = {}
        for dev in (False, True):
            rc, info, bufs = self.raw(cuts, first, end, inline, pcap, tcap, dev, skip)
            assert rc == abi.OK and info.status == abi.OL_OK, (rc, info.status, info.bad_cut)
            gi = {k: int(getattr(info, k)) for k in BO.INFO_FIELDS}
            assert gi == m["info"], (dev, gi, m["info"])
            self.compare(m, bufs, pcap, tcap, dev)
            got[dev] = bufs
        for k in got[False]:
            assert np.array_equal(got[False][k], got[True][k]), k            # host and device output pointers: the same bytes
        return m

    def compare(self, m, bufs, pcap, tcap, dev):
        P, K, Wd = min(pcap, len(m["passes"])), min(tcap, len(m["truncates"])), self.W
        if "passes" in bufs:
            want = np.array([[p[f] for f in BO.PASS_FIELDS] for p in m["passes"][:P]], dtype=np.uint64).reshape(P, 7)
            got = bufs["passes"][:7 * P].reshape(P, 7)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert not len(bad), (dev, int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())
            assert (bufs["passes"][7 * P:] == FILL).all(), dev
        if "ends" in bufs:
            assert bufs["ends"][:P].tolist() == [p["end_event"] for p in m["passes"][:P]], dev
            assert (bufs["ends"][P:] == FILL).all(), dev
        if "touched" in bufs:
            want = np.zeros((P, Wd), dtype=np.uint64)
            for p, slots in enumerate(m["touched"][:P]):
                for s in slots:
                    want[p, s // 64] |= np.uint64(1 << (s % 64))
            got = bufs["touched"][:Wd * P].reshape(P, Wd)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert not len(bad), (dev, int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())
            assert (bufs["touched"][Wd * P:] == FILL).all(), dev
        if "truncates" in bufs:
            want = np.array([[t | (s << 32), e] for t, s, e in m["truncates"][:K]], dtype=np.uint64).reshape(K, 2)
            assert np.array_equal(bufs["truncates"][:2 * K].reshape(K, 2), want), dev
            assert (bufs["truncates"][2 * K:] == FILL).all(), dev
        if "slots" in bufs:
            want = np.zeros((self.ns, 2, 6), dtype=np.uint64)
            want[:, 1, :] = np.uint64(BO.NONE)
            for s, (rows, first) in m["census"].items():
                want[s, 0], want[s, 1] = rows, first
            got = bufs["slots"][:12 * self.ns].reshape(self.ns, 2, 6)
            bad = np.flatnonzero((got != want).any(axis=(1, 2)))
            assert not len(bad), (dev, int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())
            assert bufs["slots"][-1] == FILL, dev

    def close(self):
        self.b.close(); self.d.close()


def _stream(msgs):
    s = SC.txn(msgs)
    return np.frombuffer(s.bytes(), dtype=np.uint8), s.offsets


COLS = [("id", SC.INT8, False, 1), ("v", SC.TEXT, True, 0)]
REL = [(1, "id", SC.INT8, -1), (0, "v", SC.TEXT, -1)]
MSG = {"D": lambda i: W.insert(42, [str(i), "v%d" % i]), "R": lambda i: W.relation(42, "public", "t", "d", REL), "T": lambda i: W.truncate([42], 0)}


def _pattern_case(pattern, tile=TILE):
    """One transaction whose events are B, then one per letter of `pattern` (D an Insert, R a Relation, T a Truncate of the table), then C."""
    c = _Case(SC.simple_table(COLS), *_stream([MSG[k](i) for i, k in enumerate(pattern)]), tile=tile)
    assert c.kinds == "B" + pattern.replace("D", "I") + "C", (c.kinds[:40], pattern[:40])
    return c


# ---------------------------------------------------------------- event-count seams, cuts left on the device by etlg_batch_cuts

_CFG2 = {}


def _cfg2(n):
    """The first n events of one cfg2 stream (every frame of it is one event)."""
    if not _CFG2:
        top = max(TILE_SIZES) + 2
        w = synth.cfg2()
        buf, offs = w.fill(top * 128 + (256 << 10))                         # (whole transactions of 1 000 rows)
        assert len(offs) - 1 >= top
        _CFG2.update(w=w, buf=buf, offs=offs)
    g = _CFG2
    return _Case(g["w"].register, g["buf"][:g["offs"][n]], g["offs"][:n + 1])


@pytest.mark.parametrize("n", TILE_SIZES)
def test_plain_transactions_across_every_level_of_the_scan(n):
    c = _cfg2(n)
    sm = BC.size_model()
    total = int(c.b.cuts(sm, 1 << 62, cap=0)[1].total)
    for budget in (1, max(1, total // 7), total + 1):
        own, ptr = _dev_put(np.full(n, FILL, dtype=np.uint64))
        _, ci = c.b.cuts(sm, budget, cap=n, on_device=ptr)                  # the cuts stay on the device
        k = int(ci.n_cuts)
        assert int(ci.stop_event) == n and k == (n if budget == 1 else 0 if budget > total else k)
        cuts = _dev_get(ptr, k)
        m = c.model(cuts)
        o = c.b.outline(cuts=ptr, n_cuts=k)                                 # device cuts, host outputs, counted and then filled
        assert {f: int(getattr(o.info, f)) for f in BO.INFO_FIELDS} == m["info"]
        assert o.passes.tolist() == [[p[f] for f in BO.PASS_FIELDS] for p in m["passes"]]
        assert o.ends.tolist() == [p["end_event"] for p in m["passes"]]
        assert [o.touched_slots(p) for p in range(len(o.passes))] == [sorted(t) for t in m["touched"]]
        assert o.slots[0, 0, 0] == m["info"]["n_rows"] and o.slots[0, 1, 0] == m["census"][0][1][0]
        assert m["info"]["n_ranges"] == (k if k and cuts[-1] == n else k + 1)
        if budget != 1 or n <= TILE * TILE + 1:
            c.check(cuts)                                                   # pattern-filled buffers, host and device
        del own
    c.close()


# ---------------------------------------------------------------- the 27 patterns, class changes on every seam

ALL27 = "".join("".join(p) for p in itertools.product("DRT", repeat=3))


def _padded():
    """Runs of one class, each change placed on the last lane of a wave, of a workgroup and of a tile and on the first lane of the next."""
    seams = [(64, 63), (64, 0), (TILE, TILE - 1), (TILE, 0)] + ([] if EMU else [(256, 255), (256, 0)])
    out = "D"
    for a, b in itertools.permutations("DRT", 2):
        for mod, at in seams:
            out += a
            while (len(out) + 1) % mod != at:                               # (event 0 is the Begin: letter k is event k + 1)
                out += a
            out += b
    return out


@pytest.mark.parametrize("inline", [False, True])
@pytest.mark.parametrize("name", ["concatenated", "padded"])
def test_the_27_patterns_and_class_changes_on_every_seam(name, inline):
    pattern = ALL27 if name == "concatenated" else _padded()
    c = _pattern_case(pattern)
    m = c.check(inline=inline)
    if name == "padded":
        change = [i for i in range(1, c.n) if BO_class(c.kinds[i], inline) != BO_class(c.kinds[i - 1], inline)]
        for mod, at in ((64, 63), (64, 0), (TILE, TILE - 1), (TILE, 0)):
            assert sum(i % mod == at for i in change) >= (2 if inline else 6), (mod, at)
    assert m["info"]["n_passes"] > (8 if inline else 12)
    c.check(inline=inline, cuts=[c.n // 3, c.n // 2])
    c.close()


@pytest.mark.parametrize("tile", BIG_TILES)
def test_the_patterns_in_tiles_of_several_chunks(tile):
    c = _pattern_case((ALL27 + _padded()[:300]) * 7, tile=tile)             # more than one tile of 2 048, every chunk with passes of its own
    assert c.n > 2048 + 256
    for inline in (False, True):
        m = c.check(inline=inline)
        assert m["info"]["n_passes"] > 80
        c.check(inline=inline, cuts=[255, 256, 257, 1000, c.n - 1], pcap=m["info"]["n_passes"] // 2, tcap=5)
    c.close()


def BO_class(kind, inline):
    return 2 if kind == "T" else 1 if kind == "R" and not inline else 0


# ---------------------------------------------------------------- as many passes as events; the caps

def test_alternating_truncate_and_insert_and_half_the_passes():
    c = _pattern_case("TD" * (3 * TILE // 2))
    m = c.check()
    assert m["info"]["n_passes"] == 3 * TILE // 2 + 1 and m["info"]["n_trunc"] == 3 * TILE // 2
    m = c.check(cuts=list(range(1, c.n + 1)))                               # and a range per event: a pass per event
    assert m["info"]["n_passes"] == c.n
    half = m["info"]["n_passes"] // 2
    for pcap, tcap in ((half, None), (half, m["info"]["n_trunc"] // 2), (1, 1), (0, 0), (c.n + 7, c.n + 7)):
        c.check(pcap=pcap, tcap=tcap)
        c.check(cuts=list(range(1, c.n + 1)), pcap=pcap, tcap=tcap)
    c.check(pcap=half, skip=("passes",))                                    # any output may be NULL
    c.check(pcap=half, skip=("ends", "touched", "truncates", "slots"))
    c.check(skip=OUTPUTS)
    c.close()


# ---------------------------------------------------------------- ranges

def test_ranges():
    #           1         2         3
    # 0123456789012345678901234567890123
    # BDDRRRTTTDDRRTTDTRDDDRRRRTTTTDDDDC
    c = _pattern_case("DDRRRTTTDDRRTTDTRDDDRRRRTTTTDDDD")
    n = c.n
    change = [i for i in range(1, n) if BO_class(c.kinds[i], False) != BO_class(c.kinds[i - 1], False)]
    for inline in (False, True):
        c.check(cuts=change, inline=inline)                                 # a cut on every class change
        c.check(cuts=[4, 7, 23, 27], inline=inline)                         # in the middle of an R run and of a T run
        c.check(cuts=[0, 0, 4, 4, 4, 7, n, n], inline=inline)               # a cut equal to first, duplicates, a cut equal to end
        c.check(cuts=[n], inline=inline)
        c.check(cuts=[9, 12, 20], first=9, end=29, inline=inline)           # the window's first event follows a T; its first cut is `first`
        c.check(cuts=[18], first=7, end=n - 1, inline=inline)               # the window starts inside a T run
        c.check(first=16, end=17, inline=inline)
    m = c.check(cuts=[0, 0, 4, 4, 4, 7, n, n])
    assert m["info"]["n_ranges"] == 8 and sorted({p["range"] for p in m["passes"]}) == [2, 5, 6]
    c.close()


def test_an_empty_window():
    c = _pattern_case("DTRD")
    for first in (0, 2, c.n):
        m = c.check(first=first, end=first)
        assert m["info"] == {"n_passes": 0, "n_trunc": 0, "n_relations": 0, "n_rows": 0, "n_ranges": 1}
        assert c.check(first=first, end=first, cuts=[first, first], pcap=3, tcap=3)["info"]["n_ranges"] == 2
    c.close()


@pytest.mark.parametrize("dev", [False, True])
def test_bad_cuts_leave_every_output_as_it_was(dev):
    c = _pattern_case("DDTDDRDDTD" * 4)
    n = c.n
    for cuts, first, end, bad in (([3, 9, 8, 20], 0, n, 2), ([3, 9, 20], 4, n, 0), ([3, 9, n - 1], 0, n - 2, 2), ([n + 1], 0, n, 0), ([5, 4, 3], 0, n, 1),
                                  ([7], 7, 7, None), ([8], 7, 7, 0), ([6], 7, 7, 0)):
        m = c.model(cuts, first, end)
        assert (m["status"], m.get("bad_cut")) == ((BO.BAD_CUTS, bad) if bad is not None else (BO.OK, None))
        rc, info, bufs = c.raw(cuts, first, end, False, n, n, dev)
        assert rc == abi.OK
        if bad is None:
            assert info.status == abi.OL_OK
            continue
        assert info.status == abi.OL_BAD_CUTS and int(info.bad_cut) == bad
        assert [int(getattr(info, f)) for f in BO.INFO_FIELDS] == [0] * 5
        for k, a in bufs.items():
            assert (a == FILL).all(), (k, cuts)
    c.close()


# ---------------------------------------------------------------- truncates

def _three_tables(t):
    for tid in (42, 43, 44):
        SC.simple_table(COLS, table_id=tid)(t)


def test_truncate_entries():
    ins = lambda tid, i: W.insert(tid, [str(i), "x"])
    msgs = [ins(42, 1), W.truncate([42, 43, 44], 0), ins(43, 2),
            W.truncate([4242], 0),                                          # a table the worker does not own: no entry
            ins(44, 3), W.truncate([43, 42], 1), W.truncate([42], 0), W.truncate([44, 42, 4242], 0),   # the same table twice in a pass, and more
            ins(42, 4), W.truncate([42], 0), ins(42, 5)]                    # and again in the next pass
    c = _Case(_three_tables, *_stream(msgs))
    m = c.check()
    assert c.kinds == "BITIITTTITIC"                                        # (the Truncate of a foreign table alone yields no event)
    assert m["info"]["n_trunc"] == 9 and [p["n_trunc"] for p in m["passes"]] == [3, 5, 1, 0]
    assert [(t, e) for t, _, e in m["truncates"][3:8]] == [(43, 5), (42, 5), (42, 6), (44, 7), (42, 7)]    # 4242 of event 7 has no entry
    assert [t for t, _, _ in BO.truncated_tables(m, 1)] == [43, 42, 44]
    o = c.b.outline()
    for p in range(len(m["passes"])):
        assert o.truncated_tables(p) == BO.truncated_tables(m, p)           # the wrapper keeps the first entry per table
    for tcap in (0, 1, 3, 4, 9):
        c.check(tcap=tcap)
        c.check(tcap=tcap, inline=True, cuts=[3, 8])
    c.close()


# ---------------------------------------------------------------- census and bitmap

@pytest.mark.parametrize("tile", [TILE] + BIG_TILES)
def test_three_tables_round_robin(tile):
    msgs = []
    for i in range(3 * TILE + 5 if tile == TILE else 2048 + 700):
        msgs.append(W.insert(42 + i % 3, [str(i), "r%d" % i]))
        if i % 50 == 17:
            msgs.append(W.truncate([43], 0))
        if i % 70 == 33:
            msgs.append(W.relation(44, "public", "t", "d", REL))
    c = _Case(_three_tables, *_stream(msgs), tile=tile)
    m = c.check()
    # (a Relation message opens a new slot for its table: the longer stream has more than three)
    assert set(m["census"]) >= {0, 1, 2} and max(len(t) for t in m["touched"]) >= 3 and m["info"]["n_passes"] >= 2
    c.check(inline=True, cuts=[c.n // 4, c.n // 2])
    c.close()


ONE = [("id", SC.INT8, False, 1)]


def _tables(n):
    def prime(t):
        for k in range(n):
            SC.simple_table(ONE, table_id=100 + k)(t)
    return prime


@pytest.mark.parametrize("tile", [TILE, 256] + BIG_TILES)
def test_seventy_tables_two_touched_words_and_a_full_lds_table(tile):
    prime = _tables(70)
    msgs = []
    for r in range(4):
        msgs += [W.insert(100 + (k * 37 + r) % 70, [str(r * 70 + k)]) for k in range(70)]   # every tile of 128 meets more than 64 slots
        msgs.append(W.truncate([100 + r, 169 - r], 0))
    msgs += [W.insert(169, ["7"]), W.insert(100, ["8"]), W.insert(164, ["9"])]
    c = _Case(prime, *_stream(msgs), tile=tile)
    assert c.ns == 70 and c.W == 2
    m = c.check()
    assert len(m["census"]) == 70 and [len(t) for t in m["touched"]] == [70, 70, 70, 70, 3]
    c.check(cuts=[40, 100, 111], pcap=3)
    c.close()


@pytest.mark.parametrize("tile", [TILE, 256] + BIG_TILES)
def test_colliding_slots_arrive_in_later_chunks_of_a_tile(tile):
    """Slots 64 .. 69 share their home in the LDS table with slots 0 .. 5. A tile that has counted the larger slot in one chunk of 256 lanes
    and meets the smaller one in a later chunk must keep the two apart (tile 1 024: 255 Inserts of slot 64, then 100 of slot 0, gave slot 0
    all 355 when a claim could move a key that had been counted)."""
    msgs, i = [], 0
    for hi, lo, a, b in ((64, 0, 255, 100), (69, 5, 300, 300), (65, 1, 100, 600), (68, 4, 257, 1), (66, 2, 64, 64), (67, 3, 1, 511)):
        msgs += [W.insert(100 + hi, [str(i + k)]) for k in range(a)] + [W.insert(100 + lo, [str(i + a + k)]) for k in range(b)]
        i += a + b
    for r in range(3):                                                      # then every slot, descending: each arrival is smaller than all that are placed
        msgs += [W.insert(100 + s, [str(i + 70 * r + s)]) for s in range(69, -1, -1)]
    c = _Case(_tables(70), *_stream(msgs), tile=tile)
    m = c.check()
    assert m["census"][64][0][0] == 255 + 3 and m["census"][0] == ([100 + 3, 0, 0, 0, 0, 0], [256] + [BO.NONE] * 5)
    assert m["census"][64][1][0] == 1 and m["census"][67][0][0] == 1 + 3 and m["census"][3][0][0] == 511 + 3
    c.check(first=200, end=c.n - 100, cuts=[256, 1024, 2048])
    c.close()


@pytest.mark.parametrize("tile", [TILE, 512])
def test_more_slots_than_the_touched_words_gathered_in_lds(tile):
    """1 100 slots: 18 touched words per pass, two of them behind the 16 a tile gathers in LDS for the pass it continues."""
    msgs = [W.insert(100 + (k * 7) % 1100, [str(k)]) for k in range(1100)]  # one pass over every slot, continued from tile to tile
    msgs += [W.truncate([100, 1199], 0)] + [W.insert(100 + s, ["1"]) for s in (1099, 1024, 1023, 0, 1087)] + [W.truncate([1123], 0)]
    msgs += [W.insert(100 + s, [str(s)]) for s in range(1099, 900, -1)]
    c = _Case(_tables(1100), *_stream(msgs), tile=tile)
    assert c.ns == 1100 and c.W == 18
    m = c.check()
    assert [len(t) for t in m["touched"]] == [1100, 5, 199] and len(m["census"]) == 1100
    c.check(cuts=[300, 1200], pcap=2)
    c.close()


def test_every_category_the_streams_can_produce():
    cols = [("id", SC.INT8, False, 1), ("a", SC.TEXT, True, 0), ("k", SC.TEXT, False, 1)]
    r = ["1", "alice", "key"]
    msgs = [W.insert(42, r), W.update(42, ["1", "bob", "key"]), W.update(42, ["1", "bob", "key2"], key=["1", N, "key"]),
            W.update(42, ["1", "carol", "key2"], old=r),
            W.update(42, ["1", W.TOAST, "key2"]),                           # an unchanged toast column and no old image: a partial Update
            W.delete(42, key=["1", N, "key2"]), W.delete(42, old=r), W.truncate([42], 0)] * 5
    c = _Case(SC.simple_table(cols), *_stream(msgs))
    m = c.check()
    rows, first = m["census"][0]
    assert rows == [5, 15, 5, 5, 5, 0] and first == [1, 2, 5, 7, 6, BO.NONE]      # (pgoutput has no Delete without an old image)
    c.check(first=6, end=c.n - 3, cuts=[20])
    c.close()


# ---------------------------------------------------------------- composition with the hand-offs

def test_pass_ends_locate_the_rows_of_every_hand_off():
    msgs = []
    for i in range(2 * TILE + 9):
        msgs.append(W.insert(42 + (i * i) % 3, [str(i), "r%d" % i]))
        if i % 23 == 11:
            msgs.append(W.truncate([42], 0))
        if i % 31 == 30:
            msgs += [W.truncate([44], 0), W.truncate([43], 0)]
    c = _Case(_three_tables, *_stream(msgs))
    m = c.model()
    P = m["info"]["n_passes"]
    bufs = {k: _dev_put(np.full(w + 1, FILL, dtype=np.uint64)) for k, w in (("ends", P), ("touched", P * c.W))}
    o = c.b.outline(passes_cap=P, trunc_cap=0, on_device={k: v[1] for k, v in bufs.items()})
    assert int(o.info.n_passes) == P
    touched = _dev_get(o.touched, P * c.W).reshape(P, c.W)
    for slot in (0, 2):
        rb = c.b.rowbinary(slot, np.ones(len(COLS) + 2, dtype=np.uint8), on_device=True)
        row_event = _dev_get(rb.view.row_event, rb.n_rows)
        pos = c.b.locate(o.ends, rb.view.row_event, rb.n_rows, n_cuts=P)    # ends_out stays on the device
        lo = 0
        for p in range(P):
            hi = int(pos[p])
            assert row_event[lo:hi].tolist() == m["rows"][p].get(slot, []), (slot, p)
            assert (hi > lo) == bool((int(touched[p, slot // 64]) >> (slot % 64)) & 1), (slot, p)
            lo = hi
        assert lo == rb.n_rows
        rb.close()
    del bufs
    c.close()


# ---------------------------------------------------------------- arguments

def test_invalid_arguments():
    from etl_amd.decoder import Decoder, EtlError
    c = _pattern_case("DTD")
    for kw in (dict(first=3, end=2), dict(end=c.n + 1), dict(first=c.n + 1, end=c.n + 1)):
        with pytest.raises(EtlError) as e:
            c.b.outline(**kw)
        assert e.value.kind == abi.InvalidArgument, kw
    c.b.host()                                                              # etlg_batch_download: the arena leaves the device
    with pytest.raises(EtlError) as e:
        c.b.outline()
    assert e.value.kind == abi.InvalidArgument and "etlg_batch_outline" in e.value.description
    c.close()
    d = Decoder(0)                                                          # a host-resident batch
    SC.simple_table(COLS)(d)
    b = d.decode(*_stream([MSG["D"](1)]))
    assert b.rc == 0
    with pytest.raises(EtlError) as e:
        b.outline()
    assert e.value.kind == abi.InvalidArgument
    b.close()
    rows = [("%d\tx\n" % i).encode() for i in range(20)]                    # a table-copy batch has no passes
    slot = d.table_ready(42, 0, [1, 1], [1, 0])
    b = d.copy_decode(slot, np.frombuffer(b"".join(rows), dtype=np.uint8), np.cumsum([0] + [len(r) for r in rows]).astype(np.uint32), flags=abi.F_OUTPUT_ON_DEVICE)
    assert b.rc == 0, b.error
    with pytest.raises(EtlError) as e:
        b.outline()
    assert e.value.kind == abi.InvalidArgument and "table-copy" in e.value.description
    b.close(); d.close()
