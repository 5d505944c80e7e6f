"""The prologue of the fixed-width decode kernels (etl_amd/csrc/plan.hip, plan_kernel) against the oracle, through the C ABI.

A wave of k_plan / k_plan2 issues every load in front of its staging at once — the tile's span and the lane's offset (both tiles' of a
two-tile wave), the pre-pass's prefix words, the carry block of a batch chained on the same stream — and decides afterwards what hangs
on them. The shapes here are the ones at which that order can go wrong: batches that end inside a tile or one frame into it, a
pre-pass group in front of a single-frame tile, an input whose last 16-byte piece is partial, chains whose first tile needs the carried
transaction state (read late from the other stream, or up front on the same one), a grid sized by a bound, the debug instantiation.
Every case under the default settings (k_plan behind k_plan_pre) and under ETLG_PLAN_PRE=0 (k_plan2 with its own look-back); every
batch: all arrays of batch.host() and the counts against the oracle's.

The chain with a malformed integer: the plan gives such a batch up with DevResult.fused_fail bit 1 alone, which load_carry
(frames.hip.h) deliberately does not take for a reason to stop its successors — they run on the state the plan published and are
decoded again by the host when the second attempt at the batch ends in its error. So a successor HAS written an arena on its first
attempt, in the parent of this change as well; what holds, and is asserted, is the oracle's report for every batch after the second
attempts and that the chain was run again."""
import os

import numpy as np
import pytest

from etl_amd import abi, synth

pytestmark = pytest.mark.gpu

_KNOBS = ("ETLG_FUSED_KERNEL", "ETLG_FORCE_MULTIPASS", "ETLG_PLAN", "ETLG_PLAN_DBG", "ETLG_PLAN_PRE", "ETLG_OVERLAP")
FLAGS = abi.F_INPUT_ON_DEVICE | abi.F_OUTPUT_ON_DEVICE | abi.F_NO_CONTROL | abi.F_ASYNC


@pytest.fixture(params=["pre_pass", "look_back"])
def mode(request):
    """The knobs are read when a context is created: set around the whole test."""
    saved = {k: os.environ.pop(k, None) for k in _KNOBS}
    if request.param == "look_back":
        os.environ["ETLG_PLAN_PRE"] = "0"
    yield request.param
    for k in _KNOBS:
        os.environ.pop(k, None)
        if saved[k] is not None:
            os.environ[k] = saved[k]


@pytest.fixture(scope="module")
def stream():
    """One cfg2 stream (Begin, 1000 Inserts, Commit, ...), shared and left unchanged: its first n frames are the n-frame batches."""
    buf, offs = synth.cfg2().fill(600 << 10)
    assert len(offs) - 1 > 4097
    buf.setflags(write=False)
    offs.setflags(write=False)
    return buf, offs


def _head(stream, n):
    buf, offs = stream
    return buf[:int(offs[n])].copy(), offs[:n + 1].copy()


def _pair(w):
    from etl_amd.decoder import Decoder
    from oracle import oracle
    d, o = Decoder(0), oracle.Oracle()
    w.register(d, ready=True)
    w.register(o, ready=True)
    return d, o


def _agree(gb, rb, what=""):
    e = gb.error
    got = (e.code, e.kind, e.description, e.frame_index) if e else (0, 0, "", -1)
    assert (rb.err_code, rb.err_kind, rb.err_desc, rb.err_frame) == got, (what, got)
    diff = rb.host_batch().diff(gb.host())   # the counts (events, frames, payload bytes, arena sizes) and all ten arrays
    assert not diff, (what, diff[:4])


@pytest.mark.parametrize("nframes", [1, 63, 64, 65, 128, 4096, 4097])
def test_batches_that_end_at_in_and_just_behind_a_tile(nframes, mode, stream):
    """1 .. 4 097 frames: a tile of one frame, a tile short of one, full tiles, one frame into the next tile (the second tile of a
    two-tile wave; alone in its wave behind two full ones), and one full pre-pass group of 64 tiles in front of a single-frame tile."""
    buf, offs = _head(stream, nframes)
    d, o = _pair(synth.cfg2())
    _agree(d.decode(buf, offs), o.decode(buf, offs), nframes)
    paths = d.debug_paths()
    assert paths["plan"] == 1 and paths["plan_redone"] == 0 and paths["redone"] == 0, paths
    d.close()


def _stream_of_65(want_multiple_of_16):
    """A Begin and 64 Inserts into cfg2's table. With ten digits in every cell — cfg2's own frames — the batch is 51 + 64 x 113 = 7 283
    bytes, three more than a multiple of 16; three cells of nine digits make it 7 280."""
    from tests import pgwire as W
    rel = synth.table_fixed()["rel_id"]
    frames = [W.frame(W.xlog(0x3000000, W.begin(0x3000F00, 1, 77)))]
    for i in range(64):
        vals = [str(10 ** 9 + 5 * i + c) for c in range(5)]
        if want_multiple_of_16 and i < 3:
            vals[0] = str(10 ** 8 + i)
        frames.append(W.frame(W.xlog(0x3000000 + 16 * (i + 1), W.insert(rel, vals))))
    buf = np.frombuffer(b"".join(frames), dtype=np.uint8).copy()
    offs = np.cumsum([0] + [len(f) for f in frames]).astype(np.uint32)
    return synth.cfg2(), buf, offs


@pytest.mark.parametrize("whole_pieces", [True, False])
def test_last_piece_of_the_input(whole_pieces, mode):
    """The 65-frame batch once with a length that is a multiple of 16 (every staging piece is whole) and once cut so that the last
    16-byte piece of the second tile crosses the end of the input (moved bytewise by the first lanes)."""
    w, buf, offs = _stream_of_65(whole_pieces)
    assert (len(buf) % 16 == 0) == whole_pieces and len(offs) == 66
    w.reset()
    d, o = _pair(w)
    _agree(d.decode(buf, offs), o.decode(buf, offs))
    assert d.debug_paths()["plan"] == 1 and d.debug_paths()["plan_redone"] == 0
    d.close()


def _chain_pieces():
    """Six batches of 65 frames over transactions of 66 (Begin, 64 Inserts, Commit): every transaction opens in batch k and commits in
    batch k + 1, so the first tile of every batch but the first starts inside one and needs in_txn / final_lsn / next_ord carried in."""
    w = synth.Workload([synth.table_fixed()], 0xE71C4A1, rows_per_txn=64, name="chain_of_65")
    buf, offs = w.fill(64 << 10)
    assert len(offs) - 1 >= 390
    pieces = []
    for k in range(6):
        o = offs[65 * k:65 * (k + 1) + 1].astype(np.int64)
        pieces.append((buf[int(o[0]):int(o[-1])].copy(), (o - o[0]).astype(np.uint32)))
        tags = [int(pieces[-1][0][int(x) + 30]) for x in pieces[-1][1][:-1]]
        assert (tags[0] == ord("B")) == (k == 0) and tags.count(ord("B")) == 1 and (tags.count(ord("C")) == 1) == (k > 0), (k, tags)
    w.reset()
    return w, pieces


def _run_chain(w, pieces):
    """The whole chain enqueued before anything is synced; then every batch against the oracle. Returns the path counters."""
    from tests.test_gpu_async import DevBufs
    d, o = _pair(w)
    dev = DevBufs(pieces)
    inflight = [d.decode_device(p, n, po, nf, FLAGS) for (p, n, po, nf) in dev.items]
    for i, ((buf, offs), b) in enumerate(zip(pieces, inflight)):
        rb = o.decode(buf, offs)
        rc = b.sync()
        assert (rb.err_code != 0) == (rc != 0), f"batch {i}: oracle error {rb.err_code} vs rc {rc} ({b.error})"
        _agree(b, rb, f"batch {i}")
        b.close()
    paths = d.debug_paths()
    paths["overlapped"] = d.debug_overlapped()
    paths["spared"] = d.debug_chains_spared()
    d.close()
    return paths


@pytest.mark.parametrize("overlap", [True, False])
def test_chain_whose_first_tiles_need_the_carried_state(overlap, mode):
    """As issued — batches alternate between the two decode streams, a batch reads its predecessor's totals late (carry_ready) — and with
    one decode stream (ETLG_OVERLAP=0): the carry block then travels with the prologue's other loads."""
    if not overlap:
        os.environ["ETLG_OVERLAP"] = "0"
    w, pieces = _chain_pieces()
    paths = _run_chain(w, pieces)
    assert paths["plan"] == 6 and paths["plan_redone"] == 0 and paths["redone"] == 0 and paths["chain_rerun"] == 0, paths
    assert (paths["overlapped"] > 0) == overlap, paths


@pytest.mark.parametrize("overlap", [True, False])
def test_chain_with_a_malformed_integer_in_batch_2(overlap, mode):
    """Batch 2's error is the oracle's; the batches behind it report what the oracle reports after the host's second attempts (module
    docstring: they did run on their first)."""
    if not overlap:
        os.environ["ETLG_OVERLAP"] = "0"
    w, pieces = _chain_pieces()
    b2, o2 = pieces[2]
    k = int(o2[40])
    assert b2[k + 30] == ord("I")
    b2[k + 43 + 1] = ord("x")           # a letter inside the first int4 text
    paths = _run_chain(w, pieces)
    assert paths["plan_redone"] >= 1 and paths["chain_rerun"] >= 1, paths


@pytest.mark.parametrize("overlap", [True, False])
def test_chain_with_an_update_the_plan_does_not_cover_in_batch_2(overlap, mode):
    """An Update with a key image: k_plan gives batch 2 up, the generic kernel's second attempt leaves the carried state the plan had
    published, and the batches behind it stand (the spared successors)."""
    from tests import pgwire as W
    if not overlap:
        os.environ["ETLG_OVERLAP"] = "0"
    w, pieces = _chain_pieces()
    b2, o2 = pieces[2]
    at = 40
    lo = int(o2[at])
    assert b2[lo + 30] == ord("I") and b2[int(o2[at - 1]) + 30] == ord("I")
    rel = int.from_bytes(b2[lo + 31:lo + 35].tobytes(), "big")
    lsn = int.from_bytes(b2[lo + 6:lo + 14].tobytes(), "big")
    upd = np.frombuffer(W.frame(W.xlog(lsn - 1, W.update(rel, ["5", "6", "7", "8", "9"], key=["4"]))), dtype=np.uint8)
    pieces[2] = (np.concatenate([b2[:lo], upd, b2[lo:]]), np.concatenate([o2[:at + 1], o2[at:] + len(upd)]).astype(np.uint32))
    paths = _run_chain(w, pieces)
    assert paths["plan_redone"] == 1 and paths["redone"] == 0 and paths["chain_rerun"] == 0 and paths["spared"] == 1, paths
    assert paths["plan"] == 5, paths


def test_grid_sized_by_a_bound(mode, stream):
    """frame_offsets = NULL: the second batch's decode is enqueued behind its boundary scan, its grid sized by a bound; the 4 097 frames
    are counted on the device and the waves beyond them return. (That order is taken for batches behind the pre-pass; with ETLG_PLAN_PRE=0
    the host collects the scan first and the same batches run with the count in hand.)"""
    from tests.test_gpu_async import DevBufs
    buf, offs = stream
    a = int(offs[500])
    first = (buf[:a].copy(), offs[:501].copy())
    o2 = offs[500:500 + 4097 + 1].astype(np.int64)
    second = (buf[a:int(o2[-1])].copy(), (o2 - o2[0]).astype(np.uint32))
    d, o = _pair(synth.cfg2())
    dev = DevBufs([first, second])
    got = [d.decode_device(p, n, None, 0, FLAGS) for (p, n, po, nf) in dev.items]
    for i, ((pb, po), b) in enumerate(zip((first, second), got)):
        rb = o.decode(pb, po)
        assert b.sync() == 0 and rb.err_code == 0, (i, b.error)
        _agree(b, rb, f"batch {i}")
        b.close()
    chained, redone = d.debug_scan_chained()
    paths = d.debug_paths()
    d.close()
    assert redone == 0 and (chained >= 1) == (mode == "pre_pass"), (mode, chained, redone)
    assert paths["plan"] == 2 and paths["plan_redone"] == 0, paths


def test_debug_instantiation_that_exits_early(mode, stream):
    """ETLG_PLAN_DBG=4 (stop behind the message heads): the launcher picks the debug instantiation, whose waves leave before they
    store anything and give the batch up; the call fails over to the generic kernels and returns the oracle's result."""
    os.environ["ETLG_PLAN_DBG"] = "4"
    buf, offs = _head(stream, 65)
    d, o = _pair(synth.cfg2())
    _agree(d.decode(buf, offs), o.decode(buf, offs))
    paths = d.debug_paths()
    assert paths["plan"] == 0 and paths["plan_redone"] == 1, paths
    d.close()
