"""tests/payload_meta.py, the host model of etlg_batch_payload, against the reference's own vectors
(crates/etl/src/metrics/source_payload_metadata.rs:318-449) and against the whole-batch oracle: the per-frame walk sums to the batch's
payload_bytes, and the ordinal join of include/etlg.h reproduces the walk's frame -> event map — batches that begin inside a transaction
included. No GPU."""
import numpy as np
import pytest

from tests import payload_meta as PM
from tests import pgwire as W
from tests import scenarios as SC


# ---------------------------------------------------------------- the reference's vectors

def test_merge_sequence_of_the_reference():
    m = PM.Meta()
    for x in (PM.Meta(), PM.Meta.of(0, 0), PM.Meta(), PM.Meta.of(1, 5), PM.Meta.of(2, PM.U64_MAX), PM.Meta.of(0, 11), PM.Meta.of(2, 1)):
        m.merge(x)
    assert m.processed() == [("insert", 11), ("update", 5), ("delete", PM.U64_MAX)]
    assert m.total() == PM.U64_MAX


def test_copy_rows_of_the_reference():
    m = PM.Meta.of(3, 3).merge(PM.Meta.of(3, 5))
    assert m.processed() == [("copy", 8)] and m.total() == 8
    assert PM.Meta.of(3, 3).observations() + PM.Meta.of(3, 5).observations() == [3.0, 5.0]
    sums = PM.range_sums(None, [3, 5], [], copy=True)
    assert sums[0, 0, 3] == 8 and sums[0, 1, 3] == 2 and not sums[0, :, :3].any()


def test_zero_bytes_is_an_observation_and_default_is_none():
    assert PM.Meta.of(0, 0).observations() == [0.0] and PM.Meta.of(0, 0).processed() == [("insert", 0)]
    assert PM.Meta().observations() == [] and PM.Meta().processed() == []
    sums = PM.range_sums([0, None], [0, 0], [1])
    assert sums[0, 1, 0] == 1 and sums[0, 0, 0] == 0                       # Some(0): a row with no bytes
    assert not sums[1].any()                                               # None


def test_buckets_are_le_and_not_cumulated():
    h = PM.buckets([(0, 0), (0, 4), (0, 5), (1, 5), (2, 6), (2, 100)], [4, 5, 50])
    assert h.tolist() == [[2, 1, 0, 0], [0, 1, 0, 0], [0, 0, 1, 1], [0, 0, 0, 0]]
    assert PM.buckets([(1, 7)], []).tolist() == [[0], [1], [0], [0]]


# ---------------------------------------------------------------- the issue's join example

COLS = [("id", SC.INT8, False, 1), ("v", SC.TEXT, True, 0)]


def _two_tables(t):
    SC.simple_table(COLS, table_id=42)(t)
    t.schema_put(43, 0, COLS)                                              # known, never owned


def test_transaction_with_a_message_of_a_table_that_is_not_owned():
    from oracle import oracle
    s = SC.txn([W.insert(42, ["1", "abc"]), W.insert(43, ["22", "abcdef"]), W.insert(42, ["3", W.NULL])])
    buf, offs = np.frombuffer(s.bytes(), dtype=np.uint8), s.offsets
    o = oracle.Oracle()
    _two_tables(o)
    hb = o.decode(buf, offs).host_batch()
    assert hb.tx_ordinal.tolist() == [0, 1, 3, 4] and tuple(hb.payload_bytes) == (13, 0, 0)
    o2 = oracle.Oracle()
    _two_tables(o2)
    w = PM.Walk(o2, buf, offs)
    assert [b for k, b, _ in w.frames if k == 0] == [4, 8, 1] and w.received() == ([13, 0, 0, 0], [3, 0, 0, 0])
    assert w.event_frames() == [0, 1, 3, 4] and w.ev_bytes().tolist() == [0, 4, 1, 0]
    assert PM.join(buf, offs, w.n_frames, hb.kind, hb.tx_ordinal, 0) == [0, 1, 3, 4]


# ---------------------------------------------------------------- every scenario

def _batches(sc):
    for buf, offs in sc.batches:
        a = np.frombuffer(bytes(buf), dtype=np.uint8) if not isinstance(buf, np.ndarray) else buf
        yield a, (PM.frame_offsets(a) if offs is None else np.asarray(offs, dtype=np.uint32)), offs


@pytest.mark.parametrize("sc", SC.all_scenarios(), ids=repr)
def test_walk_sums_to_the_batch_and_the_join_finds_every_event(sc):
    from oracle import oracle
    whole, frames = oracle.Oracle(), oracle.Oracle()
    for t in (whole, frames):
        if sc.worker:
            t.set_worker(*sc.worker)
        sc.prime(t)
    entry = 0
    for buf, offs, given in _batches(sc):
        rb = whole.decode(buf, given)
        hb = rb.host_batch()
        w = PM.Walk(frames, buf, offs)
        assert w.n_frames == hb.n_frames, (w.n_frames, hb.n_frames, w.err, rb.err_code)
        # (without a sidecar the batch may also fail behind its last whole frame, on bytes that are no frame: the walk ends in front of them)
        assert bool(w.err) == bool(rb.err_code) or (given is None and not w.err and w.n_frames == len(offs) - 1)
        assert tuple(w.received()[0][:3]) == tuple(hb.payload_bytes)
        assert len(w.event_frames()) == hb.n_events
        assert PM.join(buf, offs, w.n_frames, hb.kind, hb.tx_ordinal, entry) == w.event_frames()
        kinds = [{0: ord("I"), 1: ord("U"), 2: ord("D")}.get(k) for k in w.ev_kinds()]
        assert all(k is None or k == int(e) for k, e in zip(kinds, hb.kind))
        entry = PM.next_entry_ord(buf, offs, w.n_frames, entry)
        if rb.err_code:
            break                                                          # (an error ends the stream: what follows starts from a state of its own)
