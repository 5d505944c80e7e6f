"""tests/iceberg_plan.py, the host model of etlg_iceberg_plan, against the outcomes of the reference's own unit tests of
iceberg_update_row / iceberg_delete_row (tests/golden/iceberg_plan_kats.py, iceberg/core.rs:794-840), hand-worked streams — members,
the write per window, other_slot_event, the three refusals and the member without a row —, and closed-form checks of the slice
arithmetic the device uses over packed 64-bit words (ones_in_range: edge words, an empty range, a range inside one word) against
counts over the unpacked bits.
pgoutput has no Delete without an old image, so ETLG_ICE_DELETE_WITHOUT_OLD_ROW is reachable here only, as ETLG_BQP_R_DELETE_NO_OLD is
in tests/test_bigquery_plan_model.py. ETLG_ICP_NEEDS_HOST is reachable here only too: etlg_batch_iceberg leaves no accepted member
without a row, and the call takes no other object."""
import random

import numpy as np

from tests import iceberg_plan as IP
from tests.golden import iceberg_plan_kats as KATS

F, K = IP.OLD_FULL, IP.OLD_KEY


def _col(kind, n, nulls=(), value_bytes=0, **more):
    v = np.ones(n, dtype=bool)
    v[list(nulls)] = False
    return dict({"kind": kind, "value_bytes": value_bytes, "validity": v, "deferred": np.zeros(n, dtype=bool)}, **more)


def test_reference_vectors():
    fn = {"iceberg_update_row": IP.iceberg_update_row, "iceberg_delete_row": IP.iceberg_delete_row}
    for name, func, image, accepted, text in KATS.ROW_IMAGE_KATS:
        why = fn[func](image)
        assert (why == 0) == accepted, name
        assert (IP.DESCRIPTION[why] if why else None) == text, name
    assert len(KATS.ROW_IMAGE_KATS) == 5 and sorted(IP.DESCRIPTION) == [1, 2, 3]


def test_refusal_is_one_test_per_kind():
    assert IP.refusal("I", IP.FLAG_PARTIAL | K) == 0                          # an Insert has no image to refuse
    assert IP.refusal("U", IP.FLAG_PARTIAL | F) == IP.PARTIAL_UPDATE and IP.refusal("U", K) == 0 and IP.refusal("U", IP.OLD_NONE) == 0
    assert IP.refusal("D", F) == 0 and IP.refusal("D", K) == IP.KEY_ONLY_DELETE
    assert IP.refusal("D", IP.OLD_NONE) == IP.DELETE_WITHOUT_OLD_ROW          # the model-only reason
    assert IP.refusal("D", IP.FLAG_PARTIAL | F) == 0                          # the partial bit is an Update's


# a hand-worked stream: B I(s0) I(s1,t9) U(s0) D(s0,full) I(s2, table 7: the slot's table under another slot) C | B I(s0) I(s2,t7) C
KINDS = "BIIUDIC" + "BIIC"
FLAGS = [0, 0, 0, K, F, 0, 0, 0, 0, 0, 0]
SLOTS = [0, 0, 1, 0, 0, 2, 0, 0, 0, 2, 0]
TABLES = [0, 7, 9, 7, 7, 7, 0, 0, 7, 7, 0]
ROWS = [1, 3, 4, 8]


def _hand(windows, kinds=KINDS, flags=FLAGS, rows=ROWS, cols=None):
    cols = cols if cols is not None else [_col(2, len(rows), nulls=[1], value_bytes=8)]
    return IP.plan(kinds, flags, SLOTS, TABLES, 0, 7, windows, rows, cols)


def test_hand_worked_stream():
    m = _hand([(0, 11)])
    assert m["status"] == IP.OK and m["info"] == {"n_writes": 1, "n_members": 4, "n_rows": 4, "n_mixed": 1}
    assert {k: m["writes"][0][k] for k in IP.WRITE_FIELDS} == {"window": 0, "first_row": 0, "end_row": 4, "first_event": 1, "last_event": 8, "n_members": 4,
                                                              "other_slot_event": 5}
    assert m["slices"] == [[{"null_count": 1, "deferred_count": 0, "byte_first": 0, "byte_end": 32, "child_first": 0, "child_end": 0, "child_null_count": 0}]]
    m = _hand([(0, 2), (2, 3), (3, 5), (5, 5), (5, 7), (7, 11)])                # the event of slot 1 is of another table: not an other_slot_event
    assert [w["n_writes"] for w in m["windows"]] == [1, 0, 1, 0, 0, 1] and [w["write_first"] for w in m["windows"]] == [0, 1, 1, 2, 2, 2]
    assert [w["other_slot_event"] for w in m["windows"]] == [IP.NONE, IP.NONE, IP.NONE, IP.NONE, IP.NONE, 9] and m["info"]["n_mixed"] == 1   # (5, 7) has no member
    assert [(w["first_row"], w["end_row"]) for w in m["windows"]] == [(0, 1), (1, 1), (1, 3), (3, 3), (3, 3), (3, 4)]
    assert [s[0]["null_count"] for s in m["slices"]] == [0, 1, 0] and [s[0]["byte_first"] for s in m["slices"]] == [0, 8, 24]
    assert _hand([(0, 5), (4, 6)]) == {"status": IP.BAD_PASSES, "bad_pass": 1} and _hand([(0, 12)]) == {"status": IP.BAD_PASSES, "bad_pass": 0}
    assert _hand([])["info"] == {"n_writes": 0, "n_members": 0, "n_rows": 0, "n_mixed": 0}


def test_refusals_and_the_member_without_a_row():
    partial = [0, 0, 0, K | IP.FLAG_PARTIAL, F, 0, 0, 0, 0, 0, 0]
    assert _hand([(0, 11)], flags=partial, rows=[1, 4, 8]) == {"status": IP.FAILED, "event": 3, "reason": IP.PARTIAL_UPDATE, "fail_pass": 0}
    assert _hand([(0, 3), (3, 11)], flags=partial, rows=[1, 4, 8])["fail_pass"] == 1
    assert _hand([(0, 3), (4, 11)], flags=partial, rows=[1, 4, 8])["status"] == IP.OK   # outside every window: no failure
    keyonly = [0, 0, 0, K | IP.FLAG_PARTIAL, K, 0, 0, 0, 0, 0, 0]                # both: the lower event wins, whichever its reason
    assert _hand([(0, 11)], flags=keyonly, rows=[1, 8]) == {"status": IP.FAILED, "event": 3, "reason": IP.PARTIAL_UPDATE, "fail_pass": 0}
    assert _hand([(4, 11)], flags=keyonly, rows=[1, 8]) == {"status": IP.FAILED, "event": 4, "reason": IP.KEY_ONLY_DELETE, "fail_pass": 0}
    noold = [0, 0, 0, K, IP.OLD_NONE, 0, 0, 0, 0, 0, 0]
    assert _hand([(0, 11)], flags=noold, rows=[1, 3, 8]) == {"status": IP.FAILED, "event": 4, "reason": IP.DELETE_WITHOUT_OLD_ROW, "fail_pass": 0}
    assert _hand([(0, 4), (4, 11)], rows=[1, 3, 8]) == {"status": IP.NEEDS_HOST, "event": 4, "fail_pass": 1}   # an accepted member without a row
    assert _hand([(0, 11)], flags=partial, rows=[1, 8])["status"] == IP.FAILED  # FAILED comes first


def test_copy_batch():
    m = IP.plan_copy(list(range(5)), [_col(IP.AK_BOOLEAN, 5, nulls=[0, 4])])
    assert m["info"] == {"n_writes": 1, "n_members": 5, "n_rows": 5, "n_mixed": 0} and m["windows"][0]["n_writes"] == 1
    assert m["slices"][0][0]["null_count"] == 2 and (m["slices"][0][0]["byte_first"], m["slices"][0][0]["byte_end"]) == (0, 5)
    m = IP.plan_copy([], [_col(IP.AK_BOOLEAN, 0)])
    assert m["info"]["n_writes"] == 0 and m["writes"] == [] and m["slices"] == [] and m["windows"][0]["end_row"] == 0


def test_slices_per_column_kind():
    n = 6
    text = _col(IP.AK_LARGE_UTF8, n, nulls=[2], offsets=np.array([0, 3, 3, 3, 10, 11, 20]))
    ints = _col(IP.AK_LIST, n, nulls=[0], offsets=np.array([0, 0, 2, 2, 5, 6, 6]), child_kind=1, child_count=6,
                child_validity=np.array([1, 0, 1, 1, 0, 1], dtype=bool), child_offsets=None)
    strs = _col(IP.AK_LIST, n, offsets=np.array([0, 1, 1, 3, 3, 3, 4]), child_kind=IP.AK_LARGE_UTF8, child_count=4,
                child_validity=np.array([1, 1, 0, 1], dtype=bool), child_offsets=np.array([0, 5, 7, 7, 30]))
    bools = _col(IP.AK_LIST, n, offsets=np.array([0, 3, 3, 3, 3, 3, 3]), child_kind=IP.AK_BOOLEAN, child_count=3, child_validity=np.ones(3, dtype=bool), child_offsets=None)
    empty = _col(IP.AK_LIST, n, offsets=np.zeros(n + 1, dtype=np.int64), child_kind=IP.AK_LARGE_UTF8, child_count=0, child_validity=np.zeros(0, dtype=bool), child_offsets=None)
    uuid = _col(IP.AK_FIXED16, n, value_bytes=16)
    val = lambda c, a, b: tuple(IP.column_slice(c, a, b)[f] for f in IP.SLICE_FIELDS)
    assert val(text, 1, 5) == (1, 0, 3, 11, 0, 0, 0) and val(text, 2, 3) == (1, 0, 3, 3, 0, 0, 0)
    assert val(ints, 0, 6) == (1, 0, 0, 24, 0, 6, 2) and val(ints, 1, 4) == (0, 0, 0, 20, 0, 5, 2) and val(ints, 4, 6) == (0, 0, 20, 24, 5, 6, 0)
    assert val(strs, 0, 6) == (0, 0, 0, 30, 0, 4, 1) and val(strs, 2, 3) == (0, 0, 5, 7, 1, 3, 1) and val(strs, 3, 5) == (0, 0, 7, 7, 3, 3, 0)
    assert val(bools, 0, 2) == (0, 0, 0, 3, 0, 3, 0)
    assert val(empty, 0, 6) == (0, 0, 0, 0, 0, 0, 0)                            # no child elements: no child offsets to read, both ends 0
    assert val(uuid, 2, 5) == (0, 0, 32, 80, 0, 0, 0)


def test_word_arithmetic_closed_form():
    """ones_in_range — a prefix difference over whole words and two masked edge words — against counts over the unpacked bits."""
    rnd = random.Random(11)
    for n in (1, 63, 64, 65, 128, 129, 200, 640):
        bits = np.array([rnd.random() < 0.6 for _ in range(n)], dtype=bool)
        words = IP.pack_bits(bits)
        assert len(words) == (n + 63) // 64
        edges = sorted(set(x for x in (0, 1, 62, 63, 64, 65, 127, 128, 129, n - 1, n) if 0 <= x <= n))
        pairs = [(a, b) for a in edges for b in edges if a <= b] + [tuple(sorted((rnd.randrange(n + 1), rnd.randrange(n + 1)))) for _ in range(200)]
        for a, b in pairs:
            assert IP.ones_in_range(words, a, b) == int(np.count_nonzero(bits[a:b])), (n, a, b)
    words = IP.pack_bits(np.ones(128, dtype=bool))
    assert IP.ones_in_range(words, 5, 5) == 0 and IP.ones_in_range(words, 64, 64) == 0 and IP.ones_in_range(words, 128, 128) == 0   # empty ranges
    assert IP.ones_in_range(words, 3, 9) == 6 and IP.ones_in_range(words, 70, 71) == 1                                              # inside one word
    assert IP.ones_in_range(words, 0, 64) == 64 and IP.ones_in_range(words, 64, 128) == 64 and IP.ones_in_range(words, 63, 65) == 2  # on and across a boundary
    garbage = np.array([0xFFFFFFFFFFFFFFFF], dtype=np.uint64)                   # bits behind the range's end never count: a bitmap's padding may hold anything
    assert IP.ones_in_range(garbage, 0, 10) == 10 and IP.ones_in_range(garbage, 7, 10) == 3


def test_slice_sums_over_covering_writes():
    rnd = random.Random(3)
    n = 150
    col = _col(2, n, nulls=[i for i in range(n) if rnd.random() < 0.3], value_bytes=8)
    cuts = sorted(set([0, n] + [rnd.randrange(n) for _ in range(9)]))
    total = sum(IP.column_slice(col, a, b)["null_count"] for a, b in zip(cuts, cuts[1:]))
    assert total == int(np.count_nonzero(~col["validity"]))
