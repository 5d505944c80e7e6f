"""tests/snowflake_plan.py, the host model of etlg_snowflake_plan, against hand-worked cases, the three refusal orders of the
reference's encode_* functions, the token order, the facts the reference's own tests state (streaming/batch.rs:272-373:
end_offset_tracks_last_row, oversized_row_rejected) and the closed form of the segment rule that the device code uses.
pgoutput has no Delete without an old image, so ETLG_SFP_R_DELETE_NO_OLD is reachable here only, as the outline's category 5 and
DuckLake's "delete requires an old row image" are."""
import bisect
import random

from tests import snowflake_plan as SP


def _plan(kinds, lens, windows=None, flags=None, keys=None, committed=None, flush=SP.MAX_UNFLUSHED_BYTES, max_row=SP.MAX_ROW_BYTES, rows=None):
    """One slot, every event a member; event i has key (10, i) unless given; every event has a row unless `rows` lists those that do."""
    n = len(kinds)
    flags = flags or [SP.OLD_FULL if k in "UD" else 0 for k in kinds]
    keys = keys or [(10, i) for i in range(n)]
    rows = list(range(n)) if rows is None else rows
    return SP.plan(kinds, flags, [0] * n, [k[0] for k in keys], [k[1] for k in keys], 0, windows or [(0, n)], rows, [lens[i] for i in rows],
                   committed=committed, flush_bytes=flush, max_row_bytes=max_row)


def _cuts(m):
    return [(s["first_row"], s["end_row"], s["flush_before"]) for s in m["segments"]]


def test_hand_worked_segments():
    # 10-byte rows, flush at 30: s = 10, 20, then 20 + 10 >= 30 flushes in front of row 2; again in front of rows 4, 6
    m = _plan("IIIIIII", [10] * 7, flush=30)
    assert _cuts(m) == [(0, 2, 0), (2, 4, 1), (4, 6, 1), (6, 7, 1)]
    assert m["info"] == {"n_segs": 4, "n_members": 7, "n_retained": 7, "n_dropped": 0, "n_rows": 7, "n_bytes": 70}
    assert [(s["byte_first"], s["byte_end"], s["first_row_bytes"]) for s in m["segments"]] == [(0, 20, 10), (20, 40, 10), (40, 60, 10), (60, 70, 10)]
    # the >= boundary on a window's first row: a row of exactly flush_bytes flushes (an empty encoder), one byte less does not
    assert _cuts(_plan("II", [30, 5], flush=30)) == [(0, 1, 1), (1, 2, 1)]          # row 1: 30 + 5 >= 30
    assert _cuts(_plan("II", [29, 5], flush=30)) == [(0, 1, 0), (1, 2, 1)]          # 0 + 29 < 30; 29 + 5 >= 30
    assert _cuts(_plan("II", [29, 1], flush=31)) == [(0, 2, 0)]
    assert _cuts(_plan("III", [40, 40, 1], flush=30)) == [(0, 1, 1), (1, 2, 1), (2, 3, 1)]   # behind a flush s restarts at the row's length
    assert _cuts(_plan("III", [1, 1, 1], flush=1)) == [(0, 1, 1), (1, 2, 1), (2, 3, 1)]      # flush_bytes 1: every row its own segment
    # a window is a fresh builder: no segment spans two, the counter restarts
    m = _plan("IIIIII", [10] * 6, windows=[(0, 3), (3, 3), (3, 6)], flush=25)
    assert _cuts(m) == [(0, 2, 0), (2, 3, 1), (3, 5, 0), (5, 6, 1)]
    assert [(w["seg_first"], w["n_segs"], w["first_row"], w["end_row"], w["n_bytes"]) for w in m["windows"]] == [(0, 2, 0, 3, 30), (2, 0, 3, 3, 0), (2, 2, 3, 6, 30)]
    # the offset range of a segment: its first and last row's keys
    s = m["segments"][2]
    assert (s["first_commit_lsn"], s["first_tx_ordinal"], s["last_commit_lsn"], s["last_tx_ordinal"]) == (10, 3, 10, 4)


def test_the_three_refusal_orders():
    part = SP.FLAG_PARTIAL | SP.OLD_KEY
    # encode_update: the partial Update is refused in front of the offset test — a committed one still fails
    assert _plan("IU", [5, 5], flags=[0, part], committed=(10, 5)) == {"status": SP.FAILED, "event": 1, "reason": SP.R_PARTIAL_UPDATE, "row_bytes": 0}
    assert _plan("IU", [5, 5], flags=[0, part])["reason"] == SP.R_PARTIAL_UPDATE
    # encode_delete: the offset test comes first — a committed Delete without an old image is dropped, a retained one fails
    m = _plan("DI", [5, 5], flags=[SP.OLD_NONE, 0], committed=(10, 0), rows=[1])
    assert m["status"] == SP.OK and m["info"]["n_dropped"] == 1 and _cuts(m) == [(0, 1, 0)]
    assert _plan("DI", [5, 5], flags=[SP.OLD_NONE, 0], rows=[1]) == {"status": SP.FAILED, "event": 0, "reason": SP.R_DELETE_NO_OLD, "row_bytes": 0}
    # encode_insert: dropped or pushed
    assert _plan("II", [5, 5], committed=(10, 0))["info"]["n_retained"] == 1
    # event order decides, whatever the reason: the oversize row in front of the partial Update, and behind it
    assert _plan("IU", [9, 5], flags=[0, part], max_row=8) == {"status": SP.FAILED, "event": 0, "reason": SP.R_ROW_TOO_LARGE, "row_bytes": 9}
    assert _plan("UI", [5, 9], flags=[part, 0], max_row=8)["reason"] == SP.R_PARTIAL_UPDATE
    # a dropped oversize row does not fail; outside every window nothing does
    assert _plan("II", [9, 5], committed=(10, 0), max_row=8)["status"] == SP.OK
    assert _plan("IU", [5, 5], flags=[0, part], windows=[(0, 1)])["status"] == SP.OK


def test_token_order_is_the_pair_order():
    rnd = random.Random(3)
    vals = [0, 1, 9, 10, 15, 16, 255, 256, (1 << 32) - 1, 1 << 32, (1 << 63), (1 << 64) - 1]
    for _ in range(2000):
        a, b = (rnd.choice(vals), rnd.choice(vals)), (rnd.choice(vals), rnd.choice(vals))
        assert (SP.token(a) >= SP.token(b)) == (a >= b)
        assert SP.is_committed(a, b) == (not b > a)                         # retained iff key > committed
    assert not SP.is_committed(None, (0, 0))


def test_facts_of_the_reference_tests():
    # end_offset_tracks_last_row (batch.rs): three rows of one batch, the range runs from the first row's token to the last row's
    m = _plan("III", [20, 20, 20], keys=[(1, 0), (1, 1), (2, 0)])
    s = m["segments"][0]
    assert len(m["segments"]) == 1 and (s["first_commit_lsn"], s["first_tx_ordinal"], s["last_commit_lsn"], s["last_tx_ordinal"]) == (1, 0, 2, 0)
    # oversized_row_rejected: a row of exactly 2 MiB passes, one byte more fails
    assert SP.MAX_ROW_BYTES == 2 * 1024 * 1024 and SP.MAX_UNFLUSHED_BYTES == 128 * 1024
    assert _plan("I", [SP.MAX_ROW_BYTES])["status"] == SP.OK
    assert _plan("I", [SP.MAX_ROW_BYTES + 1]) == {"status": SP.FAILED, "event": 0, "reason": SP.R_ROW_TOO_LARGE, "row_bytes": SP.MAX_ROW_BYTES + 1}


def test_statuses_of_the_model():
    assert _plan("IIII", [5] * 4, windows=[(0, 2), (1, 3)]) == {"status": SP.BAD_PASSES, "bad_pass": 1}
    assert _plan("IIII", [5] * 4, windows=[(2, 1)]) == {"status": SP.BAD_PASSES, "bad_pass": 0}
    assert _plan("IIII", [5] * 4, windows=[(0, 5)]) == {"status": SP.BAD_PASSES, "bad_pass": 0}
    keys = [(10, 0), (10, 1), (20, 0), (5, 0)]
    assert _plan("IIII", [5] * 4, keys=keys, committed=(10, 0)) == {"status": SP.NOT_PREFIX, "event": 3}
    assert _plan("IIII", [5] * 4, keys=keys, committed=(10, 0), windows=[(0, 3), (3, 4)])["info"]["n_retained"] == 2   # a new window is a new prefix
    assert _plan("III", [5] * 3, rows=[0, 2]) == {"status": SP.NEEDS_HOST, "event": 1}
    assert _plan("III", [5] * 3, rows=[0, 2], committed=(10, 1))["status"] == SP.OK            # the event without a row is dropped
    m = SP.plan("II", [0, 0], [0, 0], [1, 1], [0, 1], 0, [(0, 2)], None, None, needs_host_event=1)
    assert m == {"status": SP.NEEDS_HOST, "event": 1}
    m = SP.plan("II", [0, 0], [0, 0], [7, 7], [3, 4], 0, [(0, 2)], [0, 1], [4, 4], zero_keys=True)   # a table-copy batch: the zero token
    assert (m["segments"][0]["first_commit_lsn"], m["segments"][0]["last_tx_ordinal"]) == (0, 0)


def test_closed_form_of_the_segment_rule():
    """What the device code rests on: with q the prefix sums of the retained rows' lengths, the segment that starts at row a ends at
    min(win_end, max(a + 1, the smallest e with q[e + 1] - q[a] >= flush_bytes))."""
    rnd = random.Random(11)
    for trial in range(3000):
        n = rnd.randrange(1, 40)
        flush = rnd.choice([1, 2, 7, 16, 50, 200])
        lens = [rnd.choice([1, flush - 1 or 1, flush, flush + 1, rnd.randrange(1, 2 * flush + 2)]) for _ in range(n)]
        cuts = sorted(rnd.sample(range(n + 1), rnd.randrange(0, min(4, n + 1))))
        windows = list(zip([0] + cuts, cuts + [n]))
        m = _plan("I" * n, lens, windows=windows, flush=flush, max_row=1 << 30)
        q = [0]
        for ln in lens:
            q.append(q[-1] + ln)
        want = []
        for lo, hi in windows:
            a = lo
            while a < hi:
                e = bisect.bisect_left(q, q[a] + flush, a + 1) - 1           # the smallest e with q[e + 1] >= q[a] + flush_bytes (n: none)
                nxt = min(hi, max(a + 1, e))
                want.append((a, nxt, 1 if a > lo or lens[a] >= flush else 0))
                a = nxt
        assert _cuts(m) == want, (trial, lens, windows, flush)
        per_window = [w["n_segs"] for w in m["windows"]]
        assert all(k <= 2 * (w["n_bytes"] // flush) + 2 for k, w in zip(per_window, m["windows"]))   # the bound the host sizes the jump levels by
