"""tests/clickhouse_plan.py, the host model of etlg_clickhouse_plan, against hand-worked cases, the refusal order of the reference's
write_events_inner (clickhouse/core.rs:1063-1136, :1359-1452) and the closed form of insert_rows' statement rule (clickhouse/client.rs:
578-600) that the device code uses.
The reference's own tests state no statement boundary as a number — they assert SQL text, encodings and schema diffs —, so there are
no vectors to transcribe: the cases below are worked by hand from the loop's text.
pgoutput has no Delete without an old image, so ETLG_CHP_R_DELETE_NO_OLD is reachable here only, as ETLG_SFP_R_DELETE_NO_OLD is in
tests/test_snowflake_plan_model.py."""
import bisect
import random

from tests import clickhouse_plan as CP


def _plan(kinds, lens, windows=None, flags=None, rows=None, **kw):
    """One slot, every event a member; every event has a row unless `rows` lists those that do."""
    n = len(kinds)
    flags = flags or [CP.OLD_FULL if k in "UD" else 0 for k in kinds]
    rows = list(range(n)) if rows is None else rows
    return CP.plan(kinds, flags, [0] * n, 0, windows or [(0, n)], rows, [lens[i] for i in rows], **kw)


def _cuts(m):
    return [(s["first_row"], s["end_row"]) for s in m["statements"]]


def test_hand_worked_statements():
    # 10-byte rows, 25 bytes per INSERT: bytes = 10, 20, 30 >= 25 closes behind row 2; again behind row 5; row 6 is the short last one
    m = _plan("IIIIIII", [10] * 7, max_bytes=25)
    assert _cuts(m) == [(0, 3), (3, 6), (6, 7)]
    assert m["info"] == {"n_stmts": 3, "n_members": 7, "n_rows": 7, "n_bytes": 70}
    assert [(s["byte_first"], s["byte_end"], s["first_event"], s["last_event"]) for s in m["statements"]] == [(0, 30, 0, 2), (30, 60, 3, 5), (60, 70, 6, 6)]
    # the statement closes on the row that REACHES the budget: exactly a prefix closes there, one byte more takes one more row
    assert _cuts(_plan("IIII", [10] * 4, max_bytes=20)) == [(0, 2), (2, 4)]
    assert _cuts(_plan("IIII", [10] * 4, max_bytes=21)) == [(0, 3), (3, 4)]
    assert _cuts(_plan("IIII", [10] * 4, max_bytes=19)) == [(0, 2), (2, 4)]
    assert _cuts(_plan("III", [10, 10, 10], max_bytes=10)) == [(0, 1), (1, 2), (2, 3)]          # a single row's length
    assert _cuts(_plan("III", [30, 1, 1], max_bytes=10)) == [(0, 1), (1, 3)]                     # a row above the budget is a statement of its own
    assert _cuts(_plan("III", [7, 8, 9], max_bytes=1)) == [(0, 1), (1, 2), (2, 3)]               # budget 1: a statement per row
    assert _cuts(_plan("III", [7, 8, 9], max_bytes=25)) == [(0, 3)]                              # more than all bytes: one statement
    assert _cuts(_plan("III", [7, 8, 9])) == [(0, 3)]                                            # the reference's 64 MiB
    assert _cuts(_plan("III", [7, 8, 9], max_bytes=1 << 63)) == [(0, 3)]
    # a window is one insert_rows call: no statement spans two, the counter restarts, an empty window has none
    m = _plan("IIIIII", [10] * 6, windows=[(0, 3), (3, 3), (3, 6)], max_bytes=20)
    assert _cuts(m) == [(0, 2), (2, 3), (3, 5), (5, 6)]
    assert [tuple(w[f] for f in CP.WIN_FIELDS) for w in m["windows"]] == [(0, 2, 0, 3, 3, 30), (2, 0, 3, 3, 0, 0), (2, 2, 3, 6, 3, 30)]
    # events of another slot and other kinds are no members
    m = CP.plan("BIxIC", [0] * 5, [0, 0, 1, 0, 0], 0, [(0, 5)], [1, 3], [4, 6], max_bytes=100)
    assert m["info"]["n_members"] == 2 and _cuts(m) == [(0, 2)] and (m["statements"][0]["first_event"], m["statements"][0]["last_event"]) == (1, 3)


def test_the_refusal_order():
    part, key = CP.FLAG_PARTIAL | CP.OLD_KEY, CP.OLD_KEY
    alt = dict(identity_type="AlternativeKey")
    rmt = dict(engine=CP.REPLACING_MERGE_TREE)

    def failed(event, reason, fail_pass=0):
        return {"status": CP.FAILED, "event": event, "reason": reason, "fail_pass": fail_pass}

    # clickhouse_update_row: the partial row first, under both engines and whatever the identity
    assert _plan("IU", [5, 5], flags=[0, part]) == failed(1, CP.R_PARTIAL_UPDATE)
    assert _plan("IU", [5, 5], flags=[0, part], **rmt, **alt) == failed(1, CP.R_PARTIAL_UPDATE)
    # ... then the identity, under ReplacingMergeTree only; PrimaryKey and Full pass
    assert _plan("IU", [5, 5], flags=[0, key], **rmt, **alt) == failed(1, CP.R_UPDATE_IDENTITY)
    assert _plan("IU", [5, 5], flags=[0, key], **rmt, identity_type="Missing") == failed(1, CP.R_UPDATE_IDENTITY)
    assert _plan("IU", [5, 5], flags=[0, key], **alt)["status"] == CP.OK
    assert _plan("IU", [5, 5], flags=[0, key], **rmt, identity_type="Full")["status"] == CP.OK
    assert _plan("IU", [5, 5], flags=[0, key], **rmt)["status"] == CP.OK
    # clickhouse_delete_old_row: no old image, both engines (reachable in this model only)
    assert _plan("DI", [5, 5], flags=[CP.OLD_NONE, 0], rows=[1]) == failed(0, CP.R_DELETE_NO_OLD)
    assert _plan("DI", [5, 5], flags=[CP.OLD_NONE, 0], rows=[1], **rmt, **alt) == failed(0, CP.R_DELETE_NO_OLD)
    # expand_key_row: the width in front of the identity, both engines; a full old image passes under any identity
    assert _plan("D", [5], flags=[key], **alt, n_ident=2, n_pk=1) == failed(0, CP.R_KEY_WIDTH)
    assert _plan("D", [5], flags=[key], n_ident=2, n_pk=1) == failed(0, CP.R_KEY_WIDTH)           # even under PrimaryKey
    assert _plan("D", [5], flags=[key], **alt) == failed(0, CP.R_KEY_IDENTITY)
    assert _plan("D", [5], flags=[key], **alt, **rmt) == failed(0, CP.R_KEY_IDENTITY)
    assert _plan("D", [5], flags=[CP.OLD_FULL], **alt, n_ident=2, n_pk=1)["status"] == CP.OK
    assert _plan("D", [5], flags=[key])["status"] == CP.OK
    # event order decides, whatever the reason; fail_pass names the window; outside every window nothing fails
    assert _plan("IUD", [5] * 3, flags=[0, part, CP.OLD_NONE]) == failed(1, CP.R_PARTIAL_UPDATE)
    assert _plan("IDU", [5] * 3, flags=[0, CP.OLD_NONE, part]) == failed(1, CP.R_DELETE_NO_OLD)
    assert _plan("IIUI", [5] * 4, flags=[0, 0, part, 0], windows=[(0, 1), (1, 2), (2, 4)]) == failed(2, CP.R_PARTIAL_UPDATE, 2)
    assert _plan("IUI", [5] * 3, flags=[0, part, 0], windows=[(0, 1), (2, 3)], rows=[0, 2])["status"] == CP.OK
    # a failing event comes before a member without a row, wherever the two lie
    assert _plan("IIU", [5] * 3, flags=[0, 0, part], rows=[0]) == failed(2, CP.R_PARTIAL_UPDATE)


def test_statuses_of_the_model():
    assert _plan("IIII", [5] * 4, windows=[(0, 2), (1, 3)]) == {"status": CP.BAD_PASSES, "bad_pass": 1}
    assert _plan("IIII", [5] * 4, windows=[(2, 1)]) == {"status": CP.BAD_PASSES, "bad_pass": 0}
    assert _plan("IIII", [5] * 4, windows=[(0, 5)]) == {"status": CP.BAD_PASSES, "bad_pass": 0}
    assert _plan("IDI", [5] * 3, flags=[0, CP.OLD_KEY, 0], rows=[0, 2]) == {"status": CP.NEEDS_HOST, "event": 1, "fail_pass": 0}
    assert _plan("IDI", [5] * 3, flags=[0, CP.OLD_KEY, 0], rows=[0, 2], windows=[(0, 1), (1, 3)]) == {"status": CP.NEEDS_HOST, "event": 1, "fail_pass": 1}
    assert _plan("IDI", [5] * 3, flags=[0, CP.OLD_KEY, 0], rows=[0, 2], windows=[(0, 1), (2, 3)])["status"] == CP.OK
    m = CP.plan("II", [0, 0], [0, 0], 0, [(0, 2)], None, None, needs_host_event=1)
    assert m == {"status": CP.NEEDS_HOST, "event": 1, "fail_pass": CP.NONE}
    m = CP.plan("IU", [0, CP.FLAG_PARTIAL], [0, 0], 0, [(0, 2)], None, None, needs_host_event=1)   # FAILED comes first
    assert m["status"] == CP.FAILED and m["event"] == 1
    assert CP.MAX_BYTES_PER_INSERT == 64 * 1024 * 1024


def test_closed_form_of_the_statement_rule():
    """What the device code rests on: with q the prefix sums of the rows' lengths, the statement that starts at row a ends at
    min(win_end, the smallest e > a with q[e] - q[a] >= max_bytes), and a window has at most bytes // max_bytes + 1 of them."""
    rnd = random.Random(11)
    for trial in range(3000):
        n = rnd.randrange(1, 40)
        budget = rnd.choice([1, 2, 7, 16, 50, 200])
        lens = [rnd.choice([1, budget - 1 or 1, budget, budget + 1, rnd.randrange(1, 2 * budget + 2)]) for _ in range(n)]
        cuts = sorted(rnd.sample(range(n + 1), rnd.randrange(0, min(4, n + 1))))
        windows = list(zip([0] + cuts, cuts + [n]))
        m = _plan("I" * n, lens, windows=windows, max_bytes=budget)
        q = [0]
        for ln in lens:
            q.append(q[-1] + ln)
        want = []
        for lo, hi in windows:
            a = lo
            while a < hi:
                nxt = min(hi, bisect.bisect_left(q, q[a] + budget, a + 1))   # the smallest e > a with q[e] >= q[a] + max_bytes (n + 1: none)
                want.append((a, nxt))
                a = nxt
        assert _cuts(m) == want, (trial, lens, windows, budget)
        assert all(w["n_stmts"] <= w["n_bytes"] // budget + 1 and w["n_stmts"] <= w["n_members"] for w in m["windows"])   # the bound the host sizes the jump levels by
        assert m["info"]["n_stmts"] <= m["info"]["n_bytes"] // budget + len(windows)                                       # ... and the emit grid
