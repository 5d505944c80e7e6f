"""tests/bigquery_plan.py, the host model of etlg_bigquery_plan, against the reference's own vectors for the table-copy split
(tests/golden/bigquery_split_kats.py: split_table_rows_* and calculate_target_batches_*, bigquery/core.rs:2277-2419), the closed form
of that split which the device code uses, hand-worked requests with two-row Updates, and the refusal order of write_events
(core.rs:997-1034, :1425-1554, :1599-1616, :1680-1696).
pgoutput has no Delete without an old image, so ETLG_BQP_R_DELETE_NO_OLD is reachable here only, as ETLG_CHP_R_DELETE_NO_OLD is in
tests/test_clickhouse_plan_model.py."""
import random

from tests import bigquery_plan as BP
from tests.golden import bigquery_split_kats as KATS


def test_split_table_rows_vectors():
    for name, lines, total, target, want in KATS.SPLIT_TABLE_ROWS:
        assert BP.split_table_rows(total, target) == want, (name, lines)


def test_calculate_target_batches_vectors():
    budget = 10 * 1024 * 1024                                                # any value: these vectors do not depend on it
    for name, lines, rows, first, want in KATS.CALCULATE_TARGET_BATCHES:
        lens = [] if not rows else [8 if first == "small" else budget + 5] * rows
        for b in (budget, 1, 1 << 63) if first != "over" else (budget,):
            assert BP.calculate_target_batches_for_table_copy(lens, b) == want, (name, lines, b)
    assert BP.calculate_target_batches_for_table_copy([0, 5, 5], 100) == 1   # an empty first row: checked_div gives None, rows_per_batch = total_rows
    assert BP.calculate_target_batches_for_table_copy([10] * 7, 9) == 1      # rows_per_batch == 0: "ensuring at least 1"
    assert BP.calculate_target_batches_for_table_copy([10] * 7, 20) == 4
    assert BP.calculate_target_batches_for_table_copy([10] + [1000] * 6, 20) == 4   # the estimate is row 0's alone


def test_closed_form_of_the_split():
    """What k_bqp_copy computes per request: request i < nsub holds q + (i < r) rows from row i * q + min(i, r)."""
    rnd = random.Random(5)
    cases = [(r, t) for r in range(0, 40) for t in range(0, 45)] + [(rnd.randrange(1, 5000), rnd.randrange(0, 300)) for _ in range(2000)]
    for R, target in cases:
        if R >= 2 and target == 0:                                           # the reference divides by zero there; calculate_target_batches gives 0 for no rows only
            continue
        want = BP.split_table_rows(R, target)
        if R == 0:
            got = []
        elif R <= 1 or target == 1 or R <= target:
            got = [(0, R)]
        else:
            opt = BP.div_ceil(R, target)
            nsub = BP.div_ceil(R, opt)
            q, r = R // nsub, R % nsub
            got = [(i * q + min(i, r), q + (1 if i < r else 0)) for i in range(nsub)]
        firsts = [sum(want[:i]) for i in range(len(want))]
        assert got == list(zip(firsts, want)), (R, target)
        assert len(want) <= max(R, 0) and sum(want) == R                     # the bound the host sizes the grid by


def test_plan_copy():
    m = BP.plan_copy(list(range(10)), [7] * 10, 7 * 3)                       # 3 rows per batch -> target 4 -> 3, 3, 2, 2
    assert m["info"] == {"n_reqs": 4, "n_members": 10, "n_rows": 10, "n_two_row": 0, "n_bytes": 70, "est_row_bytes": 7, "target_batches": 4}
    assert [(s["first_row"], s["end_row"], s["byte_first"], s["byte_end"], s["n_members"]) for s in m["requests"]] == \
        [(0, 3, 0, 21, 3), (3, 6, 21, 42, 3), (6, 8, 42, 56, 2), (8, 10, 56, 70, 2)]
    assert m["windows"] == [{"req_first": 0, "n_reqs": 4, "first_row": 0, "end_row": 10, "n_members": 10, "n_two_row": 0, "n_bytes": 70}]
    m = BP.plan_copy([], [], 100)
    assert m["info"]["n_reqs"] == 0 and m["info"]["target_batches"] == 0 and m["requests"] == [] and m["windows"][0]["end_row"] == 0
    assert BP.plan_copy([0], [5], 1)["info"]["n_reqs"] == 1
    assert BP.plan_copy([0, 1], [5, 5], 100, needs_host_event=1) == {"status": BP.NEEDS_HOST, "event": 1, "fail_pass": BP.NONE}


def _plan(kinds, windows=None, flags=None, row_event=None, lens=None, **kw):
    """One slot, every event a member; every event has one row of 10 bytes unless row_event says otherwise."""
    n = len(kinds)
    flags = flags or [BP.OLD_FULL if k in "UD" else 0 for k in kinds]
    row_event = list(range(n)) if row_event is None else row_event
    return BP.plan(kinds, flags, [0] * n, 0, windows or [(0, n)], row_event, lens or [10] * len(row_event), **kw)


def test_hand_worked_requests_with_two_row_updates():
    # event 1 and event 3 changed the key: a DELETE row and an UPSERT row each
    ev = [0, 1, 1, 2, 3, 3, 4]
    m = _plan("IUIUD", row_event=ev, lens=[10, 3, 10, 10, 3, 10, 3])
    assert m["info"] == {"n_reqs": 1, "n_members": 5, "n_rows": 7, "n_two_row": 2, "n_bytes": 49, "est_row_bytes": 0, "target_batches": 0}
    assert [m["requests"][0][f] for f in BP.REQ_FIELDS] == [0, 0, 7, 0, 4, 0, 49, 5]
    # a window that ends on a two-row Update takes both rows, the next begins behind them; one that begins on one takes both
    m = _plan("IUIUD", windows=[(0, 2), (2, 3), (3, 5)], row_event=ev, lens=[10, 3, 10, 10, 3, 10, 3])
    assert [tuple(w[f] for f in BP.WIN_FIELDS) for w in m["windows"]] == [(0, 1, 0, 3, 2, 1, 23), (1, 1, 3, 4, 1, 0, 10), (2, 1, 4, 7, 2, 1, 16)]
    assert [(s["window"], s["first_row"], s["end_row"], s["first_event"], s["last_event"]) for s in m["requests"]] == [(0, 0, 3, 0, 1), (1, 3, 4, 2, 2), (2, 4, 7, 3, 4)]
    # windows without a member: no request, first_row == end_row == the rows in front of data_end
    m = _plan("IUIUD", windows=[(0, 0), (0, 2), (2, 2), (5, 5)], row_event=ev, lens=[10, 3, 10, 10, 3, 10, 3])
    assert [(w["n_reqs"], w["first_row"], w["end_row"]) for w in m["windows"]] == [(0, 0, 0), (1, 0, 3), (0, 3, 3), (0, 7, 7)]
    assert m["info"]["n_reqs"] == 1 and m["requests"][0]["window"] == 1
    # events of another slot and other kinds are no members
    m = BP.plan("BIxIC", [0] * 5, [0, 0, 1, 0, 0], 0, [(0, 5)], [1, 3], [4, 6])
    assert m["info"]["n_members"] == 2 and (m["requests"][0]["first_event"], m["requests"][0]["last_event"], m["requests"][0]["byte_end"]) == (1, 3, 10)


def test_the_refusal_order():
    part, key, none = BP.FLAG_PARTIAL, BP.OLD_KEY, BP.OLD_NONE
    alt = dict(identity_type="AlternativeKey")
    wide = dict(identity_type="AlternativeKey", n_ident=1, n_pk=2)

    def failed(event, reason, fail_pass=0):
        return {"status": BP.FAILED, "event": event, "reason": reason, "fail_pass": fail_pass}

    # bigquery_update_new_row first, whatever the old image and the identity
    for old in (none, key, BP.OLD_FULL):
        assert _plan("IU", flags=[0, part | old]) == failed(1, BP.R_PARTIAL_UPDATE)
        assert _plan("IU", flags=[0, part | old], **wide) == failed(1, BP.R_PARTIAL_UPDATE)
    # an Update without an old image: only under PrimaryKey
    assert _plan("IU", flags=[0, none])["status"] == BP.OK
    assert _plan("IU", flags=[0, none], **alt) == failed(1, BP.R_UPDATE_NO_OLD_IDENTITY)
    assert _plan("IU", flags=[0, none], identity_type="Full") == failed(1, BP.R_UPDATE_NO_OLD_IDENTITY)
    assert _plan("IU", flags=[0, none], **wide) == failed(1, BP.R_UPDATE_NO_OLD_IDENTITY)   # (no key image: the width is not looked at)
    # a key image: the width in front of the identity, on Update and on Delete
    for k in "UD":
        assert _plan("I" + k, flags=[0, key], **wide) == failed(1, BP.R_KEY_WIDTH)
        assert _plan("I" + k, flags=[0, key], n_ident=2, n_pk=1) == failed(1, BP.R_KEY_WIDTH)   # even under PrimaryKey
        assert _plan("I" + k, flags=[0, key], **alt) == failed(1, BP.R_KEY_IDENTITY)
        assert _plan("I" + k, flags=[0, key])["status"] == BP.OK
        assert _plan("I" + k, flags=[0, BP.OLD_FULL], **wide)["status"] == BP.OK                # a full old image passes under any identity
    # bigquery_delete_old_row (reachable in this model only)
    assert _plan("DI", flags=[none, 0], row_event=[1]) == failed(0, BP.R_DELETE_NO_OLD)
    assert _plan("DI", flags=[none, 0], row_event=[1], **wide) == failed(0, BP.R_DELETE_NO_OLD)
    # event order decides, whatever the reason; fail_pass names the window; outside every window nothing fails
    assert _plan("IUD", flags=[0, part, none]) == failed(1, BP.R_PARTIAL_UPDATE)
    assert _plan("IDU", flags=[0, none, part]) == failed(1, BP.R_DELETE_NO_OLD)
    assert _plan("IIUI", flags=[0, 0, part, 0], windows=[(0, 1), (1, 2), (2, 4)]) == failed(2, BP.R_PARTIAL_UPDATE, 2)
    assert _plan("IUI", flags=[0, part, 0], windows=[(0, 1), (2, 3)], row_event=[0, 2])["status"] == BP.OK
    # a failing event comes before a member without a row, wherever the two lie
    assert _plan("IUU", flags=[0, BP.OLD_FULL, part], row_event=[0]) == failed(2, BP.R_PARTIAL_UPDATE)


def test_statuses_of_the_model():
    assert _plan("IIII", windows=[(0, 2), (1, 3)]) == {"status": BP.BAD_PASSES, "bad_pass": 1}
    assert _plan("IIII", windows=[(2, 1)]) == {"status": BP.BAD_PASSES, "bad_pass": 0}
    assert _plan("IIII", windows=[(0, 5)]) == {"status": BP.BAD_PASSES, "bad_pass": 0}
    assert _plan("IUI", row_event=[0, 2]) == {"status": BP.NEEDS_HOST, "event": 1, "fail_pass": 0}
    assert _plan("IUI", row_event=[0, 2], windows=[(0, 1), (1, 3)]) == {"status": BP.NEEDS_HOST, "event": 1, "fail_pass": 1}
    assert _plan("IUI", row_event=[0, 2], windows=[(0, 1), (2, 3)])["status"] == BP.OK
    m = BP.plan("II", [0, 0], [0, 0], 0, [(0, 2)], None, None, needs_host_event=1)
    assert m == {"status": BP.NEEDS_HOST, "event": 1, "fail_pass": BP.NONE}
    m = BP.plan("IU", [0, BP.FLAG_PARTIAL], [0, 0], 0, [(0, 2)], None, None, needs_host_event=1)   # FAILED comes first
    assert m["status"] == BP.FAILED and m["event"] == 1
