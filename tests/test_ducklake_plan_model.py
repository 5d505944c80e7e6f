"""tests/ducklake_plan.py, the host model of etlg_ducklake_plan, against the reference's own vectors (tests/golden/ducklake_plan_kats.json:
the six prepare_mutation_table_batches_* tests and retain_mutations_after_sequence_key_drops_applied_prefix of ducklake/batches.rs),
against a second restatement that derives the ops from a run-length encoding of the categories, and on the three refusals. pgoutput has
no Delete without an old image, so "DuckLake delete requires an old row image" is reachable here only, as the outline's category 5 is."""
import itertools
import json
import os
import random

import pytest

from tests import ducklake_plan as DP

KATS = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "ducklake_plan_kats.json")))
KIND = {"upsert": DP.UPSERT, "delete": DP.OP_DELETE, "update": DP.OP_UPDATE}
ORIGIN = {None: None, "delete": DP.O_DELETE, "update": DP.O_UPDATE, "replace": DP.O_REPLACE}


def _mutations(v):
    if "generate" in v:
        g = v["generate"]
        return [[g["start_lsn0"] + i, g["commit_lsn0"] + i, g["tx_ordinal"], g["kind"]] for i in range(g["count"])]
    return v["mutations"]


def _plan(muts, watermark=None, n_ident=1, windows=None, flags=None):
    """One slot, every mutation an event of it; U = a full Update with a full old image, D = a Delete with one."""
    kinds = "".join(m[3] for m in muts)
    flags = flags or [DP.OLD_FULL if k in "UD" else 0 for k in kinds]
    return DP.plan(kinds, flags, [0] * len(muts), [m[0] for m in muts], [m[1] for m in muts], [m[2] for m in muts], 0,
                   windows or [(0, len(muts))], watermark=watermark, n_ident=n_ident)


@pytest.mark.parametrize("v", KATS["prepare"], ids=lambda v: v["name"])
def test_reference_prepare_vectors(v):
    assert KATS["batch_size"] == DP.BATCH_SIZE
    muts = _mutations(v)
    m = _plan(muts)
    assert m["status"] == DP.OK and m["info"]["n_batches"] == len(v["batches"])
    assert m["info"]["n_members"] == m["info"]["n_retained"] == len(muts)
    for got, want in zip(m["batches"], v["batches"]):
        ops = m["ops"][got["op_first"]:got["op_first"] + got["n_ops"]]
        if "n_ops" in want:
            assert got["n_ops"] == want["n_ops"]
        for o, (kind, origin, cnt) in zip(ops, want.get("ops") or [want["first_op"]]):
            assert o["kind"] == KIND[kind]
            assert origin is None or o["origin"] == ORIGIN[origin]
            assert cnt is None or o["n"] == cnt
        first, last = muts[got["first_event"]], muts[got["end_event"] - 1]
        assert (got["first_start_lsn"], got["last_commit_lsn"]) == (first[0], last[1])       # build_mutation_batch_identity :1440-1445
        assert (got["first_commit_lsn"], got["first_tx_ordinal"], got["last_tx_ordinal"]) == (first[1], first[2], last[2])
    assert sum(b["n_members"] for b in m["batches"]) == len(muts)


def test_reference_predicates_of_contiguous_deletes():
    """The two predicates the reference asserts are what tests/ducklake_literals.py writes for the rows' key cells."""
    from tests import ducklake_literals as DL
    v = next(x for x in KATS["prepare"] if "predicates" in x)
    assert [DL.predicate(["id"], [("I32", int(r[0]))]).decode() for r in v["rows"]] == v["predicates"]
    m = _plan(_mutations(v))
    assert [(o["kind"], o["origin"], o["n"]) for o in m["ops"]] == [(DP.OP_DELETE, DP.O_DELETE, len(v["predicates"]))]


@pytest.mark.parametrize("v", KATS["retain"], ids=lambda v: v["name"])
def test_reference_retain_vector(v):
    muts = v["mutations"]
    keys = [(m[1], m[2]) for m in muts]
    kept = DP.retain(range(len(muts)), keys, v["watermark"])
    assert [list(keys[i]) for i in kept] == v["retained"]
    m = _plan(muts, watermark=v["watermark"])
    assert m["status"] == DP.OK and (m["info"]["n_retained"], m["info"]["n_dropped"]) == (1, 2)
    assert m["batches"][0]["first_event"] == 2


def _ops_by_run_length(cats):
    """The second restatement: the categories run-length encoded; a run of Inserts or Deletes is one op, every other member its own."""
    out, at = [], 0
    for cat, run in itertools.groupby(cats):
        n = len(list(run))
        if cat == DP.INSERT:
            out.append((DP.UPSERT, DP.O_NONE, at, n))
        elif cat == DP.DELETE:
            out.append((DP.OP_DELETE, DP.O_DELETE, at, n))
        else:
            for k in range(n):
                if cat == DP.UPDATE_PARTIAL:
                    out.append((DP.OP_UPDATE, DP.O_NONE, at + k, 1))
                else:
                    out += [(DP.OP_DELETE, DP.O_UPDATE if cat == DP.UPDATE_FULL else DP.O_REPLACE, at + k, 1), (DP.UPSERT, DP.O_NONE, at + k, 1)]
        at += n
    return out


def test_two_restatements_agree_on_random_sequences():
    rnd = random.Random(7)
    shape = {DP.INSERT: ("I", 0), DP.UPDATE_FULL: ("U", DP.OLD_KEY), DP.REPLACE: ("U", DP.OLD_NONE), DP.UPDATE_PARTIAL: ("U", DP.FLAG_PARTIAL | DP.OLD_FULL),
             DP.DELETE: ("D", DP.OLD_KEY)}
    for trial in range(300):
        n = rnd.randrange(1, 70)
        weights = [rnd.random() ** 2 + 0.01 for _ in range(5)]
        cats = rnd.choices(range(5), weights=weights, k=n)
        muts = [[100 + i, 200 + i // 3, i % 3, shape[c][0]] for i, c in enumerate(cats)]
        cuts = sorted(rnd.sample(range(n + 1), rnd.randrange(0, min(4, n + 1))))
        windows = list(zip([0] + cuts, cuts + [n]))
        m = _plan(muts, windows=windows, flags=[shape[c][1] for c in cats])
        assert m["status"] == DP.OK
        want_b, want_ops = [], []
        for lo, hi in windows:
            for at in range(lo, hi, DP.BATCH_SIZE):
                end = min(at + DP.BATCH_SIZE, hi)
                ops = [(k, o, at + f, c) for k, o, f, c in _ops_by_run_length(cats[at:end])]
                want_b.append((at, end, len(want_ops), len(ops)))
                want_ops += ops
        assert [(b["first_event"], b["end_event"], b["op_first"], b["n_ops"]) for b in m["batches"]] == want_b, trial
        assert [(o["kind"], o["origin"], o["first_event"], o["n"]) for o in m["ops"]] == want_ops, trial
        assert all(b["n_ops"] <= 32 for b in m["batches"])
        assert [b["n_cat"] for b in m["batches"]] == [[cats[a:e].count(k) for k in range(5)] for a, e, _, _ in want_b]


def test_the_three_refusals_and_their_order():
    muts = [[1, 2, 0, "I"], [1, 2, 1, "U"], [1, 2, 2, "D"]]
    assert _plan(muts, n_ident=0) == {"status": DP.REFUSED, "event": 1, "reason": DP.R_UPDATE_IDENTITY}
    assert _plan(muts[::2], n_ident=0) == {"status": DP.REFUSED, "event": 1, "reason": DP.R_DELETE_IDENTITY}
    assert _plan(muts, flags=[0, DP.OLD_KEY, DP.OLD_NONE]) == {"status": DP.REFUSED, "event": 2, "reason": DP.R_DELETE_NO_OLD}
    assert _plan(muts, n_ident=0, flags=[0, DP.OLD_KEY, DP.OLD_NONE])["reason"] == DP.R_UPDATE_IDENTITY     # the identity is looked at first
    assert set(DP.REASON_TEXT) == {1, 2, 3}
    # refusal comes before the replay filter: the refused Delete lies below the watermark
    assert _plan(muts, flags=[0, DP.OLD_KEY, DP.OLD_NONE], watermark=(2, 5))["status"] == DP.REFUSED
    # ... and only inside a window
    assert _plan(muts, flags=[0, DP.OLD_KEY, DP.OLD_NONE], windows=[(0, 2)])["status"] == DP.OK


def test_statuses_of_the_model():
    muts = [[1, 10, 0, "I"], [1, 10, 1, "I"], [1, 20, 0, "I"], [1, 5, 0, "I"]]
    assert _plan(muts, windows=[(0, 2), (1, 3)]) == {"status": DP.BAD_PASSES, "bad_pass": 1}
    assert _plan(muts, windows=[(2, 1)]) == {"status": DP.BAD_PASSES, "bad_pass": 0}
    assert _plan(muts, windows=[(0, 5)]) == {"status": DP.BAD_PASSES, "bad_pass": 0}
    assert _plan(muts, watermark=(10, 0)) == {"status": DP.NOT_PREFIX, "event": 3}
    assert _plan(muts, watermark=(10, 0), windows=[(0, 3), (3, 4)])["info"]["n_retained"] == 2      # a new window is a new prefix
    kinds = "III"
    m = DP.plan(kinds, [0] * 3, [0] * 3, [1] * 3, [2] * 3, [0, 1, 2], 0, [(0, 3)], tuples=[0, 2])
    assert m == {"status": DP.NEEDS_HOST, "event": 1}
