"""The DuckLake sink's own vectors for partial Updates (tests/golden/ducklake_update_kats.py, transcribed from ducklake/batches.rs and
core.rs) against the CPU restatement tests/ducklake_updates.py, string for string as the reference's tests compare them; then the
rules for the events the host keeps, and the zero-present-cells rule, which the wire cannot produce (a tuple of 'u' cells only would be
an Update that changes nothing)."""
import pytest

from tests import ducklake_literals as DL
from tests import ducklake_updates as DU
from tests.golden import ducklake_update_kats as K


@pytest.mark.parametrize("names,ident,event,want_set,want_pred", K.UPDATES)
def test_prepare_table_mutations_update(names, ident, event, want_set, want_pred):
    assert [p for _, p in DU.assignments(names, event["row"])] == want_set
    recs, idx, ends, host = DU.update_records([event], 0, names, ident)
    assert recs == [b", ".join(want_set), want_pred] and idx == [0, 0] and host == 0
    # col_ends cut the records back into the reference's Vec<String> assignments and into the predicate's terms
    for rec, e, sep in zip(recs, ends, (b", ", b" AND ")):
        assert len(e) == len(names) and e[-1] == len(rec)
        pieces = [rec[a:b] for a, b in zip([0] + e[:-1], e) if b > a]
        assert [p[len(sep):] if k else p for k, p in enumerate(pieces)] == rec.split(sep)
    present = [c for c in range(len(names)) if not DU.is_missing(event["row"][c])]
    assert [c for c, (a, b) in enumerate(zip([0] + ends[0][:-1], ends[0])) if b > a] == present
    # the literal hash_partial_table_row_ref takes: the piece minus len(quoted name) + 3
    for k, c in enumerate(present):
        a, b = ([0] + ends[0])[c] + (2 if k else 0), ends[0][c]
        assert recs[0][a:b][len(DL.quote_identifier(names[c])) + 3:] == DL.literal(event["row"][c])


def test_key_row_from_updated_partial_row_uses_alternative_identity_columns():
    names, ident, row, want = K.KEY_ROW
    assert DU.key_row(ident, row) == want
    e = {"kind": "U", "schema_slot": 0, "partial": True, "old_kind": "None", "row": row}
    recs, idx, ends, host = DU.update_records([e], 0, names, ident)
    assert recs == [b"\"id\" = 1, \"email\" = 'alice@example.com'", b"\"email\" = 'alice@example.com'"] and host == 0
    assert ends == [[8, 39, 39], [0, 29, 29]]                      # 8 + len(", ") + 7 + 3 + 19


def test_key_row_from_updated_partial_row_rejects_missing_replica_identity():
    names, ident, row, why = K.NO_IDENTITY
    with pytest.raises(DU.HostRow, match=why):
        DU.key_row(ident, row)
    for old in ({"old_kind": "None"}, {"old_kind": "Full", "old_row": row}):
        e = dict({"kind": "U", "schema_slot": 0, "partial": True, "row": row}, **old)
        assert DU.update_records([e], 0, names, ident) == ([], [], [], 1)


def test_host_row_rules_and_events_that_give_nothing():
    names, ident = ["id", "s", "k"], [1, 0, 1]
    ev = {"kind": "U", "schema_slot": 0, "partial": True, "old_kind": "None"}
    # an identity column that is MISSING without an old image: the host's (core.rs:896-905) ...
    miss = [("I32", 1), ("String", b"x"), ("Missing",)]
    with pytest.raises(DU.HostRow, match=K.MISSING_KEY):
        DU.key_row(ident, miss)
    assert DU.update_records([dict(ev, row=miss)], 0, names, ident) == ([], [], [], 1)
    # ... with a key image the predicate comes from that image
    recs, idx, ends, host = DU.update_records([dict(ev, row=miss, old_kind="Key", old_row=[("I32", 1), ("Null",)])], 0, names, ident)
    assert recs == [b"\"id\" = 1, \"s\" = 'x'", b'"id" = 1 AND "k" IS NULL'] and host == 0 and ends == [[8, 19, 19], [8, 8, 24]]
    # no present cell at all (batches.rs:1337): the host's, whatever the old image
    none = [("Missing",)] * 3
    with pytest.raises(DU.HostRow, match=K.NO_ASSIGNMENTS):
        DU.assignments(names, none)
    for old in ({"old_kind": "None"}, {"old_kind": "Key", "old_row": [("I32", 1), ("I32", 2)]}):
        assert DU.update_records([dict(ev, row=none, **old)], 0, names, ident) == ([], [], [], 1)
    # a NULL in a SET column is `= NULL`, not IS NULL
    recs = DU.update_records([dict(ev, row=[("I32", 1), ("Null",), ("Null",)])], 0, names, ident)[0]
    assert recs == [b'"id" = 1, "s" = NULL, "k" = NULL', b'"id" = 1 AND "k" IS NULL']
    # Inserts, Deletes, Updates with a full new row and events of other slots: nothing, and no host rows
    full = [("I32", 1), ("String", b"x"), ("I32", 2)]
    others = [{"kind": "I", "schema_slot": 0, "row": full}, {"kind": "D", "schema_slot": 0, "old_kind": "Full", "old_row": full},
              {"kind": "U", "schema_slot": 0, "partial": False, "old_kind": "None", "row": full}, dict(ev, row=miss, schema_slot=1),
              {"kind": "B"}, {"kind": "C"}]
    assert DU.update_records(others, 0, names, ident) == ([], [], [], 0)


def test_failures_report_the_set_record_first():
    from oracle.rowbinary import NeedsHost
    names, ident = ["id", "f", "j"], [1, 0, 0]
    ev = {"kind": "U", "schema_slot": 0, "partial": True, "old_kind": "None"}
    deferred = ("Deferred", 701, b"1e400x")
    with pytest.raises(NeedsHost):
        DL.literal(deferred)
    with pytest.raises(DL.Failure) as fi:
        DU.update_records([dict(ev, row=[("I32", 1), deferred, ("Missing",)]), dict(ev, row=[("I32", 1), ("Missing",), ("Deferred", 114, b"{bad")])], 0, names, ident)
    assert (fi.value.kind, fi.value.event) == ("json", 1)
    with pytest.raises(DL.Failure) as fi:
        DU.update_records([dict(ev, row=[("I32", 1), deferred, ("Missing",)])], 0, names, ident)
    assert (fi.value.kind, fi.value.event, fi.value.column) == ("host", 0, 1)
    # the same cells in a MISSING position do neither
    assert DU.update_records([dict(ev, row=[("I32", 1), ("Missing",), ("Missing",)])], 0, names, ident)[0] == [b'"id" = 1', b'"id" = 1']
