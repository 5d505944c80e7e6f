"""TEST INFRASTRUCTURE — CPU restatement of what the DuckLake sink makes of a partial Update, for the parity tests of
etlg_batch_duckdb(ETLG_DL_UPDATES) (etl_amd/csrc/columns.hip dl_selected, rowformats.hip.h dl_row). Never imported by the product path.

Follows crates/etl-destinations/src/ducklake: core.rs:1846-1913 (the row choice: TableMutation::Update { delete_row, new_row: Partial },
delete_row the old image, else the key row built from the partial row itself), core.rs:846-939 key_row_from_updated_partial_row,
batches.rs:1179-1190 (PreparedTableMutation::Update { assignments, predicate }), batches.rs:1319-1399
update_assignments_from_partial_row, batches.rs:2125 (the assignments joined by ", "), batches.rs:1229-1316 delete_predicate_from_row.
Literals, identifiers and the predicate text are those of tests/ducklake_literals.py.

Works on the events of etl_amd.view.HostBatch.materialize(): a partial row carries ("Missing",) cells and e["partial"]."""
from oracle import arrays
from oracle.rowbinary import NeedsHost
from tests import ducklake_literals as DL


class HostRow(Exception):
    """An event the host has to take: the reference's error description."""


def is_missing(c):
    return c[0] == "Missing"


def assignments(names, row):
    """update_assignments_from_partial_row -> [(column index, `"c" = lit`)]. Raises HostRow when no cell is present."""
    out = [(i, DL.quote_identifier(names[i]) + b" = " + DL.literal(c)) for i, c in enumerate(row) if not is_missing(c)]
    if not out:
        raise HostRow("DuckLake partial update row has no assignments")
    return out


def key_row(identity, row):
    """key_row_from_updated_partial_row -> the identity cells of a partial row. Raises HostRow."""
    key_cols = [i for i, f in enumerate(identity) if f]
    if not key_cols:
        raise HostRow("DuckLake update requires a replica identity")
    if any(is_missing(row[i]) for i in key_cols):
        raise HostRow("DuckLake partial update is missing replica-identity columns")
    return [row[i] for i in key_cols]


def choose(e, identity):
    """core.rs:1846-1913 for a partial Update -> [(identity column, cell)] of the mutation's delete_row. Raises HostRow."""
    key_cols = [i for i, f in enumerate(identity) if f]
    if not key_cols:                                  # validate_ducklake_replica_identity(.., "update")
        raise HostRow("DuckLake update requires a replica identity")
    if e["old_kind"] == "Full":
        return [(c, e["old_row"][c]) for c in key_cols]
    if e["old_kind"] == "Key":
        return list(zip(key_cols, e["old_row"]))
    return list(zip(key_cols, key_row(identity, e["row"])))


def _ends(n_cols, pieces, sep):
    """col_ends of a record built from [(column, piece)] joined by sep."""
    ends, at, k = [], 0, 0
    for c in range(n_cols):
        if k < len(pieces) and pieces[k][0] == c:
            at += (len(sep) if k else 0) + len(pieces[k][1])
            k += 1
        ends.append(at)
    return ends


def update_records(events, slot_index, names, identity):
    """(records, event index of every record, col_ends rows, events left to the host): two records per partial Update of the slot —
    its SET clause, then its predicate. Raises DL.Failure: a json cell that is not JSON first, else the first record in event order the
    device hands back (its first column)."""
    recs, idx, ends, host, fails = [], [], [], 0, []
    n = len(names)
    for i, e in enumerate(events):
        if e["kind"] != "U" or e.get("schema_slot") != slot_index or not e.get("partial"):
            continue
        row = e["row"]
        try:
            look = choose(e, identity)
            if all(is_missing(c) for c in row):
                raise HostRow("DuckLake partial update row has no assignments")
        except HostRow:
            host += 1
            continue
        first = None
        for rec in ([(c, x) for c, x in enumerate(row) if not is_missing(x)], look):
            mine = None
            for col, c in rec:
                try:
                    DL.literal(c)
                except arrays.JsonDecodeError:
                    mine = DL.Failure("json", i)
                    break
                except NeedsHost:
                    mine = mine or DL.Failure("host", i, col)
            if mine and (first is None or (mine.kind == "json" and first.kind != "json")):
                first = mine
        if first:
            fails.append(first)
            continue
        sets = assignments(names, row)
        preds = [(c, DL.predicate([names[c]], [x])) for c, x in look]
        recs += [b", ".join(p for _, p in sets), b" AND ".join(p for _, p in preds)]
        idx += [i, i]
        ends += [_ends(n, sets, b", "), _ends(n, preds, b" AND ")]
    js = [f for f in fails if f.kind == "json"]
    if js or fails:
        raise (js or fails)[0]
    return recs, idx, ends, host
