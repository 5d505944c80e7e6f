"""TEST INFRASTRUCTURE — host model of etlg_clickhouse_plan (include/etlg.h): the ClickHouse sink's INSERT statements of one schema slot.
It restates the reference as the plain sequential loop it is: per window one pass of write_events_inner
(crates/etl-destinations/src/clickhouse/core.rs:1063-1136) with its refusals in their own order — clickhouse_update_row :1359-1382,
clickhouse_delete_old_row :1385-1400, expand_key_row :1437-1452 with ensure_clickhouse_key_identity_is_primary_key :1404-1427 — and,
for the rows the pass gathered, insert_rows' loop with its byte counter that restarts with every statement (clickhouse/client.rs:
578-600). No prefix sums, no jump tables: the device code is written the other way round and tests/test_gpu_clickhouse_plan.py
compares the two field by field.
The reference's own tests state no statement boundary as a number, so there are no vectors to transcribe;
tests/test_clickhouse_plan_model.py checks this loop against hand-worked cases and the closed form of the statement rule."""
import bisect

NONE = (1 << 64) - 1
OK, BAD_PASSES, FAILED, NEEDS_HOST = range(4)
R_PARTIAL_UPDATE, R_UPDATE_IDENTITY, R_DELETE_NO_OLD, R_KEY_WIDTH, R_KEY_IDENTITY = 1, 2, 3, 4, 5
OLD_NONE, OLD_FULL, OLD_KEY, FLAG_PARTIAL = 0, 1, 2, 4
MERGE_TREE, REPLACING_MERGE_TREE = 0, 1
MAX_BYTES_PER_INSERT = 64 * 1024 * 1024                                      # core.rs:234 (DEFAULT_MAX_BYTES_PER_INSERT)
STMT_FIELDS = ("window", "first_row", "end_row", "first_event", "last_event", "byte_first", "byte_end")
WIN_FIELDS = ("stmt_first", "n_stmts", "first_row", "end_row", "n_members", "n_bytes")
INFO_FIELDS = ("n_stmts", "n_members", "n_rows", "n_bytes")


def refusal(kind, fl, engine, identity_type, n_ident, n_pk):
    """What write_events_inner raises at one event of the table, 0 for none; the tests in the reference's order."""
    key_identity = identity_type in ("PrimaryKey", "Full")
    if kind == "U":
        if fl & FLAG_PARTIAL:                                                # clickhouse_update_row: not UpdatedTableRow::Full
            return R_PARTIAL_UPDATE
        if engine == REPLACING_MERGE_TREE and not key_identity:              # ... then, under ReplacingMergeTree only, the identity
            return R_UPDATE_IDENTITY
    if kind == "D":
        if fl & 3 == OLD_NONE:                                               # clickhouse_delete_old_row
            return R_DELETE_NO_OLD
        if fl & 3 == OLD_KEY:                                                # expand_key_row: the width first, then the identity
            if n_ident != n_pk:
                return R_KEY_WIDTH
            if not key_identity:
                return R_KEY_IDENTITY
    return 0


def plan(kinds, flags, slots, slot, windows, row_event, row_len, engine=MERGE_TREE, identity_type="PrimaryKey", n_ident=1, n_pk=1,
         max_bytes=MAX_BYTES_PER_INSERT, needs_host_event=None):
    """kinds: one letter per event; flags, slots: per event; windows: [(first_event, data_end)]; row_event / row_len: the RowBinary
    object's rows (ascending events) and their lengths; engine: the one the object was built for; identity_type, n_ident, n_pk: the
    slot's; needs_host_event: the object came back NEEDS_HOST with this host_event and has no rows. Returns {"status", ...} as info does."""
    assert max_bytes >= 1                                                    # with 0 the reference's loop never ends
    n = len(kinds)
    for p, (lo, hi) in enumerate(windows):
        if lo > hi or hi > n or (p and lo < windows[p - 1][1]):
            return {"status": BAD_PASSES, "bad_pass": p}
    no_rows = needs_host_event is not None
    row_event = [] if no_rows else [int(e) for e in row_event]
    offs = [0]
    for ln in ([] if no_rows else row_len):
        offs.append(offs[-1] + int(ln))
    failed = needs_host = None
    stmts, wins = [], []
    n_members = 0
    for w, (lo, hi) in enumerate(windows):
        pending, members = [], 0                                             # the table's Vec<PendingRow> of this pass
        for i in range(lo, hi):
            if kinds[i] not in "IUD" or int(slots[i]) != slot:
                continue
            members += 1
            why = refusal(kinds[i], int(flags[i]), engine, identity_type, n_ident, n_pk)
            if why:
                if failed is None:
                    failed = {"status": FAILED, "event": i, "reason": why, "fail_pass": w}
                continue
            if no_rows:
                continue
            r = bisect.bisect_left(row_event, i)
            if r >= len(row_event) or row_event[r] != i:
                if needs_host is None:
                    needs_host = {"status": NEEDS_HOST, "event": i, "fail_pass": w}
                continue
            pending.append(r)
        mine, k = [], 0                                                      # insert_rows (client.rs:578-600)
        while k < len(pending):
            nbytes, first = 0, k
            while nbytes < max_bytes and k < len(pending):
                nbytes += offs[pending[k] + 1] - offs[pending[k]]
                k += 1
            a, e = pending[first], pending[k - 1]
            mine.append({"window": w, "first_row": a, "end_row": e + 1, "first_event": row_event[a], "last_event": row_event[e],
                         "byte_first": offs[a], "byte_end": offs[e + 1], "_rows": pending[first:k], "_bytes": nbytes})
        end_row = bisect.bisect_left(row_event, hi)
        wins.append({"stmt_first": len(stmts), "n_stmts": len(mine), "first_row": pending[0] if pending else end_row, "end_row": end_row,
                     "n_members": members, "n_bytes": sum(s["_bytes"] for s in mine)})
        stmts += mine
        n_members += members
    if failed is not None:
        return failed
    if no_rows:
        return {"status": NEEDS_HOST, "event": needs_host_event, "fail_pass": NONE}
    if needs_host is not None:
        return needs_host
    for s in stmts:                                                          # what the INSERT of one byte range rests on: consecutive rows
        assert s["_rows"] == list(range(s["first_row"], s["end_row"])) and s["_bytes"] == s["byte_end"] - s["byte_first"]
    info = {"n_stmts": len(stmts), "n_members": n_members, "n_rows": n_members, "n_bytes": sum(wn["n_bytes"] for wn in wins)}
    return {"status": OK, "info": info, "statements": stmts, "windows": wins}


def of_host_batch(hb):
    """(kinds, flags, slots) of an oracle host batch (etl_amd.view.HostBatch)."""
    import numpy as np
    kinds = "".join(chr(k) for k in hb.kind.tolist())
    return kinds, np.asarray(hb.flags), np.asarray(hb.schema_slot)
