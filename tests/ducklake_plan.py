"""TEST INFRASTRUCTURE — host model of etlg_ducklake_plan (include/etlg.h): the DuckLake sink's atomic batches of one schema slot. It
restates the reference as the three plain loops it is — retain_mutations_after_sequence_key (crates/etl-destinations/src/ducklake/
batches.rs:932-946), prepare_mutation_table_batches (:727-758, chunks of CDC_MUTATION_BATCH_SIZE) and prepare_table_mutations
(:1128-1226, with its two pending lists) — once per window, the window being one segment of write_events_inner (core.rs:1815-1947). No
ranks, no scans: the device code is written the other way round and tests/test_gpu_ducklake_plan.py compares the two field by field.
tests/test_ducklake_plan_model.py checks this restatement against the reference's own vectors (tests/golden/ducklake_plan_kats.json)."""
import bisect

import numpy as np

NONE = (1 << 64) - 1
OK, BAD_PASSES, REFUSED, NOT_PREFIX, NEEDS_HOST = range(5)
R_UPDATE_IDENTITY, R_DELETE_IDENTITY, R_DELETE_NO_OLD = 1, 2, 3
REASON_TEXT = {R_UPDATE_IDENTITY: "DuckLake update requires a replica identity", R_DELETE_IDENTITY: "DuckLake delete requires a replica identity",
               R_DELETE_NO_OLD: "DuckLake delete requires an old row image"}
INSERT, UPDATE_FULL, REPLACE, UPDATE_PARTIAL, DELETE = range(5)
UPSERT, OP_DELETE, OP_UPDATE = range(3)
O_NONE, O_DELETE, O_UPDATE, O_REPLACE = range(4)
ORIGIN_TEXT = {O_NONE: None, O_DELETE: "delete", O_UPDATE: "update", O_REPLACE: "replace"}
OLD_NONE, OLD_FULL, OLD_KEY, FLAG_PARTIAL = 0, 1, 2, 4
BATCH_SIZE = 16                                                              # CDC_MUTATION_BATCH_SIZE, batches.rs:79
BATCH_FIELDS = ("first_event", "end_event", "first_start_lsn", "last_commit_lsn", "first_commit_lsn", "first_tx_ordinal", "last_tx_ordinal",
                "window", "op_first", "n_members", "n_ops")
INFO_FIELDS = ("n_batches", "n_ops", "n_members", "n_retained", "n_dropped")


def category(kind, flags):
    if kind == "I":
        return INSERT
    if kind == "U":
        return UPDATE_PARTIAL if flags & FLAG_PARTIAL else REPLACE if flags & 3 == OLD_NONE else UPDATE_FULL
    return DELETE


def refusal(kind, flags, n_ident):
    """validate_ducklake_replica_identity first (core.rs:371-392), then the Delete's old row (:1919-1929)."""
    if kind == "U" and n_ident == 0:
        return R_UPDATE_IDENTITY
    if kind == "D":
        return R_DELETE_IDENTITY if n_ident == 0 else R_DELETE_NO_OLD if flags & 3 == OLD_NONE else 0
    return 0


def retain(members, keys, watermark):
    """retain_mutations_after_sequence_key: tuples compare lexicographically, as compare_sequence_keys does."""
    if watermark is None:
        return list(members)
    return [i for i in members if keys[i] > tuple(watermark)]


def prepare_table_mutations(cats):
    """[(member index, category)] of one atomic batch -> [(kind, origin, first member index, n)], the reference's loop with its two
    pending lists: an Insert flushes the pending Deletes, a Delete the pending Inserts, an Update / Replace both."""
    out, upsert_rows, delete_predicates = [], [], []

    def flush_upserts():
        if upsert_rows:
            out.append((UPSERT, O_NONE, upsert_rows[0], len(upsert_rows)))
            upsert_rows.clear()

    def flush_deletes():
        if delete_predicates:
            out.append((OP_DELETE, O_DELETE, delete_predicates[0], len(delete_predicates)))
            delete_predicates.clear()

    for i, cat in cats:
        if cat == INSERT:
            flush_deletes()
            upsert_rows.append(i)
        elif cat == DELETE:
            flush_upserts()
            delete_predicates.append(i)
        else:
            flush_upserts()
            flush_deletes()
            if cat == UPDATE_PARTIAL:
                out.append((OP_UPDATE, O_NONE, i, 1))
            else:
                out.append((OP_DELETE, O_UPDATE if cat == UPDATE_FULL else O_REPLACE, i, 1))
                out.append((UPSERT, O_NONE, i, 1))
    flush_upserts()
    flush_deletes()
    return out


def _record(row_event, i):
    """(index, present) of event i's first record in an ascending row_event list."""
    at = bisect.bisect_left(row_event, i)
    return at, at < len(row_event) and row_event[at] == i


def plan(kinds, flags, slots, start, commit, ordinal, slot, windows, watermark=None, n_ident=1, tuples=None, predicates=None, updates=None):
    """kinds: one letter per event; flags, slots, start, commit, ordinal: per event; windows: [(first_event, data_end)]; tuples /
    predicates / updates: the row_event list of the object, None when it is not given. Returns {"status", ...} as info does."""
    n = len(kinds)
    for p, (lo, hi) in enumerate(windows):
        if lo > hi or hi > n or (p and lo < windows[p - 1][1]):
            return {"status": BAD_PASSES, "bad_pass": p}
    keys = [(int(commit[i]), int(ordinal[i])) for i in range(n)]
    segments = [[i for i in range(lo, hi) if kinds[i] in "IUD" and int(slots[i]) == slot] for lo, hi in windows]
    for seg in segments:                                                     # (windows ascend: the first refusal met is the lowest event)
        for i in seg:
            why = refusal(kinds[i], int(flags[i]), n_ident)
            if why:
                return {"status": REFUSED, "event": i, "reason": why}
    kept = [retain(seg, keys, watermark) for seg in segments]
    for seg, keep in zip(segments, kept):
        if keep:
            late = [i for i in seg if i > keep[0] and i not in set(keep)]
            if late:
                return {"status": NOT_PREFIX, "event": late[0]}
    objs = {"t": tuples, "p": predicates, "u": updates}
    needs = {INSERT: "t", UPDATE_FULL: "tp", REPLACE: "tp", UPDATE_PARTIAL: "u", DELETE: "p"}
    for keep in kept:
        for i in keep:
            for o in needs[category(kinds[i], int(flags[i]))]:
                if objs[o] is not None and not _record(objs[o], i)[1]:
                    return {"status": NEEDS_HOST, "event": i}
    batches, ops = [], []
    for w, keep in enumerate(kept):
        for at in range(0, len(keep), BATCH_SIZE):                           # prepare_mutation_table_batches: a batch per 16, and the rest
            mem = keep[at:at + BATCH_SIZE]
            cats = [(i, category(kinds[i], int(flags[i]))) for i in mem]
            mine = []
            for kind, origin, first, cnt in prepare_table_mutations(cats):
                obj = objs["u" if kind == OP_UPDATE else "t" if kind == UPSERT else "p"]
                mine.append({"kind": kind, "origin": origin, "first_event": first, "n": cnt, "rec_first": NONE if obj is None else _record(obj, first)[0]})
            first, last = mem[0], mem[-1]
            batches.append({"first_event": first, "end_event": last + 1, "first_start_lsn": int(start[first]), "last_commit_lsn": int(commit[last]),
                            "first_commit_lsn": keys[first][0], "first_tx_ordinal": keys[first][1], "last_tx_ordinal": keys[last][1], "window": w,
                            "op_first": len(ops), "n_members": len(mem), "n_ops": len(mine), "n_cat": [sum(1 for _, c in cats if c == k) for k in range(5)],
                            "members": mem})
            ops += mine
    n_members, n_kept = sum(len(s) for s in segments), sum(len(k) for k in kept)
    info = {"n_batches": len(batches), "n_ops": len(ops), "n_members": n_members, "n_retained": n_kept, "n_dropped": n_members - n_kept}
    return {"status": OK, "info": info, "batches": batches, "ops": ops}


def of_host_batch(hb):
    """(kinds, flags, slots, start, commit, ordinal) of an oracle host batch (etl_amd.view.HostBatch)."""
    kinds = "".join(chr(k) for k in hb.kind.tolist())
    return kinds, np.asarray(hb.flags), np.asarray(hb.schema_slot), np.asarray(hb.start_lsn), np.asarray(hb.commit_lsn), np.asarray(hb.tx_ordinal)
