"""TEST INFRASTRUCTURE — host model of etlg_bigquery_plan (include/etlg.h): the BigQuery sink's append requests of one schema slot.
It restates the reference as the plain sequential loop it is: per window one turn of write_events' outer loop
(crates/etl-destinations/src/bigquery/core.rs:959-1040) with its refusals in their own order — bigquery_update_new_row :1478-1494,
bigquery_update_rows :1425-1476 with ensure_bigquery_update_without_old_row_can_skip_delete :1516-1534, bigquery_primary_key_changed
:1557-1644, bigquery_delete_old_row :1497-1512, bigquery_primary_key_tagged_cells_from_old_row :1647-1739 and
ensure_bigquery_key_image_matches_primary_key :1537-1554 — and, for the rows the turn gathered, the one create_append_request of the
table (:1043-1064). An event's rows are looked up one event at a time (an Update that changed the primary key has two); no prefix
sums and no lower bounds over windows: the device code is written the other way round and tests/test_gpu_bigquery_plan.py compares
the two field by field.
The table-copy path is two functions of the reference restated line by line: calculate_target_batches_for_table_copy (:1760-1784) and
split_table_rows (:1790-1827); tests/test_bigquery_plan_model.py holds them against the reference's own vectors
(tests/golden/bigquery_split_kats.py)."""
import bisect

NONE = (1 << 64) - 1
OK, BAD_PASSES, FAILED, NEEDS_HOST = range(4)
R_PARTIAL_UPDATE, R_UPDATE_NO_OLD_IDENTITY, R_KEY_WIDTH, R_KEY_IDENTITY, R_DELETE_NO_OLD = 1, 2, 3, 4, 5
OLD_NONE, OLD_FULL, OLD_KEY, FLAG_PARTIAL = 0, 1, 2, 4
REQ_FIELDS = ("window", "first_row", "end_row", "first_event", "last_event", "byte_first", "byte_end", "n_members")
WIN_FIELDS = ("req_first", "n_reqs", "first_row", "end_row", "n_members", "n_two_row", "n_bytes")
INFO_FIELDS = ("n_reqs", "n_members", "n_rows", "n_two_row", "n_bytes", "est_row_bytes", "target_batches")


def key_image_refusal(identity_type, n_ident, n_pk):
    """OldTableRow::Key in bigquery_primary_key_changed (:1599-1616) and in bigquery_primary_key_tagged_cells_from_old_row (:1680-1696):
    the width first, then the identity."""
    if n_ident != n_pk:
        return R_KEY_WIDTH
    if identity_type != "PrimaryKey":
        return R_KEY_IDENTITY
    return 0


def refusal(kind, fl, identity_type, n_ident, n_pk):
    """What write_events raises at one event of the table, 0 for none; the tests in the reference's order."""
    old = fl & 3
    if kind == "U":
        if fl & FLAG_PARTIAL:                                                # :1000 bigquery_update_new_row, before the old image is looked at
            return R_PARTIAL_UPDATE
        if old == OLD_NONE:                                                  # :1439-1442
            return 0 if identity_type == "PrimaryKey" else R_UPDATE_NO_OLD_IDENTITY
        if old == OLD_KEY:                                                   # :1437 -> :1599-1616
            return key_image_refusal(identity_type, n_ident, n_pk)
    if kind == "D":
        if old == OLD_NONE:                                                  # :1020 bigquery_delete_old_row
            return R_DELETE_NO_OLD
        if old == OLD_KEY:                                                   # :1029 -> :1749 -> :1680-1696
            return key_image_refusal(identity_type, n_ident, n_pk)
    return 0


def plan(kinds, flags, slots, slot, windows, row_event, row_len, identity_type="PrimaryKey", n_ident=1, n_pk=1, needs_host_event=None):
    """kinds: one letter per event; flags, slots: per event; windows: [(first_event, data_end)]; row_event / row_len: the protobuf
    object's rows (ascending events, an event may own two) and their lengths; identity_type, n_ident, n_pk: the slot's;
    needs_host_event: the object came back NEEDS_HOST with this host_event and has no rows. Returns {"status", ...} as info does."""
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
    reqs, wins = [], []
    for w, (lo, hi) in enumerate(windows):
        table_rows, members = [], 0                                          # the table's Vec<BigQueryTableRow> of this turn
        for i in range(lo, hi):
            if kinds[i] not in "IUD" or int(slots[i]) != slot:
                continue
            members += 1
            why = refusal(kinds[i], int(flags[i]), identity_type, n_ident, n_pk)
            if why:
                if failed is None:
                    failed = {"status": FAILED, "event": i, "reason": why, "fail_pass": w}
                continue
            if no_rows:
                continue
            mine = [r for r in range(bisect.bisect_left(row_event, i), len(row_event)) if row_event[r] == i][:2]   # entry.1.push / .extend
            if not mine:
                if needs_host is None:
                    needs_host = {"status": NEEDS_HOST, "event": i, "fail_pass": w}
                continue
            table_rows += mine
        end_row = bisect.bisect_left(row_event, hi)
        nbytes = sum(offs[r + 1] - offs[r] for r in table_rows)
        wn = {"req_first": len(reqs), "n_reqs": 1 if members else 0, "first_row": table_rows[0] if table_rows else end_row, "end_row": end_row,
              "n_members": members, "n_two_row": len(table_rows) - members if members else 0, "n_bytes": nbytes}
        if members and table_rows:                                           # :1043-1064: one create_append_request of all the table's rows
            a, e = table_rows[0], table_rows[-1]
            reqs.append({"window": w, "first_row": a, "end_row": e + 1, "first_event": row_event[a], "last_event": row_event[e],
                         "byte_first": offs[a], "byte_end": offs[e + 1], "n_members": members, "_rows": table_rows, "_bytes": nbytes})
        wins.append(wn)
    if failed is not None:
        return failed
    if no_rows:
        return {"status": NEEDS_HOST, "event": needs_host_event, "fail_pass": NONE}
    if needs_host is not None:
        return needs_host
    for s in reqs:                                                           # what one byte range per request rests on: consecutive rows
        assert s["_rows"] == list(range(s["first_row"], s["end_row"])) and s["_bytes"] == s["byte_end"] - s["byte_first"]
    info = {"n_reqs": len(reqs), "n_members": sum(wn["n_members"] for wn in wins), "n_rows": sum(len(s["_rows"]) for s in reqs),
            "n_two_row": sum(wn["n_two_row"] for wn in wins), "n_bytes": sum(wn["n_bytes"] for wn in wins), "est_row_bytes": 0, "target_batches": 0}
    return {"status": OK, "info": info, "requests": reqs, "windows": wins}


def div_ceil(a, b):
    return -(-a // b)


def calculate_target_batches_for_table_copy(row_lens, max_batch_size_bytes):
    """core.rs:1760-1784, line by line; row_lens: encoded_len() of every row."""
    if not row_lens:                                                         # let Some(encoded_row) = table_rows.first() else { return Ok(0) }
        return 0
    total_rows = len(row_lens)
    estimated_row_size = int(row_lens[0])
    rows_per_batch = max_batch_size_bytes // estimated_row_size if estimated_row_size else total_rows   # checked_div(..).unwrap_or(total_rows)
    return div_ceil(total_rows, rows_per_batch) if rows_per_batch > 0 else 1


def split_table_rows(total_rows, target_batches):
    """core.rs:1790-1827, line by line -> the batches' lengths."""
    if total_rows == 0:
        return []
    if total_rows <= 1 or target_batches == 1 or total_rows <= target_batches:
        return [total_rows]
    optimal_rows_per_batch = div_ceil(total_rows, target_batches)
    if optimal_rows_per_batch == 0:
        return [total_rows]
    num_sub_batches = div_ceil(total_rows, optimal_rows_per_batch)
    rows_per_sub_batch = total_rows // num_sub_batches
    extra_rows = total_rows % num_sub_batches
    batches, remaining = [], total_rows
    for i in range(num_sub_batches):
        batch_size = rows_per_sub_batch + (1 if i < extra_rows else 0)
        remaining -= batch_size                                              # remaining.split_off(batch_size)
        batches.append(batch_size)
    assert remaining == 0
    return batches


def plan_copy(row_event, row_len, max_batch_bytes, needs_host_event=None):
    """A table-copy batch (write_table_rows :602-649): one window over all rows, the requests split_table_rows cuts."""
    assert 1 <= max_batch_bytes <= 1 << 63
    if needs_host_event is not None:
        return {"status": NEEDS_HOST, "event": needs_host_event, "fail_pass": NONE}
    lens = [int(x) for x in row_len]
    offs = [0]
    for ln in lens:
        offs.append(offs[-1] + ln)
    target = calculate_target_batches_for_table_copy(lens, max_batch_bytes)
    reqs, a = [], 0
    for ln in split_table_rows(len(lens), target):
        reqs.append({"window": 0, "first_row": a, "end_row": a + ln, "first_event": int(row_event[a]), "last_event": int(row_event[a + ln - 1]),
                     "byte_first": offs[a], "byte_end": offs[a + ln], "n_members": ln})
        a += ln
    assert a == len(lens)
    wins = [{"req_first": 0, "n_reqs": len(reqs), "first_row": 0, "end_row": len(lens), "n_members": len(lens), "n_two_row": 0, "n_bytes": offs[-1]}]
    info = {"n_reqs": len(reqs), "n_members": len(lens), "n_rows": len(lens), "n_two_row": 0, "n_bytes": offs[-1],
            "est_row_bytes": lens[0] if lens else 0, "target_batches": target}
    return {"status": OK, "info": info, "requests": reqs, "windows": wins}


def of_host_batch(hb):
    """(kinds, flags, slots) of an oracle host batch (etl_amd.view.HostBatch)."""
    import numpy as np
    kinds = "".join(chr(k) for k in hb.kind.tolist())
    return kinds, np.asarray(hb.flags), np.asarray(hb.schema_slot)
