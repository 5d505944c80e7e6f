"""TEST INFRASTRUCTURE — host model of etlg_snowflake_plan (include/etlg.h): the Snowflake sink's row batches of one schema slot. It
restates the reference as the plain sequential loop it is: per window a fresh RowBatchBuilder (accumulate_data_events,
crates/etl-destinations/src/snowflake/core.rs:279-303), per event encode_insert / encode_update / encode_delete in their own order
(:345-438, with snowflake_update_row :572-588 and snowflake_delete_row :591-608) and RowBatchBuilder::push_row (streaming/batch.rs:
150-189) with its byte counter that resets at a flush. No prefix sums, no jump tables: the device code is written the other way round
and tests/test_gpu_snowflake_plan.py compares the two field by field.
The reference's own tests state no flush position as a number (batch.rs:272-373 assert row counts, the offset range and the oversize
error), so there are no vectors to transcribe; tests/test_snowflake_plan_model.py checks this loop against hand-worked cases, the
facts those tests do state, and the closed form of the segment rule."""
import bisect

NONE = (1 << 64) - 1
OK, BAD_PASSES, FAILED, NOT_PREFIX, NEEDS_HOST = range(5)
R_PARTIAL_UPDATE, R_DELETE_NO_OLD, R_ROW_TOO_LARGE = 1, 2, 3
OLD_NONE, OLD_FULL, OLD_KEY, FLAG_PARTIAL = 0, 1, 2, 4
MAX_UNFLUSHED_BYTES = 128 * 1024                                             # batch.rs:26
MAX_ROW_BYTES = 2 * 1024 * 1024                                              # batch.rs:31 (MAX_UNCOMPRESSED_ROW_BYTES)
SEG_FIELDS = ("window", "first_row", "end_row", "first_event", "last_event", "byte_first", "byte_end", "first_row_bytes",
              "first_commit_lsn", "first_tx_ordinal", "last_commit_lsn", "last_tx_ordinal", "flush_before")
WIN_FIELDS = ("seg_first", "n_segs", "first_row", "end_row", "n_members", "n_retained", "n_bytes")
INFO_FIELDS = ("n_segs", "n_members", "n_retained", "n_dropped", "n_rows", "n_bytes")


def token(key):
    """OffsetToken's string form (streaming/offset_token.rs:21-23)."""
    return "%016x/%016x" % (key[0], key[1])


def is_committed(committed, key):
    """streaming/channel.rs:175-177: committed_offset >= offset, on the tokens' strings."""
    return committed is not None and token(tuple(committed)) >= token(key)


def plan(kinds, flags, slots, commit, ordinal, slot, windows, row_event, row_len, committed=None, flush_bytes=MAX_UNFLUSHED_BYTES,
         max_row_bytes=MAX_ROW_BYTES, zero_keys=False, needs_host_event=None):
    """kinds: one letter per event; flags, slots, commit, ordinal: per event; windows: [(first_event, data_end)]; row_event / row_len:
    the NDJSON object's rows (ascending events) and their lengths with the '\\n'; needs_host_event: the object came back NEEDS_HOST
    with this host_event and has no rows. zero_keys: a table-copy batch. Returns {"status", ...} as info does."""
    n = len(kinds)
    for p, (lo, hi) in enumerate(windows):
        if lo > hi or hi > n or (p and lo < windows[p - 1][1]):
            return {"status": BAD_PASSES, "bad_pass": p}
    no_rows = needs_host_event is not None
    row_event = [] if no_rows else [int(e) for e in row_event]
    offs = [0]
    for ln in ([] if no_rows else row_len):
        offs.append(offs[-1] + int(ln))
    keys = [(0, 0) if zero_keys else (int(commit[i]), int(ordinal[i])) for i in range(n)]
    failed = not_prefix = needs_host = None
    segs, wins = [], []
    n_members = n_retained = 0
    for w, (lo, hi) in enumerate(windows):
        since_flush, mine, pushed, members, seen_retained = 0, [], [], 0, False
        for i in range(lo, hi):
            if kinds[i] not in "IUD" or int(slots[i]) != slot:
                continue
            members += 1
            fl = int(flags[i])
            why = 0
            if kinds[i] == "U" and fl & FLAG_PARTIAL:                        # snowflake_update_row, in front of the offset test
                why = R_PARTIAL_UPDATE
            elif is_committed(committed, keys[i]):                           # the three encode_* functions: the event is dropped
                if seen_retained and not_prefix is None:
                    not_prefix = i
                continue
            elif kinds[i] == "D" and fl & 3 == OLD_NONE:                     # snowflake_delete_row, behind the offset test
                why = R_DELETE_NO_OLD
            if why:
                if failed is None:
                    failed = {"status": FAILED, "event": i, "reason": why, "row_bytes": 0}
                if not is_committed(committed, keys[i]):
                    seen_retained = True
                continue
            seen_retained = True
            if no_rows:
                pushed.append(None)
                continue
            r = bisect.bisect_left(row_event, i)
            if r >= len(row_event) or row_event[r] != i:
                if needs_host is None:
                    needs_host = i
                continue
            ln = offs[r + 1] - offs[r]
            if ln > max_row_bytes:                                           # push_row: batch.rs:160
                if failed is None:
                    failed = {"status": FAILED, "event": i, "reason": R_ROW_TOO_LARGE, "row_bytes": ln}
                continue
            flush = since_flush + ln >= flush_bytes                          # batch.rs:166
            if flush:
                since_flush = 0
            if flush or not mine:
                mine.append({"window": w, "first_row": r, "end_row": r, "first_event": i, "byte_first": offs[r], "first_row_bytes": ln,
                             "first_commit_lsn": keys[i][0], "first_tx_ordinal": keys[i][1], "flush_before": 1 if flush else 0})
            since_flush += ln
            mine[-1].update({"end_row": r + 1, "last_event": i, "byte_end": offs[r + 1], "last_commit_lsn": keys[i][0], "last_tx_ordinal": keys[i][1]})
            pushed.append(r)
        kept = len(pushed)                                                   # (every retained member, when the status is OK)
        end_row = bisect.bisect_left(row_event, hi)
        first_row = pushed[0] if pushed and pushed[0] is not None else end_row
        wins.append({"seg_first": len(segs), "n_segs": len(mine), "first_row": first_row, "end_row": end_row, "n_members": members,
                     "n_retained": kept, "n_bytes": sum(s["byte_end"] - s["byte_first"] for s in mine)})
        segs += mine
        n_members += members
        n_retained += kept
    if failed is not None:
        return failed
    if not_prefix is not None:
        return {"status": NOT_PREFIX, "event": not_prefix}
    if no_rows:
        return {"status": NEEDS_HOST, "event": needs_host_event}
    if needs_host is not None:
        return {"status": NEEDS_HOST, "event": needs_host}
    for s in segs:                                                            # what the write_all of one byte range rests on
        assert row_event[s["first_row"]] == s["first_event"] and row_event[s["end_row"] - 1] == s["last_event"]
    info = {"n_segs": len(segs), "n_members": n_members, "n_retained": n_retained, "n_dropped": n_members - n_retained, "n_rows": n_retained,
            "n_bytes": sum(wn["n_bytes"] for wn in wins)}
    return {"status": OK, "info": info, "segments": segs, "windows": wins}


def of_host_batch(hb):
    """(kinds, flags, slots, commit, ordinal) of an oracle host batch (etl_amd.view.HostBatch)."""
    import numpy as np
    kinds = "".join(chr(k) for k in hb.kind.tolist())
    return kinds, np.asarray(hb.flags), np.asarray(hb.schema_slot), np.asarray(hb.commit_lsn), np.asarray(hb.tx_ordinal)
