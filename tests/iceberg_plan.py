"""TEST INFRASTRUCTURE — host model of etlg_iceberg_plan (include/etlg.h): the Iceberg sink's writes of one schema slot and the Arrow
slices of the changelog object's columns over each write's rows. It restates the reference as the plain sequential loop it is: per
window one turn of write_events' outer loop (crates/etl-destinations/src/iceberg/core.rs:300-416) — the inner loop that breaks at a
Truncate only (:310-312), iceberg_update_row (:636-652) and iceberg_delete_row (:655-680) at every Update and Delete, and the one
insert_rows of the table (:395-409) — and write_table_rows (:268-291) for a table-copy batch. An event's row is looked up one event at
a time and a slice's counts are numpy counts over the unpacked bits of the row range; no prefix sums, no popcounts of words and no
lower bounds over windows: the device code is written the other way round and tests/test_gpu_iceberg_plan.py compares the two field
by field. ones_in_range is the closed form of the device's arithmetic over packed 64-bit words, held against the unpacked counts by
tests/test_iceberg_plan_model.py."""
import bisect

import numpy as np

NONE = (1 << 64) - 1
OK, BAD_PASSES, FAILED, NEEDS_HOST = range(4)
PARTIAL_UPDATE, KEY_ONLY_DELETE, DELETE_WITHOUT_OLD_ROW = 1, 2, 3             # ETLG_ICE_*
DESCRIPTION = {PARTIAL_UPDATE: "Iceberg update requires a full new row image", KEY_ONLY_DELETE: "Iceberg delete requires a full old row image",
               DELETE_WITHOUT_OLD_ROW: "Iceberg delete requires an old row image"}   # core.rs:644, :663, :672
OLD_NONE, OLD_FULL, OLD_KEY, FLAG_PARTIAL = 0, 1, 2, 4
AK_BOOLEAN, AK_FIXED16, AK_LARGE_UTF8, AK_LARGE_BINARY, AK_TEXT_FORM, AK_LIST = 0, 9, 10, 11, 12, 13
WIDTH = {1: 4, 2: 8, 3: 4, 4: 8, 5: 4, 6: 8, 7: 8, 8: 8, 9: 16}               # the fixed-width etlg_arrow_kind values
WRITE_FIELDS = ("window", "first_row", "end_row", "first_event", "last_event", "n_members", "other_slot_event")
WIN_FIELDS = ("write_first", "n_writes", "first_row", "end_row", "n_members", "other_slot_event")
SLICE_FIELDS = ("null_count", "deferred_count", "byte_first", "byte_end", "child_first", "child_end", "child_null_count")
INFO_FIELDS = ("n_writes", "n_members", "n_rows", "n_mixed")


def iceberg_update_row(image):
    """core.rs:636-652: image "full" | "partial" -> 0, or the reason."""
    return 0 if image == "full" else PARTIAL_UPDATE


def iceberg_delete_row(image):
    """core.rs:655-680: image "full" | "key" | "none" -> 0, or the reason."""
    return {"full": 0, "key": KEY_ONLY_DELETE, "none": DELETE_WITHOUT_OLD_ROW}[image]


def refusal(kind, fl):
    """What write_events raises at one event, 0 for none: one test per event kind (:332-350)."""
    if kind == "U":
        return iceberg_update_row("partial" if fl & FLAG_PARTIAL else "full")
    if kind == "D":
        return iceberg_delete_row({OLD_FULL: "full", OLD_KEY: "key", OLD_NONE: "none"}[fl & 3])
    return 0


def column_slice(col, r0, r1):
    """The Arrow slice of one column over rows [r0, r1). col: {"kind", "value_bytes", "validity", "deferred": bool arrays per row,
    "offsets", and for a list "child_kind", "child_validity", "child_offsets", "child_count"}."""
    k = col["kind"]
    s = dict.fromkeys(SLICE_FIELDS, 0)
    s["null_count"] = int(np.count_nonzero(~col["validity"][r0:r1]))
    s["deferred_count"] = int(np.count_nonzero(col["deferred"][r0:r1]))
    if k == AK_LIST:
        c0, c1 = int(col["offsets"][r0]), int(col["offsets"][r1])
        s["child_first"], s["child_end"] = c0, c1
        s["child_null_count"] = int(np.count_nonzero(~col["child_validity"][c0:c1]))
        ck = col["child_kind"]
        if ck in WIDTH:
            s["byte_first"], s["byte_end"] = c0 * WIDTH[ck], c1 * WIDTH[ck]
        elif ck == AK_BOOLEAN:
            s["byte_first"], s["byte_end"] = c0, c1
        elif col["child_count"]:
            s["byte_first"], s["byte_end"] = int(col["child_offsets"][c0]), int(col["child_offsets"][c1])
    elif k in WIDTH:
        s["byte_first"], s["byte_end"] = r0 * col["value_bytes"], r1 * col["value_bytes"]
    elif k == AK_BOOLEAN:
        s["byte_first"], s["byte_end"] = r0, r1
    else:
        assert k in (AK_LARGE_UTF8, AK_LARGE_BINARY, AK_TEXT_FORM), k
        s["byte_first"], s["byte_end"] = int(col["offsets"][r0]), int(col["offsets"][r1])
    return s


def plan(kinds, flags, slots, tables, slot, table_id, windows, row_event, columns):
    """kinds: one letter per event; flags, slots, tables: per event; windows: [(first_event, data_end)]; row_event: the changelog
    object's rows (ascending events, one row per event); columns: its columns as column_slice takes them. Returns {"status", ...}."""
    n = len(kinds)
    for p, (lo, hi) in enumerate(windows):
        if lo > hi or hi > n or (p and lo < windows[p - 1][1]):
            return {"status": BAD_PASSES, "bad_pass": p}
    row_event = [int(e) for e in row_event]
    failed = needs_host = None
    writes, wins, slices = [], [], []
    for w, (lo, hi) in enumerate(windows):
        table_rows, members, other = [], 0, NONE                              # the (schema, rows) entry of the slot's table in this turn
        for i in range(lo, hi):
            if kinds[i] not in "IUD":
                continue
            if int(slots[i]) != slot:
                if int(tables[i]) == table_id and other == NONE:             # the same HashMap key under another schema (:304-307)
                    other = i
                continue
            members += 1
            why = refusal(kinds[i], int(flags[i]))
            if why:
                if failed is None:
                    failed = {"status": FAILED, "event": i, "reason": why, "fail_pass": w}
                continue
            r = bisect.bisect_left(row_event, i)
            if r == len(row_event) or row_event[r] != i:
                if needs_host is None:
                    needs_host = {"status": NEEDS_HOST, "event": i, "fail_pass": w}
                continue
            table_rows.append(r)
        end_row = bisect.bisect_left(row_event, hi)
        if not members:                                                      # the table's entry of this turn is not this slot's: nothing is mixed
            other = NONE
        wins.append({"write_first": len(writes), "n_writes": 1 if members else 0, "first_row": table_rows[0] if table_rows else end_row, "end_row": end_row,
                     "n_members": members, "other_slot_event": other})
        if members and table_rows:                                           # :395-409: one insert_rows of all the table's rows
            a, e = table_rows[0], table_rows[-1]
            writes.append({"window": w, "first_row": a, "end_row": e + 1, "first_event": row_event[a], "last_event": row_event[e], "n_members": members,
                           "other_slot_event": other, "_rows": table_rows})
    if failed is not None:
        return failed
    if needs_host is not None:
        return needs_host
    for s in writes:                                                         # what one row range per write rests on: consecutive rows, one per member
        assert s["_rows"] == list(range(s["first_row"], s["end_row"])) and len(s["_rows"]) == s["n_members"]
        slices.append([column_slice(c, s["first_row"], s["end_row"]) for c in columns])
    info = {"n_writes": len(writes), "n_members": sum(wn["n_members"] for wn in wins), "n_rows": sum(len(s["_rows"]) for s in writes),
            "n_mixed": sum(1 for wn in wins if wn["other_slot_event"] != NONE)}
    return {"status": OK, "info": info, "writes": writes, "windows": wins, "slices": slices}


def plan_copy(row_event, columns):
    """A table-copy batch (write_table_rows :268-291): one window over all rows, one write unless table_rows.is_empty()."""
    R = len(row_event)
    writes = [{"window": 0, "first_row": 0, "end_row": R, "first_event": int(row_event[0]), "last_event": int(row_event[R - 1]), "n_members": R,
               "other_slot_event": NONE}] if R else []
    wins = [{"write_first": 0, "n_writes": len(writes), "first_row": 0, "end_row": R, "n_members": R, "other_slot_event": NONE}]
    info = {"n_writes": len(writes), "n_members": R, "n_rows": R, "n_mixed": 0}
    return {"status": OK, "info": info, "writes": writes, "windows": wins, "slices": [[column_slice(c, 0, R) for c in columns] for _ in writes]}


def pack_bits(bits):
    """A bool array as the 64-bit words of an Arrow bitmap, LSB first, padded to a whole word with zeros."""
    b = np.zeros((len(bits) + 63) // 64 * 64, dtype=np.uint8)
    b[:len(bits)] = np.asarray(bits, dtype=np.uint8)
    return np.packbits(b, bitorder="little").view(np.uint64)


def ones_in_range(words, lo, hi):
    """The device's arithmetic over packed words, in closed form: set bits in the bit range [lo, hi) as the whole words in
    [lo // 64, hi // 64) — a prefix difference on the device — less the low lo % 64 bits of word lo // 64, plus the low hi % 64 bits of
    word hi // 64. A word is looked at only where the range cuts it: hi on a word boundary reads nothing at or behind words[hi // 64]."""
    pop = lambda x: bin(int(x)).count("1")
    pre = [0]
    for x in words:
        pre.append(pre[-1] + pop(x))
    n = pre[hi >> 6] - pre[lo >> 6]
    if lo & 63:
        n -= pop(int(words[lo >> 6]) & ((1 << (lo & 63)) - 1))
    if hi & 63:
        n += pop(int(words[hi >> 6]) & ((1 << (hi & 63)) - 1))
    return n


def of_host_batch(hb):
    """(kinds, flags, slots, tables) of an oracle host batch (etl_amd.view.HostBatch)."""
    kinds = "".join(chr(k) for k in hb.kind.tolist())
    return kinds, np.asarray(hb.flags), np.asarray(hb.schema_slot), np.asarray(hb.table_id)
