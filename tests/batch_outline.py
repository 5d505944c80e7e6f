"""TEST INFRASTRUCTURE — host model of etlg_batch_outline (include/etlg.h): the pass plan of the destinations' write_events loops. It
restates crates/etl-destinations/src/clickhouse/core.rs:1063-1164 as the plain sequential loop it is — peek, collect Insert / Update /
Delete rows per table until a Relation or a Truncate, consume the run of Relations, consume the run of Truncates, start over — once per
write_events range; `relations_inline` is Iceberg's loop (iceberg/core.rs:300-432), which breaks at Truncate only and meets Relation
events inside the data run. No flags, no scans: the device code is written the other way round and tests/test_gpu_batch_outline.py
compares the two field by field. The reference's tests state no pass boundary as a number, so there is no vector to transcribe;
tests/test_batch_outline_model.py checks this restatement against hand-written expectations."""
import struct

import numpy as np

NONE = (1 << 64) - 1
OK, BAD_CUTS = 0, 1
PASS_FIELDS = ("first_event", "data_end", "rel_end", "end_event", "range", "trunc_first", "n_trunc")
INFO_FIELDS = ("n_passes", "n_trunc", "n_relations", "n_rows", "n_ranges")
OLD_FULL, OLD_KEY, FLAG_PARTIAL = 1, 2, 4


def category(kind, flags):
    """0 Insert, 1 Update with a full new row, 2 partial Update, 3 Delete with the full old row, 4 Delete by key, 5 Delete without an old row."""
    if kind == "I":
        return 0
    if kind == "U":
        return 2 if flags & FLAG_PARTIAL else 1
    return {OLD_FULL: 3, OLD_KEY: 4}.get(flags & 3, 5)


def ranges_of(first, end, cuts):
    """The write_events ranges [(lo, hi)] of the window, or the index of the first cut that is outside [first, end] or below its predecessor."""
    out, lo = [], first
    for k, c in enumerate(cuts):
        if c < first or c > end or c < lo:
            return None, k
        out.append((lo, c))
        lo = c
    if not cuts or lo < end:
        out.append((lo, end))
    return out, None


def outline(kinds, flags, slots, trunc_bodies, first=0, end=None, cuts=(), relations_inline=False):
    """kinds: a str / sequence of one-letter kinds per event; flags, slots: per event; trunc_bodies: {event: [(table_id, schema_slot)]}.
    Returns {"status", "bad_cut"} for bad cuts, else {"status", "info", "passes", "touched" (per pass: the set of slots), "rows" (per pass:
    {slot: [events]}), "truncates" [(table_id, schema_slot, event)], "census" {slot: (rows[6], first[6])}}."""
    end = len(kinds) if end is None else end
    rngs, bad = ranges_of(first, end, list(cuts))
    if rngs is None:
        return {"status": BAD_CUTS, "bad_cut": bad}
    passes, rows, truncs, census = [], [], [], {}
    n_rel = n_rows = 0
    for r, (lo, hi) in enumerate(rngs):
        i = lo
        while i < hi:                                                        # while event_iter.peek().is_some()
            p = {"first_event": i, "range": r, "trunc_first": len(truncs)}
            pending = {}
            while i < hi and kinds[i] != "T" and (relations_inline or kinds[i] != "R"):
                k = kinds[i]
                if k in "IUD":
                    pending.setdefault(int(slots[i]), []).append(i)
                    n_rows += 1
                    cr, cf = census.setdefault(int(slots[i]), ([0] * 6, [NONE] * 6))
                    c = category(k, int(flags[i]))
                    cr[c] += 1
                    cf[c] = min(cf[c], i)
                elif k == "R":
                    n_rel += 1
                i += 1
            p["data_end"] = i                                                # flush_pending_rows(pending)
            while i < hi and kinds[i] == "R":                                # (never entered with relations_inline: the data run took them)
                n_rel += 1
                i += 1
            p["rel_end"] = i
            while i < hi and kinds[i] == "T":
                truncs += [(t, s, i) for t, s in trunc_bodies.get(i, [])]
                i += 1
            p["end_event"], p["n_trunc"] = i, len(truncs) - p["trunc_first"]
            passes.append(p)
            rows.append(pending)
    info = {"n_passes": len(passes), "n_trunc": len(truncs), "n_relations": n_rel, "n_rows": n_rows, "n_ranges": len(rngs)}
    return {"status": OK, "info": info, "passes": passes, "touched": [set(r) for r in rows], "rows": rows, "truncates": truncs, "census": census}


def truncated_tables(model, p):
    """The tables pass p truncates: the first entry per table_id (HashMap::entry().or_insert(), clickhouse/core.rs:1148-1155)."""
    ps, seen = model["passes"][p], {}
    for t, s, e in model["truncates"][ps["trunc_first"]:ps["trunc_first"] + ps["n_trunc"]]:
        seen.setdefault(t, (t, s, e))
    return list(seen.values())


def of_host_batch(hb):
    """(kinds, flags, slots, trunc_bodies) of an oracle host batch (etl_amd.view.HostBatch)."""
    kinds = "".join(chr(k) for k in hb.kind.tolist())
    fx = hb.fixed.tobytes()
    bodies = {i: [struct.unpack_from("<II", fx, int(hb.body_off[i]) + 8 * j) for j in range(int(hb.table_id[i]))] for i, k in enumerate(kinds) if k == "T"}
    return kinds, np.asarray(hb.flags), np.asarray(hb.schema_slot), bodies
