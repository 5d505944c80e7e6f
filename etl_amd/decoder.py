"""Host-side mirror of the reference interface for the decode hot path.

`Decoder` is what the reference's `ApplyLoop` is to its codec: it owns the
per-stream transaction state and the shared table cache (inside the native
context), is primed with stored schemas / table states the way
`SchemaStore` / `StateStore` are (crates/etl/src/store/schema/base.rs:19-69,
crates/etl/src/store/state/base.rs:25-139), and turns batches of raw
logical-replication messages into the events `Destination::write_events`
would receive (crates/etl/src/destination/base.rs:207). All per-row work runs
in the gfx950 kernels of libetl_gfx950.so; this module only moves pointers.
"""
import ctypes as C

import numpy as np

from . import abi, native
from .view import HostBatch


class EtlError(Exception):
    """EtlError {kind, description, detail} (crates/etl/src/error.rs:27-76)."""

    def __init__(self, kind, code, description, detail, frame_index):
        self.kind, self.code, self.description, self.detail, self.frame_index = kind, code, description, detail, frame_index
        super().__init__(f"{abi.KIND_NAMES.get(kind, kind)}: {description} (frame {frame_index})")


def _ptr(a):
    return a.ctypes.data if a is not None else None


class Payload:
    """What Batch.payload returns: info (abi.PayloadInfo), hist, ev_bytes, sums — arrays, or the device addresses the caller gave."""

    def __init__(self, info, hist, ev_bytes, sums):
        self.info, self.hist, self.ev_bytes, self.sums = info, hist, ev_bytes, sums


TRUNC_DTYPE = np.dtype([("table_id", np.uint32), ("schema_slot", np.uint32), ("event", np.uint64)])   # etlg_outline_trunc
PASS_FIELDS = ("first_event", "data_end", "rel_end", "end_event", "range", "trunc_first", "n_trunc")    # etlg_outline_pass


class Outline:
    """What Batch.outline returns: info (abi.OutlineInfo) and, as arrays cut to what was written — or as the device addresses the caller
    gave —, passes (np.uint64[P, 7], columns PASS_FIELDS), ends (np.uint64[P]), touched (np.uint64[P, W]), truncates (TRUNC_DTYPE[K])
    and slots (np.uint64[n_slots, 2, 6]: rows and first per category)."""

    def __init__(self, info, passes, ends, touched, truncates, slots):
        self.info, self.passes, self.ends, self.touched, self.truncates, self.slots = info, passes, ends, touched, truncates, slots

    def touched_slots(self, p):
        """The slots pass p holds rows of (host arrays only)."""
        return [64 * w + b for w, word in enumerate(self.touched[p].tolist()) for b in range(64) if (word >> b) & 1]

    def truncated_tables(self, p):
        """[(table_id, schema_slot, event)] pass p truncates: the first entry per table_id, as truncate_schemas.entry(id).or_insert(schema)
        keeps it (clickhouse/core.rs:1148-1155). Host arrays only; entries beyond trunc_cap are not there to be looked at."""
        lo, n = int(self.passes[p][5]), int(self.passes[p][6])
        seen = {}
        for t, s, e in self.truncates[lo:lo + n].tolist():
            seen.setdefault(t, (t, s, e))
        return list(seen.values())


class DuckLakePlan:
    """What Batch.ducklake_plan returns: info (abi.DlPlanInfo) and, cut to what was written — or as the device addresses the caller
    gave —, ranges (abi.DlRange per group: what ducklake_fingerprints takes), batches (abi.DlBatch) and ops (abi.DlOp)."""

    def __init__(self, info, ranges, batches, ops):
        self.info, self.ranges, self.batches, self.ops = info, ranges, batches, ops

    def fingerprint_ranges(self):
        """[(first_event, end_event, seed)] for Batch.ducklake_fingerprints (host arrays only)."""
        return [(int(r.first_event), int(r.end_event), int(r.seed)) for r in self.ranges]


class SnowflakePlan:
    """What Batch.snowflake_plan returns: info (abi.SfPlanInfo) and, cut to what was written — or as the device addresses the caller
    gave —, segments (abi.SfSegment) and windows (abi.SfWindow, one per pass)."""

    def __init__(self, info, segments, windows):
        self.info, self.segments, self.windows = info, segments, windows


class ClickHousePlan:
    """What Batch.clickhouse_plan returns: info (abi.ChPlanInfo) and, cut to what was written — or as the device addresses the caller
    gave —, statements (abi.ChStatement) and windows (abi.ChWindow, one per pass)."""

    def __init__(self, info, statements, windows):
        self.info, self.statements, self.windows = info, statements, windows


class BigQueryPlan:
    """What Batch.bigquery_plan returns: info (abi.BqPlanInfo) and, cut to what was written — or as the device addresses the caller
    gave —, requests (abi.BqRequest) and windows (abi.BqWindow, one per pass; one on a table-copy batch)."""

    def __init__(self, info, requests, windows):
        self.info, self.requests, self.windows = info, requests, windows


class IcebergPlan:
    """What Batch.iceberg_plan returns: info (abi.IcePlanInfo) and, cut to what was written — or as the device addresses the caller
    gave —, writes (abi.IceWrite), slices (per write a list of abi.IceSlice, one per column of the changelog object) and windows
    (abi.IceWindow, one per pass; one on a table-copy batch)."""

    def __init__(self, info, writes, slices, windows):
        self.info, self.writes, self.slices, self.windows = info, writes, slices, windows


class Batch:
    """A decoded batch (etlg_batch). `host()` copies the arena into numpy arrays."""

    def __init__(self, dec, handle, rc, keep=None):
        self.dec, self.h, self.rc = dec, handle, rc
        self._keep = keep
        self.error = dec.last_error() if rc != abi.OK else None

    def view(self):
        v = abi.BatchView()
        self.dec.L.etlg_batch_view_get(self.h, C.byref(v))
        return v

    def sync(self):
        self.rc = self.dec.L.etlg_batch_sync(self.dec.h, self.h)
        self.error = self.dec.last_error() if self.rc != abi.OK else None
        return self.rc

    def header_to_device(self, dst_ptr):
        """Enqueue the 64-byte result header into device memory (multi-GPU all-gather input)."""
        return self.dec.L.etlg_batch_header_to_device(self.dec.h, self.h, C.c_void_p(dst_ptr))

    def host(self):
        v = self.view()
        if v.on_device:
            rc = self.dec.L.etlg_batch_download(self.dec.h, self.h)
            if rc != abi.OK:
                raise self.dec.last_error()
            v = self.view()
        return HostBatch.from_view(v)

    def columns(self, slot, kinds=("I",), on_device=False, parse_arrays=False, format_json=False):
        """Arrow-layout column buffers of the rows decoded against schema slot `slot`, built on the device
        (etlg_batch_columns). The batch must still be device-resident. parse_arrays: bool / int2 / int4 / int8 / oid array
        columns are parsed on the device into list columns (abi.AK_LIST); a malformed literal raises the reference's error.
        format_json: json / jsonb columns leave as LargeUtf8 of serde_json's `Value::to_string()` (abi.ROWS_FORMAT_JSON)."""
        rk = ((abi.ROWS_INSERT if "I" in kinds else 0) | (abi.ROWS_UPDATE if "U" in kinds else 0) | (abi.ROWS_PARSE_ARRAYS if parse_arrays else 0)
              | (abi.ROWS_FORMAT_JSON if format_json else 0))
        out = C.c_void_p()
        rc = self.dec.L.etlg_batch_columns(self.dec.h, self.h, slot, rk, abi.F_OUTPUT_ON_DEVICE if on_device else 0, C.byref(out))
        if rc != abi.OK or not out:
            raise self.dec.last_error()
        return Columns(self.dec, out)

    def iceberg(self, slot, parse_arrays=False, format_json=False, on_device=False):
        """The Iceberg sink's changelog rows of schema slot `slot` (etlg_batch_iceberg): Insert -> the row, Update -> the new row,
        Delete -> the full old row, as the column buffers of columns() followed by the two CDC columns cdc_operation and
        sequence_number. Returns a `Columns` whose `.changelog` (abi.ChangelogInfo) counts the events the sink refuses (partial
        updates, deletes without a full old row) and names the first of them: the caller raises the sink's error for it."""
        opts = (abi.ROWS_PARSE_ARRAYS if parse_arrays else 0) | (abi.ROWS_FORMAT_JSON if format_json else 0)
        out = C.c_void_p()
        rc = self.dec.L.etlg_batch_iceberg(self.dec.h, self.h, slot, opts, abi.F_OUTPUT_ON_DEVICE if on_device else 0, C.byref(out))
        if rc != abi.OK or not out:
            raise self.dec.last_error()
        cols = Columns(self.dec, out)
        cols.changelog = abi.ChangelogInfo()
        rc = self.dec.L.etlg_columns_changelog_get(out, C.byref(cols.changelog))
        assert rc == abi.OK, rc
        return cols

    def ducklake_copy(self, slot, on_device=False):
        """DuckLake's Arrow copy staging of schema slot `slot` of a table-copy batch (etlg_batch_ducklake_copy): every row, as the
        column buffers of the RecordBatch the sink appends — Int16 for int2, UInt64 for oid, Utf8 / Binary with int32 offsets. Returns a
        `Columns` whose `.ducklake` (abi.DuckLakeCopyInfo) says whether anything was built: status abi.DLC_NOT_ARROW (a uuid, json or
        array column: the sink takes its row path) and abi.DLC_OFFSETS_OVERFLOW (a column's bytes pass 2^31 - 1) name the column and
        come without rows. Raises EtlError (InvalidArgument) for a batch that is not a table copy."""
        out = C.c_void_p()
        rc = self.dec.L.etlg_batch_ducklake_copy(self.dec.h, self.h, slot, abi.F_OUTPUT_ON_DEVICE if on_device else 0, C.byref(out))
        if rc != abi.OK or not out:
            raise self.dec.last_error()
        cols = Columns(self.dec, out)
        cols.ducklake = abi.DuckLakeCopyInfo()
        rc = self.dec.L.etlg_columns_ducklake_get(out, C.byref(cols.ducklake))
        assert rc == abi.OK, rc
        return cols

    def finish_cells(self, what=abi.FINISH_ARRAYS | abi.FINISH_FLOATS):
        """Typed arrays / exact floats in the arena, on the device (etlg_batch_finish_cells). Returns abi.FinishStats."""
        st = abi.FinishStats()
        rc = self.dec.L.etlg_batch_finish_cells(self.dec.h, self.h, what, C.byref(st))
        if rc != abi.OK:
            raise self.dec.last_error()
        return st

    def size_hints(self, model):
        """Event::size_hint per event (np.uint64; bit 63 = abi.SIZE_HINT_INCOMPLETE), computed on the device
        (etlg_batch_size_hints). `model`: abi.SizeModel — the reference's size_of constants."""
        out = np.zeros(int(self.view().n_events), dtype=np.uint64)
        rc = self.dec.L.etlg_batch_size_hints(self.dec.h, self.h, C.byref(model), 0, out.ctypes.data)
        if rc != abi.OK:
            raise self.dec.last_error()
        return out

    def cuts(self, model, budget, carry_in=0, first=0, end=None, hints=None, cap=None, on_device=False):
        """Where the apply loop cuts events [first, end) into write_events batches, found on the device (etlg_batch_cuts): a cut behind
        the event at which carry_in + the hints since the last cut reach `budget`. `model`: abi.SizeModel, or None with `hints`, the
        address of a DEVICE array of n_events hints (size_hints' format) that replaces the library's own. `cap`: the cuts to write at most
        (default: as many as the range has events). on_device: False -> the cuts come back as np.uint64[min(n_cuts, cap)]; the address
        of a device array of `cap` u64 -> they are written there and the address is returned.
        Returns (cuts, abi.CutsInfo): n_cuts may exceed cap; stop_event < end names the first INCOMPLETE event."""
        end = int(self.view().n_events) if end is None else int(end)
        cap = max(0, end - int(first)) if cap is None else int(cap)
        info = abi.CutsInfo()
        out = None if on_device else np.zeros(cap, dtype=np.uint64)
        ptr = (int(on_device) if cap else None) if on_device else (out.ctypes.data if cap else None)
        rc = self.dec.L.etlg_batch_cuts(self.dec.h, self.h, C.byref(model) if model is not None else None, hints, int(first), end, int(budget), int(carry_in),
                                        abi.F_OUTPUT_ON_DEVICE if on_device else 0, ptr, cap, C.byref(info))
        if rc != abi.OK:
            raise self.dec.last_error()
        return (on_device if on_device else out[:min(cap, int(info.n_cuts))]), info

    def locate(self, cuts, row_event, n_rows, n_cuts=None, out=None):
        """Rows in front of every cut (etlg_cuts_locate): np.uint64[k] = the number of entries of `row_event` below cuts[k]. `row_event`:
        the address of the DEVICE row_event array (n_rows entries) of a hand-off object built from this batch. `cuts`: a host array, or the
        address of a device array of `n_cuts` entries. `out`: the address of a device array the counts go to instead (returned as is)."""
        if isinstance(cuts, (int, np.integer)):
            cptr, n, dev = int(cuts), int(n_cuts), 1
        else:
            cuts = np.ascontiguousarray(cuts, dtype=np.uint64)
            cptr, n, dev = (cuts.ctypes.data if len(cuts) else None), len(cuts), 0
        res = None if out else np.zeros(n, dtype=np.uint64)
        rc = self.dec.L.etlg_cuts_locate(self.dec.h, cptr, n, dev, row_event, int(n_rows), abi.F_OUTPUT_ON_DEVICE if out else 0,
                                         int(out) if out else (res.ctypes.data if n else None))
        if rc != abi.OK:
            raise self.dec.last_error()
        return out if out else res

    def outline(self, cuts=None, n_cuts=None, first=0, end=None, relations_inline=False, passes_cap=None, trunc_cap=None, on_device=False):
        """The pass plan of a sink's write_events loop over events [first, end), built on the device (etlg_batch_outline). `cuts`: the
        ends of the write_events ranges, a host array or the address of a device array of `n_cuts` entries (Batch.cuts leaves them so);
        None: one range. relations_inline: Iceberg's loop (abi.OL_RELATIONS_INLINE). on_device: False -> arrays; a dict of device
        addresses under "passes", "ends", "touched", "truncates", "slots" (absent: that part is skipped) -> written there, with
        passes_cap / trunc_cap saying what they hold. Host caps left None: one call counts, a second one fills arrays of exactly that size.
        Returns an Outline; with info.status == abi.OL_BAD_CUTS nothing but info.bad_cut is set."""
        v = self.view()
        end = int(v.n_events) if end is None else int(end)
        ns, W = int(v.n_slots), (int(v.n_slots) + 63) // 64
        if cuts is None:
            cptr, nc, cdev = None, 0, 0
        elif isinstance(cuts, (int, np.integer)):
            cptr, nc, cdev = int(cuts), int(n_cuts), 1
        else:
            cuts = np.ascontiguousarray(cuts, dtype=np.uint64)
            cptr, nc, cdev = (cuts.ctypes.data if len(cuts) else None), len(cuts), 0
        opts = abi.OL_RELATIONS_INLINE if relations_inline else 0

        def call(flags, pp, ep, tp, pcap, kp, kcap, sp):
            info = abi.OutlineInfo()
            rc = self.dec.L.etlg_batch_outline(self.dec.h, self.h, int(first), end, cptr, nc, cdev, opts, flags, pp, ep, tp, pcap, kp, kcap, sp, C.byref(info))
            if rc != abi.OK:
                raise self.dec.last_error()
            return info

        if on_device:
            g = lambda k: int(on_device[k]) if on_device.get(k) else None
            info = call(abi.F_OUTPUT_ON_DEVICE, g("passes"), g("ends"), g("touched"), int(passes_cap or 0), g("truncates"), int(trunc_cap or 0), g("slots"))
            return Outline(info, g("passes"), g("ends"), g("touched"), g("truncates"), g("slots"))
        if passes_cap is None or trunc_cap is None:
            info = call(0, None, None, None, 0, None, 0, None)
            if info.status != abi.OL_OK:
                return Outline(info, None, None, None, None, None)
            passes_cap = int(info.n_passes) if passes_cap is None else int(passes_cap)
            trunc_cap = int(info.n_trunc) if trunc_cap is None else int(trunc_cap)
        pc, kc = int(passes_cap), int(trunc_cap)
        passes, ends, touched = np.zeros((pc, 7), dtype=np.uint64), np.zeros(pc, dtype=np.uint64), np.zeros((pc, W), dtype=np.uint64)
        trunc, slots = np.zeros(kc, dtype=TRUNC_DTYPE), np.zeros((ns, 2, 6), dtype=np.uint64)
        info = call(0, passes.ctypes.data if pc else None, ends.ctypes.data if pc else None, touched.ctypes.data if pc and W else None, pc,
                    trunc.ctypes.data if kc else None, kc, slots.ctypes.data if ns else None)
        if info.status != abi.OL_OK:
            return Outline(info, None, None, None, None, None)
        P, K = min(pc, int(info.n_passes)), min(kc, int(info.n_trunc))
        return Outline(info, passes[:P], ends[:P], touched[:P], trunc[:K], slots)

    def payload(self, buf, offs, cuts=None, bounds=(), on_device=False, nbytes=None, nframes=None, n_cuts=None, sums=True):
        """Source payload accounting of the batch, on the device (etlg_batch_payload). `buf`, `offs`: the input the batch was decoded
        from — numpy arrays, or device addresses with `nbytes` / `nframes`; for a table-copy batch the rows and row_offsets. `cuts`: the
        ends of the write_events ranges, a host array or the address of a device array of `n_cuts` entries (Batch.cuts leaves them so);
        None: one range. `bounds`: ascending histogram bounds (<= 64). on_device: False -> ev_bytes (np.uint32[n_events]) and sums
        (np.uint64[n_ranges, 2, 4]: bytes and rows per abi.PK_*) come back as arrays; a pair (ev_bytes address or None, sums address or
        None) of device arrays -> they are written there. sums=False: no range sums.
        Returns a Payload: info (abi.PayloadInfo), hist (np.uint64[4, len(bounds) + 1]), ev_bytes, sums."""
        in_dev = isinstance(buf, (int, np.integer))
        if in_dev:
            bptr, blen, optr, nf = int(buf), int(nbytes), int(offs), int(nframes)
        else:
            buf = np.ascontiguousarray(buf, dtype=np.uint8)
            offs = None if offs is None else np.ascontiguousarray(offs, dtype=np.uint32)
            bptr, blen, optr = (buf.ctypes.data if len(buf) else None), len(buf), _ptr(offs)
            nf = (len(offs) - 1 if offs is not None else 0) if nframes is None else int(nframes)
        if cuts is None:
            cptr, nc, cdev = None, 0, 0
        elif isinstance(cuts, (int, np.integer)):
            cptr, nc, cdev = int(cuts), int(n_cuts), 1
        else:
            cuts = np.ascontiguousarray(cuts, dtype=np.uint64)
            cptr, nc, cdev = (cuts.ctypes.data if len(cuts) else None), len(cuts), 0
        bnd = np.ascontiguousarray(bounds, dtype=np.uint64)
        hist = np.zeros((4, len(bnd) + 1), dtype=np.uint64)
        ne = int(self.view().n_events)
        flags = (abi.F_INPUT_ON_DEVICE if in_dev else 0) | (abi.F_OUTPUT_ON_DEVICE if on_device else 0)
        if on_device:
            ev, sm = on_device
            eptr, sptr = (int(ev) if ev else None), (int(sm) if sm else None)
        else:
            ev, sm = np.zeros(ne, dtype=np.uint32), (np.zeros((nc + 1, 2, 4), dtype=np.uint64) if sums else None)
            eptr, sptr = (ev.ctypes.data if ne else None), _ptr(sm)
        info = abi.PayloadInfo()
        rc = self.dec.L.etlg_batch_payload(self.dec.h, self.h, bptr, blen, optr, nf, cptr, nc, cdev, (bnd.ctypes.data if len(bnd) else None), len(bnd), flags,
                                           eptr, sptr, hist.ctypes.data, C.byref(info))
        if rc != abi.OK:
            raise self.dec.last_error()
        return Payload(info, hist, ev, sm)

    def rowbinary(self, slot, nullable_flags, engine=abi.CH_MERGE_TREE, on_device=False):
        """ClickHouse RowBinary rows of schema slot `slot`, encoded on the device (etlg_batch_rowbinary). Raises EtlError for
        the reference's ConversionErrors; `RowBinary.status == abi.RB_NEEDS_HOST` when a cell has no device encoding."""
        nf = np.ascontiguousarray(nullable_flags, dtype=np.uint8)
        out = C.c_void_p()
        rc = self.dec.L.etlg_batch_rowbinary(self.dec.h, self.h, slot, nf.ctypes.data, len(nf), engine,
                                             abi.F_OUTPUT_ON_DEVICE if on_device else 0, C.byref(out))
        if rc != abi.OK or not out:
            raise self.dec.last_error()
        return RowBinary(self.dec, out)

    def protobuf(self, slot, on_device=False):
        """BigQuery protobuf rows (one per Insert event) of schema slot `slot`, encoded on the device (etlg_batch_protobuf)."""
        out = C.c_void_p()
        rc = self.dec.L.etlg_batch_protobuf(self.dec.h, self.h, slot, abi.F_OUTPUT_ON_DEVICE if on_device else 0, C.byref(out))
        if rc != abi.OK or not out:
            raise self.dec.last_error()
        return RowBinary(self.dec, out)

    def ndjson(self, slot, names, on_device=False):
        """Snowflake NDJSON lines (one per row, each ending in '\\n') of schema slot `slot`, encoded on the device (etlg_batch_ndjson).
        `names`: the slot's replicated column names (str or bytes) in slot order. Raises EtlError for the sink's encoding errors and
        ETLG_E_JSON; `RowBinary.status == abi.RB_NEEDS_HOST` when a cell has no device encoding."""
        raw = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
        blob = b"".join(n + b"\0" for n in raw)
        out = C.c_void_p()
        rc = self.dec.L.etlg_batch_ndjson(self.dec.h, self.h, slot, blob, len(raw), abi.F_OUTPUT_ON_DEVICE if on_device else 0, C.byref(out))
        if rc != abi.OK or not out:
            raise self.dec.last_error()
        return RowBinary(self.dec, out)

    def duckdb(self, slot, names, what=abi.DL_TUPLES, on_device=False):
        """DuckLake SQL literals of schema slot `slot`, encoded on the device (etlg_batch_duckdb): `what=abi.DL_TUPLES` one
        "(lit, lit, ...)" per row the sink upserts, `abi.DL_PREDICATES` one `"col" = lit AND ...` per row image it deletes / matches
        by, `abi.DL_UPDATES` two records per partial Update — its SET clause `"col" = lit, ...`, then its predicate — with
        `RowBinary.col_ends()` cutting every record into its columns' pieces; no separator between records. `names` as for ndjson().
        Raises EtlError for ETLG_E_JSON and bad arguments; `RowBinary.status == abi.RB_NEEDS_HOST` when a cell has no device encoding."""
        raw = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
        blob = b"".join(n + b"\0" for n in raw)
        out = C.c_void_p()
        rc = self.dec.L.etlg_batch_duckdb(self.dec.h, self.h, slot, what, blob, len(raw), abi.F_OUTPUT_ON_DEVICE if on_device else 0, C.byref(out))
        if rc != abi.OK or not out:
            raise self.dec.last_error()
        r = RowBinary(self.dec, out)
        r.n_cols = len(raw)
        return r

    def ducklake_fingerprints(self, slot, names, ranges, tuples, predicates, updates=None):
        """DuckLake batch identities of schema slot `slot`, hashed on the device (etlg_ducklake_fingerprints): for every
        (first_event, end_event, seed) of `ranges` — ascending, disjoint — the FNV-1a-64 state after `seed` has absorbed the byte stream
        of the slot's Insert / Update / Delete events in [first_event, end_event). `tuples` / `predicates` / `updates` (or None): the
        device-resident results of duckdb(slot, names, what=abi.DL_TUPLES / DL_PREDICATES / DL_UPDATES, on_device=True) on this batch.
        Returns (np.uint64[len(ranges)], abi.DlFpInfo); with info.status == abi.RB_NEEDS_HOST the array holds nothing."""
        raw = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
        blob = b"".join(n + b"\0" for n in raw)
        rs = (abi.DlRange * max(1, len(ranges)))()
        for i, (first, end, seed) in enumerate(ranges):
            rs[i].first_event, rs[i].end_event, rs[i].seed = int(first), int(end), int(seed)
        out = np.zeros(len(ranges), dtype=np.uint64)
        info = abi.DlFpInfo()
        rc = self.dec.L.etlg_ducklake_fingerprints(self.dec.h, self.h, slot, tuples.h, predicates.h, updates.h if updates is not None else None, blob, len(raw),
                                                   C.addressof(rs), len(ranges), out.ctypes.data, C.byref(info))
        if rc != abi.OK:
            raise self.dec.last_error()
        return out, info

    def ducklake_plan(self, slot, passes, n_passes=None, watermark=None, seed=0, tuples=None, predicates=None, updates=None,
                      batches_cap=None, ops_cap=None, on_device=False):
        """The DuckLake sink's atomic batches of schema slot `slot`, cut on the device (etlg_ducklake_plan). `passes`: what
        Batch.outline gave — np.uint64[P, 7], or the address of a device array of `n_passes` etlg_outline_pass; only first_event and
        data_end are read. watermark: None or (commit_lsn, tx_ordinal), the sequence key already applied. seed: the table's hasher state,
        copied into every range. tuples / predicates / updates: the device-resident duckdb() results of this batch and slot, or None.
        on_device: False -> arrays; a dict of device addresses under "ranges", "batches", "ops" (absent: that part is skipped) ->
        written there, with batches_cap / ops_cap saying what they hold. Host caps left None: one call counts, a second one fills arrays
        of exactly that size. Returns a DuckLakePlan; with info.status != abi.DLP_OK nothing but info is set."""
        if isinstance(passes, (int, np.integer)):
            pptr, npass, pdev = int(passes), int(n_passes), 1
        else:
            passes = np.ascontiguousarray(passes, dtype=np.uint64).reshape(-1, 7)
            pptr, npass, pdev = (passes.ctypes.data if len(passes) else None), len(passes), 0
        has_wm, wl, wo = (0, 0, 0) if watermark is None else (1, int(watermark[0]), int(watermark[1]))
        h = lambda r: r.h if r is not None else None

        def call(flags, rp, bp, bcap, op, ocap):
            info = abi.DlPlanInfo()
            rc = self.dec.L.etlg_ducklake_plan(self.dec.h, self.h, slot, pptr, npass, pdev, has_wm, wl, wo, int(seed), h(tuples), h(predicates), h(updates),
                                               flags, rp, bp, bcap, op, ocap, C.byref(info))
            if rc != abi.OK:
                raise self.dec.last_error()
            return info

        if on_device:
            g = lambda k: int(on_device[k]) if on_device.get(k) else None
            info = call(abi.F_OUTPUT_ON_DEVICE, g("ranges"), g("batches"), int(batches_cap or 0), g("ops"), int(ops_cap or 0))
            return DuckLakePlan(info, g("ranges"), g("batches"), g("ops"))
        if batches_cap is None or ops_cap is None:
            info = call(0, None, None, 0, None, 0)
            if info.status != abi.DLP_OK:
                return DuckLakePlan(info, None, None, None)
            batches_cap = int(info.n_batches) if batches_cap is None else int(batches_cap)
            ops_cap = int(info.n_ops) if ops_cap is None else int(ops_cap)
        bc, oc = int(batches_cap), int(ops_cap)
        ranges, batches, ops = (abi.DlRange * max(1, bc))(), (abi.DlBatch * max(1, bc))(), (abi.DlOp * max(1, oc))()
        info = call(0, C.addressof(ranges) if bc else None, C.addressof(batches) if bc else None, bc, C.addressof(ops) if oc else None, oc)
        if info.status != abi.DLP_OK:
            return DuckLakePlan(info, None, None, None)
        B, K = min(bc, int(info.n_batches)), min(oc, int(info.n_ops))
        return DuckLakePlan(info, [ranges[i] for i in range(B)], [batches[i] for i in range(B)], [ops[i] for i in range(K)])

    def snowflake_plan(self, slot, passes, ndjson, n_passes=None, committed=None, flush_bytes=abi.SF_MAX_UNFLUSHED_BYTES,
                       max_row_bytes=abi.SF_MAX_ROW_BYTES, segs_cap=None, on_device=False):
        """The Snowflake sink's row batches of schema slot `slot`, planned on the device (etlg_snowflake_plan): which rows of `ndjson`
        — the device-resident ndjson() result of this batch and slot — each window's RowBatchBuilder takes, and where push_row flushes.
        `passes`: what Batch.outline gave — np.uint64[P, 7], or the address of a device array of `n_passes` etlg_outline_pass; only
        first_event and data_end are read; None on a table-copy batch: one window over all rows. committed: None or (commit_lsn,
        tx_ordinal), the channel's committed offset. on_device: False -> arrays; a dict of device addresses under "segments", "windows"
        (absent: that part is skipped) -> written there, with segs_cap saying what "segments" holds. segs_cap left None on the host: one
        call counts, a second one fills an array of exactly that size. Returns a SnowflakePlan; with info.status != abi.SFP_OK nothing
        but info is set."""
        if passes is None:
            pptr, npass, pdev = None, 0, 0
        elif isinstance(passes, (int, np.integer)):
            pptr, npass, pdev = int(passes), int(n_passes), 1
        else:
            passes = np.ascontiguousarray(passes, dtype=np.uint64).reshape(-1, 7)
            pptr, npass, pdev = (passes.ctypes.data if len(passes) else None), len(passes), 0
        has_c, cl, co = (0, 0, 0) if committed is None else (1, int(committed[0]), int(committed[1]))
        nwin = npass if passes is not None else 1

        def call(flags, sp, scap, wp):
            info = abi.SfPlanInfo()
            rc = self.dec.L.etlg_snowflake_plan(self.dec.h, self.h, slot, pptr, npass, pdev, has_c, cl, co, ndjson.h if ndjson is not None else None,
                                                int(flush_bytes), int(max_row_bytes), flags, sp, scap, wp, C.byref(info))
            if rc != abi.OK:
                raise self.dec.last_error()
            return info

        if on_device:
            g = lambda k: int(on_device[k]) if on_device.get(k) else None
            info = call(abi.F_OUTPUT_ON_DEVICE, g("segments"), int(segs_cap or 0), g("windows"))
            return SnowflakePlan(info, g("segments"), g("windows"))
        if segs_cap is None:
            info = call(0, None, 0, None)
            if info.status != abi.SFP_OK:
                return SnowflakePlan(info, None, None)
            segs_cap = int(info.n_segs)
        sc = int(segs_cap)
        segs, wins = (abi.SfSegment * max(1, sc))(), (abi.SfWindow * max(1, nwin))()
        info = call(0, C.addressof(segs) if sc else None, sc, C.addressof(wins) if nwin else None)
        if info.status != abi.SFP_OK:
            return SnowflakePlan(info, None, None)
        return SnowflakePlan(info, [segs[i] for i in range(min(sc, int(info.n_segs)))], [wins[i] for i in range(nwin)])

    def clickhouse_plan(self, slot, passes, rowbinary, n_passes=None, max_bytes_per_insert=abi.CH_MAX_BYTES_PER_INSERT, stmts_cap=None, on_device=False):
        """The ClickHouse sink's INSERT statements of schema slot `slot`, cut on the device (etlg_clickhouse_plan): which rows of
        `rowbinary` — the device-resident rowbinary() result of this batch and slot, whose engine decides the refusals — each statement
        of insert_rows takes, per window. `passes`: what Batch.outline gave — np.uint64[P, 7], or the address of a device array of
        `n_passes` etlg_outline_pass; only first_event and data_end are read; None on a table-copy batch: one window over all rows.
        on_device: False -> arrays; a dict of device addresses under "statements", "windows" (absent: that part is skipped) -> written
        there, with stmts_cap saying what "statements" holds. stmts_cap left None on the host: one call counts, a second one fills an
        array of exactly that size. Returns a ClickHousePlan; with info.status != abi.CHP_OK nothing but info is set."""
        if passes is None:
            pptr, npass, pdev = None, 0, 0
        elif isinstance(passes, (int, np.integer)):
            pptr, npass, pdev = int(passes), int(n_passes), 1
        else:
            passes = np.ascontiguousarray(passes, dtype=np.uint64).reshape(-1, 7)
            pptr, npass, pdev = (passes.ctypes.data if len(passes) else None), len(passes), 0
        nwin = npass if passes is not None else 1

        def call(flags, sp, scap, wp):
            info = abi.ChPlanInfo()
            rc = self.dec.L.etlg_clickhouse_plan(self.dec.h, self.h, slot, pptr, npass, pdev, rowbinary.h if rowbinary is not None else None,
                                                 int(max_bytes_per_insert), flags, sp, scap, wp, C.byref(info))
            if rc != abi.OK:
                raise self.dec.last_error()
            return info

        if on_device:
            g = lambda k: int(on_device[k]) if on_device.get(k) else None
            info = call(abi.F_OUTPUT_ON_DEVICE, g("statements"), int(stmts_cap or 0), g("windows"))
            return ClickHousePlan(info, g("statements"), g("windows"))
        if stmts_cap is None:
            info = call(0, None, 0, None)
            if info.status != abi.CHP_OK:
                return ClickHousePlan(info, None, None)
            stmts_cap = int(info.n_stmts)
        sc = int(stmts_cap)
        stmts, wins = (abi.ChStatement * max(1, sc))(), (abi.ChWindow * max(1, nwin))()
        info = call(0, C.addressof(stmts) if sc else None, sc, C.addressof(wins) if nwin else None)
        if info.status != abi.CHP_OK:
            return ClickHousePlan(info, None, None)
        return ClickHousePlan(info, [stmts[i] for i in range(min(sc, int(info.n_stmts)))], [wins[i] for i in range(nwin)])

    def bigquery_plan(self, slot, passes, protobuf, n_passes=None, max_batch_bytes=0, reqs_cap=None, on_device=False):
        """The BigQuery sink's append requests of schema slot `slot`, planned on the device (etlg_bigquery_plan): which rows of
        `protobuf` — the device-resident protobuf() result of this batch and slot — each create_append_request takes, one per window
        with a member. `passes`: what Batch.outline gave — np.uint64[P, 7], or the address of a device array of `n_passes`
        etlg_outline_pass; only first_event and data_end are read; None on a table-copy batch, whose rows split_table_rows cuts by
        `max_batch_bytes` (the client crate's MAX_BATCH_SIZE_BYTES; required there, ignored elsewhere).
        on_device: False -> arrays; a dict of device addresses under "requests", "windows" (absent: that part is skipped) -> written
        there, with reqs_cap saying what "requests" holds. reqs_cap left None on the host: one call counts, a second one fills an
        array of exactly that size. Returns a BigQueryPlan; with info.status != abi.BQP_OK nothing but info is set."""
        if passes is None:
            pptr, npass, pdev = None, 0, 0
        elif isinstance(passes, (int, np.integer)):
            pptr, npass, pdev = int(passes), int(n_passes), 1
        else:
            passes = np.ascontiguousarray(passes, dtype=np.uint64).reshape(-1, 7)
            pptr, npass, pdev = (passes.ctypes.data if len(passes) else None), len(passes), 0
        nwin = npass if passes is not None else 1

        def call(flags, rp, rcap, wp):
            info = abi.BqPlanInfo()
            rc = self.dec.L.etlg_bigquery_plan(self.dec.h, self.h, slot, pptr, npass, pdev, protobuf.h if protobuf is not None else None,
                                               int(max_batch_bytes), flags, rp, rcap, wp, C.byref(info))
            if rc != abi.OK:
                raise self.dec.last_error()
            return info

        if on_device:
            g = lambda k: int(on_device[k]) if on_device.get(k) else None
            info = call(abi.F_OUTPUT_ON_DEVICE, g("requests"), int(reqs_cap or 0), g("windows"))
            return BigQueryPlan(info, g("requests"), g("windows"))
        if reqs_cap is None:
            info = call(0, None, 0, None)
            if info.status != abi.BQP_OK:
                return BigQueryPlan(info, None, None)
            reqs_cap = int(info.n_reqs)
        rc_ = int(reqs_cap)
        reqs, wins = (abi.BqRequest * max(1, rc_))(), (abi.BqWindow * max(1, nwin))()
        info = call(0, C.addressof(reqs) if rc_ else None, rc_, C.addressof(wins) if nwin else None)
        if info.status != abi.BQP_OK:
            return BigQueryPlan(info, None, None)
        return BigQueryPlan(info, [reqs[i] for i in range(min(rc_, int(info.n_reqs)))], [wins[i] for i in range(nwin)])

    def iceberg_plan(self, slot, passes, changelog, n_passes=None, writes_cap=None, on_device=False):
        """The Iceberg sink's writes of schema slot `slot`, planned on the device (etlg_iceberg_plan): which rows of `changelog` — the
        device-resident iceberg() result of this batch and slot — each insert_rows takes, one per window with a member, and per
        write and column of the object the Arrow slice over those rows (null, deferred and child null counts, value and child
        ranges). `passes`: what Batch.outline gave WITH abi.OL_RELATIONS_INLINE — np.uint64[P, 7], or the address of a device array
        of `n_passes` etlg_outline_pass; only first_event and data_end are read; None on a table-copy batch.
        on_device: False -> arrays; a dict of device addresses under "writes", "slices", "windows" (absent: that part is skipped)
        -> written there, with writes_cap saying what "writes" holds ("slices": writes_cap * n_cols entries). writes_cap left None
        on the host: one call counts, a second one fills arrays of exactly that size. Returns an IcebergPlan — slices[k][c] is
        the slice of write k and column c —; with info.status != abi.ICP_OK nothing but info is set."""
        if passes is None:
            pptr, npass, pdev = None, 0, 0
        elif isinstance(passes, (int, np.integer)):
            pptr, npass, pdev = int(passes), int(n_passes), 1
        else:
            passes = np.ascontiguousarray(passes, dtype=np.uint64).reshape(-1, 7)
            pptr, npass, pdev = (passes.ctypes.data if len(passes) else None), len(passes), 0
        nwin = npass if passes is not None else 1
        ncols = int(changelog.view.n_cols) if changelog is not None else 0

        def call(flags, wp, wcap, sp, np_):
            info = abi.IcePlanInfo()
            rc = self.dec.L.etlg_iceberg_plan(self.dec.h, self.h, slot, pptr, npass, pdev, changelog.h if changelog is not None else None,
                                              flags, wp, wcap, sp, np_, C.byref(info))
            if rc != abi.OK:
                raise self.dec.last_error()
            return info

        if on_device:
            g = lambda k: int(on_device[k]) if on_device.get(k) else None
            info = call(abi.F_OUTPUT_ON_DEVICE, g("writes"), int(writes_cap or 0), g("slices"), g("windows"))
            return IcebergPlan(info, g("writes"), g("slices"), g("windows"))
        if writes_cap is None:
            info = call(0, None, 0, None, None)
            if info.status != abi.ICP_OK:
                return IcebergPlan(info, None, None, None)
            writes_cap = int(info.n_writes)
        wc = int(writes_cap)
        writes, slices, wins = (abi.IceWrite * max(1, wc))(), (abi.IceSlice * max(1, wc * ncols))(), (abi.IceWindow * max(1, nwin))()
        info = call(0, C.addressof(writes) if wc else None, wc, C.addressof(slices) if wc else None, C.addressof(wins) if nwin else None)
        if info.status != abi.ICP_OK:
            return IcebergPlan(info, None, None, None)
        nw = min(wc, int(info.n_writes))
        return IcebergPlan(info, [writes[i] for i in range(nw)], [[slices[k * ncols + c] for c in range(ncols)] for k in range(nw)], [wins[i] for i in range(nwin)])

    def close(self):
        if self.h:
            self.dec.L.etlg_batch_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Columns:
    """etlg_columns: `view` = etlg_columns_view; `host_arrays()` wraps host-resident buffers as numpy arrays."""

    def __init__(self, dec, handle):
        self.dec, self.h = dec, handle
        self.changelog = None   # abi.ChangelogInfo of a Batch.iceberg() result
        self.ducklake = None    # abi.DuckLakeCopyInfo of a Batch.ducklake_copy() result
        self.view = abi.ColumnsView()
        dec.L.etlg_columns_view_get(handle, C.byref(self.view))

    @property
    def n_rows(self):
        return int(self.view.n_rows)

    def column(self, i):
        return self.view.cols[i]

    def _np(self, ptr, nbytes, dtype):
        if not nbytes:
            return np.zeros(0, dtype=dtype)
        assert not self.view.on_device, "device-resident buffers: read them through abi.device_tensor"
        return np.frombuffer((C.c_uint8 * nbytes).from_address(ptr), dtype=dtype)

    def host_arrays(self, i):
        """(validity bits u8[], deferred bits u8[], values u8[], offsets i64[] | None) of column i (views into the block); the offsets
        of an abi.AK_UTF8 / AK_BINARY column are i32[]."""
        k, n = self.view.cols[i], self.n_rows
        if k.arrow_kind == abi.AK_NONE:
            return None
        bm = (n + 63) // 64 * 8
        o32 = k.arrow_kind in (abi.AK_UTF8, abi.AK_BINARY)
        offs = self._np(k.offsets, (n + 1) * (4 if o32 else 8), np.int32 if o32 else np.int64) if k.offsets else None
        return self._np(k.validity, bm, np.uint8), self._np(k.deferred, bm, np.uint8), self._np(k.values, int(k.values_bytes), np.uint8), offs

    def child_validity(self, i):
        k = self.view.cols[i]
        return self._np(k.child_validity, (int(k.child_count) + 63) // 64 * 8, np.uint8)

    def child_offsets(self, i):
        k = self.view.cols[i]
        return self._np(k.child_offsets, (int(k.child_count) + 1) * 8, np.int64) if k.child_offsets else None

    def row_event(self):
        return self._np(self.view.row_event, self.n_rows * 8, np.uint64)

    def close(self):
        if self.h:
            self.dec.L.etlg_columns_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RowBinary:
    """etlg_rowbinary: `view` = etlg_rowbinary_view; the accessors below wrap host-resident buffers."""

    def __init__(self, dec, handle):
        self.dec, self.h = dec, handle
        self.n_cols = None      # the slot's width, of a Batch.duckdb() result (col_ends)
        self.view = abi.RowBinaryView()
        dec.L.etlg_rowbinary_view_get(handle, C.byref(self.view))

    status = property(lambda self: int(self.view.status))
    n_rows = property(lambda self: int(self.view.n_rows))

    def _np(self, ptr, nbytes, dtype):
        if not nbytes or not ptr:
            return np.zeros(0, dtype=dtype)
        assert not self.view.on_device
        return np.frombuffer((C.c_uint8 * nbytes).from_address(ptr), dtype=dtype)

    def bytes(self):
        return self._np(self.view.bytes, int(self.view.n_bytes), np.uint8)

    def row_offsets(self):
        return self._np(self.view.row_offsets, (self.n_rows + 1) * 8, np.int64)

    def row_event(self):
        return self._np(self.view.row_event, self.n_rows * 8, np.uint64)

    def col_ends_ptr(self):
        """Address of the n_rows * n_cols u32 array of a Batch.duckdb(what=abi.DL_UPDATES) result (etlg_rowbinary_col_ends_get), on
        the host or the device like the view's arrays. Raises EtlError (InvalidArgument) for any other object."""
        p = C.c_void_p()
        if self.dec.L.etlg_rowbinary_col_ends_get(self.h, C.byref(p)) != abi.OK:
            raise EtlError(abi.InvalidArgument, abi.InvalidArgument, "etlg_rowbinary_col_ends_get: not an ETLG_DL_UPDATES result", None, -1)
        return p.value or 0

    def col_ends(self):
        """[n_rows, n_cols] u32: bytes of record r written once column c is done (host-resident results)."""
        return self._np(self.col_ends_ptr(), self.n_rows * self.n_cols * 4, np.uint32).reshape(self.n_rows, self.n_cols)

    def close(self):
        if self.h:
            self.dec.L.etlg_rowbinary_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Decoder:
    def __init__(self, device=0, stream=None):
        self.L = native.lib()
        h = C.c_void_p()
        rc = self.L.etlg_ctx_create(device, C.byref(h))
        if rc != abi.OK:
            why = (self.L.etlg_create_error() or b"").decode()
            raise RuntimeError(f"etlg_ctx_create failed ({abi.KIND_NAMES.get(rc, rc)}: {why}): an MI355X (gfx950) device is required")
        self.h = h
        if stream is not None:
            self.set_stream(stream)

    def close(self):
        if getattr(self, "h", None):
            self.L.etlg_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- control plane (same calls the oracle wrapper exposes)
    def set_stream(self, cuda_stream_ptr):
        return self.L.etlg_ctx_set_stream(self.h, C.c_void_p(cuda_stream_ptr))

    def set_worker(self, worker=abi.WORKER_APPLY, table_id=0, bootstrap_lsn=0):
        return self.L.etlg_ctx_set_worker(self.h, worker, table_id, bootstrap_lsn)

    def debug_overlapped(self):
        """ASYNC batches enqueued beside their predecessor on the second decode stream (debugging aid, not in etlg.h)."""
        self.L.etlg_ctx_debug_overlapped.restype = C.c_ulonglong
        self.L.etlg_ctx_debug_overlapped.argtypes = [C.c_void_p]
        return int(self.L.etlg_ctx_debug_overlapped(self.h))

    def debug_ctl_ahead(self):
        """Batches whose control pre-pass ran ahead of their decode (ASYNC without NO_CONTROL on a stream with Relation / DDL frames)."""
        self.L.etlg_ctx_debug_ctl_ahead.restype = C.c_ulonglong
        self.L.etlg_ctx_debug_ctl_ahead.argtypes = [C.c_void_p]
        return int(self.L.etlg_ctx_debug_ctl_ahead(self.h))

    def fence(self):
        """The context's stream waits (device side) for every ASYNC batch enqueued so far — decode kernels on the library's two
        decode streams and header copies (etlg_ctx_fence); call before enqueuing a consumer of their arenas / headers on it."""
        return self.L.etlg_ctx_fence(self.h)

    def reset_stream_state(self):
        return self.L.etlg_ctx_reset_stream_state(self.h)

    def schema_put(self, table_id, snapshot_lsn, cols, schema="public", name="t"):
        arr = abi.make_cols(cols)
        return self.L.etlg_schema_put(self.h, table_id, snapshot_lsn, schema.encode(), name.encode(), len(cols), arr)

    def table_state(self, table_id, kind, lsn=0):
        return self.L.etlg_table_state(self.h, table_id, kind, lsn)

    def table_ready(self, table_id, snapshot_lsn, repl_mask, ident_mask):
        r = np.asarray(repl_mask, dtype=np.uint8)
        i = np.asarray(ident_mask, dtype=np.uint8)
        return self.L.etlg_table_ready(self.h, table_id, snapshot_lsn, _ptr(r), _ptr(i), len(r))

    def table_forget(self, table_id):
        """SharedTableCache::remove_table (table_cache.rs:131-145)."""
        return self.L.etlg_table_forget(self.h, table_id)

    def cache_state(self, table_id):
        """SharedTableCache::get (table_cache.rs:99-102): None, or (kind 1 WaitingForRelation | 2 Ready, snapshot id, schema slot)."""
        k, sn, sl = C.c_int32(), C.c_uint64(), C.c_int32()
        if not self.L.etlg_table_cache_get(self.h, table_id, C.byref(k), C.byref(sn), C.byref(sl)):
            return None
        return k.value, sn.value, sl.value

    def last_error(self):
        e = self.L.etlg_last_error(self.h).contents
        return EtlError(e.kind, e.code, (e.description or b"").decode(), (e.detail or b"").decode() or None, e.frame_index)

    # ---- decode
    def decode(self, buf, offsets=None, flags=0):
        """Host buffers: buf = bytes / np.uint8, offsets = optional u32 sidecar."""
        a = np.frombuffer(buf, dtype=np.uint8) if not isinstance(buf, np.ndarray) else np.ascontiguousarray(buf)
        off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint32)
        nfr = 0 if off is None else len(off) - 1
        out = C.c_void_p()
        rc = self.L.etlg_decode(self.h, _ptr(a), a.size, _ptr(off), nfr, flags & ~abi.F_INPUT_ON_DEVICE, C.byref(out))
        if not out:
            raise self.last_error()
        return Batch(self, out, rc, keep=(a, off))

    def host_alloc(self, nbytes):
        """Pinned host memory (etlg_host_alloc) as a writable np.uint8 array; free it with host_free(array)."""
        p = C.c_void_p()
        if self.L.etlg_host_alloc(self.h, nbytes, C.byref(p)) != abi.OK:
            raise self.last_error()
        a = np.frombuffer((C.c_uint8 * nbytes).from_address(p.value), dtype=np.uint8)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[a.ctypes.data] = p.value
        return a

    def host_free(self, a):
        self.L.etlg_host_free(C.c_void_p(self._pinned.pop(a.ctypes.data)))

    def decode_host_ptr(self, buf_ptr, nbytes, offs_ptr, nframes, flags):
        """Host buffers by address (pinned staging buffers of a batcher): with abi.F_ASYNC | abi.F_OUTPUT_ON_DEVICE the upload
        travels on the library's copy stream beside the previous batch's decode; the buffers stay untouched until the batch is synced."""
        out = C.c_void_p()
        rc = self.L.etlg_decode(self.h, C.c_void_p(buf_ptr), nbytes, C.c_void_p(offs_ptr), nframes, flags & ~abi.F_INPUT_ON_DEVICE, C.byref(out))
        if not out:
            raise self.last_error()
        return Batch(self, out, rc)

    def debug_staged(self):
        self.L.etlg_ctx_debug_staged.restype = C.c_ulonglong
        self.L.etlg_ctx_debug_staged.argtypes = [C.c_void_p]
        return int(self.L.etlg_ctx_debug_staged(self.h))

    def decode_device(self, buf_ptr, nbytes, offs_ptr, nframes, flags=abi.F_OUTPUT_ON_DEVICE):
        """Device-resident input (raw device pointers, e.g. torch tensor .data_ptr())."""
        out = C.c_void_p()
        rc = self.L.etlg_decode(self.h, C.c_void_p(buf_ptr), nbytes, C.c_void_p(offs_ptr), nframes,
                                flags | abi.F_INPUT_ON_DEVICE, C.byref(out))
        if not out:
            raise self.last_error()
        return Batch(self, out, rc)

    def copy_decode(self, slot, buf, row_offsets, flags=0):
        """Table-copy rows (COPY text format) from host buffers against schema slot `slot`
        (the value table_ready returned)."""
        a = np.frombuffer(buf, dtype=np.uint8) if not isinstance(buf, np.ndarray) else np.ascontiguousarray(buf)
        off = np.ascontiguousarray(row_offsets, dtype=np.uint32)
        out = C.c_void_p()
        rc = self.L.etlg_copy_decode(self.h, slot, _ptr(a), a.size, _ptr(off), len(off) - 1, flags & ~abi.F_INPUT_ON_DEVICE, C.byref(out))
        if not out:
            raise self.last_error()
        return Batch(self, out, rc, keep=(a, off))

    def copy_decode_device(self, slot, buf_ptr, nbytes, offs_ptr, nrows, flags=abi.F_OUTPUT_ON_DEVICE):
        out = C.c_void_p()
        rc = self.L.etlg_copy_decode(self.h, slot, C.c_void_p(buf_ptr), nbytes, C.c_void_p(offs_ptr), nrows,
                                     flags | abi.F_INPUT_ON_DEVICE, C.byref(out))
        if not out:
            raise self.last_error()
        return Batch(self, out, rc)

    # ---- measurement
    def profile(self, enable=True):
        """HIP-event timing of every kernel launch (etlg_ctx_profile). enable=2: additionally keep ASYNC batches on ONE decode stream,
        so that the durations are those of a kernel running alone (with two streams consecutive kernels overlap)."""
        return self.L.etlg_ctx_profile(self.h, 2 if enable == 2 else 1 if enable else 0)

    def profile_read(self):
        arr = (abi.KernelStat * 24)()
        n = C.c_uint32()
        self.L.etlg_ctx_profile_read(self.h, arr, 24, C.byref(n))
        return {arr[i].name.decode(): (arr[i].launches, arr[i].total_ms) for i in range(n.value)}

    def debug_paths(self):
        """Batches finished per kernel path (debugging aid, not in etlg.h): 'fused' / 'cells' / 'plan' = produced by that
        single-pass kernel, 'multipass' = decoded by the multi-pass kernels directly, 'redone' = a single-pass result thrown
        away and redone by the multi-pass kernels (errors), 'plan_redone' = a fixed-width-plan result redone by the generic
        kernel, 'control' = batches that took the control path (a Relation / DDL frame), 'chain_rerun' = ASYNC batches run
        again because their predecessor failed."""
        out = (C.c_ulonglong * 8)()
        self.L.etlg_ctx_debug_paths8(self.h, out)
        return dict(zip(("fused", "cells", "multipass", "redone", "plan", "plan_redone", "control", "chain_rerun"), [int(x) for x in out]))

    def debug_rows(self):
        """Batches by the row-synchronous kernel (debugging aid, not in etlg.h): 'rows' = produced by k_rows, 'rows_redone' = handed back by it
        (a tile that did not fit its LDS window / image) and decoded again by k_cells / k_fused."""
        out = (C.c_ulonglong * 3)()
        self.L.etlg_ctx_debug_rows(self.h, out)
        return {"rows": int(out[0]), "rows_redone": int(out[1]), "rows_resized": int(out[2])}

    def debug_copy(self):
        """Table-copy batches by path (debugging aid, not in etlg.h): 'direct' = produced by the rows -> arena kernel (k_copy_cells),
        'frames' = decoded through the row -> frame rewrite (a malformed row, rows wider than a tile's window, ETLG_COPY_DIRECT=0)."""
        out = (C.c_ulonglong * 2)()
        self.L.etlg_ctx_debug_copy(self.h, out)
        return {"direct": int(out[0]), "frames": int(out[1])}

    def debug_ring_recleared(self):
        """Result blocks cleared again after a second attempt behind their lap's re-initialisation (debugging aid, not in etlg.h)."""
        out = (C.c_ulonglong * 8)()
        self.L.etlg_ctx_debug_ring(self.h, out)
        return int(out[0])

    def debug_chains_healed(self):
        """ASYNC chains that were finished early because their last batch was marked for a second attempt (debugging aid)."""
        out = (C.c_ulonglong * 8)()
        self.L.etlg_ctx_debug_ring(self.h, out)
        return int(out[1])

    def debug_chains_spared(self):
        """Second attempts of a fixed-width-plan batch that left the carried transaction state its first attempt had published: the batches
        in flight behind it were NOT decoded again (debugging aid)."""
        out = (C.c_ulonglong * 8)()
        self.L.etlg_ctx_debug_ring(self.h, out)
        return int(out[5])

    def debug_scan_chained(self):
        """(batches whose decode was enqueued behind their boundary scan with the frame count read on the device, those of them that
        had to be decoded again with the count in hand) — debugging aid."""
        out = (C.c_ulonglong * 8)()
        self.L.etlg_ctx_debug_ring(self.h, out)
        return int(out[3]), int(out[4])

    def debug_chain_reissued(self):
        """Always 0: it counted the ASYNC batches of the re-issue experiment (tools/experiments/r06_chain_reissue.diff), which left the tree;
        the word of etlg_ctx_debug_ring stays so that callers keep their layout (debugging aid)."""
        out = (C.c_ulonglong * 8)()
        self.L.etlg_ctx_debug_ring(self.h, out)
        return int(out[2])

    def frame_tags(self, buf, offsets):
        """pgoutput tag of every frame (np.uint8; 0 = malformed), classified on the device (etlg_frame_tags)."""
        import numpy as np
        a = np.ascontiguousarray(buf, dtype=np.uint8)
        o = np.ascontiguousarray(offsets, dtype=np.uint32)
        out = np.zeros(len(o) - 1, dtype=np.uint8)
        rc = self.L.etlg_frame_tags(self.h, a.ctypes.data, len(a), o.ctypes.data, len(o) - 1, 0, out.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"etlg_frame_tags failed: {rc}")
        return out

    def frame_tags_device(self, buf_ptr, nbytes, offs_ptr, nframes, out_ptr):
        """Device-resident variant: raw device pointers in and out."""
        rc = self.L.etlg_frame_tags(self.h, C.c_void_p(buf_ptr), nbytes, C.c_void_p(offs_ptr), nframes,
                                    abi.F_INPUT_ON_DEVICE | abi.F_OUTPUT_ON_DEVICE, C.c_void_p(out_ptr))
        if rc != 0:
            raise RuntimeError(f"etlg_frame_tags failed: {rc}")

    def shard_plan(self, buf, offsets, n_shards):
        """[(f0, f1)] commit-aligned, byte-balanced frame ranges of a HOST stream (etlg_shard_plan: classified and cut on the device)."""
        a = np.ascontiguousarray(buf, dtype=np.uint8)
        o = np.ascontiguousarray(offsets, dtype=np.uint32)
        return self._shard_plan(a.ctypes.data, len(a), o.ctypes.data, len(o) - 1, n_shards, 0)

    def shard_plan_device(self, buf_ptr, nbytes, offs_ptr, nframes, n_shards):
        """... of a device-resident stream (raw device pointers)."""
        return self._shard_plan(buf_ptr, nbytes, offs_ptr, nframes, n_shards, abi.F_INPUT_ON_DEVICE)

    def _shard_plan(self, buf_ptr, nbytes, offs_ptr, nframes, n_shards, flags):
        cuts = np.zeros(n_shards + 1, dtype=np.uint64)
        rc = self.L.etlg_shard_plan(self.h, C.c_void_p(buf_ptr), nbytes, C.c_void_p(offs_ptr), nframes, n_shards, flags, cuts.ctypes.data)
        if rc != abi.OK:
            raise self.last_error()
        return [(int(cuts[k]), int(cuts[k + 1])) for k in range(n_shards)]

    def shard_replay(self, buf, offsets):
        """Applies the control stream of an EARLIER shard to this context and leaves it outside any transaction (etlg_shard_replay)."""
        a = np.ascontiguousarray(buf, dtype=np.uint8)
        o = np.ascontiguousarray(offsets, dtype=np.uint32)
        rc = self.L.etlg_shard_replay(self.h, a.ctypes.data if len(a) else None, len(a), o.ctypes.data, len(o) - 1)
        if rc != abi.OK:
            raise self.last_error()

    def control_stream(self, buf_ptr, nbytes, offs_ptr, nframes, on_device=True):
        """The control stream of a frame range, extracted on the device (etlg_control_stream): (bytes np.uint8, offsets np.uint32,
        tag of the range's last frame). `buf_ptr` / `offs_ptr`: device pointers (or host addresses with on_device=False)."""
        flags = abi.F_INPUT_ON_DEVICE if on_device else 0
        nb, nf, last = C.c_size_t(), C.c_size_t(), C.c_uint32()
        out, offs = np.zeros(1 << 16, dtype=np.uint8), np.zeros(1 << 10, dtype=np.uint32)
        for _ in range(2):
            rc = self.L.etlg_control_stream(self.h, C.c_void_p(buf_ptr), nbytes, C.c_void_p(offs_ptr), nframes, flags, out.ctypes.data, out.size,
                                            offs.ctypes.data, offs.size, C.byref(nb), C.byref(nf), C.byref(last))
            if rc == abi.OK:
                return out[:nb.value].copy(), offs[:nf.value + 1].copy(), int(last.value)
            if rc != abi.InvalidArgument or (nb.value <= out.size and nf.value + 1 <= offs.size):
                raise self.last_error()
            out, offs = np.zeros(nb.value + 64, dtype=np.uint8), np.zeros(nf.value + 2, dtype=np.uint32)
        raise self.last_error()

    def scan_boundaries_device(self, buf_ptr, nbytes, out_ptr, cap):
        """Record-boundary scan of a device-resident stream into a device array of `cap` u32 entries; returns nframes."""
        n = C.c_size_t()
        rc = self.L.etlg_scan_boundaries(self.h, C.c_void_p(buf_ptr), nbytes, abi.F_INPUT_ON_DEVICE | abi.F_OUTPUT_ON_DEVICE,
                                         C.c_void_p(out_ptr), cap, C.byref(n))
        if rc != 0:
            raise RuntimeError(f"etlg_scan_boundaries failed: {rc}")
        return int(n.value)

    def scan_boundaries(self, buf, max_frames=None):
        """Record-boundary scan of a host buffer on the device: np.uint32 offsets (nframes + 1)."""
        import numpy as np
        a = np.ascontiguousarray(buf, dtype=np.uint8)
        cap = (len(a) // 5 + 3) if max_frames is None else max_frames + 1
        out = np.empty(cap, dtype=np.uint32)
        n = C.c_size_t()
        rc = self.L.etlg_scan_boundaries(self.h, a.ctypes.data, len(a), 0, out.ctypes.data, cap, C.byref(n))
        if rc != 0:
            raise RuntimeError(f"etlg_scan_boundaries failed: {rc}")
        return out[:n.value + 1].copy()

    def debug_scan(self):
        """(scans that needed a hinted rerun, scans that fell back to the one-lane walk)."""
        out = (C.c_ulonglong * 2)()
        self.L.etlg_ctx_debug_scan(self.h, out)
        return int(out[0]), int(out[1])
