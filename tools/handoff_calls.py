"""Every hand-off call once per interesting argument, on the SIMT emulator, with the emulator's call log on: the file ETLG_SIMT_CALLS names
gets one line per runtime call the host code makes (launches with kernel symbol and grid, copies with size and direction, memsets, stops,
allocations; tests/simt/simt.h) and, from this script, a `# section` line in front of every hand-off call and a `-> outcome` line behind
it. Two builds of the host layer that issue the same calls in the same order write the same file: the comparison a host refactor needs
beside byte-for-byte output.

  ETLG_LIB_PATH=<emulator library> ETLG_SIMT_RUN=1 ETLG_SIMT_CALLS=<log> python tools/handoff_calls.py

Batches: synth.type_matrix_stream (every class, mixed Inserts / Updates / Deletes), a small cfg3 batch, table-copy batches (one with an
Arrow form, one without, one under a lowered offset cap), and one small batch per error path of the row formats and of the columns."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from etl_amd import abi, synth  # noqa: E402
from etl_amd.decoder import Decoder, EtlError  # noqa: E402
from tests import pgwire as W  # noqa: E402
from tests import scenarios as SC  # noqa: E402

LOG = os.environ["ETLG_SIMT_CALLS"]
assert os.environ.get("ETLG_SIMT_RUN") == "1", "this tool runs on the emulator build (tests/simt)"


def note(text):
    with open(LOG, "a") as f:
        f.write(text + "\n")


def call(name, fn):
    note("# " + name)
    try:
        r = fn()
    except EtlError as e:
        note(f"-> error kind {e.kind} code {e.code} frame {e.frame_index} | {e.description} | {e.detail}")
        return
    v = r.view
    out = [f"rows {int(v.n_rows)}", f"on_device {int(v.on_device)}"]
    for k in ("n_cols", "n_bytes", "status", "n_host_rows", "host_event", "host_column"):
        if hasattr(v, k):
            out.append(f"{k} {int(getattr(v, k))}")
    for k in ("ducklake", "changelog"):
        info = getattr(r, k, None)
        if info is not None:
            out.append(k + " " + " ".join(str(int(getattr(info, f))) for f, _ in info._fields_ if not f.startswith("_")))
    note("-> " + ", ".join(out))
    r.close()


def row_formats(b, names, nullable, tag, engines=(abi.CH_MERGE_TREE, abi.CH_REPLACING_MERGE_TREE)):
    for dev in (False, True):
        where = "device" if dev else "host"
        for e in engines:
            call(f"{tag} rowbinary engine {e} {where}", lambda: b.rowbinary(0, nullable + [0, 0], e, on_device=dev))
        call(f"{tag} protobuf {where}", lambda: b.protobuf(0, on_device=dev))
        call(f"{tag} ndjson {where}", lambda: b.ndjson(0, names, on_device=dev))
        for what in (abi.DL_TUPLES, abi.DL_PREDICATES, abi.DL_UPDATES):
            call(f"{tag} duckdb what {what} {where}", lambda: b.duckdb(0, names, what, on_device=dev))


def columns(b, tag, kinds_list, options):
    for dev in (False, True):
        where = "device" if dev else "host"
        for kinds in kinds_list:
            for pa, fj in options:
                call(f"{tag} columns {''.join(kinds)} parse_arrays {int(pa)} format_json {int(fj)} {where}",
                     lambda: b.columns(0, kinds=kinds, on_device=dev, parse_arrays=pa, format_json=fj))
        for pa, fj in options:
            call(f"{tag} iceberg parse_arrays {int(pa)} format_json {int(fj)} {where}", lambda: b.iceberg(0, parse_arrays=pa, format_json=fj, on_device=dev))


def wal_batch(prime, buf, offs, flags=abi.F_OUTPUT_ON_DEVICE):
    d = Decoder(0)
    prime(d)
    b = d.decode(buf, offs, flags=flags)
    assert b.rc == 0, b.error
    return b, d


def small(cols, rows):
    s = SC.txn([W.insert(42, r) for r in rows])
    return wal_batch(SC.simple_table(cols), np.frombuffer(s.bytes(), dtype=np.uint8), s.offsets)


def copy_batch(cols, rows, cap=None):
    lines = [("\t".join(rows_cell for rows_cell in r) + "\n").encode() for r in rows]
    buf = np.frombuffer(b"".join(lines), dtype=np.uint8)
    offs = np.cumsum([0] + [len(x) for x in lines]).astype(np.uint32)
    if cap is not None:
        os.environ["ETLG_DLC_OFFSET_CAP"] = str(cap)   # (read when the context is created)
    d = Decoder(0)
    os.environ.pop("ETLG_DLC_OFFSET_CAP", None)
    d.schema_put(42, 0, cols)
    slot = d.table_ready(42, 0, [1] * len(cols), [1 if c[3] else 0 for c in cols])
    b = d.copy_decode(slot, buf, offs, flags=abi.F_OUTPUT_ON_DEVICE)
    assert b.rc == 0, b.error
    return b, d


def main():
    every = [(False, False), (True, False), (False, True), (True, True)]
    # 1. the type matrix: every class, Inserts / Updates with a key image / Deletes by key
    buf, offs = synth.type_matrix_stream(300, rows_per_txn=70, mix=True)
    b, d = wal_batch(synth.type_matrix_register, buf, offs)
    names = [c[0] for c in synth.TYPE_MATRIX_COLS]
    columns(b, "type_matrix", [("I",), ("U",), ("I", "U")], every)
    row_formats(b, names, [1] * len(names), "type_matrix")
    b.close(); d.close()
    # 2. a small cfg3 batch (twelve mixed columns, several workgroups)
    w = synth.cfg3()
    buf, offs = w.fill(192 << 10)
    b, d = wal_batch(w.register, buf, offs, abi.F_OUTPUT_ON_DEVICE | abi.F_NO_CONTROL)
    nc = int(b.view().slots[0].n_cols)
    columns(b, "cfg3", [("I", "U")], [(False, False)])
    row_formats(b, [f"c{i}" for i in range(nc)], [1] * nc, "cfg3")
    b.close(); d.close()
    # 3. table-copy batches: one with an Arrow form, one without, one over a lowered offset cap
    cols = [("id", SC.INT4, False, 1), ("a", 25, True, 0), ("n", SC.NUMERIC, True, 0), ("t", 25, True, 0)]
    rows = [[str(i), "ab" * (i % 7), "\\N" if i % 5 == 0 else "%d.%02d" % (i, i % 100), "%040d" % i] for i in range(257)]
    b, d = copy_batch(cols, rows)
    for dev in (False, True):
        call(f"copy ducklake_copy {'device' if dev else 'host'}", lambda: b.ducklake_copy(0, on_device=dev))
    columns(b, "copy", [("I",)], [(False, False)])
    row_formats(b, [c[0] for c in cols], [1] * len(cols), "copy")
    b.close(); d.close()
    b, d = copy_batch(cols, rows, cap=4096)
    for dev in (False, True):
        call(f"copy ducklake_copy over the offset cap {'device' if dev else 'host'}", lambda: b.ducklake_copy(0, on_device=dev))
    b.close(); d.close()
    b, d = copy_batch([("id", SC.INT4, False, 1), ("s", 25, True, 0), ("v", SC.UUID, True, 0)], [[str(i), "x", "123e4567-e89b-12d3-a456-426614174000"] for i in range(65)])
    for dev in (False, True):
        call(f"copy ducklake_copy refused table {'device' if dev else 'host'}", lambda: b.ducklake_copy(0, on_device=dev))
    b.close(); d.close()
    # 4. the error paths of rows_report_error, one batch each, and the columns' first malformed cell
    idc = ("id", SC.INT8, False, 1)
    deferred = "50537618.817359292015891086651596749e82"   # a float text the fast rule leaves DEFERRED: the host's cell
    for tag, cols, rows, fn in (
            ("json error", [idc, ("j", 114, True, 0)], [["1", "{}"], ["2", "{bad"]], lambda b: b.rowbinary(0, [0, 1, 0, 0])),
            ("host cell", [idc, ("x", SC.FLOAT8, True, 0)], [["1", "1.5"], ["2", deferred]], lambda b: b.ndjson(0, ["id", "x"])),
            ("host cell updates", [idc, ("x", SC.FLOAT8, True, 0)], [["1", "1.5"], ["2", deferred]], lambda b: b.duckdb(0, ["id", "x"], abi.DL_TUPLES, on_device=True)),
            ("snowflake NaN", [idc, ("x", SC.FLOAT8, True, 0)], [["1", "1"], ["2", "NaN"]], lambda b: b.ndjson(0, ["id", "x"])),
            ("snowflake numeric infinity", [idc, ("n", SC.NUMERIC, True, 0)], [["1", "1"], ["2", "Infinity"]], lambda b: b.ndjson(0, ["id", "n"])),
            ("bigquery numeric scale", [idc, ("n", SC.NUMERIC, True, 0)], [["1", "1"], ["2", "1e-40"]], lambda b: b.protobuf(0)),
            ("bigquery array null", [idc, ("a", SC.INT4_A, True, 0)], [["1", "{1}"], ["2", "{1,NULL}"]], lambda b: b.protobuf(0)),
            ("clickhouse null", [idc, ("s", 25, True, 0)], [["1", "x"], ["2", W.NULL]], lambda b: b.rowbinary(0, [0, 0, 0, 0])),
            ("clickhouse date range", [idc, ("d", SC.DATE, True, 0)], [["1", "2000-01-01"], ["2", "1800-01-01"]], lambda b: b.rowbinary(0, [0, 1, 0, 0])),
            ("width mismatch", [idc, ("s", 25, True, 0)], [["1", "x"]], lambda b: b.rowbinary(0, [0, 0, 0])),
            ("malformed array", [idc, ("a", SC.INT4_A, True, 0), ("c", SC.INT4_A, True, 0)], [["1", "{1,2}", "{3}"], ["2", "{1,2", "{4}"]], lambda b: b.columns(0, parse_arrays=True)),
            ("array handed back", [idc, ("a", SC.INT4_A, True, 0)], [["1", "{1,2}"], ["2", "{{1},{2}}"], ["3", "{1"]], lambda b: b.columns(0, parse_arrays=True)),
            ("malformed json column", [idc, ("j", 114, True, 0)], [["1", "{}"], ["2", "{bad"]], lambda b: b.columns(0, format_json=True))):
        b, d = small(cols, rows)
        call("error path: " + tag, lambda: fn(b))
        b.close(); d.close()
    note("# end")


if __name__ == "__main__":
    main()
