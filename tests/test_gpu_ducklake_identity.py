"""Device-side DuckLake batch identities (etlg_ducklake_fingerprints, etl_amd/csrc/fingerprint.hip) against tests/ducklake_identity.py
(restatement of crates/etl-destinations/src/ducklake/batches.rs:260-289, 1402-1464, 1562-1594), exact equality: batches of 1 .. 1 025
slot events with one range over everything, ranges that begin and end inside a chunk, one range per event (ranges that hold only another
table's events, Begin or Commit among them) and empty ranges; 256 seeds that differ in the low byte over the same few events; every
replica-identity shape; every event kind in one batch with partial Updates behind MISSING columns and a '"' in a column name; table-copy
batches with and without primary-key columns (empty predicate records); a 256 KiB text cell among short rows; the type-matrix table; the
hand-backs and the argument errors.
The kernels' constants: k_fp_plan takes 256 events per workgroup and k_fp_write 64 (both counts, and one past, are in the list of batch
sizes); the hashing kernels cut the STREAM, not the events, into chunks of 16 384 bytes — test_stream_of_one_chunk_and_one_byte_more
builds a stream of exactly one chunk and of one byte more; k_fp_low walks a range's pieces 64 at a time and k_fp_fold 256 at a time —
test_ranges_of_64_65_256_and_257_pieces gives single ranges of exactly those piece counts and one past.
Every parity case asserts status == ETLG_RB_OK; only the explicit hand-back cases expect ETLG_RB_NEEDS_HOST."""
import numpy as np
import pytest

from etl_amd import abi, synth
from tests import ducklake_identity as ID
from tests import pgwire as W
from tests import scenarios as SC
from tests.test_gpu_duckdb_updates import COLS5, _mixed, _two_tables
from tests.test_gpu_rowbinary import _both, _stream

pytestmark = pytest.mark.gpu
T = W.TOAST
CHUNK = 16384
SEED = ID.seed("mutation", "public_t")


class _Case:
    """One batch and slot: the model's per-event streams and the three device-resident record objects, built once; check() runs one
    set of ranges through the device call."""

    def __init__(self, hb, b, names, slot=0, copy=False, pk=None, with_updates=True):
        self.b, self.names, self.slot = b, names, slot
        events = hb.materialize()
        self.n_events = len(events)
        ident = [c.identity for c in hb.slots[slot].cols]
        self.streams = ID.batch_streams(events, slot, names, ident, copy=copy, primary_key=pk, with_updates=with_updates)
        self.t = b.duckdb(slot, names, what=abi.DL_TUPLES, on_device=True)
        self.p = b.duckdb(slot, names, what=abi.DL_PREDICATES, on_device=True)
        self.u = b.duckdb(slot, names, what=abi.DL_UPDATES, on_device=True) if with_updates else None
        for r in (self.t, self.p, self.u):
            assert r is None or r.status == abi.RB_OK

    def slot_events(self):
        return [i for i, s in enumerate(self.streams) if s is ID.HOST or s]

    def call(self, ranges):
        return self.b.ducklake_fingerprints(self.slot, self.names, ranges, self.t, self.p, self.u)

    def check(self, ranges):
        want, host = ID.fingerprints(self.streams, ranges)
        got, info = self.call(ranges)
        if host is not None:
            assert (info.status, int(info.host_event)) == (abi.RB_NEEDS_HOST, host), (info.status, int(info.host_event), host)
            return None
        assert info.status == abi.RB_OK, (info.status, int(info.host_event))
        assert [int(x) for x in got] == want, [(k, ranges[k][:2], hex(int(g)), hex(w)) for k, (g, w) in enumerate(zip(got, want)) if int(g) != w][:4]
        return want

    def ok_runs(self, seed=SEED):
        """Ranges over the maximal runs of events without a HOST event."""
        runs, first = [], 0
        for i, s in enumerate(self.streams + [ID.HOST]):
            if s is ID.HOST:
                if i > first:
                    runs.append((first, i, seed ^ i))
                first = i + 1
        return runs

    def close(self):
        for r in (self.t, self.p, self.u):
            if r is not None:
                r.close()


COLS3 = [("id", SC.INT8, False, 1), ("v", SC.INT4, True, 0), ("s", 25, True, 0)]
OTHER = [("id", SC.INT8, False, 1), ("t", 25, True, 0)]


def _n_slot_events(n):
    """n Insert / Update / Delete events of table 42 (every full kind, texts of 0 .. 600 bytes) with events of table 43 in between."""
    msgs = []
    for i in range(n):
        row = [str(i), W.NULL if i % 7 == 2 else str(-i), "t'%d" % i * (1 + (i * 37) % 40) if i % 5 else ""]
        m = i % 6
        if m in (0, 1):
            msgs.append(W.insert(42, row))
        elif m == 2:
            msgs.append(W.update(42, row, key=[str(i), W.NULL, W.NULL]))
        elif m == 3:
            msgs.append(W.update(42, row))                                     # TableMutation::Replace
        elif m == 4:
            msgs.append(W.delete(42, key=[str(i), W.NULL, W.NULL]))
        else:
            msgs.append(W.update(42, row, old=row))
        if i % 3 == 1:
            msgs.append(W.insert(43, [str(i), "other %d" % i]))
    return msgs


def _prime2(t):
    SC.simple_table(COLS3)(t)
    SC.simple_table(OTHER, table_id=43)(t)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1025])
def test_batch_sizes_and_range_shapes(n):
    buf, offs = _stream(_n_slot_events(n))
    hb, b, d = _both(_prime2, buf, offs)
    c = _Case(hb, b, [x[0] for x in COLS3])
    ne, se = c.n_events, c.slot_events()
    assert len(se) == n and all(s is not ID.HOST for s in c.streams)
    total = sum(len(s) for s in c.streams)
    if n >= 257:
        assert total > CHUNK                                                   # more than one chunk, cut inside events
    whole = c.check([(0, ne, SEED)])
    assert whole == [ID.fnv1a(b"".join(c.streams), SEED)]
    assert c.check([(se[0], se[-1] + 1, SEED)]) == whole                       # Begin / Commit / the other table add nothing
    # ranges that begin and end in the middle of a chunk, with gaps and an empty range between them
    cuts = sorted({0, ne // 7, ne // 3, ne // 3 + 1, ne // 2, (2 * ne) // 3, ne - 1, ne})
    c.check([(a, z, SEED + k) for k, (a, z) in enumerate(zip(cuts, cuts[1:]))])
    a, m, z = cuts[1], cuts[len(cuts) // 2], cuts[-2]
    c.check([(0, a, 1), (a, a, 2), (max(a, m), max(a, m, z), 3), (ne, ne, 4)])
    # one range per event: Begin, Commit and table 43's events are ranges that hold nothing of the slot and return their seed
    one = c.check([(i, i + 1, SEED ^ (i * 0x9E3779B97F4A7C15 & ID.M64)) for i in range(ne)])
    assert one[0] == SEED and sum(1 for i in range(ne) if one[i] == SEED ^ (i * 0x9E3779B97F4A7C15 & ID.M64)) == ne - n
    assert c.check([(0, 0, 5), (0, 1, 6)]) == [5, 6]                           # an empty range, then Begin alone
    # the other table's own identities on the same batch
    c.close()
    if n >= 2:
        c2 = _Case(hb, b, ["id", "t"], slot=1)
        assert len(c2.slot_events()) == (n + 1) // 3 and c2.check([(0, ne, SEED)])
        c2.close()
    b.close(); d.close()


def test_stream_of_one_chunk_and_one_byte_more():
    cols = [("id", SC.INT8, False, 1), ("s", 25, True, 0)]
    for extra in (0, 1):
        pad = 0
        for _ in range(2):                                                      # the second pass pads the stream to its length
            buf, offs = _stream([W.insert(42, ["1", "a" * 700]), W.insert(42, ["2", "x" * pad]), W.insert(42, ["3", "b" * 900])])
            hb, b, d = _both(SC.simple_table(cols), buf, offs)
            c = _Case(hb, b, ["id", "s"])
            total = sum(len(s) for s in c.streams)
            if total != CHUNK + extra:
                pad = CHUNK + extra - total
                assert pad > 0
                c.close(); b.close(); d.close()
        assert total == CHUNK + extra
        c.check([(0, c.n_events, SEED)])
        c.check([(0, 2, SEED), (2, 3, 7), (3, c.n_events, 9)])
        c.close(); b.close(); d.close()


def test_every_low_byte_of_the_seed():
    """256 calls over the same few events: every row of the pieces' permutations is used, and the carry out of the low byte differs."""
    buf, offs = _stream(_n_slot_events(5))
    hb, b, d = _both(_prime2, buf, offs)
    c = _Case(hb, b, [x[0] for x in COLS3])
    data = b"".join(c.streams)
    seen = set()
    for k in range(256):
        seed = 0x6C62272E07BB0100 ^ k ^ (k << 40)
        got, info = c.call([(0, c.n_events, seed)])
        assert info.status == abi.RB_OK and int(got[0]) == ID.fnv1a(data, seed), k
        seen.add(int(got[0]))
    assert len(seen) == 256
    c.close(); b.close(); d.close()


def _pieces(offs, first, end):
    """Pieces (chunks touched) of the range of events [first, end), from the stream offsets of the events."""
    rb, re = offs[first], offs[end]
    return 0 if rb == re else (re - 1) // CHUNK - rb // CHUNK + 1


BIG = [("id", SC.INT8, False, 1), ("s", 25, True, 0)]


def test_every_low_byte_of_the_seed_across_a_chunk_boundary():
    """256 calls over a range of two pieces: every row of the SECOND piece's permutation goes through k_fp_low's chain as well."""
    buf, offs = _stream([W.insert(42, [str(i), ("%d'r\\" % i) * 1500]) for i in range(4)])
    hb, b, d = _both(SC.simple_table(BIG), buf, offs)
    c = _Case(hb, b, ["id", "s"])
    so = np.cumsum([0] + [len(x) for x in c.streams]).tolist()
    assert _pieces(so, 2, 4) == 2 and so[2] % CHUNK and so[4] % CHUNK           # begins and ends inside a chunk
    seeds = [0x6C62272E07BB0100 ^ k ^ (k << 40) for k in range(256)]
    want = ID.fnv1a_many(b"".join(c.streams[2:4]), seeds)
    for k in range(256):
        got, info = c.call([(2, 4, seeds[k])])
        assert info.status == abi.RB_OK and int(got[0]) == want[k], k
    assert len(set(want)) == 256
    c.close(); b.close(); d.close()


def test_ranges_of_64_65_256_and_257_pieces():
    """k_fp_low takes a range's permutations 64 at a time and k_fp_fold its maps 256 at a time: single ranges of exactly 64, 65, 256 and
    257 pieces (1 - 4.2 MB of stream) reach the second batch of both loops, its one-piece tail, and the state carried between batches;
    a second range of 65 pieces behind one of 64 has its pieces' ids offset by the range index. The model hashes the stream serially
    once and notes the state at every event (nested ranges from one seed share it)."""
    msgs = [W.insert(42, [str(i), ("%d'row\\" % i) * 1100]) for i in range(420)]
    buf, offs = _stream(msgs)
    hb, b, d = _both(SC.simple_table(BIG), buf, offs)
    c = _Case(hb, b, ["id", "s"])
    assert all(s is not ID.HOST for s in c.streams) and max(len(s) for s in c.streams) < CHUNK
    so = np.cumsum([0] + [len(x) for x in c.streams]).tolist()
    state, h = [SEED, SEED], SEED                                               # state[e]: after the events [1, e)
    for s in c.streams[1:]:
        h = ID.fnv1a(s, h)
        state.append(h)
    end = {}
    for want in (64, 65, 256, 257):
        end[want] = next(e for e in range(2, c.n_events + 1) if _pieces(so, 1, e) == want)
        got, info = c.call([(1, end[want], SEED)])
        assert info.status == abi.RB_OK and int(got[0]) == state[end[want]], (want, hex(int(got[0])), hex(state[end[want]]))
    e2 = next(e for e in range(end[64] + 1, c.n_events + 1) if _pieces(so, end[64], e) == 65)
    got, info = c.call([(0, 1, 9), (1, end[64], SEED), (end[64], e2, state[end[64]]), (e2, e2, 11)])
    assert info.status == abi.RB_OK and [int(x) for x in got] == [9, state[end[64]], state[e2], 11]
    c.close(); b.close(); d.close()


@pytest.mark.parametrize("ident_name", ["Default", "Index", "Full", "None"])
def test_identity_shapes(ident_name):
    ident = {"Default": [0, 1, 0, 1, 0], "Index": [0, 0, 1, 1, 0], "Full": [1, 1, 1, 1, 1], "None": [0, 0, 0, 0, 0]}[ident_name]
    buf, offs = _stream(_mixed(ident))
    hb, b, d = _both(_two_tables(ident), buf, offs)
    c = _Case(hb, b, [x[0] for x in COLS5])
    hosts = [i for i, s in enumerate(c.streams) if s is ID.HOST]
    assert hosts                                                               # (every shape leaves some partial Update to the host)
    assert c.check([(0, c.n_events, SEED)]) is None                            # NEEDS_HOST at the first of them
    runs = c.ok_runs()
    assert len(runs) > 5 and c.check(runs)
    if ident_name in ("Default", "Index"):                                     # partial Updates the device hashes
        assert any(e["kind"] == "U" and e.get("partial") and c.streams[i] not in (b"", ID.HOST) for i, e in enumerate(hb.materialize()))
    c.close(); b.close(); d.close()


QCOLS = [('a"x', SC.INT4, True, 0), ("k", SC.INT8, False, 1), ('s""', 25, True, 0), ("m", 25, True, 0), ('bi"g', 25, True, 0)]


def test_every_event_kind_in_one_batch():
    names = [x[0] for x in QCOLS]
    row = ["5", "1", "it's", "mm", "big"]
    key = [W.NULL, "1", W.NULL, W.NULL, W.NULL]
    msgs = [W.insert(42, row), W.delete(42, old=row), W.delete(42, key=key), W.update(42, row, old=row), W.update(42, row, key=key), W.update(42, row),
            W.update(42, [T, "1", 'q"', T, T]),                                  # leading MISSING column, no old image
            W.update(42, [T, T, T, "only m", T], key=key),                       # three leading MISSING columns, a key image
            W.update(42, ["7", "2", W.NULL, T, 'b"']),                           # NULL in the SET clause, the quoted last column present
            W.update(42, [T, "1", T, T, T]), W.insert(42, ["6", "2", "", W.NULL, ""])]
    buf, offs = _stream(msgs)
    hb, b, d = _both(SC.simple_table(QCOLS), buf, offs)
    c = _Case(hb, b, names)
    ev = hb.materialize()
    assert [e["kind"] for e in ev[1:-1]] == list("IDDUUUUUUUI") and [bool(e.get("partial")) for e in ev[4:11]] == [False] * 3 + [True] * 4
    assert all(s is not ID.HOST for s in c.streams)
    assert b'replace\xff"k" = 1\xff(5, 1, \'it\'\'s\', \'mm\', \'big\')\xff' in c.streams[6]
    assert c.streams[7].endswith(b'update\xff"k" = 1\xff' + ID.le64(5) + ID.le64(1) + b"1\xff" + ID.le64(2) + b"'q\"'\xff")
    assert c.streams[9].endswith(ID.le64(0) + b"7\xff" + ID.le64(1) + b"2\xff" + ID.le64(2) + b"NULL\xff" + ID.le64(4) + b"'b\"'\xff")
    c.check([(0, c.n_events, SEED)])
    c.check([(i, i + 1, SEED + i) for i in range(c.n_events)])
    c.close()
    # without the updates object the partial Updates are the host's; ranges in front of the first are served
    c = _Case(hb, b, names, with_updates=False)
    assert c.check([(0, c.n_events, SEED)]) is None and c.check([(0, 3, 1), (3, 7, 2), (8, 8, 3)])
    got, info = c.call([(0, 7, 1), (9, 12, 2)])
    assert (info.status, int(info.host_event)) == (abi.RB_NEEDS_HOST, 9)
    c.close(); b.close(); d.close()


def _copy_batch(cols, pk, rows):
    from etl_amd.decoder import Decoder
    from oracle import oracle
    o, d = oracle.Oracle(), Decoder(0)
    for t in (o, d):
        t.schema_put(42, 0, cols)
    so, sd = o.table_ready(42, 0, [1] * len(cols), pk), d.table_ready(42, 0, [1] * len(cols), pk)
    buf = np.frombuffer(b"".join(rows), dtype=np.uint8)
    offs = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint32)
    rb, gb = o.copy_decode(so, buf, offs), d.copy_decode(sd, buf, offs, flags=abi.F_OUTPUT_ON_DEVICE)
    assert gb.rc == 0 and rb.err_code == 0
    return rb.host_batch(), gb, d


@pytest.mark.parametrize("pk", [[1, 0, 0, 1], [0, 0, 0, 0]])
def test_table_copy_batch(pk):
    """P FF T FF per row, no LSNs; without primary-key columns every predicate record is empty (one 0xFF per row)."""
    cols = [("id", SC.INT8, False, pk[0]), ("s", 25, True, pk[1]), ("f", SC.FLOAT8, True, pk[2]), ("k", 25, True, pk[3])]
    rows = [b"%d\ttext %d\\twith tab and ' quote\t%s\t%s\n" % (i, i, b"1.5" if i % 2 else b"\\N", b"\\N" if i % 5 == 0 else b"k%d" % i) for i in range(400)]
    hb, gb, d = _copy_batch(cols, pk, rows)
    c = _Case(hb, gb, [x[0] for x in cols], copy=True, pk=pk, with_updates=False)
    seed = ID.seed("copy", "public_t")
    assert c.n_events == 400 and sum(len(s) for s in c.streams) > CHUNK
    assert c.streams[0].startswith(b'"id" = 0 AND "k" IS NULL\xff(' if any(pk) else b"\xff(")
    assert c.check([(0, 400, seed)]) == [ID.fnv1a(b"".join(c.streams), seed)]
    c.check([(0, 1, seed), (1, 100, seed), (100, 100, 3), (101, 399, seed)])
    c.close()
    u = gb.duckdb(0, [x[0] for x in cols], what=abi.DL_UPDATES, on_device=True)   # a copy batch has no Updates: an empty object changes nothing
    c = _Case(hb, gb, [x[0] for x in cols], copy=True, pk=pk, with_updates=False)
    c.u = u
    c.check([(0, 400, seed)])
    c.close(); gb.close(); d.close()


def test_one_text_cell_of_256_kib_among_short_rows():
    cols = [("id", SC.INT8, False, 1), ("s", 25, True, 0)]
    big = ("0123456789abcde'" * (256 * 1024 // 16))
    msgs = [W.insert(42, [str(i), "s%d" % i]) for i in range(40)] + [W.insert(42, ["40", big])] + [W.update(42, [str(i), "u"]) for i in range(41, 80)]
    buf, offs = _stream(msgs)
    hb, b, d = _both(SC.simple_table(cols), buf, offs)
    c = _Case(hb, b, ["id", "s"])
    assert len(c.streams[41]) > 256 * 1024 + 16384                             # (the quotes are doubled)
    c.check([(0, c.n_events, SEED)])
    c.check([(0, 41, 1), (41, 42, 2), (42, c.n_events, 3)])
    c.close(); b.close(); d.close()


def test_type_matrix_table():
    from etl_amd.decoder import Decoder
    from oracle import oracle
    o, d = oracle.Oracle(), Decoder(0)
    buf, offs = synth.type_matrix_stream(40, mix=True)
    synth.type_matrix_register(o)
    synth.type_matrix_register(d)
    rb = o.decode(buf, offs)
    assert rb.err_code == 0
    gb = d.decode(buf, offs, flags=abi.F_NO_CONTROL | abi.F_OUTPUT_ON_DEVICE)
    assert gb.rc == 0, gb.error
    c = _Case(rb.host_batch(), gb, [x[0] for x in synth.TYPE_MATRIX_COLS])
    assert len(c.slot_events()) >= 40 and max(len(s) for s in c.streams if s is not ID.HOST) > 1000
    if any(s is ID.HOST for s in c.streams):
        assert c.check([(0, c.n_events, SEED)]) is None
    runs = c.ok_runs()
    assert runs and c.check(runs)
    c.check([(a, a + (z - a) // 2, s) for a, z, s in runs])
    c.close(); gb.close(); d.close()


def test_hand_backs():
    # a slot without identity columns: Updates and Deletes have no predicate record
    cols = [("id", SC.INT8, False, 0), ("s", 25, True, 0)]
    buf, offs = _stream([W.insert(42, ["1", "a"]), W.insert(42, ["2", "b"]), W.delete(42, old=["1", "a"]), W.insert(42, ["3", "c"]), W.update(42, ["2", "x"])])
    hb, b, d = _both(SC.simple_table(cols, ident=[0, 0]), buf, offs)
    c = _Case(hb, b, ["id", "s"])
    assert [i for i, s in enumerate(c.streams) if s is ID.HOST] == [3, 5]
    assert c.check([(0, c.n_events, SEED)]) is None
    got, info = c.call([(0, 3, 1), (4, 6, 2)])
    assert (info.status, int(info.host_event)) == (abi.RB_NEEDS_HOST, 5) and not got.any()      # no fingerprint is written
    assert c.check([(0, 3, 1), (4, 5, 2), (6, 7, 3)])                           # the ranges around them
    c.close(); b.close(); d.close()


def test_argument_errors():
    from etl_amd.decoder import EtlError
    deferred = "50537618.817359292015891086651596749e82"                        # a float text the fast rule leaves DEFERRED
    buf, offs = _stream(_n_slot_events(6))
    hb, b, d = _both(_prime2, buf, offs)
    names = [x[0] for x in COLS3]
    c = _Case(hb, b, names)
    ne = c.n_events
    other = _Case(hb, b, ["id", "t"], slot=1)
    hb2, b2, d2 = _both(_prime2, buf, offs)
    foreign = b2.duckdb(0, names, what=abi.DL_TUPLES, on_device=True)
    on_host = b.duckdb(0, names, what=abi.DL_TUPLES)
    whole = [(0, ne, SEED)]

    def bad(ranges=whole, t=None, p=None, u=c.u, nm=names, slot=0):
        with pytest.raises(EtlError) as ei:
            b.ducklake_fingerprints(slot, nm, ranges, t or c.t, p or c.p, u)
        assert ei.value.kind == abi.InvalidArgument

    bad(t=foreign)                                                             # another batch
    bad(t=other.t); bad(p=other.p); bad(u=other.u)                             # another slot
    bad(t=c.p); bad(p=c.t); bad(u=c.t); bad(t=c.u)                             # another `what`
    bad(t=on_host)                                                             # on the host
    bad(nm=names[:2]); bad(nm=names + ["x"])                                   # n_names
    bad(slot=1)                                                                # (the objects are slot 0's)
    bad(ranges=[(3, 5, 1), (0, 2, 2)]); bad(ranges=[(0, 4, 1), (3, 5, 2)])     # not ascending, not disjoint
    bad(ranges=[(0, ne + 1, 1)]); bad(ranges=[(4, 3, 1)])                      # beyond the batch, backwards
    assert c.check(whole) and c.check([]) == [] and c.check([(0, 2, 1), (2, 2, 2), (2, ne, 3)])   # the same objects are fine; touching ranges are disjoint
    for r in (foreign, on_host):
        r.close()
    other.close(); c.close(); b2.close(); d2.close(); b.close(); d.close()
    # an object that came back as ETLG_RB_NEEDS_HOST
    cols = [("id", SC.INT8, False, 1), ("f", SC.FLOAT8, True, 0)]
    buf, offs = _stream([W.insert(42, ["1", "1.5"]), W.insert(42, ["2", deferred])])
    hb, b, d = _both(SC.simple_table(cols), buf, offs)
    t = b.duckdb(0, ["id", "f"], what=abi.DL_TUPLES, on_device=True)
    p = b.duckdb(0, ["id", "f"], what=abi.DL_PREDICATES, on_device=True)
    assert t.status == abi.RB_NEEDS_HOST and p.status == abi.RB_OK
    with pytest.raises(EtlError) as ei:
        b.ducklake_fingerprints(0, ["id", "f"], [(0, 1, 1)], t, p, None)
    assert ei.value.kind == abi.InvalidArgument
    t.close(); p.close(); b.close(); d.close()
