"""TEST INFRASTRUCTURE — CPU restatement of the DuckLake sink's batch identities, for the parity tests of etlg_ducklake_fingerprints
(etl_amd/csrc/fingerprint.hip; its stream walker fp_walk is this file's event_stream). Never imported by the product path.

Follows crates/etl-destinations/src/ducklake/batches.rs: BatchIdHasher :260-289 (FNV-1a-64: h = (h ^ byte) * 0x100000001b3 from
0xcbf29ce484222325), build_mutation_batch_identity :1402-1446, build_copy_batch_identity :1449-1464, hash_partial_table_row_ref
:1562-1594, and Rust's Hash impls as the reference drives them through Hasher::write: a str / String is its bytes followed by one 0xFF,
a u64 / usize 8 little-endian bytes.

UNPINNED: the reference's tests (:3290-3396) assert only that ids are equal or differ; no fingerprint is written down as a number and
there is no Rust toolchain here to make one. Pinned are FNV-1a (the standard vectors) and the records' bytes (the DuckLake tests);
the interleaving is restated here and in fp_walk, once each.

Records come from tests/ducklake_literals.event_records and tests/ducklake_updates.update_records; the literals of a partial Update's
present cells from ducklake_literals.literal directly (the device cuts them out of the SET record by col_ends)."""
from tests import ducklake_literals as DL
from tests import ducklake_updates as DU

OFFSET_BASIS = 0xCBF29CE484222325
PRIME = 0x100000001B3
M64 = (1 << 64) - 1
HOST = "host"          # a slot event that lacks a record the stream needs


def fnv1a(data, h=OFFSET_BASIS):
    """BatchIdHasher::write over `data` from state `h`: plain and serial."""
    for b in bytes(data):
        h = ((h ^ b) * PRIME) & M64
    return h


def fnv1a_many(data, seeds):
    """fnv1a(data, s) for every s of `seeds` at once (numpy, 64-bit wrap-around): the same serial chain, one lane per seed."""
    import numpy as np
    with np.errstate(over="ignore"):
        h = np.array(seeds, dtype=np.uint64)
        for b in bytes(data):
            h = (h ^ np.uint64(b)) * np.uint64(PRIME)
    return [int(x) for x in h]


def hash_str(s):
    """`impl Hash for str`: the bytes, then 0xFF."""
    return (s.encode() if isinstance(s, str) else bytes(s)) + b"\xff"


def le64(v):
    """`impl Hash for u64 / usize` on a 64-bit little-endian target."""
    return int(v).to_bytes(8, "little")


def seed(kind, table_id):
    """The state the host hands over: after "mutation" / "copy" and table_name.id(), both hashed as strings."""
    return fnv1a(hash_str(kind) + hash_str(table_id))


def event_stream(e, t, p, u, n_cols, copy=False):
    """THE INTERLEAVING: what one slot event feeds the hasher. t / p: its tuple / predicate record or None; u: (predicate record,
    [(column, literal)]) of a partial Update or None. Returns bytes, or HOST when a record the event needs is missing."""
    if copy:
        return HOST if t is None or p is None else hash_str(p) + hash_str(t)
    head = le64(e["start_lsn"]) + le64(e["commit_lsn"])
    k = e["kind"]
    if k == "I":
        return HOST if t is None else head + hash_str("insert") + hash_str(t)
    if k == "D":
        return HOST if p is None else head + hash_str("delete") + hash_str(p)
    if e["partial"]:
        if u is None:
            return HOST
        return head + hash_str("update") + hash_str(u[0]) + le64(n_cols) + b"".join(le64(c) + hash_str(lit) for c, lit in u[1])
    if t is None or p is None:
        return HOST
    return head + hash_str("update" if e["old_kind"] != "None" else "replace") + hash_str(p) + hash_str(t)


def batch_streams(events, slot, names, identity, copy=False, primary_key=None, with_updates=True):
    """Per event of the batch: b"" (not a slot event), its stream, or HOST."""
    tr, ti, _ = DL.event_records(events, slot, names, identity, DL.TUPLES, copy=copy, primary_key=primary_key)
    pr, pi, _ = DL.event_records(events, slot, names, identity, DL.PREDICATES, copy=copy, primary_key=primary_key)
    t_of, p_of, u_of = dict(zip(ti, tr)), dict(zip(pi, pr)), {}
    if with_updates and not copy:
        ur, ui, _, _ = DU.update_records(events, slot, names, identity)
        for k in range(0, len(ur), 2):
            row = events[ui[k]]["row"]
            u_of[ui[k]] = (ur[k + 1], [(c, DL.literal(x)) for c, x in enumerate(row) if not DU.is_missing(x)])
    out = []
    for i, e in enumerate(events):
        if e["kind"] not in "IUD" or e.get("schema_slot") != slot:
            out.append(b"")
        else:
            out.append(event_stream(e, t_of.get(i), p_of.get(i), u_of.get(i), len(names), copy=copy))
    return out


def fingerprints(streams, ranges):
    """([fingerprint per range], None), or (None, the first event inside a range that is HOST)."""
    host = [i for first, end, _ in ranges for i in range(first, end) if streams[i] is HOST]
    if host:
        return None, min(host)
    return [fnv1a(b"".join(streams[first:end]), s) for first, end, s in ranges], None


# ---- the arithmetic the kernels rest on: a run of bytes as a low-byte permutation and an affine map

def low_perm(data):
    """The permutation of 0..255 a run of bytes is for the low byte of the state: l' = ((l ^ b) * 0xB3) & 0xFF per byte."""
    perm = list(range(256))
    for b in bytes(data):
        perm = [((l ^ b) * 0xB3) & 0xFF for l in perm]
    return perm


def affine(data, l):
    """(P^n, C) of a run entered with low byte l: h -> h * P^n + C, from h ^ b == h + d with d = (l ^ b) - l."""
    a, c = 1, 0
    for b in bytes(data):
        c = ((c + ((l ^ b) - l)) * PRIME) & M64
        a = (a * PRIME) & M64
        l = ((l ^ b) * 0xB3) & 0xFF
    return a, c


def fnv1a_split(data, cuts, h=OFFSET_BASIS):
    """The hash of `data` from `h` through the summaries of its pieces (cut at `cuts`): permutations composed for the entering low
    bytes, then the affine maps folded — never a byte-serial chain across pieces."""
    edges = [0] + sorted(cuts) + [len(data)]
    pieces = [bytes(data[a:b]) for a, b in zip(edges, edges[1:])]
    perms = [low_perm(x) for x in pieces]
    l, enter = h & 0xFF, []
    for pm in perms:
        enter.append(l)
        l = pm[l]
    for x, l0 in zip(pieces, enter):
        a, c = affine(x, l0)
        h = (h * a + c) & M64
    return h
