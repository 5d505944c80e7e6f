"""The host model of the DuckLake batch identities (tests/ducklake_identity.py) on its own: FNV-1a against the standard vectors, the
`str` / `u64` encodings, the per-kind streams of a hand-written five-event batch spelled out as literal bytes, and the split identity —
hashing a stream in pieces through the low-byte permutations and the affine maps equals the serial hash — which pins the arithmetic
etl_amd/csrc/fingerprint.hip rests on independently of the kernels."""
import random

from tests import ducklake_identity as ID


def test_fnv1a_standard_vectors():
    assert ID.fnv1a(b"") == 0xCBF29CE484222325
    assert ID.fnv1a(b"a") == 0xAF63DC4C8601EC8C
    assert ID.fnv1a(b"foobar") == 0x85944171F73967E8
    assert ID.fnv1a(b"bar", ID.fnv1a(b"foo")) == 0x85944171F73967E8         # the state carries over writes


def test_many_seeds_at_once_equal_the_serial_hash():
    seeds = [0xCBF29CE484222325, 0, ID.M64, 0x6C62272E07BB01FF, 7]
    for data in (b"", b"a", b"foobar", bytes(range(256)) * 3):
        assert ID.fnv1a_many(data, seeds) == [ID.fnv1a(data, s) for s in seeds]


def test_str_and_u64_encodings():
    assert ID.hash_str("insert") == b"insert\xff" and ID.hash_str(b"") == b"\xff" and ID.hash_str("é") == b"\xc3\xa9\xff"
    assert ID.le64(1) == b"\x01" + b"\0" * 7 and ID.le64(0x0102030405060708) == bytes(range(8, 0, -1)) and ID.le64(2**64 - 1) == b"\xff" * 8
    assert ID.seed("mutation", "public_t") == ID.fnv1a(b"mutation\xffpublic_t\xff")
    assert ID.seed("copy", "a") != ID.seed("mutation", "a")


def _ev(kind, start, commit, **kw):
    return dict(kind=kind, start_lsn=start, commit_lsn=commit, partial=False, old_kind="None", **kw)


def test_per_kind_streams_of_a_five_event_batch():
    lsn = b"\x10\x00\x00\x00\x00\x00\x00\x00" + b"\x00\x01\x00\x00\x00\x00\x00\x00"
    t, p = b"(1, 'a')", b'"id" = 1'
    assert ID.event_stream(_ev("I", 16, 256), t, None, None, 2) == lsn + b"insert\xff(1, 'a')\xff"
    assert ID.event_stream(_ev("D", 16, 256, ), None, p, None, 2) == lsn + b'delete\xff"id" = 1\xff'
    assert ID.event_stream(dict(_ev("U", 16, 256), old_kind="Key"), t, p, None, 2) == lsn + b'update\xff"id" = 1\xff(1, \'a\')\xff'
    assert ID.event_stream(dict(_ev("U", 16, 256), old_kind="Full"), t, p, None, 2) == lsn + b'update\xff"id" = 1\xff(1, \'a\')\xff'
    assert ID.event_stream(_ev("U", 16, 256), t, p, None, 2) == lsn + b'replace\xff"id" = 1\xff(1, \'a\')\xff'
    part = dict(_ev("U", 16, 256), partial=True)
    assert ID.event_stream(part, None, None, (p, [(0, b"1"), (2, b"'x'")]), 3) == (
        lsn + b'update\xff"id" = 1\xff' + b"\x03" + b"\0" * 7 + b"\0" * 8 + b"1\xff" + b"\x02" + b"\0" * 7 + b"'x'\xff")
    # a table-copy row: P FF T FF, no LSNs; an empty predicate (no primary key) is one 0xFF
    assert ID.event_stream(_ev("I", 0, 0), t, p, None, 2, copy=True) == b'"id" = 1\xff(1, \'a\')\xff'
    assert ID.event_stream(_ev("I", 0, 0), t, b"", None, 2, copy=True) == b"\xff(1, 'a')\xff"
    # a record the kind needs is missing
    for e, tt, pp, uu in ((_ev("I", 1, 2), None, p, None), (_ev("D", 1, 2), t, None, None), (_ev("U", 1, 2), t, None, None), (_ev("U", 1, 2), None, p, None),
                          (part, t, p, None)):
        assert ID.event_stream(e, tt, pp, uu, 2) is ID.HOST
    streams = [b"", b"ab", ID.HOST, b"", b"cd"]
    assert ID.fingerprints(streams, [(0, 2, 7), (3, 5, 9), (5, 5, 11)]) == ([ID.fnv1a(b"ab", 7), ID.fnv1a(b"cd", 9), 11], None)
    assert ID.fingerprints(streams, [(0, 2, 7), (2, 5, 9)]) == (None, 2)


def test_low_byte_permutation_and_affine_map_of_a_run():
    rng = random.Random(11)
    for n in (0, 1, 2, 63, 64, 300):
        data = bytes(rng.randrange(256) for _ in range(n))
        perm = ID.low_perm(data)
        assert sorted(perm) == list(range(256))
        for h in (ID.OFFSET_BASIS, 0, ID.M64, rng.getrandbits(64), rng.getrandbits(64)):
            want = ID.fnv1a(data, h)
            assert perm[h & 0xFF] == want & 0xFF
            a, c = ID.affine(data, h & 0xFF)
            assert a == pow(ID.PRIME, n, 1 << 64) and (h * a + c) & ID.M64 == want


def test_split_identity_for_random_cuts():
    rng = random.Random(5)
    for trial in range(60):
        n = rng.choice([0, 1, 5, 64, 65, 257, 1000, 3000])
        data = bytes(rng.randrange(256) for _ in range(n)) if trial % 3 else bytes([0xFF, 0x00, 0x80])[: min(n, 3)] * (n // 3 + 1)
        cuts = sorted(rng.randrange(len(data) + 1) for _ in range(rng.choice([0, 1, 2, 7, 40])))   # repeated cuts: empty pieces
        for h in (ID.OFFSET_BASIS, rng.getrandbits(64), 0xFF, 0):
            assert ID.fnv1a_split(data, cuts, h) == ID.fnv1a(data, h), (trial, n, cuts[:5], hex(h))
    assert ID.fnv1a_split(b"foobar", [3]) == 0x85944171F73967E8 and ID.fnv1a_split(b"foobar", [0, 1, 1, 6]) == 0x85944171F73967E8
