"""The Iceberg sink's own test vectors for its changelog rows, transcribed by hand from the reference with their file:line. Cells are in
materialize() form, events in the form tests/iceberg_changelog.py takes. Data only."""

# crates/etl/src/event.rs:443-464 generate_sequence_number_fn: (start_lsn, commit_lsn, expected). The string is
# `{commit_lsn:016x}/{start_lsn:016x}` (:370-375) — the layout of EventSequenceKey's Display `{commit_lsn:016x}/{tx_ordinal:016x}` (:346-351)
SEQUENCE_NUMBERS = [
    (0, 0, b"0000000000000000/0000000000000000"),                    # :445-447 — also the copy token, generate_sequence_number(0, 0)
    (1, 0, b"0000000000000000/0000000000000001"),                    # :449-451
    (255, 0, b"0000000000000000/00000000000000ff"),                  # :453-455 (lower-case hex)
    (65535, 0, b"0000000000000000/000000000000ffff"),                # :457-459
    (2**64 - 1, 0, b"0000000000000000/ffffffffffffffff"),            # :461-463
]

# crates/etl-destinations/src/iceberg/core.rs:77-85 IcebergOperationType Display
OPERATIONS = [("I", b"INSERT"), ("U", b"UPDATE"), ("D", b"DELETE")]

# core.rs:778-791 replicated_schema(): users(id int4 primary key, name text), IdentityMask [1, 0]
USERS_ROW = [("I32", 1), ("String", b"alice")]                        # :796, :816
# core.rs:794-840: (event, accepted row | None, refusal reason 1 partial update / 2 key-only delete / 3 delete without an old row)
ROW_IMAGES = [
    ({"kind": "U", "schema_slot": 0, "partial": False, "old_kind": "None", "row": USERS_ROW}, USERS_ROW, 0),      # :794-801 accepts_full_new_row
    ({"kind": "U", "schema_slot": 0, "partial": True, "old_kind": "None", "row": [("I32", 1), ("Missing",)]}, None, 1),   # :804-811 rejects_partial_new_row
    ({"kind": "D", "schema_slot": 0, "old_kind": "Full", "old_row": USERS_ROW}, USERS_ROW, 0),                    # :814-821 accepts_full_old_row
    ({"kind": "D", "schema_slot": 0, "old_kind": "Key", "old_row": [("I32", 1)]}, None, 2),                       # :824-831 rejects_key_only_old_row
    ({"kind": "D", "schema_slot": 0, "old_kind": "None"}, None, 3),                                               # :834-840 rejects_missing_old_row
]

# core.rs:642-678: the descriptions of the three SourceReplicaIdentityErrors, by reason
DESCRIPTIONS = {
    1: "Iceberg update requires a full new row image",               # :644
    2: "Iceberg delete requires a full old row image",               # :663
    3: "Iceberg delete requires an old row image",                   # :672
}
