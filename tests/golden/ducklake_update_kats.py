"""The DuckLake sink's own vectors for partial Updates, transcribed by hand from the reference (crates/etl-destinations/src/ducklake/...),
each with its file:line. Cells are in materialize() form (a column the partial row does not carry is ("Missing",)); events in the form
tests/ducklake_updates.py update_records() takes. Data only."""

# batches.rs prepare_table_mutations_update_*: (column names, identity flags, event, expected assignments, expected predicate)
USERS = (["id", "name"], [1, 0])                                                   # make_replicated_schema :2326-2339
UPDATES = [
    # :2742-2771 update_emits_update_statement: a key image, a partial row that misses nothing (assignments :2763, predicate :2765)
    (USERS[0], USERS[1],
     {"kind": "U", "schema_slot": 0, "partial": True, "old_kind": "Key", "old_row": [("I32", 1)], "row": [("I32", 1), ("String", b"after")]},
     [b'"id" = 1', b"\"name\" = 'after'"], b'"id" = 1'),
    # :2773-2827 uses_alternative_identity_key_for_changed_key_update: IdentityMask [0, 1, 0, 0], missing [3] (assignments :2815-2819,
    # predicate :2821)
    (["id", "email", "name", "payload"], [0, 1, 0, 0],
     {"kind": "U", "schema_slot": 0, "partial": True, "old_kind": "Key", "old_row": [("String", b"alice@example.com")],
      "row": [("I32", 1), ("String", b"alice@new.example.com"), ("String", b"ripe"), ("Missing",)]},
     [b'"id" = 1', b"\"email\" = 'alice@new.example.com'", b"\"name\" = 'ripe'"], b"\"email\" = 'alice@example.com'"),
    # :2829-2890 uses_full_replica_identity_predicate: IdentityMask [1, 1, 1, 1], a full old image, missing [3] (assignments :2874-2878,
    # predicate :2882-2883)
    (["id", "email", "name", "payload"], [1, 1, 1, 1],
     {"kind": "U", "schema_slot": 0, "partial": True, "old_kind": "Full",
      "old_row": [("I32", 1), ("String", b"alice@example.com"), ("String", b"seed"), ("String", b"toast")],
      "row": [("I32", 1), ("String", b"alice@example.com"), ("String", b"grown"), ("Missing",)]},
     [b'"id" = 1', b"\"email\" = 'alice@example.com'", b"\"name\" = 'grown'"],
     b"\"id\" = 1 AND \"email\" = 'alice@example.com' AND \"name\" = 'seed' AND \"payload\" = 'toast'"),
]

# core.rs:2902-2918 key_row_from_updated_partial_row_uses_alternative_identity_columns: make_alternative_identity_schema (:2826-2842,
# IdentityMask [0, 1, 0]), PartialTableRow::new(3, [I32(1), String("alice@example.com")], missing [2]) -> the key row (:2917)
KEY_ROW = (["id", "email", "payload"], [0, 1, 0], [("I32", 1), ("String", b"alice@example.com"), ("Missing",)],
           [("String", b"alice@example.com")])

# core.rs:2920-2937 key_row_from_updated_partial_row_rejects_missing_replica_identity: make_missing_identity_schema (:2844-2852,
# IdentityMask [0, 0]), PartialTableRow::new(2, [I32(1), String("alice")], missing []) -> SourceReplicaIdentityError (:2935-2936)
NO_IDENTITY = (["id", "name"], [0, 0], [("I32", 1), ("String", b"alice")], "DuckLake update requires a replica identity")

# the descriptions of the two other errors the host raises for an event counted in n_host_rows (core.rs:896-905, batches.rs:1337-1346)
MISSING_KEY = "DuckLake partial update is missing replica-identity columns"
NO_ASSIGNMENTS = "DuckLake partial update row has no assignments"
