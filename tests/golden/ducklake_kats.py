"""The DuckLake sink's own test vectors, transcribed by hand from the reference (crates/etl-destinations/src/ducklake/...), each with
its file:line. Cells are in materialize() form; events in the form tests/ducklake_literals.py event_records() takes. Vectors whose
test also checks a partial row's SET assignments are transcribed for their predicate only. Data only."""

# encoding.rs:756-768 array_cell_to_sql_literal_preserves_nulls: (array type oid, source literal, expected text)
ARRAYS = [
    (1007, b"{1,NULL,3}", b"[1, NULL, 3]"),                                        # :758-759 ArrayCell::I32([Some(1), None, Some(3)])
    (199, b'{"{\\"a\\": 1}",NULL}', b"[CAST('{\"a\":1}' AS JSON), NULL]"),         # :762-766 ArrayCell::Json([Some({"a": 1}), None])
]

# encoding.rs:771-780 prepare_rows_uses_sql_literals_for_arrays, :840-842 prepare_copy_rows_falls_back_for_array_columns: (cells, tuple)
TUPLES = [
    ([("I32", 1), ("Deferred", 1007, b"{1,NULL,3}")], b"(1, [1, NULL, 3])"),       # :779
    ([("I32", 1), ("Deferred", 1007, b"{1,NULL}")], b"(1, [1, NULL])"),            # :841
]

# sql.rs:41-46 quote_identifier_escapes_duckdb_identifiers
IDENTIFIERS = [
    ("plain", b'"plain"'),
    ('users"; DROP TABLE other; --', b'"users""; DROP TABLE other; --"'),
]

# batches.rs delete_predicate_from_row_*: (column names, identity flags, full row, expected predicate)
PREDICATES = [
    # :2615-2633 uses_only_replica_identity_columns ("tenant_id" and "id" are the primary key)
    (["tenant_id", "id", "name"], [1, 1, 0], [("I32", 7), ("I32", 42), ("String", b"alice")], b'"tenant_id" = 7 AND "id" = 42'),
    # :2636-2661 supports_alternative_identity_without_primary_key (IdentityMask [0, 1, 0])
    (["id", "email", "name"], [0, 1, 0], [("I32", 7), ("String", b"alice@example.com"), ("String", b"alice")], b"\"email\" = 'alice@example.com'"),
    # :2664-2689 uses_full_replica_identity_columns (IdentityMask [1, 1, 1])
    (["id", "email", "name"], [1, 1, 1], [("I32", 7), ("String", b"alice@example.com"), ("String", b"alice")],
     b"\"id\" = 7 AND \"email\" = 'alice@example.com' AND \"name\" = 'alice'"),
]

# batches.rs:2692-2705 delete_predicate_from_row_rejects_missing_replica_identity: IdentityMask [0, 0] -> SourceReplicaIdentityError
# "DuckLake delete requires a replica identity" (here: the event is counted for the host)
NO_IDENTITY = (["id", "name"], [0, 0], {"kind": "D", "schema_slot": 0, "old_kind": "Full", "old_row": [("I32", 1), ("String", b"alice")]})

# prepare_table_mutations_* / prepare_mutation_table_batches_*: (names, identity, events, expected predicates in event order)
USERS = (["id", "name"], [1, 0])                                                   # make_replicated_schema :2326-2339
MUTATIONS = [
    # :2708-2721 replace_emits_delete_then_upsert: TableMutation::Replace(row) = an Update with a full new row and no old image
    (USERS[0], USERS[1], [{"kind": "U", "schema_slot": 0, "partial": False, "old_kind": "None", "row": [("I32", 1), ("String", b"alice")]}],
     [b'"id" = 1']),
    # :2743-2771 update_emits_update_statement: a key image and a partial new row (predicate :2765)
    (USERS[0], USERS[1], [{"kind": "U", "schema_slot": 0, "partial": True, "old_kind": "Key", "old_row": [("I32", 1)],
                           "row": [("I32", 1), ("String", b"after")]}], [b'"id" = 1']),
    # :2774-2827 uses_alternative_identity_key_for_changed_key_update (IdentityMask [0, 1, 0, 0]; predicate :2821)
    (["id", "email", "name", "payload"], [0, 1, 0, 0],
     [{"kind": "U", "schema_slot": 0, "partial": True, "old_kind": "Key", "old_row": [("String", b"alice@example.com")],
       "row": [("I32", 1), ("String", b"alice@new.example.com"), ("String", b"ripe"), ("Toast",)]}], [b"\"email\" = 'alice@example.com'"]),
    # :2830-2890 uses_full_replica_identity_predicate (IdentityMask [1, 1, 1, 1]; predicate :2882-2883)
    (["id", "email", "name", "payload"], [1, 1, 1, 1],
     [{"kind": "U", "schema_slot": 0, "partial": True, "old_kind": "Full",
       "old_row": [("I32", 1), ("String", b"alice@example.com"), ("String", b"seed"), ("String", b"toast")],
       "row": [("I32", 1), ("String", b"alice@example.com"), ("String", b"grown"), ("Toast",)]}],
     [b"\"id\" = 1 AND \"email\" = 'alice@example.com' AND \"name\" = 'seed' AND \"payload\" = 'toast'"]),
    # :3005-3046 group_contiguous_deletes: two Deletes with full old rows (predicates :3043)
    (USERS[0], USERS[1], [{"kind": "D", "schema_slot": 0, "old_kind": "Full", "old_row": [("I32", 1), ("String", b"alice")]},
                          {"kind": "D", "schema_slot": 0, "old_kind": "Full", "old_row": [("I32", 2), ("String", b"bob")]}],
     [b'"id" = 1', b'"id" = 2']),
]

# batches.rs:2596-2597: the shape of a text predicate as the reference's own failure test writes it by hand
TEXT_PREDICATE = ("token", ("String", b"secret-token"), b"\"token\" = 'secret-token'")
