"""DATA ONLY — the outcomes of the reference's own unit tests of the Iceberg sink's two row-image functions
(crates/etl-destinations/src/iceberg/core.rs:794-840): per test its name, the function, the image the test passes, and whether the
function accepts it or refuses it with ErrorKind::SourceReplicaIdentityError — with the error's description text (core.rs:644, :663,
:672), which the driver raises for the reason the plan reports."""

# (test, function, image, accepted, description of the error)
ROW_IMAGE_KATS = [
    ("iceberg_update_row_accepts_full_new_row", "iceberg_update_row", "full", True, None),
    ("iceberg_update_row_rejects_partial_new_row", "iceberg_update_row", "partial", False, "Iceberg update requires a full new row image"),
    ("iceberg_delete_row_accepts_full_old_row", "iceberg_delete_row", "full", True, None),
    ("iceberg_delete_row_rejects_key_only_old_row", "iceberg_delete_row", "key", False, "Iceberg delete requires a full old row image"),
    ("iceberg_delete_row_rejects_missing_old_row", "iceberg_delete_row", "none", False, "Iceberg delete requires an old row image"),
]
