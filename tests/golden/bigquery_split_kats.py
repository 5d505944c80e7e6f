"""The reference's own vectors for the BigQuery table-copy split, as data: the unit tests of split_table_rows and of
calculate_target_batches_for_table_copy in crates/etl-destinations/src/bigquery/core.rs (the functions: :1760-1784, :1790-1827).
Every entry names the test and its lines. tests/test_bigquery_plan_model.py holds tests/bigquery_plan.py against them,
tests/test_gpu_bigquery_plan.py reproduces the split vectors through etlg_bigquery_plan."""

# (test, core.rs lines, total_rows, target_batches) -> the lengths of the batches, in order
SPLIT_TABLE_ROWS = [
    ("split_table_rows_empty_input", "2277-2281", 0, 4, []),
    ("split_table_rows_zero_concurrent_streams", "2284-2289", 1, 0, [1]),
    ("split_table_rows_single_concurrent_stream", "2292-2300", 2, 1, [2]),
    ("split_table_rows_fewer_rows_than_streams", "2303-2311", 2, 5, [2]),
    ("split_table_rows_equal_distribution", "2314-2321", 4, 2, [2, 2]),
    ("split_table_rows_uneven_distribution", "2324-2332", 5, 3, [2, 2, 1]),
    ("split_table_rows_many_streams", "2335-2350", 10, 4, [3, 3, 2, 2]),
    ("split_table_rows_single_row", "2353-2358", 1, 5, [1]),
]

# The vectors of calculate_target_batches_for_table_copy that do not depend on the client crate's MAX_BATCH_SIZE_BYTES, whose value the
# reference does not state: (test, core.rs lines, rows, the first row relative to the budget) -> target_batches.
#   "small": a row far below any plausible budget; "over": a row of MAX_BATCH_SIZE_BYTES + 1 payload bytes, longer than the budget.
CALCULATE_TARGET_BATCHES = [
    ("calculate_target_batches_empty_rows", "2361-2365", 0, None, 0),
    ("calculate_target_batches_single_small_row", "2368-2376", 1, "small", 1),
    ("calculate_target_batches_very_large_single_row", "2408-2419", 1, "over", 1),
]
# Not asserted, the constant is not in the reference:
#   calculate_target_batches_many_small_rows (:2379-2390): 100 000 rows of "value_{i}" (about 50 bytes encoded) -> 1
#   calculate_target_batches_large_rows      (:2393-2405): 50 rows of a 1 MiB string -> 3
# (the latter holds for any budget B with 17 <= B // len(row) <= 24, that is between about 17 and 25 MiB: ceil(50 / 17) = ceil(50 / 24) = 3)
