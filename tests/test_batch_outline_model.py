"""tests/batch_outline.py, the sequential restatement of the write_events loop (clickhouse/core.rs:1063-1164; iceberg/core.rs:300-432 with
relations_inline), against expectations written by hand: where each of the 27 three-event patterns over {data, Relation, Truncate} is
split into passes, in both variants; ranges that start inside a Relation run and inside a Truncate run; empty ranges; bad cuts; the
truncate entries and the first-entry-per-table rule; the census. CPU only, no library."""
import itertools

import pytest

from tests import batch_outline as BO

# '|' = a new pass starts. ClickHouse / BigQuery / Snowflake / DuckLake: the data run ends at R or T, then the R run, then the T run.
SPLIT = {
    "DDD": "DDD", "DDR": "DDR", "DDT": "DDT", "DRD": "DR|D", "DRR": "DRR", "DRT": "DRT", "DTD": "DT|D", "DTR": "DT|R", "DTT": "DTT",
    "RDD": "R|DD", "RDR": "R|DR", "RDT": "R|DT", "RRD": "RR|D", "RRR": "RRR", "RRT": "RRT", "RTD": "RT|D", "RTR": "RT|R", "RTT": "RTT",
    "TDD": "T|DD", "TDR": "T|DR", "TDT": "T|DT", "TRD": "T|R|D", "TRR": "T|RR", "TRT": "T|RT", "TTD": "TT|D", "TTR": "TT|R", "TTT": "TTT",
}
# Iceberg: the data run ends at T only and takes the Relations with it.
SPLIT_INLINE = {
    "DDD": "DDD", "DDR": "DDR", "DDT": "DDT", "DRD": "DRD", "DRR": "DRR", "DRT": "DRT", "DTD": "DT|D", "DTR": "DT|R", "DTT": "DTT",
    "RDD": "RDD", "RDR": "RDR", "RDT": "RDT", "RRD": "RRD", "RRR": "RRR", "RRT": "RRT", "RTD": "RT|D", "RTR": "RT|R", "RTT": "RTT",
    "TDD": "T|DD", "TDR": "T|DR", "TDT": "T|DT", "TRD": "T|RD", "TRR": "T|RR", "TRT": "T|RT", "TTD": "TT|D", "TTR": "TT|R", "TTT": "TTT",
}


def _run(pattern, **kw):
    kinds = pattern.replace("D", "I")
    bodies = {i: [(42, 0)] for i, k in enumerate(kinds) if k == "T"}
    return BO.outline(kinds, [0] * len(kinds), [0] * len(kinds), bodies, **kw)


def _expect(split, inline):
    """[(first_event, data_end, rel_end, end_event)] from a split written by hand: the leading data, then Relations, then Truncates."""
    out, at = [], 0
    for part in split.split("|"):
        data = len(part) - len(part.lstrip("DR" if inline else "D"))
        rel = data if inline else len(part) - len(part.lstrip("DR"))
        assert part[rel:] == "T" * (len(part) - rel), part              # (the hand-written split is a pass: nothing falls inside it)
        out.append((at, at + data, at + rel, at + len(part)))
        at += len(part)
    return out


@pytest.mark.parametrize("inline", [False, True])
def test_the_27_three_event_patterns(inline):
    table = SPLIT_INLINE if inline else SPLIT
    assert sorted(table) == sorted("".join(p) for p in itertools.product("DRT", repeat=3))
    for pattern, split in table.items():
        m = _run(pattern, relations_inline=inline)
        got = [(p["first_event"], p["data_end"], p["rel_end"], p["end_event"]) for p in m["passes"]]
        assert got == _expect(split, inline), (pattern, got)
        assert m["info"] == {"n_passes": split.count("|") + 1, "n_trunc": pattern.count("T"), "n_relations": pattern.count("R"),
                             "n_rows": pattern.count("D"), "n_ranges": 1}
        assert [sorted(t) for t in m["touched"]] == [[0] if "D" in part else [] for part in split.split("|")]


def test_ranges_that_start_inside_a_relation_run_and_inside_a_truncate_run():
    #          0123456789
    pattern = "DRRRTTTDRT"
    m = _run(pattern, cuts=[2, 5])                                       # [0, 2) [2, 5) [5, 10)
    got = [(p["first_event"], p["data_end"], p["rel_end"], p["end_event"], p["range"]) for p in m["passes"]]
    assert got == [(0, 1, 2, 2, 0), (2, 2, 4, 5, 1), (5, 5, 5, 7, 2), (7, 8, 9, 10, 2)]
    assert m["info"]["n_ranges"] == 3 and m["info"]["n_passes"] == 4
    m = _run(pattern, cuts=[2, 5], relations_inline=True)
    got = [(p["first_event"], p["data_end"], p["rel_end"], p["end_event"], p["range"]) for p in m["passes"]]
    assert got == [(0, 2, 2, 2, 0), (2, 4, 4, 5, 1), (5, 5, 5, 7, 2), (7, 9, 9, 10, 2)]


def test_empty_ranges_have_no_pass_and_are_counted():
    m = _run("DDTDD", cuts=[0, 2, 2, 2, 5])                              # a cut at `first`, duplicates, a cut at `end`
    got = [(p["first_event"], p["end_event"], p["range"]) for p in m["passes"]]
    assert got == [(0, 2, 1), (2, 3, 4), (3, 5, 4)]
    assert m["info"]["n_ranges"] == 5                                    # the last cut is `end`: no range behind it
    m = _run("DDTDD", cuts=[0, 2, 2, 2])
    assert m["info"]["n_ranges"] == 5 and [p["range"] for p in m["passes"]] == [1, 4, 4]
    m = _run("DDTDD", first=3, end=3)
    assert m["passes"] == [] and m["info"] == {"n_passes": 0, "n_trunc": 0, "n_relations": 0, "n_rows": 0, "n_ranges": 1}
    m = _run("DDTDD", first=3, end=3, cuts=[3, 3])
    assert m["passes"] == [] and m["info"]["n_ranges"] == 2


def test_a_window_behind_a_truncate_starts_a_pass_at_its_first_event():
    m = _run("DTTRD", first=2)
    got = [(p["first_event"], p["data_end"], p["rel_end"], p["end_event"]) for p in m["passes"]]
    assert got == [(2, 2, 2, 3), (3, 3, 4, 4), (4, 5, 5, 5)]
    assert m["info"]["n_trunc"] == 1 and m["info"]["n_rows"] == 1


def test_bad_cuts():
    assert _run("DDDD", cuts=[3, 2]) == {"status": BO.BAD_CUTS, "bad_cut": 1}
    assert _run("DDDD", first=1, cuts=[0, 2]) == {"status": BO.BAD_CUTS, "bad_cut": 0}
    assert _run("DDDD", end=3, cuts=[1, 2, 4]) == {"status": BO.BAD_CUTS, "bad_cut": 2}
    assert _run("DDDD", cuts=[1, 1, 4])["status"] == BO.OK


def test_truncate_entries_in_event_then_body_order_and_the_first_entry_rule():
    kinds = "ITTITI"
    bodies = {1: [(42, 0), (43, 1), (44, 2)], 2: [(43, 5), (42, 0)], 4: []}     # 43 again with another slot; a Truncate of no owned table
    m = BO.outline(kinds, [0] * 6, [0, 0, 0, 1, 0, 2], bodies)
    assert m["truncates"] == [(42, 0, 1), (43, 1, 1), (44, 2, 1), (43, 5, 2), (42, 0, 2)]
    assert [(p["trunc_first"], p["n_trunc"]) for p in m["passes"]] == [(0, 5), (5, 0), (5, 0)]
    assert BO.truncated_tables(m, 0) == [(42, 0, 1), (43, 1, 1), (44, 2, 1)]    # entry().or_insert(): the first schema of a table stays
    assert BO.truncated_tables(m, 1) == [] and BO.truncated_tables(m, 2) == []
    assert [sorted(t) for t in m["touched"]] == [[0], [1], [2]]
    m = BO.outline("TIT", [0] * 3, [0] * 3, {0: [(42, 0)], 2: [(42, 0)]})
    assert BO.truncated_tables(m, 0) == [(42, 0, 0)] and BO.truncated_tables(m, 1) == [(42, 0, 2)]   # the same table again in the next pass


def test_census_categories_and_first_events():
    #        I  U     U partial  D full  D key  D none  I(slot 3)  B  C
    kinds = "IUUDDDIBC"
    flags = [0, 1, 4 | 2, 1, 2, 0, 0, 0, 0]
    slots = [1, 1, 1, 1, 1, 1, 3, 0, 0]
    m = BO.outline(kinds, flags, slots, {})
    assert m["census"] == {1: ([1, 1, 1, 1, 1, 1], [0, 1, 2, 3, 4, 5]), 3: ([1, 0, 0, 0, 0, 0], [6] + [BO.NONE] * 5)}
    assert m["info"]["n_rows"] == 7 and m["rows"] == [{1: [0, 1, 2, 3, 4, 5], 3: [6]}]
    m = BO.outline(kinds, flags, slots, {}, first=2, end=7)
    assert m["census"][1] == ([0, 0, 1, 1, 1, 1], [BO.NONE, BO.NONE, 2, 3, 4, 5]) and m["info"]["n_rows"] == 5
