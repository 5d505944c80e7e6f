"""tests/batch_cuts.py on its own: the sequential cut rule against a second, independent formulation — the plain prefix sums of the hints
and one binary search per cut (the batch that starts at a ends at the smallest e with P[e] - P[a] >= budget), which is also the
decomposition etl_amd/csrc/finish.hip rests on — over random hint arrays with fixed seeds and the edge budgets; INCOMPLETE events, carries,
sub-ranges, chained ranges, and locate() with repeated row_event entries."""
import bisect
import random

import numpy as np

from tests import batch_cuts as BC


def _by_prefix_sums(hints, budget, carry_in=0, first=0, end=None):
    end = len(hints) if end is None else end
    inc = np.flatnonzero(hints[first:end] >> np.uint64(63))
    stop = first + int(inc[0]) if len(inc) else end
    P = [0] + [int(x) for x in np.cumsum(hints[first:stop], dtype=np.uint64)]   # P[k]: the first k hints of the range
    L, out, a, owed = stop - first, [], 0, budget - carry_in
    while True:
        e = bisect.bisect_left(P, P[a] + owed, a + 1)
        if e > L:
            break
        out.append(first + e)
        a, owed = e, budget
    return out, {"n_cuts": len(out), "stop_event": stop, "carry_out": P[L] - P[a] + (0 if out else carry_in), "total": P[L]}


def _budgets(h, rng):
    clean = [int(x) for x in h if not int(x) >> 63] or [1]
    total = sum(clean)
    return sorted({1, min(clean) or 1, max(clean) or 1, max(clean) + 1, max(1, total // 3), max(1, total), total + 1} | {rng.randrange(1, total + 2) for _ in range(5)})


def _arrays():
    rng = random.Random(0xC075)
    yield np.zeros(0, dtype=np.uint64)
    for n in (1, 2, 3, 64, 257, 1000):
        yield np.array([rng.randrange(1, 600) for _ in range(n)], dtype=np.uint64)
        yield np.full(n, 104, dtype=np.uint64)
        yield np.array([rng.choice([24, 24, 24, 5000, 1]) for _ in range(n)], dtype=np.uint64)


def test_sequential_rule_equals_prefix_sums_and_searches():
    rng = random.Random(1)
    for h in _arrays():
        for budget in _budgets(h, rng):
            for carry in sorted({0, 1, budget - 1}):
                if carry < budget:
                    assert BC.cuts(h, budget, carry) == _by_prefix_sums(h, budget, carry), (len(h), budget, carry)


def test_budget_one_cuts_behind_every_event_and_total_plus_one_never():
    h = np.array([7, 1, 300, 2], dtype=np.uint64)
    assert BC.cuts(h, 1) == ([1, 2, 3, 4], {"n_cuts": 4, "stop_event": 4, "carry_out": 0, "total": 310})
    assert BC.cuts(h, 310) == ([4], {"n_cuts": 1, "stop_event": 4, "carry_out": 0, "total": 310})
    assert BC.cuts(h, 311) == ([], {"n_cuts": 0, "stop_event": 4, "carry_out": 310, "total": 310})
    assert BC.cuts(h, 311, carry_in=1) == ([4], {"n_cuts": 1, "stop_event": 4, "carry_out": 0, "total": 310})
    assert BC.cuts(h, 8) == ([2, 3], {"n_cuts": 2, "stop_event": 4, "carry_out": 2, "total": 310})      # 7 + 1 | 300 | 2 open


def test_incomplete_events_stop_the_walk():
    h = np.array([5, 5, 5 | (1 << 63), 5, 5], dtype=np.uint64)
    assert BC.cuts(h, 10) == ([2], {"n_cuts": 1, "stop_event": 2, "carry_out": 0, "total": 10})
    assert BC.cuts(h, 10, first=2) == ([], {"n_cuts": 0, "stop_event": 2, "carry_out": 0, "total": 0})
    assert BC.cuts(h, 10, carry_in=3, first=2) == ([], {"n_cuts": 0, "stop_event": 2, "carry_out": 3, "total": 0})
    assert BC.cuts(h, 10, first=3) == ([5], {"n_cuts": 1, "stop_event": 5, "carry_out": 0, "total": 10})
    rng = random.Random(2)
    h = np.array([rng.randrange(1, 90) | ((1 << 63) if rng.random() < 0.02 else 0) for _ in range(700)], dtype=np.uint64)
    for first in (0, 100, 333):
        for budget in (1, 50, 1000, 10 ** 6):
            assert BC.cuts(h, budget, 0, first) == _by_prefix_sums(h, budget, 0, first)


def test_ranges_chained_through_the_carry_equal_one_range():
    rng = random.Random(3)
    h = np.array([rng.randrange(1, 400) for _ in range(900)], dtype=np.uint64)
    for budget in (1, 77, 400, 5000, 10 ** 5):
        whole, wi = BC.cuts(h, budget)
        for mid in (0, 1, 449, 899, 900):
            a, ai = BC.cuts(h, budget, 0, 0, mid)
            b, bi = BC.cuts(h, budget, ai["carry_out"], mid, 900)
            assert a + b == whole and bi["carry_out"] == wi["carry_out"] and ai["total"] + bi["total"] == wi["total"]
    assert BC.cuts(h, 50, carry_in=49, first=10, end=10) == ([], {"n_cuts": 0, "stop_event": 10, "carry_out": 49, "total": 0})


def test_locate_keeps_the_rows_of_one_event_together():
    row_event = [0, 0, 3, 4, 4, 4, 9]
    assert list(BC.locate(row_event, [0, 1, 4, 5, 9, 10])) == [0, 2, 3, 6, 6, 7]
    assert list(BC.locate([], [3])) == [0] and len(BC.locate(row_event, [])) == 0
