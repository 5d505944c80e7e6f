"""bench.py's all-cores CPU leg (SURVEY.md §8(d) leg (ii)): every frame of every batch is decoded exactly once
across the commit-aligned shards, by independent oracle contexts. And what --dump-outputs writes of a decoded batch."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench  # noqa: E402
from etl_amd import synth  # noqa: E402


def test_threads_leg_covers_every_frame():
    w = synth.cfg3()
    pool = [w.fill(2 << 20) for _ in range(2)]
    r = bench.cpu_baseline_threads(w, pool, 3, 0.2)
    assert r["cores"] == 3 and r["unit"] == "GB/s" and r["value"] > 0
    frames = sum(len(o) - 1 for _, o in pool)
    nbytes = sum(len(b) for b, _ in pool)
    # events_per_s and value are quoted on the same best pass: their ratio is frames / bytes of the pool
    assert abs(r["events_per_s"] / (r["value"] * 1e9) - frames / nbytes) < 0.01 * frames / nbytes


def test_cpu_threads_default_is_bounded():
    assert 1 <= bench.cpu_threads(0) <= 64
    assert bench.cpu_threads(5) == 5


class _Decoded:
    """A decoded batch as bench.dump_outputs sees one: host() hands back the arena (here the oracle's)."""
    def __init__(self, hb):
        self.hb = hb

    def host(self):
        return self.hb


def _oracle_batch(mk=synth.cfg2, cap=1 << 20):
    from oracle import oracle
    w = mk()
    o = oracle.Oracle()
    w.register(o)
    buf, offs = w.fill(cap)
    rb = o.decode(buf, offs)
    assert rb.err_code == 0
    return rb.host_batch()


def test_dump_outputs_writes_every_arena_array_exactly(tmp_path):
    import numpy as np
    hb = _oracle_batch()
    bench.dump_outputs(_Decoded(hb), str(tmp_path))
    for name in hb.ARRAYS:
        if not len(getattr(hb, name)):   # (cfg2 writes no heap bytes: no file, its length is in counts.npy)
            assert not (tmp_path / (name + ".npy")).exists(), name
            continue
        a = np.load(tmp_path / (name + ".npy"))
        assert a.dtype == np.float64 and len(a) and np.array_equal(a, getattr(hb, name).astype(np.float64)), name
    counts = np.load(tmp_path / "counts.npy")
    assert list(counts[:4]) == [hb.n_events, hb.n_frames, len(hb.fixed), len(hb.heap)]


def test_dump_outputs_samples_long_arrays_at_fixed_positions(tmp_path, monkeypatch):
    import numpy as np
    hb = _oracle_batch()
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 1000)
    bench.dump_outputs(_Decoded(hb), str(tmp_path / "a"))
    bench.dump_outputs(_Decoded(hb), str(tmp_path / "b"))
    assert len(hb.fixed) > 1000
    for name in hb.ARRAYS:
        if not len(getattr(hb, name)):
            continue
        a, b = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert len(a) == min(1000, len(getattr(hb, name))) and np.array_equal(a, b), name
    full = hb.fixed.astype(np.float64)
    a = np.load(tmp_path / "a" / "fixed.npy")
    assert np.isin(a, full).all()


def test_dump_outputs_writes_the_heap_of_a_text_workload(tmp_path):
    import numpy as np
    hb = _oracle_batch(synth.cfg3, 128 << 10)
    assert 0 < len(hb.heap) <= bench.DUMP_MAX_ELEMS
    bench.dump_outputs(_Decoded(hb), str(tmp_path))
    for name in hb.ARRAYS:
        a = np.load(tmp_path / (name + ".npy"))
        assert len(a) and np.array_equal(a, getattr(hb, name).astype(np.float64)), name
