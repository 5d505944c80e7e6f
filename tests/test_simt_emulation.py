"""Kernel logic on a box without a GPU: the kernel sources of etl_amd/csrc and host.cpp are compiled with g++
against a small SIMT emulator (tests/simt: lanes are fibers, wave / workgroup collectives are rendezvous points)
and the parity test files run against that build in a subprocess. TEST INFRASTRUCTURE only — the product never
contains the emulator (etl_amd/native.py refuses to load it outside this run), and the emulator models neither
timing nor memory ordering nor races between waves: the -m gpu suite on an MI355X stays the gate."""
import os
import queue
import subprocess
import sys
import threading

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIMT = os.path.join(ROOT, "tests", "simt")
CXXFLAGS = ["-std=c++17", "-O1", "-g", "-pthread", "-fno-strict-aliasing", "-Wno-unknown-pragmas", "-Wno-attributes", "-I", os.path.join(SIMT, "include")]


@pytest.fixture(scope="module")
def simt_lib():
    sys.path.insert(0, SIMT)
    try:
        import build as simt_build
    finally:
        sys.path.pop(0)
    return simt_build.build()


def test_emulator_primitives_against_scalar_loops(tmp_path):
    exe = str(tmp_path / "simt_selftest")
    subprocess.check_call(["g++"] + CXXFLAGS + [os.path.join(SIMT, "selftest.cpp"), os.path.join(SIMT, "simt.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:]
    # the same binary with the scheduling models on: several workgroups resident, lazy streams (selftest.cpp's stream_tests: event order,
    # the stale read of an unordered consumer, pageable / pinned copy semantics, a polling kernel, hipFree draining)
    for extra in ({"ETLG_SIMT_GRID": "3"}, {"ETLG_SIMT_STREAMS": "lazy"}, {"ETLG_SIMT_STREAMS": "random", "ETLG_SIMT_SEED": "5"}):
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, **extra))
        assert out.returncode == 0, (extra, out.stdout[-2000:])


def test_product_loader_refuses_the_emulator_build(simt_lib):
    code = "from etl_amd import native\ntry:\n    native.lib()\nexcept native.NativeLibraryMissing as e:\n    print('refused')\n"
    env = dict(os.environ, ETLG_LIB_PATH=simt_lib)
    env.pop("ETLG_SIMT_RUN", None)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
    assert "refused" in out.stdout, out.stdout + out.stderr


def _emu_env(simt_lib, timeout, order=None, drop=("ETLG_FUSED_KERNEL", "ETLG_FORCE_MULTIPASS", "ETLG_FUSED_DBG", "ETLG_PLAN", "ETLG_PLAN_DBG", "ETLG_PLAN_PRE"), grid=None, streams=None):
    env = dict(os.environ, ETLG_LIB_PATH=simt_lib, ETLG_SIMT_RUN="1", ETLG_SIMT_WATCHDOG=str(timeout))
    for k in ("ETLG_SIMT_ORDER", "ETLG_SIMT_GRID", "ETLG_SIMT_GRID_ORDER", "ETLG_SIMT_SEED", "ETLG_SIMT_BIG_BYTES", "ETLG_SIMT_STREAMS"):
        env.pop(k, None)
    if streams:   # "lazy": enqueued work runs as late as the HIP ordering rules allow (tests/simt/simt.h)
        env["ETLG_SIMT_STREAMS"] = streams
    if grid or streams:   # these runs also start every workgroup's dynamic LDS and every device allocation as garbage, as the GPU may
        env["ETLG_SIMT_LDS_POISON"] = env["ETLG_SIMT_MALLOC_POISON"] = "1"
    if grid:   # several workgroups resident and interleaved: (how many, "shuffle" | "reverse") — tests/simt/simt.cpp
        env["ETLG_SIMT_GRID"], env["ETLG_SIMT_GRID_ORDER"] = str(grid[0]), grid[1]
    if order:
        env["ETLG_SIMT_ORDER"] = order   # the lanes of a workgroup run in another order than 0, 1, 2, ... between rendezvous (tests/simt/simt.cpp)
    for k in drop:
        env.pop(k, None)
    return env


def _pytest_job(args, timeout, order=None, grid=None, streams=None):
    return dict(cmd=[sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider"] + args, timeout=timeout, order=order, drop=None, grid=grid, streams=streams)


# Every emulated run of this file is a subprocess of its own (the parity files pick the library up from the environment). They run side
# by side, at most one per CPU this process may use, the longest first: each run is single-threaded, and its time limit (also the
# emulator's watchdog, ETLG_SIMT_WATCHDOG) counts from its own start, so a box with few CPUs makes the suite longer, not the runs
# time out. The suite's wall time is about the sum of the runs over the CPUs.
_JOBS = {
    "scenarios": _pytest_job(["tests/test_gpu_parity.py", "-k", "scenario_parity or temporal_matrix or wider_than_16 or type_matrix"], 900),
    "shim_twin": _pytest_job(["tests/test_shim_twin.py"], 600),
    "shard_async": _pytest_job(["tests/test_shard_decode.py", "tests/test_gpu_async.py", "-k", "not 8-"], 900),
    "copy_scan": _pytest_job(["tests/test_gpu_copy.py", "tests/test_gpu_scan.py", "-k", "not device_resident and not device_input and not 16777216"], 600),
    "plans": _pytest_job(["tests/test_gpu_fixed_plan.py", "tests/test_gpu_fuzz.py", "-k", "fixed_plan or k_plan or prepass or (cfg2 and default)"], 900),
    "finish_pass": _pytest_job(["tests/test_gpu_finish.py"], 600),
    "round6_lazy_streams": _pytest_job(["tests/test_gpu_finish.py", "tests/test_gpu_async.py", "-k", "finish or behind_its_boundary_scan or without_a_sidecar or result_ring"], 900, streams="lazy"),
    "hand_off": _pytest_job(["tests/test_gpu_columns.py", "tests/test_gpu_rowbinary.py", "tests/test_gpu_size_hints.py", "tests/test_gpu_protobuf.py", "tests/test_arrow_kats.py", "tests/test_gpu_json_display.py"], 600),
    "hand_off_lazy": _pytest_job(["tests/test_gpu_columns.py", "tests/test_gpu_rowbinary.py", "tests/test_gpu_protobuf.py", "tests/test_gpu_ndjson.py", "tests/test_gpu_duckdb.py",
                                  "tests/test_gpu_duckdb_updates.py", "tests/test_gpu_iceberg.py", "tests/test_gpu_copy_sinks.py", "-k", "not full_size and not synthetic"], 600, streams="lazy"),
    "lane_order": _pytest_job(["tests/test_gpu_copy.py", "tests/test_gpu_rowbinary.py", "tests/test_gpu_protobuf.py",
                               "-k", "not device_resident and not device_input and not 16777216 and not synthetic and not kat_ and not random"], 600, order="shuffle"),
    "plans_shuffled": _pytest_job(["tests/test_gpu_fixed_plan.py", "-k", "prepass or conforming or mix_in_one_launch"], 900, order="shuffle"),
    "resident_shuffle": _pytest_job(["tests/test_gpu_fuzz.py", "-k", "back_to_back"], 900, grid=(8, "shuffle")),
    "resident_reverse": _pytest_job(["tests/test_gpu_fuzz.py", "-k", "many_tile and not cfg2"], 900, grid=(8, "reverse")),
    "lazy_streams": _pytest_job(["tests/test_gpu_async.py", "tests/test_shim_twin.py", "tests/test_gpu_copy.py", "-k",
                                 "(async or shim or twin or chain or copy_generated) and not device_resident and not device_input and not 16777216"], 900, streams="lazy"),
    "other_compiler": dict(cmd=[sys.executable, os.path.join(ROOT, "tools", "simt_other_compiler.py")], timeout=900, order=None, drop=None),
    "long_chains": dict(cmd=[sys.executable, os.path.join(ROOT, "tools", "async_long_fuzz.py"), "45", "21"], timeout=600, order=None,
                        drop=("ETLG_FUSED_KERNEL", "ETLG_FORCE_MULTIPASS", "ETLG_FUSED_DBG", "ETLG_PLAN", "ETLG_PLAN_DBG", "ETLG_PLAN_PRE", "ETLG_OVERLAP")),
    "copy_fuzz": dict(cmd=[sys.executable, os.path.join(ROOT, "tools", "copy_fuzz.py"), "160", "101"], timeout=600, order=None,
                      drop=("ETLG_FUSED_KERNEL", "ETLG_FORCE_MULTIPASS", "ETLG_FUSED_DBG", "ETLG_COPY_DIRECT", "ETLG_COPY_KERNEL")),
    "cell_fuzz": dict(cmd=[sys.executable, os.path.join(ROOT, "tools", "cell_fuzz.py"), "3", "7"], timeout=600, order=None,
                      drop=("ETLG_FUSED_KERNEL", "ETLG_FORCE_MULTIPASS", "ETLG_FUSED_DBG")),
}


def _cpus():
    """CPUs this process may use: its affinity mask, within the cgroup's CPU quota when there is one and within MAX_JOBS when the
    environment sets that budget."""
    n = len(os.sched_getaffinity(0))
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            vals = open(path).read().split()
            if path.endswith("cpu.max"):
                quota, period = vals
            else:
                quota, period = vals[0], open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read().split()[0]
            if quota not in ("max", "-1"):
                n = min(n, max(1, int(quota) // int(period)))
        except (OSError, ValueError):
            pass
    if os.environ.get("MAX_JOBS", "").isdigit():
        n = min(n, int(os.environ["MAX_JOBS"]))
    return max(1, n)


# the longest runs first (alone, on one CPU each: scenarios 310 s, lazy_streams 245, shard_async 187, resident_reverse 138, then 80 s and
# less): the suite ends soon after its longest run
_ORDER = ["scenarios", "lazy_streams", "shard_async", "resident_reverse", "plans", "copy_scan", "lane_order", "other_compiler",
          "round6_lazy_streams", "shim_twin", "resident_shuffle", "plans_shuffled", "hand_off_lazy", "finish_pass", "hand_off", "long_chains",
          "copy_fuzz", "cell_fuzz"]
assert sorted(_ORDER) == sorted(_JOBS)


class _EmuJobs:
    """The emulated runs of _JOBS, started in _ORDER by _cpus() workers; result(name) waits for one of them."""

    def __init__(self, simt_lib):
        self.simt_lib = simt_lib
        self.results = {}
        self.done = {name: threading.Event() for name in _JOBS}
        self.running = {}
        self.stop = False
        self.queue = queue.Queue()
        for name in _ORDER:
            self.queue.put(name)
        self.workers = [threading.Thread(target=self._work, daemon=True) for _ in range(min(_cpus(), len(_ORDER)))]
        for t in self.workers:
            t.start()

    def _work(self):
        while not self.stop:
            try:
                name = self.queue.get_nowait()
            except queue.Empty:
                return
            j = _JOBS[name]
            env = _emu_env(self.simt_lib, j["timeout"], j["order"], grid=j.get("grid"), streams=j.get("streams")) if j["drop"] is None else _emu_env(self.simt_lib, j["timeout"], j["order"], j["drop"])
            pr = subprocess.Popen(j["cmd"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT, env=env)
            self.running[name] = pr
            try:
                out, err = pr.communicate(timeout=j["timeout"] + 120)
            except subprocess.TimeoutExpired:
                pr.kill()
                out, err = pr.communicate()
                err += f"\n(killed after {j['timeout'] + 120} s)"
            self.results[name] = (pr.returncode, out, err)
            self.done[name].set()

    def result(self, name):
        self.done[name].wait()
        return self.results[name]

    def close(self):
        self.stop = True
        for pr in list(self.running.values()):
            if pr.poll() is None:
                pr.kill()
        for t in self.workers:
            t.join()


@pytest.fixture(scope="module")
def emu_jobs(simt_lib):
    jobs = _EmuJobs(simt_lib)
    yield jobs
    jobs.close()


def _result(emu_jobs, name):
    """(return code, stdout, stderr) of one of the emulated runs."""
    return emu_jobs.result(name)


def _passed(emu_jobs, name):
    rc, out, err = _result(emu_jobs, name)
    tail = out[-3000:] + err[-1000:]
    assert rc == 0, tail
    assert " passed" in tail and "failed" not in tail, tail
    return tail


def test_scenarios_on_every_kernel_path(emu_jobs):
    """Every scenario of tests/scenarios.py on the device paths (default choice, k_fused 256 / 64, k_cells, the plan kernels,
    multi-pass), byte for byte against the oracle — the same test the GPU box runs, on emulated kernels; plus the temporal matrix
    (fast paths + chrono grammar) and tables of 17 / 24 / 32 columns (k_cells' WIDE instantiation)."""
    _passed(emu_jobs, "scenarios")


def test_rust_shim_twin(emu_jobs):
    """tests/native/shim_twin.cpp — the Rust crate's call sequence (ring of pinned buffers, decode_async / finish, the oversize-message
    path, FlushTracker, InFlight's drop order) through the C ABI — over fuzzed streams on the emulated library: events against the
    oracle's, LSN bookkeeping against the reference's per-message rules."""
    _passed(emu_jobs, "shim_twin")


def test_sharded_decode_and_async_chain(emu_jobs):
    """The multi-GPU recipe (cut after Commit, broadcast control frames, decode per shard, concatenate) and the ASYNC batch
    chain (device-side carried transaction state, poisoned successors), through the C ABI and the emulated kernels."""
    _passed(emu_jobs, "shard_async")


def test_copy_rows_and_boundary_scan(emu_jobs):
    _passed(emu_jobs, "copy_scan")


def test_fixed_width_plans(emu_jobs):
    """k_plan (plan.hip) and the fixed-width plan of k_fused (fixed_tile.hip.h): their own parity file with the demand that
    conforming streams really take the plan, and the cfg2 mutation fuzz on the default path (k_plan first, the generic kernel
    behind it)."""
    _passed(emu_jobs, "plans")


def test_fixed_width_plans_with_the_lanes_shuffled(emu_jobs):
    """The plan kernels and the sidecar pre-pass (workgroups of sixteen waves, LDS hand-over of the waves' aggregates, a ticket, the last
    group's scan) with the lanes of a workgroup run in a shuffled order between rendezvous: results must not depend on it."""
    _passed(emu_jobs, "plans_shuffled")


def test_look_back_kernels_with_workgroups_interleaved(emu_jobs):
    """The kernels that talk between workgroups of one launch (the two-level look-backs of k_fused / k_cells / k_plan2, the pre-pass's
    ticket and group words, the descriptor buffers in rotation) with EIGHT workgroups resident at a time and the processor changing hands
    between them in a shuffled order, at every poll and after a random number of scheduling rounds: a tile then meets words its
    predecessors have not written yet — aggregates instead of inclusive prefixes, empty words, whatever an earlier launch left in the
    buffer. Clean many-tile batches of different streams and sizes back to back on one context per kernel path, every arena byte against
    the oracle. (The emulator's default — one workgroup after the other — shows none of this: VERDICT r4. A kernel that skips the
    clear of the next-but-one descriptor buffer passes the default run and fails this one.)"""
    _passed(emu_jobs, "resident_shuffle")


def test_look_back_kernels_newest_workgroup_first(emu_jobs):
    """The same machinery in the order that is worst for a look-back: among the resident workgroups the NEWEST one that is not waiting
    runs first, so every tile resolves as early as the protocol allows and finds its predecessors as late as it allows; mutated
    many-tile batches of the variable-length and the DDL workloads (error cut, rerun by the multi-pass kernels, the next batch reusing
    the buffers) on every kernel path."""
    _passed(emu_jobs, "resident_reverse")


def test_host_orchestration_with_lazy_streams(emu_jobs):
    """The library's stream plumbing (two decode streams, control / copy / result / scan streams, events between them) under the
    emulator's LAZY stream model: every enqueued kernel, copy and memset runs as late as the HIP ordering rules allow — when the host
    synchronises with its stream or event, or when a stream that is being run reaches a wait for it; copies from pageable memory are
    staged at the call, copies into pageable memory complete at the call, pinned memory is read and written when the copy runs; a kernel
    that polls for another stream's result (the late carry of a batch decoded BESIDE its predecessor) lets the other streams' work run.
    Work the host code forgot to order then happens in the wrong order and the arenas differ from the oracle's. The ASYNC chains
    (device-chained state, ring laps, reruns, the pipelined control path, pinned host input), the Rust shim's twin and the ASYNC table
    copy. (With the decode streams' wait for a batch's upload taken out, these tests pass under immediate execution and fail here;
    the whole -m gpu suite passes this way — 1 635 tests)"""
    _passed(emu_jobs, "lazy_streams")


def test_scenarios_on_the_library_built_by_rocm_clang(emu_jobs):
    """tools/simt_other_compiler.py: the emulated library built by ROCm's clang++ -O2 (hipcc's front and middle end) instead of g++ -O1,
    every scenario on every kernel path against the oracle. Skipped where that compiler is not installed."""
    rc, out, err = _result(emu_jobs, "other_compiler")
    if rc == 77:
        pytest.skip("no ROCm clang++ in this image")
    tail = out[-3000:] + err[-1000:]
    assert rc == 0 and " passed" in tail and "failed" not in tail, tail


def test_columnar_hand_off(emu_jobs):
    """etlg_batch_columns / etlg_batch_rowbinary (columns.hip, rowformats.hip): the Arrow-layout buffers built by the emulated kernels against
    the host hand-off of the oracle's arena, the RowBinary bytes against oracle/rowbinary.py."""
    _passed(emu_jobs, "hand_off")


def test_hand_off_builders_with_lazy_streams_and_poisoned_memory(emu_jobs):
    """build_columns and handoff_rows (host_handoff_columns.inc, host_handoff_rows.inc) behind all seven entry points with enqueued work
    running as late as the HIP ordering rules allow, LDS and device allocations starting as garbage: a scratch block (the select
    scratch, block S) or a device block given back ahead of the stop that covers it is read after it went to the next taker, and the
    bytes differ from the oracle's. The columns, row-format, Iceberg and table-copy files, without their full-size cases (50 s alone)."""
    _passed(emu_jobs, "hand_off_lazy")


def test_finish_pass_typed_arrays_and_exact_floats(emu_jobs):
    """etlg_batch_finish_cells / ETLG_F_FINISH_CELLS (finish.hip: k_fin_count / k_fin_fill, float_slow.h): the reference's array vectors
    through the emulated kernels, the type-matrix table, fuzzed literals in every image, the float matrix — tests/test_gpu_finish.py."""
    _passed(emu_jobs, "finish_pass")


def test_round6_paths_with_lazy_streams_and_poisoned_memory(emu_jobs):
    """The finish pass, the decode enqueued behind its boundary scan and the guarded result ring with enqueued work running as late as the
    HIP ordering rules allow, LDS and device allocations starting as garbage: a missing event / a read of something never written shows."""
    _passed(emu_jobs, "round6_lazy_streams")


def test_long_async_chains_with_second_attempts(emu_jobs):
    """tools/async_long_fuzz.py: chains of 80-200 cfg2 batches on ONE context (the result ring laps several times), a random window in
    flight, an UPDATE the fixed-width plan does not cover in a few batches (decoded again at their sync, with the batches behind them):
    every batch against the oracle, and the chain has to heal — second attempts within a window's worth per such batch. Against the
    host code before round 5's second session every chain reports CHAIN DID NOT HEAL."""
    rc, out, err = _result(emu_jobs, "long_chains")
    assert rc == 0 and " 0 problems" in out, out[-2000:] + err[-1000:]


def test_copy_mutation_fuzz(emu_jobs):
    """tools/copy_fuzz.py on the emulated kernels: generated COPY rows with a few mutated bytes (specials, invalid UTF-8, deletions) or
    many benign escape insertions, table-copy path against the oracle — same error, same row, same arena before it; a batch the
    reference rejects never comes out of the one-kernel path. (It found the out-of-field copy loop behind a malformed row boundary.)"""
    rc, out, err = _result(emu_jobs, "copy_fuzz")
    assert rc == 0 and "mismatches 0" in out, out[-2000:] + err[-1000:]


def test_value_codec_fuzz(emu_jobs):
    """tools/cell_fuzz.py on the emulated kernels: mutated texts of every value class (temporal shapes around chrono's grammar, json
    validity, numeric / float forms, array literals, bytea, uuid) through the decode kernels on three kernel paths, and the decoded
    arena through the Arrow columns, RowBinary and BigQuery rows — against the oracle and its hand-off restatements."""
    rc, out, err = _result(emu_jobs, "cell_fuzz")
    assert rc == 0 and "mismatching batches 0" in out and "MISMATCH" not in out, out[-2000:] + err[-1000:]


def test_results_do_not_depend_on_the_lane_order(emu_jobs):
    """Between two rendezvous the GPU runs the lanes of a workgroup in no particular order; the emulator's default is 0, 1, 2, ...,
    which hides races (round 3's bytea[] walker had one that only the MI355X showed). The table-copy and hand-off tests again with
    the lanes shuffled at every scheduling round. (The whole GPU suite passes that way too — 1418 tests, a nine-minute run that is
    not part of this suite: ETLG_SIMT_ORDER=shuffle with the recipe of DESIGN §6 'Kernel logic without a GPU'.)"""
    _passed(emu_jobs, "lane_order")
