"""The plan's sidecar pre-pass (k_plan_pre, etl_amd/csrc/plan.hip) at the shapes at which its layout can go wrong — workgroups of eight
waves, a wave takes 8 tiles, a group is 64 tiles, the last group to arrive scans 64 groups per trip: batches that end one frame
before, on, and one frame behind a tile seam at every count of tiles around a wave's share, a group, a trip and several trips; a chain
longer than many rotations of the prefix buffers with 24 batches in flight, a buffer that has to grow while batches are in flight, a
batch the decode kernel gives up, a batch of one frame; host input that arrives on the copy stream. Every batch against the oracle.

(The file's name is the experiment it was written for: the pre-pass AHEAD of its batch on a stream of its own, which did not ship —
tools/experiments/r07_plan_pre_ahead_stream.diff, profiles/r07_plan_pre_ahead.md. The reshaped pre-pass did, and these are its tests.)"""
import os

import numpy as np
import pytest

from etl_amd import abi, synth

pytestmark = pytest.mark.gpu

EMU = os.environ.get("ETLG_SIMT_RUN") == "1"
FLAGS = abi.F_INPUT_ON_DEVICE | abi.F_OUTPUT_ON_DEVICE | abi.F_NO_CONTROL | abi.F_ASYNC
PRE_BUFS = 4   # etlg_ctx::kPreBufs (host_state.h)


def _decoder(w):
    """A context with the plan as first attempt."""
    from etl_amd.decoder import Decoder
    saved = os.environ.get("ETLG_FUSED_KERNEL")
    os.environ["ETLG_FUSED_KERNEL"] = "3"
    try:
        d = Decoder(0)
    finally:
        os.environ.pop("ETLG_FUSED_KERNEL", None)
        if saved is not None:
            os.environ["ETLG_FUSED_KERNEL"] = saved
    w.register(d)
    return d


def _device(pieces):
    """Device copies of (bytes, offsets); on the emulator build device memory is host memory."""
    keep, items = [], []
    if not EMU:
        import torch
    for buf, offs in pieces:
        o32 = np.ascontiguousarray(offs.astype(np.uint32))
        if EMU:
            b = np.ascontiguousarray(buf)
            keep += [b, o32]
            items.append((b.ctypes.data, len(b), o32.ctypes.data, len(o32) - 1))
        else:
            tb = torch.from_numpy(np.ascontiguousarray(buf).copy()).cuda()
            to = torch.from_numpy(o32.view(np.int32).copy()).cuda()
            keep += [tb, to]
            items.append((tb.data_ptr(), tb.numel(), to.data_ptr(), len(o32) - 1))
    if not EMU:
        torch.cuda.synchronize()
    return keep, items


def _slices(buf, offs, counts):
    """Consecutive batches of exactly counts[i] frames off one framed stream (transactions span the cuts)."""
    out, a = [], 0
    o64 = offs.astype(np.int64)
    for n in counts:
        o = o64[a:a + n + 1]
        assert len(o) == n + 1, "the stream is shorter than the batches asked for"
        out.append((buf[int(o[0]):int(o[-1])].copy(), (o - o[0]).astype(np.uint32)))
        a += n
    return out


def _oracle_chain(w, pieces):
    from oracle import oracle
    o = oracle.Oracle()
    w.register(o)
    return o, [o.decode(buf, offs) for buf, offs in pieces]


def _chain(w, items, want, window=24):
    """The chain, `window` batches in flight, synced in issue order, every batch against the oracle's."""
    d = _decoder(w)
    inflight, done = [], 0

    def collect():
        nonlocal done
        b, rb = inflight[done], want[done]
        rc = b.sync()
        assert (rb.err_code != 0) == (rc != 0), f"batch {done}: oracle error {rb.err_code} vs rc {rc} ({b.error})"
        if rb.err_code:
            assert (b.error.code, b.error.frame_index) == (rb.err_code, rb.err_frame), f"batch {done}"
        diff = rb.host_batch().diff(b.host())   # the eight header columns, the fixed arena, the heap
        assert not diff, f"batch {done}: {diff[:6]}"
        b.close()
        done += 1
    for (p, n, po, nf) in items:
        if len(inflight) - done >= window:
            collect()
        inflight.append(d.decode_device(p, n, po, nf, FLAGS))
    while done < len(inflight):
        collect()
    paths = d.debug_paths()
    d.close()
    return paths


# tiles per batch: around the group of the pre-pass (64 tiles: one workgroup, eight waves of 8) and its multiples.
# (The emulator runs the seams of the first trip: a lane is a fiber there, and 380 k frames are minutes.)
SEAM_TILES = (1, 31, 32, 33, 63, 64, 65) if EMU else (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513)


@pytest.mark.parametrize("txn", ["seven_row_transactions", "one_transaction"])
def test_batches_that_end_at_every_group_seam(txn):
    """Batches of 64 t - 1, 64 t and 64 t + 1 frames. With 7-row transactions a Begin or a Commit sits on every seam of tiles, waves and
    groups and the open Begin's LSN crosses each of them; with one transaction over everything no batch but the first holds a mark,
    and every prefix is the carried state plus a sum. Header columns and arenas equal the oracle's, every batch produced by the plan."""
    counts = [64 * t + k for t in SEAM_TILES for k in (-1, 0, 1)]
    total = sum(counts)
    w = synth.Workload([synth.table_fixed()], 0xE7A0001, rows_per_txn=7 if txn == "seven_row_transactions" else total - 2)
    buf, offs = w.fill(total * 120 + (1 << 16))
    pieces = _slices(buf, offs, counts)
    if txn == "one_transaction":
        assert buf[int(offs[0]) + 30] == ord("B") and all(buf[int(o) + 30] == ord("I") for o in offs[1:total - 1:997])
    keep, items = _device(pieces)
    o, want = _oracle_chain(w, pieces)
    p = _chain(w, items, want)
    assert p["plan"] == len(pieces) and p["plan_redone"] == 0 and p["redone"] == 0, p
    del keep


def _pad_a_begin(buf, offs):
    """One zero byte behind the first Begin that is not the batch's first frame (the wire parser ignores bytes behind a message; the
    pre-pass prices the frame as a row, the decode kernel notices and gives the batch up)."""
    o = offs.astype(np.int64)
    for f in range(1, len(o) - 1):
        if o[f + 1] - o[f] == 51 and buf[o[f] + 30] == ord("B"):
            nb = np.concatenate([buf[:o[f + 1]], np.zeros(1, dtype=np.uint8), buf[o[f + 1]:]])
            # CopyData's length word (4 bytes behind the 'd') counts the byte too
            ln = int.from_bytes(bytes(nb[o[f] + 1:o[f] + 5]), "big") + 1
            nb[o[f] + 1:o[f] + 5] = np.frombuffer(ln.to_bytes(4, "big"), dtype=np.uint8)
            no = o.copy()
            no[f + 1:] += 1
            return nb, no.astype(np.uint32)
    raise AssertionError("no Begin inside the batch")


def test_long_chain_through_the_buffer_rotation_growth_and_a_give_up():
    """83 batches of 115 KiB - 2.5 MiB in varying order (cfg2's 1000-row transactions span every cut), 24 in flight: every prefix
    buffer is taken twenty times, by batches of 1 to 6 groups in no order, and the status tag goes through its cycle.
    In the middle one batch of 6 MiB (the buffers grow with batches in flight), one whose Begin is padded (the decode kernel gives
    the batch up: plan_redone; its successors start from the right state) and one of a single frame."""
    scale = 16 if EMU else 1   # (the emulator: the same chain with every batch a sixteenth of the size)
    n = 20 * PRE_BUFS + 3   # (twenty rotations of the buffers)
    rng = np.random.default_rng(0xE7A0002)
    kib = [int(x) for x in rng.choice([115, 120, 130, 250, 700, 1200, 2100, 2500], n)]
    kib[n // 2] = 6 * 1024
    w = synth.cfg2()
    avg = 113
    counts = [max(2, (k << 10) // scale // avg) for k in kib]
    counts[n // 2 + 7] = 1
    buf, offs = w.fill(sum(counts) * 120 + (1 << 20))
    pieces = _slices(buf, offs, counts)
    k_pad = n // 2 + 3
    pieces[k_pad] = _pad_a_begin(*pieces[k_pad])
    keep, items = _device(pieces)
    o, want = _oracle_chain(w, pieces)
    p = _chain(w, items, want)
    assert p["plan_redone"] >= 1 and p["plan"] >= n - 24 - 2, p   # (the give-up and what was in flight behind it may be decoded again)
    del keep


def test_pinned_host_input_waits_for_its_upload():
    """Three 256 KiB batches from pinned host buffers: bytes and sidecar travel on the copy stream, and the pre-pass reads them on the
    decode stream behind the upload's event (h2d_done)."""
    w = synth.cfg2()
    nfr = (256 << 10) // 113
    buf, offs = w.fill(3 * nfr * 120 + (1 << 16))
    pieces = _slices(buf, offs, [nfr, nfr, nfr])
    o, want = _oracle_chain(w, pieces)
    flags = abi.F_OUTPUT_ON_DEVICE | abi.F_NO_CONTROL | abi.F_ASYNC
    d = _decoder(w)
    ring = [(d.host_alloc(len(pb) + 64), d.host_alloc((len(po) + 1) * 4)) for pb, po in pieces]
    inflight = []
    for (pb, po), (hb, ho) in zip(pieces, ring):
        hb[:len(pb)] = pb
        ho.view(np.uint32)[:len(po)] = po
        inflight.append(d.decode_host_ptr(hb.ctypes.data, len(pb), ho.ctypes.data, len(po) - 1, flags))
    for k, (b, rb) in enumerate(zip(inflight, want)):
        assert b.sync() == 0 and rb.err_code == 0, (k, b.error)
        diff = rb.host_batch().diff(b.host())
        assert not diff, f"batch {k}: {diff[:6]}"
        b.close()
    p = d.debug_paths()
    assert d.debug_staged() == 3 and p["plan"] == 3 and p["plan_redone"] == 0, p
    for hb, ho in ring:
        d.host_free(hb); d.host_free(ho)
    d.close()
