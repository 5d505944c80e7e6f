"""The prologue the classify-based synchronous entry points share (host.cpp: classify_begin, upload_input, batch_too_large):
etlg_frame_tags, etlg_shard_plan and etlg_control_stream give the same answer for host input as for device input, the answer of the
host models in etl_amd/shard.py, on the three batch shapes at which the prologue takes another path — no frame (nothing is launched),
one frame, and one transaction of kBlock + 1 frames (two classify blocks) with a Relation frame in it; and all four entry points that
take a byte length, etlg_scan_boundaries included, refuse a length beyond the 4 GiB limit before they touch the buffer."""
import ctypes as C
import os

import numpy as np
import pytest

from etl_amd import abi, shard
from tests import pgwire as W
from tests.test_gpu_async import DevBufs

pytestmark = pytest.mark.gpu
K_BLOCK = 256   # frames per workgroup of k_classify (dev_types.h: kBlock)


def _batches():
    one = W.Stream().add(W.begin(0x2000))
    s = W.Stream().add(W.begin(0x9000)).add(W.relation(16384, "public", "t", "d", [(1, "id", 23, -1), (0, "v", 25, -1)]))
    for k in range(K_BLOCK - 2):
        s.add(W.insert(16384, [str(k), "v%d" % k]))
    s.add(W.commit(0x9000, 0x9008))
    assert len(s.offsets) - 1 == K_BLOCK + 1
    out = {"empty": (np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint32))}
    for name, st in (("one_frame", one), ("block_plus_one", s)):
        out[name] = (np.frombuffer(st.bytes(), dtype=np.uint8).copy(), np.array(st.offsets, dtype=np.uint32))
    return out


BATCHES = _batches()


@pytest.fixture(scope="module")
def dec():
    from etl_amd.decoder import Decoder
    d = Decoder(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def dev():
    names = sorted(BATCHES)
    bufs = DevBufs([BATCHES[n] for n in names])
    return {n: bufs.items[i] for i, n in enumerate(names)}, bufs


def _tags_on_device(d, ptr, nbytes, optr, nf):
    if os.environ.get("ETLG_SIMT_RUN") == "1":   # the emulator's device memory is host memory
        out = np.zeros(nf, dtype=np.uint8)
        d.frame_tags_device(ptr, nbytes, optr, nf, out.ctypes.data)
        return out
    import torch
    out = torch.zeros(max(nf, 1), dtype=torch.uint8, device="cuda")
    d.frame_tags_device(ptr, nbytes, optr, nf, out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()[:nf]


@pytest.mark.parametrize("name", sorted(BATCHES))
def test_frame_tags_host_input_device_input_and_model_agree(dec, dev, name):
    buf, offs = BATCHES[name]
    want = shard.frame_tags(buf, offs)
    assert np.array_equal(dec.frame_tags(buf, offs), want)
    assert np.array_equal(_tags_on_device(dec, *dev[0][name]), want)
    if name == "block_plus_one":
        assert bytes(want[:3]) == b"BRI" and want[-1] == ord("C")


@pytest.mark.parametrize("n_shards", [2, 3])
@pytest.mark.parametrize("name", sorted(BATCHES))
def test_shard_plan_host_input_device_input_and_model_agree(dec, dev, name, n_shards):
    buf, offs = BATCHES[name]
    want = shard.plan_shards(buf, offs, n_shards)
    assert dec.shard_plan(buf, offs, n_shards) == want
    assert dec.shard_plan_device(*dev[0][name], n_shards) == want


@pytest.mark.parametrize("name", sorted(BATCHES))
def test_control_stream_host_input_device_input_and_model_agree(dec, dev, name):
    buf, offs = BATCHES[name]
    want_b, want_o = shard.control_stream(buf, offs)
    tags = shard.frame_tags(buf, offs)
    got = [dec.control_stream(buf.ctypes.data, len(buf), offs.ctypes.data, len(offs) - 1, on_device=False),
           dec.control_stream(*dev[0][name], on_device=True)]
    for got_b, got_o, last in got:
        assert bytes(got_b) == bytes(want_b) and list(got_o) == list(want_o)
        assert last == (int(tags[-1]) if len(tags) else 0)
    if name == "block_plus_one":
        assert len(want_o) - 1 == 3   # Begin, Relation, Commit — the Commit lies in the second classify block


def test_a_length_beyond_4_gib_is_refused_by_every_entry_point(dec):
    one = np.zeros(1, dtype=np.uint8)
    offs = np.array([0, 1], dtype=np.uint32)
    out = np.zeros(16, dtype=np.uint64)
    too_long = 0xFFFFFFFF   # (the limit leaves room for the 16 bytes a reader may touch past the input)
    nb, nf, last, n = C.c_size_t(), C.c_size_t(), C.c_uint32(), C.c_size_t()
    L, h = dec.L, dec.h
    calls = {
        "etlg_frame_tags": lambda: L.etlg_frame_tags(h, one.ctypes.data, too_long, offs.ctypes.data, 1, 0, out.ctypes.data),
        "etlg_shard_plan": lambda: L.etlg_shard_plan(h, C.c_void_p(one.ctypes.data), too_long, C.c_void_p(offs.ctypes.data), 1, 2, 0, out.ctypes.data),
        "etlg_control_stream": lambda: L.etlg_control_stream(h, C.c_void_p(one.ctypes.data), too_long, C.c_void_p(offs.ctypes.data), 1, 0, out.ctypes.data, 8,
                                                             out.ctypes.data + 64, 8, C.byref(nb), C.byref(nf), C.byref(last)),
        "etlg_scan_boundaries": lambda: L.etlg_scan_boundaries(h, one.ctypes.data, too_long, 0, out.ctypes.data, 16, C.byref(n)),
    }
    for name, call in calls.items():
        assert call() == abi.InvalidArgument, name
        assert "batch too large" in dec.last_error().description, name
    assert np.array_equal(dec.frame_tags(*BATCHES["one_frame"]), [ord("B")])   # the context goes on working
