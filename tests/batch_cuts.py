"""TEST INFRASTRUCTURE — host model of etlg_batch_cuts / etlg_cuts_locate (include/etlg.h): where the reference's apply loop cuts the event
stream into write_events batches. The rule restates three lines: EventBatch::push adds event.size_hint() to size_hint_bytes
(crates/etl/src/replication/apply.rs:656-657), the loop flushes after a message once size_hint_bytes >= the batch budget (:1932-1935), and
the flush starts the next batch at zero. The reference's own tests state no cut position as a number (its batching tests run a pipeline
with max_bytes: 1 and count rows), so there is no vector to transcribe into tests/golden/: what the GPU file checks is the device against
this restatement, and tests/test_batch_cuts_model.py checks this restatement against a second formulation."""
import numpy as np

INCOMPLETE = np.uint64(1 << 63)
MASK = (1 << 63) - 1


def cuts(hints, budget, carry_in=0, first=0, end=None):
    """The sequential rule over hints[first:end] (np.uint64, bit 63 = INCOMPLETE) -> (cuts, info): cuts the exclusive ends of the closed
    batches, info = {n_cuts, stop_event, carry_out, total}. The walk stops in front of the first INCOMPLETE event."""
    end = len(hints) if end is None else end
    s, total, out, stop = int(carry_in), 0, [], end
    for i, h in enumerate(np.asarray(hints[first:end], dtype=np.uint64).tolist(), first):
        if h >> 63:
            stop = i
            break
        s += h
        total += h
        if s >= budget:
            out.append(i + 1)
            s = 0
    return out, {"n_cuts": len(out), "stop_event": stop, "carry_out": s, "total": total}


def locate(row_event, cut_list):
    """Rows in front of every cut: the number of entries of the ascending row_event below it."""
    return np.searchsorted(np.asarray(row_event, dtype=np.uint64), np.asarray(cut_list, dtype=np.uint64), "left").astype(np.uint64)


def hints_of(hb):
    """Event::size_hint of every event of a host batch (oracle/size_hint.py), np.uint64 with bit 63 on the events the host must finish."""
    from oracle import size_hint as SH
    return np.array([SH.event_hint(e, hb.slots, SH.MODEL) for e in hb.materialize()], dtype=np.uint64)


def size_model():
    from etl_amd import abi
    from oracle import size_hint as SH
    m = abi.SizeModel()
    for k, v in SH.MODEL.items():
        setattr(m, k, v)
    return m
