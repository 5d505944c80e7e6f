"""TEST INFRASTRUCTURE — host model of etlg_batch_payload (include/etlg.h): the source payload metadata the reference's apply loop builds
per row message. The per-frame reference is the oracle fed ONE frame per call: it is stateful across calls, the call's payload_bytes is
the frame's kind and value bytes (StreamingPayloadMetadata::{insert,update,delete}, apply.rs:2459-2463 / :2503-2507 / :2547-2551 over
calculate_tuple_bytes, codec/event.rs:261-297 — recorded before should_apply_changes), and its n_events says whether the frame delivered
an event. Range sums (EventBatch::push's merge, apply.rs:656-658; source_payload_metadata.rs) and `le` buckets are plain Python here.
For table-copy rows the reference is the offsets (TableCopyPayloadMetadata, table_copy.rs:84)."""
import numpy as np

U64_MAX = (1 << 64) - 1
KINDS = ("insert", "update", "delete", "copy")
CONSUMERS = b"BRIUDTC"          # the frames that take the transaction's next ordinal (apply.rs:2291, 2339, 2377, 2457, 2501, 2545, 2587)


# ---------------------------------------------------------------- StreamingPayloadMetadata, restated

class Meta:
    """Option<u64> per operation; merge adds with saturation, None + x = x (source_payload_metadata.rs)."""

    def __init__(self, **kw):
        self.v = {k: kw.get(k) for k in KINDS}

    @classmethod
    def of(cls, kind, nbytes):
        return cls(**{KINDS[kind]: int(nbytes)})

    def merge(self, other):
        for k in KINDS:
            a, b = self.v[k], other.v[k]
            if b is not None:
                self.v[k] = b if a is None else min(U64_MAX, a + b)
        return self

    def processed(self):
        """record_processed's (label, bytes) pairs: the operations that are present."""
        return [(k, self.v[k]) for k in KINDS if self.v[k] is not None]

    def total(self):
        t = 0
        for _, b in self.processed():
            t = min(U64_MAX, t + b)
        return t

    def observations(self):
        """record_row_size: one observation per present operation."""
        return [float(b) for _, b in self.processed()]


# ---------------------------------------------------------------- the per-frame walk

def frame_offsets(buf):
    """Offsets of the CopyData frames of a stream without a sidecar: 'd' + Int32 length; stops in front of what is not a whole frame."""
    b, o, out = bytes(buf), 0, [0]
    while o + 5 <= len(b) and b[o:o + 1] == b"d":
        n = int.from_bytes(b[o + 1:o + 5], "big")
        if n < 4 or o + 1 + n > len(b):
            break
        o += 1 + n
        out.append(o)
    return np.array(out, dtype=np.uint32)


def frame_tag(buf, o0, o1):
    """The pgoutput tag of an XLogData frame, 0 for anything else."""
    return int(buf[o0 + 30]) if o1 - o0 > 30 and buf[o0] == ord("d") and buf[o0 + 5] == ord("w") else 0


class Walk:
    """One decode batch walked a frame per call on `orc` (an oracle primed like the decoder, carrying the stream's state).
    frames[f] = (kind or None, bytes, delivered) for every frame looked at: the consumed ones and, after an error, the failing one.
    n_frames = frames consumed; err = the oracle's error code of the failing frame (0: none)."""

    def __init__(self, orc, buf, offs):
        buf = np.frombuffer(bytes(buf), dtype=np.uint8) if not isinstance(buf, np.ndarray) else buf
        self.frames, self.err, self.n_frames = [], 0, 0
        for f in range(len(offs) - 1):
            o0, o1 = int(offs[f]), int(offs[f + 1])
            rb = orc.decode(buf[o0:o1], np.array([0, o1 - o0], dtype=np.uint32))
            hb = rb.host_batch()
            pay = [int(x) for x in hb.payload_bytes]
            tag = frame_tag(buf, o0, o1)
            kind = {ord("I"): 0, ord("U"): 1, ord("D"): 2}.get(tag)
            if rb.err_code:
                # the failing frame has recorded its metrics when the error came behind them: the oracle's view says so
                counted = kind is not None and self._counted(orc, rb, pay, kind)
                self.frames.append((kind if counted else None, pay[kind] if counted else 0, 0))
                self.err = rb.err_code
                rb.close()
                break
            assert sum(1 for x in pay if x) <= 1 and all(pay[k] == 0 for k in range(3) if k != kind), (f, pay, tag)
            self.frames.append((kind, pay[kind] if kind is not None else 0, int(hb.n_events)))
            assert hb.n_events <= 1
            self.n_frames += 1
            rb.close()

    @staticmethod
    def _counted(orc, rb, pay, kind):
        # the message is measured once it has parsed and passed the transaction-state check (apply.rs:2451-2463): every later error —
        # a missing schema, a cell that does not decode — finds its metrics recorded. The oracle's own sum must agree.
        from etl_amd import abi
        counted = rb.err_code not in (abi.E_WIRE, abi.E_TXN_STATE)
        assert counted or pay[kind] == 0, (rb.err_code, pay)
        return counted

    def received(self):
        by, rows = [0, 0, 0, 0], [0, 0, 0, 0]
        for kind, nbytes, _ in self.frames:
            if kind is not None:
                by[kind] += nbytes
                rows[kind] += 1
        return by, rows

    def sizes(self):
        """(kind, bytes) of every received row message, frame order."""
        return [(k, b) for k, b, _ in self.frames if k is not None]

    def event_frames(self):
        """Frame of every delivered event, event order."""
        return [f for f, (_, _, d) in enumerate(self.frames[:self.n_frames]) if d]

    def ev_bytes(self):
        return np.array([self.frames[f][1] for f in self.event_frames()], dtype=np.uint32)

    def ev_kinds(self):
        return [self.frames[f][0] for f in self.event_frames()]


# ---------------------------------------------------------------- ranges and buckets

def range_sums(ev_kinds, ev_bytes, cuts, copy=False):
    """np.uint64[n_cuts + 1, 2, 4]: bytes and rows per kind of the events [cuts[k - 1], cuts[k]), the last range up to the end."""
    n = len(ev_bytes)
    edges = [0] + [int(c) for c in cuts] + [n]
    out = np.zeros((len(edges) - 1, 2, 4), dtype=np.uint64)
    for k in range(len(edges) - 1):
        m = Meta()
        rows = [0, 0, 0, 0]
        for i in range(edges[k], edges[k + 1]):
            kind = 3 if copy else ev_kinds[i]
            if kind is not None:
                m.merge(Meta.of(kind, ev_bytes[i]))
                rows[kind] += 1
        for kind in range(4):
            out[k, 0, kind] = m.v[KINDS[kind]] or 0
            out[k, 1, kind] = rows[kind]
            assert (m.v[KINDS[kind]] is None) == (rows[kind] == 0)
    return out


def buckets(sizes, bounds):
    """np.uint64[4, len(bounds) + 1]: Prometheus `le` buckets, not cumulated — bounds[j - 1] < bytes <= bounds[j]; the last is the overflow."""
    out = np.zeros((4, len(bounds) + 1), dtype=np.uint64)
    for kind, nbytes in sizes:
        j = 0
        while j < len(bounds) and nbytes > bounds[j]:
            j += 1
        out[kind, j] += 1
    return out


# ---------------------------------------------------------------- the ordinal join

def join(buf, offs, n_frames, ev_kind, ev_ord, entry_ord):
    """Frame of every event by the rule of include/etlg.h: the (rank of the transaction's Begin + ev_tx_ordinal)-th ordinal-taking frame,
    the j-th 'B' event being the j-th Begin frame; in front of the first Begin the (ev_tx_ordinal - entry_ord)-th. None: no such frame,
    or one of another kind."""
    tags = [frame_tag(buf, int(offs[f]), int(offs[f + 1])) for f in range(n_frames)]
    r2f = [f for f, t in enumerate(tags) if t and bytes([t]) in CONSUMERS]
    brank = [r for r, f in enumerate(r2f) if tags[f] == ord("B")]
    out, begins = [], 0
    for kind, ordinal in zip(ev_kind, ev_ord):
        begins += int(kind) == ord("B")
        if begins:
            rank = brank[begins - 1] + int(ordinal) if begins <= len(brank) else -1
        else:
            rank = int(ordinal) - entry_ord
        f = r2f[rank] if 0 <= rank < len(r2f) else None
        out.append(f if f is not None and tags[f] == int(kind) else None)
    return out


def next_entry_ord(buf, offs, n_frames, entry_ord):
    """The ordinal the batch behind this one starts from."""
    o = entry_ord
    for f in range(n_frames):
        t = frame_tag(buf, int(offs[f]), int(offs[f + 1]))
        if t == ord("B"):
            o = 0
        if t and bytes([t]) in CONSUMERS:
            o += 1
    return o
