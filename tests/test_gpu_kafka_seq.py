"""GPU: the five Kafka kernels of csrc/ysb_kafka.hip on the generated corpus (tests/kafka_seqgen.py)
against the pure-Python model tests/kafka_model.py, exactly: a bad record in every round of the
walk and both kinds of fault in one round, a batch cut at chosen bytes, a `length` varint of every
width split at every byte across the walk's window edges at every residue of the first record
byte (all in one launch), the base kernel's scan and verdict past its first chunk of 256 batches,
the gather's stores next to shared 16-byte vectors and staging chunk edges between canaries, the
output capacity verdict, and the same faults and window shapes inside LZ4 frames.  The corpus,
malformed batches included, is the one tests/test_kafka_seq_logic.py passes through the sanitized
host build of the shared reader and pins by digest."""
import numpy as np
import pytest

import kafka_lz4_model as Z
import kafka_model as M
import kafka_seqgen as G
from test_gpu_parity import make_ctx
from ysb_amd import YsbError, kafka

pytestmark = pytest.mark.gpu

FILL = 0xA5
CANARY = 64
COUNTERS = ("records", "null_values", "keyed", "headers", "value_bytes")


class Device:
    """The device buffers of the synchronous calls, allocated once for the module.  The output
    pointer of a call is d_out + CANARY + out_shift; everything else of d_out is canary."""
    IN, OUT, RECS = 8 << 20, 5 << 20, 1 << 14

    def __init__(self, c):
        self.c = c
        self.d_in, self.d_out, self.d_off = c.device_alloc(self.IN), c.device_alloc(self.OUT), c.device_alloc(4 * self.RECS)
        assert self.d_in % 16 == 0 and self.d_out % 16 == 0
        self.fill_out = np.full(self.OUT, FILL, dtype=np.uint8)
        self.fill_off = np.full(4 * self.RECS, FILL, dtype=np.uint8)

    def close(self):
        for p in (self.d_in, self.d_out, self.d_off):
            self.c.device_free(p)

    def run(self, blob, idx, nval, out_shift=0, in_shift=0, out_cap=None, lz4=None):
        """One call over the pre-filled output and offsets allocations: (values, offsets).  Every
        byte of the output allocation outside the nval bytes and every offsets word behind
        n + 1 keeps the pre-fill; a refused call leaves both allocations as they were (and
        raises its YsbError)."""
        c = self.c
        blob = np.frombuffer(bytes(blob), dtype=np.uint8)
        nrec = int(idx["n_records"].sum()) if idx.size else 0
        lo = CANARY + out_shift
        assert in_shift + blob.size <= self.IN and lo + nval + CANARY <= self.OUT and nrec + 1 < self.RECS
        if blob.size:
            c.h2d(self.d_in + in_shift, blob)
        c.h2d(self.d_out, self.fill_out)
        c.h2d(self.d_off, self.fill_off)
        cap = nval if out_cap is None else out_cap
        refused = None
        try:
            if lz4 is None:
                got = c.kafka_unframe_device(self.d_in + in_shift, blob.size, idx, self.d_out + lo, cap, self.d_off, nrec + 1)
            else:
                got = c.kafka_unframe_lz4_device(self.d_in + in_shift, blob.size, idx, lz4[0], lz4[1], self.d_out + lo, cap,
                                                 self.d_off, nrec + 1)
        except YsbError as e:
            refused = e
        out = c.d2h(np.empty(self.OUT, dtype=np.uint8), self.d_out)
        off = c.d2h(np.empty(self.RECS, dtype=np.uint32), self.d_off)
        if refused is not None:
            assert (out == FILL).all(), "a refused call wrote to the output"
            assert (off == 0xA5A5A5A5).all(), "a refused call wrote offsets"
            raise refused
        assert got == (nrec, nval)
        assert (out[:lo] == FILL).all(), "bytes in front of the output were written"
        assert (out[lo + nval:] == FILL).all(), "bytes behind the output were written"
        assert (off[nrec + 1:] == 0xA5A5A5A5).all(), "offsets behind n + 1 were written"
        return out[lo:lo + nval], off[:nrec + 1]


@pytest.fixture(scope="module")
def ctx():
    with make_ctx(max_batch_bytes=8 << 20, timing=True) as c:
        yield c


@pytest.fixture(scope="module")
def dev(ctx):
    d = Device(ctx)
    yield d
    d.close()


def model_of(blob):
    return M.unframe(blob, M.index(blob, check_crc=True)[0])


def check_good(dev, blob, want, out_shift=0, lz4_blob=None):
    """A good call equals the model: values, offsets, the five counters, no verdict."""
    mout, moff, mct = want
    if lz4_blob is None:
        idx, info = kafka.index(blob, check_crc=True)
        assert info["consumed"] == len(blob)
        out, off = dev.run(blob, idx, len(mout), out_shift)
    else:
        idx, fr, bl, info = kafka.index_lz4(lz4_blob, check_crc=True)
        assert info["consumed"] == len(lz4_blob)
        out, off = dev.run(lz4_blob, idx, len(mout), out_shift, in_shift=1, lz4=(fr, bl))
    assert out.tobytes() == mout, "value bytes differ"
    assert off.tolist() == moff, "offsets differ"
    ki = dev.c.kafka_info()
    assert {k: ki[k] for k in COUNTERS} == mct
    assert ki["batches"] == idx.size and ki["verdict"]["first_bad"] is None and ki["verdict"]["bad_batches"] == 0


def check_bad(dev, blob, verdict, what="ysb_kafka_unframe_device", lz4=False):
    """A call with bad batches: code -5, the message names the batch and the record, the verdict
    is (bad_batches, first_bad, record, rule), nothing is written."""
    if lz4:
        idx, fr, bl, _ = kafka.index_lz4(blob, check_crc=True)
    else:
        idx, _ = kafka.index(blob, check_crc=True)
    with pytest.raises(YsbError) as e:
        dev.run(blob, idx, 4096, out_shift=3, in_shift=1 if lz4 else 0, lz4=(fr, bl) if lz4 else None)
    first = verdict[1]
    assert e.value.code == -5 and "%s: Kafka batch %d (baseOffset %d), record %d" % (
        what, first, idx[first]["base_offset"], verdict[2]) in str(e.value), str(e.value)
    v = dev.c.kafka_info()["verdict"]
    assert (v["bad_batches"], v["first_bad"], v["record"], v["rule"]) == verdict, (v, verdict)


# ---- 1. the walk's verdict in every round -------------------------------------------------------

def test_fault_at_record_k(dev):
    """Every fault case between a good batch in front and one behind, one call each: the verdict
    names batch 1 and the case's (record, rule) -- from a ballot over the bodies, from the chain,
    with both in one round, and with the batch's end on a round's boundary."""
    cases = G.fault_cases()
    assert len(cases) == 141
    for b in cases:
        check_bad(dev, G.with_neighbours(b), (1, 1) + b.expect)
    # the device is as it was: a good call right behind
    blob = G.blob_of(G.base_calls()[0].batches[:5])
    check_good(dev, blob, model_of(blob))


def test_cuts(dev):
    """One valid 130-record batch cut at the first and last byte of records 63, 64, 65 and 128,
    inside their varints, and at the walk's window edges."""
    for b in G.cut_cases():
        check_bad(dev, G.with_neighbours(b), (1, 1) + b.expect)


# ---- 2. the window ring ---------------------------------------------------------------------------

def test_windows_in_one_launch(dev):
    """All window batches in one call, each one wave of the same launch, each with its first
    record byte at its residue (the device buffer is 16-byte aligned); once more with the output
    shifted by 9."""
    placed = G.place(G.window_batches())
    blob = G.blob_of(placed)
    want = model_of(blob)
    assert want[2]["records"] == sum(b.count for b in placed) and len(placed) == 2 * 1616
    check_good(dev, blob, want)
    check_good(dev, blob, want, out_shift=9)


# ---- 3. the base kernel past its first chunk ------------------------------------------------------

def test_base_chunks(dev):
    """255, 256, 257, 513 and 600 batches whose counters differ in every chunk of 256; one bad
    batch at 0, 255, 256 and 599; {300, 10}: first_bad in an earlier chunk than another bad batch;
    {256, 257, 599}."""
    for call in G.base_calls():
        blob = G.blob_of(call.batches)
        if call.verdict is None:
            check_good(dev, blob, model_of(blob), out_shift=5)
        else:
            assert M.verdict_all(blob, M.index(blob)[0]) == call.verdict
            check_bad(dev, blob, call.verdict)


# ---- 4. the gather's edges ------------------------------------------------------------------------

def test_gather_edges(dev):
    """Every gather call at out_shift 0, 1, 15, 16 and 17, the call whose four runs write 5 bytes
    each into shared 16-byte vectors at all 16: between canaries (Device.run)."""
    for i, call in enumerate(G.gather_calls()):
        blob = G.blob_of(call.batches)
        want = model_of(blob)
        for shift in (range(16) if i == 0 else G.OUT_SHIFTS):
            check_good(dev, blob, want, out_shift=shift)
    # no records at all: line_off[0] alone is written
    idx = np.zeros(0, dtype=kafka.BATCH)
    out, off = dev.run(b"", idx, 0)
    assert out.size == 0 and off.tolist() == [0]
    # records without a value byte: the all-empty early return, every offset 0
    blob = M.pack([b"", None] * 150, 100)
    check_good(dev, blob, model_of(blob), out_shift=7)


def test_output_capacity(dev):
    """out_cap one byte short: YSB_ERR_CAPACITY with the byte count, nothing written; the exact
    capacity succeeds on the same context; out_cap 0 is refused the same way."""
    blob = M.pack([G.value(i, 10 + i % 50) for i in range(600)], 100)
    idx, _ = kafka.index(blob, check_crc=True)
    want = model_of(blob)
    nval = len(want[0])
    for cap in (nval - 1, 0):
        with pytest.raises(YsbError) as e:
            dev.run(blob, idx, nval, out_shift=3, out_cap=cap)
        assert e.value.code == -4 and "%d value bytes do not fit the output" % nval in str(e.value), str(e.value)
        assert dev.c.kafka_info()["verdict"]["bad_batches"] == 0
        check_good(dev, blob, want, out_shift=3)


# ---- 5. the same inside LZ4 frames ------------------------------------------------------------------

def framed(b, i, base_offset):
    """A batch's record bytes in a good frame, compressed or (every other one) all literals."""
    fr = Z.frame(b.raw) if i % 2 == 0 else Z.frame(b.raw, compress=Z.compress_literal, allow_stored=False)
    return Z.pack_batch(None, base_offset=base_offset, frame_bytes=fr, records_count=b.count)


def test_faults_inside_lz4_frames(dev):
    """The fault cases at records 64 and 129 and the two-fault cases, each inside a good frame
    (the automatic decoder choice): the uncompressed verdict.  The skip-then-straddle and the
    steps-from-next batches inside frames, each extent at its residue (1 and 15) in the inflated
    buffer: the plain unframing's result."""
    dev.c.lz4_set_decoder(0)
    cases = [b for b in G.fault_cases() if b.name.endswith((" at record 64", " at record 129"))] + list(G.two_fault_cases())
    assert len(cases) == 33
    front, back = Z.pack_batch([M.Record(b"ok")]), Z.pack_batch(G.BACK_RECORDS, base_offset=1000)
    for i, b in enumerate(cases):
        check_bad(dev, front + framed(b, i, 1) + back, (1, 1) + b.expect, "ysb_kafka_unframe_lz4_device", lz4=True)
    shapes = [b for b in G.window_batches() if b.mis in (1, 15) and ("skip, then" in b.name or "nine steps" in b.name)]
    assert len(shapes) == 6
    batches, at = [], 0
    for i, b in enumerate(shapes):      # the extents lie back to back from a 256-byte aligned start
        n = 16 + (b.mis - at) % 16
        batches += [G.valid_batch("extent filler %d" % i, [G.record_spanning(n, i)]), b]
        at += n
        assert at % 16 == b.mis
        at += len(b.raw)
    plain = G.blob_of(batches)
    wire, base = bytearray(), 0
    for i, b in enumerate(batches):
        wire += framed(b, i // 2, base)
        base += b.count
    check_good(dev, plain, model_of(plain), out_shift=3, lz4_blob=bytes(wire))
