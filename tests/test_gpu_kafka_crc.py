"""GPU: CRC-32C of Kafka record batches verified on the device (kafka_crc_kernel,
csrc/ysb_kafka.hip; the arithmetic: csrc/ysb_kafka_crc.h) -- the kernel alone
(ysb_kafka_crc_device) against tests/kafka_model.py batch by batch, over the range lengths
around the vector and window edges at all 16 byte addresses mod 16, one batch of 1 MiB + 3 and
more batches than the grid holds waves; rule 9 through ysb_kafka_unframe_device, ysb_submit_kafka
and ysb_submit_kafka_mapped with ysb_kafka_set_crc on; the mode off; compressed batches."""
import os

import numpy as np
import pytest

import golden_data as gd
import kafka_model as M
from test_gpu_kafka import SLOT, counts_and_stats, fixture_lines, record_spanning, unframe_device
from test_gpu_mapped import aligned
from test_gpu_parity import make_ctx
from ysb_amd import YsbError, kafka

pytestmark = pytest.mark.gpu

RULE_CRC = 9
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kafka")


@pytest.fixture(scope="module")
def ctx():
    with make_ctx(max_batch_bytes=SLOT, timing=True) as c:
        yield c


def model_crcs(blob, idx, crc=M.crc32c):
    """(computed, stored) of every indexed batch by the model."""
    got, want = [], []
    for b in idx:
        ro, n = int(b["records_off"]), int(b["records_bytes"])
        got.append(crc(blob[ro - 40:ro + n]))
        want.append(int.from_bytes(blob[ro - 44:ro - 40], "big"))
    return got, want


def crc_device_at(c, blob, idx, residue=0):
    """The kernel alone over blob placed `residue` bytes into a device allocation that ends with
    the blob's last byte's vector."""
    arr = np.frombuffer(bytes(blob), dtype=np.uint8)
    d = c.device_alloc(arr.size + residue)
    try:
        c.h2d(d + residue, arr)
        return c.kafka_crc_device(d + residue, arr.size, idx)
    finally:
        c.device_free(d)


# ---- 1. the kernel alone ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def edge_blob():
    """Batches of 0 records (a 40-byte range) and of 1 record, and batches whose range (40 + the
    records' bytes) is one byte short of, exactly and one byte over 64 bytes, one window and two
    windows: placed at every address mod 16 every end falls on, in front of and behind a vector
    boundary and a window's.  The model's CRCs once."""
    parts = [M.pack_batch([], base_offset=0), M.pack_batch([M.Record(b"x")], base_offset=1)]
    for i, total in enumerate(t + d for t in (64, 1024, 2048) for d in (-1, 0, 1)):
        parts.append(M.pack_batch([record_spanning(total - 40, i)], base_offset=10 + i, base_timestamp=i))
    blob = b"".join(parts)
    idx, info = kafka.index(blob, check_crc=True)
    assert info["consumed"] == len(blob) and idx.size == 11
    assert [int(b["records_bytes"]) + 40 for b in idx] == [40, 40 + int(idx[1]["records_bytes"]), 63, 64, 65, 1023, 1024, 1025,
                                                           2047, 2048, 2049]
    got, want = model_crcs(blob, idx)
    assert got == want
    return blob, idx, got


@pytest.mark.parametrize("residue", range(16))
def test_crc_device_at_every_address(ctx, edge_blob, residue):
    blob, idx, want = edge_blob
    got, stored = crc_device_at(ctx, blob, idx, residue)
    assert [int(v) for v in got] == want, "computed"
    assert [int(v) for v in stored] == want, "stored"
    info = ctx.kafka_crc_info()
    assert info["batches"] == idx.size and info["bad_batches"] == 0 and info["first_bad"] is None
    assert info["bytes"] == int(idx["records_bytes"].sum()) + 40 * idx.size and info["crc_ms"] > 0


@pytest.fixture(scope="module")
def crc_on_ctx():
    with make_ctx(max_batch_bytes=SLOT, timing=True) as c:
        c.kafka_set_crc(kafka.CRC_DEVICE)
        yield c


@pytest.fixture(scope="module")
def registered(crc_on_ctx):
    """One registered array for the module's in-place submits: whole pages of a mapping of its own
    (4 MiB: not carved out of the small-object heap), registered once and unregistered at the end."""
    raw = np.zeros((4 << 20) + 8192, dtype=np.uint8)
    a = (-raw.ctypes.data) % 4096
    buf = raw[a:a + (4 << 20)]
    crc_on_ctx.host_register(buf)
    yield buf
    crc_on_ctx.host_unregister(buf)


def mapped_at(c, buf, blob, idx, residue, slot):
    """blob read in place from the registered array at an address that is `residue` mod 16 (every
    submit is settled before the array is rewritten: sync waits for the slot's copy even when it
    raises the dropped batch's error)."""
    at = 4096 + 64 + residue
    assert (buf.ctypes.data + at) % 16 == residue and at + len(blob) <= buf.size
    buf[at:at + len(blob)] = np.frombuffer(bytes(blob), dtype=np.uint8)
    c.submit_kafka_mapped(buf, at, len(blob), idx, slot=slot)
    c.sync()


@pytest.mark.parametrize("residue", range(16))
def test_mapped_submit_at_every_address(crc_on_ctx, registered, edge_blob, residue):
    """The same batches (0 records, 1 record, ranges of 64, 1024 and 2048 bytes -1 / 0 / +1) read in
    place from registered memory at every address mod 16 with the mode on: all verify; then with one
    bit flipped in the last byte of one of them (which one turns with the residue): that batch is
    rule 9 and the computed and stored values are the model's."""
    c = crc_on_ctx
    blob, idx, want = edge_blob
    mapped_at(c, registered, blob, idx, residue, residue & 1)
    ci = c.kafka_crc_info()
    assert (ci["batches"], ci["bad_batches"], ci["first_bad"], ci["mode"]) == (idx.size, 0, None, 1)
    assert ci["bytes"] == int(idx["records_bytes"].sum()) + 40 * idx.size
    ki = c.kafka_info()
    assert ki["records"] == int(idx["n_records"].sum()) and ki["verdict"]["first_bad"] is None
    k = residue % idx.size
    bad = bytearray(blob)
    bad[int(idx[k]["records_off"]) + int(idx[k]["records_bytes"]) - 1] ^= 0x20
    got_m, stored_m = model_crcs(bytes(bad), idx[k:k + 1])
    assert stored_m[0] == want[k] != got_m[0]
    with pytest.raises(YsbError) as e:
        mapped_at(c, registered, bytes(bad), idx, residue, residue & 1)
    assert e.value.code == -5 and "stored %08x, computed %08x" % (stored_m[0], got_m[0]) in str(e.value), str(e.value)
    ci = c.kafka_crc_info(check=False)
    assert (ci["bad_batches"], ci["first_bad"], ci["stored"], ci["computed"]) == (1, k, stored_m[0], got_m[0])
    assert c.kafka_info(check=False)["verdict"] == dict(bad_batches=1, first_bad=k, record=0, rule=RULE_CRC)
    c.reset()


@pytest.mark.parametrize("residue", [1, 15])
def test_mapped_mebibyte_batch(crc_on_ctx, registered, residue):
    """One batch of 1 MiB + 3 read in place at an odd address: its CRC is the model's (a flipped
    copy names both values, which are compared)."""
    c = crc_on_ctx
    rec = record_spanning((1 << 20) + 3 - 40, 0)
    rec.value = (b"0123456789abcdef" * (len(rec.value) // 16 + 1))[:len(rec.value)]
    blob = M.pack_batch([M.Record(b"front")]) + M.pack_batch([rec], base_offset=1)
    idx, _ = kafka.index(blob)
    assert int(idx[1]["records_bytes"]) + 40 == (1 << 20) + 3
    mapped_at(c, registered, blob, idx, residue, 0)
    ci = c.kafka_crc_info()
    assert (ci["batches"], ci["bad_batches"]) == (2, 0) and ci["bytes"] == len(blob) - 2 * 21
    bad = bytearray(blob)
    bad[len(blob) // 2] ^= 0x01
    got_m, stored_m = model_crcs(bytes(bad), idx[1:2], M.crc32c_fast)
    with pytest.raises(YsbError):
        mapped_at(c, registered, bytes(bad), idx, residue, 1)
    ci = c.kafka_crc_info(check=False)
    assert (ci["first_bad"], ci["stored"], ci["computed"]) == (1, stored_m[0], got_m[0])
    c.reset()


def test_one_batch_of_a_mebibyte_and_three(ctx):
    """1024 windows and a remainder for one wave; the model's table loop is the reference here (the
    bitwise one takes several seconds over a mebibyte; test_kafka_crc_logic.py holds the two equal)."""
    rng = np.random.default_rng(11)
    rec = record_spanning((1 << 20) + 3 - 40, 0)
    rec.value = rng.integers(0, 256, len(rec.value), dtype=np.uint8).tobytes()
    blob = M.pack_batch([M.Record(b"front")]) + M.pack_batch([rec], base_offset=1)
    idx, _ = kafka.index(blob)
    assert int(idx[1]["records_bytes"]) + 40 == (1 << 20) + 3
    want, stored = model_crcs(blob, idx, M.crc32c_fast)
    assert want == stored
    for residue in (0, 5):
        got, st = crc_device_at(ctx, blob, idx, residue)
        assert [int(v) for v in got] == want and [int(v) for v in st] == want


def test_more_batches_than_the_grid_holds_waves(ctx):
    """Two turns of the kernel's loop and three batches more, every batch's CRC its own (the base
    timestamp is inside the range; baseOffset is not)."""
    waves = ctx.kafka_crc_info()["grid_waves"]
    assert 64 <= waves <= 1 << 16
    n = 2 * waves + 3
    blob = b"".join(M.pack_batch([], base_offset=i, base_timestamp=i * 7919) for i in range(n))
    idx, info = kafka.index(blob)
    assert idx.size == n
    want, stored = model_crcs(blob, idx, M.crc32c_fast)
    assert want == stored and len(set(want)) > n // 2
    got, st = crc_device_at(ctx, blob, idx, 3)
    assert (got == np.array(want, dtype=np.uint32)).all() and (st == got).all()
    assert ctx.kafka_crc_info()["batches"] == n


def test_arguments(ctx):
    blob = M.pack_batch([M.Record(b"abc")])
    idx, _ = kafka.index(blob)
    bad = idx.copy()
    bad["records_off"] = 43
    bad["records_bytes"] = 1
    with pytest.raises(YsbError) as e:
        crc_device_at(ctx, blob, bad)
    assert e.value.code == -1 and "44" in str(e.value)
    with pytest.raises(YsbError) as e:
        ctx.kafka_set_crc(2)
    assert e.value.code == -1
    assert ctx.kafka_crc_info()["mode"] == 0


# ---- 2. one-bit flips through the three paths ----------------------------------------------------

def flip(blob, at, bit=0x04):
    b = bytearray(blob)
    b[at] ^= bit
    return bytes(b)


@pytest.fixture(scope="module")
def fixture_batches():
    data, off, lines = fixture_lines("gen_s7")
    blob = M.pack(lines, 50, base_offset=500)
    idx, _ = kafka.index(blob, check_crc=True)
    assert idx.size >= 5
    return blob, idx


def spot(idx, k, where):
    start = int(idx[k]["records_off"]) - M.HEADER
    return start + where if where >= 0 else int(idx[k]["records_off"]) + int(idx[k]["records_bytes"]) + where


# the first byte of the range (`attributes`), the batch's last byte, the stored CRC itself
COVERED = {"attributes": 21, "last byte": -1, "stored crc": 17}
# baseOffset, batchLength's neighbour and magic's neighbour (partitionLeaderEpoch): not covered
UNCOVERED = {"baseOffset": 7, "batchLength's neighbour": 12, "magic's neighbour": 15}


def submit_unframe(c, blob, idx):
    """The unframing alone of a response with a bad batch: it raises, and nothing was written to the
    output or the offsets and nothing was counted (this call leaves no sticky error, so the
    counters are readable at once)."""
    arr = np.frombuffer(bytes(blob), dtype=np.uint8)
    nrec = int(idx["n_records"].sum())
    d_in, d_out, d_off = c.device_alloc(arr.size), c.device_alloc(arr.size), c.device_alloc(4 * (nrec + 1))
    try:
        c.h2d(d_in, arr)
        c.h2d(d_out, np.full(arr.size, 0xA5, dtype=np.uint8))
        c.h2d(d_off, np.full(4 * (nrec + 1), 0xA5, dtype=np.uint8))
        try:
            c.kafka_unframe_device(d_in, arr.size, idx, d_out, arr.size, d_off, nrec + 1)
        finally:
            assert (c.d2h(np.empty(arr.size, dtype=np.uint8), d_out) == 0xA5).all(), "the output was written"
            assert (c.d2h(np.empty(4 * (nrec + 1), dtype=np.uint8), d_off) == 0xA5).all(), "the offsets were written"
            st = c.stats()
            assert st["events"] == 0 and st["batches"] == 0, st
    finally:
        for p in (d_in, d_out, d_off):
            c.device_free(p)


def submit_slot(c, blob, idx):
    c.submit_kafka(blob, idx, slot=0)
    c.sync()


def submit_mapped(c, blob, idx):
    buf = aligned(len(blob) + 16)
    buf[5:5 + len(blob)] = np.frombuffer(blob, dtype=np.uint8)
    c.host_register(buf)
    try:
        c.submit_kafka_mapped(buf, 5, len(blob), idx, slot=1)
        c.sync()
    finally:
        try:
            c.host_unregister(buf)
        except YsbError:
            pass      # (the sticky error of the dropped batch)


@pytest.mark.parametrize("path", [submit_unframe, submit_slot, submit_mapped], ids=["unframe_device", "submit_kafka", "mapped"])
@pytest.mark.parametrize("name", sorted(COVERED))
def test_flip_is_rule_9(fixture_batches, path, name):
    blob, idx = fixture_batches
    rows, st = gd.expected("gen_s7")
    bad = flip(blob, spot(idx, 3, COVERED[name]))
    bidx, _ = kafka.index(bad)
    assert (bidx["records_off"] == idx["records_off"]).all()
    want = kafka.verdict_crc(bad, bidx)
    assert want == dict(bad_batches=1, first_bad=3, record=0, rule=RULE_CRC)
    got_m, stored_m = model_crcs(bad, bidx[3:4])
    with make_ctx(max_batch_bytes=SLOT) as c:
        c.kafka_set_crc(kafka.CRC_DEVICE)
        with pytest.raises(YsbError) as e:
            path(c, bad, bidx)
        msg = str(e.value)
        assert e.value.code == -5 and "Kafka batch 3 (baseOffset 650)" in msg, msg
        assert "stored %08x, computed %08x" % (stored_m[0], got_m[0]) in msg and "nothing of the call was counted" in msg, msg
        assert c.kafka_info(check=False)["verdict"] == want
        ci = c.kafka_crc_info(check=False)
        assert (ci["calls"], ci["mode"], ci["batches"], ci["bad_batches"], ci["first_bad"]) == (1, 1, idx.size, 1, 3)
        assert (ci["stored"], ci["computed"]) == (stored_m[0], got_m[0])
        if path is not submit_unframe:
            with pytest.raises(YsbError) as e2:          # sticky until reset
                c.submit_kafka(blob, idx, slot=0)
            assert e2.value.code == -5 and "Kafka batch 3" in str(e2.value)
        c.reset()
        assert c.stats()["events"] == 0 and c.kafka_crc_info()["mode"] == 1 and c.kafka_crc_info()["calls"] == 0
        c.submit_kafka(blob, idx, slot=1)                # the clean bytes, the mode still on
        on = counts_and_stats(c)
        assert c.kafka_crc_info()["bad_batches"] == 0 and c.kafka_crc_info()["calls"] == 1
    with make_ctx(max_batch_bytes=SLOT) as off:
        off.submit_kafka(blob, idx, slot=1)
        assert counts_and_stats(off) == on and on[0] == rows


@pytest.mark.parametrize("name", sorted(UNCOVERED))
def test_flip_outside_the_range_counts_exactly(fixture_batches, name):
    blob, idx = fixture_batches
    rows, st = gd.expected("gen_s7")
    bad = flip(blob, spot(idx, 3, UNCOVERED[name]), 0x01)
    bidx, _ = kafka.index(bad)
    with make_ctx(max_batch_bytes=SLOT) as c:
        c.kafka_set_crc(kafka.CRC_DEVICE)
        unframe_device(c, bad, bidx)
        submit_slot(c, bad, bidx)
        got = counts_and_stats(c)
        assert got[0] == rows and all(got[1][k] == v for k, v in st.items())
        submit_mapped(c, bad, bidx)
        ci = c.kafka_crc_info()
        assert ci["calls"] == 3 and ci["bad_batches"] == 0


def test_smallest_bad_batch_whichever_kind(ctx):
    """A bad record in batch 0 and a bad CRC in batch 3: the verdict is batch 0's record rule and
    two batches are bad; both faults in batch 0: rule 9."""
    data, off, lines = fixture_lines("gen_s7")
    name, rule, count, rec = M.malformed_corpus()[8]
    blob = M.pack_batch(None, base_offset=0, records_count=count, raw_records=rec) + M.pack(lines[:80], 20, base_offset=2)
    idx, _ = kafka.index(blob, check_crc=True)
    end = lambda k: int(idx[k]["records_off"]) + int(idx[k]["records_bytes"])
    bad = flip(blob, end(3) - 1)
    both = flip(bad, end(0) - 1)
    ctx.kafka_set_crc(1)
    try:
        for b in (bad, both):
            want = kafka.verdict_crc(b, idx)
            with pytest.raises(YsbError):
                unframe_device(ctx, b, idx, nval=len(b))
            assert ctx.kafka_info()["verdict"] == want and want["bad_batches"] == 2 and want["first_bad"] == 0
        assert want["rule"] == RULE_CRC and kafka.verdict_crc(bad, idx)["rule"] == M.RULE[rule]
    finally:
        ctx.kafka_set_crc(0)


def test_mode_off_lets_the_flipped_bytes_through(fixture_batches):
    """Existing behaviour: without ysb_kafka_set_crc a flipped value byte that keeps the framing
    whole is counted as it is, no CRC kernel runs, nothing is allocated for one."""
    blob, idx = fixture_batches
    at = spot(idx, 3, -3)                       # inside the last record's value
    bad = flip(blob, at, 0x01)
    assert kafka.verdict(bad, idx)["bad_batches"] == 0
    with make_ctx(max_batch_bytes=SLOT) as c:
        c.submit_kafka(bad, idx)
        c.sync()
        ki = c.kafka_info()
        assert ki["records"] == int(idx["n_records"].sum()) and ki["verdict"]["first_bad"] is None
        if hasattr(c, "kafka_crc_info"):
            assert c.kafka_crc_info()["calls"] == 0 and c.kafka_crc_info()["mode"] == 0


# ---- 3. compressed batches -------------------------------------------------------------------------

def test_compressed_batches(ctx):
    """gen_s7 as LZ4-compressed batches plus a codec-0 batch in one response: exact with the mode
    on; a flip in a compressed block is rule 9 (the CRC is over the wire bytes and comes first)."""
    raw, offs = gd.events("gen_s7")
    offs = np.asarray(offs, dtype=np.int64)
    rows, st = gd.expected("gen_s7")
    n = len(offs)
    z = kafka.pack(raw[:int(offs[n - 10])], offs[:n - 10], batch_bytes=16384, codec="lz4").tobytes()
    tail = kafka.pack(raw[int(offs[n - 10]):], offs[n - 10:] - offs[n - 10], base_offset=n - 10).tobytes()
    blob = z + tail
    idx, frames, blocks, info = kafka.index_lz4(blob, check_crc=True)
    assert info["compressed_batches"] == idx.size - 1 >= 2 and list(frames["codec"][-2:]) == [3, 0]
    with make_ctx(max_batch_bytes=SLOT) as c:
        c.kafka_set_crc(1)
        c.submit_kafka_lz4(blob, idx, frames, blocks)
        got = counts_and_stats(c)
        assert got[0] == rows and all(got[1][k] == v for k, v in st.items())
        ci = c.kafka_crc_info()
        assert ci["calls"] == 1 and ci["batches"] == idx.size and ci["bad_batches"] == 0
        assert ci["bytes"] == int(idx["records_bytes"].sum()) + 40 * idx.size
        bad = flip(blob, int(blocks[int(frames[1]["first_block"])]["offset"]) + 9, 0x80)
        want = kafka.verdict_crc_lz4(bad, idx, frames, blocks)
        assert want == dict(bad_batches=1, first_bad=1, record=0, rule=RULE_CRC)
        c.submit_kafka_lz4(bad, idx, frames, blocks, slot=1)
        with pytest.raises(YsbError) as e:
            c.sync()
        assert e.value.code == -5 and "Kafka batch 1 " in str(e.value) and "stored" in str(e.value)
        assert c.kafka_info(check=False)["verdict"] == want
    # the synchronous entry, the same two responses
    arr = np.frombuffer(bad, dtype=np.uint8)
    nrec = int(idx["n_records"].sum())
    ctx.kafka_set_crc(1)
    d_in, d_out, d_off = ctx.device_alloc(arr.size), ctx.device_alloc(len(raw) + 64), ctx.device_alloc(4 * (nrec + 1))
    try:
        ctx.h2d(d_in, arr)
        with pytest.raises(YsbError):
            ctx.kafka_unframe_lz4_device(d_in, arr.size, idx, frames, blocks, d_out, len(raw) + 64, d_off, nrec + 1)
        assert ctx.kafka_info()["verdict"] == want
        ctx.h2d(d_in, np.frombuffer(blob, dtype=np.uint8))
        assert ctx.kafka_unframe_lz4_device(d_in, arr.size, idx, frames, blocks, d_out, len(raw) + 64, d_off, nrec + 1) == (nrec, len(raw))
    finally:
        ctx.kafka_set_crc(0)
        for p in (d_in, d_out, d_off):
            ctx.device_free(p)


def test_committed_segment_verifies_clean(ctx):
    """tests/golden/kafka/segment.kafka (frames by liblz4, a codec-0 batch, a control batch): every
    data batch's CRC on the device, the control batch's on the host at index time."""
    with open(os.path.join(GOLDEN, "segment.kafka"), "rb") as f:
        blob = f.read()
    idx, frames, blocks, info = kafka.index_lz4(blob, check_control_crc=True)
    assert info["control_batches"] == 1 == info["crc_checked"]
    got, stored = crc_device_at(ctx, blob, idx, 7)
    want, wstored = model_crcs(blob, idx, M.crc32c_fast)
    assert [int(v) for v in got] == want == wstored == [int(v) for v in stored]
