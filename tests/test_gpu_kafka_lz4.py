"""GPU: LZ4-compressed Kafka record batches inflated and unframed on the device
(kafka_inflate_plan_kernel and kafka_codec_kernel in csrc/ysb_kafka.hip between the unchanged
measure, decode, walk, base and gather kernels) -- ysb_kafka_unframe_lz4_device against the host
model (csrc/ysb_kafka_lz4.h) and the pure-Python model (tests/kafka_lz4_model.py), byte for byte
on values, offsets, counters and verdict, with the automatic decoder choice (both decode kernels,
each on its size class) and each kernel forced on every shape; then
counts through the slots (ysb_submit_kafka_lz4, _mapped) against ysb_submit of the same lines.

The plan kernel scans 256 blocks per step (YSB's KAFKA_PLAN_STEP): the block counts below sit on
both sides of one and two steps.

Not covered: "a block that the measure pass accepts and only the decoder refuses".  Under the
library's rules there is none: the measure walk and the decoder call the one sequence reader
with the same bounds (lz4_read_seq tracks the output position in measure mode too, so an offset
in front of the block is refused by both), and the decode kernels' in-place checks never fire for
a block the reader accepts (tests/native/lz4_logic.cpp walks the corpus with them).  The
decoder's per-block flag and its merge into the verdict are therefore reachable only through a
fault of the decoder itself; the measured-0 path is what the malformed cases below exercise.
"""
import numpy as np
import pytest

import golden_data as gd
import kafka_lz4_model as Z
import kafka_model as K
import lz4_model as L
from test_gpu_kafka import counts_and_stats, fixture_lines, record_spanning, value
from test_gpu_kafka import unframe_device as unframe_plain_device
from test_gpu_mapped import aligned
from test_gpu_parity import make_ctx
from ysb_amd import YsbError, kafka

pytestmark = pytest.mark.gpu

SLOT = 1 << 20     # max_batch_bytes of the slot tests' contexts: 16 blocks by the capacity rule
STEP = 256         # blocks per step of the plan kernel's scan
DECODERS = (0, 1, 2)  # YSB_LZ4_DECODER_AUTO (both kernels, each on its size class), _NARROW, _WIDE


class Device:
    """The device buffers of the synchronous calls, allocated once for the module."""
    IN, OUT, RECS = 2 << 20, 4 << 20, 1 << 16

    def __init__(self, c):
        self.c = c
        self.d_in, self.d_out, self.d_off = c.device_alloc(self.IN), c.device_alloc(self.OUT), c.device_alloc(4 * self.RECS)

    def close(self):
        for p in (self.d_in, self.d_out, self.d_off):
            self.c.device_free(p)

    def run(self, blob, idx, fr, bl, nval, shift=3, fill=None):
        """One call; the wire bytes end at an odd address inside d_in, the output starts at one."""
        c = self.c
        blob = np.frombuffer(bytes(blob), dtype=np.uint8)
        nrec = int(idx["n_records"].sum()) if idx.size else 0
        assert blob.size + 16 <= self.IN and nval + shift + 1 <= self.OUT and nrec + 1 <= self.RECS
        if blob.size:
            c.h2d(self.d_in + 1, blob)
        if fill is not None:
            c.h2d(self.d_out, np.full(nval + shift + 1, fill, dtype=np.uint8))
        n, nb = c.kafka_unframe_lz4_device(self.d_in + 1, blob.size, idx, fr, bl, self.d_out + shift, nval, self.d_off, nrec + 1)
        assert (n, nb) == (nrec, nval)
        out = c.d2h(np.empty(nval + shift + 1, dtype=np.uint8), self.d_out)[shift:shift + nval]
        off = c.d2h(np.empty(nrec + 1, dtype=np.uint32), self.d_off)
        return out, off

    def written(self, n, fill):
        return bool((self.c.d2h(np.empty(n, dtype=np.uint8), self.d_out) != fill).any())


@pytest.fixture(scope="module")
def ctx():
    with make_ctx(max_batch_bytes=SLOT, timing=True) as c:
        yield c


@pytest.fixture(scope="module")
def dev(ctx):
    d = Device(ctx)
    yield d
    d.close()


def check_device(dev, blob, expect_records=None):
    """The library's index and host model equal the Python model's; the device equals both, with
    each decode kernel."""
    c = dev.c
    idx, fr, bl, info = kafka.index_lz4(blob, check_crc=True)
    mi, mf, mb, minfo = Z.index(blob, True)
    assert info["consumed"] == len(blob)
    assert [tuple(x) for x in fr] == mf and [(int(o), int(w)) for o, w, _ in bl] == mb
    for k, v in minfo.items():
        assert info[k] == v, k
    want, woff, wct = kafka.unframe_lz4_host(blob, idx, fr, bl)
    mout, moff, mct, mv = Z.unframe(blob, mi, mf, mb)
    assert mv is None and want.tobytes() == mout and list(woff) == moff
    assert {k: wct[k] for k in mct} == mct
    for decoder in DECODERS:
        c.lz4_set_decoder(decoder)
        out, off = dev.run(blob, idx, fr, bl, len(mout))
        assert out.tobytes() == mout, "value bytes differ (decoder %d)" % decoder
        assert list(off) == moff, "offsets differ (decoder %d)" % decoder
        ki, li = c.kafka_info(), c.kafka_lz4_info()
        for k in ("records", "null_values", "keyed", "headers", "value_bytes"):
            assert ki[k] == mct[k], k
        assert ki["batches"] == idx.size and ki["framed_bytes"] == len(blob) and ki["verdict"]["first_bad"] is None
        assert (li["blocks"], li["stored_blocks"], li["compressed_batches"], li["wire_bytes"], li["bad_blocks"]) == \
            (len(mb), minfo["stored_blocks"], minfo["compressed_batches"], len(blob), 0)
        assert li["inflated_bytes"] == wct["inflated_bytes"] and li["decoder"] == ((decoder or 3) if mb else 0)
    c.lz4_set_decoder(0)
    if expect_records is not None:
        assert mct["records"] == expect_records
    return ki, li


def check_verdict(dev, blob, shift=3):
    """A call with a bad batch: the device's verdict is the library model's and the Python
    model's, with each decode kernel, and nothing is written."""
    c = dev.c
    idx, fr, bl, _ = kafka.index_lz4(blob, check_crc=True)
    mi, mf, mb, _ = Z.index(blob, True)
    mv = Z.unframe(blob, mi, mf, mb)[3]
    assert mv is not None
    hv = kafka.verdict_lz4(blob, idx, fr, bl)
    assert (hv["bad_batches"], hv["first_bad"], hv["record"], hv["rule"]) == mv
    for decoder in DECODERS:
        c.lz4_set_decoder(decoder)
        with pytest.raises(YsbError) as e:
            dev.run(blob, idx, fr, bl, 4096, shift, fill=0xA5)
        what = "block" if mv[3] == Z.RULE_CODEC else "record"
        assert e.value.code == -5 and "Kafka batch %d (baseOffset %d), %s %d" % (
            mv[1], idx[mv[1]]["base_offset"], what, mv[2]) in str(e.value), str(e.value)
        v = c.kafka_info()["verdict"]
        assert (v["bad_batches"], v["first_bad"], v["record"], v["rule"]) == mv, (v, mv, decoder)
        assert not dev.written(4096 + shift + 1, 0xA5)
    c.lz4_set_decoder(0)
    return mv


# ---- 1. the plan's scan ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, STEP - 1, STEP, STEP + 1, 2 * STEP - 1, 2 * STEP, 2 * STEP + 1])
def test_scan_step_edges(dev, n):
    """n one-block batches (alternately compressed, literal-only and stored-by-codec-0), values of
    every length mod 16: the two running prefixes across one and two steps."""
    blob = bytearray()
    for i in range(n):
        recs = [K.Record(value(i, 5 + i % 23), key=b"k" if i % 2 else None)]
        if i % 3 == 2:
            blob += K.pack_batch(recs, base_offset=i)
        else:
            blob += Z.pack_batch(recs, base_offset=i, compress=Z.compress_literal if i % 3 else Z.compress_greedy,
                                 allow_stored=False)
    ki, li = check_device(dev, bytes(blob), n)
    assert li["blocks"] == n and li["plan_ms"] > 0 and li["measure_ms"] > 0 and li["decode_ms"] > 0


def test_batch_sum_crosses_a_step_edge(dev):
    """A Kafka batch of three blocks that starts at the last block of a step (block 255), between
    one-block batches: its extent is a difference of prefixes from two steps."""
    blob = bytearray()
    for i in range(STEP - 1):
        blob += Z.pack_batch([K.Record(value(i, 9 + i % 5))], base_offset=i)
    three = [K.Record(value(900 + i, 60)) for i in range(3)]
    rb = Z.records_bytes(three)
    blob += Z.pack_batch(three, base_offset=1000, block_bytes=(len(rb) + 2) // 3)
    for i in range(5):
        blob += Z.pack_batch([K.Record(value(i, 31))], base_offset=2000 + i)
    _, fr, _, _ = kafka.index_lz4(bytes(blob))
    assert tuple(fr[STEP - 1]) == (STEP - 1, 3, 3)
    check_device(dev, bytes(blob), STEP - 1 + 3 + 5)


# ---- 2. block sizes --------------------------------------------------------------------------------

def test_block_sizes(dev):
    """A block of exactly 1 raw byte (the records' last byte in a block of its own) and blocks of
    exactly 65536; a frame of stored blocks only, holding random values; an empty frame with zero
    records; all optional frame flags."""
    recs = [K.Record(value(i, 40 + i)) for i in range(6)]
    rb = Z.records_bytes(recs)
    one = Z.pack_batch(recs, block_bytes=len(rb) - 1, allow_stored=False)
    big = [K.Record(L.random_bytes(30000, 7 + i)[:65536 * 2 // 5 - 9]) for i in range(5)]
    full = Z.pack_batch(big, base_offset=10, compress=Z.compress_literal)      # random bytes: stored, 64 KiB blocks
    idx, fr, bl, info = kafka.index_lz4(one + full)
    assert bytes(one[int(bl[1]["offset"]):][:2]) == bytes([0x10, rb[-1]]) and int(bl[1]["comp_bytes"]) == 2
    assert info["stored_blocks"] >= 3 and int(bl[2]["comp_bytes"]) == (65536 | L.STORED)
    empty = Z.pack_batch([], base_offset=20)
    flags = Z.pack_batch(recs, base_offset=30, flags=True)
    check_device(dev, one + full + empty + flags, 6 + 5 + 0 + 6)
    check_device(dev, empty, 0)


def test_records_without_blocks_is_rule_7(dev):
    """recordsCount > 0 over an empty frame: rule 7, as the model says (record 0)."""
    blob = Z.pack_batch([K.Record(b"a")]) + Z.pack_batch(None, base_offset=1, frame_bytes=Z.frame(b""), records_count=2)
    assert check_verdict(dev, blob) == (1, 1, 0, K.RULE["count"])


# ---- 3. records across seams ----------------------------------------------------------------------

def test_records_straddle_block_seams(dev):
    """Inside one batch of 64 KiB blocks: a record's length varint starting at the last byte of
    block 0 (the header straddles the seam) and a value that lies across the second seam."""
    first = record_spanning(65535, 1)
    second = K.Record(value(2, 70000), key=b"kk")
    third = K.Record(b"third")
    for compress in (Z.compress_greedy, Z.compress_literal):      # (literal-only: longer than raw, so stored)
        blob = Z.pack_batch([first, second, third], compress=compress)
        idx, fr, bl, _ = kafka.index_lz4(blob)
        assert fr[0]["n_blocks"] == 3
        check_device(dev, blob, 3)


def test_extents_at_every_residue_and_the_buffer_edges(dev):
    """Batches whose inflated extents start at every residue modulo 16 (the walk loads whole
    16-byte vectors around an extent); the first and last batch lie at the inflated buffer's
    edges and the wire bytes end at the last byte given."""
    blob, starts, at = bytearray(), set(), 0
    for i in range(48):       # (records of i + 10 bytes: the starts run through the triangular numbers)
        recs = [K.Record(value(i, 3 + i))]
        starts.add(at % 16)
        at += len(Z.records_bytes(recs))
        blob += Z.pack_batch(recs, base_offset=i, compress=Z.compress_literal if i % 2 else Z.compress_greedy,
                             allow_stored=False)
    assert starts == set(range(16))
    check_device(dev, bytes(blob), 48)


# ---- 4. mixed calls ---------------------------------------------------------------------------------

def test_mixed_call_equals_the_uncompressed_unframing(dev):
    """Compressed, uncompressed (as stored blocks, one above 64 KiB) and control batches together:
    the result equals ysb_kafka_unframe_device on the same records packed uncompressed."""
    groups = [[K.Record(value(10 * g + i, (17 * g + 90 * i) % 700), key=b"k" * (g % 3)) for i in range(1 + g * 7)]
              for g in range(6)]
    groups[3] = [K.Record(value(i, 9000)) for i in range(9)]     # 81 KB of records: two stored blocks as codec 0
    control = K.pack_batch([K.Record(b"\0\0\0\0", key=b"\0\0\0\1")], base_offset=500, attributes=0x20)
    mixed, plain = bytearray(), bytearray()
    for g, recs in enumerate(groups):
        plain += K.pack_batch(recs, base_offset=100 * g)
        mixed += K.pack_batch(recs, base_offset=100 * g) if g % 2 else Z.pack_batch(recs, base_offset=100 * g)
        if g in (1, 4):
            mixed += control
            plain += control
    idx, fr, bl, info = kafka.index_lz4(bytes(mixed))
    assert info["control_batches"] == 2 and info["compressed_batches"] == 3 and fr[3]["n_blocks"] == 2
    ki, _ = check_device(dev, bytes(mixed))
    assert ki["control_skipped"] == 2
    pidx, _ = kafka.index(bytes(plain))
    pout, poff, pki = unframe_plain_device(dev.c, bytes(plain), pidx)
    out, off = dev.run(bytes(mixed), idx, fr, bl, pout.size)
    assert out.tobytes() == pout.tobytes() and list(off) == list(poff)
    assert {k: ki[k] for k in ("records", "null_values", "keyed", "headers", "value_bytes", "control_skipped")} == \
        {k: pki[k] for k in ("records", "null_values", "keyed", "headers", "value_bytes", "control_skipped")}


# ---- 5. malformed input -----------------------------------------------------------------------------

def bad_block_call(comp, j, k, n_batches=4):
    """comp as block j of batch k's frame of three blocks; good batches around it."""
    blob = bytearray()
    for b in range(n_batches):
        recs = [K.Record(value(b, 50)) for _ in range(3)]
        if b != k:
            blob += Z.pack_batch(recs, base_offset=10 * b)
            continue
        rb = Z.records_bytes(recs)
        parts = [(Z.compress_literal(rb[a:a + 60]), False) for a in range(0, 180, 60)][:3]
        parts[j] = (bytes(comp), False)
        blob += Z.pack_batch(None, base_offset=10 * b, frame_bytes=Z.frame_of_blocks(parts), records_count=3)
    return bytes(blob)


def test_malformed_blocks_equal_the_model(dev):
    """Every case of lz4_model.malformed_blocks() (the corpus the sanitized native LZ4 program has
    walked; a frame cannot hold a block of no bytes or of more than 64 KiB) as block j of batch k.  A frame records no raw
    size, so a case is bad exactly when the measure walk refuses it: then rule 8 with the block
    index, nothing written; a cut that still measures (it decodes to other bytes) leaves the
    verdict to the record walk -- the models say which."""
    rule8 = other = 0
    for i, (name, comp, _raw) in enumerate(L.malformed_blocks()):
        if not comp or len(comp) > Z.BLOCK_MAX:
            continue
        j, k = i % 3, (i // 3) % 4
        mv = check_verdict(dev, bad_block_call(comp, j, k), shift=i % 5)
        try:
            L.measure_block(comp)
            other += 1
            assert mv[1] == k and mv[3] != Z.RULE_CODEC, name
        except L.Bad:
            rule8 += 1
            assert mv == (1, k, j, Z.RULE_CODEC), (name, mv)
    assert rule8 > 100 and other > 10


def test_bad_blocks_count_per_block_and_per_batch(dev):
    """Two bad blocks in one batch (the smallest is named) and a bad block in another batch:
    bad_batches 2, bad_blocks 3."""
    bad = bytes([0x40]) + L._lits(4, 7) + bytes([5, 0, 0x00])      # offset before the block's start
    recs = [K.Record(value(1, 50))]
    two = Z.pack_batch(None, base_offset=5, records_count=1, frame_bytes=Z.frame_of_blocks(
        [(Z.compress_literal(b"abc"), False), (bad, False), (bad, False)]))
    one = Z.pack_batch(None, base_offset=9, records_count=1, frame_bytes=Z.frame_of_blocks([(bad, False)]))
    blob = Z.pack_batch(recs) + two + Z.pack_batch(recs, base_offset=7) + one
    assert check_verdict(dev, blob) == (2, 1, 1, Z.RULE_CODEC)
    assert dev.c.kafka_lz4_info()["bad_blocks"] == 3


def test_record_corpus_inside_good_frames(dev):
    """The malformed record corpus carried inside good frames: the verdicts for rules 1-7 are the
    uncompressed verdicts."""
    front, back = Z.pack_batch([K.Record(b"ok")]), Z.pack_batch([K.Record(b"after")], base_offset=9)
    for name, rule, count, rec in K.malformed_corpus():
        plain = K.pack_batch([K.Record(b"ok")]) + K.pack_batch(None, base_offset=1, records_count=count, raw_records=rec) + \
            K.pack_batch([K.Record(b"after")], base_offset=9)
        want = K.verdict(plain, K.index(plain)[0])
        blob = front + Z.pack_batch(None, base_offset=1, frame_bytes=Z.frame(rec), records_count=count) + back
        assert check_verdict(dev, blob) == (1,) + want, name


@pytest.mark.parametrize("record_first", [True, False])
def test_both_kinds_of_fault_in_one_call(dev, record_first):
    """A bad record in batch 2 and a bad block in batch 5, and the reverse: the verdict is the
    smaller batch's, whichever kind it is; bad_batches counts both."""
    name, rule, count, rec = K.malformed_corpus()[8]
    bad_rec = Z.pack_batch(None, base_offset=100, frame_bytes=Z.frame(rec), records_count=count)
    bad_blk = Z.pack_batch(None, base_offset=200, records_count=1, frame_bytes=Z.frame_of_blocks(
        [(Z.compress_literal(b"xy"), False), (bytes([0x40]) + L._lits(4, 7) + bytes([0, 0, 0]), False)]))
    good = [Z.pack_batch([K.Record(value(i, 40))], base_offset=i) for i in range(6)]
    at2, at5 = (bad_rec, bad_blk) if record_first else (bad_blk, bad_rec)
    blob = b"".join(good[:2]) + at2 + b"".join(good[2:4]) + at5 + good[4]
    mv = check_verdict(dev, blob)
    assert mv[0] == 2 and mv[1] == 2 and (mv[3] == Z.RULE_CODEC) == (not record_first)
    if not record_first:
        assert mv[2] == 1


# ---- 6. through the slots -----------------------------------------------------------------------------

def lz4_runs(blob, idx, fr, bl, max_blocks):
    """Runs of whole batches by the capacity rule: (b0, b1, batches, frames, blocks) rebased."""
    runs, x = [], 0
    while x < idx.size:
        y, nblk = x, 0
        while y < idx.size and nblk + int(fr[y]["n_blocks"]) <= max_blocks:
            nblk += int(fr[y]["n_blocks"])
            y += 1
        assert y > x
        b0 = int(idx[x]["records_off"]) - K.HEADER
        b1 = int(idx[y - 1]["records_off"]) + int(idx[y - 1]["records_bytes"])
        si, sf = idx[x:y].copy(), fr[x:y].copy()
        f0 = int(sf["first_block"][0])
        sb = bl[f0:f0 + nblk].copy()
        si["records_off"] -= b0
        si["first_record"] -= si["first_record"][0]
        sf["first_block"] -= f0
        sb["offset"] -= b0
        runs.append((b0, b1, si, sf, sb, int(idx[x]["first_record"]), int(si["n_records"].sum())))
        x = y
    return runs


def test_slot_counts_equal_ysb_submit():
    """gen_s7 through submit_kafka_lz4 and submit_kafka_lz4_mapped (odd byte addresses), two slots
    alternately, runs cut by the capacity rule: the counts and stats of ysb_submit on the same
    lines, and gen_s7's expected rows."""
    data, off, lines = fixture_lines("gen_s7")
    blob = kafka.pack(data, off, batch_bytes=16384, codec="lz4").tobytes()
    mi, mf, mb, _ = Z.index(blob, True)
    assert Z.unframe(blob, mi, mf, mb)[0] == data           # the model reads what the library packed
    idx, fr, bl, info = kafka.index_lz4(blob, check_crc=True)
    assert info["compressed_batches"] == idx.size > 4
    runs = lz4_runs(blob, idx, fr, bl, SLOT // 65536)
    assert len(runs) >= 2
    ends = np.append(off[1:], len(data)).astype(np.int64)
    with make_ctx(max_batch_bytes=SLOT) as ref:
        for i, (_, _, _, _, _, first, n) in enumerate(runs):
            a0, a1 = int(off[first]), int(ends[first + n - 1])
            ref.submit(data[a0:a1], off[first:first + n] - a0, slot=i % 2)
        want = counts_and_stats(ref)
    rows, st = gd.expected("gen_s7")
    assert want[0] == rows
    with make_ctx(max_batch_bytes=SLOT) as a:
        for i, (b0, b1, si, sf, sb, _, _) in enumerate(runs):
            a.submit_kafka_lz4(blob[b0:b1], si, sf, sb, slot=i % 2)
        assert counts_and_stats(a) == want
        li = a.kafka_lz4_info()
        assert li["calls"] == len(runs) and li["bad_blocks"] == 0 and li["inflated_buffer_bytes"] == 2 * (SLOT + 64)
        assert a.kafka_info()["records"] == runs[-1][6]
    buf = aligned(len(blob) + 64 * len(runs))
    places, pos = [], 0
    for i, (b0, b1, *_rest) in enumerate(runs):
        pos += (2 * i + 1 - pos) % 16
        buf[pos:pos + b1 - b0] = np.frombuffer(blob[b0:b1], dtype=np.uint8)
        places.append(pos)
        pos += b1 - b0
    assert all(p % 2 == 1 for p in places)
    with make_ctx(max_batch_bytes=SLOT) as m:
        m.host_register(buf)
        for i, (b0, b1, si, sf, sb, _, _) in enumerate(runs):
            m.submit_kafka_lz4_mapped(buf, places[i], b1 - b0, si, sf, sb, slot=i % 2)
        got = counts_and_stats(m)
        m.host_unregister(buf)
    assert got == want


def test_capacity_rule_at_the_call():
    """n_blocks x 65536 above max_batch_bytes: YSB_ERR_CAPACITY at the call, whatever the blocks
    hold; the next smaller run is accepted."""
    vals = [b'{"x":%d}' % i for i in range(17)]
    blob = Z.pack(vals, 1)
    idx, fr, bl, _ = kafka.index_lz4(blob)
    assert bl.size == 17 == SLOT // 65536 + 1
    with make_ctx(max_batch_bytes=SLOT) as c:
        with pytest.raises(YsbError) as e:
            c.submit_kafka_lz4(blob, idx, fr, bl)
        assert e.value.code == -4 and "17 blocks" in str(e.value)
        cut = int(idx[16]["records_off"]) - K.HEADER
        c.submit_kafka_lz4(blob[:cut], idx[:16], fr[:16], bl[:16])
        c.sync()
        assert c.kafka_info()["records"] == 16 and c.kafka_lz4_info()["blocks"] == 16


def test_bad_slot_batch_is_sticky_until_reset():
    """A bad block in a slot batch: nothing of it is counted, YSB_ERR_FORMAT names the Kafka batch
    and the block, sticky until ysb_reset; a good batch counts exactly afterwards."""
    data, off, lines = fixture_lines("gen_s7")
    good = kafka.pack(data, off, batch_bytes=200000, codec="lz4").tobytes()
    gidx, gfr, gbl, _ = kafka.index_lz4(good)
    assert gbl.size <= SLOT // 65536
    bad = Z.pack(lines[:100], 50) + Z.pack_batch(None, base_offset=100, records_count=1, frame_bytes=Z.frame_of_blocks(
        [(Z.compress_literal(b"abc"), False), (bytes([0x40]) + L._lits(4, 7) + bytes([0, 0, 0]), False)]))
    bidx, bfr, bbl, _ = kafka.index_lz4(bad, check_crc=True)
    rows, st = gd.expected("gen_s7")
    with make_ctx(max_batch_bytes=SLOT) as c:
        c.submit_kafka_lz4(bad, bidx, bfr, bbl, slot=0)
        with pytest.raises(YsbError) as e:
            c.sync()
        assert e.value.code == -5 and "Kafka batch 2 (baseOffset 100), block 1" in str(e.value), str(e.value)
        with pytest.raises(YsbError) as e2:
            c.submit_kafka_lz4(good, gidx, gfr, gbl, slot=1)
        assert e2.value.code == -5 and "Kafka batch 2" in str(e2.value)
        v = c.kafka_info(check=False)["verdict"]
        assert (v["bad_batches"], v["first_bad"], v["record"], v["rule"]) == (1, 2, 1, Z.RULE_CODEC)
        assert c.kafka_lz4_info(check=False)["bad_blocks"] == 1
        c.reset()
        assert c.stats()["events"] == 0
        c.submit_kafka_lz4(good, gidx, gfr, gbl, slot=1)
        c.sync()
        assert c.drain_buckets() == rows and all(c.stats()[k] == x for k, x in st.items())


def test_uncompressed_submits_allocate_no_inflated_buffer():
    data, off, lines = fixture_lines("gen_s7")
    blob = K.pack(lines, 150)
    idx, _ = kafka.index(blob)
    with make_ctx(max_batch_bytes=SLOT) as c:
        c.submit_kafka(blob, idx)
        c.sync()
        li = c.kafka_lz4_info()
        assert li["inflated_buffer_bytes"] == 0 and li["calls"] == 0
        idx2, fr2, bl2, _ = kafka.index_lz4(blob)
        c.submit_kafka_lz4(blob, idx2, fr2, bl2, slot=1)     # uncompressed batches as stored blocks
        c.sync()
        li = c.kafka_lz4_info()
        assert li["inflated_buffer_bytes"] == SLOT + 64 and li["stored_blocks"] == li["blocks"] == bl2.size
        assert c.stats()["events"] == 2 * len(lines)
