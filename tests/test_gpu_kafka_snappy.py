"""GPU: snappy-compressed Kafka record batches inflated and unframed on the device
(snappy_preamble_kernel and snappy_decode_kernel in csrc/ysb_snappy.hip, beside the LZ4 kernels in
the compressed chain of csrc/ysb_kafka.hip) -- ysb_kafka_unframe_lz4_device over hand-built blocks
against the host model (csrc/ysb_snappy.h) and the pure-Python model (tests/snappy_model.py), byte
for byte on values, offsets and verdict; then one mixed call of codecs 0, 2, 2 and 3 through the
slots (ysb_submit_kafka_lz4, _mapped) against gen_s7's expected counts.

A hand-built block is one Kafka record: its header the front of the first literal, its value
whatever the elements produce, its last byte the record's header count.  The input shift is the
block's address modulo 16 (the reader's register window starts at the dword in front of it, 256
bytes at a time), the output shift its place in the context's inflated buffer modulo 16, set by an
uncompressed batch in front of it.
"""
import numpy as np
import pytest

import golden_data as gd
import kafka_lz4_model as Z
import kafka_model as K
import snappy_model as S
from test_gpu_kafka import counts_and_stats, fixture_lines
from test_gpu_mapped import aligned
from test_gpu_parity import make_ctx
from ysb_amd import YsbError, kafka

pytestmark = pytest.mark.gpu

SLOT = 2 << 20
SHIFTS = (0, 1, 15)
WINDOW = 256       # the reader's register window (Lz4GlobalIn)
CODECS = ("lz4", "snappy")


def filler(n, seed):
    return bytes((seed * 31 + j * 7 + j // 11) % 251 for j in range(n))


def record_block(elements, seed=1, pre_pad=0):
    """A block of one record from elements ("lit", n[, length bytes]) and ("c1" | "c2" | "c4",
    length, offset): (block, raw bytes, value).  The first element is a literal that holds the
    record's header; a last literal of the header count's 0 byte is appended."""
    total = sum(e[1] for e in elements) + 1
    assert elements[0][0] == "lit" and elements[0][1] >= 12
    # (no minimal record takes 65 or 8194 bytes: there its `length` gets a non-minimal byte)
    for vlen, pad in [(v, p) for p in (0, 1) for v in range(total - 15, total - 5)]:
        rb = Z.records_bytes([K.Record(bytes(vlen), length_pad=pad)])
        if len(rb) == total:
            break
    else:
        raise AssertionError("no record of %d bytes" % total)
    hdr = rb[:total - vlen - 1]
    stream = hdr + filler(total, seed)
    out, at = bytearray(S.preamble(total, pre_pad)), 0
    for e in elements:
        if e[0] == "lit":
            out += S.literal(stream[at:at + e[1]], e[2] if len(e) > 2 else None)
            at += e[1]
        else:
            out += {"c1": S.copy1, "c2": S.copy2, "c4": S.copy4}[e[0]](e[1], e[2])
    out += S.literal(b"\0")
    raw = S.decode_block(bytes(out))
    assert len(raw) == total and raw[:len(hdr)] == hdr
    return bytes(out), raw, raw[len(hdr):-1]


def call_of(blocks, out_shift, xerial=True, lead_base=16, n_records=None, tail=True):
    """An uncompressed batch whose records take lead_base + out_shift bytes, then one codec-2 batch
    whose section holds `blocks` (a record each unless n_records says otherwise: xerial chunks, or one raw block), then
    an uncompressed batch (tail False: none, so that the last snappy block's last byte is the
    call's last): (blob, batches, frames, block entries) with hand-made entries -- the index would
    refuse some of the blocks the device must call bad."""
    for vlen in range(1, 64):
        lead = [K.Record(filler(vlen, 3))]
        if len(Z.records_bytes(lead)) == lead_base + out_shift:
            break
    else:
        raise AssertionError("no lead record")
    a = K.pack_batch(lead, base_offset=0)
    section = S.xerial_of_chunks(blocks) if xerial else blocks[0]
    assert xerial or len(blocks) == 1
    n_records = len(blocks) if n_records is None else n_records
    b = K.pack_batch(None, base_offset=1, attributes=2, records_count=n_records, raw_records=section)
    c = K.pack_batch([K.Record(b"tail")], base_offset=1 + n_records)
    parts = ((a, 1, 0), (b, n_records, 2)) + (((c, 1, 0),) if tail else ())
    blob = b"".join(p for p, _, _ in parts)
    idx = np.zeros(len(parts), dtype=kafka.BATCH)
    fr = np.zeros(len(parts), dtype=kafka.FRAME)
    bl = np.zeros(len(parts) - 1 + len(blocks), dtype=kafka.BLOCK)
    pos, first, blk = 0, 0, 0
    for k, (part, n, codec) in enumerate(parts):
        idx[k] = (pos + K.HEADER, len(part) - K.HEADER, n, first, first, 0, 0)
        if codec == 0:
            fr[k] = (blk, 1, 0)
            bl[blk] = (pos + K.HEADER, (len(part) - K.HEADER) | 0x80000000, 0)
            blk += 1
        else:
            fr[k] = (blk, len(blocks), 2)
            at = pos + K.HEADER + (S.XERIAL_HEADER if xerial else 0)
            for z in blocks:
                at += 4 if xerial else 0
                bl[blk] = (at, len(z) | S.SNAPPY_BLOCK, 0)
                blk += 1
                at += len(z)
        pos += len(part)
        first += n
    return blob, idx, fr, bl, lead[0].value


class Device:
    """The device buffers of the synchronous calls, allocated once for the module."""
    IN, OUT, RECS = 1 << 20, 1 << 20, 4096

    def __init__(self, c):
        self.c = c
        self.d_in, self.d_out, self.d_off = c.device_alloc(self.IN), c.device_alloc(self.OUT), c.device_alloc(4 * self.RECS)

    def close(self):
        for p in (self.d_in, self.d_out, self.d_off):
            self.c.device_free(p)

    def run(self, blob, idx, fr, bl, nval, place, fill=None):
        c = self.c
        blob = np.frombuffer(bytes(blob), dtype=np.uint8)
        nrec = int(idx["n_records"].sum())
        assert place + blob.size <= self.IN and nval + 4 <= self.OUT and nrec + 1 <= self.RECS
        c.h2d(self.d_in + place, blob)
        if fill is not None:
            c.h2d(self.d_out, np.full(nval + 4, fill, dtype=np.uint8))
        n, nb = c.kafka_unframe_lz4_device(self.d_in + place, blob.size, idx, fr, bl, self.d_out + 3, nval, self.d_off, nrec + 1)
        assert (n, nb) == (nrec, nval)
        return c.d2h(np.empty(nval + 4, dtype=np.uint8), self.d_out)[3:3 + nval], c.d2h(np.empty(nrec + 1, dtype=np.uint32), self.d_off)

    def written(self, n, fill):
        return bool((self.c.d2h(np.empty(n, dtype=np.uint8), self.d_out) != fill).any())

    def place_for(self, blob, block_at, in_shift, at_end=False):
        """Where in d_in the blob goes so that its byte block_at lies at in_shift modulo 16 (d_in is
        256-byte aligned); at_end: the blob's last byte is the allocation's last."""
        if at_end:
            return self.IN - len(blob)
        return 256 + (in_shift - block_at) % 16


@pytest.fixture(scope="module")
def ctx():
    with make_ctx(max_batch_bytes=SLOT, timing=True) as c:
        c.kafka_set_codecs(CODECS)
        yield c


@pytest.fixture(scope="module")
def dev(ctx):
    d = Device(ctx)
    assert d.d_in % 256 == 0
    yield d
    d.close()


def check_good(dev, blocks, values, in_shift=0, out_shift=0, xerial=True, at_end=False):
    """The call of call_of(blocks), a record per value: the host model and the device give the
    values, byte for byte.  at_end: the snappy batch is the call's last and its last block's last
    byte the device allocation's last byte -- a read past comp_bytes would leave the allocation."""
    blob, idx, fr, bl, lead = call_of(blocks, out_shift, xerial, n_records=len(values), tail=not at_end)
    tails = [] if at_end else [b"tail"]
    want = lead + b"".join(values) + b"".join(tails)
    woff = list(np.cumsum([0] + [len(v) for v in [lead] + list(values) + tails]))
    if at_end:
        assert int(bl[-1]["offset"]) + (int(bl[-1]["comp_bytes"]) & S.LEN_MASK) == len(blob) and int(bl[-1]["comp_bytes"]) & S.SNAPPY_BLOCK
    hout, hoff, hct = kafka.unframe_lz4_host(blob, idx, fr, bl)
    assert hout.tobytes() == want and list(hoff) == woff
    place = dev.place_for(blob, int(bl[1]["offset"]), in_shift, at_end)
    out, off = dev.run(blob, idx, fr, bl, len(want), place)
    assert out.tobytes() == want, "value bytes differ (in %d, out %d)" % (in_shift, out_shift)
    assert list(off) == woff
    li = dev.c.kafka_lz4_info()
    assert (li["blocks"], li["snappy_blocks"], li["stored_blocks"], li["bad_blocks"]) == (bl.size, len(blocks), 1 if at_end else 2, 0)
    assert li["inflated_bytes"] == hct["inflated_bytes"] and li["preamble_ms"] > 0 and li["decode_ms"] > 0
    return li


def check_bad(dev, blocks, j, in_shift=0, out_shift=0, xerial=True):
    """Block j of the call is bad: rule 8 with the smallest bad block, by the model, the host model
    and the device; nothing is written."""
    blob, idx, fr, bl, _ = call_of(blocks, out_shift, xerial)
    for i, z in enumerate(blocks):
        try:
            S.decode_block(z)
            assert i != j
        except S.Bad:
            assert i >= j
    hv = kafka.verdict_lz4(blob, idx, fr, bl)
    assert (hv["bad_batches"], hv["first_bad"], hv["record"], hv["rule"]) == (1, 1, j, 8)
    place = dev.place_for(blob, int(bl[1 + j]["offset"]), in_shift)
    with pytest.raises(YsbError) as e:
        dev.run(blob, idx, fr, bl, 4096, place, fill=0xA5)
    assert e.value.code == -5 and "Kafka batch 1 (baseOffset 1), block %d" % j in str(e.value), str(e.value)
    v = dev.c.kafka_info()["verdict"]
    assert (v["bad_batches"], v["first_bad"], v["record"], v["rule"]) == (1, 1, j, 8)
    assert not dev.written(4100, 0xA5)


# ---- 1. raw sizes ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("in_shift,out_shift", [(0, 0), (1, 15), (15, 1)])
def test_raw_sizes(dev, in_shift, out_shift):
    """Blocks of 63, 64, 65, 32768 and 65536 raw bytes, and a block of exactly 1 raw byte (a record's
    last byte in a chunk of its own), as literals and copies of a run."""
    blocks, values = [], []
    for total in (63, 64, 65, 32768, 65536):
        el = [("lit", 20)]
        left = total - 21
        while left > 0:
            n = min(left, 64 if len(el) % 2 else 257)
            el.append(("c2", n, 1 + len(el) % 9) if len(el) % 2 else ("lit", n))
            left -= n
        z, raw, v = record_block(el, seed=total)
        assert len(raw) == total
        blocks.append(z)
        values.append(v)
    check_good(dev, blocks, values, in_shift, out_shift)
    # a record cut in front of its last byte: chunks of total - 1 and of 1 raw byte
    z, raw, v = record_block([("lit", 40), ("c1", 11, 7), ("lit", 61)], seed=5)
    two = [S.preamble(len(raw) - 1) + S.literal(raw[:-1]), S.preamble(1) + S.literal(raw[-1:])]
    check_good(dev, two, [v], in_shift, out_shift)


# ---- 2. literal lengths -------------------------------------------------------------------------------

@pytest.mark.parametrize("in_shift,out_shift", [(0, 0), (1, 1), (15, 15)])
def test_literal_lengths(dev, in_shift, out_shift):
    """Literals of 1, 60, 61 (one length byte), 257 (two) bytes and one with a 4-byte non-minimal
    length, and a non-minimal preamble; then with the last snappy block's last byte the device
    allocation's last byte, in both framings, the block starting at several addresses modulo 4."""
    z, raw, v = record_block([("lit", 12), ("lit", 1), ("lit", 60), ("lit", 61), ("lit", 257), ("lit", 33, 4), ("lit", 70, 3),
                              ("lit", 5, 1)], seed=in_shift, pre_pad=2)
    assert bytes([60 << 2, 60]) in z and bytes([61 << 2, 0, 1]) in z and bytes([63 << 2, 32, 0, 0, 0]) in z
    check_good(dev, [z], [v], in_shift, out_shift)
    check_good(dev, [z], [v], in_shift, out_shift, xerial=False)
    for extra in range(4):      # a second block whose length, so its start at the allocation's end, differs modulo 4
        z2, _, v2 = record_block([("lit", 13 + extra), ("c2", 9, 5), ("lit", 61)], seed=7)
        if (len(z2) - len(z)) % 4 == 1 + in_shift % 3:
            break
    else:
        raise AssertionError("no second block whose length differs as wanted modulo 4")
    starts = set()
    for blocks, values, xerial in (([z], [v], True), ([z], [v], False), ([z, z2], [v, v2], True), ([z2], [v2], False),
                                   ([z2, z], [v2, v], True)):
        check_good(dev, blocks, values, in_shift, out_shift, xerial=xerial, at_end=True)
        starts.add((Device.IN - len(blocks[-1])) % 4)
    assert len(starts) >= 2


# ---- 3. copy forms --------------------------------------------------------------------------------------

@pytest.mark.parametrize("in_shift,out_shift", [(0, 15), (1, 0), (15, 1)])
def test_copy_forms(dev, in_shift, out_shift):
    """copy-1 of 4 and 11 bytes at offsets 1 and 2047; copy-2 of 1 and 64 bytes at offsets 1, 3, 63,
    64, 65 and 65535; copy-4 with a small offset; a copy whose source is the literal just written;
    an offset equal to the output position."""
    el = [("lit", 2047)]
    for ln in (4, 11):
        for off in (1, 2047):
            el += [("c1", ln, off), ("lit", 3)]
    for ln in (1, 64):
        for off in (1, 3, 63, 64, 65):
            el += [("c2", ln, off), ("lit", 2)]
    el += [("c4", 64, 5), ("c4", 1, 1), ("lit", 7), ("c2", 7, 7), ("c4", 30, 2100)]
    z, raw, v = record_block(el, seed=9)
    # an offset equal to the output position, far into a block
    zb, rawb, vb = record_block([("lit", 60000), ("c2", 1, 60000), ("lit", 400)], seed=4)
    assert rawb[60000] == rawb[0]
    # offset 65535: a record across two chunks, the second of 65536 raw bytes whose last byte -- the
    # record's header count, 0 -- is a copy of its first
    vlen = 100 + 65535
    rb = Z.records_bytes([K.Record(bytes(vlen))])
    head = rb[:len(rb) - vlen - 1] + filler(100, 1)
    body = b"\0" + filler(65534, 2)
    za = S.preamble(len(head)) + S.literal(head)
    zc = S.preamble(65536) + S.literal(body) + S.copy2(1, 65535)
    assert S.decode_block(zc) == body + b"\0"
    check_good(dev, [z, zb, za, zc], [v, vb, filler(100, 1) + body], in_shift, out_shift)


def test_offset_one_past_the_output_is_bad(dev):
    good = S.preamble(13) + S.literal(b"abcdefgh") + S.copy2(4, 8) + S.literal(b"\0")
    assert S.decode_block(good) == b"abcdefghabcd\0"
    ok, _, _ = record_block([("lit", 30)])
    bad = S.preamble(13) + S.literal(b"abcdefgh") + S.copy2(4, 9) + S.literal(b"\0")
    check_bad(dev, [ok, bad, ok], 1)


# ---- 4. the reader's window edges -----------------------------------------------------------------------

@pytest.mark.parametrize("in_shift", SHIFTS)
def test_tags_at_the_window_edge(dev, in_shift):
    """Each element form with its tag as the last byte of the reader's 256-byte input window and its
    operand bytes in the next one, at the first and at the second window edge."""
    mis = in_shift & 3
    forms = [("lit", 70, 1), ("lit", 300, 2), ("lit", 20, 4), ("c1", 9, 200), ("c2", 40, 17), ("c4", 33, 5)]
    blocks, values = [], []
    for edge in (1, 2):
        for f in forms:
            # preamble (2 bytes) + a literal header (2 bytes: 61..256 bytes, or 3) + its bytes, then the tag
            first = edge * WINDOW - 1 - mis - 2 - (2 if edge == 1 else 3)
            z, raw, v = record_block([("lit", first), f, ("lit", 9)], seed=edge)
            tag_at = 2 + (2 if edge == 1 else 3) + first
            assert (tag_at + mis) % WINDOW == WINDOW - 1 and len(S.preamble(len(raw))) == 2
            assert z[tag_at] & 3 == {"lit": 0, "c1": 1, "c2": 2, "c4": 3}[f[0]]
            blocks.append(z)
            values.append(v)
    # every block of the call lies at the same address modulo 4: one call per block
    for z, v in zip(blocks, values):
        check_good(dev, [z], [v], in_shift, 0)


# ---- 5. bad blocks ------------------------------------------------------------------------------------------

def test_bad_blocks_store_nothing_and_name_the_smallest(dev):
    """Every malformed block of the model's corpus (offset 0, a copy at output position 0, cut
    elements, output over and under the preamble's size, preambles of 0, 65537 and 6 bytes, ...) as
    chunk j between good chunks, and twice in one call: rule 8 with the smallest bad block."""
    ok, _, _ = record_block([("lit", 30), ("c2", 20, 3)])
    for i, (name, bad, _rule) in enumerate(S.malformed_blocks()):
        j = i % 3
        blocks = [ok] * j + [bad] + [ok] + ([bad] if i % 2 else [])
        check_bad(dev, blocks, j, in_shift=SHIFTS[i % 3], out_shift=SHIFTS[(i + 1) % 3])
    assert dev.c.kafka_lz4_info()["bad_blocks"] >= 1
    name, bad, _ = S.malformed_blocks()[0]
    check_bad(dev, [bad], 0, xerial=False)


def test_a_block_past_its_preambles_size_on_a_large_block(dev):
    """Output over and under the preamble's size at 64 KiB: the last copy one byte long or short."""
    z, raw, v = record_block([("lit", 65000), ("c2", 64, 100), ("lit", 400)], seed=2)
    over = S.preamble(len(raw) - 1) + z[len(S.preamble(len(raw))):]
    under = S.preamble(len(raw) + 1) + z[len(S.preamble(len(raw))):]
    check_good(dev, [z], [v])
    check_bad(dev, [z, over], 1)
    check_bad(dev, [under, z], 0)


def test_a_batch_past_the_inflated_buffer_is_bad(dev):
    """The plan kernel's own bound (a slot batch's capacity is checked on the host, but registered
    bytes may change afterwards): with the limit set inside the snappy batch's second block, that
    batch is rule 8 with block 1, the batch behind it is bad too, and nothing is written; with the
    limit at the call's last inflated byte the call is good."""
    z, raw, v = record_block([("lit", 40), ("c2", 30, 7)], seed=3)
    blocks = [z, z, z]
    blob, idx, fr, bl, lead = call_of(blocks, 0)
    before = 16 + len(raw)                                      # the lead batch's 16 bytes and block 0
    total = 16 + 3 * len(raw) + len(Z.records_bytes([K.Record(b"tail")]))
    c = dev.c
    place = dev.place_for(blob, int(bl[1]["offset"]), 0)
    try:
        c.kafka_test_inflated_cap(before + len(raw) - 1)
        with pytest.raises(YsbError) as e:
            dev.run(blob, idx, fr, bl, 4096, place, fill=0xA5)
        assert e.value.code == -5 and "Kafka batch 1 (baseOffset 1), block 1" in str(e.value), str(e.value)
        vd = c.kafka_info()["verdict"]
        assert (vd["bad_batches"], vd["first_bad"], vd["record"], vd["rule"]) == (2, 1, 1, 8)
        assert not dev.written(4100, 0xA5)
        c.kafka_test_inflated_cap(total)
        check_good(dev, blocks, [v, v, v])
        c.kafka_test_inflated_cap(total - 1)                      # the last batch alone is over
        with pytest.raises(YsbError) as e:
            dev.run(blob, idx, fr, bl, 4096, place, fill=0xA5)
        vd = c.kafka_info()["verdict"]
        assert (vd["bad_batches"], vd["first_bad"], vd["record"], vd["rule"]) == (1, 2, 0, 8)
        c.reset()                                                 # a reset lifts the limit, as 0 does
        check_good(dev, blocks, [v, v, v])
        c.kafka_test_inflated_cap(before)
    finally:
        c.kafka_test_inflated_cap(0)
    check_good(dev, blocks, [v, v, v])


# ---- 6. through the slots: one mixed call ---------------------------------------------------------------------

def mixed_blob(corrupt=False):
    """gen_s7 as batches of codec 0, 2 (xerial, chunks of 100 bytes: records straddle them), 2 (one
    raw block per batch) and 3, a quarter of the lines each."""
    data, off, lines = fixture_lines("gen_s7")
    n = len(lines)
    cuts = [0, n // 4, n // 2, 3 * n // 4, n]
    ends = np.append(off[1:], len(data)).astype(np.int64)
    kinds = [dict(), dict(codec="snappy", snappy_chunk=100), dict(codec="snappy", snappy_framing="raw"), dict(codec="lz4")]
    blob = bytearray()
    for q, kw in enumerate(kinds):
        a, b = cuts[q], cuts[q + 1]
        a0, a1 = int(off[a]), int(ends[b - 1])
        blob += kafka.pack(data[a0:a1], off[a:b] - a0, batch_bytes=16384, base_offset=a, **kw).tobytes()
    return bytes(blob)


def test_mixed_call_counts_exactly():
    blob = mixed_blob()
    idx, fr, bl, info = kafka.index_lz4(blob, check_crc=True, accept_snappy=True)
    codecs = [int(c) for c in fr["codec"]]
    assert sorted(set(codecs)) == [0, 2, 3] and info["consumed"] == len(blob)
    mi, mf, mb, _ = S.index(blob, True)
    assert [tuple(x) for x in fr] == mf and [(int(o), int(w)) for o, w, _ in bl] == mb
    rows, st = gd.expected("gen_s7")
    with make_ctx(max_batch_bytes=SLOT, timing=True) as c:
        with pytest.raises(YsbError) as e:                   # the context has not been told: as before
            c.submit_kafka_lz4(blob, idx, fr, bl)
        assert e.value.code == -1 and "codec 2" in str(e.value)
        c.kafka_set_codecs(CODECS)
        c.submit_kafka_lz4(blob, idx, fr, bl)
        c.sync()
        assert c.drain_buckets() == rows and all(c.stats()[k] == x for k, x in st.items())
        li = c.kafka_lz4_info()
        nsnappy = sum(1 for _, w, _ in bl if int(w) & S.SNAPPY_BLOCK)
        assert (li["blocks"], li["snappy_blocks"], li["bad_blocks"], li["decoder"]) == (bl.size, nsnappy, 0, 3) and nsnappy > 500
        assert li["inflated_bytes"] == kafka.unframe_lz4_host(blob, idx, fr, bl)[2]["inflated_bytes"]
        c.reset()                                            # the setting is kept across reset
        c.submit_kafka_lz4(blob, idx, fr, bl, slot=1)
        c.sync()
        assert c.drain_buckets() == rows
    buf = aligned(len(blob) + 64)
    buf[5:5 + len(blob)] = np.frombuffer(blob, dtype=np.uint8)
    with make_ctx(max_batch_bytes=SLOT) as m:
        m.kafka_set_codecs(CODECS)
        m.host_register(buf)
        m.submit_kafka_lz4_mapped(buf, 5, len(blob), idx, fr, bl)
        got = counts_and_stats(m)
        m.host_unregister(buf)
    assert got[0] == rows and all(got[1][k] == x for k, x in st.items() if k in got[1])


def test_bad_block_in_the_middle_batch_drops_the_slot_batch():
    """A chunk of a xerial batch whose preamble says one byte more: the slot batch is dropped, the
    error is sticky and names the Kafka batch and the block."""
    blob = bytearray(mixed_blob())
    idx, fr, bl, _ = kafka.index_lz4(bytes(blob), accept_snappy=True)
    k = [int(c) for c in fr["codec"]].index(2) + 1            # the second xerial batch
    j = int(fr[k]["n_blocks"]) // 2
    at = int(bl[int(fr[k]["first_block"]) + j]["offset"])
    assert blob[at] == 100
    blob[at] = 101
    blob = bytes(blob)
    hv = kafka.verdict_lz4(blob, idx, fr, bl)
    assert (hv["bad_batches"], hv["first_bad"], hv["record"], hv["rule"]) == (1, k, j, 8)
    rows, st = gd.expected("gen_s7")
    with make_ctx(max_batch_bytes=SLOT) as c:
        c.kafka_set_codecs(CODECS)
        c.submit_kafka_lz4(blob, idx, fr, bl)
        with pytest.raises(YsbError) as e:
            c.sync()
        want = "Kafka batch %d (baseOffset %d), block %d" % (k, int(idx[k]["base_offset"]), j)
        assert e.value.code == -5 and want in str(e.value), str(e.value)
        good = mixed_blob()
        with pytest.raises(YsbError) as e2:
            c.submit_kafka_lz4(good, idx, fr, bl, slot=1)
        assert e2.value.code == -5 and want in str(e2.value)
        v = c.kafka_info(check=False)["verdict"]
        assert (v["bad_batches"], v["first_bad"], v["record"], v["rule"]) == (1, k, j, 8)
        c.reset()
        assert c.stats()["events"] == 0
        c.submit_kafka_lz4(good, idx, fr, bl)
        c.sync()
        assert c.drain_buckets() == rows


def test_a_flipped_wire_byte_is_rule_9_with_the_crc_on_the_device(dev):
    """With kafka_set_crc(CRC_DEVICE) a flipped byte inside a snappy batch's chunk is the CRC's to
    find (rule 9) though the block no longer decodes (rule 8 without the check)."""
    ok, _, v = record_block([("lit", 30), ("c2", 20, 3)])
    blob, idx, fr, bl, lead = call_of([ok, ok], 0)
    blob = bytearray(blob)
    blob[int(bl[2]["offset"])] ^= 0x01                           # the second chunk's preamble: another raw size
    blob = bytes(blob)
    assert kafka.verdict_lz4(blob, idx, fr, bl)["rule"] == 8
    hv = kafka.verdict_crc_lz4(blob, idx, fr, bl)
    assert (hv["first_bad"], hv["rule"]) == (1, 9)
    c = dev.c
    place = dev.place_for(blob, int(bl[1]["offset"]), 0)
    with pytest.raises(YsbError) as e:
        dev.run(blob, idx, fr, bl, 4096, place, fill=0xA5)
    assert "block 1" in str(e.value) and c.kafka_info()["verdict"]["rule"] == 8
    c.kafka_set_crc(kafka.CRC_DEVICE)
    try:
        with pytest.raises(YsbError) as e:
            dev.run(blob, idx, fr, bl, 4096, place, fill=0xA5)
        v = c.kafka_info()["verdict"]
        assert e.value.code == -5 and (v["bad_batches"], v["first_bad"], v["rule"]) == (1, 1, 9), str(e.value)
        assert not dev.written(4100, 0xA5)
    finally:
        c.kafka_set_crc(kafka.CRC_OFF)


def test_without_set_codecs_the_entries_refuse():
    ok, _, v = record_block([("lit", 30)])
    blob, idx, fr, bl, _ = call_of([ok], 0)
    with make_ctx(max_batch_bytes=SLOT) as c:
        d_in, d_out, d_off = c.device_alloc(4096), c.device_alloc(4096), c.device_alloc(64)
        c.h2d(d_in, np.frombuffer(blob, dtype=np.uint8))
        for call in (lambda: c.kafka_unframe_lz4_device(d_in, len(blob), idx, fr, bl, d_out, 4096, d_off, 16),
                     lambda: c.submit_kafka_lz4(blob, idx, fr, bl)):
            with pytest.raises(YsbError) as e:
                call()
            assert e.value.code == -1 and "codec 2" in str(e.value)
        with pytest.raises(YsbError) as e:
            c.kafka_set_codecs(0x5)
        assert e.value.code == -1
        c.kafka_set_codecs(CODECS)
        n, nb = c.kafka_unframe_lz4_device(d_in, len(blob), idx, fr, bl, d_out, 4096, d_off, 16)
        assert n == 3
        for p in (d_in, d_out, d_off):
            c.device_free(p)


def test_capacity_counts_the_preambles():
    """A slot batch's snappy blocks count their preambles' raw sizes, the other blocks 65536."""
    vals = [b'{"x":%d}' % i for i in range(40)]
    blob = S.pack(vals, 1)                                     # 40 batches of one small xerial chunk
    idx, fr, bl, _ = kafka.index_lz4(blob, accept_snappy=True)
    assert bl.size == 40
    with make_ctx(max_batch_bytes=1 << 20) as c:                # 40 x 65536 would not fit; the preambles' sum does
        c.kafka_set_codecs(CODECS)
        c.submit_kafka_lz4(blob, idx, fr, bl)
        c.sync()
        assert c.kafka_info()["records"] == 40 and c.kafka_lz4_info()["snappy_blocks"] == 40
        plain = K.pack([b"v%d" % i for i in range(17)], 1)
        mixed = blob + plain
        idx, fr, bl, _ = kafka.index_lz4(mixed, accept_snappy=True)
        with pytest.raises(YsbError) as e:
            c.submit_kafka_lz4(mixed, idx, fr, bl, slot=1)
        assert e.value.code == -4 and "17 other blocks" in str(e.value)
