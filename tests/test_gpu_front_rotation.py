"""GPU: every input format that is staged into a slot, through the same two slots of one context
in rotation.  The formats share the slot's wire buffer; the two Kafka kinds share its index
buffers with different layouts and different pinned sizes; the LZ4 directory and frame kinds
share its descriptor buffers.  Each format's own tests keep to one format per context: here a
slot takes each of the nine entries once, behind a different neighbour in the two orders, and
the counts must be those of ysb_submit on the same lines.

gen_s7's 1500 lines are cut at line starts into 18 consecutive pieces of 83 or 84 lines; piece i
goes to slot i % 2 through entry i % 9 of the order (nine is odd: every entry runs once on each
slot).  A piece is below 64 KiB, so it is one LZ4 block wherever it is compressed and both
capacity rules (frame batches, compressed Kafka batches) hold by construction."""
import numpy as np
import pytest

import golden_data as gd
from test_gpu_kafka import counts_and_stats, fixture_lines
from test_gpu_mapped import aligned
from test_gpu_parity import make_ctx
from ysb_amd import kafka, lz4

pytestmark = pytest.mark.gpu

SLOT = 1 << 20      # max_batch_bytes, as the neighbouring slot tests'
PIECES = 18
ENTRIES = ("raw", "raw_mapped", "raw_lz4", "lz4_mapped", "lz4_blocks", "lz4_blocks_mapped", "kafka", "kafka_mapped",
           "kafka_lz4")
MAPPED = {"raw_mapped", "lz4_mapped", "lz4_blocks_mapped", "kafka_mapped"}


@pytest.fixture(scope="module")
def pieces():
    """[(bytes, line offsets)] and the counts and stats of ysb_submit on them, slots alternating."""
    data, off, lines = fixture_lines("gen_s7")
    assert len(lines) == 1500
    cuts = [len(lines) * i // PIECES for i in range(PIECES + 1)]
    out = []
    for a, b in zip(cuts, cuts[1:]):
        assert b - a in (83, 84)
        part = lines[a:b]
        out.append((b"".join(part), np.cumsum([0] + [len(l) for l in part[:-1]]).astype(np.uint32)))
        assert len(out[-1][0]) <= 65536
    assert b"".join(p for p, _ in out) == data
    with make_ctx(max_batch_bytes=SLOT) as ref:
        for i, (p, o) in enumerate(out):
            ref.submit(p, o, slot=i % 2)
        want = counts_and_stats(ref)
    assert want[0] == gd.expected("gen_s7")[0]
    return out, want


def wire(entry, piece, off):
    """What the entry puts on the wire for a piece, and the arrays that go with it."""
    if entry in ("raw", "raw_mapped"):
        return np.frombuffer(piece, dtype=np.uint8), ()
    if entry in ("raw_lz4", "lz4_mapped"):
        blocks, directory = lz4.pack(piece, block_bytes=65536)
        assert len(directory) == 1
        return blocks, (directory,)
    if entry in ("lz4_blocks", "lz4_blocks_mapped"):      # each piece its own frame, no `more`
        frame = lz4.frame_pack(piece)
        index, _ = lz4.frame_index(frame)
        assert index.size == 1
        return frame, (index,)
    if entry in ("kafka", "kafka_mapped"):
        blob = kafka.pack(piece, off, batch_bytes=16384)
        index, _ = kafka.index(blob, check_crc=True)
        assert index.size > 1
        return blob, (index,)
    blob = kafka.pack(piece, off, batch_bytes=65536, codec="lz4")
    index, frames, blocks, info = kafka.index_lz4(blob, check_crc=True)
    assert blocks.size == 1 and info["compressed_batches"] == 1
    return blob, (index, frames, blocks)


def rotate(ctx, pieces, order):
    """Piece i to slot i % 2 through order[i % 9]; the mapped pieces lie in one registered buffer,
    each at a 16-byte boundary.  Returns counts_and_stats."""
    staged = [(order[i % len(order)],) + wire(order[i % len(order)], p, o) for i, (p, o) in enumerate(pieces)]
    places, pos = {}, 16
    for i, (entry, blob, _) in enumerate(staged):
        if entry in MAPPED:
            places[i] = pos
            pos += (blob.size + 15) // 16 * 16 + 16
    buf = aligned(pos)
    for i, at in places.items():
        buf[at:at + staged[i][1].size] = staged[i][1]
    ctx.host_register(buf)
    for i, (entry, blob, arrays) in enumerate(staged):
        slot, at = i % 2, places.get(i)
        if entry == "raw":
            ctx.submit_raw(blob, slot=slot)
        elif entry == "raw_mapped":
            ctx.submit_raw_mapped(buf, at, blob.size, slot=slot)
        elif entry == "raw_lz4":
            ctx.submit_raw_lz4(blob, arrays[0], slot=slot)
        elif entry == "lz4_mapped":                      # the GPU split, no rebase
            ctx.submit_lz4_mapped(buf, at, blob.size, arrays[0], slot=slot)
        elif entry == "lz4_blocks":
            ctx.submit_lz4_blocks(blob, arrays[0], slot=slot)
        elif entry == "lz4_blocks_mapped":               # (the index's offsets refer to the registered array)
            index = arrays[0].copy()
            index["offset"] += at
            ctx.submit_lz4_blocks_mapped(buf, index, slot=slot)
        elif entry == "kafka":
            ctx.submit_kafka(blob, arrays[0], slot=slot)
        elif entry == "kafka_mapped":
            ctx.submit_kafka_mapped(buf, at, blob.size, arrays[0], slot=slot)
        else:
            ctx.submit_kafka_lz4(blob, *arrays, slot=slot)
    got = counts_and_stats(ctx)
    ctx.host_unregister(buf)
    return got


@pytest.mark.parametrize("order", [ENTRIES, ENTRIES[::-1]], ids=["forward", "reversed"])
def test_rotation_counts_equal_ysb_submit(pieces, order):
    """Both orders (each format follows a different neighbour): the counts and stats of ysb_submit
    on the same pieces, which are gen_s7's expected rows."""
    parts, want = pieces
    with make_ctx(max_batch_bytes=SLOT) as ctx:
        assert rotate(ctx, parts, order) == want


def test_rotation_with_timing_settles_every_batch(pieces):
    """YSB_F_TIMING set (the formats share their slot's timing marks too): the same counts, and
    each front end has settled its batches -- two directory entries and two frame entries ran
    twice each, three Kafka entries twice each, one of them compressed."""
    parts, want = pieces
    with make_ctx(max_batch_bytes=SLOT, timing=True) as ctx:
        assert rotate(ctx, parts, ENTRIES) == want
        assert ctx.lz4_info()["batches"] == 4
        assert ctx.lz4_frame_info()["batches"] == 4
        assert ctx.kafka_info()["calls"] == 6
        assert ctx.kafka_lz4_info()["calls"] == 2
