"""LZ4-compressed Kafka record batches restated in pure Python (csrc/ysb_kafka_lz4.h is the C++
statement): kafka_model's batches whose records section is one standard LZ4 frame (attributes
codec 3), indexed, inflated with lz4_model's decoder and unframed with kafka_model's walk.

It holds its own XXH32, frame writer, a small greedy block compressor and a literal-only
compressor, so inputs do not depend on the library's compressor.  test_kafka_lz4_logic.py
compares it with the C ABI in both directions; the GPU tests check the device against both.
"""
import struct

import kafka_model as K
import lz4_model as L

MAGIC = 0x184D2204
BLOCK_MAX = 65536
RULE_CODEC = 8
CODEC_NAMES = {1: "gzip", 2: "snappy", 4: "zstd"}


# ---- XXH32 ---------------------------------------------------------------------------------

_P1, _P2, _P3, _P4, _P5 = 2654435761, 2246822519, 3266489917, 668265263, 374761393
_M = 0xFFFFFFFF


def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & _M


def xxh32(data, seed=0):
    data = bytes(data)
    n, p = len(data), 0
    if n >= 16:
        v = [(seed + _P1 + _P2) & _M, (seed + _P2) & _M, seed & _M, (seed - _P1) & _M]
        while n - p >= 16:
            for k in range(4):
                w, = struct.unpack_from("<I", data, p + 4 * k)
                v[k] = (_rotl((v[k] + w * _P2) & _M, 13) * _P1) & _M
            p += 16
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & _M
    else:
        h = (seed + _P5) & _M
    h = (h + n) & _M
    while n - p >= 4:
        w, = struct.unpack_from("<I", data, p)
        h = (_rotl((h + w * _P3) & _M, 17) * _P4) & _M
        p += 4
    while p < n:
        h = (_rotl((h + data[p] * _P5) & _M, 11) * _P1) & _M
        p += 1
    h ^= h >> 15
    h = (h * _P2) & _M
    h ^= h >> 13
    h = (h * _P3) & _M
    h ^= h >> 16
    return h


# ---- block compressors ------------------------------------------------------------------------

def _length(n):
    out = bytearray()
    while n >= 255:
        out.append(255)
        n -= 255
    out.append(n)
    return bytes(out)


def _seq(lits, off=0, ml=0):
    """One sequence: literals, then (ml >= 4) a match; ml 0: the block's last sequence."""
    m = ml - 4 if ml else 0
    out = bytearray([(min(len(lits), 15) << 4) | min(m, 15)])
    if len(lits) >= 15:
        out += _length(len(lits) - 15)
    out += lits
    if ml:
        out += struct.pack("<H", off)
        if m >= 15:
            out += _length(m - 15)
    return bytes(out)


def compress_literal(raw):
    """A block of one sequence: every byte a literal (always longer than raw)."""
    return _seq(bytes(raw))


def compress_greedy(raw):
    """A small greedy compressor: the last occurrence of each 4-byte window, the format's
    end-of-block conventions (the last 5 bytes literals, no match starting in the last 12)."""
    raw = bytes(raw)
    n, out, table = len(raw), bytearray(), {}
    i = anchor = 0
    while n >= 13 and i <= n - 12:
        w = raw[i:i + 4]
        c = table.get(w)
        table[w] = i
        if c is not None and i - c <= 65535:
            ml = 4
            while i + ml < n - 5 and raw[c + ml] == raw[i + ml]:
                ml += 1
            out += _seq(raw[anchor:i], i - c, ml)
            i += ml
            anchor = i
        else:
            i += 1
    out += _seq(raw[anchor:])
    return bytes(out)


# ---- the frame writer -------------------------------------------------------------------------

def frame_header(block_checksum=False, content_size=None, content_checksum=False, flg_extra=0, bd=0x40):
    flg = 0x40 | 0x20 | (0x10 if block_checksum else 0) | (0x08 if content_size is not None else 0) | \
        (0x04 if content_checksum else 0) | flg_extra
    desc = bytes([flg & 0xFF, bd]) + (struct.pack("<Q", content_size) if content_size is not None else b"")
    if flg & 1:
        desc += struct.pack("<I", 7)
    return struct.pack("<I", MAGIC) + desc + bytes([(xxh32(desc) >> 8) & 0xFF])


def frame_of_blocks(blocks, block_checksum=False, content_size=None, content_checksum=None, **hdr):
    """blocks: [(bytes, stored)] as they go on the wire; the frame around them."""
    out = bytearray(frame_header(block_checksum, content_size, content_checksum is not None, **hdr))
    for data, stored in blocks:
        out += struct.pack("<I", len(data) | (L.STORED if stored else 0)) + data
        if block_checksum:
            out += struct.pack("<I", xxh32(data))
    out += struct.pack("<I", 0)
    if content_checksum is not None:
        out += struct.pack("<I", xxh32(content_checksum))
    return bytes(out)


def frame(raw, block_bytes=BLOCK_MAX, compress=compress_greedy, allow_stored=True, flags=False):
    """raw as one frame of blocks of block_bytes raw bytes; a block that does not shrink stored.
    flags: block checksums, the content size and the content checksum all set."""
    raw = bytes(raw)
    blocks = []
    for a in range(0, len(raw), block_bytes):
        part = raw[a:a + block_bytes]
        comp = compress(part)
        blocks.append((part, True) if allow_stored and len(comp) >= len(part) else (comp, False))
    if flags:
        return frame_of_blocks(blocks, True, len(raw), raw)
    return frame_of_blocks(blocks)


# ---- batches ------------------------------------------------------------------------------------

def records_bytes(records):
    """The records section of K.pack_batch(records), uncompressed."""
    return K.pack_batch(records)[K.HEADER:]


def pack_batch(records, base_offset=0, codec=3, frame_bytes=None, records_count=None, **fr):
    """One batch whose records are a frame (or frame_bytes as it is, with records_count)."""
    if frame_bytes is None:
        frame_bytes = frame(records_bytes(records), **fr)
        records_count = len(records) if records_count is None else records_count
    return K.pack_batch(None, base_offset=base_offset, attributes=codec, records_count=records_count,
                        raw_records=frame_bytes)


def pack(values, per_batch, base_offset=0, frame_opts=None, **rec):
    out = bytearray()
    for i in range(0, len(values), per_batch):
        out += pack_batch([K.Record(v, **rec) for v in values[i:i + per_batch]], base_offset=base_offset + i,
                          **(frame_opts or {}))
    return bytes(out)


class FrameRefusal(Exception):
    def __init__(self, at, rule):
        super().__init__("byte %d: %s" % (at, rule))
        self.at, self.rule = at, rule


def frame_index(b):
    """[(offset, comp field)] of the frames in b; FrameRefusal(byte, short rule name)."""
    b = bytes(b)
    at, out = 0, []
    while at < len(b):
        if len(b) - at < 4:
            raise FrameRefusal(at, "truncated")
        magic, = struct.unpack_from("<I", b, at)
        if magic & 0xFFFFFFF0 == 0x184D2A50:
            if len(b) - at < 8:
                raise FrameRefusal(at, "truncated")
            size, = struct.unpack_from("<I", b, at + 4)
            at += 8
            if len(b) - at < size:
                raise FrameRefusal(at, "truncated")
            at += size
            continue
        if magic != MAGIC:
            raise FrameRefusal(at, "magic")
        at += 4
        if len(b) - at < 3:
            raise FrameRefusal(at, "truncated")
        flg, bd = b[at], b[at + 1]
        if flg >> 6 != 1:
            raise FrameRefusal(at, "version")
        if flg & 2 or bd & 0x8F:
            raise FrameRefusal(at + (0 if flg & 2 else 1), "reserved")
        hdr = 2 + (8 if flg & 8 else 0) + (4 if flg & 1 else 0)
        if len(b) - at < hdr + 1:
            raise FrameRefusal(at, "truncated")
        if b[at + hdr] != (xxh32(b[at:at + hdr]) >> 8) & 0xFF:
            raise FrameRefusal(at + hdr, "checksum")
        if not flg & 0x20:
            raise FrameRefusal(at, "linked")
        if flg & 1:
            raise FrameRefusal(at, "dictionary")
        if (bd >> 4) & 7 != 4:
            raise FrameRefusal(at + 1, "block maximum")
        at += hdr + 1
        while True:
            if len(b) - at < 4:
                raise FrameRefusal(at, "truncated")
            word, = struct.unpack_from("<I", b, at)
            at += 4
            if word == 0:
                break
            size = word & ~L.STORED
            if size > BLOCK_MAX or size == 0:
                raise FrameRefusal(at - 4, "block size")
            if len(b) - at < size:
                raise FrameRefusal(at, "truncated")
            out.append((at, word))
            at += size
            if flg & 0x10:
                if len(b) - at < 4:
                    raise FrameRefusal(at, "truncated")
                at += 4
        if flg & 4:
            if len(b) - at < 4:
                raise FrameRefusal(at, "truncated")
            at += 4
    return out


class Refusal(Exception):
    def __init__(self, offset, field, value, frame_at=None, rule=None):
        super().__init__("batch at byte %d: %s = %d (%s)" % (offset, field, value, rule))
        self.offset, self.field, self.value, self.frame_at, self.rule = offset, field, value, frame_at, rule


def index(buf, check_crc=False):
    """(batches, frames, blocks, summary): kafka_model.index accepting codec 0 and 3.  batches as
    K.index's dicts, frames [(first_block, n_blocks, codec)], blocks [(offset, comp field)]."""
    buf = bytes(buf)
    pos, out, frames, blocks, nrec, control, before, compressed = 0, [], [], [], 0, 0, 0, 0
    while len(buf) - pos >= K.HEADER:
        base_offset, batch_len, _epoch, magic, crc, attributes = struct.unpack_from(">qiibIh", buf, pos)
        count, = struct.unpack_from(">i", buf, pos + 57)
        if magic != 2:
            raise Refusal(pos, "magic", magic)
        if batch_len < 49:
            raise Refusal(pos, "batchLength", batch_len)
        codec = attributes & 7
        if codec not in (0, 3):
            raise Refusal(pos, "attributes.codec", codec, rule=CODEC_NAMES.get(codec, "unknown"))
        if count < 0:
            raise Refusal(pos, "recordsCount", count)
        span = 12 + batch_len
        if len(buf) - pos < span:
            break
        if check_crc and K.crc32c_fast(buf[pos + 21:pos + span]) != crc:
            raise Refusal(pos, "crc", crc)
        if attributes & 0x20:
            control += 1
            before += 1
        else:
            roff, rbytes = pos + K.HEADER, span - K.HEADER
            if codec == 3:
                try:
                    mine = [(roff + o, w) for o, w in frame_index(buf[roff:roff + rbytes])]
                except FrameRefusal as e:
                    raise Refusal(pos, "attributes.codec", 3, e.at, e.rule)
                compressed += 1
            else:
                mine = [(roff + a, min(BLOCK_MAX, rbytes - a) | L.STORED) for a in range(0, rbytes, BLOCK_MAX)]
            out.append(dict(records_off=roff, records_bytes=rbytes, n_records=count, first_record=nrec,
                            base_offset=base_offset, control_before=before))
            frames.append((len(blocks), len(mine), codec))
            blocks += mine
            before = 0
            nrec += count
        pos += span
    return out, frames, blocks, dict(n_batches=len(out), n_records=nrec, consumed=pos, control_batches=control,
                                     compressed_batches=compressed, blocks=len(blocks),
                                     stored_blocks=sum(1 for _, w in blocks if w & L.STORED),
                                     comp_bytes=sum(w & ~L.STORED for _, w in blocks))


def inflate_batch(buf, frame_entry, blocks):
    """The batch's decoded bytes, or the index of its smallest bad block."""
    first, n, _ = frame_entry
    out = bytearray()
    for j in range(n):
        off, word = blocks[first + j]
        data = buf[off:off + (word & ~L.STORED)]
        if word & L.STORED:
            out += data
            continue
        try:
            out += L.decode_block(data, L.measure_block(data))
        except L.Bad:
            return j
    return bytes(out)


def unframe(buf, idx, frames, blocks):
    """(values, offsets, counters, verdict): verdict None or (bad_batches, first_bad, record,
    rule) over ALL batches, as the library reports it; values only for a good call."""
    buf = bytes(buf)
    out, offs = bytearray(), []
    ct = dict(records=0, null_values=0, keyed=0, headers=0, value_bytes=0)
    bad, first = 0, None
    for k, b in enumerate(idx):
        rec = inflate_batch(buf, frames[k], blocks)
        if isinstance(rec, int):
            v = (k, rec, RULE_CODEC)
        else:
            one = dict(b, records_off=0, records_bytes=len(rec), first_record=0)
            v = K.verdict(rec, [one])
            v = None if v is None else (k, v[1], v[2])
        if v is not None:
            bad += 1
            first = first or v
            continue
        if not bad:
            o, of, c = K.unframe(rec, [one])
            offs += [len(out) + x for x in of[:-1]]
            out += o
            for key in ("records", "null_values", "keyed", "headers"):
                ct[key] += c[key]
    if bad:
        return None, None, None, (bad,) + first
    offs.append(len(out))
    ct["value_bytes"] = len(out)
    return bytes(out), offs, ct, None
