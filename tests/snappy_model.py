"""Snappy blocks and snappy-compressed Kafka record batches restated in pure Python
(csrc/ysb_snappy.h and the codec-2 parts of csrc/ysb_kafka_lz4.h are the C++ statement): the
preamble, the four element forms, a block decoder with every refusal, element builders for
hand-made blocks, a small greedy compressor of its own, the Java client's xerial framing, and
kafka_lz4_model's index, inflate and unframe with codec 2 accepted.

test_snappy_logic.py compares it with the C ABI in both directions and with the real snappy
(pyarrow's); the GPU tests check the device against both.
"""
import struct

import kafka_lz4_model as Z
import kafka_model as K
import lz4_model as L

MAX_RAW = 65536
MAX_COMP = 32 + MAX_RAW + MAX_RAW // 6
SNAPPY_BLOCK = 0x40000000
LEN_MASK = 0x3FFFFFFF
XERIAL_MAGIC = b"\x82SNAPPY\x00"
XERIAL_HEADER = 16
XERIAL_CHUNK = 32768
CODEC = 2


class Bad(Exception):
    """A block that breaks the format's rules (`rule` a short name)."""

    def __init__(self, rule):
        super().__init__(rule)
        self.rule = rule


# ---- element builders ---------------------------------------------------------------------------

def preamble(n, pad=0):
    """n as a varint; pad: that many extra bytes in a non-minimal form (85 00 for 5)."""
    out = bytearray()
    while n >= 128:
        out.append((n & 127) | 128)
        n >>= 7
    out.append(n)
    for _ in range(pad):
        out[-1] |= 128
        out.append(0)
    return bytes(out)


def literal(data, length_bytes=None):
    """A literal; length_bytes 1..4 forces that many length bytes (a non-minimal form)."""
    data = bytes(data)
    m = len(data) - 1
    if length_bytes is None:
        length_bytes = 0 if m < 60 else 1 if m < 256 else 2 if m < 65536 else 3 if m < 1 << 24 else 4
    if length_bytes == 0:
        return bytes([m << 2]) + data
    return bytes([(59 + length_bytes) << 2]) + m.to_bytes(length_bytes, "little") + data


def copy1(length, offset):
    assert 4 <= length <= 11 and 0 <= offset < 2048
    return bytes([1 | (length - 4) << 2 | (offset >> 8) << 5, offset & 255])


def copy2(length, offset):
    assert 1 <= length <= 64 and 0 <= offset < 65536
    return bytes([2 | (length - 1) << 2]) + struct.pack("<H", offset)


def copy4(length, offset):
    assert 1 <= length <= 64
    return bytes([3 | (length - 1) << 2]) + struct.pack("<I", offset)


# ---- the decoder ----------------------------------------------------------------------------------

def read_preamble(b):
    """(raw size, first element's position) of block b; Bad for a preamble of more than 5 bytes,
    a value >= 2^32, or one the block's end cuts."""
    v = 0
    for i in range(5):
        if i >= len(b):
            raise Bad("preamble cut")
        c = b[i]
        if i == 4 and c > 15:
            raise Bad("preamble long")
        v |= (c & 127) << (7 * i)
        if c < 128:
            return v, i + 1
    raise Bad("preamble long")


def block_raw(b):
    """The preamble's size when it is in 1..65536, else 0 (what the index and the kernels take)."""
    try:
        raw, _ = read_preamble(b)
    except Bad:
        return 0
    return raw if raw <= MAX_RAW else 0


def decode_block(b):
    """The raw bytes of block b; Bad(rule) for a block that breaks a rule."""
    b = bytes(b)
    raw, ip = read_preamble(b)
    if raw == 0 or raw > MAX_RAW:
        raise Bad("size")
    out = bytearray()
    n = len(b)
    while ip < n:
        tag = b[ip]
        ip += 1
        kind = tag & 3
        if kind == 0:
            m = tag >> 2
            if m >= 60:
                nb = m - 59
                if n - ip < nb:
                    raise Bad("cut")
                m = int.from_bytes(b[ip:ip + nb], "little")
                ip += nb
            ln = m + 1
            if ln > raw - len(out):
                raise Bad("over")
            if ln > n - ip:
                raise Bad("cut")
            out += b[ip:ip + ln]
            ip += ln
            continue
        if kind == 1:
            if n - ip < 1:
                raise Bad("cut")
            ln, off = 4 + ((tag >> 2) & 7), (tag >> 5) << 8 | b[ip]
            ip += 1
        elif kind == 2:
            if n - ip < 2:
                raise Bad("cut")
            ln, off = (tag >> 2) + 1, b[ip] | b[ip + 1] << 8
            ip += 2
        else:
            if n - ip < 4:
                raise Bad("cut")
            ln, off = (tag >> 2) + 1, int.from_bytes(b[ip:ip + 4], "little")
            ip += 4
        if off == 0:
            raise Bad("offset 0")
        if off > len(out):
            raise Bad("offset before the block")
        if ln > raw - len(out):
            raise Bad("over")
        for _ in range(ln):          # byte order: an overlap replicates
            out.append(out[-off])
    if len(out) != raw:
        raise Bad("under")
    return bytes(out)


# ---- a compressor of the model's own ---------------------------------------------------------------

def compress_literal(raw):
    """A block of literals of at most 60 bytes each (always longer than raw)."""
    raw = bytes(raw)
    return preamble(len(raw)) + b"".join(literal(raw[a:a + 60]) for a in range(0, len(raw), 60))


def compress_greedy(raw):
    """Greedy over the last occurrence of each 4-byte window; copies in pieces of at most 64, the
    one-byte-offset form where it fits, else the two-byte form."""
    raw = bytes(raw)
    n, out, table = len(raw), bytearray(preamble(len(raw))), {}
    i = anchor = 0
    while i + 4 <= n:
        w = raw[i:i + 4]
        c = table.get(w)
        table[w] = i
        if c is None or i - c > 65535:
            i += 1
            continue
        ml = 4
        while i + ml < n and raw[c + ml] == raw[i + ml]:
            ml += 1
        if i > anchor:
            out += literal(raw[anchor:i])
        off = i - c
        i += ml
        anchor = i
        while ml > 0:
            piece = 64 if ml >= 68 else 60 if ml > 64 else ml
            out += copy1(piece, off) if 4 <= piece <= 11 and off < 2048 else copy2(piece, off)
            ml -= piece
    if n > anchor:
        out += literal(raw[anchor:])
    return bytes(out)


# ---- the records section: a xerial stream or one raw block ------------------------------------------

def xerial(raw, chunk=XERIAL_CHUNK, compress=compress_greedy, version=1, compat=1):
    raw = bytes(raw)
    out = bytearray(XERIAL_MAGIC + struct.pack(">ii", version, compat))
    for a in range(0, len(raw), chunk):
        z = compress(raw[a:a + chunk])
        out += struct.pack(">i", len(z)) + z
    return bytes(out)


def xerial_of_chunks(chunks, version=1, compat=1):
    return XERIAL_MAGIC + struct.pack(">ii", version, compat) + b"".join(struct.pack(">i", len(z)) + z for z in chunks)


class SectionRefusal(Exception):
    def __init__(self, at, rule):
        super().__init__("byte %d: %s" % (at, rule))
        self.at, self.rule = at, rule


def section_index(b):
    """[(offset, length)] of the blocks of a records section; SectionRefusal(byte, short rule)."""
    b = bytes(b)

    def block(at, ln):
        if ln > MAX_COMP:
            raise SectionRefusal(at, "block bound")
        try:
            raw, _ = read_preamble(b[at:at + ln])
        except Bad:
            raise SectionRefusal(at, "preamble")
        if raw == 0 or raw > MAX_RAW:
            raise SectionRefusal(at, "raw size")
        return at, ln

    if b[:8] != XERIAL_MAGIC:
        if not b:
            raise SectionRefusal(0, "empty")
        return [block(0, len(b))]
    if len(b) < XERIAL_HEADER:
        raise SectionRefusal(8, "header cut")
    compat, = struct.unpack_from(">i", b, 12)
    if compat != 1:
        raise SectionRefusal(12, "compatible version")
    out, pos = [], XERIAL_HEADER
    while pos < len(b):
        if len(b) - pos < 4:
            raise SectionRefusal(pos, "trailing bytes")
        ln, = struct.unpack_from(">i", b, pos)
        if ln <= 0:
            raise SectionRefusal(pos, "chunk length not positive")
        if ln > len(b) - pos - 4:
            raise SectionRefusal(pos, "chunk length past the section")
        out.append(block(pos + 4, ln))
        pos += 4 + ln
    return out


# ---- batches -------------------------------------------------------------------------------------------

def pack_batch(records, base_offset=0, framing="xerial", chunk=XERIAL_CHUNK, compress=compress_greedy, section=None,
               records_count=None):
    """One codec-2 batch: the records as a xerial stream or one raw block (or `section` as it is)."""
    if section is None:
        body = Z.records_bytes(records)
        section = xerial(body, chunk, compress) if framing == "xerial" else compress(body)
        records_count = len(records) if records_count is None else records_count
    return K.pack_batch(None, base_offset=base_offset, attributes=CODEC, records_count=records_count, raw_records=section)


def pack(values, per_batch, base_offset=0, **kw):
    out = bytearray()
    for i in range(0, len(values), per_batch):
        out += pack_batch([K.Record(v) for v in values[i:i + per_batch]], base_offset=base_offset + i, **kw)
    return bytes(out)


def index(buf, check_crc=False):
    """kafka_lz4_model.index with codec 2 accepted: blocks [(offset, comp field)], a snappy block's
    field its length | SNAPPY_BLOCK.  Z.Refusal with frame_at the chunk's byte inside the records."""
    buf = bytes(buf)
    pos, out, frames, blocks, nrec, control, before, compressed = 0, [], [], [], 0, 0, 0, 0
    while len(buf) - pos >= K.HEADER:
        base_offset, batch_len, _epoch, magic, crc, attributes = struct.unpack_from(">qiibIh", buf, pos)
        count, = struct.unpack_from(">i", buf, pos + 57)
        if magic != 2:
            raise Z.Refusal(pos, "magic", magic)
        if batch_len < 49:
            raise Z.Refusal(pos, "batchLength", batch_len)
        codec = attributes & 7
        if codec not in (0, 2, 3):
            raise Z.Refusal(pos, "attributes.codec", codec, rule=Z.CODEC_NAMES.get(codec, "unknown"))
        if count < 0:
            raise Z.Refusal(pos, "recordsCount", count)
        span = 12 + batch_len
        if len(buf) - pos < span:
            break
        if check_crc and K.crc32c_fast(buf[pos + 21:pos + span]) != crc:
            raise Z.Refusal(pos, "crc", crc)
        if attributes & 0x20:
            control += 1
            before += 1
        else:
            roff, rbytes = pos + K.HEADER, span - K.HEADER
            if codec == 3:
                try:
                    mine = [(roff + o, w) for o, w in Z.frame_index(buf[roff:roff + rbytes])]
                except Z.FrameRefusal as e:
                    raise Z.Refusal(pos, "attributes.codec", 3, e.at, e.rule)
                compressed += 1
            elif codec == 2:
                try:
                    mine = [(roff + o, n | SNAPPY_BLOCK) for o, n in section_index(buf[roff:roff + rbytes])]
                except SectionRefusal as e:
                    raise Z.Refusal(pos, "attributes.codec", 2, e.at, e.rule)
                compressed += 1
            else:
                mine = [(roff + a, min(Z.BLOCK_MAX, rbytes - a) | L.STORED) for a in range(0, rbytes, Z.BLOCK_MAX)]
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
                                     comp_bytes=sum(w & LEN_MASK for _, w in blocks))


def inflate_batch(buf, frame_entry, blocks):
    """The batch's decoded bytes, or the index of its smallest bad block."""
    first, n, _ = frame_entry
    out = bytearray()
    for j in range(n):
        off, word = blocks[first + j]
        if word & SNAPPY_BLOCK:
            try:
                out += decode_block(buf[off:off + (word & LEN_MASK)])
            except Bad:
                return j
            continue
        one = Z.inflate_batch(buf, (first + j, 1, 0), blocks)
        if isinstance(one, int):
            return j
        out += one
    return bytes(out)


def unframe(buf, idx, frames, blocks):
    """kafka_lz4_model.unframe over an index that may hold snappy blocks: (values, offsets,
    counters, verdict), verdict None or (bad_batches, first_bad, record, rule)."""
    buf = bytes(buf)
    out, offs = bytearray(), []
    ct = dict(records=0, null_values=0, keyed=0, headers=0, value_bytes=0)
    bad, first = 0, None
    for k, b in enumerate(idx):
        rec = inflate_batch(buf, frames[k], blocks)
        if isinstance(rec, int):
            v = (k, rec, Z.RULE_CODEC)
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


# ---- hand-made blocks for the device and the native tests --------------------------------------------

def malformed_blocks():
    """[(name, block bytes, rule)]: each breaks exactly one rule."""
    lit8 = literal(b"abcdefgh")
    return [
        ("offset 0", preamble(12) + lit8 + copy2(4, 0), "offset 0"),
        ("copy at output position 0", preamble(4) + copy2(4, 1), "offset before the block"),
        ("offset one past the output", preamble(12) + lit8 + copy2(4, 9), "offset before the block"),
        ("cut literal", preamble(8) + lit8[:-1], "cut"),
        ("cut length bytes", preamble(300) + bytes([61 << 2, 0x2B]), "cut"),
        ("cut copy-1", preamble(12) + lit8 + copy1(4, 1)[:1], "cut"),
        ("cut copy-2", preamble(12) + lit8 + copy2(4, 1)[:2], "cut"),
        ("cut copy-4", preamble(12) + lit8 + copy4(4, 1)[:4], "cut"),
        ("literal over the size", preamble(7) + lit8, "over"),
        ("copy over the size", preamble(11) + lit8 + copy2(4, 8), "over"),
        ("input left at the size", preamble(8) + lit8 + literal(b"x"), "over"),
        ("output under the size", preamble(13) + lit8 + copy2(4, 8), "under"),
        ("only a preamble", preamble(5), "under"),
        ("a preamble of 0", preamble(0), "size"),
        ("a preamble of 65537", preamble(65537) + literal(b"x"), "size"),
        ("a 6-byte preamble", bytes([0x88, 0x80, 0x80, 0x80, 0x80, 0x00]) + lit8, "preamble long"),
        ("a preamble of 2^32", bytes([0x80, 0x80, 0x80, 0x80, 0x10]) + lit8, "preamble long"),
        ("a cut preamble", bytes([0x88, 0x80]), "preamble cut"),
        ("a 4-byte literal length of 2^32 - 1", preamble(8) + bytes([63 << 2, 255, 255, 255, 255]) + b"abcdefgh", "over"),
    ]
