"""A pure-Python restatement of Kafka's record batch format (message format v2), written from
the format's description, not from the library's C++: the packer, the index and the unframer
that tests compare the C ABI (ysb_kafka_index / _unframe_host / _pack) and the GPU against, in
both directions.

Everything is big-endian.  A batch: baseOffset i64, batchLength i32 (the bytes after it),
partitionLeaderEpoch i32, magic i8 = 2, crc u32 (CRC-32C from attributes to the end), attributes
i16, lastOffsetDelta i32, baseTimestamp i64, maxTimestamp i64, producerId i64, producerEpoch i16,
baseSequence i32, recordsCount i32 (61 bytes), then the records.  A record: length varint,
attributes i8, timestampDelta varlong, offsetDelta varint, keyLength varint (-1 null), key,
valueLength varint (-1 null), value, headersCount varint, then per header keyLength varint, key,
valueLength varint (-1 null), value.  Varints: base-128 little-endian groups of a zigzag value.

No Kafka library is installed where the tests run, so parity against a real broker is not pinned.
"""
import struct

HEADER = 61
RULE = {"varint": 1, "length": 2, "past_batch": 3, "key": 4, "value": 5, "headers": 6, "count": 7}


def crc32c(data, crc=0):
    crc ^= 0xFFFFFFFF
    for b in bytes(data):
        crc ^= b
        for _ in range(8):
            crc = (crc >> 1) ^ (0x82F63B78 if crc & 1 else 0)
    return crc ^ 0xFFFFFFFF


_CRC_TABLE = []
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = (_c >> 1) ^ (0x82F63B78 if _c & 1 else 0)
    _CRC_TABLE.append(_c)


def crc32c_fast(data):
    crc = 0xFFFFFFFF
    t = _CRC_TABLE
    for b in bytes(data):
        crc = t[(crc ^ b) & 255] ^ (crc >> 8)
    return crc ^ 0xFFFFFFFF


def zigzag(v, bits=32):
    return ((v << 1) ^ (v >> (bits - 1))) & ((1 << bits) - 1)


def unzigzag(u):
    return (u >> 1) ^ -(u & 1)


def uvarint(u, pad=0):
    """u as base-128 groups; pad extra groups make a non-minimal (legal) encoding."""
    out = bytearray()
    while u >= 128:
        out.append((u & 127) | 128)
        u >>= 7
    out.append(u)
    for _ in range(pad):
        out[-1] |= 128
        out.append(0)
    return bytes(out)


def varint(v, pad=0):
    return uvarint(zigzag(v, 32), pad)


def varlong(v, pad=0):
    return uvarint(zigzag(v, 64), pad)


class BadVarint(Exception):
    pass


def read_varint(buf, pos, end, limit=5, bits=32):
    """(value, next position).  BadVarint when the groups pass `limit` bytes or `end`."""
    u = 0
    for k in range(limit):
        if pos >= end:
            raise BadVarint()
        b = buf[pos]
        pos += 1
        u |= (b & 127) << (7 * k)
        if not b & 128:
            return unzigzag(u & ((1 << bits) - 1)), pos
    raise BadVarint()


class Record:
    def __init__(self, value, key=None, headers=(), ts_delta=0, offset_delta=None, attributes=0, pad=0, length_pad=0):
        self.value, self.key, self.headers = value, key, tuple(headers)
        self.ts_delta, self.offset_delta, self.attributes = ts_delta, offset_delta, attributes
        self.pad, self.length_pad = pad, length_pad   # non-minimal varints inside the record / for its length

    def body(self, offset_delta):
        p = self.pad
        b = bytearray([self.attributes & 255])
        b += varlong(self.ts_delta, p)
        b += varint(offset_delta, p)
        b += varint(-1 if self.key is None else len(self.key), p)
        b += self.key or b""
        b += varint(-1 if self.value is None else len(self.value), p)
        b += self.value or b""
        b += varint(len(self.headers), p)
        for k, v in self.headers:
            b += varint(len(k), p) + k
            b += varint(-1 if v is None else len(v), p) + (v or b"")
        return bytes(b)


def pack_batch(records, base_offset=0, base_timestamp=0, attributes=0, records_count=None, raw_records=None):
    """One batch.  records: Record objects (offsetDelta i unless a record names its own);
    raw_records: the records' bytes as they are (malformed corpora), with records_count."""
    if raw_records is None:
        body = bytearray()
        last = 0
        for i, r in enumerate(records):
            d = i if r.offset_delta is None else r.offset_delta
            last = max(last, d)
            rb = r.body(d)
            body += varint(len(rb), r.length_pad) + rb
        n = len(records)
        max_ts = base_timestamp + max([r.ts_delta for r in records] + [0])
    else:
        body, n, last, max_ts = bytes(raw_records), records_count, max((records_count or 1) - 1, 0), base_timestamp
    if records_count is not None:
        n = records_count
    tail = struct.pack(">hiqqqhii", attributes, last, base_timestamp, max_ts, -1, -1, -1, n) + bytes(body)
    return struct.pack(">qiibI", base_offset, 4 + 1 + 4 + len(tail), 0, 2, crc32c_fast(tail)) + tail


def pack(values, per_batch, base_offset=0, **rec):
    """values (bytes or None each) as batches of per_batch records, offsets consecutive."""
    out = bytearray()
    for i in range(0, len(values), per_batch):
        out += pack_batch([Record(v, **rec) for v in values[i:i + per_batch]], base_offset=base_offset + i)
    return bytes(out)


class Refusal(Exception):
    def __init__(self, offset, field, value):
        super().__init__("batch at byte %d: %s = %d" % (offset, field, value))
        self.offset, self.field, self.value = offset, field, value


def index(buf, check_crc=False):
    """([{records_off, records_bytes, n_records, first_record, base_offset, control_before}],
    {n_batches, n_records, consumed, control_batches})."""
    buf = bytes(buf)
    pos, out, nrec, control, before = 0, [], 0, 0, 0
    while len(buf) - pos >= HEADER:
        base_offset, batch_len, _epoch, magic, crc, attributes = struct.unpack_from(">qiibIh", buf, pos)
        count, = struct.unpack_from(">i", buf, pos + 57)
        if magic != 2:
            raise Refusal(pos, "magic", magic)
        if batch_len < 49:
            raise Refusal(pos, "batchLength", batch_len)
        if attributes & 7:
            raise Refusal(pos, "attributes.codec", attributes & 7)
        if count < 0:
            raise Refusal(pos, "recordsCount", count)
        span = 12 + batch_len
        if len(buf) - pos < span:
            break
        if check_crc and crc32c_fast(buf[pos + 21:pos + span]) != crc:
            raise Refusal(pos, "crc", crc)
        if attributes & 0x20:
            control += 1
            before += 1
        else:
            out.append(dict(records_off=pos + HEADER, records_bytes=span - HEADER, n_records=count, first_record=nrec,
                            base_offset=base_offset, control_before=before))
            before = 0
            nrec += count
        pos += span
    return out, dict(n_batches=len(out), n_records=nrec, consumed=pos, control_batches=control)


class BadBatch(Exception):
    def __init__(self, batch, record, rule):
        super().__init__("batch %d record %d: %s" % (batch, record, rule))
        self.batch, self.record, self.rule = batch, record, RULE[rule]


def _record(buf, pos, n):
    """The record at pos of the n record bytes buf: (value or None, end, keyed, headers), or
    raises the rule's name."""
    try:
        length, pos = read_varint(buf, pos, n)
    except BadVarint:
        raise ValueError("varint")
    if length < 6:
        raise ValueError("length")
    if length > n - pos:
        raise ValueError("past_batch")
    end = pos + length
    try:
        pos += 1
        _, pos = read_varint(buf, pos, end, 10, 64)
        _, pos = read_varint(buf, pos, end)
        klen, pos = read_varint(buf, pos, end)
        if klen < -1 or klen > end - pos:
            raise ValueError("key")
        pos += max(klen, 0)
        vlen, pos = read_varint(buf, pos, end)
        if vlen < -1 or vlen > end - pos:
            raise ValueError("value")
        value = None if vlen < 0 else buf[pos:pos + vlen]
        pos += max(vlen, 0)
        nh, pos = read_varint(buf, pos, end)
        if nh < 0:
            raise ValueError("headers")
        for _ in range(nh):
            hk, pos = read_varint(buf, pos, end)
            if hk < 0 or hk > end - pos:
                raise ValueError("headers")
            pos += hk
            hv, pos = read_varint(buf, pos, end)
            if hv < -1 or hv > end - pos:
                raise ValueError("headers")
            pos += max(hv, 0)
    except BadVarint:
        raise ValueError("varint")
    if pos != end:
        raise ValueError("headers")
    return value, end, klen >= 0, nh


def unframe(buf, idx):
    """(values back to back, offsets with the total last, counters) of the indexed batches;
    BadBatch for the first bad (batch, record, rule)."""
    buf = bytes(buf)
    out, offs = bytearray(), []
    ct = dict(records=0, null_values=0, keyed=0, headers=0, value_bytes=0)
    for k, b in enumerate(idx):
        rec = buf[b["records_off"]:b["records_off"] + b["records_bytes"]]
        n, pos = len(rec), 0
        for i in range(b["n_records"]):
            if pos >= n:
                raise BadBatch(k, i, "count")
            try:
                value, pos, keyed, nh = _record(rec, pos, n)
            except ValueError as e:
                raise BadBatch(k, i, e.args[0])
            offs.append(len(out))
            out += value or b""
            ct["records"] += 1
            ct["null_values"] += value is None
            ct["keyed"] += keyed
            ct["headers"] += nh
        if pos != n:
            raise BadBatch(k, b["n_records"], "count")
    offs.append(len(out))
    ct["value_bytes"] = len(out)
    return bytes(out), offs, ct


def verdict(buf, idx):
    """The first bad (batch, record, rule number) or None."""
    try:
        unframe(buf, idx)
    except BadBatch as e:
        return e.batch, e.record, e.rule
    return None


def verdict_all(buf, idx):
    """Every batch walked on its own, as the library reports a call: None, or (bad_batches,
    first_bad, record, rule number) with the record and rule of the first bad batch."""
    bad = []
    for k, b in enumerate(idx):
        v = verdict(buf, [b])
        if v is not None:
            bad.append((k,) + v[1:])
    return ((len(bad),) + bad[0]) if bad else None


def malformed_corpus():
    """One case per rule: [(name, rule, records_count, record bytes)], a good record in front of
    the broken one.  Byte for byte the corpus of tests/native/kafka_logic.cpp (test_kafka_logic.py
    compares them), which that program walks under the host sanitizers, each case cut at every byte."""
    good = Record(b'{"a":1}', key=b"k", headers=[(b"h", None)], ts_delta=-3).body(0)
    g = varint(len(good)) + good

    def case(body, length=None):
        return g + varint(len(body) if length is None else length) + body

    head = bytes([0]) + varlong(0) + varint(1)   # a second record up to its key length
    ts11 = bytes([0]) + b"\x80" * 10 + b"\x01\x00\x00\x00\x00\x00"
    return [
        ("length varint of six bytes", "varint", 2, g + b"\x80\x80\x80\x80\x80\x01" + good),
        ("length varint cut by the batch", "varint", 2, g + b"\x80\x80"),
        ("length 5", "length", 2, case(good[:5])),
        ("negative length", "length", 2, case(good, -3)),
        ("record past the batch", "past_batch", 2, case(good, len(good) + 1)),
        ("timestamp delta of eleven bytes", "varint", 2, case(ts11)),
        ("key past the record", "key", 2, case(head + varint(100) + b"abcdef")),
        ("key length -2", "key", 2, case(head + varint(-2) + b"abcdef")),
        ("value past the record", "value", 2, case(head + varint(-1) + varint(50) + b"abcdef")),
        ("bytes behind the headers", "headers", 2, case(good + b"x")),
        ("three headers stated, one present", "varint", 2,
         case(head + varint(-1) + varint(2) + b"ab" + varint(3) + varint(1) + b"h" + varint(1) + b"v")),
        ("header value past the record", "headers", 2,
         case(head + varint(-1) + varint(2) + b"ab" + varint(1) + varint(1) + b"h" + varint(9) + b"v")),
        ("negative headers count", "headers", 2, case(head + varint(-1) + varint(2) + b"ab" + varint(-1))),
        ("a record short", "count", 3, case(good)),
        ("a record over", "count", 1, case(good)),
    ]
