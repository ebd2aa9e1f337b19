"""Kafka record batches on the host side (csrc/ysb_kafka.h through the C ABI): the index of a
fetch response or a .log segment, the host model of the GPU's unframing, and a packer for
sources, tools and tests that have no Kafka client of their own.

YsbContext.submit_kafka takes the bytes and the index that `index` returns.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib

CHECK_CRC = 1
CHECK_CRC_CONTROL = 2   # only the control batches the index skips: the rest is the device's (CRC_DEVICE)
CRC_OFF, CRC_DEVICE = 0, 1   # YsbContext.kafka_set_crc
BATCH = np.dtype([("records_off", "<u8"), ("records_bytes", "<u4"), ("n_records", "<u4"), ("first_record", "<u8"),
                  ("base_offset", "<i8"), ("control_before", "<u4"), ("reserved", "<u4")])
FRAME = np.dtype([("first_block", "<u8"), ("n_blocks", "<u4"), ("codec", "<u4")])
BLOCK = np.dtype([("offset", "<u8"), ("comp_bytes", "<u4"), ("reserved", "<u4")])   # ysb_lz4_frame_block
CODEC_LZ4 = 3
CODEC_SNAPPY = 2
ACCEPT_SNAPPY = 0x100        # index_lz4(accept_snappy=True)
SNAPPY_BLOCK = 0x40000000    # BLOCK.comp_bytes bit 30: a snappy block
CODECS = {"none": 1, "snappy": 4, "lz4": 8}   # YsbContext.kafka_set_codecs
RULES = {0: "none", 1: "varint", 2: "length", 3: "past_batch", 4: "key", 5: "value", 6: "headers", 7: "count",
         8: "codec", 9: "crc"}
DEFAULT_BATCH = 16384   # a producer's default batch.size


def _u8(data):
    return np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) \
        else np.ascontiguousarray(data, dtype=np.uint8)


def crc32c(data):
    """CRC-32C (Castagnoli) as the batch header carries it."""
    src = _u8(data)
    return lib().ysb_kafka_crc32c(src.ctypes.data if src.size else None, src.size)


def _index_flags(check_crc, check_control_crc):
    return (CHECK_CRC if check_crc else 0) | (CHECK_CRC_CONTROL if check_control_crc else 0)


def index(data, check_crc=False, check_control_crc=False):
    """ysb_kafka_index: (index, summary dict) of a buffer of record batches.  index is a BATCH
    array with one entry per data batch; summary["consumed"] stops in front of a last batch that
    is not whole.  Raises YsbError (YSB_ERR_FORMAT) naming the byte offset, the field and the rule
    for a batch the library does not take (magic other than 2, a codec, batchLength < 49, a negative
    recordsCount, with check_crc a CRC-32C mismatch; check_control_crc verifies only the control
    batches the index skips, which the device's check never sees)."""
    src = _u8(data)
    flags = _index_flags(check_crc, check_control_crc)
    info = _lib.YsbKafkaSummary()
    p = src.ctypes.data if src.size else None
    rc = lib().ysb_kafka_index(p, src.size, flags, None, 0, C.byref(info))
    if rc not in (0, -4):
        check(rc)
    idx = np.zeros(info.n_batches, dtype=BATCH)
    if info.n_batches:
        check(lib().ysb_kafka_index(p, src.size, flags, idx.ctypes.data, idx.size, C.byref(info)))
    return idx, {k: getattr(info, k) for k, _ in info._fields_}


def index_lz4(data, check_crc=False, check_control_crc=False, accept_snappy=False):
    """ysb_kafka_index_lz4: (batches, frames, blocks, summary dict) of a buffer whose record
    batches are uncompressed (codec 0) or LZ4-compressed (codec 3).  batches is a BATCH array
    (records_off / records_bytes: the wire bytes), frames a FRAME array with one entry per batch,
    blocks a BLOCK array with every block's place in `data`.  Raises YsbError (YSB_ERR_FORMAT) for
    what `index` refuses, for gzip, snappy and zstd by name, and for a frame the LZ4 frame index
    refuses (naming the Kafka batch, its byte, and the frame's byte and rule).
    accept_snappy=True: snappy batches (codec 2) are indexed too, a block per xerial chunk or one
    for a raw block, each tagged SNAPPY_BLOCK in comp_bytes; a context takes such an index after
    kafka_set_codecs(("lz4", "snappy"))."""
    src = _u8(data)
    flags = _index_flags(check_crc, check_control_crc) | (ACCEPT_SNAPPY if accept_snappy else 0)
    info = _lib.YsbKafkaLz4Summary()
    p = src.ctypes.data if src.size else None
    rc = lib().ysb_kafka_index_lz4(p, src.size, flags, None, None, 0, None, 0, C.byref(info))
    if rc not in (0, -4):
        check(rc)
    idx = np.zeros(info.n_batches, dtype=BATCH)
    frames = np.zeros(info.n_batches, dtype=FRAME)
    blocks = np.zeros(info.blocks, dtype=BLOCK)
    if info.n_batches:
        check(lib().ysb_kafka_index_lz4(p, src.size, flags, idx.ctypes.data, frames.ctypes.data, idx.size,
                                        blocks.ctypes.data if blocks.size else None, blocks.size, C.byref(info)))
    return idx, frames, blocks, {k: getattr(info, k) for k, _ in info._fields_}


def unframe_lz4_host(data, idx, frames, blocks, sizes_only=False):
    """ysb_kafka_unframe_lz4_host, the model of the GPU's inflate and unframing: (values, line
    offsets, counters dict with "inflated_bytes").  Raises YsbError (YSB_ERR_FORMAT) for a bad
    batch; `verdict_lz4` returns the verdict (rule 8: a block does not decode) without raising."""
    out, off, ct, vd, rc = _unframe_lz4(data, idx, frames, blocks, sizes_only)
    check(rc)
    return out, off, ct


def verdict_lz4(data, idx, frames, blocks):
    """The compressed model's verdict as a dict: bad_batches, first_bad (None: none), record, rule."""
    return _unframe_lz4(data, idx, frames, blocks, True)[3]


def _unframe_lz4(data, idx, frames, blocks, sizes_only):
    src = _u8(data)
    idx = np.ascontiguousarray(idx, dtype=BATCH)
    frames = np.ascontiguousarray(frames, dtype=FRAME)
    blocks = np.ascontiguousarray(blocks, dtype=BLOCK)
    n, nb, infl = C.c_uint64(), C.c_uint64(), C.c_uint64()
    ct, vd = _lib.YsbKafkaCounters(), _lib.YsbKafkaVerdict()
    p = src.ctypes.data if src.size else None
    ip = idx.ctypes.data if idx.size else None
    fp = frames.ctypes.data if frames.size else None
    bp = blocks.ctypes.data if blocks.size else None

    def call(o, ocap, lo, locap):
        return lib().ysb_kafka_unframe_lz4_host(p, src.size, ip, fp, idx.size, bp, blocks.size, o, ocap, lo, locap,
                                                C.byref(n), C.byref(nb), C.byref(infl), C.byref(ct), C.byref(vd))
    rc = call(None, 0, None, 0)
    out = np.zeros(0, dtype=np.uint8)
    off = np.zeros(0, dtype=np.uint32)
    if rc == 0 and not sizes_only:
        out = np.empty(max(nb.value, 1), dtype=np.uint8)
        off = np.empty(n.value + 1, dtype=np.uint32)
        rc = call(out.ctypes.data, out.size, off.ctypes.data, off.size)
        out = out[:nb.value]
    v = {k: getattr(vd, k) for k, _ in vd._fields_}
    if v["first_bad"] == 0xFFFFFFFF:
        v["first_bad"] = None
    c = {k: getattr(ct, k) for k, _ in ct._fields_}
    c["inflated_bytes"] = infl.value
    return out, off, c, v, rc


def _verdict_dict(vd):
    v = {k: getattr(vd, k) for k, _ in vd._fields_}
    if v["first_bad"] == 0xFFFFFFFF:
        v["first_bad"] = None
    return v


def verdict_crc(data, idx, raises=False):
    """ysb_kafka_verdict_crc_host: the model's verdict when every batch's CRC-32C is checked in
    front of its records (rule 9), as a dict.  raises=True: YsbError for a bad batch, its message
    naming the stored and the computed value."""
    src = _u8(data)
    idx = np.ascontiguousarray(idx, dtype=BATCH)
    vd = _lib.YsbKafkaVerdict()
    rc = lib().ysb_kafka_verdict_crc_host(src.ctypes.data if src.size else None, src.size,
                                          idx.ctypes.data if idx.size else None, idx.size, C.byref(vd))
    if rc != -5 or raises:
        check(rc)
    return _verdict_dict(vd)


def verdict_crc_lz4(data, idx, frames, blocks, raises=False):
    """ysb_kafka_verdict_crc_lz4_host: verdict_crc for batches indexed by index_lz4 (the CRC is
    over the wire bytes and comes in front of the decode: rule 9, not 8)."""
    src = _u8(data)
    idx = np.ascontiguousarray(idx, dtype=BATCH)
    frames = np.ascontiguousarray(frames, dtype=FRAME)
    blocks = np.ascontiguousarray(blocks, dtype=BLOCK)
    vd = _lib.YsbKafkaVerdict()
    rc = lib().ysb_kafka_verdict_crc_lz4_host(src.ctypes.data if src.size else None, src.size,
                                              idx.ctypes.data if idx.size else None, frames.ctypes.data if frames.size else None,
                                              idx.size, blocks.ctypes.data if blocks.size else None, blocks.size, C.byref(vd))
    if rc != -5 or raises:
        check(rc)
    return _verdict_dict(vd)


def unframe_host(data, idx, sizes_only=False):
    """ysb_kafka_unframe_host, the model of the GPU's unframing: (values back to back as a uint8
    array, line offsets with the total as the last entry, counters dict).  Raises YsbError
    (YSB_ERR_FORMAT) for a bad batch; `verdict(data, idx)` returns it without raising."""
    out, off, ct, vd, rc = _unframe(data, idx, sizes_only)
    check(rc)
    return out, off, ct


def verdict(data, idx):
    """The model's verdict as a dict: bad_batches, first_bad (None: none), record, rule."""
    vd = _unframe(data, idx, True)[3]
    return vd


def _unframe(data, idx, sizes_only):
    src = _u8(data)
    idx = np.ascontiguousarray(idx, dtype=BATCH)
    n, nb = C.c_uint64(), C.c_uint64()
    ct, vd = _lib.YsbKafkaCounters(), _lib.YsbKafkaVerdict()
    p = src.ctypes.data if src.size else None
    ip = idx.ctypes.data if idx.size else None
    rc = lib().ysb_kafka_unframe_host(p, src.size, ip, idx.size, None, 0, None, 0, C.byref(n), C.byref(nb), C.byref(ct),
                                      C.byref(vd))
    out = np.zeros(0, dtype=np.uint8)
    off = np.zeros(0, dtype=np.uint32)
    if rc == 0 and not sizes_only:
        out = np.empty(max(nb.value, 1), dtype=np.uint8)
        off = np.empty(n.value + 1, dtype=np.uint32)
        rc = lib().ysb_kafka_unframe_host(p, src.size, ip, idx.size, out.ctypes.data, out.size, off.ctypes.data, off.size,
                                          C.byref(n), C.byref(nb), C.byref(ct), C.byref(vd))
        out = out[:nb.value]
    v = {k: getattr(vd, k) for k, _ in vd._fields_}
    if v["first_bad"] == 0xFFFFFFFF:
        v["first_bad"] = None
    return out, off, {k: getattr(ct, k) for k, _ in ct._fields_}, v, rc


def inflate_bounds(data, idx, frames, blocks):
    """ysb_kafka_inflate_bounds: per batch what the capacity rule of the compressed submits counts
    (a snappy block its preamble's raw size, every other block 65536), an int64 array."""
    src = _u8(data)
    idx = np.ascontiguousarray(idx, dtype=BATCH)
    frames = np.ascontiguousarray(frames, dtype=FRAME)
    blocks = np.ascontiguousarray(blocks, dtype=BLOCK)
    out = np.zeros(idx.size, dtype=np.uint64)
    check(lib().ysb_kafka_inflate_bounds(src.ctypes.data if src.size else None, src.size, idx.ctypes.data if idx.size else None,
                                         frames.ctypes.data if frames.size else None, idx.size,
                                         blocks.ctypes.data if blocks.size else None, blocks.size,
                                         out.ctypes.data if out.size else None))
    return out.astype(np.int64)


def snappy_compress_block(data):
    """ysb_snappy_compress_block: 1..65536 bytes as one raw snappy block (preamble included) by the
    host compressor; a uint8 array."""
    src = _u8(data)
    dst = np.empty(32 + src.size + src.size // 6, dtype=np.uint8)
    n = C.c_uint32()
    check(lib().ysb_snappy_compress_block(src.ctypes.data if src.size else None, src.size, dst.ctypes.data, dst.size, C.byref(n)))
    return dst[:n.value]


def snappy_decompress_block(data):
    """ysb_snappy_decompress_block, the model of the GPU's decoder: the block's raw bytes as a
    uint8 array; YsbError (YSB_ERR_FORMAT) for a block that breaks the format's rules."""
    src = _u8(data)
    dst = np.empty(65536, dtype=np.uint8)
    n = C.c_uint32()
    check(lib().ysb_snappy_decompress_block(src.ctypes.data if src.size else None, src.size, dst.ctypes.data, dst.size, C.byref(n)))
    return dst[:n.value]


class _Opts:
    """ysb_kafka_pack_opts with the arrays it points to kept alive."""

    def __init__(self, n_lines, batch_bytes, batch_records, base_offset, base_timestamp, keys, ts_delta, headers,
                 codec=None, snappy_framing="xerial", snappy_chunk=0):
        o = self.o = _lib.YsbKafkaPackOpts()
        if codec not in (None, "none", "lz4", "snappy"):
            raise ValueError("codec %r: None, \"lz4\" or \"snappy\"" % (codec,))
        if snappy_framing not in ("xerial", "raw"):
            raise ValueError("snappy_framing %r: \"xerial\" or \"raw\"" % (snappy_framing,))
        o.codec = CODEC_LZ4 if codec == "lz4" else CODEC_SNAPPY if codec == "snappy" else 0
        o.snappy_framing, o.snappy_chunk = int(snappy_framing == "raw"), int(snappy_chunk or 0)
        o.batch_bytes, o.batch_records = int(batch_bytes or 0), int(batch_records or 0)
        o.base_offset, o.base_timestamp = int(base_offset), int(base_timestamp)
        self.keep = []
        if keys is not None:
            if len(keys) != n_lines:
                raise ValueError("one key per line")
            koff = np.zeros(n_lines + 1, dtype=np.uint32)
            koff[1:] = np.cumsum([len(k) for k in keys])
            kb = np.frombuffer(b"".join(bytes(k) for k in keys) + b"\0", dtype=np.uint8)
            self.keep += [koff, kb]
            o.key_off, o.keys = koff.ctypes.data, kb.ctypes.data
        if ts_delta is not None:
            ts = np.ascontiguousarray(ts_delta, dtype=np.int64)
            if ts.size != n_lines:
                raise ValueError("one timestamp delta per line")
            self.keep.append(ts)
            o.ts_delta = ts.ctypes.data
        if headers:
            n = len(headers)
            hk = (C.c_char_p * n)(*[bytes(k) for k, _ in headers])
            hv = (C.c_char_p * n)(*[None if v is None else bytes(v) for _, v in headers])
            hl = (C.c_int32 * n)(*[-1 if v is None else len(v) for _, v in headers])
            self.keep += [hk, hv, hl]
            o.n_headers, o.header_keys, o.header_vals, o.header_val_len = n, hk, hv, hl


def _lines(data, offsets):
    return _u8(data), np.ascontiguousarray(offsets, dtype=np.uint32)


def pack(data, offsets, batch_bytes=DEFAULT_BATCH, batch_records=0, base_offset=0, base_timestamp=0, keys=None,
         ts_delta=None, headers=None, codec=None, snappy_framing="xerial", snappy_chunk=0):
    """ysb_kafka_pack: the lines data[offsets[i]:offsets[i + 1]] (the last one ends at len(data))
    as record batches of at most batch_bytes bytes (uncompressed) or batch_records records; a
    uint8 array.  codec="lz4": each batch's records as one standard LZ4 frame (attributes 3).
    codec="snappy" (attributes 2): as the Java client's xerial stream of chunks of snappy_chunk raw
    bytes (0: its 32 KiB), or with snappy_framing="raw" as one raw block (batch_bytes at most 64 KiB).
    keys: None (null keys) or one bytes per line; ts_delta: None or one int per line; headers: a
    list of (key bytes, value bytes or None) put on every record."""
    src, off = _lines(data, offsets)
    o = _Opts(off.size, batch_bytes, batch_records, base_offset, base_timestamp, keys, ts_delta, headers, codec,
              snappy_framing, snappy_chunk)
    dst = np.empty(max(lib().ysb_kafka_bound(src.size, off.size, C.byref(o.o)), 1), dtype=np.uint8)
    n, nb = C.c_uint64(), C.c_uint64()
    check(lib().ysb_kafka_pack(src.ctypes.data if src.size else None, src.size, off.ctypes.data if off.size else None,
                               off.size, C.byref(o.o), dst.ctypes.data, dst.size, C.byref(n), C.byref(nb)))
    return dst[:n.value]


def write_file(path, data, offsets, **kw):
    """ysb_kafka_write_file: `pack` into a file -- a partition's .log segment (what ysb_gen
    --kafka writes and ysb_topology --kafka reads)."""
    src, off = _lines(data, offsets)
    o = _Opts(off.size, kw.pop("batch_bytes", DEFAULT_BATCH), kw.pop("batch_records", 0), kw.pop("base_offset", 0),
              kw.pop("base_timestamp", 0), kw.pop("keys", None), kw.pop("ts_delta", None), kw.pop("headers", None),
              kw.pop("codec", None), kw.pop("snappy_framing", "xerial"), kw.pop("snappy_chunk", 0))
    if kw:
        raise TypeError("unknown options %s" % sorted(kw))
    check(lib().ysb_kafka_write_file(str(path).encode(), src.ctypes.data if src.size else None, src.size,
                                     off.ctypes.data if off.size else None, off.size, C.byref(o.o)))
