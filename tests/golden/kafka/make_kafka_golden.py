"""Writes the compressed Kafka segment fixture beside this script: record batches (message format
v2) over the lines of ../gen_s7.jsonl whose records sections the system's liblz4 compressed
(LZ4F_compressBegin / Update / End through ctypes, independent 64 KiB blocks as librdkafka asks and
as the Java client's KafkaLZ4BlockOutputStream writes).  Data only; the library version is recorded
in versions.txt.  No Kafka library exists where the tests run, so parity with a broker's own bytes
stays unpinned: the batch headers are tests/kafka_model.py's.

  segment.kafka   batch 0   20 lines, liblz4's default level
                batch 1   20 lines, HC level 9
                batch 2   10 lines, block checksums, a content checksum and the content size
                batch 3   the next lines up to 140,000 record bytes: three blocks, records
                          straddle both block edges
                batch 4   15 lines, uncompressed (codec 0)
                          a control batch
                batch 5   5 lines, the default level

Run from anywhere: python tests/golden/kafka/make_kafka_golden.py"""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import kafka_model as K   # noqa: E402


class FrameInfo(ctypes.Structure):
    _fields_ = [("blockSizeID", ctypes.c_int), ("blockMode", ctypes.c_int), ("contentChecksumFlag", ctypes.c_int),
                ("frameType", ctypes.c_int), ("contentSize", ctypes.c_ulonglong), ("dictID", ctypes.c_uint),
                ("blockChecksumFlag", ctypes.c_int)]


class Preferences(ctypes.Structure):
    _fields_ = [("frameInfo", FrameInfo), ("compressionLevel", ctypes.c_int), ("autoFlush", ctypes.c_uint),
                ("favorDecSpeed", ctypes.c_uint), ("reserved", ctypes.c_uint * 3)]


def liblz4():
    L = ctypes.CDLL("liblz4.so.1")
    L.LZ4_versionString.restype = ctypes.c_char_p
    for fn in (L.LZ4F_compressBound, L.LZ4F_compressBegin, L.LZ4F_compressUpdate, L.LZ4F_compressEnd,
               L.LZ4F_createCompressionContext, L.LZ4F_freeCompressionContext):
        fn.restype = ctypes.c_size_t
    L.LZ4F_compressBound.argtypes = [ctypes.c_size_t, ctypes.POINTER(Preferences)]
    L.LZ4F_createCompressionContext.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
    L.LZ4F_freeCompressionContext.argtypes = [ctypes.c_void_p]
    L.LZ4F_compressBegin.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(Preferences)]
    L.LZ4F_compressUpdate.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                                      ctypes.c_void_p]
    L.LZ4F_compressEnd.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.LZ4F_isError.argtypes = [ctypes.c_size_t]
    return L


def frame(L, src, level=0, flags=False):
    """src as one frame: independent blocks, 64 KiB block maximum (the streaming entry points:
    LZ4F_compressFrame rewrites the block maximum and mode of a source that fits one block)."""
    p = Preferences()
    p.frameInfo.blockSizeID = 4
    p.frameInfo.blockMode = 1
    p.frameInfo.contentChecksumFlag = int(flags)
    p.frameInfo.blockChecksumFlag = int(flags)
    p.frameInfo.contentSize = len(src) if flags else 0
    p.compressionLevel = level
    ctx = ctypes.c_void_p()
    assert not L.LZ4F_isError(L.LZ4F_createCompressionContext(ctypes.byref(ctx), 100))
    dst = ctypes.create_string_buffer(L.LZ4F_compressBound(len(src), ctypes.byref(p)) + 64)
    n = L.LZ4F_compressBegin(ctx, dst, len(dst), ctypes.byref(p))
    assert not L.LZ4F_isError(n)
    for a in range(0, len(src), 65536):
        k = L.LZ4F_compressUpdate(ctx, ctypes.byref(dst, n), len(dst) - n, src[a:a + 65536], len(src[a:a + 65536]), None)
        assert not L.LZ4F_isError(k)
        n += k
    k = L.LZ4F_compressEnd(ctx, ctypes.byref(dst, n), len(dst) - n, None)
    assert not L.LZ4F_isError(k)
    L.LZ4F_freeCompressionContext(ctx)
    return dst.raw[:n + k]


def main():
    L = liblz4()
    with open(os.path.join(HERE, "..", "gen_s7.jsonl"), "rb") as f:
        lines = f.read().split(b"\n")[:-1]
    out, at = bytearray(), 0

    def take(n):
        nonlocal at
        recs = [K.Record(v) for v in lines[at:at + n]]
        at += n
        return recs

    def compressed(recs, **kw):
        body = K.pack_batch(recs)[K.HEADER:]
        return K.pack_batch(None, base_offset=at - len(recs), attributes=3, records_count=len(recs),
                            raw_records=frame(L, body, **kw)), body

    out += compressed(take(20))[0]
    out += compressed(take(20), level=9)[0]
    out += compressed(take(10), flags=True)[0]
    n = 0
    while len(K.pack_batch([K.Record(v) for v in lines[at:at + n + 1]])) - K.HEADER <= 140000:
        n += 1
    big, body = compressed(take(n))
    assert 131072 < len(body) <= 140000
    out += big
    recs = take(15)
    out += K.pack_batch(recs, base_offset=at - 15)
    out += K.pack_batch([K.Record(b"\0\0\0\0", key=b"\0\0\0\1")], base_offset=at, attributes=0x20)
    out += compressed(take(5))[0]
    with open(os.path.join(HERE, "segment.kafka"), "wb") as f:
        f.write(out)
    with open(os.path.join(HERE, "versions.txt"), "w") as f:
        f.write("liblz4 %s\nlines %d\nbig_batch_records %d\nbig_batch_record_bytes %d\n"
                % (L.LZ4_versionString().decode(), at, n, len(body)))
    print("segment.kafka: %d bytes, %d lines" % (len(out), at))


if __name__ == "__main__":
    main()
