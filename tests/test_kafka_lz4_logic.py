"""CPU: the rules of LZ4-compressed Kafka record batches (csrc/ysb_kafka_lz4.h: the index that
accepts codec 0 and 3, the host model, the packer) -- as a stand-alone native program,
tests/native/kafka_lz4_logic.cpp, plain and under the host sanitizers; through the C ABI's host
entries against the pure-Python model tests/kafka_lz4_model.py, in both directions; against the
system's liblz4 where there is one; and over the committed liblz4 fixture tests/golden/kafka.
No GPU.  No Kafka library exists where the tests run: parity with a broker's own bytes stays
unpinned (the batch headers are the models')."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import golden_data as gd
import kafka_lz4_model as Z
import kafka_model as K
import lz4_model as L
from test_capi import ROOT, run_native
from test_kafka_logic import lines_of
from ysb_amd import YsbError, kafka

GOLDEN = os.path.join(ROOT, "tests", "golden", "kafka")


def test_kafka_lz4_logic_native(tmp_path):
    """The index over hand-built compressed batches (one block, several, a stored block inside a
    frame, every optional frame flag, an empty frame with recordsCount 0, a compressed batch next to
    an uncompressed and a control batch), every refusal with its byte, every buffer cut at every
    byte, the malformed record corpus inside good frames (rules 1-7 as uncompressed), bad blocks
    (rule 8) with a bad record in another batch in both orders, the packer's round trip."""
    run_native(tmp_path, "kafka_lz4_logic")


def test_kafka_lz4_logic_native_sanitized(tmp_path):
    """The same program with -fsanitize=address,undefined, as a stand-alone program: the index and
    the host model over cut and malformed input in exact-size heap buffers.  This is the gate of
    the GPU malformed-input tests."""
    exe = tmp_path / "kafka_lz4_logic_san"
    inc = [a for d in (("streaming-benchmarks_amd", "csrc"), ("include",)) for a in ("-I", os.path.join(ROOT, *d))]
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
                   + inc + [os.path.join(ROOT, "tests", "native", "kafka_lz4_logic.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK") and not r.stderr, r.stdout + r.stderr


def test_xxh32_vectors():
    assert Z.xxh32(b"") == 0x02CC5D05 and Z.xxh32(b"a") == 0x550D7456 and Z.xxh32(b"abc") == 0x32D153FF
    assert Z.xxh32(b"Nobody inspects the spammish repetition") == 0xE2293B2F


def same_index(blob, check_crc=True):
    idx, fr, bl, info = kafka.index_lz4(blob, check_crc=check_crc)
    mi, mf, mb, minfo = Z.index(blob, check_crc)
    assert [tuple(x) for x in fr] == mf and [(int(o), int(w)) for o, w, _ in bl] == mb
    for i, b in enumerate(mi):
        for k, v in b.items():
            assert int(idx[i][k]) == v, (i, k)
    for k, v in minfo.items():
        assert info[k] == v, k
    return (idx, fr, bl, info), (mi, mf, mb)


@pytest.mark.parametrize("stem", ["gen_s7", "edge", "edge_long"])
@pytest.mark.parametrize("compress", ["greedy", "literal"])
def test_model_packs_library_reads(stem, compress):
    """Batches the model compressed (its own greedy compressor, or literal-only blocks) with keys
    and headers: the library's index equals the model's and its host model unframes the lines."""
    raw, offs, lines = lines_of(stem)
    comp = Z.compress_greedy if compress == "greedy" else Z.compress_literal
    blob = Z.pack(lines, 200, key=b"k", headers=[(b"h", None)],
                  frame_opts=dict(compress=comp, allow_stored=False, block_bytes=20000, flags=compress == "literal"))
    (idx, fr, bl, info), (mi, mf, mb) = same_index(blob)
    assert info["compressed_batches"] == idx.size and (info["blocks"] > idx.size or stem == "edge")
    out, off, ct = kafka.unframe_lz4_host(blob, idx, fr, bl)
    mout, moff, mct, mv = Z.unframe(blob, mi, mf, mb)
    assert mv is None and out.tobytes() == mout == b"".join(lines) and list(off) == moff
    assert {k: ct[k] for k in mct} == mct and ct["headers"] == len(lines) == ct["keyed"]


@pytest.mark.parametrize("batch_bytes", [1, 4096, 16384, 200000])
def test_library_packs_model_reads(batch_bytes):
    """pack(codec="lz4"): the model reads it (every CRC over the wire bytes, attributes 3, one
    standard frame per batch, 64 KiB blocks); batches close by their uncompressed size."""
    raw, offs, lines = lines_of("gen_s7")
    data = b"".join(lines)
    off = np.cumsum([0] + [len(l) for l in lines[:-1]]).astype(np.uint32)
    data, off, lines = (data[:int(off[200])], off[:200], lines[:200]) if batch_bytes == 1 else (data, off, lines)
    blob = kafka.pack(data, off, batch_bytes=batch_bytes, base_offset=77, codec="lz4").tobytes()
    plain = kafka.pack(data, off, batch_bytes=batch_bytes, base_offset=77).tobytes()
    (idx, fr, bl, info), (mi, mf, mb) = same_index(blob)
    pidx, _ = kafka.index(plain)
    assert list(idx["n_records"]) == list(pidx["n_records"]) and list(idx["base_offset"]) == list(pidx["base_offset"])
    assert info["compressed_batches"] == idx.size and [b["base_offset"] for b in mi] == [77 + b["first_record"] for b in mi]
    assert Z.unframe(blob, mi, mf, mb)[0] == data
    if batch_bytes == 200000:
        assert max(n for _, n, _ in mf) >= 3 and len(blob) < 0.6 * len(plain)
    with pytest.raises(YsbError) as e:
        kafka.index(blob)
    assert "attributes.codec = 3" in str(e.value) and "codec 0 only" in str(e.value)


def test_pack_refuses_other_codecs():
    from ysb_amd import _lib
    o = _lib.YsbKafkaPackOpts()
    o.codec = 1
    n = ctypes.c_uint64()
    dst = np.zeros(4096, dtype=np.uint8)
    off = np.zeros(1, dtype=np.uint32)
    rc = _lib.lib().ysb_kafka_pack(dst.ctypes.data, 4, off.ctypes.data, 1, ctypes.byref(o), dst.ctypes.data, dst.size, ctypes.byref(n), None)
    assert rc == -1
    with pytest.raises(ValueError):
        kafka.pack(b"ab", [0], codec="gzip")


def refusal(blob):
    with pytest.raises(YsbError) as e:
        kafka.index_lz4(blob)
    with pytest.raises(Z.Refusal) as m:
        Z.index(blob)
    assert e.value.code == -5
    return str(e.value), m.value


def test_refusals_name_the_batch_the_byte_and_the_rule():
    good = Z.pack_batch([K.Record(b"ok")])
    recs = Z.records_bytes([K.Record(b"x" * 100), K.Record(b"y" * 50)])
    blocks = [(Z.compress_greedy(recs), False)]

    def hdr_frame(**kw):
        return Z.frame_of_blocks(blocks, **kw)

    linked = bytearray(hdr_frame())
    linked[4] &= ~0x20 & 0xFF
    linked[6] = (Z.xxh32(bytes(linked[4:6])) >> 8) & 0xFF
    bad_hc = bytearray(hdr_frame())
    bad_hc[6] ^= 0x40
    cut = hdr_frame()[:-9]
    cases = [
        ("linked", bytes(linked), "linked", ("LZ4F_blockIndependent",)),
        ("a 256 KiB block maximum", hdr_frame(bd=0x50), "block maximum", ("LZ4F_max64KB",)),
        ("a dictionary id", hdr_frame(flg_extra=1), "dictionary", ("dictionar",)),
        ("a bad header checksum", bytes(bad_hc), "checksum", ("header checksum",)),
        ("truncation inside the records", cut, "truncated", ("the buffer ends",)),
        ("bytes behind the last frame", hdr_frame() + b"junk!", "magic", ("not an LZ4 frame magic",)),
    ]
    for name, fb, mrule, words in cases:
        blob = good + Z.pack_batch(None, base_offset=1, frame_bytes=fb, records_count=2) + good
        msg, m = refusal(blob)
        assert "Kafka batch 1 at byte %d:" % len(good) in msg and "attributes.codec = 3" in msg, (name, msg)
        assert "at byte %d," % (len(good) + K.HEADER) in msg and "LZ4 frame: byte %d:" % m.frame_at in msg, (name, msg)
        assert m.offset == len(good) and m.rule == mrule and all(w in msg for w in words), (name, msg, m.rule)
    for codec, word in ((1, "gzip"), (2, "snappy"), (4, "zstd")):
        blob = good + K.pack_batch([K.Record(b"v")], base_offset=1, attributes=codec)
        msg, m = refusal(blob)
        assert "Kafka batch 1 at byte %d: attributes.codec = %d: %s-compressed" % (len(good), codec, word) in msg
        assert m.rule == word and m.offset == len(good)


def test_verdicts_equal_the_model():
    """Bad blocks (rule 8, the smallest bad block of the smallest bad batch), the record corpus in
    good frames, and both kinds in one call in both orders: the library's verdict is the model's."""
    good = [Z.pack_batch([K.Record(b"v%d" % i)], base_offset=i) for i in range(8)]
    calls = []
    for i, (name, comp, _raw) in enumerate(L.malformed_bases()):
        if comp and len(comp) <= Z.BLOCK_MAX:
            fb = Z.frame_of_blocks([(Z.compress_literal(b"abc"), False)] * (i % 3) + [(comp, False)] + [(b"zz", True)])
            calls.append(good[0] + Z.pack_batch(None, base_offset=1, frame_bytes=fb, records_count=1) + good[2])
    corpus = K.malformed_corpus()
    for name, rule, count, rec in corpus:
        calls.append(good[0] + Z.pack_batch(None, base_offset=1, frame_bytes=Z.frame(rec, block_bytes=16), records_count=count))
    bad_rec = Z.pack_batch(None, base_offset=100, frame_bytes=Z.frame(corpus[8][3]), records_count=corpus[8][2])
    bad_blk = Z.pack_batch(None, base_offset=200, records_count=1, frame_bytes=Z.frame_of_blocks(
        [(Z.compress_literal(b"xy"), False), (bytes([0x40, 1, 2, 3, 4, 0, 0, 0]), False)]))
    for a, b in ((bad_rec, bad_blk), (bad_blk, bad_rec)):
        calls.append(b"".join(good[:2]) + a + b"".join(good[2:4]) + b + good[4])
    seen = set()
    for blob in calls:
        idx, fr, bl, _ = kafka.index_lz4(blob, check_crc=True)
        mi, mf, mb, _ = Z.index(blob, True)
        mv = Z.unframe(blob, mi, mf, mb)[3]
        hv = kafka.verdict_lz4(blob, idx, fr, bl)
        assert mv is not None and (hv["bad_batches"], hv["first_bad"], hv["record"], hv["rule"]) == mv
        with pytest.raises(YsbError) as e:
            kafka.unframe_lz4_host(blob, idx, fr, bl)
        assert e.value.code == -5 and ("block %d" if mv[3] == 8 else "record %d") % mv[2] in str(e.value)
        seen.add(mv[3])
    assert seen == set(range(1, 9)) and kafka.RULES[8] == "codec"


def _liblz4():
    try:
        lib = ctypes.CDLL("liblz4.so.1")
    except OSError:
        pytest.skip("the system has no liblz4.so.1")
    return lib


class _FrameInfo(ctypes.Structure):
    _fields_ = [("blockSizeID", ctypes.c_int), ("blockMode", ctypes.c_int), ("contentChecksumFlag", ctypes.c_int),
                ("frameType", ctypes.c_int), ("contentSize", ctypes.c_ulonglong), ("dictID", ctypes.c_uint),
                ("blockChecksumFlag", ctypes.c_int)]


class _Preferences(ctypes.Structure):
    _fields_ = [("frameInfo", _FrameInfo), ("compressionLevel", ctypes.c_int), ("autoFlush", ctypes.c_uint),
                ("favorDecSpeed", ctypes.c_uint), ("reserved", ctypes.c_uint * 3)]


def test_liblz4_compress_frame_is_indexed_and_unframed():
    """Records compressed by LZ4F_compressFrame with independent 64 KiB blocks, as librdkafka asks:
    indexed and unframed to the input lines."""
    lib = _liblz4()
    lib.LZ4F_compressFrameBound.restype = lib.LZ4F_compressFrame.restype = ctypes.c_size_t
    lib.LZ4F_compressFrameBound.argtypes = [ctypes.c_size_t, ctypes.POINTER(_Preferences)]
    lib.LZ4F_compressFrame.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(_Preferences)]
    lib.LZ4F_isError.argtypes = [ctypes.c_size_t]
    raw, offs, lines = lines_of("gen_s7")
    blob = bytearray()
    for a in range(0, len(lines), 400):       # 400 lines: about 100 KB of records, two blocks
        recs = [K.Record(v) for v in lines[a:a + 400]]
        body = Z.records_bytes(recs)
        p = _Preferences()
        p.frameInfo.blockSizeID, p.frameInfo.blockMode = 4, 1
        dst = ctypes.create_string_buffer(lib.LZ4F_compressFrameBound(len(body), ctypes.byref(p)))
        n = lib.LZ4F_compressFrame(dst, len(dst), body, len(body), ctypes.byref(p))
        assert not lib.LZ4F_isError(n)
        blob += Z.pack_batch(None, base_offset=a, frame_bytes=dst.raw[:n], records_count=len(recs))
    (idx, fr, bl, info), _ = same_index(bytes(blob))
    assert info["compressed_batches"] == idx.size == 4 and info["blocks"] >= 7
    out, off, ct = kafka.unframe_lz4_host(bytes(blob), idx, fr, bl)
    assert out.tobytes() == b"".join(lines) and ct["records"] == len(lines)


def test_liblz4_decompresses_what_pack_wrote():
    lib = _liblz4()
    lib.LZ4F_createDecompressionContext.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
    lib.LZ4F_createDecompressionContext.restype = ctypes.c_size_t
    lib.LZ4F_freeDecompressionContext.argtypes = [ctypes.c_void_p]
    lib.LZ4F_decompress.restype = ctypes.c_size_t
    lib.LZ4F_decompress.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t), ctypes.c_void_p,
                                    ctypes.POINTER(ctypes.c_size_t), ctypes.c_void_p]
    lib.LZ4F_isError.argtypes = [ctypes.c_size_t]
    raw, offs, lines = lines_of("gen_s7")
    data = b"".join(lines)
    off = np.cumsum([0] + [len(l) for l in lines[:-1]]).astype(np.uint32)
    blob = kafka.pack(data, off, batch_bytes=150000, codec="lz4")
    plain = kafka.pack(data, off, batch_bytes=150000).tobytes()
    idx, fr, bl, _ = kafka.index_lz4(blob)
    pidx, _ = kafka.index(plain)
    for b, pb in zip(idx, pidx):
        dctx = ctypes.c_void_p()
        assert not lib.LZ4F_isError(lib.LZ4F_createDecompressionContext(ctypes.byref(dctx), 100))
        dst = ctypes.create_string_buffer(int(pb["records_bytes"]) + 16)
        n_dst, n_src = ctypes.c_size_t(len(dst)), ctypes.c_size_t(int(b["records_bytes"]))
        rc = lib.LZ4F_decompress(dctx, dst, ctypes.byref(n_dst), blob.ctypes.data + int(b["records_off"]), ctypes.byref(n_src), None)
        lib.LZ4F_freeDecompressionContext(dctx)
        assert rc == 0 and n_src.value == int(b["records_bytes"])       # complete, every wire byte consumed
        assert dst.raw[:n_dst.value] == plain[int(pb["records_off"]):int(pb["records_off"]) + int(pb["records_bytes"])]


def test_golden_segment():
    """The committed segment that liblz4 compressed (tests/golden/kafka/make_kafka_golden.py):
    default and HC levels, every optional frame flag, a batch of three blocks whose records
    straddle both block edges, an uncompressed batch and a control batch."""
    with open(os.path.join(GOLDEN, "segment.kafka"), "rb") as f:
        blob = f.read()
    meta = dict(l.split() for l in open(os.path.join(GOLDEN, "versions.txt")).read().splitlines())
    raw, offs, lines = lines_of("gen_s7")
    lines = [l.rstrip(b"\n") for l in lines][:int(meta["lines"])]
    (idx, fr, bl, info), (mi, mf, mb) = same_index(blob)
    assert [tuple(x)[1:] for x in fr] == [(1, 3), (1, 3), (1, 3), (3, 3), (1, 0), (1, 3)]
    assert info["control_batches"] == 1 and idx[5]["control_before"] == 1 and info["consumed"] == len(blob)
    assert blob[int(idx[2]["records_off"]) + 4] == 0x40 | 0x20 | 0x10 | 0x08 | 0x04
    out, off, ct = kafka.unframe_lz4_host(blob, idx, fr, bl)
    assert out.tobytes() == b"".join(lines) and ct["records"] == len(lines) == int(meta["lines"])
    assert ct["inflated_bytes"] > 2 * 65536 + 70 * 254
    assert Z.unframe(blob, mi, mf, mb)[0] == b"".join(lines)
    # records straddle both block edges of the three-block batch
    big = Z.inflate_batch(blob, mf[3], mb)
    assert len(big) == int(meta["big_batch_record_bytes"]) > 131072
    pos, starts = 0, set()
    while pos < len(big):
        starts.add(pos)
        _, pos, _, _ = K._record(big, pos, len(big))
    assert 65536 not in starts and 131072 not in starts


def test_golden_folder_stays_small():
    total = sum(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN))
    assert total < 150_000
