"""CPU: the rules of snappy blocks and of snappy-compressed Kafka record batches (csrc/ysb_snappy.h,
the codec-2 parts of csrc/ysb_kafka_lz4.h) -- as a stand-alone native program,
tests/native/snappy_logic.cpp, plain and under the host sanitizers; through the C ABI's host
entries against the pure-Python model tests/snappy_model.py, in both directions; and against the
real snappy: the committed blocks that pyarrow's bundled snappy compressed (tests/golden/snappy)
and, where pyarrow imports, its decoder over what the host compressor writes.
No GPU.  No Kafka client exists where the tests run: a producer's own xerial bytes stay unpinned
(the framing around pyarrow's blocks is the fixture maker's)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import kafka_lz4_model as Z
import kafka_model as K
import snappy_model as S
from test_capi import ROOT, run_native
from test_kafka_logic import lines_of
from ysb_amd import YsbError, kafka

GOLDEN = os.path.join(ROOT, "tests", "golden", "snappy")


def test_snappy_logic_native(tmp_path):
    """The readers, the host decoder over every malformed block and every cut, the compressor's
    round trip (all three copy forms, overlapping copies, its bound), the xerial index and every
    refusal with its byte, the opt-in at the index and the entries, the host model, the packer."""
    run_native(tmp_path, "snappy_logic")


def test_snappy_logic_native_sanitized(tmp_path):
    """The same program with -fsanitize=address,undefined, as a stand-alone program: the index and
    the decoder over cut and malformed input in exact-size heap buffers.  This is the gate of the
    GPU malformed-input tests."""
    exe = tmp_path / "snappy_logic_san"
    inc = [a for d in (("streaming-benchmarks_amd", "csrc"), ("include",)) for a in ("-I", os.path.join(ROOT, *d))]
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
                   + inc + [os.path.join(ROOT, "tests", "native", "snappy_logic.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK") and not r.stderr, r.stdout + r.stderr


def index_both(blob, check_crc=True):
    idx, fr, bl, info = kafka.index_lz4(blob, check_crc=check_crc, accept_snappy=True)
    mi, mf, mb, minfo = S.index(blob, check_crc)
    assert [tuple(x) for x in fr] == mf and [(int(o), int(w)) for o, w, _ in bl] == mb
    for i, b in enumerate(mi):
        for k, v in b.items():
            assert int(idx[i][k]) == v, (i, k)
    for k, v in minfo.items():
        assert info[k] == v, k
    return (idx, fr, bl, info), (mi, mf, mb)


def test_model_decodes_its_own_forms():
    d8 = b"abcdefgh"
    assert S.preamble(5, 1) == b"\x85\x00" and S.read_preamble(b"\x85\x00") == (5, 2)
    assert S.decode_block(S.preamble(8, 2) + S.literal(d8, 4)) == d8
    assert S.decode_block(S.preamble(12) + S.literal(d8) + S.copy2(4, 3)) == b"abcdefghfghf"
    assert S.decode_block(S.preamble(12) + S.literal(d8) + S.copy4(4, 1)) == b"abcdefghhhhh"
    run = S.preamble(65) + S.literal(b"z") + S.copy2(64, 1)
    assert run == bytes([65, 0, ord("z"), 0xFE, 1, 0]) and S.decode_block(run) == b"z" * 65
    for name, block, rule in S.malformed_blocks():
        with pytest.raises(S.Bad) as e:
            S.decode_block(block)
        assert e.value.rule == rule, name
        with pytest.raises(YsbError) as e:
            kafka.snappy_decompress_block(block)
        assert e.value.code == -5, name


@pytest.mark.parametrize("stem", ["gen_s7", "edge", "edge_long"])
@pytest.mark.parametrize("form", ["xerial", "xerial-100", "raw", "literal"])
def test_model_packs_library_reads(stem, form):
    """Batches the model compressed (its own greedy compressor, or literal-only blocks; xerial
    chunks of 32 KiB and of 100 bytes, so that records straddle chunks; one raw block): the
    library's index equals the model's and its host model unframes the lines."""
    raw, offs, lines = lines_of(stem)
    kw = dict(framing="raw") if form == "raw" else dict(chunk=100) if form == "xerial-100" else \
        dict(compress=S.compress_literal, chunk=4096) if form == "literal" else {}
    per = 150 if form == "raw" else 200
    if stem == "edge_long" and form == "raw":
        lines = [l for l in lines if len(l) < 60000]       # one raw block holds 64 KiB of records at the most
        per = 1
    blob = S.pack(lines, per, **kw)
    (idx, fr, bl, info), (mi, mf, mb) = index_both(blob)
    assert info["compressed_batches"] == idx.size and all(int(w) & S.SNAPPY_BLOCK for _, w, _ in bl)
    out, off, ct = kafka.unframe_lz4_host(blob, idx, fr, bl)
    mout, moff, mct, mv = S.unframe(blob, mi, mf, mb)
    assert mv is None and out.tobytes() == mout == b"".join(lines) and list(off) == moff
    assert {k: ct[k] for k in mct} == mct


@pytest.mark.parametrize("kw", [dict(), dict(snappy_chunk=1, batch_bytes=2000), dict(snappy_chunk=100),
                                dict(snappy_framing="raw"), dict(batch_bytes=200000), dict(batch_bytes=200000, snappy_chunk=65536)])
def test_library_packs_model_reads(kw):
    """pack(codec="snappy"): the model reads it (every CRC over the wire bytes, attributes 2, the
    xerial header and chunks or one raw block); batches close by their uncompressed size; without
    the flag the index still refuses the batch by name."""
    raw, offs, lines = lines_of("gen_s7")
    data = b"".join(lines)
    off = np.cumsum([0] + [len(l) for l in lines[:-1]]).astype(np.uint32)
    if kw.get("snappy_chunk") == 1:
        data, off, lines = data[:int(off[100])], off[:100], lines[:100]
    blob = kafka.pack(data, off, base_offset=77, codec="snappy", **kw).tobytes()
    plain = kafka.pack(data, off, base_offset=77, **{k: v for k, v in kw.items() if k == "batch_bytes"}).tobytes()
    (idx, fr, bl, info), (mi, mf, mb) = index_both(blob)
    pidx, _ = kafka.index(plain)
    assert list(idx["n_records"]) == list(pidx["n_records"]) and list(idx["base_offset"]) == list(pidx["base_offset"])
    assert info["compressed_batches"] == idx.size and all(c == 2 for _, _, c in mf)
    assert S.unframe(blob, mi, mf, mb)[0] == data
    first = blob[int(idx[0]["records_off"]):][:8]
    assert (first == S.XERIAL_MAGIC) == (kw.get("snappy_framing") != "raw")
    if kw.get("snappy_chunk") == 100:
        assert info["blocks"] > 10 * idx.size
    if kw == dict(batch_bytes=200000):
        assert max(n for _, n, _ in mf) == 7 and len(blob) < 0.6 * len(plain)      # 32 KiB chunks of about 198 KB
    for refuses in (lambda: kafka.index_lz4(blob), lambda: kafka.index(blob)):
        with pytest.raises(YsbError) as e:
            refuses()
        assert "attributes.codec = 2" in str(e.value) and e.value.code == -5
    with pytest.raises(YsbError) as e:
        kafka.index_lz4(blob)
    assert "Kafka batch 0 at byte 0: attributes.codec = 2: snappy-compressed record batches are not read" in str(e.value)


def test_pack_refuses_what_one_raw_block_cannot_hold():
    raw, offs, lines = lines_of("gen_s7")
    data = b"".join(lines)
    off = np.cumsum([0] + [len(l) for l in lines[:-1]]).astype(np.uint32)
    with pytest.raises(YsbError) as e:
        kafka.pack(data, off, batch_bytes=100000, codec="snappy", snappy_framing="raw")
    assert e.value.code == -1 and "1..65536 bytes" in str(e.value)
    with pytest.raises(ValueError):
        kafka.pack(data, off, codec="snappy", snappy_framing="framed")
    with pytest.raises(YsbError):
        kafka.pack(data, off, codec="snappy", snappy_chunk=65537)


def refusal(blob):
    with pytest.raises(YsbError) as e:
        kafka.index_lz4(blob, accept_snappy=True)
    with pytest.raises(Z.Refusal) as m:
        S.index(blob)
    assert e.value.code == -5
    return str(e.value), m.value


def test_refusals_name_the_batch_the_byte_the_chunk_and_the_rule():
    good = S.pack_batch([K.Record(b"ok")])
    a = S.compress_greedy(b"abcd" * 200)
    big = S.preamble(65537) + S.literal(b"x")
    cases = [
        ("a compatible version of 2", S.xerial_of_chunks([a], compat=2), 12, "compatible version", ("compatible version 2", "only 1")),
        ("a chunk length of 0", S.XERIAL_MAGIC + struct.pack(">iii", 1, 1, 0), 16, "chunk length not positive", ("chunk length 0",)),
        ("a negative chunk length", S.XERIAL_MAGIC + struct.pack(">iii", 1, 1, -7) + a, 16, "chunk length not positive", ("chunk length -7",)),
        ("a chunk past the records", S.XERIAL_MAGIC + struct.pack(">iii", 1, 1, len(a) + 1) + a, 16, "chunk length past the section",
         ("chunk length %d runs past the records section" % (len(a) + 1),)),
        ("trailing bytes", S.xerial_of_chunks([a]) + b"\0\0", 20 + len(a), "trailing bytes", ("2 trailing bytes", "length word")),
        ("a cut header", S.XERIAL_MAGIC + b"\0\0\0\1", 8, "header cut", ("header is cut",)),
        ("a raw block above 64 KiB", big, 0, "raw size", ("a raw block of 65537 bytes", "Java client's framing", "batch.size of at most 64 KiB")),
        ("the same inside a chunk", S.xerial_of_chunks([a, big]), 24 + len(a), "raw size", ("a raw block of 65537 bytes",)),
        ("a raw size of 0", S.preamble(0), 0, "raw size", ("a raw block of 0 bytes",)),
        ("a 6-byte preamble", bytes([0x88, 0x80, 0x80, 0x80, 0x80, 0x00]) + a, 0, "preamble", ("not a varint of at most 5 bytes",)),
        ("a preamble of 2^32", bytes([0x80, 0x80, 0x80, 0x80, 0x10]) + a, 0, "preamble", ("below 2^32",)),
    ]
    for name, section, at, mrule, words in cases:
        blob = good + S.pack_batch(None, base_offset=1, section=section, records_count=2) + good
        msg, m = refusal(blob)
        assert "Kafka batch 1 at byte %d:" % len(good) in msg and "attributes.codec = 2" in msg, (name, msg)
        assert "%d bytes at byte %d," % (len(section), len(good) + K.HEADER) in msg and "snappy: byte %d:" % at in msg, (name, msg)
        assert m.offset == len(good) and m.frame_at == at and m.rule == mrule and all(w in msg for w in words), (name, msg, m.rule)
    for codec, word in ((1, "gzip"), (4, "zstd")):
        blob = good + K.pack_batch([K.Record(b"v")], base_offset=1, attributes=codec)
        msg, m = refusal(blob)
        assert "Kafka batch 1 at byte %d: attributes.codec = %d: %s-compressed" % (len(good), codec, word) in msg
    from ysb_amd import _lib
    with pytest.raises(YsbError) as e:
        _lib.check(_lib.lib().ysb_kafka_index_lz4(None, 0, 0x200, None, None, 0, None, 0, None))
    assert e.value.code == -1 and "unknown flags" in str(e.value)


def test_verdicts_equal_the_model():
    """Every malformed block of the model's corpus inside a xerial chunk of the middle batch (rule
    8, the smallest bad block of the smallest bad batch), next to a bad record in another batch in
    both orders, and with the CRC checked first (rule 9 for a flipped wire byte)."""
    good = [S.pack_batch([K.Record(b"v%d" % i)], base_offset=i) for i in range(8)]
    ok = S.compress_greedy(Z.records_bytes([K.Record(b"abc")]))
    calls = []
    for i, (name, block, _rule) in enumerate(S.malformed_blocks()):
        section = S.xerial_of_chunks([ok] * (i % 3) + [block] + [ok])
        # (the index refuses the blocks whose preamble it would refuse: those go in hand-made entries on the GPU)
        try:
            S.section_index(section)
        except S.SectionRefusal:
            continue
        calls.append(good[0] + S.pack_batch(None, base_offset=1, section=section, records_count=1) + good[2])
    assert len(calls) >= 13
    corpus = K.malformed_corpus()
    bad_rec = S.pack_batch(None, base_offset=100, section=S.xerial(corpus[8][3], chunk=16), records_count=corpus[8][2])
    bad_blk = S.pack_batch(None, base_offset=200, records_count=1, section=S.xerial_of_chunks([ok, S.preamble(9) + S.literal(b"xy")]))
    for a, b in ((bad_rec, bad_blk), (bad_blk, bad_rec)):
        calls.append(b"".join(good[:2]) + a + b"".join(good[2:4]) + b + good[4])
    seen = set()
    for blob in calls:
        idx, fr, bl, _ = kafka.index_lz4(blob, check_crc=True, accept_snappy=True)
        mi, mf, mb, _ = S.index(blob, True)
        mv = S.unframe(blob, mi, mf, mb)[3]
        hv = kafka.verdict_lz4(blob, idx, fr, bl)
        assert mv is not None and (hv["bad_batches"], hv["first_bad"], hv["record"], hv["rule"]) == mv
        with pytest.raises(YsbError) as e:
            kafka.unframe_lz4_host(blob, idx, fr, bl)
        assert e.value.code == -5 and ("block %d" if mv[3] == 8 else "record %d") % mv[2] in str(e.value)
        seen.add(mv[3])
    assert 8 in seen and len(seen) >= 2
    blob = bytearray(calls[0])
    idx, fr, bl, _ = kafka.index_lz4(bytes(blob), accept_snappy=True)
    blob[int(idx[1]["records_off"]) + 3] ^= 0x10
    v = kafka.verdict_crc_lz4(bytes(blob), idx, fr, bl)
    assert (v["first_bad"], v["rule"]) == (1, 9)


def _golden(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


@pytest.mark.parametrize("name,block", [("gen_s7_128k.b64k.xerial", 65536), ("gen_s7_128k.b32k.xerial", 32768)])
def test_golden_blocks_of_the_real_snappy(name, block):
    """The committed blocks that pyarrow's bundled snappy compressed: the host decoder (through a
    codec-2 batch around the stream) and the model reproduce the bytes."""
    meta = dict(l.split() for l in open(os.path.join(GOLDEN, "versions.txt")).read().splitlines())
    want = open(os.path.join(ROOT, "tests", "golden", "gen_s7.jsonl"), "rb").read()[:int(meta["raw_bytes"])]
    section = _golden(name)
    chunks = S.section_index(section)
    assert len(chunks) == len(want) // block
    assert b"".join(S.decode_block(section[o:o + n]) for o, n in chunks) == want
    assert b"".join(kafka.snappy_decompress_block(section[o:o + n]).tobytes() for o, n in chunks) == want
    # the stream as a codec-2 batch's records section: the library's index finds pyarrow's blocks
    blob = K.pack_batch(None, attributes=2, records_count=0, raw_records=section)
    idx, fr, bl, info = kafka.index_lz4(blob, check_crc=True, accept_snappy=True)
    assert info["blocks"] == len(chunks) and [int(o) - K.HEADER for o, _, _ in bl] == [o for o, _ in chunks]


def test_golden_folder_stays_small():
    total = sum(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN))
    assert total < 150_000


def test_pyarrow_decodes_what_the_host_compressor_writes():
    pa = pytest.importorskip("pyarrow")
    raw, offs, lines = lines_of("gen_s7")
    data = b"".join(lines)
    off = np.cumsum([0] + [len(l) for l in lines[:-1]]).astype(np.uint32)
    for kw in (dict(batch_bytes=200000, snappy_chunk=65536), dict(), dict(snappy_framing="raw"), dict(snappy_chunk=333)):
        blob = kafka.pack(data, off, codec="snappy", **kw).tobytes()
        plain = kafka.pack(data, off, **{k: v for k, v in kw.items() if k == "batch_bytes"}).tobytes()
        idx, fr, bl, _ = kafka.index_lz4(blob, accept_snappy=True)
        pidx, _ = kafka.index(plain)
        got = bytearray()
        for o, w, _ in bl:
            z = blob[int(o):int(o) + (int(w) & S.LEN_MASK)]
            got += pa.decompress(z, decompressed_size=S.block_raw(z), codec="snappy", asbytes=True)
        want = b"".join(plain[int(b["records_off"]):int(b["records_off"]) + int(b["records_bytes"])] for b in pidx)
        assert bytes(got) == want
    # and the real codec accepts a non-minimal preamble, as the reader here does
    z = S.preamble(5, 1) + S.literal(b"hello")
    assert pa.decompress(z, decompressed_size=5, codec="snappy", asbytes=True) == b"hello" == S.decode_block(z)
    assert kafka.snappy_decompress_block(z).tobytes() == b"hello"
    for raw in (b"x", data[:65536], bytes(1000), np.random.RandomState(7).bytes(65536)):
        z = kafka.snappy_compress_block(raw).tobytes()
        assert pa.decompress(z, decompressed_size=len(raw), codec="snappy", asbytes=True) == raw == S.decode_block(z)
        assert kafka.snappy_decompress_block(pa.compress(raw, codec="snappy", asbytes=True)).tobytes() == raw
