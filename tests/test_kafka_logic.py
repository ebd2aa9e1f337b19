"""CPU: the Kafka record batch rules (csrc/ysb_kafka.h: the record reader the kernels share, the
index, the host unframer, CRC-32C, the packer) -- as a stand-alone native program,
tests/native/kafka_logic.cpp, plain and under the host sanitizers, and through the C ABI's host
entries against the pure-Python model tests/kafka_model.py, in both directions.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import golden_data as gd
import kafka_model as M
from test_capi import ROOT, run_native
from ysb_amd import YsbError, kafka

FIXTURES = ["gen_s7", "edge", "edge_orgjson", "edge_long"]
PER_BATCH = [1, 63, 64, 65, 1000]


def lines_of(stem):
    raw, offs = gd.events(stem)
    ends = list(offs[1:]) + [len(raw)]
    return raw, offs, [raw[a:b] for a, b in zip(offs, ends)]


def model_index_as_array(idx):
    a = np.zeros(len(idx), dtype=kafka.BATCH)
    for i, b in enumerate(idx):
        for k, v in b.items():
            a[i][k] = v
    return a


def test_kafka_logic_native(tmp_path):
    """Vectors (CRC-32C, zigzag, the 5- and 10-byte varint limits, a non-minimal varint), round
    trips of the four fixtures at 1, 63, 64, 65 and 1000 records per batch with keys, headers and
    timestamp deltas, the malformed corpus (one case per rule, each cut at every byte) through the
    model and through the kernel's order of work, and the index's rules."""
    run_native(tmp_path, "kafka_logic")


def test_kafka_logic_native_sanitized(tmp_path):
    """The same program with -fsanitize=address,undefined, as a stand-alone program: the shared
    reader and the host model over the malformed corpus in exact-size heap buffers.  This is the
    gate of the GPU malformed-input test."""
    exe = tmp_path / "kafka_logic_san"
    inc = [a for d in (("streaming-benchmarks_amd", "csrc"), ("include",)) for a in ("-I", os.path.join(ROOT, *d))]
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
                   + inc + [os.path.join(ROOT, "tests", "native", "kafka_logic.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK") and not r.stderr, r.stdout + r.stderr


def test_model_corpus_is_the_native_corpus(tmp_path):
    """The Python malformed corpus (what the GPU test feeds the kernels) is byte for byte the one
    the native program walks under the sanitizers."""
    exe = tmp_path / "kafka_logic"
    inc = [a for d in (("streaming-benchmarks_amd", "csrc"), ("include",)) for a in ("-I", os.path.join(ROOT, *d))]
    subprocess.run(["g++", "-O1", "-std=c++17"] + inc + [os.path.join(ROOT, "tests", "native", "kafka_logic.cpp"), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe), "--corpus"], capture_output=True, text=True, check=True).stdout.splitlines()
    native = [(n, int(r), int(c), bytes.fromhex(h)) for n, r, c, h in (l.split("|") for l in out)]
    assert native == [(n, M.RULE[r], c, b) for n, r, c, b in M.malformed_corpus()] and len(native) == 15


def test_known_vectors():
    assert kafka.crc32c(b"123456789") == 0xE3069283 == M.crc32c(b"123456789") == M.crc32c_fast(b"123456789")
    assert [M.zigzag(v) for v in (0, -1, 1, -2)] == [0, 1, 2, 3]
    assert M.uvarint(300) == b"\xac\x02"
    assert len(M.varint(2**31 - 1)) == 5 and len(M.varint(-2**31)) == 5 and len(M.varlong(-2**63)) == 10
    assert M.read_varint(M.varint(-2**31), 0, 5) == (-2**31, 5)
    assert M.read_varint(M.varlong(-2**63), 0, 10, 10, 64) == (-2**63, 10)
    assert M.read_varint(b"\x80\x00", 0, 2) == (0, 2)                      # non-minimal: legal
    with pytest.raises(M.BadVarint):
        M.read_varint(b"\x80\x80\x80\x80\x80\x00", 0, 6)                   # six bytes: illegal
    with pytest.raises(M.BadVarint):
        M.read_varint(b"\x80" * 10 + b"\x00", 0, 11, 10, 64)
    # the library's reader on the same vectors, through a record whose value length is non-minimal
    blob = M.pack_batch([M.Record(b"abc", pad=1, length_pad=1)])
    idx, _ = kafka.index(blob, check_crc=True)
    out, off, ct = kafka.unframe_host(blob, idx)
    assert out.tobytes() == b"abc" and list(off) == [0, 3]
    blob = M.pack_batch([M.Record(b"abc", length_pad=4)])                  # a length of five bytes
    assert kafka.unframe_host(blob, kafka.index(blob)[0])[0].tobytes() == b"abc"
    blob = M.pack_batch([M.Record(b"abc", length_pad=5)])                  # ... of six
    assert kafka.verdict(blob, kafka.index(blob)[0]) == dict(bad_batches=1, first_bad=0, record=0, rule=M.RULE["varint"])


@pytest.mark.parametrize("stem", FIXTURES)
@pytest.mark.parametrize("per_batch", PER_BATCH)
def test_model_packed_host_unframed(stem, per_batch):
    raw, offs, lines = lines_of(stem)
    blob = M.pack(lines, per_batch, base_offset=77, key=b"user-1", headers=[(b"h", b"v"), (b"n", None)], ts_delta=-9)
    idx, info = kafka.index(blob, check_crc=True)
    midx, minfo = M.index(blob, check_crc=True)
    assert info["consumed"] == len(blob) == minfo["consumed"] and info["n_records"] == len(lines)
    assert [{k: int(b[k]) for k in m} for b, m in zip(idx, midx)] == midx
    out, off, ct = kafka.unframe_host(blob, idx)
    mout, moff, mct = M.unframe(blob, midx)
    assert out.tobytes() == raw == mout and list(off) == list(offs) + [len(raw)] == moff
    assert ct == mct and ct["keyed"] == len(lines) and ct["headers"] == 2 * len(lines)


@pytest.mark.parametrize("stem", FIXTURES)
@pytest.mark.parametrize("per_batch", PER_BATCH)
def test_host_packed_model_unframed(stem, per_batch):
    raw, offs, lines = lines_of(stem)
    keys = [b"k" * (i % 5) for i in range(len(lines))]
    blob = kafka.pack(raw, offs, batch_bytes=0, batch_records=per_batch, base_offset=5, base_timestamp=10**12, keys=keys,
                      ts_delta=np.arange(len(lines)) * 7 - 3, headers=[(b"trace", b"\x00\x01"), (b"n", None)]).tobytes()
    midx, minfo = M.index(blob, check_crc=True)      # (the CRC, offsets and counts a consumer checks)
    assert minfo["consumed"] == len(blob) and minfo["n_records"] == len(lines)
    assert [b["base_offset"] for b in midx] == [5 + b["first_record"] for b in midx]
    mout, moff, mct = M.unframe(blob, midx)
    assert mout == raw and moff == list(offs) + [len(raw)] and mct["keyed"] == len(lines)
    # lastOffsetDelta and each record's offsetDelta
    import struct
    for b in midx:
        last, = struct.unpack_from(">i", blob, b["records_off"] - 61 + 23)
        assert last == b["n_records"] - 1
    # a target size in bytes: no batch above it unless it is one record
    blob = kafka.pack(raw, offs, batch_bytes=4096).tobytes()
    midx, _ = M.index(blob)
    assert all(b["records_bytes"] + 61 <= 4096 or b["n_records"] == 1 for b in midx) and M.unframe(blob, midx)[0] == raw


def test_record_shapes_both_ways():
    """Keys null / empty / 1 / 36 / 300 bytes, headers 0 / 1 / 3 with a null value, negative and
    10-byte timestamp deltas, offset-delta gaps, null and empty values, values whose record
    length takes 1, 2 and 3 bytes."""
    recs = []
    for i, vlen in enumerate((20, 254, 9000, 0, None, 5000)):
        for key in (None, b"", b"k", b"u" * 36, b"K" * 300):
            for headers in ((), ((b"a", b"1"),), ((b"a", b"1"), (b"b", None), (b"", b""))):
                value = None if vlen is None else bytes((i + j) % 251 for j in range(vlen))
                recs.append(M.Record(value, key=key, headers=headers, ts_delta=(-1, -2**63, 2**62, 5)[len(recs) % 4],
                                     offset_delta=3 * len(recs)))
    blob = b"".join(M.pack_batch(recs[i:i + 7], base_offset=i) for i in range(0, len(recs), 7))
    idx, _ = kafka.index(blob, check_crc=True)
    out, off, ct = kafka.unframe_host(blob, idx)
    mout, moff, mct = M.unframe(blob, M.index(blob)[0])
    assert out.tobytes() == mout and list(off) == moff and ct == mct
    assert ct["null_values"] == 15 and ct["records"] == len(recs) == 90


def test_malformed_model_and_host_agree():
    """One case per rule, each also cut at every byte: the model and the host unframer give the
    same verdict (batch, record, rule), with a good batch in front."""
    front = M.pack_batch([M.Record(b"ok")])
    n = 0
    for name, rule, count, rec in M.malformed_corpus():
        for cut in [len(rec)] + list(range(len(rec))):
            blob = front + M.pack_batch(None, records_count=count, raw_records=rec[:cut])
            idx, _ = kafka.index(blob, check_crc=True)
            want = M.verdict(blob, M.index(blob)[0])
            got = kafka.verdict(blob, idx)
            if want is None:
                assert got["bad_batches"] == 0 and got["first_bad"] is None, (name, cut)
            else:
                assert (got["first_bad"], got["record"], got["rule"]) == want and want[0] == 1, (name, cut, got, want)
            if cut == len(rec):
                assert want is not None and want[2] == M.RULE[rule], (name, want)
                with pytest.raises(YsbError) as e:
                    kafka.unframe_host(blob, idx)
                assert e.value.code == -5 and "Kafka batch 1 " in str(e.value) and "record %d" % want[1] in str(e.value)
            n += 1
    assert n > 400


def test_index_rules():
    raw, offs, lines = lines_of("gen_s7")
    blob = M.pack(lines[:39], 13)
    idx, info = kafka.index(blob)
    assert info["n_batches"] == 3 and info["control_batches"] == 0
    assert kafka.index(b"")[1]["consumed"] == 0 and kafka.index(b"")[0].size == 0
    last = int(idx[2]["records_off"]) - 61
    for cut in range(last, len(blob)):                      # a fetch response's partial tail
        i2, s2 = kafka.index(blob[:cut], check_crc=True)
        assert s2["consumed"] == last and s2["n_batches"] == 2 == i2.size and M.index(blob[:cut])[1]["consumed"] == last
    at = int(idx[1]["records_off"]) - 61
    for pos, val, field in ((16, 1, "magic = 1"), (16, 0, "magic = 0"), (22, 3, "codec = 3"), (22, 1, "codec = 1"),
                            (57, 0x80, "recordsCount = -")):
        bad = bytearray(blob)
        bad[at + pos] = val
        with pytest.raises(YsbError) as e:
            kafka.index(bytes(bad))
        assert e.value.code == -5 and field in str(e.value) and "at byte %d" % at in str(e.value), str(e.value)
        with pytest.raises(M.Refusal) as me:
            M.index(bytes(bad))
        assert me.value.offset == at
    bad = bytearray(blob)
    bad[at + 8:at + 12] = (48).to_bytes(4, "big")
    with pytest.raises(YsbError) as e:
        kafka.index(bytes(bad))
    assert "batchLength = 48" in str(e.value)
    # CRC on and off, one flipped bit
    bad = bytearray(blob)
    bad[-1] ^= 0x10
    assert kafka.index(bytes(bad))[1]["n_batches"] == 3
    with pytest.raises(YsbError) as e:
        kafka.index(bytes(bad), check_crc=True)
    assert e.value.code == -5 and "crc" in str(e.value) and "at byte %d" % last in str(e.value)
    assert kafka.index(blob, check_crc=True)[1]["crc_checked"] == 3
    # a control batch in the middle: skipped and counted
    ctl = M.pack_batch([M.Record(b"\x00\x00\x00\x00", key=b"\x00\x00\x00\x01")], attributes=0x20)
    mixed = blob[:at] + ctl + blob[at:]
    i3, s3 = kafka.index(mixed, check_crc=True)
    assert s3["n_batches"] == 3 and s3["control_batches"] == 1 and list(i3["control_before"]) == [0, 1, 0]
    assert list(i3["first_record"]) == [0, 13, 26] and M.index(mixed)[1]["control_batches"] == 1
    assert kafka.unframe_host(mixed, i3)[0].tobytes() == b"".join(lines[:39])


def test_unframe_argument_errors():
    blob = M.pack([b"abc", b"de"], 1)
    idx, _ = kafka.index(blob)
    bad = idx.copy()
    bad[1]["first_record"] = 5
    with pytest.raises(YsbError) as e:
        kafka.unframe_host(blob, bad)
    assert e.value.code == -1
    bad = idx.copy()
    bad[1]["records_bytes"] += 1
    with pytest.raises(YsbError) as e:
        kafka.unframe_host(blob, bad)
    assert e.value.code == -1
