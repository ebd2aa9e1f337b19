"""CPU: CRC-32C of Kafka record batches as the GPU verifies it (csrc/ysb_kafka_crc.h) -- the
arithmetic and the 64-lane decomposition as a stand-alone native program,
tests/native/kafka_crc_logic.cpp, plain and under the host sanitizers; rule 9 in the host models
through the C ABI (ysb_kafka_verdict_crc_host / _lz4_host) against tests/kafka_model.py, whose
bitwise crc32c is the independent reference; the index's flag for control batches.  No GPU.

A single flipped bit is always detected by a 32-bit CRC, so no case here depends on luck."""
import os
import subprocess

import numpy as np
import pytest

import golden_data as gd
import kafka_model as M
from test_capi import ROOT, run_native
from ysb_amd import YsbError, kafka

RULE_CRC = 9


def test_kafka_crc_logic_native(tmp_path):
    """Vectors (empty, "123456789", 32 zero and 32 0xFF bytes, the RFC 3720 iSCSI ones), mulmod and
    the powers of x against the bitwise definition, reg(A || B) for every split of 300 bytes, the
    tables' entries, the sliced host CRC against the byte loop, the lanes over every length 0..2200
    at every residue mod 16 and 65535, 65536, 65537 and 1 MiB + 3 at residues 0, 1, 15."""
    run_native(tmp_path, "kafka_crc_logic")


def test_kafka_crc_logic_native_sanitized(tmp_path):
    """The same program with -fsanitize=address,undefined, as a stand-alone program: every range in
    a heap block of exactly the 16-byte vectors the decomposition may read."""
    exe = tmp_path / "kafka_crc_logic_san"
    inc = [a for d in (("streaming-benchmarks_amd", "csrc"), ("include",)) for a in ("-I", os.path.join(ROOT, *d))]
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
                   + inc + [os.path.join(ROOT, "tests", "native", "kafka_crc_logic.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK") and not r.stderr, r.stdout + r.stderr


def test_library_crc_equals_the_bitwise_model():
    rng = np.random.default_rng(5)
    data = rng.integers(0, 256, 3000, dtype=np.uint8).tobytes()
    for n in list(range(0, 70)) + [255, 256, 257, 1023, 1024, 1025, 3000]:
        assert kafka.crc32c(data[:n]) == M.crc32c(data[:n]), n
    assert kafka.crc32c(b"123456789") == 0xE3069283 and kafka.crc32c(b"") == 0


def lines_of(stem):
    raw, offs = gd.events(stem)
    ends = list(offs[1:]) + [len(raw)]
    return [raw[a:b] for a, b in zip(offs, ends)]


def five_batches():
    """Five batches of 20 gen_s7 lines, the index, and batch 3's place."""
    blob = M.pack(lines_of("gen_s7")[:100], 20, base_offset=1000)
    idx, info = kafka.index(blob, check_crc=True)
    assert info["n_batches"] == 5
    return blob, idx


def flip(blob, at, bit=0x04):
    b = bytearray(blob)
    b[at] ^= bit
    return bytes(b)


def batch_start(idx, k):
    return int(idx[k]["records_off"]) - M.HEADER


def batch_end(idx, k):
    return int(idx[k]["records_off"]) + int(idx[k]["records_bytes"])


# where a flipped bit must give rule 9, as an offset from the batch's start (negative: from its end)
COVERED = {"attributes": 21, "last byte": -1, "stored crc": 17}
# ... and where it must not: the CRC does not cover bytes 0..20 (partitionLeaderEpoch is bytes 12..15)
UNCOVERED = {"baseOffset": 7, "batchLength's neighbour": 12, "magic's neighbour": 15}


def place(idx, k, where):
    return batch_start(idx, k) + where if where >= 0 else batch_end(idx, k) + where


@pytest.mark.parametrize("name", sorted(COVERED))
def test_flip_inside_the_range_is_rule_9(name):
    blob, idx = five_batches()
    at = place(idx, 3, COVERED[name])
    bad = flip(blob, at)      # (`attributes`: its high byte, the range's first; no codec or control bit lies there)
    bidx, _ = kafka.index(bad)
    assert bidx.size == 5 and (bidx["records_off"] == idx["records_off"]).all()
    assert kafka.verdict_crc(bad, bidx) == dict(bad_batches=1, first_bad=3, record=0, rule=RULE_CRC)
    # the model: exactly batch 3's CRC differs
    s, e = batch_start(bidx, 3), batch_end(bidx, 3)
    stored, computed = int.from_bytes(bad[s + 17:s + 21], "big"), M.crc32c(bad[s + 21:e])
    assert stored != computed
    assert [M.crc32c(bad[batch_start(bidx, k) + 21:batch_end(bidx, k)]) ==
            int.from_bytes(bad[batch_start(bidx, k) + 17:batch_start(bidx, k) + 21], "big") for k in range(5)] == \
        [True, True, True, False, True]
    with pytest.raises(YsbError) as e_:
        kafka.verdict_crc(bad, bidx, raises=True)
    msg = str(e_.value)
    assert e_.value.code == -5 and "Kafka batch 3 (baseOffset 1060)" in msg, msg
    assert "stored %08x, computed %08x" % (stored, computed) in msg and "changed between the producer and here" in msg, msg
    # without the check the walk decides alone (only a flip inside the records can trouble it)
    if name == "stored crc":
        assert kafka.verdict(bad, bidx)["bad_batches"] == 0


@pytest.mark.parametrize("name", sorted(UNCOVERED))
def test_flip_outside_the_range_is_clean(name):
    blob, idx = five_batches()
    bad = flip(blob, place(idx, 3, UNCOVERED[name]), 0x01)
    bidx, _ = kafka.index(bad, check_crc=True)          # the index's own CRC pass agrees: not covered
    assert bidx.size == 5
    assert kafka.verdict_crc(bad, bidx) == dict(bad_batches=0, first_bad=None, record=0, rule=0)
    assert kafka.unframe_host(bad, bidx)[0].tobytes() == kafka.unframe_host(blob, idx)[0].tobytes()


def test_smallest_bad_batch_wins_whichever_kind():
    """A bad record in batch 0 and a bad CRC in batch 3: first_bad 0 with its record rule, two bad
    batches.  Both faults in one batch: rule 9."""
    lines = lines_of("gen_s7")
    name, rule, count, rec = M.malformed_corpus()[8]
    front = M.pack_batch(None, base_offset=0, records_count=count, raw_records=rec)   # (its CRC is right)
    rest = M.pack(lines[:80], 20, base_offset=2)
    blob = front + rest
    idx, _ = kafka.index(blob, check_crc=True)
    want = M.verdict(blob, M.index(blob)[0])
    assert want[0] == 0 and want[2] == M.RULE[rule]
    bad = flip(blob, batch_end(idx, 3) - 1)
    v = kafka.verdict_crc(bad, idx)
    assert v == dict(bad_batches=2, first_bad=0, record=want[1], rule=want[2])
    # both in batch 0: the CRC comes first
    both = flip(bad, batch_end(idx, 0) - 1)
    assert kafka.verdict_crc(both, idx) == dict(bad_batches=2, first_bad=0, record=0, rule=RULE_CRC)
    assert kafka.verdict(both, idx)["rule"] != RULE_CRC


def test_entries_without_room_for_the_header_are_an_argument_error():
    blob, idx = five_batches()
    cut = idx.copy()
    cut["records_off"] -= 30          # batch 0's records_off becomes 31: no stored CRC in front of it
    with pytest.raises(YsbError) as e:
        kafka.verdict_crc(blob, cut)
    assert e.value.code == -1 and "44" in str(e.value)


def test_compressed_flip_in_a_block_is_rule_9_not_8():
    raw, offs = gd.events("gen_s7")
    z = kafka.pack(raw, offs, batch_bytes=16384, codec="lz4").tobytes()
    plain = M.pack_batch([M.Record(b'{"a":1}')], base_offset=10**6)   # a codec-0 batch in the same response
    blob = z + plain
    idx, frames, blocks, info = kafka.index_lz4(blob, check_crc=True)
    assert info["compressed_batches"] == idx.size - 1 >= 2
    assert kafka.verdict_crc_lz4(blob, idx, frames, blocks) == dict(bad_batches=0, first_bad=None, record=0, rule=0)
    # a flip in a block's token bytes that the decoder refuses: rule 8 without the check, 9 with it
    k = 1
    b0 = int(frames[k]["first_block"])
    found = None
    for at in range(int(blocks[b0]["offset"]), int(blocks[b0]["offset"]) + 64):
        for bit in (0x80, 0x40, 0x10):
            cand = flip(blob, at, bit)
            if kafka.verdict_lz4(cand, idx, frames, blocks)["rule"] == 8:
                found = cand
                break
        if found:
            break
    assert found is not None, "no flip in the block's first 64 bytes makes it undecodable"
    assert kafka.verdict_lz4(found, idx, frames, blocks)["first_bad"] == k
    assert kafka.verdict_crc_lz4(found, idx, frames, blocks) == dict(bad_batches=1, first_bad=k, record=0, rule=RULE_CRC)
    # the codec-0 batch's last byte
    tail = flip(blob, len(blob) - 1)
    assert kafka.verdict_crc_lz4(tail, idx, frames, blocks)["first_bad"] == idx.size - 1


def test_index_flag_for_control_batches():
    lines = lines_of("gen_s7")
    blob = M.pack(lines[:39], 13)
    idx, _ = kafka.index(blob)
    at = batch_start(idx, 1)
    ctl = M.pack_batch([M.Record(b"\x00\x00\x00\x00", key=b"\x00\x00\x00\x01")], attributes=0x20)
    mixed = blob[:at] + ctl + blob[at:]
    i0, s0 = kafka.index(mixed, check_control_crc=True)
    assert s0["control_batches"] == 1 and s0["crc_checked"] == 1 and i0.size == 3
    assert kafka.index(mixed, check_crc=True, check_control_crc=True)[1]["crc_checked"] == 4
    assert kafka.index(mixed)[1]["crc_checked"] == 0
    bad = flip(mixed, at + len(ctl) - 1)                   # the control batch's last byte
    assert kafka.index(bad)[1]["control_batches"] == 1     # passed over without the flag
    with pytest.raises(YsbError) as e:
        kafka.index(bad, check_control_crc=True)
    assert e.value.code == -5 and "crc" in str(e.value) and "at byte %d" % at in str(e.value)
    # a flipped DATA batch is not this flag's: the device verifies those
    dbad = flip(mixed, len(mixed) - 1)
    assert kafka.index(dbad, check_control_crc=True)[1]["crc_checked"] == 1
    # the compressed index takes the same flag
    assert kafka.index_lz4(mixed, check_control_crc=True)[3]["crc_checked"] == 1
    with pytest.raises(YsbError):
        kafka.index_lz4(bad, check_control_crc=True)
    assert kafka.index_lz4(bad)[3]["control_batches"] == 1
