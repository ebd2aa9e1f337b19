"""CPU: the LZ4 batch rules (csrc/ysb_lz4.h: the sequence reader the kernel shares, the host
decoder, the compressor) -- as a stand-alone native program, tests/native/lz4_logic.cpp, plain
and under the host sanitizers, and through the C ABI's host entries against the pure-Python
model tests/lz4_model.py, the system's liblz4 and the committed liblz4 fixtures.  No GPU."""
import ctypes
import os
import subprocess

import pytest

import lz4_model as M
from test_capi import ROOT, run_native
from ysb_amd import YsbError, lz4

GOLD = os.path.join(ROOT, "tests", "golden")


def read(name):
    with open(os.path.join(GOLD, name), "rb") as f:
        return f.read()


def host_valid(comp, field, raw):
    try:
        return lz4.decompress_block(comp, field, raw)
    except YsbError as e:
        assert e.code == -5, e
        return None


def test_lz4_logic_native(tmp_path):
    """Round trips of gen_s7.jsonl / .tbl at block sizes 1, 13, 64, 4096, 65536 (and line-aligned),
    65536 equal bytes, the periods around the copy widths, random bytes stored and literal-only,
    empty input; the hand-assembled blocks; the malformed corpus cut at every byte; the
    directory's rules; the kernel's in-place window on every block decoded."""
    run_native(tmp_path, "lz4_logic")


def test_lz4_logic_native_sanitized(tmp_path):
    """The same program with -fsanitize=address,undefined, as a stand-alone program: the shared
    reader and the host decoder over the malformed corpus in exact-size heap buffers.  This is
    the gate of the GPU malformed-input test."""
    exe = tmp_path / "lz4_logic_san"
    inc = [a for d in (("streaming-benchmarks_amd", "csrc"), ("include",)) for a in ("-I", os.path.join(ROOT, *d))]
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
                   + inc + [os.path.join(ROOT, "tests", "native", "lz4_logic.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK") and not r.stderr, r.stdout + r.stderr


def test_hand_blocks_model_and_host():
    for name, comp, raw in M.hand_blocks():
        assert M.decode_block(comp, len(raw)) == raw, name
        assert host_valid(comp, len(comp), len(raw)) == raw, name


def test_malformed_model_and_host_agree():
    """One case per rule, each cut at every byte position: the model and the host decoder agree
    on valid / invalid, and on a batch's first bad block."""
    cases = M.malformed_blocks()
    assert len(cases) > 500
    for name, comp, raw in cases:
        want = M.is_valid(comp, raw)
        got = host_valid(comp, len(comp), raw)
        assert (got is not None) == want, name
    for name, comp, raw in M.malformed_bases():
        assert not M.is_valid(comp, raw), name
    # stored blocks hold exactly raw_bytes bytes
    assert host_valid(b"abc", 3 | M.STORED, 3) == b"abc" and M.decode_entry(b"abc", 3 | M.STORED, 3) == b"abc"
    assert host_valid(b"abc", 3 | M.STORED, 4) is None and not M.is_valid(b"abc", 4, stored=True)


@pytest.mark.parametrize("name", ["gen_s7.jsonl", "gen_s7.tbl"])
@pytest.mark.parametrize("block,aligned", [(13, False), (64, True), (4096, False), (16384, True), (65536, True)])
def test_pack_round_trip_through_the_model(name, block, aligned):
    data = read(name)
    if block < 64:
        data = data[:20000]
    blob, d = lz4.pack(data, block, aligned, threads=3)
    directory = [(int(c), int(r)) for c, r in d]
    assert sum(c & ~M.STORED for c, _ in directory) == blob.size
    out, bad, ranges = M.decode_batch(blob.tobytes(), directory)
    assert bad == M.NO_BAD and out == data
    if aligned and block >= 4096:   # every block but the last ends on a line terminator (a line is far below such a block)
        assert all(data[e - 1:e] in (b"\n", b"\r") for _, e in ranges[:-1])
    assert all(1 <= r <= block for _, r in directory)


def test_pack_special_inputs():
    blob, d = lz4.pack(b"", 4096)
    assert blob.size == 0 and d.shape == (0, 2)
    same = bytes([0x61]) * 65536
    comp, (field, raw) = lz4.compress_block(same)
    assert len(comp) < 300 and comp.count(255) >= 250 and M.decode_block(comp, 65536) == same
    for period in (2, 3, 7, 15, 16, 17, 63, 64, 65):
        p = M.periodic(period)
        comp, (field, raw) = lz4.compress_block(p)
        assert not field & M.STORED and M.decode_block(comp, 65536) == p, period
    rnd = M.random_bytes(65536)
    comp, (field, raw) = lz4.compress_block(rnd)
    assert field == 65536 | M.STORED and comp == rnd
    comp, (field, raw) = lz4.compress_block(rnd, allow_stored=False)
    assert not field & M.STORED and len(comp) > 65536 and M.decode_block(comp, 65536) == rnd
    assert host_valid(comp, field, raw) == rnd


def _liblz4():
    try:
        L = ctypes.CDLL("liblz4.so.1")
    except OSError:
        pytest.skip("the system has no liblz4.so.1")
    return L


def test_cross_check_with_liblz4():
    L = _liblz4()
    for name in ("gen_s7.jsonl", "gen_s7.tbl"):
        data = read(name)
        for block in (64, 4096, 65536):
            for at in range(0, min(len(data), 4 * 65536), block):
                src = data[at:at + block]
                # ours -> LZ4_decompress_safe
                comp, (field, raw) = lz4.compress_block(src, allow_stored=False)
                dst = ctypes.create_string_buffer(len(src))
                assert L.LZ4_decompress_safe(comp, dst, len(comp), len(src)) == len(src)
                assert dst.raw == src
                # LZ4_compress_default -> ours
                cap = L.LZ4_compressBound(len(src))
                cb = ctypes.create_string_buffer(cap)
                n = L.LZ4_compress_default(src, cb, len(src), cap)
                assert n > 0 and host_valid(cb.raw[:n], n, len(src)) == src
                assert M.decode_block(cb.raw[:n], len(src)) == src


@pytest.mark.parametrize("fixture", ["gen_s7_64k.default.lz4", "gen_s7_64k.hc.lz4"])
def test_liblz4_fixtures(fixture):
    comp = read(os.path.join("lz4", fixture))
    want = read("gen_s7.jsonl")[:65536]
    assert M.decode_block(comp, 65536) == want
    assert host_valid(comp, len(comp), 65536) == want
    assert host_valid(comp[:-1], len(comp) - 1, 65536) is None and not M.is_valid(comp[:-1], 65536)


def test_fixtures_are_small():
    d = os.path.join(GOLD, "lz4")
    assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) < 100_000
