"""CPU: standard LZ4 frames (csrc/ysb_lz4_frame.h: the index and its refusals, XXH32, the frame
writer, the measure model, the carry rule) -- as a stand-alone native program,
tests/native/lz4_frame_logic.cpp, plain and under the host sanitizers, and through the C ABI's
host entries against the pure-Python model tests/lz4_model.py, the system's liblz4 and the
committed liblz4 frame fixtures (tests/golden/lz4frame).  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import lz4_model as M
from test_capi import ROOT, run_native
from ysb_amd import YsbError, lz4

GOLD = os.path.join(ROOT, "tests", "golden")
FRAMES = os.path.join(GOLD, "lz4frame")


def read(*name):
    with open(os.path.join(GOLD, *name), "rb") as f:
        return f.read()


def block_bytes(frame, entry):
    at, n = int(entry["offset"]), int(entry["comp_bytes"]) & ~M.STORED
    return bytes(frame[at:at + n]), int(entry["comp_bytes"])


def decode_frame(frame):
    """Every indexed block measured by the host model and decoded by the Python model."""
    frame = bytes(frame)
    index, info = lz4.frame_index(frame)
    out = b""
    for e in index:
        comp, field = block_bytes(frame, e)
        out += M.decode_entry(comp, field, lz4.measure_block(comp, field))
    return out, index, info


def test_lz4_frame_logic_native(tmp_path):
    """XXH32's known answers; the index over hand-built frames with and without each optional
    field, empty frames, concatenated and skippable frames, a stored block, a short cap; the
    liblz4 fixtures; one case per refusal; a frame cut at every byte; the writer at block sizes
    1 .. 65536; the measure model against the host decoder; the carry rule over streams of 40
    lines in 13-, 64- and 251-byte one-block batches."""
    run_native(tmp_path, "lz4_frame_logic")


def test_lz4_frame_logic_native_sanitized(tmp_path):
    """The same program with -fsanitize=address,undefined, as a stand-alone program: the index
    reads nothing past nbytes of an exact-size heap buffer at any cut, the measure walk nothing
    past a block.  This is the gate of the GPU tests' malformed input."""
    exe = tmp_path / "lz4_frame_logic_san"
    inc = [a for d in (("streaming-benchmarks_amd", "csrc"), ("include",)) for a in ("-I", os.path.join(ROOT, *d))]
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined"] + inc
                   + [os.path.join(ROOT, "tests", "native", "lz4_frame_logic.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK") and not r.stderr, r.stdout + r.stderr


def test_measure_model_against_the_python_model():
    """hand_blocks() and malformed_blocks(400): the measured raw size is the one size with which
    the model decodes the block; a block is valid exactly when the existing host decoder accepts
    it with the measured size."""
    for name, comp, raw in M.hand_blocks():
        assert lz4.measure_block(comp) == len(raw), name
    cases = M.malformed_blocks(400)
    assert len(cases) > 500
    measured = 0
    for name, comp, raw in cases:
        try:
            got = lz4.measure_block(comp)
        except YsbError as e:
            assert e.code == -5, name
            # no raw size makes it valid: in particular not the corpus's
            assert not M.is_valid(comp, raw), name
            continue
        measured += 1
        assert 1 <= got <= M.MAX_RAW and M.is_valid(comp, got), name
        assert lz4.decompress_block(comp, len(comp), got) == M.decode_block(comp, got), name
        assert M.is_valid(comp, raw) == (raw == got), name
        for other in (got - 1, got + 1):
            if 1 <= other <= M.MAX_RAW:
                assert not M.is_valid(comp, other), name
    assert measured >= 10   # (a cut behind a whole sequence's literals is a shorter valid block)
    assert lz4.measure_block(b"abc", 3 | M.STORED) == 3


@pytest.mark.parametrize("block", [1, 13, 64, 251, 4096, 65536])
def test_frame_write_index_decode(tmp_path, block):
    data = read("gen_s7.jsonl")[:2000 if block == 1 else 30000 if block < 4096 else 200000]
    frame = lz4.frame_pack(data, block, threads=3)
    out, index, info = decode_frame(frame)
    assert out == data and index.size == -(-len(data) // block)
    assert info["frames"] == 1 and info["content_sizes"] == 1 and info["content_bytes"] == len(data)
    assert info["block_checksums"] == 0 and info["content_checksums"] == 0
    assert info["comp_bytes"] == int((index["comp_bytes"] & 0x7FFFFFFF).sum())
    path = tmp_path / "x.lz4"
    lz4.frame_write(path, data, block)
    assert path.read_bytes() == frame.tobytes() and lz4.is_frame(frame)


def test_frame_write_stores_what_does_not_shrink():
    rnd = M.random_bytes(70000)
    out, index, info = decode_frame(lz4.frame_pack(rnd))
    assert out == rnd and info["stored_blocks"] == 2 and all(int(c) & M.STORED for c in index["comp_bytes"])
    out, index, info = decode_frame(lz4.frame_pack(b""))
    assert out == b"" and index.size == 0 and info["frames"] == 1


def _liblz4():
    try:
        L = ctypes.CDLL("liblz4.so.1")
    except OSError:
        pytest.skip("the system has no liblz4.so.1")
    L.LZ4F_createDecompressionContext.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
    L.LZ4F_createDecompressionContext.restype = ctypes.c_size_t
    L.LZ4F_freeDecompressionContext.argtypes = [ctypes.c_void_p]
    L.LZ4F_decompress.restype = ctypes.c_size_t
    L.LZ4F_decompress.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t), ctypes.c_void_p,
                                  ctypes.POINTER(ctypes.c_size_t), ctypes.c_void_p]
    L.LZ4F_isError.argtypes = [ctypes.c_size_t]
    return L


@pytest.mark.parametrize("block", [13, 4096, 65536])
def test_liblz4_reads_what_frame_write_wrote(block):
    """frame_write -> LZ4F_decompress -> the input: the frame is a standard one."""
    L = _liblz4()
    data = read("gen_s7.jsonl")[:5000 if block == 13 else 200000] + M.random_bytes(3000)
    frame = lz4.frame_pack(data, block)
    dctx = ctypes.c_void_p()
    assert not L.LZ4F_isError(L.LZ4F_createDecompressionContext(ctypes.byref(dctx), 100))
    dst = ctypes.create_string_buffer(len(data) + 16)
    n_dst, n_src = ctypes.c_size_t(len(dst)), ctypes.c_size_t(frame.size)
    rc = L.LZ4F_decompress(dctx, dst, ctypes.byref(n_dst), frame.ctypes.data, ctypes.byref(n_src), None)
    L.LZ4F_freeDecompressionContext(dctx)
    assert rc == 0 and n_src.value == frame.size   # 0: the frame is complete, every byte consumed
    assert dst.raw[:n_dst.value] == data


def test_liblz4_frame_fixtures():
    lines = read("gen_s7.jsonl")
    out, index, info = decode_frame(read("lz4frame", "gen_s7_150k.lz4"))
    assert index.size == 3 and 2 * 65536 < len(out) <= 150000 and out == lines[:len(out)] and out.endswith(b"\n")
    assert out[65535:65536] != b"\n" and out[131071:131072] != b"\n"   # lines straddle both block edges
    assert [lz4.measure_block(*block_bytes(read("lz4frame", "gen_s7_150k.lz4"), e)) for e in index] == \
        [65536, 65536, len(out) - 131072]
    out, index, info = decode_frame(read("lz4frame", "small_checksums.lz4"))
    assert (info["block_checksums"], info["content_checksums"], info["content_sizes"]) == (1, 1, 1)
    assert info["content_bytes"] == len(out) and out == lines[:len(out)]
    out, index, info = decode_frame(read("lz4frame", "small_skip_two.lz4"))
    assert (info["frames"], info["skippable_frames"], index.size) == (2, 1, 2) and out == lines[:len(out)]
    for name, way_out in (("small_linked.lz4", ("lz4 -BI", "LZ4F_blockIndependent", "block_linked=False")),
                          ("small_b5.lz4", ("-B4",))):
        with pytest.raises(YsbError) as e:
            lz4.frame_index(read("lz4frame", name))
        assert e.value.code == -5 and "byte " in str(e.value) and all(w in str(e.value) for w in way_out), str(e.value)


def test_index_capacity_and_truncation_through_the_abi():
    frame = lz4.frame_pack(read("gen_s7.jsonl")[:1000], 300)
    index, _ = lz4.frame_index(frame)
    assert index.size == 4
    from ysb_amd._lib import lib
    n = ctypes.c_uint64()
    short = np.zeros(2, dtype=lz4.FRAME_BLOCK)
    assert lib().ysb_lz4_frame_index(frame.ctypes.data, frame.size, short.ctypes.data, 2, ctypes.byref(n), None) == -4
    assert n.value == 4 and (short == index[:2]).all()
    for cut in (3, 6, 18, 20, 100, frame.size - 1):
        with pytest.raises(YsbError) as e:
            lz4.frame_index(frame[:cut].copy())
        assert e.value.code == -5 and "ends" in str(e.value), cut
    assert lz4.frame_index(b"")[0].size == 0


def test_carry_cut_through_the_abi():
    assert lz4.frame_carry_cut(b"ab\ncd\r") == 3 and lz4.frame_carry_cut(b"ab\ncd\r", more=False) == 6
    assert lz4.frame_carry_cut(b"ab\rcd") == 3 and lz4.frame_carry_cut(b"ab\r\ncd") == 4
    assert lz4.frame_carry_cut(b"abc") == 0 and lz4.frame_carry_cut(b"") == 0


def test_frame_fixtures_are_small():
    assert sum(os.path.getsize(os.path.join(FRAMES, f)) for f in os.listdir(FRAMES)) < 150_000
