"""LZ4 batches on the host side (csrc/ysb_lz4.h through the C ABI): the library's own small
compressor and decoder, for sources, tools and tests that have no codec library of their own.

A batch is LZ4 blocks back to back and a directory: an (n, 2) uint32 array of
(comp_bytes | STORED, raw_bytes).  YsbContext.submit_raw_lz4 takes exactly that.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib

STORED = 0x80000000
MAX_RAW = 65536
DEFAULT_BLOCK = 8192   # the largest size at which the decode keeps the path PCIe-bound (DESIGN.md, LZ4 batches)


def _u8(data):
    return np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) \
        else np.ascontiguousarray(data, dtype=np.uint8)


def pack(data, block_bytes=DEFAULT_BLOCK, line_aligned=True, allow_stored=True, threads=1):
    """data cut into blocks of block_bytes (with line_aligned every block ends behind a line
    terminator where its range holds one, so any run of whole blocks is a raw batch of whole
    lines) and compressed.  Returns (blocks as a uint8 array, directory)."""
    src = _u8(data)
    # the sizes first (line-aligned cuts depend on the data): YSB_ERR_CAPACITY with both set
    n_bytes, n_blocks = C.c_uint64(), C.c_uint64()
    rc = lib().ysb_lz4_pack(src.ctypes.data, src.size, block_bytes, int(line_aligned), int(allow_stored), threads,
                            None, 0, C.byref(n_bytes), None, 0, C.byref(n_blocks))
    if rc not in (0, -4):
        check(rc)
    dst = np.empty(max(n_bytes.value, 1), dtype=np.uint8)
    directory = np.empty((max(n_blocks.value, 1), 2), dtype=np.uint32)
    check(lib().ysb_lz4_pack(src.ctypes.data, src.size, block_bytes, int(line_aligned), int(allow_stored), threads,
                             dst.ctypes.data, dst.size, C.byref(n_bytes), directory.ctypes.data, directory.shape[0],
                             C.byref(n_blocks)))
    return dst[:n_bytes.value], directory[:n_blocks.value]


def compress_block(data, allow_stored=True):
    """One block (1..65536 bytes) -> (compressed bytes, (comp_bytes field, raw_bytes))."""
    src = _u8(data)
    dst = np.empty(lib().ysb_lz4_compress_bound(src.size), dtype=np.uint8)
    e = _lib.YsbLz4Block()
    check(lib().ysb_lz4_compress_block(src.ctypes.data, src.size, dst.ctypes.data, dst.size, int(allow_stored), C.byref(e)))
    return dst[:e.comp_bytes & ~STORED].tobytes(), (e.comp_bytes, e.raw_bytes)


def decompress_block(comp, comp_field, raw_bytes):
    """The host decoder on one block; raises YsbError (YSB_ERR_FORMAT) for an invalid one."""
    src = _u8(comp) if len(comp) else np.zeros(1, dtype=np.uint8)
    dst = np.empty(max(raw_bytes, 1), dtype=np.uint8)
    e = _lib.YsbLz4Block(comp_field, raw_bytes)
    check(lib().ysb_lz4_decompress_block(src.ctypes.data, C.byref(e), dst.ctypes.data, dst.size))
    return dst[:raw_bytes].tobytes()


FILE_MAGIC = b"YSBLZ4B\n"
FILE_LINE_ALIGNED = 1


def write_file(path, data, block_bytes=DEFAULT_BLOCK, line_aligned=True, allow_stored=True, threads=1):
    """ysb_lz4_write_file: data as a compressed replay file (header, directory, blocks) -- what
    ysb_gen --lz4 writes and ysb_topology --lz4 reads."""
    src = _u8(data)
    check(lib().ysb_lz4_write_file(str(path).encode(), src.ctypes.data, src.size, block_bytes, int(line_aligned),
                                   int(allow_stored), threads))


def read_file(path):
    """(flags, raw_bytes, blocks as a uint8 array, directory) of a compressed replay file."""
    buf = np.fromfile(str(path), dtype=np.uint8)
    if buf.size < 32 or buf[:8].tobytes() != FILE_MAGIC:
        raise ValueError("%s is not a compressed replay file" % path)
    version, flags = (int(x) for x in buf[8:16].view(np.uint32))
    n, raw = (int(x) for x in buf[16:32].view(np.uint64))
    if version != 1 or 32 + 8 * n > buf.size:
        raise ValueError("%s: version %d, %d blocks in %d bytes" % (path, version, n, buf.size))
    directory = buf[32:32 + 8 * n].view(np.uint32).reshape(-1, 2)
    blocks = buf[32 + 8 * n:]
    if int((directory[:, 0] & 0x7FFFFFFF).sum()) != blocks.size or int(directory[:, 1].sum()) != raw:
        raise ValueError("%s: the directory does not match the file" % path)
    return flags, raw, blocks, directory


# ---- standard LZ4 frames (csrc/ysb_lz4_frame.h) ------------------------------------------------

FRAME_MAGIC = b"\x04\x22\x4d\x18"
FRAME_BLOCK = np.dtype([("offset", "<u8"), ("comp_bytes", "<u4"), ("reserved", "<u4")])


def is_frame(head):
    """True when the bytes begin like a standard frame (or a skippable frame in front of one)."""
    head = bytes(head[:4])
    return head == FRAME_MAGIC or (len(head) == 4 and head[1:] == b"\x2a\x4d\x18" and 0x50 <= head[0] <= 0x5F)


def frame_index(data):
    """ysb_lz4_frame_index: (index, summary dict) of a buffer of concatenated standard frames.
    index is a FRAME_BLOCK array: offset of each block's first data byte, comp_bytes | STORED.
    Raises YsbError (YSB_ERR_FORMAT) naming the byte offset and the rule for a frame the library
    does not take (linked blocks, a dictionary, a block maximum above 64 KiB, any truncation)."""
    src = _u8(data)
    n, info = C.c_uint64(), _lib.YsbLz4FrameSummary()
    rc = lib().ysb_lz4_frame_index(src.ctypes.data, src.size, None, 0, C.byref(n), C.byref(info))
    if rc not in (0, -4):
        check(rc)
    index = np.zeros(n.value, dtype=FRAME_BLOCK)
    if n.value:
        check(lib().ysb_lz4_frame_index(src.ctypes.data, src.size, index.ctypes.data, index.size, C.byref(n), C.byref(info)))
    return index, {k: getattr(info, k) for k, _ in info._fields_ if k != "reserved"}


def frame_pack(data, block_bytes=MAX_RAW, threads=1):
    """ysb_lz4_frame_pack: data as one standard frame (independent blocks, 64 KiB maximum, no
    checksums, content size set) that any LZ4 tool reads; a uint8 array."""
    src = _u8(data)
    dst = np.empty(lib().ysb_lz4_frame_bound(src.size, block_bytes), dtype=np.uint8)
    n = C.c_uint64()
    check(lib().ysb_lz4_frame_pack(src.ctypes.data, src.size, block_bytes, threads, dst.ctypes.data, dst.size, C.byref(n)))
    return dst[:n.value]


def frame_write(path, data, block_bytes=MAX_RAW, threads=1):
    """ysb_lz4_frame_write: frame_pack into a file (what `lz4 -B4 -BI` would write)."""
    src = _u8(data)
    check(lib().ysb_lz4_frame_write(str(path).encode(), src.ctypes.data, src.size, block_bytes, threads))


def measure_block(comp, comp_field=None):
    """The host model of the measure pass: a frame block's raw size by its tokens alone;
    raises YsbError (YSB_ERR_FORMAT) when no raw size makes the block valid."""
    src = _u8(comp) if len(comp) else np.zeros(1, dtype=np.uint8)
    raw = C.c_uint32()
    check(lib().ysb_lz4_measure_block(src.ctypes.data, len(comp) if comp_field is None else comp_field, C.byref(raw)))
    return raw.value


def frame_carry_cut(data, more=True):
    """ysb_lz4_frame_carry_cut: how many of data's bytes are whole lines when more batches
    follow; the rest is carried in front of the next batch."""
    src = _u8(data)
    return lib().ysb_lz4_frame_carry_cut(src.ctypes.data if src.size else None, src.size, int(more))
