"""Writes the liblz4 frame fixtures beside this script, with the system liblz4's
LZ4F_compressBegin / Update / End through ctypes.  Data only; the library version is recorded in versions.txt.

  gen_s7_150k.lz4        the first whole lines of ../gen_s7.jsonl up to 150,000 bytes as one frame
                         of independent 64 KiB blocks (two full blocks and a short one; lines
                         straddle both edges), no checksums, no content size
  small_checksums.lz4    the first whole lines up to 3,000 bytes: block checksums, a content
                         checksum and the content size
  small_linked.lz4       the same lines with linked blocks (refused)
  small_b5.lz4           ... with a 256 KiB block maximum (refused)
  small_skip_two.lz4     a frame of the first half of those lines, a skippable frame of 11
                         bytes, a frame of the second half

Run from anywhere: python tests/golden/lz4frame/make_lz4frame_golden.py"""
import ctypes
import os
import struct

HERE = os.path.dirname(os.path.abspath(__file__))


class FrameInfo(ctypes.Structure):
    _fields_ = [("blockSizeID", ctypes.c_int), ("blockMode", ctypes.c_int), ("contentChecksumFlag", ctypes.c_int),
                ("frameType", ctypes.c_int), ("contentSize", ctypes.c_ulonglong), ("dictID", ctypes.c_uint),
                ("blockChecksumFlag", ctypes.c_int)]


class Preferences(ctypes.Structure):
    _fields_ = [("frameInfo", FrameInfo), ("compressionLevel", ctypes.c_int), ("autoFlush", ctypes.c_uint),
                ("favorDecSpeed", ctypes.c_uint), ("reserved", ctypes.c_uint * 3)]


def whole_lines(data, limit):
    return data[:data.rindex(b"\n", 0, limit) + 1]


def main():
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

    def frame(src, block_id=4, independent=True, content_checksum=False, block_checksum=False, content_size=False):
        p = Preferences()
        p.frameInfo.blockSizeID = block_id
        p.frameInfo.blockMode = 1 if independent else 0
        p.frameInfo.contentChecksumFlag = int(content_checksum)
        p.frameInfo.blockChecksumFlag = int(block_checksum)
        p.frameInfo.contentSize = len(src) if content_size else 0
        # (the streaming entry points: LZ4F_compressFrame rewrites the block maximum and the block
        # mode of a source that fits one block)
        cctx = ctypes.c_void_p()
        assert not L.LZ4F_isError(L.LZ4F_createCompressionContext(ctypes.byref(cctx), 100))
        cap = L.LZ4F_compressBound(len(src), ctypes.byref(p)) + 64
        dst = ctypes.create_string_buffer(cap)
        n = L.LZ4F_compressBegin(cctx, dst, cap, ctypes.byref(p))
        assert not L.LZ4F_isError(n)
        for step in (lambda at: L.LZ4F_compressUpdate(cctx, ctypes.byref(dst, at), cap - at, src, len(src), None),
                     lambda at: L.LZ4F_compressEnd(cctx, ctypes.byref(dst, at), cap - at, None)):
            k = step(n)
            assert not L.LZ4F_isError(k)
            n += k
        L.LZ4F_freeCompressionContext(cctx)
        return dst.raw[:n]

    data = open(os.path.join(HERE, "..", "gen_s7.jsonl"), "rb").read()
    big, small = whole_lines(data, 150000), whole_lines(data, 3000)
    half = small.index(b"\n", len(small) // 2) + 1
    files = {
        "gen_s7_150k.lz4": frame(big),
        "small_checksums.lz4": frame(small, content_checksum=True, block_checksum=True, content_size=True),
        "small_linked.lz4": frame(small, independent=False),
        "small_b5.lz4": frame(small, block_id=5),
        "small_skip_two.lz4": frame(small[:half]) + struct.pack("<II", 0x184D2A53, 11) + b"skip me now" + frame(small[half:]),
    }
    for name, blob in files.items():
        with open(os.path.join(HERE, name), "wb") as f:
            f.write(blob)
        print(name, len(blob))
    with open(os.path.join(HERE, "versions.txt"), "w") as f:
        f.write("liblz4 %s\nbig_raw_bytes %d\nsmall_raw_bytes %d\nsmall_half %d\n"
                % (L.LZ4_versionString().decode(), len(big), len(small), half))


if __name__ == "__main__":
    main()
