"""Writes the liblz4 fixtures beside this script: the first 65536 bytes of ../gen_s7.jsonl as one
LZ4 block from the system liblz4's default (LZ4_compress_default) and HC (LZ4_compress_HC,
level 9) entry points.  Data only; the library version is recorded in versions.txt.
Run from anywhere: python tests/golden/lz4/make_lz4_golden.py"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    L = ctypes.CDLL("liblz4.so.1")
    L.LZ4_versionString.restype = ctypes.c_char_p
    src = open(os.path.join(HERE, "..", "gen_s7.jsonl"), "rb").read()[:65536]
    cap = L.LZ4_compressBound(len(src))
    for name, fn, extra in (("gen_s7_64k.default.lz4", L.LZ4_compress_default, ()),
                            ("gen_s7_64k.hc.lz4", L.LZ4_compress_HC, (9,))):
        dst = ctypes.create_string_buffer(cap)
        n = fn(src, dst, len(src), cap, *extra)
        assert n > 0
        with open(os.path.join(HERE, name), "wb") as f:
            f.write(dst.raw[:n])
        print(name, n)
    with open(os.path.join(HERE, "versions.txt"), "w") as f:
        f.write("liblz4 %s\nraw_bytes 65536\n" % L.LZ4_versionString().decode())


if __name__ == "__main__":
    main()
