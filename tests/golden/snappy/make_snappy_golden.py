"""Writes the snappy fixtures beside this script: the first 131072 bytes of ../gen_s7.jsonl cut to
blocks of 65536 and of 32768 raw bytes, each block compressed by the real snappy that pyarrow
bundles (pyarrow.compress(..., codec="snappy"): one raw block, preamble included), the blocks of a
file laid out as a xerial stream -- the 16-byte header and a big-endian length word in front of
each block are written here, the blocks' bytes are the library's.  Data only; the versions are
recorded in versions.txt.  Run from anywhere: python tests/golden/snappy/make_snappy_golden.py"""
import os
import struct

import pyarrow as pa

HERE = os.path.dirname(os.path.abspath(__file__))
RAW_BYTES = 131072


def main():
    src = open(os.path.join(HERE, "..", "gen_s7.jsonl"), "rb").read()[:RAW_BYTES]
    for name, block in (("gen_s7_128k.b64k.xerial", 65536), ("gen_s7_128k.b32k.xerial", 32768)):
        out = bytearray(b"\x82SNAPPY\x00" + struct.pack(">ii", 1, 1))
        for a in range(0, len(src), block):
            z = pa.compress(src[a:a + block], codec="snappy", asbytes=True)
            out += struct.pack(">i", len(z)) + z
        with open(os.path.join(HERE, name), "wb") as f:
            f.write(out)
        print(name, len(out))
    with open(os.path.join(HERE, "versions.txt"), "w") as f:
        f.write("pyarrow %s\nraw_bytes %d\n" % (pa.__version__, RAW_BYTES))


if __name__ == "__main__":
    main()
