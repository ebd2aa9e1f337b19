"""A pure-Python model of the LZ4 batches the library accepts (ysb_submit_raw_lz4), written from
the format's description, not from csrc/ysb_lz4.h:

  * a batch is blocks back to back plus a directory of (comp_bytes, raw_bytes); bit 31 of
    comp_bytes marks a stored block (raw_bytes bytes as they are); a block decodes to 1..65536
    bytes; outputs are back to back in directory order;
  * a sequence is a token, the 255-extension bytes of the literal length (when the high nibble
    is 15), the literals, a 2-byte little-endian offset in 1..65535, the extension bytes of the
    match length (when the low nibble is 15); the match length is the low nibble + 4 + the
    extensions; the block's last sequence ends after its literals;
  * a block is invalid when its input runs out inside a token, an extension, the literals or
    the offset; when an offset is 0 or reaches before the block's first byte; when literals or a
    match run past raw_bytes; when the block ends with fewer or more than raw_bytes bytes;
  * a block whose raw size nothing records (a standard frame's) is measured by its tokens alone
    (measure_block): the same rules, 65536 as the cap, the end where the input ends.

Also here: the corpora that the CPU tests (tests/test_lz4_logic.py) and the GPU tests
(tests/test_gpu_lz4.py) share: hand-assembled blocks, the malformed corpus, periodic and random
inputs.
"""
import os

STORED = 0x80000000
MAX_RAW = 65536
NO_BAD = 0xFFFFFFFF
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class Bad(Exception):
    pass


def _ext(src, ip, length):
    while True:
        if ip >= len(src):
            raise Bad("input exhausted inside a length extension")
        b = src[ip]
        ip += 1
        length += b
        if b != 255:
            return ip, length


def decode_block(src, raw_bytes):
    """The raw_bytes bytes a compressed (not stored) block decodes to; Bad if it is invalid."""
    if not 1 <= raw_bytes <= MAX_RAW:
        raise Bad("raw size")
    src = bytes(src)
    out = bytearray()
    ip = 0
    while True:
        if ip >= len(src):
            raise Bad("input exhausted where a token should be")
        tok = src[ip]
        ip += 1
        lit = tok >> 4
        if lit == 15:
            ip, lit = _ext(src, ip, lit)
        if ip + lit > len(src):
            raise Bad("input exhausted inside the literals")
        if len(out) + lit > raw_bytes:
            raise Bad("literals run past raw_bytes")
        out += src[ip:ip + lit]
        ip += lit
        if ip == len(src):           # the last sequence ends after its literals
            if len(out) != raw_bytes:
                raise Bad("the block ends with fewer bytes than raw_bytes")
            return bytes(out)
        if ip + 2 > len(src):
            raise Bad("input exhausted inside the offset")
        off = src[ip] | (src[ip + 1] << 8)
        ip += 2
        if off == 0:
            raise Bad("offset 0")
        if off > len(out):
            raise Bad("the offset reaches before the block's start")
        ml = tok & 15
        if ml == 15:
            ip, ml = _ext(src, ip, ml)
        ml += 4
        if len(out) + ml > raw_bytes:
            raise Bad("the match runs past raw_bytes")
        for _ in range(ml):          # byte by byte: an overlapping match replicates
            out.append(out[-off])


def measure_block(src):
    """The raw size of a compressed block that records none (a frame's block), by its tokens
    alone: the literal and match lengths add up, no more than MAX_RAW; the block ends where its
    input does, behind a sequence's literals; Bad for anything else the format forbids."""
    src = bytes(src)
    ip = op = 0
    while True:
        if ip >= len(src):
            raise Bad("input exhausted where a token should be")
        tok = src[ip]
        ip += 1
        lit = tok >> 4
        if lit == 15:
            ip, lit = _ext(src, ip, lit)
        if ip + lit > len(src):
            raise Bad("input exhausted inside the literals")
        ip += lit
        op += lit
        if op > MAX_RAW:
            raise Bad("literals run past the largest block")
        if ip == len(src):
            if op == 0:
                raise Bad("a block of no bytes")
            return op
        if ip + 2 > len(src):
            raise Bad("input exhausted inside the offset")
        off = src[ip] | (src[ip + 1] << 8)
        ip += 2
        if off == 0 or off > op:
            raise Bad("offset 0 or before the block's start")
        ml = tok & 15
        if ml == 15:
            ip, ml = _ext(src, ip, ml)
        op += ml + 4
        if op > MAX_RAW:
            raise Bad("a match runs past the largest block")


def decode_entry(src, comp_field, raw_bytes):
    if not 1 <= raw_bytes <= MAX_RAW:
        raise Bad("raw size")
    if comp_field & STORED:
        if len(src) != raw_bytes:
            raise Bad("a stored block of another size")
        return bytes(src)
    return decode_block(src, raw_bytes)


def decode_batch(blob, directory):
    """(output with each bad block's range left as b'\\0', first bad block or NO_BAD,
    [(start, end) of every block's output])."""
    out = bytearray()
    first_bad = NO_BAD
    ranges = []
    ip = 0
    for i, (cf, raw) in enumerate(directory):
        n = cf & ~STORED
        try:
            dec = decode_entry(blob[ip:ip + n], cf, raw)
        except Bad:
            dec = bytes(raw)
            if first_bad == NO_BAD:
                first_bad = i
        ranges.append((len(out), len(out) + raw))
        out += dec
        ip += n
    return bytes(out), first_bad, ranges


# ---- hand-assembled blocks: (name, compressed bytes, raw bytes they decode to) --------------

def _lits(n, seed=1):
    return bytes((seed * 37 + i * 11) & 0xFF for i in range(n))


def hand_blocks():
    cases = []
    a15 = _lits(15)
    cases.append(("literal length exactly 15, extension byte 0", bytes([0xF0, 0]) + a15, a15))
    a270 = _lits(270, 2)
    cases.append(("literal length 15 + 255, a terminating 0", bytes([0xF0, 255, 0]) + a270, a270))
    a8 = _lits(8, 3)
    # 8 literals, match length 19 = 15 + 4 (extension byte 0) at offset 8, then 1 literal
    cases.append(("match length exactly 19", bytes([0x8F]) + a8 + bytes([8, 0, 0, 0x10, 0x77]),
                  a8 + (a8 * 3)[:19] + b"\x77"))
    # The largest offset a valid block can use: a match is at least 4 bytes and a block at most
    # 65536, so at most 65532 bytes are out when a match starts.  (Offset 65535 "in a
    # 65536-byte block" can therefore only be an invalid block: malformed_blocks has it.)
    big = _lits(65532, 4)
    lit_hdr = bytes([0xF0]) + bytes([255] * ((65532 - 15) // 255)) + bytes([(65532 - 15) % 255])
    cases.append(("offset 65532 = the bytes produced so far, ending a 65536-byte block",
                  lit_hdr + big + bytes([0xFC, 0xFF, 0x00]), big + big[:4]))
    a5 = _lits(5, 5)
    cases.append(("offset equal to the bytes produced so far", bytes([0x51]) + a5 + bytes([5, 0, 0x10, 0x42]),
                  a5 + a5 + b"\x42"))
    cases.append(("a block of one literal", bytes([0x10, 0x5A]), b"\x5A"))
    cases.append(("an empty last sequence after a match", bytes([0x40]) + _lits(4, 6) + bytes([4, 0, 0x00]),
                  _lits(4, 6) * 2))
    return cases


# ---- the malformed corpus: (name, compressed bytes, raw_bytes) -- one base case per rule, and
# every base case (the valid hand-assembled blocks too) truncated at every byte position -------

def malformed_bases():
    a4 = _lits(4, 7)
    big = _lits(65535, 8)
    lit_hdr = bytes([0xF0]) + bytes([255] * ((65535 - 15) // 255)) + bytes([(65535 - 15) % 255])
    return [
        ("no input at all", b"", 1),
        ("input exhausted inside a literal extension", bytes([0xF0, 255, 255]), 600),
        ("input exhausted inside the literals", bytes([0x80]) + a4, 8),
        ("input exhausted inside the offset", bytes([0x40]) + a4 + bytes([4]), 12),
        ("input exhausted inside a match extension", bytes([0x4F]) + a4 + bytes([4, 0, 255]), 600),
        ("offset 0", bytes([0x40]) + a4 + bytes([0, 0, 0x00]), 12),
        ("offset before the block's start", bytes([0x40]) + a4 + bytes([5, 0, 0x00]), 12),
        ("literals past raw_bytes", bytes([0x40]) + a4, 3),
        ("match past raw_bytes", bytes([0x40]) + a4 + bytes([4, 0, 0x00]), 7),
        ("fewer bytes than raw_bytes", bytes([0x40]) + a4, 5),
        ("more: input left after raw_bytes are out", bytes([0x40]) + a4 + bytes([4, 0, 0x10, 0x33]), 8),
        ("the block ends with a match", bytes([0x40]) + a4 + bytes([4, 0]), 8),
        ("offset 65535 in a 65536-byte block", lit_hdr + big + bytes([0xFF, 0xFF]) + bytes([0x00]), 65536),
        ("a literal length of 64 KiB of 255s", bytes([0xF0]) + bytes([255] * 300), 65536),
        ("a match length far past raw_bytes", bytes([0x4F]) + a4 + bytes([1, 0]) + bytes([255] * 300) + bytes([0, 0]), 65536),
    ]


def malformed_blocks(max_len=400):
    """(name, bytes, raw): the bases, and every base and valid hand block up to max_len bytes
    cut at every byte position."""
    out = list(malformed_bases())
    for name, comp, raw in malformed_bases() + [(n, c, len(r)) for n, c, r in hand_blocks()]:
        if len(comp) > max_len:
            continue
        for cut in range(len(comp)):
            out.append(("%s, cut at %d" % (name, cut), comp[:cut], raw))
    return out


def is_valid(comp, raw, stored=False):
    try:
        decode_entry(comp, len(comp) | (STORED if stored else 0), raw)
        return True
    except Bad:
        return False


def periodic(period, n=65536):
    return bytes((i % period) * 29 & 0xFF for i in range(n))


def random_bytes(n, seed=12345):
    x = seed
    out = bytearray(n)
    for i in range(n):
        x = (x * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        out[i] = x >> 56
    return bytes(out)
