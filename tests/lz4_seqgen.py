"""LZ4 blocks written from explicit sequence lists, not by a compressor: the corpus of
tests/test_lz4_seq_logic.py (CPU, the sanitized host build of the shared reader) and
tests/test_gpu_lz4_seq.py (both decode kernels and the measure kernel).

A compressor reaches a biased corner of the format: it never ends a block with a match, it keeps
the end-of-block conventions, and how many sequences a block has or where a token falls against
a reader's window is left to chance.  Here each of those is chosen:

  build(seqs, tail)   [(literals, offset, match_len)] and the last sequence's literals -> the
                      block in the canonical length encoding and the bytes it decodes to, by
                      replaying the list (lz4_model.decode_block is not called);
  count_blocks()      exactly k sequences for k around the wide kernel's batch of 64 and its ring
                      of three buffers, in four literal-run styles;
  straddle_blocks()   every literal run 40..1100 in front of a match, so that the offset bytes,
                      the match extension, the next token and its literal extension land at every
                      position across the readers' 64-, 256- and 512-byte boundaries;
  extreme_blocks()    16,384 sequences in 65,536 bytes, a full block ending in a match, 64 long
                      runs, every sequence through the reader's jump path;
  mutants(blocks)     invalid blocks made from valid ones deep inside them.

Everything is drawn from the LCG below, so the corpus is the same bytes everywhere; the CPU test
pins its SHA-256.
"""
import collections
import functools
import struct

import lz4_model as M

LIT_RUNS = (0, 1, 7, 8, 9, 31, 32, 33, 127, 128, 129)     # against the literal copier's split at 32
LIT_EXT_RUNS = (14, 15, 16, 269, 270, 271)                # last extension byte 0, 254, 255 then 0
OFFSETS = (1, 2, 3, 4, 15, 16, 17, 31, 32, 33, 63, 64, 65)
MATCH_LENS = (63, 64, 65, 128)                            # against the 64-byte chunk
MATCH_EXT_LENS = (18, 19, 20, 273, 274, 275)
COUNTS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193, 256, 257)
STYLES = ("zero", "short", "long", "mixed")
TAILS = (0, 1, 5, 33)
BOUNDARIES = (64, 256, 512, 768, 1024)
MANY = 16384

# One sequence as build() laid it out: positions in the compressed block of the token, the
# literals and the offset's low byte (-1 in the last sequence), how many extension bytes follow
# the token (behind it) and the offset (behind its high byte), the literal run, the offset and
# match length, and how many bytes were produced when the match began.
Seq = collections.namedtuple("Seq", "tok lit_ext lit_pos lit_len off_pos match_ext offset match_len op")


class Lcg:
    """lz4_model.random_bytes's generator, one draw at a time."""

    def __init__(self, seed):
        self.x = seed

    def below(self, n):
        self.x = (self.x * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        return (self.x >> 33) % n

    def pick(self, items):
        return items[self.below(len(items))]


_POOL = M.random_bytes(1 << 16, seed=20240607)


def lits(rng, n):
    """n literal bytes: a slice of one random pool at a drawn position."""
    at = rng.below(len(_POOL) - n)
    return _POOL[at:at + n]


def _length(n):
    """A length's extension bytes (n: what is above the nibble's 15)."""
    return bytes([255]) * (n // 255) + bytes([n % 255])


def layout(seqs, tail):
    """(compressed block, the bytes it decodes to, [Seq] with the last sequence included)."""
    comp, raw, fields = bytearray(), bytearray(), []
    for lit, off, ml in seqs:
        ll = len(lit)
        assert ml >= 4 and 1 <= off <= 65535
        tok = len(comp)
        comp.append(min(ll, 15) << 4 | min(ml - 4, 15))
        lx = _length(ll - 15) if ll >= 15 else b""
        comp += lx
        lit_pos = len(comp)
        comp += lit
        raw += lit
        assert off <= len(raw), "an offset before the block's start"
        off_pos = len(comp)
        comp += bytes((off & 255, off >> 8))
        mx = _length(ml - 19) if ml >= 19 else b""
        comp += mx
        fields.append(Seq(tok, len(lx), lit_pos, ll, off_pos, len(mx), off, ml, len(raw)))
        at = len(raw) - off
        if off >= ml:
            raw += raw[at:at + ml]
        else:                       # an overlapping match replicates the `off` bytes before it
            raw += (raw[at:] * (ml // off + 1))[:ml]
    ll = len(tail)
    tok = len(comp)
    comp.append(min(ll, 15) << 4)
    lx = _length(ll - 15) if ll >= 15 else b""
    comp += lx
    fields.append(Seq(tok, len(lx), len(comp), ll, -1, 0, 0, 0, len(raw) + ll))
    comp += tail
    raw += tail
    assert 1 <= len(raw) <= M.MAX_RAW
    return bytes(comp), bytes(raw), fields


def build(seqs, tail):
    comp, raw, _ = layout(seqs, tail)
    return comp, raw


_FIELDS = {}   # a valid block's name -> its [Seq]


def fields_of(name):
    return _FIELDS[name]


def _named(name, seqs, tail, k=None):
    comp, raw, fields = layout(seqs, tail)
    assert k is None or len(fields) == k, (name, len(fields))
    assert name not in _FIELDS or _FIELDS[name] == fields
    _FIELDS[name] = fields
    return name, comp, raw


# ---- exactly k sequences ---------------------------------------------------------------------

def _pairs(rng):
    """Every edge offset with the match lengths off - 1, off, off + 1 and every edge length, in a
    drawn order."""
    out = []
    for off in OFFSETS:
        for ml in (off - 1, off, off + 1, 4) + MATCH_LENS + MATCH_EXT_LENS:
            if ml >= 4 and (off, ml) not in out:
                out.append((off, ml))
    for i in range(len(out) - 1, 0, -1):
        j = rng.below(i + 1)
        out[i], out[j] = out[j], out[i]
    return out


_RUNS = {"zero": (0,), "short": tuple(r for r in LIT_RUNS if r <= 32), "long": tuple(r for r in LIT_RUNS if r > 32),
         "mixed": LIT_RUNS + LIT_EXT_RUNS}


@functools.lru_cache(maxsize=None)
def count_blocks():
    """Blocks of exactly k sequences, the last one included, for k in COUNTS and each style of
    literal runs: none but the block's first byte, all <= 32, all > 32, mixed.  Offsets and
    match lengths walk the shuffled edge pairs; an offset larger than what is produced so far
    becomes equal to it.  Long matches draw on a budget per block (then they shrink to 4..16), so
    the largest block stays far below 65,536 bytes."""
    rng = Lcg(0x5EC0)
    pairs = _pairs(rng)
    cursor = 0
    out = []
    for ki, k in enumerate(COUNTS):
        for si, style in enumerate(STYLES):
            seqs, op, budget = [], 0, 2000 + 40 * k
            for i in range(k - 1):
                ll = rng.pick(_RUNS[style])
                if i == 0 and ll == 0:
                    ll = 1
                off, ml = pairs[cursor % len(pairs)]
                cursor += 1
                op += ll
                off = min(off, op)
                if ml > 70:
                    if budget >= ml:
                        budget -= ml
                    else:
                        ml = 4 + ml % 13
                seqs.append((lits(rng, ll), off, ml))
                op += ml
            tail = 0 if style == "zero" else TAILS[(ki + si) % 4]
            if k == 1:
                tail = max(tail, 1)
            out.append(_named("%d sequences, %s runs, tail %d" % (k, style, tail), seqs, lits(rng, tail), k))
    return tuple(out)


# ---- field positions against the readers' windows ----------------------------------------------

def _header(n):
    """Bytes in front of a run of n literals: the token and the extension."""
    return 1 + (0 if n < 15 else 1 + (n - 15) // 255)


def _run_ending_at(pos):
    """The literal run of a block's first sequence whose offset's low byte is at `pos`, or None."""
    for n in range(max(pos - 8, 1), pos):
        if _header(n) + n == pos:
            return n
    return None


@functools.lru_cache(maxsize=None)
def straddle_blocks(max_l=1100):
    """For every literal run L in 40..max_l: L literals and a match of 19, 274 or 529 (one, two,
    three extension bytes), a sequence of 15..17 literals (one literal extension byte), a short
    one, a tail.  The first offset's low byte is at L + 2 .. L + 6, so over all L the offset
    bytes, the match extension, the next token and its extension byte each pass every position
    across the 64-, 256- and 512-byte boundaries, and from L = 510 on the wide reader jumps.
    Around each boundary two more shapes: a first match without extension (the next token right
    behind the offset), and a short sequence in front of a run of 271 or 600 literals (that
    run's own token and its two or three extension bytes across the boundary; with 600, a jump
    that starts next to a refill)."""
    rng = Lcg(0x57AD)
    out = []
    for L in range(40, max_l + 1):
        seqs = [(lits(rng, L), min(OFFSETS[L % len(OFFSETS)], L), (19, 274, 529)[L % 3]),
                (lits(rng, 15 + L % 3), rng.pick(OFFSETS), 4 + L % 5),
                (lits(rng, L % 4), rng.pick(OFFSETS), 18 + L % 3)]
        out.append(_named("straddle L=%d" % L, seqs, lits(rng, TAILS[L % 4])))
    # The measure pass sees an offset only through "0" and "before the block's start": runs of
    # zero bytes, so that an offset byte read from anywhere in the run instead of behind it
    # (a stale window) makes the block bad there too.
    for L in list(range(248, 264)) + list(range(500, 520)):
        if L <= max_l:
            seqs = [(bytes(L), 1 + L % 200, 4 + L % 3)]
            out.append(_named("straddle, %d zero literals" % L, seqs, b"\x01"))
    for B in BOUNDARIES:
        for at in range(B - 8, B + 8):
            n = _run_ending_at(at - 2)        # the second sequence's token at `at`
            if n is None or n > max_l:
                continue
            seqs = [(lits(rng, n), rng.pick(OFFSETS[:10]), 5 + at % 7), (lits(rng, 3), 2, 4)]
            out.append(_named("straddle, a token behind the offset at %d" % at, seqs, lits(rng, 1)))
            for L2, ml in ((271, 274), (600, 19)):
                if n + L2 > max_l + 300:
                    continue
                seqs = [(lits(rng, n), rng.pick(OFFSETS[:10]), 4), (lits(rng, L2), rng.pick(OFFSETS), ml),
                        (lits(rng, 2), 1, 6)]
                out.append(_named("straddle, a run of %d with its token at %d" % (L2, at), seqs, lits(rng, 5)))
    return tuple(out)


# ---- the outliers ----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def extreme_blocks():
    rng = Lcg(0xE87E)
    out = []
    # 65,536 bytes in 16,384 sequences: 256 stages of the wide kernel
    seqs = [(lits(rng, 1), 1, 4)]
    for i in range(MANY - 2):
        seqs.append((b"", min(1 + i % 5, 5), 4))
    name, comp, raw = _named("%d sequences in 65536 bytes" % MANY, seqs, lits(rng, 3), MANY)
    assert len(raw) == 65536 and len(comp) == 49154
    out.append((name, comp, raw))
    # a full block that ends with a match and an empty last sequence
    seqs = [(lits(rng, 300), 64, 30000), (lits(rng, 33), 333, 275), (b"", 7, 65536 - 300 - 30000 - 33 - 275)]
    name, comp, raw = _named("65536 bytes ending with a match", seqs, b"")
    assert len(raw) == 65536
    out.append((name, comp, raw))
    # one batch of the wide kernel, every run long: a full ballot
    seqs = [(lits(rng, 129), rng.pick(OFFSETS), 4 + i % 3) for i in range(63)]
    out.append(_named("64 sequences of 129 literals", seqs, lits(rng, 129), 64))
    # every sequence steps over more than two windows, then reads on from the prefetched one
    seqs = [(lits(rng, 600), rng.pick(OFFSETS), 4) for i in range(100)]
    out.append(_named("600-literal runs and 4-byte matches", seqs, lits(rng, 600)))
    return tuple(out)


def valid_blocks():
    return count_blocks() + straddle_blocks() + extreme_blocks()


# ---- invalid blocks ----------------------------------------------------------------------------

def mutants(blocks, limit=2000):
    """[(name, comp, raw)], each invalid by construction, from valid blocks of at least 130
    sequences.  At sequence j in {0, 63, 64, 65, 127, 128, the last match}: the offset 0; the
    offset one more than the bytes produced before the match; the input cut behind the token (or
    inside its extension), inside the literals, between the offset's bytes, and inside the match
    extension (or behind the offset: a block that ends with a match).  For the block: raw one
    smaller and one larger, and a cut in each of the last 40 bytes.  Blocks whose decoding is
    long (above 1,000 sequences) get the offset and raw mutants only."""
    out = []
    for name, comp, raw_bytes in blocks:
        f = fields_of(name)
        assert len(f) >= 130, name
        raw, small = len(raw_bytes), len(f) <= 1000
        for j in (0, 63, 64, 65, 127, 128, len(f) - 2):
            s = f[j]
            zero = bytearray(comp)
            zero[s.off_pos:s.off_pos + 2] = b"\0\0"
            out.append(("%s: sequence %d, offset 0" % (name, j), bytes(zero), raw))
            if s.op + 1 <= 65535:
                far = bytearray(comp)
                far[s.off_pos:s.off_pos + 2] = struct.pack("<H", s.op + 1)
                out.append(("%s: sequence %d, offset %d of %d" % (name, j, s.op + 1, s.op), bytes(far), raw))
            if not small:
                continue
            cuts = [("the token's extension", s.tok + 1 + max(s.lit_ext - 1, 0)),
                    ("the offset", s.off_pos + 1),
                    ("the match extension", s.off_pos + 2 + max(s.match_ext - 1, 0))]
            if s.lit_len:
                cuts.append(("the literals", s.lit_pos + s.lit_len // 2))
            for what, cut in cuts:
                out.append(("%s: sequence %d, cut inside %s" % (name, j, what), comp[:cut], raw))
        if raw > 1:
            out.append(("%s: raw one smaller" % name, comp, raw - 1))
        if raw < M.MAX_RAW:
            out.append(("%s: raw one larger" % name, comp, raw + 1))
        if small:
            for c in range(1, 41):
                out.append(("%s: the last %d bytes cut" % (name, c), comp[:len(comp) - c], raw))
    assert len(out) <= limit, len(out)
    return out


def mutant_bases():
    """The blocks the tests make mutants of: the count blocks of 191 sequences and more, and
    the block of 16,384."""
    return [b for b in count_blocks() if len(fields_of(b[0])) >= 191] + [extreme_blocks()[0]]


def serialize(valid, bad):
    """The corpus as tests/native/lz4_seq_logic.cpp reads it: u32 count, then per block u32
    comp_len, raw, valid, the compressed bytes and (valid blocks) the raw bytes."""
    parts = [struct.pack("<I", len(valid) + len(bad))]
    for _, comp, raw in valid:
        parts += [struct.pack("<III", len(comp), len(raw), 1), comp, raw]
    for _, comp, raw in bad:
        parts += [struct.pack("<III", len(comp), raw, 0), comp]
    return b"".join(parts)
