// ysb_snappy.h -- snappy blocks (Kafka attributes codec 2: ysb_kafka_lz4.h, ysb_snappy.hip): what
// a consumer holds when the topic's producers set compression.type=snappy.  A byte-oriented LZ77
// format without an entropy stage, like LZ4 (ysb_lz4.h), with two differences that matter here: a
// block opens with its own raw size, so nothing has to measure it, and the compressed bytes may
// outgrow the raw ones (65536 random bytes take 65542), so the kernel's in-place window of
// ysb_lz4.h does not carry over.
//
// No HIP here: the format's rules in ONE element reader and ONE preamble reader that the host
// model below and the kernels (ysb_snappy.hip) both call, the host block decoder (a plain byte
// loop: the model), a small greedy compressor (test inputs and the tools' batches; its ratio is
// not a goal), and the two framings a Kafka batch's records section takes -- the Java client's
// xerial stream of chunks, or one raw block.  tests/native/snappy_logic.cpp runs all of it on
// the CPU.
//
// Format.  A block is a preamble -- its raw size as a little-endian base-128 varint of at most 5
// bytes and a value below 2^32; non-minimal forms are legal -- and elements keyed by the tag's
// low two bits:
//   00  a literal: length - 1 in the upper six bits, 60..63 meaning that 1..4 little-endian
//       length bytes follow (non-minimal forms are legal), then the bytes;
//   01  a copy of 4..11 bytes, the offset's upper three bits in the tag and one byte behind it;
//   10  a copy of 1..64 bytes, a 16-bit little-endian offset;
//   11  a copy of 1..64 bytes, a 32-bit little-endian offset (a small one is legal).
// A copy with offset < length replicates the bytes before it.  This project reads blocks of
// 1..65536 raw bytes (SNAPPY_MAX_RAW): larger ones are chains of 64 KiB fragments whose
// compressed boundaries nothing records ("What is not built").
#pragma once
#include <cstdio>
#include <cstring>

#include "../../include/ysb_hip.h"
#include "ysb_common.h"

namespace ysb {

constexpr u32 SNAPPY_MAX_RAW = 65536;                                         // a block's raw size: 1..SNAPPY_MAX_RAW
YSB_HD u32 snappy_bound(u32 raw) { return 32 + raw + raw / 6; }               // the format's own bound on a block
constexpr u32 SNAPPY_MAX_COMP = 32 + SNAPPY_MAX_RAW + SNAPPY_MAX_RAW / 6;     // ... of the largest block read: 76490
// comp_bytes bit 30 of an index entry (ysb_lz4_frame_block): the block is snappy, not LZ4
constexpr u32 SNAPPY_BLOCK = YSB_SNAPPY_BLOCK;
constexpr u32 SNAPPY_LEN_MASK = 0x3FFFFFFFu;

enum : u32 { SNAPPY_EL_OK = 0, SNAPPY_EL_BAD = 1 };

// One element as the reader found it: `len` bytes, a literal's (offset 0) at input position
// `pos`, a copy's from `offset` bytes back; the next tag is at `next`.
struct SnappyEl {
    u32 pos, len, offset, next;
};

// THE preamble reader: the raw size at the front of a block of `comp` bytes, *next the first
// element's position.  false: the input ends inside it, more than 5 bytes, or a value >= 2^32.
// In::byte(pos) is called with pos < comp only.
template <class In>
YSB_HD bool snappy_read_preamble(In& in, u32 comp, u32* raw, u32* next) {
    u32 v = 0;
    for (u32 i = 0; i < 5; ++i) {
        if (i >= comp) return false;
        const u32 b = in.byte(i);
        if (i == 4 && b > 15u) return false;   // a sixth byte would follow, or bits 32 and up are set
        v |= (b & 127u) << (7 * i);
        if (b < 128u) {
            *raw = v;
            *next = i + 1;
            return true;
        }
    }
    return false;
}

// A block's size as the index and the kernels take it: the preamble's value when it is in
// 1..SNAPPY_MAX_RAW, else 0.
template <class In>
YSB_HD u32 snappy_block_raw(In& in, u32 comp, u32* next) {
    u32 raw = 0, nx = 0;
    if (!snappy_read_preamble(in, comp, &raw, &nx) || raw > SNAPPY_MAX_RAW) return 0;
    if (next) *next = nx;
    return raw;
}

// THE reader: the element whose tag is at input position ip < comp, of a block of `comp`
// compressed and `raw` raw bytes of which `op` are produced (op <= raw).  Every bounds rule is here:
//   an element cut off by the block's end (inside the length bytes, the offset or the literal);
//   offset 0; an offset reaching in front of the block's first output byte;
//   a literal or a copy running past raw.
// The caller walks while ip < comp and then asks for op == raw (the input ending with the output
// short); input left when raw bytes are out is an element of at least one byte past raw, so the
// reader refuses it.  It reads input only and copies nothing; every call consumes the tag at
// least, so a walk over `comp` bytes ends.  In::byte(pos) is called with pos < comp only.
template <class In>
YSB_HD u32 snappy_read_el(In& in, u32 ip, u32 comp, u32 op, u32 raw, SnappyEl* e) {
    const u32 tag = in.byte(ip++);
    const u32 kind = tag & 3u;
    if (kind == 0) {
        u32 len = tag >> 2;   // length - 1
        if (len >= 60u) {
            const u32 nb = len - 59u;
            if (comp - ip < nb) return SNAPPY_EL_BAD;
            len = 0;
            for (u32 i = 0; i < nb; ++i) len |= in.byte(ip + i) << (8 * i);
            ip += nb;
        }
        if (len >= raw - op || len >= comp - ip) return SNAPPY_EL_BAD;   // (length = len + 1; no sum overflows)
        e->pos = ip;
        e->len = len + 1;
        e->offset = 0;
        e->next = ip + len + 1;
        return SNAPPY_EL_OK;
    }
    u32 len, off;
    if (kind == 1) {
        if (comp - ip < 1) return SNAPPY_EL_BAD;
        len = 4 + ((tag >> 2) & 7u);
        off = (tag >> 5) << 8 | in.byte(ip);
        ip += 1;
    } else if (kind == 2) {
        if (comp - ip < 2) return SNAPPY_EL_BAD;
        len = (tag >> 2) + 1;
        off = in.byte(ip) | in.byte(ip + 1) << 8;
        ip += 2;
    } else {
        if (comp - ip < 4) return SNAPPY_EL_BAD;
        len = (tag >> 2) + 1;
        off = in.byte(ip) | in.byte(ip + 1) << 8 | in.byte(ip + 2) << 16 | in.byte(ip + 3) << 24;
        ip += 4;
    }
    if (off == 0 || off > op || len > raw - op) return SNAPPY_EL_BAD;
    e->pos = 0;
    e->len = len;
    e->offset = off;
    e->next = ip;
    return SNAPPY_EL_OK;
}

// LDS bytes of a decode launch whose largest block holds max_raw bytes: the output block alone,
// up to 15 bytes in front (it starts at its global address mod 16), a multiple of 16.
YSB_HD u32 snappy_lds_bytes(u32 max_raw) { return (16 + max_raw + 15) & ~15u; }

#if !defined(__HIP_DEVICE_COMPILE__)

// ---- host model -------------------------------------------------------------------------

struct SnappyHostIn {
    const u8* p;
    u32 byte(u32 pos) const { return p[pos]; }
};

// A block's raw size by its preamble (0: a bad preamble, 0, or above SNAPPY_MAX_RAW).
static inline u32 snappy_raw_of(const u8* in, u32 comp) {
    SnappyHostIn src{in};
    return snappy_block_raw(src, comp, nullptr);
}

// One block into out (SNAPPY_MAX_RAW bytes at least, or the preamble's size where the caller
// knows it).  Returns the raw size, 0: invalid (out may hold a decoded prefix).
static inline u32 snappy_decode_block(const u8* in, u32 comp, u8* out) {
    SnappyHostIn src{in};
    u32 ip = 0, op = 0;
    const u32 raw = snappy_block_raw(src, comp, &ip);
    if (!raw) return 0;
    while (ip < comp) {
        SnappyEl e;
        if (snappy_read_el(src, ip, comp, op, raw, &e) != SNAPPY_EL_OK) return 0;
        if (e.offset == 0) std::memcpy(out + op, in + e.pos, e.len);
        else
            for (u32 k = 0; k < e.len; ++k) out[op + k] = out[op + k - e.offset];   // byte order: an overlap replicates
        op += e.len;
        ip = e.next;
    }
    return op == raw ? raw : 0;
}

// ---- host compressor --------------------------------------------------------------------
// Greedy, one hash table of 4-byte windows.  It makes inputs, not ratios: a copy of 4..11 bytes
// within 2047 takes the one-byte-offset form, a piece of 12 bytes or more from 32768 or further
// back the four-byte-offset form (legal for any offset, and so all three forms come out of
// ordinary data), the rest the two-byte form; a match above 64 bytes goes out in pieces of 64 and
// a last one of at least 4, and a run of one byte as copies of offset 1.

static inline u32 snappy_put_preamble(u8* dst, u32 n) {
    u32 o = 0;
    for (; n >= 128u; n >>= 7) dst[o++] = (u8)(n | 128u);
    dst[o++] = (u8)n;
    return o;
}

static inline u32 snappy_put_literal(u8* dst, u32 o, const u8* src, u32 len) {   // len >= 1
    const u32 m = len - 1;
    if (m < 60u) {
        dst[o++] = (u8)(m << 2);
    } else {
        const u32 nb = m < 256u ? 1 : m < 65536u ? 2 : m < (1u << 24) ? 3 : 4;
        dst[o++] = (u8)((59u + nb) << 2);
        for (u32 i = 0; i < nb; ++i) dst[o++] = (u8)(m >> (8 * i));
    }
    std::memcpy(dst + o, src, len);
    return o + len;
}

static inline u32 snappy_put_copy(u8* dst, u32 o, u32 off, u32 len) {   // len in 1..64
    if (len >= 4 && len <= 11 && off < 2048u) {
        dst[o++] = (u8)(1u | (len - 4) << 2 | (off >> 8) << 5);
        dst[o++] = (u8)off;
    } else if (off >= 32768u && len >= 12) {
        dst[o++] = (u8)(3u | (len - 1) << 2);
        for (u32 i = 0; i < 4; ++i) dst[o++] = (u8)(off >> (8 * i));
    } else {
        dst[o++] = (u8)(2u | (len - 1) << 2);
        dst[o++] = (u8)off;
        dst[o++] = (u8)(off >> 8);
    }
    return o;
}

// src[0, n), 1 <= n <= SNAPPY_MAX_RAW, into dst (snappy_bound(n) bytes at least) as one block,
// preamble included; returns the compressed size.
static inline u32 snappy_compress_block(const u8* src, u32 n, u8* dst) {
    constexpr u32 HASH_BITS = 13;
    u32 table[1u << HASH_BITS] = {};   // position + 1 of the last window with this hash (0: none)
    auto rd32 = [&](u32 i) { u32 v; std::memcpy(&v, src + i, 4); return v; };
    u32 o = snappy_put_preamble(dst, n), anchor = 0, i = 0;
    while (n >= 4 && i <= n - 4) {
        const u32 v = rd32(i), h = (v * 2654435761u) >> (32 - HASH_BITS);
        const u32 cand = table[h];
        table[h] = i + 1;
        if (cand && rd32(cand - 1) == v) {
            const u32 c = cand - 1, off = i - c;
            u32 ml = 4;
            while (i + ml < n && src[c + ml] == src[i + ml]) ++ml;
            if (i > anchor) o = snappy_put_literal(dst, o, src + anchor, i - anchor);
            i += ml;
            anchor = i;
            for (; ml >= 68; ml -= 64) o = snappy_put_copy(dst, o, off, 64);
            if (ml > 64) {
                o = snappy_put_copy(dst, o, off, 60);
                ml -= 60;
            }
            o = snappy_put_copy(dst, o, off, ml);
        } else {
            ++i;
        }
    }
    if (n > anchor) o = snappy_put_literal(dst, o, src + anchor, n - anchor);
    return o;
}

// ---- a Kafka batch's records section: the xerial stream or one raw block -------------------
constexpr u32 XERIAL_HEADER = 16;
constexpr u32 XERIAL_CHUNK = 32768;   // SnappyOutputStream's default block size
static const u8 XERIAL_MAGIC[8] = {0x82, 'S', 'N', 'A', 'P', 'P', 'Y', 0};

struct SnappyError {
    u64 at = 0;          // the chunk's (or the header field's) byte within the records section
    char msg[256] = {0};
};

static inline u32 snappy_be32(const u8* p) { return (u32)p[0] << 24 | (u32)p[1] << 16 | (u32)p[2] << 8 | p[3]; }
static inline void snappy_put_be32(u8* p, u32 v) {
    p[0] = (u8)(v >> 24);
    p[1] = (u8)(v >> 16);
    p[2] = (u8)(v >> 8);
    p[3] = (u8)v;
}
static inline bool snappy_is_xerial(const u8* p, u64 n) { return n >= 8 && std::memcmp(p, XERIAL_MAGIC, 8) == 0; }

// The blocks of a records section p[0, n): one entry per xerial chunk, or one for a raw block --
// offset (relative to p) at the preamble, comp_bytes the chunk's length | SNAPPY_BLOCK.  blocks
// may be NULL or short (cap): *n_blocks counts them all.  YSB_OK, or YSB_ERR_FORMAT with the
// chunk's byte and the rule in err.
static inline int snappy_index(const u8* p, u64 n, ysb_lz4_frame_block* blocks, u64 cap, u64* n_blocks, SnappyError* err) {
    u64 nb = 0, pos = 0;
    auto refuse = [&](u64 at, const char* fmt, long long v) -> int {
        char rule[200];
        std::snprintf(rule, sizeof rule, fmt, v);
        err->at = at;
        std::snprintf(err->msg, sizeof err->msg, "snappy: byte %llu: %s", (unsigned long long)at, rule);
        *n_blocks = nb;
        return YSB_ERR_FORMAT;
    };
    auto block = [&](u64 at, u64 len) -> int {
        if (len > SNAPPY_MAX_COMP)
            return refuse(at, "a block of %lld bytes, above 76490, the format's bound for 65536 raw bytes", (long long)len);
        const u32 raw = snappy_raw_of(p + at, (u32)len);
        if (!raw) {
            u32 v = 0, nx = 0;
            SnappyHostIn src{p + at};
            if (!snappy_read_preamble(src, (u32)len, &v, &nx))
                return refuse(at, "the block's preamble is not a varint of at most 5 bytes below 2^32 (%lld bytes here)", (long long)len);
            return refuse(at, "a raw block of %lld bytes: blocks of 1..65536 raw bytes are read (have the producer use the Java "
                          "client's framing, whose chunks are 32 KiB, or a batch.size of at most 64 KiB)", (long long)v);
        }
        if (blocks && nb < cap) blocks[nb] = ysb_lz4_frame_block{at, (u32)len | SNAPPY_BLOCK, 0};
        ++nb;
        return YSB_OK;
    };
    if (snappy_is_xerial(p, n)) {
        if (n < XERIAL_HEADER) return refuse(8, "the xerial header is cut: %lld bytes of 16", (long long)n);
        const int32_t compat = (int32_t)snappy_be32(p + 12);
        if (compat != 1) return refuse(12, "xerial compatible version %lld: only 1 is read", compat);
        pos = XERIAL_HEADER;
        while (pos < n) {
            if (n - pos < 4) return refuse(pos, "%lld trailing bytes, shorter than a chunk's length word", (long long)(n - pos));
            const int32_t len = (int32_t)snappy_be32(p + pos);
            if (len <= 0) return refuse(pos, "chunk length %lld: not positive", len);
            if ((u64)len > n - pos - 4) return refuse(pos, "chunk length %lld runs past the records section", len);
            if (int rc = block(pos + 4, (u64)len)) return rc;
            pos += 4 + (u64)len;
        }
    } else {
        if (!n) return refuse(0, "an empty records section: no preamble (%lld bytes)", 0);
        if (int rc = block(0, n)) return rc;
    }
    *n_blocks = nb;
    return YSB_OK;
}

// What snappy_pack writes at the most for nbytes raw bytes (chunk: 0 takes XERIAL_CHUNK; raw
// framing takes one block).
static inline u64 snappy_pack_bound(u64 nbytes, u32 chunk, bool xerial) {
    if (!xerial) return 32 + nbytes + nbytes / 6;
    const u64 c = chunk ? chunk : XERIAL_CHUNK, chunks = (nbytes + c - 1) / c;
    return XERIAL_HEADER + nbytes + nbytes / 6 + chunks * 36;
}

// src[0, nbytes) as a xerial stream of chunks of `chunk` raw bytes (0: XERIAL_CHUNK; at most
// SNAPPY_MAX_RAW), or -- xerial false, 1 <= nbytes <= SNAPPY_MAX_RAW -- as one raw block.  dst
// holds snappy_pack_bound bytes; returns the size.
static inline u64 snappy_pack(const u8* src, u64 nbytes, u32 chunk, bool xerial, u8* dst) {
    if (!xerial) return snappy_compress_block(src, (u32)nbytes, dst);
    const u64 c = chunk ? (chunk < SNAPPY_MAX_RAW ? chunk : SNAPPY_MAX_RAW) : XERIAL_CHUNK;
    std::memcpy(dst, XERIAL_MAGIC, 8);
    snappy_put_be32(dst + 8, 1);
    snappy_put_be32(dst + 12, 1);
    u64 o = XERIAL_HEADER;
    for (u64 at = 0; at < nbytes; at += c) {
        const u32 len = (u32)(nbytes - at < c ? nbytes - at : c);
        const u32 z = snappy_compress_block(src + at, len, dst + o + 4);
        snappy_put_be32(dst + o, z);
        o += 4 + z;
    }
    return o;
}

#endif   // !__HIP_DEVICE_COMPILE__

}  // namespace ysb
