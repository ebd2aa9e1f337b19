// ysb_kafka_crc.h -- CRC-32C (Castagnoli, reflected 0x82F63B78, init and final xor 0xFFFFFFFF) as
// arithmetic in GF(2)[x] / P: what kafka_crc_kernel (ysb_kafka.hip) computes a record batch's
// checksum with, 64 lanes at a time, and what the host's kafka_crc32c slices with.  No HIP here:
// the kernel and the host model (kafka_crc_lanes_host) call the same pieces, and
// tests/native/kafka_crc_logic.cpp runs all of it on the CPU.
//
// The raw register (no init, no final xor) of a message M is reg(M) = M(x) * x^32 mod P, kept
// reflected: bit 31 is x^0, bit 0 is x^31.  Three identities carry the layout:
//   1. reg(A || B) = reg(A) * x^(8|B|) + reg(B): the CRC is linear over GF(2).
//   2. Zero bytes in front of a message leave a zero register as it is, so a range at any byte
//      address is treated as left-padded with zeros to the grid of 16-byte vectors.
//   3. The init value is a register of 0xFFFFFFFF in front of the first byte.  That is the register
//      four bytes K = 0xFFFFFFFF * x^-32 leave behind them (reg(K) = K * x^32), so the init costs
//      no x^(8n): the four bytes in front of the range are read AS K.  In a record batch those
//      four bytes are the stored CRC's own field, which the kernel loads anyway.
//
// The layout.  The range's vectors [0, span) are cut into windows of CRC_WIN = 1024 bytes, right-
// aligned on the last vector's end; lane i owns the i-th vector of every window and keeps a
// register s_i.  Per window s_i <- reg-process(s_i, own 16 bytes || 1008 zero bytes): ONE round of
// 16 independent lookups in slicing tables built for a distance of 1024 bytes (table j, entry v:
// reg(v || 1023 - j zero bytes)), the first four own bytes xored with s_i in front.  Behind the
// last window lane i's register stands 16 i bytes behind the last vector's end, which lies z <
// 16 bytes behind the range's end: one multiplication by the constant x^(-8 (16 i + z)) (x is
// invertible: P's constant term is 1), an xor over the lanes, the final xor.
#pragma once
#include "ysb_common.h"

namespace ysb {

constexpr u32 CRC32C_POLY = 0x82F63B78u;
constexpr u32 CRC_ONE = 0x80000000u;     // x^0
constexpr u32 CRC_X8 = 0x00800000u;      // x^8
constexpr u32 CRC_WIN = 1024;            // a window: KAFKA_WIN, one 16-byte vector per lane
constexpr u32 CRC_LANES = 64;
constexpr u32 CRC_TABLE_WORDS = 16 * 256;                    // sixteen slicing tables
constexpr u32 CRC_CONST_WORDS = 16 * CRC_LANES;              // x^(-8 (16 i + z)) at [z * 64 + i]
constexpr u32 KAFKA_CRC_STORED = 44;     // the stored CRC lies this far in front of the first record byte ...
constexpr u32 KAFKA_CRC_COVERED = 40;    // ... and the range begins this far in front of it (`attributes`)

YSB_HD constexpr u32 crc_mulx(u32 a) { return (a >> 1) ^ ((a & 1u) ? CRC32C_POLY : 0u); }
YSB_HD constexpr u32 crc_divx(u32 a) { return (a & CRC_ONE) ? (((a ^ CRC32C_POLY) << 1) | 1u) : (a << 1); }
// a * b mod P: 32 shift-xor steps
YSB_HD constexpr u32 crc_mulmod(u32 a, u32 b) {
    u32 p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (CRC_ONE >> i)) p ^= b;
        b = crc_mulx(b);
    }
    return p;
}
YSB_HD constexpr u32 crc_pow(u32 base, u64 n) {
    u32 r = CRC_ONE;
    while (n) {
        if (n & 1) r = crc_mulmod(r, base);
        base = crc_mulmod(base, base);
        n >>= 1;
    }
    return r;
}
YSB_HD constexpr u32 crc_x8_inv() {
    u32 a = CRC_ONE;
    for (int i = 0; i < 8; ++i) a = crc_divx(a);
    return a;
}
YSB_HD constexpr u32 crc_xpow8(u64 n) { return crc_pow(CRC_X8, n); }            // x^(8n)
YSB_HD constexpr u32 crc_xpow8_inv(u64 n) { return crc_pow(crc_x8_inv(), n); }  // x^(-8n)
// the register one byte leaves: the bitwise definition, eight steps
YSB_HD constexpr u32 crc_byte(u32 v) {
    for (int k = 0; k < 8; ++k) v = crc_mulx(v);
    return v;
}
// identity 1
YSB_HD constexpr u32 crc_combine(u32 reg_a, u32 reg_b, u64 len_b) { return crc_mulmod(reg_a, crc_xpow8(len_b)) ^ reg_b; }
// identity 3: the four bytes (little-endian) that leave 0xFFFFFFFF behind them
constexpr u32 CRC_INIT_BYTES = crc_mulmod(0xFFFFFFFFu, crc_xpow8_inv(4));

// The table generator: t[j * 256 + v] = reg(v || dist - 1 - j zero bytes), j < 16.  dist 16: the
// usual slicing-by-16 tables (the host's); dist CRC_WIN: the kernel's.
inline void crc_fill_tables(u32* t, u32 dist) {
    for (u32 j = 0; j < 16; ++j) {
        const u32 m = crc_xpow8(dist - 1 - j);
        for (u32 v = 0; v < 256; ++v) t[j * 256 + v] = crc_mulmod(crc_byte(v), m);
    }
}
inline void crc_fill_consts(u32* c) {
    for (u32 z = 0; z < 16; ++z)
        for (u32 i = 0; i < CRC_LANES; ++i) c[z * CRC_LANES + i] = crc_xpow8_inv(16 * i + z);
}

struct CrcVec {
    u32 w[4];   // sixteen bytes, little-endian words
};
// One round: the register s in front of the sixteen bytes v, by the tables t (any distance).
YSB_HD u32 crc_step16(const u32* t, u32 s, const CrcVec& v) {
    const u32 a = v.w[0] ^ s, b = v.w[1], c = v.w[2], d = v.w[3];
    return t[0 * 256 + (a & 255)] ^ t[1 * 256 + ((a >> 8) & 255)] ^ t[2 * 256 + ((a >> 16) & 255)] ^ t[3 * 256 + (a >> 24)] ^
           t[4 * 256 + (b & 255)] ^ t[5 * 256 + ((b >> 8) & 255)] ^ t[6 * 256 + ((b >> 16) & 255)] ^ t[7 * 256 + (b >> 24)] ^
           t[8 * 256 + (c & 255)] ^ t[9 * 256 + ((c >> 8) & 255)] ^ t[10 * 256 + ((c >> 16) & 255)] ^ t[11 * 256 + (c >> 24)] ^
           t[12 * 256 + (d & 255)] ^ t[13 * 256 + ((d >> 8) & 255)] ^ t[14 * 256 + ((d >> 16) & 255)] ^ t[15 * 256 + (d >> 24)];
}

// A range's place on the vector grid.  Offsets count from g0, the 16-byte boundary at or in
// front of the first byte that may be loaded (`pre` bytes in front of the range, which a record
// batch has: the stored CRC; 0 for a bare range).  [lo, hi) is the range, [lo - 4, lo) reads as
// CRC_INIT_BYTES, everything else in the vectors [0, span) as zero.  Where fewer than four bytes
// lie between g0 and the range the grid begins one vector earlier: a vector that is never loaded
// (`first` = 16; the loader maps offset o >= first to g0 + o - first).
struct CrcGrid {
    u32 first, lo, hi, span, windows, z;
};
YSB_HD CrcGrid crc_grid(u64 addr, u32 pre, u32 n) {
    CrcGrid g;
    const u32 mis = (u32)(addr & 15);
    g.first = mis + pre < 4 ? 16u : 0u;
    g.lo = g.first + mis + pre;
    g.hi = g.lo + n;
    g.span = (g.hi + 15) & ~15u;
    g.z = g.span - g.hi;
    g.windows = (g.span + CRC_WIN - 1) / CRC_WIN;
    return g;
}
// lane i's vector of window w (may be negative: a vector of leading zeros, never loaded)
YSB_HD i64 crc_vec_off(const CrcGrid& g, u32 w, u32 lane) {
    return (i64)g.span - (i64)(g.windows - w) * CRC_WIN + 16 * (i64)lane;
}
YSB_HD bool crc_is_edge(const CrcGrid& g, u32 off) { return off < g.lo || off + 16 > g.hi; }
// a vector that holds bytes outside the range: those are masked, never trusted
YSB_HD void crc_edge(const CrcGrid& g, u32 off, CrcVec* v) {
    for (u32 b = 0; b < 16; ++b) {
        const u32 p = off + b, sh = 8 * (b & 3);
        u32 byte = (v->w[b >> 2] >> sh) & 255u;
        if (p < g.lo || p >= g.hi) byte = (p + 4 >= g.lo && p < g.lo) ? (CRC_INIT_BYTES >> (8 * (p + 4 - g.lo))) & 255u : 0u;
        v->w[b >> 2] = (v->w[b >> 2] & ~(255u << sh)) | (byte << sh);
    }
}
// behind the last window: lane i's share of the range's register
YSB_HD u32 crc_lane_finish(const u32* consts, const CrcGrid& g, u32 lane, u32 s) { return crc_mulmod(s, consts[g.z * CRC_LANES + lane]); }

#if !defined(__HIP_DEVICE_COMPILE__)

struct CrcTables {
    u32 slice16[CRC_TABLE_WORDS];   // distance 16: kafka_crc32c
    u32 win[CRC_TABLE_WORDS];       // distance CRC_WIN: the kernel's, copied to the device once per context
    u32 consts[CRC_CONST_WORDS];
    CrcTables() {
        crc_fill_tables(slice16, 16);
        crc_fill_tables(win, CRC_WIN);
        crc_fill_consts(consts);
    }
};
inline const CrcTables& crc_tables() {
    static const CrcTables T;
    return T;
}

// CRC-32C of p[0, n), continuing from crc: sixteen bytes a round by the distance-16 tables, the
// rest a byte at a time (table 15 is the byte table: reg(v), no zero byte behind it).
inline u32 kafka_crc32c(const u8* p, u64 n, u32 crc = 0) {
    const u32* t = crc_tables().slice16;
    crc = ~crc;
    for (; n >= 16; p += 16, n -= 16) {
        CrcVec v;
        for (int k = 0; k < 4; ++k)
            v.w[k] = (u32)p[4 * k] | (u32)p[4 * k + 1] << 8 | (u32)p[4 * k + 2] << 16 | (u32)p[4 * k + 3] << 24;
        crc = crc_step16(t, crc, v);
    }
    for (u64 i = 0; i < n; ++i) crc = t[15 * 256 + ((crc ^ p[i]) & 255)] ^ (crc >> 8);
    return ~crc;
}

// The kernel's decomposition as a plain loop over 64 "lanes": CRC-32C of p[0, n), where `pre`
// bytes in front of p may be read (0 or more; their values never matter).  Only the 16-byte
// vectors, by p's address, that hold [p - pre, p + n) are read.
inline u32 kafka_crc_lanes_host(const u8* p, u32 pre, u32 n) {
    const CrcTables& T = crc_tables();
    const u8* from = p - pre;
    const CrcGrid g = crc_grid((u64)reinterpret_cast<uintptr_t>(from), pre, n);
    const u8* g0 = from - (reinterpret_cast<uintptr_t>(from) & 15);
    u32 total = 0;
    for (u32 lane = 0; lane < CRC_LANES; ++lane) {
        u32 s = 0;
        for (u32 w = 0; w < g.windows; ++w) {
            const i64 off = crc_vec_off(g, w, lane);
            CrcVec v{{0, 0, 0, 0}};
            if (off >= (i64)g.first) {
                const u8* q = g0 + (off - g.first);
                for (int k = 0; k < 4; ++k)
                    v.w[k] = (u32)q[4 * k] | (u32)q[4 * k + 1] << 8 | (u32)q[4 * k + 2] << 16 | (u32)q[4 * k + 3] << 24;
            }
            if (off >= 0 && crc_is_edge(g, (u32)off)) crc_edge(g, (u32)off, &v);
            s = crc_step16(T.win, s, v);
        }
        total ^= crc_lane_finish(T.consts, g, lane, s);
    }
    return ~total;
}

#endif  // !__HIP_DEVICE_COMPILE__

}  // namespace ysb
