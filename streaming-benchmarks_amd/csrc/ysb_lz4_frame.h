// ysb_lz4_frame.h -- standard LZ4 *frames* (ysb_lz4_frame_index, include/ysb_hip.h): what
// `lz4 -B4`, liblz4's LZ4F_*, Python's lz4.frame and a Kafka LZ4 codec write, next to the
// library's own block batches (ysb_lz4.h).  A frame records each block's compressed size only,
// so the batch directory's raw_bytes is unknown: the host reads one size word per block (the
// index, here) and a block's raw size comes from a walk of its tokens (lz4_measure_block here,
// lz4_measure_kernel on the GPU -- both call ysb_lz4.h's ONE sequence reader in measure mode).
//
// No HIP here, as in ysb_lz4.h: the frame rules (header, descriptor checksum, block words,
// every refusal), XXH32, the frame writer, the measure model and the carry rule of a stream of
// frame batches are written once; the C ABI and tests/native/lz4_frame_logic.cpp call this copy.
//
// Frame.  Magic 04 22 4D 18; FLG (version 01 in bits 7-6, B.Indep 5, B.Checksum 4, C.Size 3,
// C.Checksum 2, reserved 1, DictID 0); BD (block maximum id in bits 6-4: 4 = 64 KiB ... 7 =
// 4 MiB, the other bits 0); an 8-byte content size if flagged; a 4-byte dictionary id if
// flagged; HC = (XXH32(FLG .. the byte before HC, 0) >> 8) & 0xFF.  Then blocks: a 4-byte
// little-endian size word (bit 31: stored; 0: the EndMark), the data, a 4-byte checksum if
// B.Checksum; behind the EndMark a 4-byte content checksum if C.Checksum.  A skippable frame is
// a magic 50..5F 2A 4D 18, a 4-byte size and that many bytes.
#pragma once
#include <algorithm>
#include <cstdio>
#include <thread>
#include <vector>

#include "ysb_lz4.h"

namespace ysb {

// ---- the measure model ----------------------------------------------------------------------
// A frame block's raw size by its tokens alone: the reader in measure mode, LZ4_MAX_RAW as the
// cap, the end rule ip == comp.  0: bad (no raw size in 1..65536 makes the block valid).  A
// block is valid exactly when lz4_decode_block accepts it with the size returned here.
template <class In>
YSB_HD u32 lz4_measure_walk(In& in, u32 comp) {
    u32 ip = 0, op = 0;
    for (;;) {
        Lz4Seq s;
        const u32 r = lz4_read_seq(in, ip, comp, op, LZ4_MAX_RAW, &s, true);
        if (r == LZ4_SEQ_BAD) return 0;
        op += s.lit_len;
        if (r == LZ4_SEQ_LAST) return op;
        op += s.match_len;
        ip = s.next;
    }
}
}  // namespace ysb

#if !defined(__HIP_DEVICE_COMPILE__)

namespace ysb {

constexpr u32 LZ4F_MAGIC = 0x184D2204u;
constexpr u32 LZ4F_MAGIC_LEGACY = 0x184C2102u;
constexpr u32 LZ4F_MAGIC_SKIP = 0x184D2A50u;   // .. 0x184D2A5F
constexpr u32 LZ4F_BLOCK_MAX = 65536;          // BD id 4, the only block maximum accepted

// ---- XXH32 (the frame format's checksum; only the header's is verified) ---------------------
static inline u32 xxh_rotl(u32 x, int r) { return (x << r) | (x >> (32 - r)); }
static inline u32 xxh_rd32(const u8* p) { return (u32)p[0] | (u32)p[1] << 8 | (u32)p[2] << 16 | (u32)p[3] << 24; }
static inline u32 xxh32(const u8* p, u64 n, u32 seed) {
    constexpr u32 P1 = 2654435761u, P2 = 2246822519u, P3 = 3266489917u, P4 = 668265263u, P5 = 374761393u;
    const u8* const end = p + n;
    u32 h;
    if (n >= 16) {
        u32 v[4] = {seed + P1 + P2, seed + P2, seed, seed - P1};
        for (; end - p >= 16; p += 16)
            for (int k = 0; k < 4; ++k) v[k] = xxh_rotl(v[k] + xxh_rd32(p + 4 * k) * P2, 13) * P1;
        h = xxh_rotl(v[0], 1) + xxh_rotl(v[1], 7) + xxh_rotl(v[2], 12) + xxh_rotl(v[3], 18);
    } else {
        h = seed + P5;
    }
    h += (u32)n;
    for (; end - p >= 4; p += 4) h = xxh_rotl(h + xxh_rd32(p) * P3, 17) * P4;
    for (; p < end; ++p) h = xxh_rotl(h + *p * P5, 11) * P1;
    h ^= h >> 15; h *= P2; h ^= h >> 13; h *= P3; h ^= h >> 16;
    return h;
}

// ---- the index ------------------------------------------------------------------------------
struct Lz4fError {
    char msg[256] = {0};
};

// ysb_lz4_frame_index (include/ysb_hip.h says what is accepted and refused).  Returns YSB_OK,
// YSB_ERR_FORMAT or YSB_ERR_CAPACITY; err->msg names the byte offset and the rule.  Every read
// is guarded by need(): nothing at or past nbytes is touched.
static inline int lz4f_index(const u8* b, u64 nbytes, ysb_lz4_frame_block* blocks, u64 cap, u64* n_blocks,
                             ysb_lz4_frame_summary* info, Lz4fError* err) {
    ysb_lz4_frame_summary sum{};
    u64 at = 0, n = 0;
    auto bad = [&](u64 where, const char* rule) {
        std::snprintf(err->msg, sizeof err->msg, "LZ4 frame: byte %llu: %s", (unsigned long long)where, rule);
        if (n_blocks) *n_blocks = n;
        return YSB_ERR_FORMAT;
    };
    auto need = [&](u64 k) { return nbytes - at >= k; };   // (at <= nbytes always)
    while (at < nbytes) {
        if (!need(4)) return bad(at, "the buffer ends inside a frame's magic number");
        const u32 magic = xxh_rd32(b + at);
        if ((magic & 0xFFFFFFF0u) == LZ4F_MAGIC_SKIP) {
            if (!need(8)) return bad(at, "the buffer ends inside a skippable frame's size");
            const u64 size = xxh_rd32(b + at + 4);
            at += 8;
            if (!need(size)) return bad(at, "the buffer ends inside a skippable frame");
            at += size;
            ++sum.skippable_frames;
            continue;
        }
        if (magic == LZ4F_MAGIC_LEGACY)
            return bad(at, "the legacy frame magic 02 21 4C 18 (lz4 -l): not supported, write a standard frame");
        if (magic != LZ4F_MAGIC) return bad(at, "not an LZ4 frame magic (04 22 4D 18)");
        const u64 desc = at + 4;
        at = desc;
        if (!need(3)) return bad(at, "the buffer ends inside the frame descriptor");
        const u32 flg = b[at], bd = b[at + 1];
        if ((flg >> 6) != 1) return bad(at, "FLG: the version bits are not 01");
        if (flg & 0x02) return bad(at, "FLG: the reserved bit is set");
        if (bd & 0x8F) return bad(at + 1, "BD: reserved bits are set");
        const u64 hdr = 2 + ((flg & 0x08) ? 8 : 0) + ((flg & 0x01) ? 4 : 0);
        if (!need(hdr + 1)) return bad(at, "the buffer ends inside the frame descriptor");
        if ((u32)b[at + hdr] != ((xxh32(b + at, hdr, 0) >> 8) & 0xFF))
            return bad(at + hdr, "HC: the header checksum does not match the descriptor");
        if (!(flg & 0x20))
            return bad(at, "FLG: linked blocks (B.Indep = 0): a block's matches reach into the block before it; write "
                           "independent blocks (lz4 -BI, LZ4F_blockIndependent, block_linked=False)");
        if (flg & 0x01) return bad(at, "FLG: a dictionary id: dictionaries are not supported");
        const u32 bid = (bd >> 4) & 7;
        if (bid < 4) return bad(at + 1, "BD: a block maximum id below 4 is not defined");
        if (bid > 4) return bad(at + 1, "BD: a block maximum above 64 KiB; write 64 KiB blocks (lz4 -B4, LZ4F_max64KB)");
        if (flg & 0x08) {
            u64 cs = 0;
            for (int k = 7; k >= 0; --k) cs = cs << 8 | b[at + 2 + k];
            sum.content_bytes += cs;
            ++sum.content_sizes;
        }
        sum.block_checksums += (flg & 0x10) ? 1 : 0;
        sum.content_checksums += (flg & 0x04) ? 1 : 0;
        at += hdr + 1;
        for (;;) {
            if (!need(4)) return bad(at, "the buffer ends before the frame's EndMark");
            const u32 word = xxh_rd32(b + at);
            at += 4;
            if (word == 0) break;
            const u32 size = word & ~LZ4_STORED;
            if (size > LZ4F_BLOCK_MAX) return bad(at - 4, "a block size word above the frame's block maximum");
            if (size == 0) return bad(at - 4, "a stored block of no bytes");
            if (!need(size)) return bad(at, "the buffer ends inside a block");
            if (n < cap && blocks) blocks[n] = ysb_lz4_frame_block{at, word, 0};
            ++n;
            sum.stored_blocks += (word & LZ4_STORED) ? 1 : 0;
            sum.comp_bytes += size;
            at += size;
            if (flg & 0x10) {
                if (!need(4)) return bad(at, "the buffer ends inside a block checksum");
                at += 4;
            }
        }
        if (flg & 0x04) {
            if (!need(4)) return bad(at, "the buffer ends inside the content checksum");
            at += 4;
        }
        ++sum.frames;
    }
    sum.blocks = n;
    if (n_blocks) *n_blocks = n;
    if (info) *info = sum;
    if (n > cap) {
        std::snprintf(err->msg, sizeof err->msg, "LZ4 frame: %llu blocks, cap %llu", (unsigned long long)n,
                      (unsigned long long)cap);
        return YSB_ERR_CAPACITY;
    }
    return YSB_OK;
}

// ---- the measure model's host entry ---------------------------------------------------------
static inline u32 lz4_measure_block(const u8* in, u32 comp_field) {
    const u32 comp = comp_field & ~LZ4_STORED;
    if (comp_field & LZ4_STORED) return comp <= LZ4_MAX_RAW ? comp : 0;
    Lz4HostIn src{in};
    return lz4_measure_walk(src, comp);
}

// ---- the carry rule -------------------------------------------------------------------------
// ysb_lz4_frame_carry_cut: frame blocks end mid-line, so of a batch's bytes (the carry of the
// batch before in front) only those up to the last CERTAIN line terminator are lines.  A '\r'
// that is the buffer's last byte is not certain: the next batch may begin with the '\n' of the
// same terminator (BufferedReader.readLine takes "\r\n" as one), so the whole last line stays.
static inline u64 lz4f_carry_cut(const u8* d, u64 n, bool more) {
    if (!more) return n;
    for (u64 e = n; e > 0; --e) {
        const u8 c = d[e - 1];
        if (c == '\n' || (c == '\r' && e < n)) {
            return e;   // (a '\r' in front of a '\n' is never met: the scan comes to the '\n' first)
        }
    }
    return 0;
}

// ---- the writer -----------------------------------------------------------------------------
static inline u64 lz4f_bound(u64 nbytes, u32 block_bytes) {
    const u64 n = block_bytes ? (nbytes + block_bytes - 1) / block_bytes : 0;
    return 4 + 2 + 8 + 1 + nbytes + 4 * n + 4;   // (a block that did not shrink is stored: never above its raw size)
}

// src[0, nbytes) as one frame into dst (lz4f_bound bytes at least); returns its size.
static inline u64 lz4f_pack(const u8* src, u64 nbytes, u32 block_bytes, int threads, u8* dst) {
    auto wr32 = [](u8* p, u32 v) { for (int k = 0; k < 4; ++k) p[k] = (u8)(v >> (8 * k)); };
    u64 o = 0;
    wr32(dst, LZ4F_MAGIC);
    o = 4;
    dst[o++] = 0x40 | 0x20 | 0x08;   // version 01, independent blocks, content size
    dst[o++] = 4 << 4;               // 64 KiB block maximum
    for (int k = 0; k < 8; ++k) dst[o++] = (u8)(nbytes >> (8 * k));
    dst[o] = (u8)(xxh32(dst + 4, o - 4, 0) >> 8);
    ++o;
    const u64 n = (nbytes + block_bytes - 1) / block_bytes;
    // each block compressed into a buffer of its own, in parallel, then laid out in order
    std::vector<std::vector<u8>> comp(n);
    std::vector<ysb_lz4_block> ent(n);
    const int nt = (int)std::max<u64>(1, std::min<u64>({(u64)std::max(threads, 1), 16, n}));
    auto work = [&](int t) {
        for (u64 i = (u64)t; i < n; i += (u64)nt) {
            const u64 a = i * block_bytes;
            const u32 len = (u32)std::min<u64>(block_bytes, nbytes - a);
            comp[i].resize(lz4_compress_bound(len));
            ent[i] = lz4_pack_block(src + a, len, comp[i].data(), true);
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < nt; ++t) pool.emplace_back(work, t);
    work(0);
    for (auto& th : pool) th.join();
    for (u64 i = 0; i < n; ++i) {
        wr32(dst + o, ent[i].comp_bytes);
        o += 4;
        std::memcpy(dst + o, comp[i].data(), lz4_entry_comp(ent[i]));
        o += lz4_entry_comp(ent[i]);
    }
    wr32(dst + o, 0);   // EndMark
    return o + 4;
}

}  // namespace ysb

#endif   // !__HIP_DEVICE_COMPILE__
