// ysb_lz4.h -- LZ4-compressed line batches (ysb_submit_raw_lz4, include/ysb_hip.h): what a
// source holds when its replay file, or its Kafka message sets (the reference's Kafka 0.8.2.1
// offers LZ4 as a message codec, stream-bench.sh), arrive compressed.  Instead of decoding them
// on a CPU in front of FileBasedDataSource.run (AdvertisingTopologyNative.java:144-165), the
// source hands the blocks over as they are; fewer bytes cross PCIe, the GPU decodes them.
//
// No HIP here: the format's rules in ONE sequence reader that the host model below and the
// kernel (ysb_lz4.hip) both call -- so "is this block valid" is written once --, the host
// decoder (a plain byte loop: the model), a small greedy compressor (test inputs, ysb_gen --lz4,
// the bench's batches; its ratio is not a goal), the directory's checks and the kernel's LDS
// geometry.  tests/native/lz4_logic.cpp runs all of it on the CPU.
//
// Format.  A batch is n_blocks independent LZ4 *blocks* back to back and a directory of
// ysb_lz4_block {comp_bytes, raw_bytes}; outputs are back to back in directory order.  Bit 31
// of comp_bytes marks a stored block (raw_bytes bytes as they are).  A block decodes to
// 1..65536 bytes.  A sequence is a token, the literal length's 255-extension bytes, the
// literals, a 2-byte little-endian offset in 1..65535 and the match length's extension bytes;
// the match length is the token's low nibble + 4 + extensions; the last sequence ends after its
// literals.  A match never reaches before its block's first byte.
#pragma once
#include <cstring>

#include "../../include/ysb_hip.h"
#include "ysb_common.h"

namespace ysb {

constexpr u32 LZ4_MAX_RAW = 65536;          // a block's raw size: 1..LZ4_MAX_RAW
constexpr u32 LZ4_STORED = 0x80000000u;     // comp_bytes bit 31
constexpr u32 LZ4_NO_BAD = 0xFFFFFFFFu;     // first_bad of a batch whose blocks are all valid

enum : u32 { LZ4_SEQ_MATCH = 0, LZ4_SEQ_LAST = 1, LZ4_SEQ_BAD = 2 };

// One sequence as the reader found it: lit_len literals at input position lit_pos, then (not in
// the last sequence) match_len bytes from `offset` bytes back; the next token is at `next`.
struct Lz4Seq {
    u32 lit_pos, lit_len, offset, match_len, next;
};

// A length's 255-extension bytes.  false: input exhausted inside them, or the length passed
// `cap` (then the literals or the match run past raw_bytes whatever follows -- and the sum
// cannot overflow: it stops at cap + 255).
template <class In>
YSB_HD bool lz4_read_ext(In& in, u32& ip, u32 comp, u32& len, u32 cap) {
    for (;;) {
        if (ip >= comp) return false;
        const u32 b = in.byte(ip++);
        len += b;
        if (len > cap) return false;
        if (b != 255) return true;
    }
}

// THE reader: the sequence whose token is at input position ip, of a block of `comp` compressed
// and `raw` raw bytes of which `op` are produced (op <= raw).  Every bounds rule is here:
//   input exhausted inside a token, an extension, the literals or the offset;
//   offset 0; an offset reaching before the block's start;
//   literals or a match running past raw_bytes;
//   the block ending with fewer (LAST with op + lit_len < raw) or more (input left when raw
//   bytes are out: the next sequence can only be empty literals at the input's end) bytes.
// It reads input only and copies nothing, so a caller copies exactly what it returns.  Every
// call consumes at least the token, so a walk over `comp` bytes ends.  In::byte(pos) is called
// with pos < comp only.
// measure (a frame's block, whose raw size nothing records: ysb_lz4_frame.h): `raw` is the cap
// (LZ4_MAX_RAW), not the size, and the end rule is ip == comp alone -- LAST then tells that the
// block decodes to op + lit_len bytes.  Every other rule is the same.
template <class In>
YSB_HD u32 lz4_read_seq(In& in, u32 ip, u32 comp, u32 op, u32 raw, Lz4Seq* s, bool measure = false) {
    if (ip >= comp) return LZ4_SEQ_BAD;
    const u32 tok = in.byte(ip++);
    u32 lit = tok >> 4;
    if (lit == 15 && !lz4_read_ext(in, ip, comp, lit, raw)) return LZ4_SEQ_BAD;
    if (lit > comp - ip || lit > raw - op) return LZ4_SEQ_BAD;
    s->lit_pos = ip;
    s->lit_len = lit;
    ip += lit;
    op += lit;
    s->offset = s->match_len = 0;
    s->next = ip;
    if (ip == comp) return (measure || op == raw) ? LZ4_SEQ_LAST : LZ4_SEQ_BAD;
    if (comp - ip < 2) return LZ4_SEQ_BAD;
    const u32 off = in.byte(ip) | (in.byte(ip + 1) << 8);
    ip += 2;
    if (off == 0 || off > op) return LZ4_SEQ_BAD;
    u32 ml = tok & 15;
    if (ml == 15 && !lz4_read_ext(in, ip, comp, ml, raw)) return LZ4_SEQ_BAD;
    ml += 4;
    if (ml > raw - op) return LZ4_SEQ_BAD;
    s->offset = off;
    s->match_len = ml;
    s->next = ip;
    return LZ4_SEQ_MATCH;
}

// A directory entry's own rule: raw_bytes in 1..LZ4_MAX_RAW (ysb_submit_raw_lz4 refuses the
// batch otherwise: YSB_ERR_ARG, not a bad block).
YSB_HD bool lz4_entry_ok(const ysb_lz4_block& e) { return e.raw_bytes >= 1 && e.raw_bytes <= LZ4_MAX_RAW; }
YSB_HD u32 lz4_entry_comp(const ysb_lz4_block& e) { return e.comp_bytes & ~LZ4_STORED; }
// A stored block is valid when it holds exactly raw_bytes bytes.
YSB_HD bool lz4_stored_ok(const ysb_lz4_block& e) { return lz4_entry_comp(e) == e.raw_bytes; }

// ---- the kernel's LDS geometry ----------------------------------------------------------
// The kernel decodes a block in place in LDS: its output grows from the window's start, its
// compressed bytes lie at the window's end, W = raw + lz4_margin(raw) bytes in all.  The write
// front never passes the read front for a block the reader accepts: a sequence of L literals
// and a match takes at most L + L / 255 + 3 + (match extensions) input bytes for at least L + 4
// + 255 * (match extensions - 1) output bytes, and the last sequence L + L / 255 + 2 for L; so
// what is left of the input never exceeds what is left of the output by more than raw / 255 + 2,
// and comp <= raw + raw / 255 + 2 <= W.  (The kernel still checks both and calls the block bad:
// for an accepted block the checks never fire -- tests/native/lz4_logic.cpp walks the corpus
// with them.)
YSB_HD u32 lz4_margin(u32 raw) { return raw / 128 + 16; }
YSB_HD u32 lz4_window(u32 raw) { return raw + lz4_margin(raw); }
// LDS bytes of a launch whose largest block decodes to max_raw bytes: 16 in front (the output
// starts at its global address mod 16) and 16 behind (so does the input), a multiple of 16.
YSB_HD u32 lz4_lds_bytes(u32 max_raw) { return (32 + lz4_window(max_raw) + 15) & ~15u; }

// ---- the several-wave kernel's LDS geometry (lz4_decode_wide_kernel) ----------------------
// The output block alone lies in LDS (16 bytes in front: it starts at its global address mod
// 16; the compressed bytes are streamed from global memory), behind it three buffers of
// LZ4W_BATCH sequence records (one is parsed while the one before has its literals copied and
// the one before that its matches) and nine control words.
constexpr u32 LZ4W_BATCH = 64;       // sequences per stage: one record per lane of a wave
constexpr u32 LZ4W_FIELDS = 5;       // literal position, literal length, output position, offset, match length
YSB_HD u32 lz4_wide_out_bytes(u32 max_raw) { return (32 + max_raw + 15) & ~15u; }
YSB_HD u32 lz4_wide_lds_bytes(u32 max_raw) { return lz4_wide_out_bytes(max_raw) + 3 * LZ4W_FIELDS * LZ4W_BATCH * 4 + 48; }
// launch_lz4_decode's choice when the context leaves it open (YSB_LZ4_DECODER_AUTO): the
// several-wave kernel for a batch whose largest block is above this many raw bytes (measured:
// DESIGN.md, LZ4 batches, "crossover").
constexpr u32 LZ4_WIDE_ABOVE = 16384;
YSB_HD u32 lz4_pick_decoder(u32 max_raw, u32 decoder) {
    if (decoder == YSB_LZ4_DECODER_NARROW || decoder == YSB_LZ4_DECODER_WIDE) return decoder;
    return max_raw > LZ4_WIDE_ABOVE ? (u32)YSB_LZ4_DECODER_WIDE : (u32)YSB_LZ4_DECODER_NARROW;
}

#if !defined(__HIP_DEVICE_COMPILE__)

// ---- host model -------------------------------------------------------------------------

struct Lz4HostIn {
    const u8* p;
    u32 byte(u32 pos) const { return p[pos]; }
};

// One block into out[0, raw_bytes).  false: invalid (out may hold a decoded prefix).
// in_place_ok (may be NULL) is cleared if the kernel's in-place checks would have fired.
static inline bool lz4_decode_block(const u8* in, const ysb_lz4_block& e, u8* out, bool* in_place_ok = nullptr) {
    if (!lz4_entry_ok(e)) return false;
    const u32 comp = lz4_entry_comp(e), raw = e.raw_bytes;
    if (e.comp_bytes & LZ4_STORED) {
        if (!lz4_stored_ok(e)) return false;
        std::memcpy(out, in, raw);
        return true;
    }
    if (in_place_ok && comp > lz4_window(raw)) *in_place_ok = false;
    const u64 in_base = (u64)lz4_window(raw) - comp;   // the input's place in the kernel's window
    Lz4HostIn src{in};
    u32 ip = 0, op = 0;
    for (;;) {
        Lz4Seq s;
        const u32 r = lz4_read_seq(src, ip, comp, op, raw, &s);
        if (r == LZ4_SEQ_BAD) return false;
        if (in_place_ok && op > in_base + s.lit_pos) *in_place_ok = false;
        for (u32 k = 0; k < s.lit_len; ++k) out[op + k] = in[s.lit_pos + k];
        op += s.lit_len;
        if (r == LZ4_SEQ_LAST) return true;
        if (in_place_ok && (u64)op + s.match_len > in_base + s.next) *in_place_ok = false;
        for (u32 k = 0; k < s.match_len; ++k) out[op + k] = out[op + k - s.offset];   // byte order: an overlap replicates
        op += s.match_len;
        ip = s.next;
    }
}

// The directory against the batch: 0, or which argument rule it breaks (the C ABI's messages).
enum : int { LZ4_DIR_OK = 0, LZ4_DIR_RAW = 1, LZ4_DIR_SUM = 2 };
static inline int lz4_check_dir(const ysb_lz4_block* dir, u32 n, u64 comp_bytes, u64* raw_total, u32* bad_entry) {
    u64 comp = 0, raw = 0;
    for (u32 i = 0; i < n; ++i) {
        if (!lz4_entry_ok(dir[i])) {
            if (bad_entry) *bad_entry = i;
            return LZ4_DIR_RAW;
        }
        comp += lz4_entry_comp(dir[i]);
        raw += dir[i].raw_bytes;
    }
    if (raw_total) *raw_total = raw;
    return comp == comp_bytes ? LZ4_DIR_OK : LZ4_DIR_SUM;
}

// A whole batch (its directory has passed lz4_check_dir) into out; returns the first bad block
// or LZ4_NO_BAD.  Like the kernel, a bad block writes nothing the caller may rely on and the
// blocks after it are decoded all the same.
static inline u32 lz4_decode_batch(const u8* in, const ysb_lz4_block* dir, u32 n, u8* out) {
    u32 first_bad = LZ4_NO_BAD;
    u64 ip = 0, op = 0;
    for (u32 i = 0; i < n; ++i) {
        if (!lz4_decode_block(in + ip, dir[i], out + op) && first_bad == LZ4_NO_BAD) first_bad = i;
        ip += lz4_entry_comp(dir[i]);
        op += dir[i].raw_bytes;
    }
    return first_bad;
}

// ---- host compressor --------------------------------------------------------------------
// Greedy, one hash table of 4-byte windows.  It obeys the format's end-of-block conventions
// (the last 5 bytes are literals, the last match starts at least 12 bytes before the end), so
// any LZ4 block decoder takes its output.

static inline u32 lz4_compress_bound(u32 raw) { return raw + raw / 255 + 16; }

static inline u32 lz4_put_len(u8* dst, u32 o, u32 len) {   // a length's extension bytes (len: what is above the nibble's 15)
    for (; len >= 255; len -= 255) dst[o++] = 255;
    dst[o++] = (u8)len;
    return o;
}

// src[0, n), 1 <= n <= LZ4_MAX_RAW, into dst (lz4_compress_bound(n) bytes at least); returns
// the compressed size.
static inline u32 lz4_compress_block(const u8* src, u32 n, u8* dst) {
    constexpr u32 HASH_BITS = 13;
    u32 table[1u << HASH_BITS] = {};   // position + 1 of the last window with this hash (0: none)
    auto rd32 = [&](u32 i) { u32 v; std::memcpy(&v, src + i, 4); return v; };
    u32 o = 0, anchor = 0, i = 0;
    auto emit = [&](u32 lit, u32 off, u32 ml) {   // ml 0: the last sequence
        const u32 m = ml ? ml - 4 : 0;
        dst[o++] = (u8)((lit < 15 ? lit : 15) << 4 | (m < 15 ? m : 15));
        if (lit >= 15) o = lz4_put_len(dst, o, lit - 15);
        std::memcpy(dst + o, src + anchor, lit);
        o += lit;
        if (!ml) return;
        dst[o++] = (u8)off;
        dst[o++] = (u8)(off >> 8);
        if (m >= 15) o = lz4_put_len(dst, o, m - 15);
    };
    while (n >= 13 && i <= n - 12) {
        const u32 v = rd32(i), h = (v * 2654435761u) >> (32 - HASH_BITS);
        const u32 cand = table[h];
        table[h] = i + 1;
        if (cand && rd32(cand - 1) == v) {   // (i - c <= 65535: positions are below 65536)
            const u32 c = cand - 1;
            u32 ml = 4;
            while (i + ml < n - 5 && src[c + ml] == src[i + ml]) ++ml;
            emit(i - anchor, i - c, ml);
            i += ml;
            anchor = i;
        } else {
            ++i;
        }
    }
    emit(n - anchor, 0, 0);
    return o;
}

// One block and its directory entry: compressed, or stored when that is allowed and the block
// did not shrink.  dst: lz4_compress_bound(n) bytes at least.
static inline ysb_lz4_block lz4_pack_block(const u8* src, u32 n, u8* dst, bool allow_stored) {
    const u32 c = lz4_compress_block(src, n, dst);
    if (allow_stored && c >= n) {
        std::memcpy(dst, src, n);
        return {n | LZ4_STORED, n};
    }
    return {c, n};
}

// Where the block that starts at `at` ends: block_bytes further on, or with line_aligned behind
// the last line terminator ('\n', or a '\r' not followed by '\n': ysb_split.hip's rule) inside
// that range -- if there is none (a line longer than a block), the block is cut where it is.
static inline u64 lz4_block_end(const u8* src, u64 n, u64 at, u32 block_bytes, bool line_aligned) {
    const u64 end = at + block_bytes < n ? at + block_bytes : n;
    if (!line_aligned || end == n) return end;
    for (u64 e = end; e > at; --e) {
        const u8 b = src[e - 1];
        if (b == '\n' || (b == '\r' && src[e] != '\n')) return e;   // (e < n here)
    }
    return end;
}

#endif   // !__HIP_DEVICE_COMPILE__

}  // namespace ysb
