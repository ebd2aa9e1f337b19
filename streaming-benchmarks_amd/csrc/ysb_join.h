// ysb_join.h -- the join's output as ordered columns (Kernel 7, ysb_scan_join.h; the calls:
// ysb_join_api.cpp, include/ysb_hip.h "joined views").  RedisJoinBolt.flatMap
// (flink-benchmarks/.../AdvertisingTopologyNative.java:460-474) emits a Tuple3(campaign_id,
// ad_id, event_time) for every view whose ad is in the map; ysb_join_device gives that stream
// for one device batch, in stream order, as columns in HBM.
//
// No HIP here: the output layout, the scratch format the three kernels share, the rank /
// prefix / clip plan -- which output rows a tile owns and what is written when cap_rows cuts a
// tile -- and a host model of the three launches on plain arrays that
// tests/native/join_logic.cpp runs on the CPU.
//
// The three launches (no workgroup waits for another, so the order of the output does not
// depend on scheduling):
//   a. join_kernel: lane i of a one-wave workgroup takes line i of a 64-line tile.  The tile's
//      joined mask is one ballot; a joined lane's rank is the popcount of the mask below it.
//      The tile's joined rows go, in rank order, into the tile's own block of the scratch area,
//      its count into tile_count[tile].
//   b. an exclusive prefix over tile_count.
//   c. join_pack_kernel: tile t moves its rows to rows [prefix[t], prefix[t] + count) of every
//      column, clipped at cap_rows.
//
// Scratch (context-owned, grown on first use): per tile one block of JOIN_TILE_BYTES (832)
// bytes, or JOIN_TILE_BYTES_KEYS (4480) with YSB_JOIN_KEYS, then tile_count and prefix, a u32
// each per tile: 13.125 bytes per line of the batch rounded up to whole tiles without keys --
// at most 16 -- and 70.125 with them -- at most 80.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "ysb_common.h"

namespace ysb {

constexpr u32 JOIN_TILE = 64;                       // lines per tile (the scan's TILE_LINES)
constexpr u64 JOIN_PAGE = 4096;                     // every column starts on a page, like Kernel 4's
constexpr u32 JOIN_KEYS = 1u;                       // YSB_JOIN_KEYS
constexpr u32 JOIN_KEY_STRIDE = MAX_KEY_BYTES;      // the key column's stride: PARK_KEY_STRIDE
constexpr u64 JOIN_MAX_ROWS = 0xFFFFFFFFull;        // rows are u32

// ---- the output layout ------------------------------------------------------------------
enum : u32 { JC_CAMPAIGN = 0, JC_ROW, JC_TIME, JC_TIME_OK, JC_KEY, JC_KEY_LEN, JC_COUNT_ };
YSB_HD u32 join_col_width(u32 c) {
    return c == JC_CAMPAIGN || c == JC_ROW ? 4u : c == JC_TIME ? 8u : c == JC_KEY ? JOIN_KEY_STRIDE : 1u;
}
YSB_HD u32 join_cols(u32 flags) { return (flags & JOIN_KEYS) ? (u32)JC_COUNT_ : (u32)JC_KEY; }
YSB_HD u64 join_page_align(u64 b) { return (b + JOIN_PAGE - 1) / JOIN_PAGE * JOIN_PAGE; }

// start[c]: column c's byte offset, each a multiple of the page; start[JC_COUNT_] the whole
// size.  A column the flags leave out is empty: it starts where the next one does.  false for
// unknown flags or more than 2^32 - 1 rows.
YSB_HD bool join_layout(u64 cap_rows, u32 flags, u64* start) {
    if ((flags & ~JOIN_KEYS) || cap_rows > JOIN_MAX_ROWS) return false;
    u64 at = 0;
    for (u32 c = 0; c < (u32)JC_COUNT_; ++c) {
        start[c] = at;
        if (c < join_cols(flags)) at += join_page_align((u64)join_col_width(c) * cap_rows);
    }
    start[JC_COUNT_] = at;
    return true;
}

// ---- the scratch format -----------------------------------------------------------------
// A tile's block holds its joined rows in rank order, one array per field: the campaigns, the
// times, one byte {line of the tile, bits 0-5; time_ok, bit 6} -- and with keys the key lengths
// and the keys at the column's stride.  Every array starts on a 16-byte boundary of a 16-byte
// aligned block, so both kernels move whole 16-byte vectors.
enum : u32 {
    JOIN_S_CAMP = 0, JOIN_S_TIME = JOIN_S_CAMP + 4 * JOIN_TILE, JOIN_S_LANE = JOIN_S_TIME + 8 * JOIN_TILE,
    JOIN_TILE_BYTES = JOIN_S_LANE + JOIN_TILE,
    JOIN_S_KLEN = JOIN_TILE_BYTES, JOIN_S_KEY = JOIN_S_KLEN + JOIN_TILE,
    JOIN_TILE_BYTES_KEYS = JOIN_S_KEY + JOIN_KEY_STRIDE * JOIN_TILE
};
static_assert(JOIN_S_TIME % 16 == 0 && JOIN_S_LANE % 16 == 0 && JOIN_S_KLEN % 16 == 0 && JOIN_S_KEY % 16 == 0 &&
                  JOIN_TILE_BYTES % 16 == 0 && JOIN_TILE_BYTES_KEYS % 16 == 0,
              "the scratch arrays are moved as 16-byte vectors");
static_assert(JOIN_TILE_BYTES + 8 <= 16 * JOIN_TILE && JOIN_TILE_BYTES_KEYS + 8 <= 80 * JOIN_TILE,
              "the scratch bound: 16 bytes per line, 80 with keys");

YSB_HD u32 join_tile_bytes(u32 flags) { return (flags & JOIN_KEYS) ? (u32)JOIN_TILE_BYTES_KEYS : (u32)JOIN_TILE_BYTES; }
YSB_HD u64 join_tiles(u64 n) { return (n + JOIN_TILE - 1) / JOIN_TILE; }
// the blocks, then tile_count[tiles], then prefix[tiles]
YSB_HD u64 join_scratch_counts(u64 n, u32 flags) { return join_tiles(n) * join_tile_bytes(flags); }
YSB_HD u64 join_scratch_bytes(u64 n, u32 flags) { return join_scratch_counts(n, flags) + join_tiles(n) * 8; }

// where field c of a tile's rows lies in its block (JC_ROW and JC_TIME_OK: the lane bytes)
YSB_HD u32 join_block_of(u32 c) {
    return c == JC_CAMPAIGN ? (u32)JOIN_S_CAMP : c == JC_TIME ? (u32)JOIN_S_TIME : c == JC_KEY ? (u32)JOIN_S_KEY
         : c == JC_KEY_LEN ? (u32)JOIN_S_KLEN : (u32)JOIN_S_LANE;
}
YSB_HD u8 join_lane_pack(u32 lane, bool time_ok) { return (u8)(lane | (time_ok ? 64u : 0u)); }
YSB_HD u32 join_lane_row(u64 tile, u32 b) { return (u32)(tile * JOIN_TILE + (b & 63u)); }
YSB_HD u8 join_lane_ok(u32 b) { return (u8)((b >> 6) & 1u); }

// ---- the rank / prefix / clip plan ------------------------------------------------------
// lane's rank among the tile's joined lanes
YSB_HD u32 join_rank(u64 mask, u32 lane) {
    u64 below = mask & (((u64)1 << lane) - 1);
    u32 r = 0;
    for (; below; below &= below - 1) ++r;
    return r;
}
// The output rows a tile owns: [first, first + count) of every column, the tile's `count` rows
// from output row `prefix` on, cut at cap_rows (a tile the capacity cuts writes its first
// cap_rows - prefix rows; a tile at or past it writes nothing).
struct JoinRun {
    u64 first;
    u32 count;
};
YSB_HD JoinRun join_run(u64 prefix, u32 count, u64 cap_rows) {
    JoinRun r;
    r.first = prefix < cap_rows ? prefix : cap_rows;
    const u64 room = cap_rows - r.first;
    r.count = (u64)count < room ? count : (u32)room;
    return r;
}
// A run of `bytes` bytes at byte `at` of a column (columns are 16-byte aligned) is stored as
// 16-byte vectors over [*a16, *b16) and narrower only at its ragged ends [at, *a16) and
// [*b16, at + bytes).
YSB_HD void join_span(u64 at, u64 bytes, u64* a16, u64* b16) {
    const u64 end = at + bytes, up = (at + 15) & ~(u64)15;
    *a16 = up < end ? up : end;
    const u64 down = end & ~(u64)15;
    *b16 = down > *a16 ? down : *a16;
}

// ---- host model -------------------------------------------------------------------------
// One line's outcome as join_kernel's lane holds it.
struct JoinLine {
    bool joined = false;
    u32 campaign = 0;
    i64 time = 0;          // 0 when !time_ok
    bool time_ok = false;
    u32 key_len = 0;
    u8 key[JOIN_KEY_STRIDE] = {};   // zero-padded
};

// a: the tiles' blocks and counts of lines[0, n) (scratch: join_scratch_bytes(n, flags) bytes)
inline void join_model_tiles(const JoinLine* lines, u64 n, u32 flags, u8* scratch) {
    const u32 tb = join_tile_bytes(flags);
    u32* count = reinterpret_cast<u32*>(scratch + join_scratch_counts(n, flags));
    for (u64 t = 0; t < join_tiles(n); ++t) {
        u64 mask = 0;
        const u32 rows = (u32)(n - t * JOIN_TILE < JOIN_TILE ? n - t * JOIN_TILE : JOIN_TILE);
        for (u32 l = 0; l < rows; ++l) mask |= (u64)(lines[t * JOIN_TILE + l].joined ? 1 : 0) << l;
        u8* blk = scratch + t * tb;
        for (u32 l = 0; l < rows; ++l) {
            const JoinLine& x = lines[t * JOIN_TILE + l];
            if (!x.joined) continue;
            const u32 r = join_rank(mask, l);
            memcpy(blk + JOIN_S_CAMP + 4 * r, &x.campaign, 4);
            memcpy(blk + JOIN_S_TIME + 8 * r, &x.time, 8);
            blk[JOIN_S_LANE + r] = join_lane_pack(l, x.time_ok);
            if (flags & JOIN_KEYS) {
                blk[JOIN_S_KLEN + r] = (u8)x.key_len;
                memcpy(blk + JOIN_S_KEY + JOIN_KEY_STRIDE * r, x.key, JOIN_KEY_STRIDE);
            }
        }
        count[t] = join_rank(mask, 63) + (u32)(mask >> 63);
    }
}

// b: prefix[t] = count[0] + ... + count[t - 1]; returns the total
inline u64 join_model_prefix(u64 n, u32 flags, u8* scratch) {
    const u32* count = reinterpret_cast<const u32*>(scratch + join_scratch_counts(n, flags));
    u32* prefix = const_cast<u32*>(count) + join_tiles(n);
    u64 run = 0;
    for (u64 t = 0; t < join_tiles(n); ++t) {
        prefix[t] = (u32)run;
        run += count[t];
    }
    return run;
}

// c: every tile's run into the columns of out (join_layout(cap_rows, flags)), 16-byte vectors
// over the aligned middle of a run and bytes at its ends; nothing else of out is touched
inline void join_model_pack(u64 n, u32 flags, const u8* scratch, u8* out, u64 cap_rows) {
    u64 start[JC_COUNT_ + 1];
    join_layout(cap_rows, flags, start);
    const u32 tb = join_tile_bytes(flags);
    const u32* count = reinterpret_cast<const u32*>(scratch + join_scratch_counts(n, flags));
    const u32* prefix = count + join_tiles(n);
    for (u64 t = 0; t < join_tiles(n); ++t) {
        const JoinRun run = join_run(prefix[t], count[t], cap_rows);
        const u8* blk = scratch + t * tb;
        for (u32 c = 0; c < join_cols(flags) && run.count; ++c) {
            const u32 w = join_col_width(c);
            std::vector<u8> src((size_t)run.count * w);
            for (u32 r = 0; r < run.count; ++r) {
                const u32 b = blk[JOIN_S_LANE + r];
                if (c == JC_ROW) { const u32 row = join_lane_row(t, b); memcpy(&src[4 * r], &row, 4); }
                else if (c == JC_TIME_OK) src[r] = join_lane_ok(b);
                else memcpy(&src[(size_t)w * r], blk + join_block_of(c) + w * r, w);
            }
            const u64 at = run.first * w, bytes = (u64)run.count * w;
            u64 a16, b16;
            join_span(at, bytes, &a16, &b16);
            u8* col = out + start[c];
            for (u64 p = at; p < a16; ++p) col[p] = src[p - at];
            for (u64 p = a16; p < b16; p += 16) memcpy(col + p, &src[p - at], 16);
            for (u64 p = b16; p < at + bytes; ++p) col[p] = src[p - at];
        }
    }
}

}  // namespace ysb
