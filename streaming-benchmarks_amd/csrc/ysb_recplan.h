// ysb_recplan.h -- record mode's plan (ysb_count.hip): the geometry of one launch as pure
// integer arithmetic, no HIP, so tests/native/recplan_logic.cpp checks it with g++ alone.
//
// A launch of `grid` scan workgroups over c_pad campaigns x W ring slots:
//   level-2 block   L2C = REC_BLOCK_CELLS / W campaigns (block = campaign >> blk_shift): its
//                   L2C x W cells are one count workgroup's LDS counters;
//   level-1 bin     S = 1 << sub_log2 consecutive blocks (bin = campaign >> (blk_shift +
//                   sub_log2)), at most REC_BINS_MAX bins of at most REC_SUB_MAX blocks;
//   sub-buffer      cap records per (scan workgroup, bin), a multiple of 32 (one 128-B line);
//   area            u32 words of one (bin, slice) partition output: the slice's sub-buffers
//                   full, plus a 32-record alignment pad per block.
// What the plan cannot hold (a ring wider than a block, more blocks than the bins take,
// cell or record indices past 32 bits) stays with the atomics: rec_plan returns false.
#pragma once
#include "ysb_common.h"

namespace ysb {

#ifndef YSB_TILE_LINES
#define YSB_TILE_LINES 64
#endif
// lines per tile: one per lane (fewer than 64 leaves lanes idle but shrinks the LDS tile,
// so more workgroups fit a CU)
constexpr int TILE_LINES = YSB_TILE_LINES;
#ifndef YSB_MAX_TILES
#define YSB_MAX_TILES 128
#endif
constexpr int MAX_TILES_PER_BLOCK = YSB_MAX_TILES;   // tile bounds preloaded into LDS

constexpr int REC_BINS_MAX = 8;       // level-1 bins of the scan's record staging
constexpr int REC_BLOCK_CELLS = 32768;  // u32 LDS counters per count workgroup (128 KiB)
#ifndef YSB_REC_QUARTERS
#define YSB_REC_QUARTERS 64
#endif
constexpr int REC_QUARTERS = YSB_REC_QUARTERS;   // partition workgroups per level-1 bin (each a slice of the scan workgroups)
constexpr int REC_SUB_MAX = 512;      // level-2 blocks per level-1 bin (the partition's staging rings)
constexpr int REC_SLICE_MAX = 128;    // scan workgroups per partition slice

YSB_HD u32 log2u(u64 x) { u32 l = 0; while (((u64)1 << l) < x) ++l; return l; }

struct RecPlan {
    u32 w_log2;                 // log2 W
    u32 blk_shift;              // block = campaign >> blk_shift (L2C = 1 << blk_shift)
    u32 n_blocks;               // ceil(c_pad / L2C)
    u32 sub_log2;               // level-2 blocks per level-1 bin = 1 << sub_log2
    u32 bins;                   // level-1 bins
    u32 cap;                    // records per sub-buffer
    u64 area;                   // u32 words of one (bin, slice) output area
    u64 part;                   // u32 words of the partitioned records: bins * REC_QUARTERS * area
};

// The plan of a launch of `grid` scan workgroups, each scanning at most tiles_per_wg_max
// tiles, over c_pad campaigns x W ring slots (W a power of two >= 16); false where record
// mode cannot run.
YSB_HD bool rec_plan(u32 c_pad, u32 W, u32 grid, u64 tiles_per_wg_max, RecPlan* out) {
    const u64 cells = (u64)c_pad * W;
    if (cells >= (1ull << 32) || W > (u32)REC_BLOCK_CELLS) return false;
    RecPlan r{};
    r.w_log2 = log2u(W);
    r.blk_shift = log2u(REC_BLOCK_CELLS / W);
    r.n_blocks = (u32)((c_pad + (1u << r.blk_shift) - 1) >> r.blk_shift);
    const u32 sub = (r.n_blocks + REC_BINS_MAX - 1) / REC_BINS_MAX;
    r.sub_log2 = log2u(sub);
    if ((1u << r.sub_log2) > (u32)REC_SUB_MAX) return false;   // beyond 8 x 512 blocks: atomics
    r.bins = (r.n_blocks + (1u << r.sub_log2) - 1) >> r.sub_log2;
    if ((grid + REC_QUARTERS - 1) / REC_QUARTERS > (u32)REC_SLICE_MAX) return false;
    // lines one workgroup scans at most in this launch; ~1/3 are joined views on generator
    // data; 3/4 of the lines spread over the bins leaves room for skew (a full sub-buffer
    // sends the rest of its views to the atomics: slower, still exact)
    const u64 lines = tiles_per_wg_max * TILE_LINES;
    u64 cap = (lines * 3 / 4 + r.bins - 1) / r.bins;
    cap = cap > 32 ? (cap + 31) / 32 * 32 : 32;
    // one (bin, slice) output area: the slice's sub-buffers plus a 32-record alignment pad per block
    const u64 area = ((u64)((grid + REC_QUARTERS - 1) / REC_QUARTERS) * cap + 32ull * (1u << r.sub_log2) + 31) / 32 * 32;
    const u64 part = (u64)r.bins * REC_QUARTERS * area;
    if (cap > 0xFFFFFFFFull || part >= (1ull << 32)) return false;
    r.cap = (u32)cap;
    r.area = area;
    r.part = part;
    *out = r;
    return true;
}

}  // namespace ysb
