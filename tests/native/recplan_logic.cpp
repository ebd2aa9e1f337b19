// Host-side checks of record mode's plan (ysb_recplan.h): the geometry rec_plan gives a launch
// -- level-2 blocks, level-1 bins, the sub-buffer capacity, the partition's output areas --
// over every ring width, the campaign counts around every block and bin boundary, grids around
// the slice limits and the tile counts a workgroup can hold.  For every accepted plan: the
// invariants the scan, partition and count kernels index by; and acceptance exactly up to each
// limit (a ring wider than a block, more blocks than the bins hold, 2^32 cells, 128 scan
// workgroups per slice, 2^32 words of partition output), restated here independently.
// Built and run by tests/test_capi.py with g++ (no GPU, no library).
#include <cstdio>
#include <set>
#include <vector>
#include "ysb_recplan.h"

using namespace ysb;

static int fails = 0;
static unsigned long long checked = 0, accepted = 0;
#define CHECK(c) do { if (!(c)) { if (++fails <= 40) std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); } } while (0)
#define CHECKF(c, ...) do { if (!(c)) { if (++fails <= 40) { std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static const u64 TWO32 = 1ull << 32;
static const u32 NONE = 0xFFFFFFFFu;   // ysb_count.hip REC_NONE: no record

// The plan restated: plain 64-bit arithmetic from the description in ysb_recplan.h.
struct Model {
    bool ok;
    u64 l2c, n_blocks, S, bins, slices, cap, area, part;
};
static Model model(u64 c_pad, u64 W, u64 grid, u64 tiles) {
    Model m{};
    if (W > (u64)REC_BLOCK_CELLS || c_pad * W >= TWO32) return m;
    m.l2c = (u64)REC_BLOCK_CELLS / W;
    m.n_blocks = (c_pad + m.l2c - 1) / m.l2c;
    m.S = 1;
    while (m.S * REC_BINS_MAX < m.n_blocks) m.S *= 2;   // the smallest power of two whose 8 bins hold the blocks
    if (m.S > (u64)REC_SUB_MAX) return m;
    m.bins = (m.n_blocks + m.S - 1) / m.S;
    m.slices = (grid + REC_QUARTERS - 1) / REC_QUARTERS;
    if (m.slices > 128) return m;
    const u64 per_bin = (tiles * TILE_LINES * 3 / 4 + m.bins - 1) / m.bins;
    m.cap = per_bin <= 32 ? 32 : (per_bin + 31) / 32 * 32;
    m.area = (m.slices * m.cap + 32 * m.S + 31) / 32 * 32;
    m.part = m.bins * REC_QUARTERS * m.area;
    if (m.part >= TWO32) return m;
    m.ok = true;
    return m;
}

static void check_plan(u32 c_pad, u32 W, u32 grid, u64 tiles) {
    ++checked;
    RecPlan p{};
    const bool ok = rec_plan(c_pad, W, grid, tiles, &p);
    const Model m = model(c_pad, W, grid, tiles);
    CHECKF(ok == m.ok, "c_pad %u W %u grid %u tiles %llu: rec_plan %d, model %d", c_pad, W, grid,
           (unsigned long long)tiles, (int)ok, (int)m.ok);
    if (!ok || !m.ok) return;
    ++accepted;
    const u64 S = 1ull << p.sub_log2, L2C = 1ull << p.blk_shift;
    // the model's numbers
    CHECK((1ull << p.w_log2) == W);
    CHECK(L2C == m.l2c && p.n_blocks == m.n_blocks && S == m.S && p.bins == m.bins);
    CHECKF(p.cap == m.cap && p.area == m.area && p.part == m.part, "c_pad %u W %u grid %u tiles %llu: cap %u/%llu area %llu/%llu",
           c_pad, W, grid, (unsigned long long)tiles, p.cap, (unsigned long long)m.cap, (unsigned long long)p.area,
           (unsigned long long)m.area);
    // bins and blocks: the scan's staging (REC_BINS_MAX rings), the partition's (REC_SUB_MAX rings)
    CHECK(p.bins >= 1 && p.bins <= (u32)REC_BINS_MAX);
    CHECK(S <= (u64)REC_SUB_MAX);
    CHECK(((u64)p.bins << p.sub_log2) >= p.n_blocks && p.n_blocks > ((u64)(p.bins - 1) << p.sub_log2));
    // every campaign has a bin
    CHECK(((u64)(c_pad - 1) >> (p.blk_shift + p.sub_log2)) < p.bins);
    // the last block holds a campaign; a block's cells are one count workgroup's counters
    CHECK(((u64)(p.n_blocks - 1) << p.blk_shift) < c_pad);
    CHECK(((u64)p.n_blocks << p.blk_shift) >= c_pad);
    CHECK(L2C * W == (u64)REC_BLOCK_CELLS);
    // whole 128-B lines
    CHECK(p.cap >= 32 && p.cap % 32 == 0);
    CHECK(p.area % 32 == 0);
    // the area bound: no slice holds more scan workgroups than ceil(grid / REC_QUARTERS); with all of
    // them full and every one of the S blocks wasting a 31-record alignment pad the runs still fit
    u64 widest = 0, covered = 0;
    for (u32 q = 0; q < (u32)REC_QUARTERS; ++q) {
        const u64 lo = (u64)q * grid / REC_QUARTERS, hi = (u64)(q + 1) * grid / REC_QUARTERS;
        widest = hi - lo > widest ? hi - lo : widest;
        covered += hi - lo;
    }
    CHECK(covered == grid && widest == m.slices);
    CHECK(widest <= 128);
    CHECK(widest * p.cap + 31 * S <= p.area);
    // the worst split of those records over the blocks: S - 1 blocks of one record, the rest in one
    if (widest * p.cap >= S) {
        const u64 big = widest * p.cap - (S - 1);
        CHECK((S - 1) * 32 + (big + 31) / 32 * 32 <= p.area);
    }
    CHECK((u64)p.bins * REC_QUARTERS * p.area == p.part && p.part < TWO32);
    // every ring cell index campaign * W + slot fits a u32 and is not the "no record" value
    CHECK((u64)(c_pad - 1) * W + (W - 1) < (u64)NONE);
}

int main() {
    const u32 grids[] = {1, 2, 63, 64, 65, 2047, 2048, 8192, 8193};
    const u64 tiles[] = {1, 2, 3, 37, (u64)MAX_TILES_PER_BLOCK};
    for (u32 W = 16; W <= 65536; W <<= 1) {
        std::set<u64> cs = {1, 129, 200000, 200001, 1000000, (TWO32 - 1) / W, (TWO32 - 1) / W + 1};
        const u64 l2c = W <= (u32)REC_BLOCK_CELLS ? (u64)REC_BLOCK_CELLS / W : 1;
        for (u64 k = 1; k <= 70; ++k)
            for (int e = -1; e <= 1; ++e) cs.insert(k * l2c + e);
        for (u64 S = 1; S <= 2 * (u64)REC_SUB_MAX; S *= 2)   // every bin boundary of every bin size, and one size too many
            for (u64 b = 1; b <= (u64)REC_BINS_MAX; ++b)
                for (int e = -1; e <= 1; ++e) cs.insert(b * S * l2c + e);
        for (u64 c : cs) {
            if (c < 1 || c > 0xFFFFFFFFull) continue;
            for (u32 g : grids)
                for (u64 t : tiles) check_plan((u32)c, W, g, t);
        }
    }
    RecPlan p{};
    // each limit, both sides
    CHECK(rec_plan(1, 32768, 64, 1, &p) && p.blk_shift == 0 && p.n_blocks == 1);           // W == REC_BLOCK_CELLS
    CHECK(!rec_plan(1, 65536, 64, 1, &p));                                                  // W > REC_BLOCK_CELLS
    CHECK(rec_plan(4096u * 2048u, 16, 64, 1, &p) && p.sub_log2 == 9 && p.bins == 8);        // S == REC_SUB_MAX
    CHECK(!rec_plan(4096u * 2048u + 1, 16, 64, 1, &p));                                     // S > REC_SUB_MAX
    CHECK(rec_plan(4096, 32768, 64, 1, &p) && p.sub_log2 == 9 && !rec_plan(4097, 32768, 64, 1, &p));
    // 2^32 cells: beyond 8 x 512 blocks of 32768 cells already (2^27), so never the first limit to
    // bind; rejected on both sides of it, and no 32-bit wrap in between
    for (u32 W = 16; W <= 32768; W <<= 1) {
        const u64 c = (TWO32 - 1) / W;
        CHECK(c * W < TWO32 && (c + 1) * W >= TWO32);
        CHECK(!rec_plan((u32)c, W, 64, 1, &p) && !rec_plan((u32)(c + 1), W, 64, 1, &p));
        CHECK(!rec_plan(0xFFFFFFFFu, W, 64, 1, &p));
    }
    CHECK(rec_plan(200000, 16, 128 * 64, 3, &p) && !rec_plan(200000, 16, 128 * 64 + 1, 3, &p));   // 128 scan workgroups per slice
    // 2^32 words of partition output: the tiles per workgroup at which it is reached (far past
    // what a launch can hold: 16 segments of MAX_TILES_PER_BLOCK + 1 tiles), found on the model
    for (u32 c_pad : {129u, 16384u, 200000u}) {
        u64 lo = 1, hi = 1ull << 40;   // model(lo) accepts, model(hi) rejects
        CHECK(model(c_pad, 16, 8192, lo).ok && !model(c_pad, 16, 8192, hi).ok);
        while (hi - lo > 1) {
            const u64 mid = lo + (hi - lo) / 2;
            (model(c_pad, 16, 8192, mid).ok ? lo : hi) = mid;
        }
        CHECK(lo > 16ull * (MAX_TILES_PER_BLOCK + 1));
        CHECK(rec_plan(c_pad, 16, 8192, lo, &p) && p.part < TWO32);
        CHECK(!rec_plan(c_pad, 16, 8192, hi, &p));
        check_plan(c_pad, 16, 8192, lo);
        check_plan(c_pad, 16, 8192, hi);
    }
    // the geometries of tests/test_gpu_record_geometry.py (campaigns, ring) -> blocks, S, bins
    const u32 geo[][5] = {{129, 16, 1, 1, 1}, {2049, 16, 2, 1, 2}, {16384, 16, 8, 1, 8}, {16385, 16, 9, 2, 5},
                          {200001, 16, 98, 16, 7}, {1000, 1024, 32, 4, 8}, {300, 32768, 300, 64, 5},
                          {2048, 32768, 2048, 256, 8}, {200000, 128, 782, 128, 7}, {600000, 16, 293, 64, 5},
                          {600000, 128, 2344, 512, 5}};
    for (const auto& g : geo) {
        CHECK(rec_plan(g[0], g[1], 313, 1, &p));
        CHECKF(p.n_blocks == g[2] && (1u << p.sub_log2) == g[3] && p.bins == g[4], "%u x %u: %u blocks, S %u, %u bins",
               g[0], g[1], p.n_blocks, 1u << p.sub_log2, p.bins);
        CHECK(p.cap == (p.bins == 1 ? 64u : 32u));   // one tile per workgroup: 48 lines over the bins, in whole lines
    }
    std::printf("%llu plans checked, %llu accepted, %d failures\n", checked, accepted, fails);
    if (fails) return 1;
    std::printf("OK\n");
    return 0;
}
