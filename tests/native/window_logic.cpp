// Host-side checks of the LDS window's and the ring base's rules (csrc/ysb_window.h): the very
// functions the device window of csrc/ysb_ring_add.h, the scan kernel and the auto-base kernels
// call, at the smallest, a middle and the largest window, and a tile-by-tile model of the window
// built from them against a plain count.
// Built and run by tests/test_window_logic.py with g++ (no GPU, no HIP header).
#include <cstdint>
#include <cstdio>
#include <map>
#include <utility>
#include <vector>
#include "ysb_parked.h"   // park_ring_base: the same rule under its older name
#include "ysb_window.h"

using namespace ysb;

static int fails = 0;
#define CHECK(...) do { if (!(__VA_ARGS__)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #__VA_ARGS__); ++fails; } } while (0)

static void test_rules() {
    for (u32 WL : {2u, 16u, 1024u}) {
        const i64 W = (i64)WL;
        // rel -1, 0, WL - 1, WL; window set and unset
        CHECK(!window_holds(true, -1, WL) && window_holds(true, 0, WL) && window_holds(true, W - 1, WL) && !window_holds(true, W, WL));
        for (i64 rel : {(i64)-1, (i64)0, W - 1, W}) CHECK(!window_holds(false, rel, WL));
        // behind the window: no move; ahead of it: a move; no window yet: any view asks
        CHECK(!window_asks_move(true, -1, WL) && window_asks_move(true, W, WL) && window_asks_move(true, W + 5, WL));
        CHECK(!window_asks_move(true, INT64_MIN / 2, WL));
        for (i64 rel : {(i64)-1, (i64)0, W - 1, W}) CHECK(window_asks_move(false, rel, WL));
        // (a view the window holds never gets as far as the question; the rule says no anyway)
        CHECK(!window_asks_move(true, 0, WL) && !window_asks_move(true, W - 1, WL));
        // the re-centred window holds its request at rel WL / 2 - 1, negative buckets included
        for (i64 req : {(i64)0, (i64)1, (i64)-1, (i64)-1000, (i64)170000000, (i64)-170000000}) {
            const i64 base = window_base_for(req, WL);
            CHECK(base == req - W / 2 + 1 && req - base == W / 2 - 1);
            CHECK(window_holds(true, req - base, WL));
            CHECK(window_holds(true, (base + W - 1) - base, WL) && !window_holds(true, (base + W) - base, WL));
            CHECK(!window_holds(true, (base - 1) - base, WL));
        }
    }
    CHECK(window_base_for(0, 2) == 0 && window_base_for(7, 2) == 7);   // the smallest window: WL / 2 - 1 = 0
    CHECK(window_base_for(0, 16) == -7 && window_base_for(-3, 16) == -10 && window_base_for(100, 1024) == -411);
}

static void test_ring_base() {
    CHECK(ring_base_for(100, 16) == 98 && ring_base_for(-3, 1024) == -131 && ring_base_for(7, 4) == 7);
    CHECK(park_ring_base(100, 16) == 98 && park_ring_base(-3, 1024) == -131 && park_ring_base(7, 4) == 7);
    CHECK(ring_base_for(0, 64) == -8 && ring_base_for(INT64_MIN / 2, 8) == INT64_MIN / 2 - 1);
}

// The window as the kernels step it, from the rules alone: tiles of rows (campaign, bucket);
// per tile the previous tile's request is applied (flush, re-centre), then every row is counted
// into the window or "the ring" (here: a plain map), and rows ahead of the window raise the
// request to their largest bucket.
struct Model {
    u32 WL;
    std::map<std::pair<u32, i64>, u64> ring, win;
    i64 base = 0, req[2] = {INT64_MIN, INT64_MIN};
    bool set = false;
    u32 tseq = 0, moves = 0, lds_adds = 0, ring_adds = 0;

    void flush() {
        for (const auto& kv : win) ring[kv.first] += kv.second;
        win.clear();
    }
    void tile(const std::vector<std::pair<u32, i64>>& rows) {
        const int par = (int)(tseq++ & 1);
        if (req[par ^ 1] != INT64_MIN) {
            if (set) flush();
            base = window_base_for(req[par ^ 1], WL);
            set = true;
            ++moves;
        }
        req[par ^ 1] = INT64_MIN;
        for (const auto& r : rows) {
            const i64 rel = r.second - base;
            if (window_holds(set, rel, WL)) {
                ++win[r];
                ++lds_adds;
            } else {
                ++ring[r];
                ++ring_adds;
                if (window_asks_move(set, rel, WL) && r.second > req[par]) req[par] = r.second;
            }
        }
    }
};

static void test_model() {
    // four full tiles and a 7-row one: no window yet; all inside the re-centred window; ahead and
    // behind in one tile; some inside the new window and some behind it; a last view that only
    // the final flush brings out
    std::vector<std::vector<std::pair<u32, i64>>> tiles(5);
    for (u32 i = 0; i < 64; ++i) tiles[0].push_back({i % 10, (i64)(i % 4)});
    for (u32 i = 0; i < 64; ++i) tiles[1].push_back({i % 10, (i64)(2 + i % 8)});
    for (u32 i = 0; i < 64; ++i) tiles[2].push_back({i % 10, i % 16 == 3 ? (i64)5 : (i64)(20 + i % 21)});
    for (u32 i = 0; i < 64; ++i) tiles[3].push_back({i % 10, (i64)(30 + i % 16)});
    for (u32 i = 0; i < 7; ++i) tiles[4].push_back({i, i == 3 ? (i64)70 : (i64)47});
    std::map<std::pair<u32, i64>, u64> want;
    Model m{16};
    for (const auto& t : tiles) {
        for (const auto& r : t) ++want[r];
        m.tile(t);
    }
    // tile 0 asked for bucket 3: base -4 holds tile 1 whole; tile 2 asked for 40: base 33
    CHECK(m.moves == 2 && m.base == window_base_for(40, 16) && m.base == 33);
    // tile 3's buckets 30..32 lie behind base 33, went to the ring and raised no request; 70 did
    CHECK(m.req[0] == 70 && m.req[1] == INT64_MIN);
    CHECK(!m.win.empty());   // 33..45 and 47 wait for the final flush
    m.flush();
    CHECK(m.ring == want);
    CHECK(m.lds_adds + m.ring_adds == 263 && m.lds_adds >= 64);
    // the smallest window under a walk of one bucket a tile: a tile ahead of it asks, the next
    // one moves it and counts in LDS -- every other tile
    Model s{2};
    std::map<std::pair<u32, i64>, u64> swant;
    for (i64 b = 0; b < 16; ++b) {
        std::vector<std::pair<u32, i64>> t;
        for (u32 i = 0; i < 8; ++i) t.push_back({i, b});
        for (const auto& r : t) ++swant[r];
        s.tile(t);
    }
    s.flush();
    CHECK(s.ring == swant && s.moves == 8 && s.lds_adds == 64 && s.ring_adds == 64);
}

int main() {
    test_rules();
    test_ring_base();
    test_model();
    std::printf(fails ? "%d FAILED\n" : "window_logic: OK\n", fails);
    return fails ? 1 : 0;
}
