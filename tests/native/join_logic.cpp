// join_logic.cpp -- the HIP-free rules of the joined-views call (csrc/ysb_join.h) on the CPU:
// the output layout, the scratch bound, the rank / prefix / clip plan and the host model of the
// three launches against a naive ordered filter.  Every buffer is an exact-size heap allocation,
// so under -fsanitize=address a write outside the scratch area or a column's rows faults.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ysb_join.h"

using namespace ysb;

static int fails = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } \
    } while (0)

static void test_layout() {
    for (u32 flags : {0u, (u32)JOIN_KEYS}) {
        for (u64 cap : {0ull, 1ull, 4097ull}) {
            u64 st[JC_COUNT_ + 1];
            CHECK(join_layout(cap, flags, st));
            u64 at = 0;
            for (u32 c = 0; c < (u32)JC_COUNT_; ++c) {
                CHECK(st[c] % JOIN_PAGE == 0 && st[c] == at);
                if (c < join_cols(flags)) {
                    const u64 bytes = (u64)join_col_width(c) * cap;
                    at += (bytes + 4095) / 4096 * 4096;
                    CHECK(at - st[c] >= bytes && at - st[c] < bytes + 4096);
                }
            }
            CHECK(st[JC_COUNT_] == at);
            if (cap == 0) CHECK(at == 0);
            if (!(flags & JOIN_KEYS)) CHECK(st[JC_KEY] == st[JC_COUNT_] && st[JC_KEY_LEN] == st[JC_COUNT_]);
        }
    }
    u64 st[JC_COUNT_ + 1];
    CHECK(join_layout(4097, 0, st) && st[1] == 20480 && st[2] == 40960 && st[3] == 77824 && st[6] == 86016);
    CHECK(join_layout(4097, JOIN_KEYS, st) && st[4] == 86016 && st[5] == 319488 && st[6] == 327680);
    CHECK(!join_layout(1, 2, st) && !join_layout(1ull << 32, 0, st) && join_layout(JOIN_MAX_ROWS, 0, st));
    CHECK(join_col_width(JC_KEY) == 56 && join_cols(0) == 4 && join_cols(JOIN_KEYS) == 6);
}

static void test_plan() {
    CHECK(join_rank(0, 63) == 0 && join_rank(~0ull, 0) == 0 && join_rank(~0ull, 63) == 63 && join_rank(0b1011, 3) == 2);
    JoinRun r = join_run(10, 5, 100);
    CHECK(r.first == 10 && r.count == 5);
    r = join_run(10, 5, 12);   // the capacity cuts the tile
    CHECK(r.first == 10 && r.count == 2);
    r = join_run(10, 5, 10);   // ... lies on its boundary
    CHECK(r.first == 10 && r.count == 0);
    r = join_run(10, 5, 3);    // ... or before it
    CHECK(r.first == 3 && r.count == 0);
    r = join_run(0, 64, 0);
    CHECK(r.count == 0);
    for (u64 at = 0; at < 40; ++at)
        for (u64 bytes = 0; bytes < 70; ++bytes) {
            u64 a, b;
            join_span(at, bytes, &a, &b);
            CHECK(at <= a && a <= b && b <= at + bytes && (b - a) % 16 == 0);
            CHECK(a - at < 16 && at + bytes - b < 16);
            CHECK(a == b || (a % 16 == 0 && b % 16 == 0));
            if (bytes >= 31) CHECK(b > a);   // a run that spans an aligned vector uses it
        }
    // the scratch bound: 16 bytes per line of whole tiles, 80 with keys
    for (u64 n : {0ull, 1ull, 63ull, 64ull, 65ull, 129ull, 10000000ull}) {
        const u64 whole = join_tiles(n) * JOIN_TILE;
        CHECK(join_scratch_bytes(n, 0) <= 16 * whole && join_scratch_bytes(n, JOIN_KEYS) <= 80 * whole);
        CHECK(join_scratch_counts(n, 0) % 16 == 0 && join_scratch_counts(n, JOIN_KEYS) % 16 == 0);
    }
    CHECK(join_lane_row(3, join_lane_pack(17, true)) == 3 * 64 + 17 && join_lane_ok(join_lane_pack(17, true)) == 1 &&
          join_lane_ok(join_lane_pack(63, false)) == 0 && join_lane_row(0, join_lane_pack(63, false)) == 63);
}

// lines[0, n) by a mask rule; the line's fields are functions of its index
enum Rule { NONE, ALL, THIRD, FIRST_TWO_TILES_EMPTY, RANDOM };
static std::vector<JoinLine> make_lines(u64 n, Rule rule, u64 seed) {
    std::vector<JoinLine> v(n);
    for (u64 i = 0; i < n; ++i) {
        JoinLine& x = v[i];
        const u64 h = mix64(seed * 1315423911ull + i);
        x.joined = rule == ALL || (rule == THIRD && i % 3 == 1) || (rule == FIRST_TWO_TILES_EMPTY && i >= 128) ||
                   (rule == RANDOM && (h & 3) == 0);
        x.campaign = (u32)(h >> 8) % 1000u;
        x.time_ok = (h >> 40) % 7 != 0;
        x.time = x.time_ok ? (i64)(h >> 3) - (i64)(1ull << 59) : 0;
        x.key_len = (u32)((h >> 20) % 57);
        for (u32 k = 0; k < x.key_len; ++k) x.key[k] = (u8)(1 + (h >> (k % 50)) % 255);
    }
    return v;
}

static void run_case(u64 n, Rule rule, u32 flags, u64 cap, u64 seed) {
    const std::vector<JoinLine> lines = make_lines(n, rule, seed);
    // the naive ordered filter
    std::vector<u64> want;
    for (u64 i = 0; i < n; ++i)
        if (lines[i].joined) want.push_back(i);
    // the model's three steps
    std::vector<u8> scratch(join_scratch_bytes(n, flags), 0xEE);
    join_model_tiles(lines.data(), n, flags, scratch.data());
    const u64 joined = join_model_prefix(n, flags, scratch.data());
    CHECK(joined == want.size());
    const u32* count = reinterpret_cast<const u32*>(scratch.data() + join_scratch_counts(n, flags));
    for (u64 t = 0; t < join_tiles(n); ++t) {
        u32 c = 0;
        for (u64 i = t * 64; i < n && i < (t + 1) * 64; ++i) c += lines[i].joined;
        CHECK(count[t] == c);
        if (rule == ALL && (t + 1) * 64 <= n) CHECK(c == 64);
        if (rule == NONE) CHECK(c == 0);
    }
    u64 st[JC_COUNT_ + 1];
    CHECK(join_layout(cap, flags, st));
    const u8 CANARY = 0xA5;
    std::vector<u8> out(st[JC_COUNT_], CANARY);
    join_model_pack(n, flags, scratch.data(), out.data(), cap);
    const u64 rows = joined < cap ? joined : cap;
    for (u64 r = 0; r < rows; ++r) {
        const JoinLine& x = lines[want[r]];
        u32 c, row;
        i64 t;
        memcpy(&c, &out[st[JC_CAMPAIGN] + 4 * r], 4);
        memcpy(&row, &out[st[JC_ROW] + 4 * r], 4);
        memcpy(&t, &out[st[JC_TIME] + 8 * r], 8);
        CHECK(c == x.campaign && row == want[r] && t == x.time && out[st[JC_TIME_OK] + r] == (x.time_ok ? 1 : 0));
        if (flags & JOIN_KEYS)
            CHECK(out[st[JC_KEY_LEN] + r] == x.key_len && !memcmp(&out[st[JC_KEY] + 56 * r], x.key, 56));
    }
    // nothing else of out is touched
    for (u32 c = 0; c < join_cols(flags); ++c)
        for (u64 p = st[c] + (u64)join_col_width(c) * rows; p < st[c + 1]; ++p)
            if (out[p] != CANARY) { CHECK(out[p] == CANARY); break; }
}

int main() {
    test_layout();
    test_plan();
    u64 seed = 1;
    for (u64 n : {0ull, 1ull, 63ull, 64ull, 65ull, 129ull, 1000ull})
        for (Rule rule : {NONE, ALL, THIRD, FIRST_TWO_TILES_EMPTY, RANDOM})
            for (u32 flags : {0u, (u32)JOIN_KEYS}) {
                u64 joined = 0;
                for (const JoinLine& x : make_lines(n, rule, seed)) joined += x.joined;
                // the capacity: none, one row, inside a tile's run, on a tile's boundary (the
                // rows of the first tile / the first two), one short, exact, ample
                u64 first = 0, two = 0;
                {
                    const std::vector<JoinLine> v = make_lines(n, rule, seed);
                    for (u64 i = 0; i < n && i < 128; ++i) { two += v[i].joined; if (i < 64) first += v[i].joined; }
                }
                for (u64 cap : std::vector<u64>{0, 1, first / 2, first, two, two + 1, joined ? joined - 1 : 0, joined, n, n + 70})
                    run_case(n, rule, flags, cap, seed);
                ++seed;
            }
    if (fails) return 1;
    std::printf("join_logic OK\n");
    return 0;
}
