// Host-side checks of the parked views' rules (csrc/ysb_parked.h): the record pack and unpack,
// the distinct-key table with the very insert routine the kernel of csrc/ysb_parked.hip calls
// (here with a plain compare-and-swap), the resolve rule, the ring-base rule, and the host model
// of park -> distinct -> resolve against a plain map.
// Built and run by tests/test_parked_logic.py with g++ (no GPU, no HIP header).
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>
#include "ysb_parked.h"

using namespace ysb;

static int fails = 0;
#define CHECK(...) do { if (!(__VA_ARGS__)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #__VA_ARGS__); ++fails; } } while (0)

struct Key {
    u32 kw[KEY_WORDS];
    u32 len;
};
static Key key_of(const std::string& id) {
    Key k{};
    k.len = (u32)id.size();
    std::memcpy(k.kw, id.data(), id.size());
    return k;
}
static std::string id_of(const u32* rec) { return std::string(reinterpret_cast<const char*>(rec), rec[PARK_LEN]); }

static void test_record() {
    CHECK(PARK_WORDS * 4 == 72 && PARK_KEY_STRIDE == 56 && PARK_TIME % 2 == 0);
    const i64 times[] = {0, 1, -1, 1700000000123LL, INT64_MAX, INT64_MIN};
    for (size_t len : {(size_t)0, (size_t)1, (size_t)36, (size_t)56}) {
        std::string id(len, 'k');
        for (size_t i = 0; i < len; ++i) id[i] = (char)(0x80 + i);   // high bytes: no sign trouble
        const Key k = key_of(id);
        for (i64 t : times)
            for (bool ok : {false, true}) {
                u32 rec[PARK_WORDS];
                std::memset(rec, 0xAB, sizeof rec);
                park_pack(rec, k.kw, k.len, ok, t);
                i64 back = 7;
                CHECK(park_time(rec, &back) == ok && back == t);
                CHECK(rec[PARK_LEN] == len && id_of(rec) == id);
                CHECK(std::memcmp(rec, k.kw, sizeof k.kw) == 0);   // zero padded: the tables' key form
                u32 again[PARK_WORDS];
                park_pack(again, k.kw, k.len, !ok, t ^ 1);
                CHECK(park_same_key(rec, again));                  // the key alone decides
            }
    }
    // equal words, another length (a key of NULs): not the same key
    u32 a[PARK_WORDS], b[PARK_WORDS];
    const Key k0 = key_of(std::string()), k1 = key_of(std::string(1, '\0'));
    park_pack(a, k0.kw, k0.len, true, 0);
    park_pack(b, k1.kw, k1.len, true, 0);
    CHECK(!park_same_key(a, b));
}

// the model's distinct() on a log of the ids given, as the set of ids of its representatives
static std::multiset<std::string> distinct_ids(const std::vector<std::string>& ids, u64 slots) {
    ParkModel m;
    m.cap = (u32)ids.size();
    for (const auto& id : ids) {
        const Key k = key_of(id);
        m.miss(true, k.kw, k.len, true, 5);
    }
    std::multiset<std::string> out;
    for (u32 i : m.distinct(slots)) out.insert(id_of(&m.log[(u64)i * PARK_WORDS]));
    return out;
}

static void test_distinct() {
    CHECK(park_distinct_slots(0) == 2 && park_distinct_slots(1) == 2 && park_distinct_slots(2) == 4 &&
          park_distinct_slots(64) == 128 && park_distinct_slots(65) == 256);
    // a 2-slot table: two keys that start at the same slot, and two that do not, each twice
    std::vector<std::string> same, other;
    for (int i = 0; same.size() < 2 || other.size() < 2; ++i) {
        const std::string id = "ad-" + std::to_string(i);
        const Key k = key_of(id);
        const u32 s = key_hash(k.kw, k.len) & 1u;
        if (s == 0 && same.size() < 2) same.push_back(id);
        if (other.size() < 2 && (other.empty() ? s == 0 : s == 1)) other.push_back(id);
    }
    for (const auto& pair : {same, other}) {
        const std::multiset<std::string> want{pair[0], pair[1]};
        CHECK(distinct_ids({pair[0], pair[1], pair[0], pair[1], pair[1]}, 2) == want);   // the table is full: at capacity
        CHECK(distinct_ids({pair[1], pair[1], pair[0]}, 2) == want);
    }
    CHECK(distinct_ids({same[0], same[0], same[0]}, 2) == std::multiset<std::string>{same[0]});
    // a third key finds the 2-slot table full: PARK_FULL, kept (asked twice at worst, never lost)
    {
        ParkModel m;
        m.cap = 3;
        for (const auto& id : {same[0], same[1], other[1]}) {
            const Key k = key_of(id);
            m.miss(true, k.kw, k.len, true, 0);
        }
        std::vector<u32> tab(2, EMPTY_SLOT);
        auto cas = [&](u32 s, u32 v) { const u32 p = tab[s]; if (p == EMPTY_SLOT) tab[s] = v; return p; };
        CHECK(park_distinct_insert(m.log.data(), 0, 1, cas) == PARK_REP);
        CHECK(park_distinct_insert(m.log.data(), 1, 1, cas) == PARK_REP);
        CHECK(park_distinct_insert(m.log.data(), 2, 1, cas) == PARK_FULL);
        CHECK(park_distinct_insert(m.log.data(), 1, 1, cas) == PARK_DUP);
    }
    // at capacity with the slots a context allocates: 64 records, 16 keys of several lengths
    std::vector<std::string> ids;
    std::multiset<std::string> want;
    for (int i = 0; i < 64; ++i) {
        const int k = i % 16;
        ids.push_back(std::string((size_t)(k * 56 / 15), (char)('a' + k)));   // lengths 0 .. 56
    }
    for (const auto& id : ids) if (!want.count(id)) want.insert(id);
    CHECK(want.size() == 16);
    CHECK(distinct_ids(ids, park_distinct_slots(64)) == want);
}

static void test_resolve_and_ring_base() {
    CHECK(park_resolve_class(true, true) == PARK_R_COUNT);
    CHECK(park_resolve_class(true, false) == PARK_R_TIME_ERR);
    CHECK(park_resolve_class(false, true) == PARK_R_MISS && park_resolve_class(false, false) == PARK_R_MISS);
    CHECK(park_ring_base(100, 16) == 98 && park_ring_base(-3, 1024) == -131 && park_ring_base(7, 4) == 7);

    const DivMagic div = div_magic(10000);
    std::map<std::string, u32> redis{{"known-good", 3}, {"known-bad-time", 4}, {std::string(56, 'x'), 5}};
    auto find = [&](const u32* kw, u32 len) {
        auto it = redis.find(std::string(reinterpret_cast<const char*>(kw), len));
        return it == redis.end() ? (u32)EMPTY_SLOT : it->second;
    };
    // a foreign key (2 shards) and one of this rank's
    std::string mine, foreign;
    for (int i = 0; mine.empty() || foreign.empty(); ++i) {
        const std::string id = "shard-" + std::to_string(i);
        const Key k = key_of(id);
        (key_shard(key_hash(k.kw, k.len), 2) == 1 ? mine : foreign) = id;
    }
    redis[mine] = 6;
    redis[foreign] = 7;

    ParkModel m;
    m.cap = 8;
    m.shard_rank = 1;
    m.shard_n = 2;
    auto park = [&](const std::string& id, bool ok, i64 t) {
        const Key k = key_of(id);
        m.miss(id.size() <= MAX_KEY_BYTES, k.kw, k.len, ok, t);
    };
    // (ids of the other shard would be foreign: give the unsharded ids to an unsharded model below)
    park(mine, true, 1230000);
    park(foreign, true, 1230000);
    CHECK(m.t.parked == 1 && m.t.foreign == 1 && m.t.misses == 0 && m.parked_now() == 1);
    CHECK(id_of(&m.log[0]) == mine);   // the foreign key is never in the log
    std::map<std::pair<u32, i64>, u64> counts;
    auto add = [&](u32 c, i64 b) { counts[{c, b}]++; };
    bool ring_set = false;
    i64 ring_lo = 0;
    m.resolve(find, add, div, 16, &ring_set, &ring_lo);
    CHECK(m.parked_now() == 0 && m.t.joined == 1 && counts.size() == 1 && counts[{6u, (i64)123}] == 1);
    CHECK(ring_set && ring_lo == 123 - 2);

    ParkModel u;
    u.cap = 6;
    auto upark = [&](const std::string& id, bool ok, i64 t) {
        const Key k = key_of(id.size() <= MAX_KEY_BYTES ? id : std::string());
        u.miss(id.size() <= MAX_KEY_BYTES, k.kw, k.len, ok, t);
    };
    upark("known-good", true, 500000);
    upark("known-good", true, 90000);          // the smallest counted bucket: 9
    upark("known-bad-time", false, 0);
    upark("nowhere", true, 10000);             // bucket 1, but never counted: not the base
    upark("nowhere", false, 0);                // not found: a miss, whatever its time
    upark(std::string(56, 'x'), true, -20000); // negative times truncate toward zero
    upark(std::string(57, 'x'), true, 1);      // cannot be a key: a miss, never parked
    upark("late", true, 1);                    // the log is full
    CHECK(u.t.parked == 6 && u.t.misses == 2 && u.t.dropped == 1 && u.parked_now() == 6);
    CHECK(u.distinct(park_distinct_slots(6)).size() == 4);
    counts.clear();
    ring_set = false;
    u.resolve(find, add, div, 16, &ring_set, &ring_lo);
    CHECK(u.t.joined == 4 && u.t.time_errors == 1 && u.t.resolved_misses == 2 && u.parked_now() == 0);
    CHECK(counts.size() == 3 && counts[{3u, (i64)50}] == 1 && counts[{3u, (i64)9}] == 1 && counts[{5u, (i64)-2}] == 1);
    CHECK(ring_set && ring_lo == -2 - 2);      // the smallest bucket counted, minus W / 8
    // a base that is set stays; a resolve that counts nothing sets none
    upark("known-good", true, 0);
    ring_lo = 77;
    u.resolve(find, add, div, 16, &ring_set, &ring_lo);
    CHECK(ring_lo == 77);
    upark("nowhere", true, 0);
    upark("known-bad-time", false, 0);
    ring_set = false;
    u.resolve(find, add, div, 16, &ring_set, &ring_lo);
    CHECK(!ring_set && u.t.resolved_misses == 3 && u.t.time_errors == 2);
    // views == joined + misses + foreign + parked at every step
    CHECK(u.t.parked + u.t.misses == 6 + 2 + 1 + 2);
    CHECK(u.t.parked == u.t.joined + u.t.resolved_misses);
}

int main() {
    test_record();
    test_distinct();
    test_resolve_and_ring_base();
    if (fails) { std::printf("%d FAILED\n", fails); return 1; }
    std::printf("parked logic OK\n");
    return 0;
}
