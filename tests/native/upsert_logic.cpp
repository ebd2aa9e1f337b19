// Host-side checks of the live map's rules (csrc/ysb_admap.h, the part ysb_ad_map_upsert
// runs): the host model of the three device passes -- with the very eviction chains, searches
// and first-fit routine the kernels of csrc/ysb_upsert.hip call -- on tiny tables whose keys
// collide, at both layouts and at a load's own sizes; the rule that decides between in place
// and rebuild at each of its three limits; the rebuild's merge; the call's records
// (duplicates, shards, rejections).  Every key is looked up with the host restatements of the
// scan's probes (cuckoo_lookup_slots, cuckoo_lookup_buckets, table_lookup).
// Built and run by tests/test_upsert_logic.py with g++ (no GPU, no HIP header).
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>
#include "ysb_admap.h"

using namespace ysb;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

typedef std::map<std::string, u32> Truth;   // the plain map the tables stand for

static std::vector<u32> record(const std::string& id, u32 camp) {
    std::vector<u32> r(SLOT_WORDS, 0);
    r[0] = (u32)id.size();
    r[1] = camp;
    std::memcpy(&r[2], id.data(), id.size());
    return r;
}
static std::string random_id(std::mt19937_64& g, size_t len = 36) {
    std::string s(len, 0);
    for (auto& ch : s) ch = (char)('!' + g() % 90);
    return s;
}
static void slots_of(const JoinTables& jt, const std::string& id, u32* a, u32* b) {
    u32 k[CKEY_WORDS];
    std::memcpy(k, id.data(), 36);
    cuckoo_slots36(k, jt.cseed, (u32)(jt.cslots - 1), a, b);
}
static bool entry_taken(const JoinTables& jt, u32 pos, u32 e) {
    return jt.ctable[jt.buckets ? (u64)pos * CB_WORDS + e * CB_STRIDE + CKEY_WORDS : (u64)pos * CSLOT_WORDS + CSLOT_CAMP] != EMPTY_SLOT;
}
static bool place_full(const JoinTables& jt, u32 pos) {
    for (u32 e = 0; e < (jt.buckets ? (u32)CB_ENTRIES : 1u); ++e)
        if (!entry_taken(jt, pos, e)) return false;
    return true;
}
static u32 cuckoo_lookup(const JoinTables& jt, const u32* k) {
    return jt.buckets ? cuckoo_lookup_buckets(jt.ctable.data(), jt.cslots, jt.cseed, k)
                      : cuckoo_lookup_slots(jt.ctable.data(), jt.cslots, jt.cseed, k);
}

// an empty map with tables of the sizes given (what a load of nothing builds, at other sizes)
static JoinTables empty_tables(u64 slots, u64 cslots, bool buckets) {
    JoinTables jt;
    jt.slots = slots;
    jt.cslots = cslots;
    jt.buckets = buckets;
    jt.cseed = cuckoo_seed(mix64(0x5EEDC0FFEEULL + cslots));
    jt.table.assign(slots * SLOT_WORDS, 0);
    for (u64 s = 0; s < slots; ++s) jt.table[s * SLOT_WORDS + 1] = EMPTY_SLOT;
    jt.ctable.assign(cslots * (buckets ? (u32)CB_WORDS : (u32)CSLOT_WORDS), 0);
    for (u64 s = 0; s < cslots; ++s)
        for (u32 e = 0; e < (buckets ? (u32)CB_ENTRIES : 1u); ++e)
            jt.ctable[buckets ? s * CB_WORDS + e * CB_STRIDE + CKEY_WORDS : s * CSLOT_WORDS + CSLOT_CAMP] = EMPTY_SLOT;
    return jt;
}

// Every key of the truth is found with its latest campaign -- a 36-byte key by the cuckoo
// probe, or with `partial` by the general probe after a cuckoo miss (the scan's deferral),
// any other key by the general probe -- and every key sits in the general table; a key in its
// second bucket has a full first one; a 36-byte key the cuckoo table lacks has both its slots
// or buckets full (it was left out because its chain ran out, or by the sparse hook) and the
// table is then partial.  Returns the 36-byte keys the cuckoo table lacks.
static u64 check_map(const JoinTables& jt, const Truth& truth, bool sparse = false) {
    u64 out = 0, occupied = 0, in_cuckoo = 0;
    for (const auto& kv : truth) {
        const std::string& id = kv.first;
        CHECK(table_lookup(jt.table.data(), jt.slots, id.data(), (u32)id.size()) == kv.second);
        if (id.size() != 36) continue;
        u32 k[CKEY_WORDS], where = 0, a, b;
        std::memcpy(k, id.data(), 36);
        const u32 c = cuckoo_lookup(jt, k);
        const u64 w = jt.buckets ? cuckoo_find_buckets(jt.ctable.data(), (u32)(jt.cslots - 1), jt.cseed, k, &where)
                                 : cuckoo_find_slots(jt.ctable.data(), (u32)(jt.cslots - 1), jt.cseed, k, &where);
        CHECK((w == CK_NONE) == (c == EMPTY_SLOT));   // the shared search agrees with the probe's restatement
        slots_of(jt, id, &a, &b);
        if (c == EMPTY_SLOT) {
            ++out;
            CHECK(jt.partial);
            if (!sparse) CHECK(place_full(jt, a) && place_full(jt, b));
            continue;
        }
        ++in_cuckoo;
        CHECK(c == kv.second && jt.ctable[w] == c);
        if (where == 2 && jt.buckets) CHECK(place_full(jt, a));
    }
    for (u64 s = 0; s < jt.slots; ++s) occupied += jt.table[s * SLOT_WORDS + 1] != EMPTY_SLOT;
    CHECK(occupied == truth.size() && jt.keys == truth.size());   // no key twice, none lost
    CHECK(jt.keys36 == in_cuckoo);
    u64 entries = 0;
    for (u64 s = 0; s < jt.cslots; ++s)
        for (u32 e = 0; e < (jt.buckets ? (u32)CB_ENTRIES : 1u); ++e) entries += entry_taken(jt, (u32)s, e);
    CHECK(entries == in_cuckoo);
    return out;
}

static UpsertCounts upsert(JoinTables* jt, Truth* truth, const std::vector<std::pair<std::string, u32>>& entries,
                           bool sparse = false) {
    std::vector<u32> rec;
    for (const auto& e : entries) {
        const std::vector<u32> r = record(e.first, e.second);
        rec.insert(rec.end(), r.begin(), r.end());
        (*truth)[e.first] = e.second;
    }
    UpsertCounts uc;
    upsert_in_place(jt, rec.data(), entries.size(), sparse, &uc);
    return uc;
}

// ids whose two slots / buckets both lie below `below` (so they collide in a tiny corner)
static std::vector<std::string> colliding_ids(const JoinTables& jt, u32 below, size_t n, u64 seed) {
    std::mt19937_64 g(seed);
    std::vector<std::string> ids;
    while (ids.size() < n) {
        const std::string id = random_id(g);
        u32 a, b;
        slots_of(jt, id, &a, &b);
        if (a < below && b < below) ids.push_back(id);
    }
    return ids;
}

int main() {
    std::string err;
    // 1. tiny tables, keys that collide: 8 slots of which the keys share 3, then 4 buckets of
    // which they share 2 (6 entries), one key per step and then several per call, updates in
    // between; the map is checked after every step
    for (int buckets = 0; buckets < 2; ++buckets) {
        JoinTables jt = empty_tables(64, buckets ? 4 : 8, buckets != 0);
        const u32 corner = buckets ? 2 : 3, room = buckets ? 6 : 3;
        const std::vector<std::string> ids = colliding_ids(jt, corner, 12, 77 + buckets);
        Truth truth;
        u64 left_out = 0;
        for (size_t i = 0; i < 8; ++i) {
            const UpsertCounts uc = upsert(&jt, &truth, {{ids[i], (u32)i}});
            CHECK(uc.inserted == 1 && uc.updated == 0 && uc.first + uc.second + uc.moved + uc.left_out == 1);
            left_out += uc.left_out;
            CHECK(check_map(jt, truth) == left_out);
            CHECK(jt.partial == (left_out > 0));
            if (i + 1 > room) CHECK(left_out >= i + 1 - room);   // more keys than the corner holds
        }
        CHECK(left_out == 8 - room);   // (these keys fill the corner: nothing is left out early)
        std::printf("%s: 8 colliding keys into room for %u: %llu left out\n", buckets ? "buckets" : "slots", room,
                    (unsigned long long)left_out);
        // every key re-pointed, those in the cuckoo table and those left out alike
        std::vector<std::pair<std::string, u32>> again;
        for (size_t i = 0; i < 8; ++i) again.push_back({ids[i], (u32)(100 + i)});
        UpsertCounts uc = upsert(&jt, &truth, again);
        CHECK(uc.updated == 8 && uc.inserted == 0);
        CHECK(check_map(jt, truth) == left_out);
        // a call of several new colliding keys and a known one
        uc = upsert(&jt, &truth, {{ids[8], 1}, {ids[9], 2}, {ids[0], 3}, {ids[10], 4}, {ids[11], 5}});
        CHECK(uc.updated == 1 && uc.inserted == 4 && uc.left_out == 4);   // the corner was full
        CHECK(check_map(jt, truth) == left_out + 4);
    }
    // ... and with room elsewhere: colliding first slots only, so the chain moves keys on
    for (int buckets = 0; buckets < 2; ++buckets) {
        JoinTables jt = empty_tables(256, 64, buckets != 0);
        std::mt19937_64 g(5 + buckets);
        Truth truth;
        u64 moved = 0, second = 0, left_out = 0;
        // keys whose first slot / bucket is one of two: their second ones spread over the table
        for (int step = 0; step < (buckets ? 40 : 12); ++step) {
            std::string id;
            u32 a, b;
            do {
                id = random_id(g);
                slots_of(jt, id, &a, &b);
            } while (a > 1);
            const UpsertCounts uc = upsert(&jt, &truth, {{id, (u32)step}});
            moved += uc.moved;
            second += uc.second;
            left_out += uc.left_out;
            CHECK(check_map(jt, truth) == left_out);
        }
        CHECK(left_out == 0 && !jt.partial && second > 0);
        std::printf("%s: shared first place: %llu second, %llu moved\n", buckets ? "buckets" : "slots",
                    (unsigned long long)second, (unsigned long long)moved);
    }
    // 2. in place or rebuild: the rule flips exactly at each of its three limits
    {
        CHECK(upsert_fits(512, 0, 1024, 64, false) && !upsert_fits(513, 0, 1024, 64, false));
        CHECK(upsert_fits(0, 0, 64, 64, false) && upsert_fits(32, 16, 64, 64, false));
        CHECK(upsert_fits(16, 16, 64, 64, false) && !upsert_fits(17, 17, 64, 64, false));
        CHECK(upsert_fits(1024, 1024, 4096, 4096, false) && !upsert_fits(1025, 1025, 4096, 4096, false));
        CHECK(upsert_fits(524288, 524288, 1ull << 20, 1ull << 20, true) && !upsert_fits(524289, 524289, 1ull << 21, 1ull << 20, true));
        CHECK(!upsert_fits(524289, 524288, 1ull << 20, 1ull << 20, true));
        // they are build_join_tables' own sizes: a load of exactly the limit has these tables,
        // one key more has larger ones
        std::mt19937_64 g(9);
        std::vector<std::string> ids;
        for (int i = 0; i < 1025; ++i) ids.push_back(random_id(g));
        std::vector<const char*> p;
        for (const auto& s : ids) p.push_back(s.data());
        const std::vector<u32> camp(ids.size(), 0);
        JoinTables at, over;
        CHECK(build_join_tables(p.data(), nullptr, camp.data(), 1024, 1, false, &at, &err) == YSB_OK);
        CHECK(build_join_tables(p.data(), nullptr, camp.data(), 1025, 1, false, &over, &err) == YSB_OK);
        CHECK(at.keys == 1024 && at.keys36 == 1024 && at.cslots == 4096 && over.cslots == 8192);
        CHECK(upsert_fits(at.keys, at.keys36, at.slots, at.cslots, at.buckets));
        CHECK(!upsert_fits(over.keys, over.keys36, at.slots, at.cslots, at.buckets));
    }
    // 3. a load's own sizes, slot layout: 600 keys loaded (and some of other lengths), 400
    // upserted in one call with updates of known keys among them; then the rebuild of a call
    // that no longer fits equals, as a map and in its sizes, a load of all the entries
    {
        std::mt19937_64 g(21);
        std::vector<std::pair<std::string, u32>> all;
        for (int i = 0; i < 1100; ++i) all.push_back({random_id(g), (u32)(i % 100)});
        all.push_back({"", 7});
        all.push_back({"short", 8});
        all.push_back({std::string(56, 'z'), 9});
        Truth truth;
        std::vector<const char*> p;
        std::vector<u32> len, camp;
        for (size_t i = 0; i < 600; ++i) {
            p.push_back(all[i].first.data());
            len.push_back(36);
            camp.push_back(all[i].second);
            truth[all[i].first] = all[i].second;
        }
        JoinTables jt;
        CHECK(build_join_tables(p.data(), len.data(), camp.data(), 600, 100, false, &jt, &err) == YSB_OK);
        CHECK(jt.slots == 2048 && jt.cslots == 4096 && jt.keys == 600 && jt.keys36 == 600);
        std::vector<std::pair<std::string, u32>> call(all.begin() + 600, all.begin() + 1000);
        for (size_t i = 0; i < 50; ++i) call.push_back({all[i].first, 99 - all[i].second});   // known keys re-pointed
        call.push_back(all[1100]);
        call.push_back(all[1101]);
        call.push_back(all[1102]);
        CHECK(upsert_fits(jt.keys + 403, jt.keys36 + 400, jt.slots, jt.cslots, jt.buckets));
        const UpsertCounts uc = upsert(&jt, &truth, call);
        CHECK(uc.updated == 50 && uc.inserted == 403 && uc.inserted36 == 400);
        CHECK(uc.first + uc.second + uc.moved == 400 && uc.left_out == 0);
        CHECK(check_map(jt, truth) == 0 && !jt.partial);
        std::printf("slots, 600 + 400: %llu first, %llu second, %llu moved\n", (unsigned long long)uc.first,
                    (unsigned long long)uc.second, (unsigned long long)uc.moved);
        // the next 100 do not fit (1100 keys > 4096 / 4): rebuild
        CHECK(!upsert_fits(jt.keys + 100, jt.keys36 + 100, jt.slots, jt.cslots, jt.buckets));
        std::vector<u32> rec, merged;
        for (size_t i = 1000; i < 1100; ++i) {
            const std::vector<u32> r = record(all[i].first, all[i].second);
            rec.insert(rec.end(), r.begin(), r.end());
            truth[all[i].first] = all[i].second;
        }
        const std::vector<u32> r0 = record(all[3].first, 55);   // and a known key, re-pointed by the call
        rec.insert(rec.end(), r0.begin(), r0.end());
        truth[all[3].first] = 55;
        upsert_merge(jt.table.data(), jt.slots, rec.data(), 101, &merged);
        CHECK(merged.size() == (1003 + 101) * SLOT_WORDS);
        JoinTables rebuilt, fresh;
        CHECK(build_join_tables_rec(merged, 100, false, &rebuilt, &err) == YSB_OK);
        p.clear(); len.clear(); camp.clear();
        for (const auto& kv : truth) {
            p.push_back(kv.first.data());
            len.push_back((u32)kv.first.size());
            camp.push_back(kv.second);
        }
        CHECK(build_join_tables(p.data(), len.data(), camp.data(), p.size(), 100, false, &fresh, &err) == YSB_OK);
        CHECK(rebuilt.slots == fresh.slots && rebuilt.cslots == fresh.cslots && rebuilt.buckets == fresh.buckets);
        CHECK(rebuilt.cslots == 8192 && rebuilt.keys == 1103 && rebuilt.keys36 == 1100 && rebuilt.keys == fresh.keys);
        CHECK(check_map(rebuilt, truth) == 0 && check_map(fresh, truth) == 0);
        // sparse hook: every other new 36-byte key of a call stays out of the cuckoo table
        JoinTables sp;
        Truth st;
        CHECK(build_join_tables(p.data(), len.data(), camp.data(), 0, 100, true, &sp, &err) == YSB_OK);
        const UpsertCounts su = upsert(&sp, &st, {all[0], all[1], all[1100], all[2], all[3], all[4]}, true);
        CHECK(su.inserted == 6 && su.inserted36 == 5 && su.left_out == 3 && su.first + su.second == 2);
        CHECK(check_map(sp, st, true) == 3 && sp.partial);
    }
    // 4. bucket layout at a load's own sizes: 262,145 keys loaded, 100,000 upserted in place
    {
        std::mt19937_64 g(33);
        const size_t n0 = 262145, n1 = 100000;
        std::vector<std::string> ids;
        for (size_t i = 0; i < n0 + n1; ++i) ids.push_back(random_id(g));
        std::vector<const char*> p;
        std::vector<u32> camp;
        Truth truth;
        for (size_t i = 0; i < n0; ++i) {
            p.push_back(ids[i].data());
            camp.push_back((u32)(i % 1000));
            truth[ids[i]] = camp[i];
        }
        JoinTables jt;
        CHECK(build_join_tables(p.data(), nullptr, camp.data(), n0, 1000, false, &jt, &err) == YSB_OK);
        CHECK(jt.buckets && jt.cslots == (1ull << 20) && jt.slots == (1ull << 20));
        CHECK(upsert_fits(n0 + n1, n0 + n1, jt.slots, jt.cslots, true) && upsert_fits(524288, 524288, jt.slots, jt.cslots, true));
        std::vector<std::pair<std::string, u32>> call;
        for (size_t i = n0; i < n0 + n1; ++i) call.push_back({ids[i], (u32)(i % 1000)});
        const UpsertCounts uc = upsert(&jt, &truth, call);
        CHECK(uc.inserted == n1 && uc.first + uc.second + uc.moved == n1 && uc.left_out == 0);
        CHECK(check_map(jt, truth) == 0);
        std::printf("buckets, 262145 + 100000: %llu first, %llu second, %llu moved\n", (unsigned long long)uc.first,
                    (unsigned long long)uc.second, (unsigned long long)uc.moved);
    }
    // 5. the call's records: a later entry of an id wins, shards, and the three rejections
    {
        const std::string a(36, 'a'), b(36, 'b'), c5("hello"), toolong(57, 'x');
        const char* ids[] = {a.data(), b.data(), a.data(), c5.data(), nullptr, a.data()};
        const u32 lens[] = {36, 36, 36, 5, 0, 36}, camp[] = {1, 2, 3, 4, 5, 6};
        std::vector<u32> rec;
        u64 foreign = 9, dups = 9;
        CHECK(upsert_records(ids, lens, camp, 6, 7, 0, 1, &rec, &foreign, &dups, &err) == YSB_OK);
        CHECK(rec.size() == 4 * SLOT_WORDS && foreign == 0 && dups == 2);
        CHECK(rec[0] == 36 && rec[1] == 6 && std::memcmp(&rec[2], a.data(), 36) == 0);   // the last a
        CHECK(rec[SLOT_WORDS] == 36 && rec[SLOT_WORDS + 1] == 2);
        CHECK(rec[2 * SLOT_WORDS] == 5 && rec[2 * SLOT_WORDS + 1] == 4 && rec[2 * SLOT_WORDS + 4] == 0);
        CHECK(rec[3 * SLOT_WORDS] == 0 && rec[3 * SLOT_WORDS + 1] == 5);
        // a later entry wins in the tables too
        JoinTables jt = empty_tables(64, 64, false);
        UpsertCounts uc;
        upsert_in_place(&jt, rec.data(), 4, false, &uc);
        u32 k[CKEY_WORDS];
        std::memcpy(k, a.data(), 36);
        CHECK(cuckoo_lookup(jt, k) == 6 && table_lookup(jt.table.data(), 64, a.data(), 36) == 6 && uc.inserted == 4);
        // shards: the ids of other shards are skipped and counted
        u64 mine = 0;
        for (int i = 0; i < 6; ++i) mine += ad_shard(lens[i] ? ids[i] : "", lens[i], 4) == 1;
        CHECK(upsert_records(ids, lens, camp, 6, 7, 1, 4, &rec, &foreign, &dups, &err) == YSB_OK);
        CHECK(foreign == 6 - mine && rec.size() / SLOT_WORDS + dups == mine);
        // the rejections leave nothing behind
        rec.assign(3, 1u);
        CHECK(upsert_records(ids, lens, camp, 6, 6, 0, 1, &rec, &foreign, &dups, &err) == YSB_ERR_FORMAT);
        CHECK(err == "campaign index 6 >= n_campaigns 6" && rec.size() == 3);
        const char* ids2[] = {a.data(), toolong.data()};
        const u32 lens2[] = {36, 57}, lens3[] = {36, 0};
        CHECK(upsert_records(ids2, lens2, camp, 2, 7, 0, 1, &rec, &foreign, &dups, &err) == YSB_ERR_FORMAT);
        CHECK(err == "ad id 1 longer than 56 bytes");
        const char* ids3[] = {nullptr, nullptr};
        CHECK(upsert_records(ids3, lens3, camp, 2, 7, 0, 1, &rec, &foreign, &dups, &err) == YSB_ERR_ARG);
        CHECK(err == "ad id 0 is NULL" && rec.size() == 3);
    }
    std::printf("%s\n", fails ? "FAILED" : "OK");
    return fails ? 1 : 0;
}
