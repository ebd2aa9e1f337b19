// Host-side checks of the ad -> campaign join tables (csrc/ysb_admap.h): the slot-layout
// cuckoo builder and its probe, the general table's later-wins rule and its probe, the
// argument checks, the sparse thinning, the switch to the bucket layout, and fingerprints of
// whole tables that pin the seed sequence and the placement order.
// Built and run by tests/test_capi.py with g++ (no GPU, no HIP header).
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "ysb_admap.h"

using namespace ysb;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

// n random 36-byte keys as words (fixed seed), and pointers to them as ad ids
static std::vector<u32> random_keys(u64 n, u64 seed) {
    std::vector<u32> w(n * CKEY_WORDS);
    std::mt19937_64 r(seed);
    for (auto& x : w) x = (u32)r();
    return w;
}
static std::vector<const char*> id_ptrs(const std::vector<u32>& w) {
    std::vector<const char*> p(w.size() / CKEY_WORDS);
    for (size_t i = 0; i < p.size(); ++i) p[i] = reinterpret_cast<const char*>(&w[i * CKEY_WORDS]);
    return p;
}
static std::vector<u32> campaigns(u64 n, u32 mod) {
    std::vector<u32> c(n);
    for (u64 i = 0; i < n; ++i) c[i] = (u32)(i % mod);
    return c;
}
// the seed build_join_tables tries first for a table of cslots
static CuckooSeed first_seed(u64 cslots) { return cuckoo_seed(mix64(0x5EEDC0FFEEULL + cslots)); }

static u64 occupied_slots(const JoinTables& jt) {
    u64 n = 0;
    for (u64 s = 0; s < jt.cslots; ++s) n += jt.ctable[s * CSLOT_WORDS + CSLOT_CAMP] != EMPTY_SLOT;
    return n;
}
static u32 cuckoo_lookup(const JoinTables& jt, const u32* k) {
    return jt.buckets ? cuckoo_lookup_buckets(jt.ctable.data(), jt.cslots, jt.cseed, k)
                      : cuckoo_lookup_slots(jt.ctable.data(), jt.cslots, jt.cseed, k);
}
static u64 fingerprint(const JoinTables& jt) {
    u64 h = 0;
    for (u32 w : jt.table) h = mix64(h + w);
    for (u32 w : jt.ctable) h = mix64(h + w);
    return h;
}
static int build(const std::vector<const char*>& ids, const u32* lens, const std::vector<u32>& camp, u32 n_campaigns,
                 bool sparse, JoinTables* jt, std::string* err) {
    return build_join_tables(ids.data(), lens, camp.data(), ids.size(), n_campaigns, sparse, jt, err);
}

int main() {
    std::string err;
    // 1. the slot builder at build_join_tables' own sizing: placed on the first seed, every
    // key found with its campaign, absent keys not found
    for (u64 n : {1ull, 16ull, 17ull, 1000ull, 20000ull}) {
        u64 cslots = 64;
        while (cslots < 4 * n) cslots <<= 1;
        const std::vector<u32> keys = random_keys(n, 100 + n), camp = campaigns(n, 1000);
        std::vector<u32> ct(cslots * CSLOT_WORDS, 0xABABABABu);   // (the builder clears it)
        const CuckooSeed cs = first_seed(cslots);
        CHECK(cuckoo_build_slots(keys.data(), camp.data(), n, cs, cslots, false, ct.data()) == 0);
        for (u64 i = 0; i < n; ++i) CHECK(cuckoo_lookup_slots(ct.data(), cslots, cs, &keys[i * CKEY_WORDS]) == camp[i]);
        const std::vector<u32> absent = random_keys(2000, 7 + n);
        for (u64 i = 0; i < 2000; ++i)
            CHECK(cuckoo_lookup_slots(ct.data(), cslots, cs, &absent[i * CKEY_WORDS]) == EMPTY_SLOT);
    }
    // 2. overfull (load 0.9) with keep_going: some keys are left out, each of them exactly
    // once, none is found with a wrong campaign; without keep_going it stops at the first
    for (u64 cslots : {1024ull, 16384ull}) {
        const u64 n = cslots * 9 / 10;
        const std::vector<u32> keys = random_keys(n, 200 + cslots), camp = campaigns(n, 1000);
        std::vector<u32> ct(cslots * CSLOT_WORDS);
        const CuckooSeed cs = first_seed(cslots);
        const u64 left_out = cuckoo_build_slots(keys.data(), camp.data(), n, cs, cslots, true, ct.data());
        u64 found = 0;
        for (u64 i = 0; i < n; ++i) {
            const u32 c = cuckoo_lookup_slots(ct.data(), cslots, cs, &keys[i * CKEY_WORDS]);
            CHECK(c == camp[i] || c == EMPTY_SLOT);
            found += c != EMPTY_SLOT;
        }
        std::printf("overfull %llu slots: %llu found + %llu left out of %llu\n", (unsigned long long)cslots,
                    (unsigned long long)found, (unsigned long long)left_out, (unsigned long long)n);
        CHECK(left_out > 0);
        CHECK(found + left_out == n);
        CHECK(cuckoo_build_slots(keys.data(), camp.data(), n, cs, cslots, false, ct.data()) == 1);
    }
    // 3. a mixed map: 36-byte keys, other lengths, a duplicate whose later campaign differs,
    // two keys that differ only past byte 36, a key that is another's zero-padded prefix
    {
        const std::vector<u32> k36 = random_keys(40, 3);
        std::vector<std::string> ids;
        for (const char* p : id_ptrs(k36)) ids.emplace_back(p, 36);
        const size_t dup = ids.size();
        ids.push_back(ids[5]);                                     // ... again, with another campaign
        ids.push_back("");                                         // 0 bytes
        ids.push_back("a");                                        // 1
        ids.push_back(std::string(35, 'b'));                       // 35
        ids.push_back(std::string(37, 'c'));                       // 37
        ids.push_back(std::string(56, 'd'));                       // 56
        ids.push_back(ids[7] + "-x1");                             // 39: the same first 36 bytes ...
        ids.push_back(ids[7] + "-x2");                             // ... as ids[7] and as each other
        ids.push_back("ab");
        ids.push_back(std::string("ab\0", 3));                     // "ab" zero padded by one byte
        std::vector<const char*> ptr;
        std::vector<u32> len, camp;
        for (size_t i = 0; i < ids.size(); ++i) {
            ptr.push_back(ids[i].empty() ? nullptr : ids[i].data());   // (a NULL id of 0 bytes is allowed)
            len.push_back((u32)ids[i].size());
            camp.push_back((u32)(i % 50));
        }
        JoinTables jt;
        CHECK(build(ptr, len.data(), camp, 50, false, &jt, &err) == YSB_OK);
        CHECK(jt.slots == 128 && jt.cslots == 256 && !jt.buckets && !jt.partial);
        for (size_t i = 0; i < ids.size(); ++i)
            CHECK(table_lookup(jt.table.data(), jt.slots, ids[i].data(), len[i]) == (i == 5 ? camp[dup] : camp[i]));
        CHECK(camp[dup] != camp[5]);
        CHECK(table_lookup(jt.table.data(), jt.slots, "ab\0\0", 4) == EMPTY_SLOT);
        CHECK(table_lookup(jt.table.data(), jt.slots, ids[7].data(), 35) == EMPTY_SLOT);
        CHECK(occupied_slots(jt) == 40);   // exactly the distinct 36-byte keys
        for (size_t i = 0; i < 40; ++i) CHECK(cuckoo_lookup(jt, &k36[i * CKEY_WORDS]) == (i == 5 ? camp[dup] : camp[i]));
        u32 w[CKEY_WORDS];
        std::memcpy(w, std::string(37, 'c').data(), 36);   // a longer key's first 36 bytes are no key
        CHECK(cuckoo_lookup(jt, w) == EMPTY_SLOT);
    }
    // 4. the three rejections
    {
        const std::string long_id(57, 'x'), ok_id(36, 'y');
        const std::vector<u32> camp{0, 7};
        std::vector<u32> len{36, 57};
        JoinTables jt;
        CHECK(build({ok_id.data(), long_id.data()}, len.data(), camp, 8, false, &jt, &err) == YSB_ERR_FORMAT);
        CHECK(err == "ad id 1 longer than 56 bytes");
        len[1] = 56;
        CHECK(build({ok_id.data(), long_id.data()}, len.data(), camp, 7, false, &jt, &err) == YSB_ERR_FORMAT);
        CHECK(err == "campaign index 7 >= n_campaigns 7");
        CHECK(build({nullptr, long_id.data()}, len.data(), camp, 8, false, &jt, &err) == YSB_ERR_ARG);
        CHECK(err == "ad id 0 is NULL");
    }
    // 5. sparse: the keys at odd positions of the extracted key list (the general table's
    // 36-byte keys in slot order) are in the cuckoo table, the others only in the general one
    {
        const u64 n = 1001;
        const std::vector<u32> keys = random_keys(n, 5), camp = campaigns(n, 100);
        JoinTables jt;
        CHECK(build(id_ptrs(keys), nullptr, camp, 100, true, &jt, &err) == YSB_OK);
        CHECK(jt.partial && !jt.buckets);
        u64 pos = 0;
        for (u64 s = 0; s < jt.slots; ++s) {
            const u32* e = &jt.table[s * SLOT_WORDS];
            if (e[1] == EMPTY_SLOT) continue;
            CHECK(e[0] == 36);
            CHECK(cuckoo_lookup(jt, e + 2) == ((pos & 1) ? e[1] : (u32)EMPTY_SLOT));
            ++pos;
        }
        CHECK(pos == n && occupied_slots(jt) == n / 2);
        CHECK(fingerprint(jt) == 0x3786ad49c59f086fULL);   // (recorded like test 7's)
        for (u64 i = 0; i < n; ++i) CHECK(table_lookup(jt.table.data(), jt.slots, &keys[i * CKEY_WORDS], 36) == camp[i]);
    }
    // 6. the layout switch on both sides of its threshold (a slot table of 64 MiB), and
    // 7. fingerprints of whole tables, recorded from the code before it moved here (the loops
    // of ysb_load_ad_map): the same seeds tried in the same order, every key in the same place
    {
        const std::vector<u32> keys = random_keys(262145, 6), camp = campaigns(262145, 1000);
        std::vector<const char*> ids = id_ptrs(keys);
        JoinTables big;
        CHECK(build(ids, nullptr, camp, 1000, false, &big, &err) == YSB_OK);
        CHECK(big.buckets && !big.partial && big.cslots == (1ull << 20) && big.ctable.size() == big.cslots * CB_WORDS);
        for (u64 i = 0; i < ids.size(); ++i) CHECK(cuckoo_lookup_buckets(big.ctable.data(), big.cslots, big.cseed, &keys[i * CKEY_WORDS]) == camp[i]);
        std::printf("fingerprint 262145 keys: 0x%016llx\n", (unsigned long long)fingerprint(big));
        CHECK(fingerprint(big) == 0xb494bae58a9a09a5ULL);
        ids.pop_back();
        JoinTables jt;
        CHECK(build(ids, nullptr, camp, 1000, false, &jt, &err) == YSB_OK);
        CHECK(!jt.buckets && !jt.partial && jt.cslots == (1ull << 20) && jt.ctable.size() == jt.cslots * CSLOT_WORDS);
        CHECK(occupied_slots(jt) == 262144);
        CHECK(fingerprint(jt) == 0x8be85ba501019f4bULL);
    }
    {
        const std::vector<u32> keys = random_keys(20000, 100 + 20000), camp = campaigns(20000, 1000);   // test 1's set
        JoinTables jt;
        CHECK(build(id_ptrs(keys), nullptr, camp, 1000, false, &jt, &err) == YSB_OK);
        std::printf("fingerprint 20000 keys: 0x%016llx\n", (unsigned long long)fingerprint(jt));
        CHECK(fingerprint(jt) == 0xb577819c0c357fddULL);
        // the generator's default map: seed 42, 100 campaigns x 10 ads (ysb_gen_default, ysb_gen_ids)
        std::vector<char> text(36 * 1000);
        std::vector<const char*> ids(1000);
        for (u64 a = 0; a < 1000; ++a) {
            u64 hi, lo;
            uuid_words(stream_key(42, S_AD), a, &hi, &lo);
            uuid_format(hi, lo, &text[36 * a]);
            ids[a] = &text[36 * a];
        }
        std::vector<u32> gcamp(1000);
        for (u32 a = 0; a < 1000; ++a) gcamp[a] = a / 10;
        CHECK(build(ids, nullptr, gcamp, 100, false, &jt, &err) == YSB_OK);
        for (u32 a = 0; a < 1000; ++a) {
            u32 w[CKEY_WORDS];
            std::memcpy(w, ids[a], 36);
            CHECK(cuckoo_lookup(jt, w) == gcamp[a]);
        }
        std::printf("fingerprint generator map: 0x%016llx\n", (unsigned long long)fingerprint(jt));
        CHECK(fingerprint(jt) == 0x9dc4b50d16804e64ULL);
    }
    std::printf("%s\n", fails ? "FAILED" : "OK");
    return fails ? 1 : 0;
}
