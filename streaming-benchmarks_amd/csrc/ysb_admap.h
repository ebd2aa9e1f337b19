// ysb_admap.h -- the ad -> campaign join tables as plain host data: everything
// ysb_load_ad_map decides before it touches the GPU (the general linear-probe table, the
// 36-byte-key cuckoo table in its slot or bucket layout, the seed-and-retry loop), the host
// restatements of the scan's three probes, and the shard hash.  No HIP and no context (the
// table layouts are ysb_common.h's, the error codes the C ABI's plain header), so
// tests/native/admap_logic.cpp checks it without a GPU; ysb_capi.cpp uploads the result.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ysb_hip.h"
#include "ysb_common.h"

// HBM-resident join table (bucket layout): buckets per key, x4 (8: 2 per key, a 4 GiB
// table at 10M ads; fewer buckets -> a smaller table, more keys in their second bucket)
#ifndef YSB_BUCKETS_X4
#define YSB_BUCKETS_X4 8
#endif

namespace ysb {

// Host build of the bucket-layout table (ysb_load_ad_map): key i (9 words) with campaign
// camp[i] into nb buckets (ct: nb * CB_WORDS words, cleared here).  A key goes to its
// first bucket while that has a free entry, else to its second; with both full it takes a
// random entry of the bucket it is headed for (which so stays full) and the evicted key
// tries only its other bucket.  So a key sits in its second bucket only while its first
// is full -- the probe's rule.  Returns the keys left out (keep_going: placement goes on
// without them, a partial table; else it stops at the first).
static inline u64 cuckoo_build_buckets(const u32* keys, const u32* camp, u64 n, const CuckooSeed& cs, u64 nb,
                                       u64 seed, bool keep_going, u32* ct) {
    for (u64 i = 0; i < nb * CB_WORDS; ++i) ct[i] = 0;
    for (u64 b = 0; b < nb; ++b)
        for (u32 e = 0; e < CB_ENTRIES; ++e) ct[b * CB_WORDS + e * CB_STRIDE + CKEY_WORDS] = EMPTY_SLOT;
    const u32 mask = (u32)(nb - 1);
    u64 rng = seed, homeless = 0;
    for (u64 i = 0; i < n; ++i) {
        u32 k[CKEY_WORDS];
        for (u32 j = 0; j < CKEY_WORDS; ++j) k[j] = keys[i * CKEY_WORDS + j];
        u32 c = camp[i];
        u32 a, b;
        cuckoo_slots36(k, cs, mask, &a, &b);
        u32 pos = a;
        bool placed = false;
        for (int kicks = 0; kicks <= 500 && !placed; ++kicks) {
            const u32 cands[2] = {pos, pos == a ? b : a};
            for (int ci = 0; ci < (kicks == 0 ? 2 : 1) && !placed; ++ci) {
                u32* bk = &ct[(u64)cands[ci] * CB_WORDS];
                for (u32 e = 0; e < CB_ENTRIES && !placed; ++e)
                    if (bk[e * CB_STRIDE + CKEY_WORDS] == EMPTY_SLOT) {
                        for (u32 j = 0; j < CKEY_WORDS; ++j) bk[e * CB_STRIDE + j] = k[j];
                        bk[e * CB_STRIDE + CKEY_WORDS] = c;
                        placed = true;
                    }
            }
            if (placed) break;
            rng = mix64(rng + 1);
            u32* en = &ct[(u64)pos * CB_WORDS + (u32)(rng % CB_ENTRIES) * CB_STRIDE];
            for (u32 j = 0; j < CKEY_WORDS; ++j) {
                const u32 t = en[j];
                en[j] = k[j];
                k[j] = t;
            }
            const u32 oc = en[CKEY_WORDS];
            en[CKEY_WORDS] = c;
            c = oc;
            cuckoo_slots36(k, cs, mask, &a, &b);
            pos = (pos == a) ? b : a;   // the evicted key's other bucket
        }
        if (!placed) {
            ++homeless;
            if (!keep_going) return homeless;
        }
    }
    return homeless;
}

// Host restatement of the scan's bucket probe (ysb_scan.hip bucket_find + the second
// bucket after a miss in a full first one): the campaign, or EMPTY_SLOT.
static inline u32 cuckoo_lookup_buckets(const u32* ct, u64 nb, const CuckooSeed& cs, const u32* k) {
    u32 a, b;
    cuckoo_slots36(k, cs, (u32)(nb - 1), &a, &b);
    for (int round = 0; round < 2; ++round) {
        const u32* bk = &ct[(u64)(round ? b : a) * CB_WORDS];
        bool full = true;
        for (u32 e = 0; e < CB_ENTRIES; ++e) {
            const u32 c = bk[e * CB_STRIDE + CKEY_WORDS];
            if (c == EMPTY_SLOT) { full = false; continue; }
            bool eq = true;
            for (u32 j = 0; j < CKEY_WORDS; ++j) eq &= bk[e * CB_STRIDE + j] == k[j];
            if (eq) return c;
        }
        if (!full) return EMPTY_SLOT;
    }
    return EMPTY_SLOT;
}

static inline CuckooSeed cuckoo_seed(u64 seed) {
    CuckooSeed cs;
    for (u32 k = 0; k < CKEY_WORDS; ++k) {
        const u64 r = mix64(seed + 2 * k + 1);
        cs.s[k] = (u32)r;
        cs.t[k] = (u32)(r >> 32);
    }
    const u64 f = mix64(seed ^ 0xF1F1F1F1F1F1F1F1ULL);
    cs.fa = (u32)f;
    cs.fb = (u32)(f >> 32);
    return cs;
}

// Host build of the slot-layout table, the bucket builder's contract (ct: cslots *
// CSLOT_WORDS words, cleared here): a key takes its first slot and evicts the occupant to
// that one's other slot, up to 500 kicks; the key in hand when they run out is the one
// left out.
static inline u64 cuckoo_build_slots(const u32* keys, const u32* camp, u64 n, const CuckooSeed& cs, u64 cslots,
                                     bool keep_going, u32* ct) {
    for (u64 i = 0; i < cslots * CSLOT_WORDS; ++i) ct[i] = 0;
    for (u64 s = 0; s < cslots; ++s) ct[s * CSLOT_WORDS + CSLOT_CAMP] = EMPTY_SLOT;
    const u32 cm = (u32)(cslots - 1);
    u64 homeless = 0;
    for (u64 i = 0; i < n; ++i) {
        u32 k[CKEY_WORDS], occ[CKEY_WORDS];
        std::memcpy(k, keys + i * CKEY_WORDS, 36);
        u32 camp_k = camp[i], a, b;
        cuckoo_slots36(k, cs, cm, &a, &b);
        u32 pos = a;
        for (int kicks = 0;;) {
            u32* sl = &ct[(u64)pos * CSLOT_WORDS];
            if (sl[CSLOT_CAMP] == EMPTY_SLOT) {
                std::memcpy(sl, k, 36);
                sl[CSLOT_CAMP] = camp_k;
                break;
            }
            // evict the occupant to its other slot
            std::memcpy(occ, sl, 36);
            const u32 oc = sl[CSLOT_CAMP];
            std::memcpy(sl, k, 36);
            sl[CSLOT_CAMP] = camp_k;
            std::memcpy(k, occ, 36);
            camp_k = oc;
            cuckoo_slots36(k, cs, cm, &a, &b);
            pos = (pos == a) ? b : a;
            if (++kicks > 500) { ++homeless; break; }
        }
        if (homeless && !keep_going) return homeless;
    }
    return homeless;
}

// Host restatement of the scan's two-slot probe (ysb_scan.hip, phase B2 without SERIAL):
// slot a when it holds the key and is not empty, else slot b when it holds the key.
static inline u32 cuckoo_lookup_slots(const u32* ct, u64 cslots, const CuckooSeed& cs, const u32* k) {
    u32 a, b;
    cuckoo_slots36(k, cs, (u32)(cslots - 1), &a, &b);
    const u32 *sa = &ct[(u64)a * CSLOT_WORDS], *sb = &ct[(u64)b * CSLOT_WORDS];
    if (std::memcmp(sa, k, 36) == 0 && sa[CSLOT_CAMP] != EMPTY_SLOT) return sa[CSLOT_CAMP];
    return std::memcmp(sb, k, 36) == 0 ? sb[CSLOT_CAMP] : EMPTY_SLOT;
}

// Host restatement of the scan's linear probe (ysb_scan.hip probe) over the general table:
// the campaign of the len-byte key, or EMPTY_SLOT.
static inline u32 table_lookup(const u32* tab, u64 slots, const void* key, u32 len) {
    u32 kw[KEY_WORDS] = {0};
    if (len) std::memcpy(kw, key, len);
    const u32 h = key_hash(kw, len), mask = (u32)(slots - 1);
    for (u64 i = 0; i < slots; ++i) {
        const u32* sl = &tab[(u64)((h + (u32)i) & mask) * SLOT_WORDS];
        if (sl[1] == EMPTY_SLOT) return EMPTY_SLOT;
        if (sl[0] == len && std::memcmp(sl + 2, kw, sizeof kw) == 0) return sl[1];
    }
    return EMPTY_SLOT;
}

// What ysb_load_ad_map uploads: the general table (slots * SLOT_WORDS words) and the cuckoo
// table of the 36-byte keys (cslots slots of CSLOT_WORDS words, or with `buckets` cslots
// buckets of CB_WORDS).  partial: some 36-byte key of the map is not in the cuckoo table, so
// its misses must go to the general path.
struct JoinTables {
    std::vector<u32> table, ctable;
    u64 slots = 0, cslots = 0;
    CuckooSeed cseed{};
    bool buckets = false, partial = false;
};

// The tables of n (ad id, campaign index) pairs (lens NULL: every id 36 bytes; a later pair
// replaces an earlier one with the same id, as HashMap.put); sparse is
// YSB_F_SPARSE_FAST_JOIN.  YSB_OK, or the error code with its text in *err.
inline int build_join_tables(const char* const* ad_ids, const u32* lens, const u32* campaign_idx, u64 n,
                             u32 n_campaigns, bool sparse, JoinTables* out, std::string* err) {
    char msg[128];
    auto bad = [&](int code, const char* fmt, unsigned long long x, unsigned y) {
        std::snprintf(msg, sizeof msg, fmt, x, y);
        *err = msg;
        return code;
    };
    u64 slots = 64;
    while (slots < 2 * n) slots <<= 1;   // load factor <= 0.5
    if (slots > (1ull << 31)) return bad(YSB_ERR_CAPACITY, "ad map too large (%llu)", n, 0);
    std::vector<u32>& tab = out->table;
    tab.assign(slots * SLOT_WORDS, 0);
    for (u64 s = 0; s < slots; ++s) tab[s * SLOT_WORDS + 1] = EMPTY_SLOT;
    const u32 mask = (u32)(slots - 1);
    for (u64 i = 0; i < n; ++i) {
        const u32 len = lens ? lens[i] : 36u;
        if (len > MAX_KEY_BYTES) return bad(YSB_ERR_FORMAT, "ad id %llu longer than %u bytes", i, MAX_KEY_BYTES);
        if (campaign_idx[i] >= n_campaigns)
            return bad(YSB_ERR_FORMAT, "campaign index %llu >= n_campaigns %u", campaign_idx[i], n_campaigns);
        if (!ad_ids[i] && len) return bad(YSB_ERR_ARG, "ad id %llu is NULL", i, 0);
        u32 kw[KEY_WORDS] = {0};
        if (len) std::memcpy(kw, ad_ids[i], len);
        const u32 h = key_hash(kw, len);
        for (u64 pr = 0;; ++pr) {
            u32* sl = &tab[(u64)((h + pr) & mask) * SLOT_WORDS];
            if (sl[1] == EMPTY_SLOT) {
                sl[0] = len;
                sl[1] = campaign_idx[i];
                std::memcpy(sl + 2, kw, sizeof kw);
                break;
            }
            if (sl[0] == len && std::memcmp(sl + 2, kw, sizeof kw) == 0) {   // HashMap.put: later wins
                sl[1] = campaign_idx[i];
                break;
            }
        }
    }
    // every 36-byte key also goes into the two-choice cuckoo table (load <= 1/4): the distinct
    // 36-byte keys (as words) with their final (later-wins) campaigns -- the general table
    // already holds exactly that set
    std::vector<u32> kw, cv;
    for (u64 sl = 0; sl < slots; ++sl) {
        const u32* e = &tab[sl * SLOT_WORDS];
        if (e[1] == EMPTY_SLOT || e[0] != 36) continue;
        kw.insert(kw.end(), e + 2, e + 2 + CKEY_WORDS);
        cv.push_back(e[1]);
    }
    bool partial = false;
    if (sparse) {   // the keys at odd positions stay
        for (size_t i = 0; 2 * i + 1 < cv.size(); ++i) {
            std::memcpy(&kw[i * CKEY_WORDS], &kw[(2 * i + 1) * CKEY_WORDS], 36);
            cv[i] = cv[2 * i + 1];
        }
        cv.resize(cv.size() / 2);
        kw.resize(cv.size() * CKEY_WORDS);
        partial = true;
    }
    u64 cslots = 64;
    while (cslots < 4 * cv.size()) cslots <<= 1;
    // tables far beyond the L2s (32 MiB) go to HBM per probe: bucket layout
    const bool buckets = cslots * CSLOT_WORDS * 4 > (64ull << 20);
    if (buckets) {
        // buckets >= YSB_BUCKETS_X4 / 4 per key (3 entries each)
        cslots = 64;
        while (cslots * 4 < (u64)YSB_BUCKETS_X4 * cv.size()) cslots <<= 1;
    }
    std::vector<u32>& ct = out->ctable;
    u64 seed = 0x5EEDC0FFEEULL;
    for (int attempt = 0;; ++attempt) {
        if (attempt == 16) { cslots <<= 1; attempt = 0; }
        if (cslots > (1ull << 26)) {
            // No placement found (a key family the hash cannot separate): keep the
            // table without the keys that did not fit; the scan defers its misses to
            // the general path, so the join stays exact.
            cslots = 1ull << 26;
            partial = true;
        }
        seed = mix64(seed + (u64)attempt + cslots);
        out->cseed = cuckoo_seed(seed);
        ct.resize(buckets ? cslots * CB_WORDS : cslots * CSLOT_WORDS);   // (the builders clear it)
        const u64 homeless =
            buckets ? cuckoo_build_buckets(kw.data(), cv.data(), cv.size(), out->cseed, cslots, seed, partial, ct.data())
                    : cuckoo_build_slots(kw.data(), cv.data(), cv.size(), out->cseed, cslots, partial, ct.data());
        if (homeless == 0 || partial) break;
    }
    out->slots = slots;
    out->cslots = cslots;
    out->buckets = buckets;
    out->partial = partial;
    return YSB_OK;
}

// ysb_ad_shard: the rank of nranks whose join-table shard holds the len-byte ad id.
inline u32 ad_shard(const char* ad_id, u32 len, u32 nranks) {
    if (nranks <= 1) return 0;
    u32 kw[KEY_WORDS] = {0};
    std::memcpy(kw, ad_id, std::min<u32>(len, MAX_KEY_BYTES));
    const u32 h = key_hash(kw, std::min<u32>(len, MAX_KEY_BYTES));
    return (u32)(((u64)mix64(h) >> 32) * nranks >> 32);
}

}  // namespace ysb
