// ysb_admap.h -- the ad -> campaign join tables as plain host data: everything
// ysb_load_ad_map decides before it touches the GPU (the general linear-probe table, the
// 36-byte-key cuckoo table in its slot or bucket layout, the seed-and-retry loop), the host
// restatements of the scan's three probes, and the shard hash; and the rules of the live map
// (ysb_ad_map_upsert): a call's records, the searches, the placement chains and the first-fit
// routine as host/device routines that ysb_upsert.hip's kernels call too, the in-place /
// rebuild rule, the host model of the device passes and the rebuild's merge.  No HIP and no
// context (the table layouts are ysb_common.h's, the error codes the C ABI's plain header), so
// tests/native/admap_logic.cpp and upsert_logic.cpp check it without a GPU; ysb_capi.cpp
// uploads the result.
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

// ---- the two placement chains, one routine per layout: the builders below run them per
// key, ysb_upsert.hip's upsert_evict_kernel runs them on the device for the keys an in-place
// upsert could not place first-fit, and the host model of that upsert (upsert_in_place) runs
// them too -- so tests/native/upsert_logic.cpp checks the code the device runs.  Plain word
// loops: no library call, nothing but loads and stores of the table.

// Where a key ended up: CK_FIRST / CK_SECOND its first / second slot or bucket without moving
// another key, CK_MOVED placed by evictions, CK_OUT the key in hand when the kicks ran out
// (not necessarily the one given) is in no slot or bucket.
enum : u32 { CK_OUT = 0, CK_FIRST = 1, CK_SECOND = 2, CK_MOVED = 3 };
enum : int { CUCKOO_MAX_KICKS = 500 };

// Bucket layout: a key goes to its first bucket while that has a free entry, else to its
// second; with both full it takes a random entry of the bucket it is headed for (which so
// stays full) and the evicted key tries only its other bucket.  So a key sits in its second
// bucket only while its first is full -- the probe's rule.  *rng: the eviction draws' state.
YSB_HD u32 cuckoo_place_buckets(u32* ct, u32 mask, const CuckooSeed& cs, const u32* key, u32 camp, u64* rng) {
    u32 k[CKEY_WORDS];
    for (u32 j = 0; j < CKEY_WORDS; ++j) k[j] = key[j];
    u32 c = camp;
    u32 a, b;
    cuckoo_slots36(k, cs, mask, &a, &b);
    u32 pos = a;
    for (int kicks = 0; kicks <= CUCKOO_MAX_KICKS; ++kicks) {
        const u32 cands[2] = {pos, pos == a ? b : a};
        for (int ci = 0; ci < (kicks == 0 ? 2 : 1); ++ci) {
            u32* bk = &ct[(u64)cands[ci] * CB_WORDS];
            for (u32 e = 0; e < CB_ENTRIES; ++e)
                if (bk[e * CB_STRIDE + CKEY_WORDS] == EMPTY_SLOT) {
                    for (u32 j = 0; j < CKEY_WORDS; ++j) bk[e * CB_STRIDE + j] = k[j];
                    bk[e * CB_STRIDE + CKEY_WORDS] = c;
                    return kicks ? (u32)CK_MOVED : ci ? (u32)CK_SECOND : (u32)CK_FIRST;
                }
        }
        *rng = mix64(*rng + 1);
        u32* en = &ct[(u64)pos * CB_WORDS + (u32)(*rng % CB_ENTRIES) * CB_STRIDE];
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
    return CK_OUT;
}

// Slot layout: a key takes its first slot and evicts the occupant to that one's other slot,
// up to CUCKOO_MAX_KICKS kicks.
YSB_HD u32 cuckoo_place_slots(u32* ct, u32 mask, const CuckooSeed& cs, const u32* key, u32 camp) {
    u32 k[CKEY_WORDS];
    for (u32 j = 0; j < CKEY_WORDS; ++j) k[j] = key[j];
    u32 camp_k = camp, a, b;
    cuckoo_slots36(k, cs, mask, &a, &b);
    u32 pos = a;
    for (int kicks = 0;;) {
        u32* sl = &ct[(u64)pos * CSLOT_WORDS];
        if (sl[CSLOT_CAMP] == EMPTY_SLOT) {
            for (u32 j = 0; j < CKEY_WORDS; ++j) sl[j] = k[j];
            sl[CSLOT_CAMP] = camp_k;
            return kicks ? (u32)CK_MOVED : (u32)CK_FIRST;
        }
        // evict the occupant to its other slot
        for (u32 j = 0; j < CKEY_WORDS; ++j) {
            const u32 t = sl[j];
            sl[j] = k[j];
            k[j] = t;
        }
        const u32 oc = sl[CSLOT_CAMP];
        sl[CSLOT_CAMP] = camp_k;
        camp_k = oc;
        cuckoo_slots36(k, cs, mask, &a, &b);
        pos = (pos == a) ? b : a;
        if (++kicks > CUCKOO_MAX_KICKS) return CK_OUT;
    }
}

// Host build of the bucket-layout table (ysb_load_ad_map): key i (9 words) with campaign
// camp[i] into nb buckets (ct: nb * CB_WORDS words, cleared here) by cuckoo_place_buckets.
// Returns the keys left out (keep_going: placement goes on without them, a partial table;
// else it stops at the first).
static inline u64 cuckoo_build_buckets(const u32* keys, const u32* camp, u64 n, const CuckooSeed& cs, u64 nb,
                                       u64 seed, bool keep_going, u32* ct) {
    for (u64 i = 0; i < nb * CB_WORDS; ++i) ct[i] = 0;
    for (u64 b = 0; b < nb; ++b)
        for (u32 e = 0; e < CB_ENTRIES; ++e) ct[b * CB_WORDS + e * CB_STRIDE + CKEY_WORDS] = EMPTY_SLOT;
    const u32 mask = (u32)(nb - 1);
    u64 rng = seed, homeless = 0;
    for (u64 i = 0; i < n; ++i) {
        if (cuckoo_place_buckets(ct, mask, cs, keys + i * CKEY_WORDS, camp[i], &rng)) continue;
        ++homeless;
        if (!keep_going) return homeless;
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
// CSLOT_WORDS words, cleared here) by cuckoo_place_slots; the key in hand when the kicks run
// out is the one left out.
static inline u64 cuckoo_build_slots(const u32* keys, const u32* camp, u64 n, const CuckooSeed& cs, u64 cslots,
                                     bool keep_going, u32* ct) {
    for (u64 i = 0; i < cslots * CSLOT_WORDS; ++i) ct[i] = 0;
    for (u64 s = 0; s < cslots; ++s) ct[s * CSLOT_WORDS + CSLOT_CAMP] = EMPTY_SLOT;
    const u32 cm = (u32)(cslots - 1);
    u64 homeless = 0;
    for (u64 i = 0; i < n; ++i) {
        if (!cuckoo_place_slots(ct, cm, cs, keys + i * CKEY_WORDS, camp[i])) ++homeless;
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
// its misses must go to the general path.  keys: the distinct keys of the map (the general
// table's occupied slots); keys36: the 36-byte keys the cuckoo table holds (what the sizing
// rules of build_join_tables and of an in-place upsert, upsert_fits, count).
struct JoinTables {
    std::vector<u32> table, ctable;
    u64 slots = 0, cslots = 0;
    u64 keys = 0, keys36 = 0;
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
    u64 keys = 0;
    for (u64 sl = 0; sl < slots; ++sl) {
        const u32* e = &tab[sl * SLOT_WORDS];
        keys += e[1] != EMPTY_SLOT;
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
    u64 seed = 0x5EEDC0FFEEULL, homeless = 0;
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
        homeless =
            buckets ? cuckoo_build_buckets(kw.data(), cv.data(), cv.size(), out->cseed, cslots, seed, partial, ct.data())
                    : cuckoo_build_slots(kw.data(), cv.data(), cv.size(), out->cseed, cslots, partial, ct.data());
        if (homeless == 0 || partial) break;
    }
    out->slots = slots;
    out->cslots = cslots;
    out->buckets = buckets;
    out->partial = partial;
    out->keys = keys;
    out->keys36 = cv.size() - homeless;
    return YSB_OK;
}

// ---- ysb_ad_map_upsert: entries added to live tables (HashMap.put on a live map) --------
// An entry travels as a record in the general table's own slot format {len, campaign, 14 key
// words}.  The device works in three passes (ysb_upsert.hip): classify (a known key's
// campaign is rewritten where the key sits, a new key is listed), insert (each new key claims
// the first free slot of its linear probe and, 36 bytes long, the first free entry of its
// first, else its second, slot or bucket), evict (the keys that found both full go through
// the builders' chains above, serially).  Below: the searches both sides share, the rule that
// decides between in place and rebuild, and the host model of the three passes.

// The records of one call: every entry checked as build_join_tables checks it (nothing is
// produced if one fails), entries of another shard skipped (*foreign), an id given more than
// once collapsed to its last campaign (*duplicates counts the earlier ones) -- so the
// records are distinct keys, in the order of their first appearance.
inline int upsert_records(const char* const* ad_ids, const u32* lens, const u32* campaign_idx, u64 n,
                          u32 n_campaigns, u32 shard_rank, u32 shard_n, std::vector<u32>* rec, u64* foreign,
                          u64* duplicates, std::string* err) {
    char msg[128];
    auto bad = [&](int code, const char* fmt, unsigned long long x, unsigned y) {
        std::snprintf(msg, sizeof msg, fmt, x, y);
        *err = msg;
        return code;
    };
    for (u64 i = 0; i < n; ++i) {
        const u32 len = lens ? lens[i] : 36u;
        if (len > MAX_KEY_BYTES) return bad(YSB_ERR_FORMAT, "ad id %llu longer than %u bytes", i, MAX_KEY_BYTES);
        if (campaign_idx[i] >= n_campaigns)
            return bad(YSB_ERR_FORMAT, "campaign index %llu >= n_campaigns %u", campaign_idx[i], n_campaigns);
        if (!ad_ids[i] && len) return bad(YSB_ERR_ARG, "ad id %llu is NULL", i, 0);
    }
    rec->clear();
    *foreign = *duplicates = 0;
    u64 cells = 64;
    while (cells < 2 * n) cells <<= 1;
    std::vector<u32> seen(cells, EMPTY_SLOT);   // open addressing by key_hash: the key's record
    rec->reserve(n * SLOT_WORDS);
    for (u64 i = 0; i < n; ++i) {
        const u32 len = lens ? lens[i] : 36u;
        u32 r[SLOT_WORDS] = {len, campaign_idx[i]};
        if (len) std::memcpy(r + 2, ad_ids[i], len);
        const u32 h = key_hash(r + 2, len);
        if (shard_n > 1 && key_shard(h, shard_n) != shard_rank) { ++*foreign; continue; }   // (ad_shard)
        for (u64 pr = h & (cells - 1);; pr = (pr + 1) & (cells - 1)) {
            if (seen[pr] == EMPTY_SLOT) {
                seen[pr] = (u32)(rec->size() / SLOT_WORDS);
                rec->insert(rec->end(), r, r + SLOT_WORDS);
                break;
            }
            u32* have = &(*rec)[(u64)seen[pr] * SLOT_WORDS];
            if (have[0] != len || std::memcmp(have + 2, r + 2, KEY_WORDS * 4) != 0) continue;
            have[1] = campaign_idx[i];   // HashMap.put: later wins
            ++*duplicates;
            break;
        }
    }
    return YSB_OK;
}

// The general table's slot that holds the len-byte key kw (KEY_WORDS zero-padded words), by
// the scan's linear probe (table_lookup's walk); -1: the key is not in the map.
YSB_HD i64 table_find(const u32* tab, u32 mask, const u32* kw, u32 len) {
    const u32 h = key_hash(kw, len);
    for (u64 i = 0; i <= mask; ++i) {
        const u64 s = (h + (u32)i) & mask;
        const u32* sl = &tab[s * SLOT_WORDS];
        if (sl[1] == EMPTY_SLOT) return -1;
        if (sl[0] != len) continue;
        u32 d = 0;
        for (u32 j = 0; j < KEY_WORDS; ++j) d |= sl[2 + j] ^ kw[j];
        if (d == 0) return (i64)s;
    }
    return -1;
}

// The word of the cuckoo table that holds key k's campaign, by the scan's probes
// (cuckoo_lookup_slots / cuckoo_lookup_buckets); *where: 1 / 2 the key's first / second slot
// or bucket.  CK_NONE: the key is not in the cuckoo table.
constexpr u64 CK_NONE = ~0ull;
YSB_HD u64 cuckoo_find_slots(const u32* ct, u32 mask, const CuckooSeed& cs, const u32* k, u32* where) {
    u32 ab[2];
    cuckoo_slots36(k, cs, mask, &ab[0], &ab[1]);
    for (u32 r = 0; r < 2; ++r) {
        const u64 at = (u64)ab[r] * CSLOT_WORDS;
        if (ct[at + CSLOT_CAMP] == EMPTY_SLOT) continue;
        u32 d = 0;
        for (u32 j = 0; j < CKEY_WORDS; ++j) d |= ct[at + j] ^ k[j];
        if (d == 0) { *where = r + 1; return at + CSLOT_CAMP; }
    }
    return CK_NONE;
}
YSB_HD u64 cuckoo_find_buckets(const u32* ct, u32 mask, const CuckooSeed& cs, const u32* k, u32* where) {
    u32 ab[2];
    cuckoo_slots36(k, cs, mask, &ab[0], &ab[1]);
    for (u32 r = 0; r < 2; ++r) {
        bool full = true;
        for (u32 e = 0; e < CB_ENTRIES; ++e) {
            const u64 at = (u64)ab[r] * CB_WORDS + e * CB_STRIDE;
            if (ct[at + CKEY_WORDS] == EMPTY_SLOT) { full = false; continue; }
            u32 d = 0;
            for (u32 j = 0; j < CKEY_WORDS; ++j) d |= ct[at + j] ^ k[j];
            if (d == 0) { *where = r + 1; return at + CKEY_WORDS; }
        }
        if (!full) return CK_NONE;   // a key sits in its second bucket only while its first is full
    }
    return CK_NONE;
}

// In place or rebuild: an upsert works in place exactly while build_join_tables' own sizing
// rules still hold for the grown map -- keys distinct keys in slots general slots (load <=
// 1/2), keys36 36-byte keys in cslots cuckoo slots (load <= 1/4) or buckets (>=
// YSB_BUCKETS_X4 / 4 buckets per key) -- so an upserted table is never denser than a fresh
// load could be.
YSB_HD bool upsert_fits(u64 keys, u64 keys36, u64 slots, u64 cslots, bool buckets) {
    return 2 * keys <= slots && (buckets ? (u64)YSB_BUCKETS_X4 * keys36 <= 4 * cslots : 4 * keys36 <= cslots);
}

// The state the eviction draws of an in-place upsert into a bucket table start from.
YSB_HD u64 upsert_rng(const CuckooSeed& cs, u64 keys) { return mix64((((u64)cs.fb << 32) | cs.fa) + keys); }

struct UpsertCounts {
    u64 updated = 0, inserted = 0, inserted36 = 0, first = 0, second = 0, moved = 0, left_out = 0;
};

// The slot (slot layout) or entry (bucket layout) a new key claims first-fit: the campaign
// word's index and CK_FIRST / CK_SECOND, or CK_OUT with both full.  `taken(word)` tells
// whether the entry with that campaign word is taken and claims it if not (the device: a
// compare-and-swap; the host model: a plain test and store).
template <class Claim>
YSB_HD u32 cuckoo_first_fit(u32 mask, bool buckets, const CuckooSeed& cs, const u32* k, Claim&& taken, u64* at) {
    u32 ab[2];
    cuckoo_slots36(k, cs, mask, &ab[0], &ab[1]);
    for (u32 r = 0; r < 2; ++r)
        for (u32 e = 0; e < (buckets ? (u32)CB_ENTRIES : 1u); ++e) {
            const u64 key_at = buckets ? (u64)ab[r] * CB_WORDS + e * CB_STRIDE : (u64)ab[r] * CSLOT_WORDS;
            if (taken(key_at + CKEY_WORDS)) continue;   // (CSLOT_CAMP == CKEY_WORDS)
            *at = key_at;
            return r ? (u32)CK_SECOND : (u32)CK_FIRST;
        }
    return CK_OUT;
}
static_assert(CSLOT_CAMP == CKEY_WORDS, "a slot and a bucket entry are both [9 key words, campaign]");

// Host model of an in-place upsert of n records (distinct keys) into jt, pass by pass as the
// device does it; the caller has checked upsert_fits for the grown map.  sparse
// (YSB_F_SPARSE_FAST_JOIN): every other new 36-byte key is left out of the cuckoo table.
inline void upsert_in_place(JoinTables* jt, const u32* rec, u64 n, bool sparse, UpsertCounts* out) {
    u32* tab = jt->table.data();
    u32* ct = jt->ctable.data();
    const u32 mask = (u32)(jt->slots - 1), cmask = (u32)(jt->cslots - 1);
    UpsertCounts uc;
    std::vector<u64> fresh, homeless;
    for (u64 i = 0; i < n; ++i) {   // classify
        const u32* r = rec + i * SLOT_WORDS;
        const i64 s = table_find(tab, mask, r + 2, r[0]);
        if (s < 0) { fresh.push_back(i); continue; }
        tab[(u64)s * SLOT_WORDS + 1] = r[1];
        ++uc.updated;
        if (r[0] != 36) continue;
        u32 where;
        const u64 w = jt->buckets ? cuckoo_find_buckets(ct, cmask, jt->cseed, r + 2, &where)
                                  : cuckoo_find_slots(ct, cmask, jt->cseed, r + 2, &where);
        if (w != CK_NONE) ct[w] = r[1];
    }
    for (u64 i : fresh) {   // insert
        const u32* r = rec + i * SLOT_WORDS;
        const u32 h = key_hash(r + 2, r[0]);
        for (u64 pr = 0;; ++pr) {
            u32* sl = &tab[(u64)((h + (u32)pr) & mask) * SLOT_WORDS];
            if (sl[1] != EMPTY_SLOT) continue;
            std::memcpy(sl, r, SLOT_WORDS * 4);
            break;
        }
        ++uc.inserted;
        if (r[0] != 36) continue;
        const u64 ord = uc.inserted36++;
        if (sparse && !(ord & 1)) { ++uc.left_out; continue; }   // the keys at odd positions stay
        u64 at = 0;
        const u32 where = cuckoo_first_fit(cmask, jt->buckets, jt->cseed, r + 2, [&](u64 w) {
            if (ct[w] != EMPTY_SLOT) return true;
            ct[w] = r[1];
            return false;
        }, &at);
        if (where == CK_OUT) { homeless.push_back(i); continue; }
        std::memcpy(ct + at, r + 2, 36);
        ++(where == CK_FIRST ? uc.first : uc.second);
    }
    u64 rng = upsert_rng(jt->cseed, jt->keys);
    for (u64 i : homeless) {   // evict
        const u32* r = rec + i * SLOT_WORDS;
        const u32 where = jt->buckets ? cuckoo_place_buckets(ct, cmask, jt->cseed, r + 2, r[1], &rng)
                                      : cuckoo_place_slots(ct, cmask, jt->cseed, r + 2, r[1]);
        ++(where == CK_OUT ? uc.left_out : uc.moved);
    }
    if (uc.left_out) jt->partial = true;
    jt->keys += uc.inserted;
    jt->keys36 += uc.first + uc.second + uc.moved;
    *out = uc;
}

// The rebuild's merge: every entry of a general table (slots slots) as records, then the
// call's records -- what build_join_tables_rec turns into the tables of the grown map (the
// call's campaigns win: they come later).
inline void upsert_merge(const u32* table, u64 slots, const u32* rec, u64 n, std::vector<u32>* merged) {
    merged->clear();
    for (u64 s = 0; s < slots; ++s)
        if (table[s * SLOT_WORDS + 1] != EMPTY_SLOT)
            merged->insert(merged->end(), table + s * SLOT_WORDS, table + (s + 1) * SLOT_WORDS);
    merged->insert(merged->end(), rec, rec + n * SLOT_WORDS);
}
inline int build_join_tables_rec(const std::vector<u32>& rec, u32 n_campaigns, bool sparse, JoinTables* out,
                                 std::string* err) {
    const u64 n = rec.size() / SLOT_WORDS;
    std::vector<const char*> ids(n);
    std::vector<u32> lens(n), camp(n);
    for (u64 i = 0; i < n; ++i) {
        ids[i] = reinterpret_cast<const char*>(&rec[i * SLOT_WORDS + 2]);
        lens[i] = rec[i * SLOT_WORDS];
        camp[i] = rec[i * SLOT_WORDS + 1];
    }
    return build_join_tables(ids.data(), lens.data(), camp.data(), n, n_campaigns, sparse, out, err);
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
