// ysb_parked.h -- parked views: the jedis.get half of RedisAdCampaignCache.execute
// (RedisAdCampaignCache.java:23-35) for the device join.  A view whose ad is in no device
// table is not dropped: it is parked as a self-contained record until the host has asked Redis
// for the ad, upserted what Redis knew (ysb_ad_map_upsert) and resolved the log against the
// tables as they are then (ysb_parked_enable / _keys / _resolve, include/ysb_hip.h).
//
// No HIP here: the record format, the rules the kernels (ysb_parked.hip, and the park sites of
// defer_kernel and colcount_kernel in the scan unit) apply, and a host model of the whole
// park -> distinct -> resolve cycle that tests/native/parked_logic.cpp runs on the CPU.
#pragma once
#include <algorithm>
#include <vector>

#include "ysb_common.h"
#include "ysb_window.h"

namespace ysb {

// One parked view, PARK_WORDS u32 (72 bytes): the decoded ad_id in the join tables' own key
// form (KEY_WORDS zero-padded words, as span_key produces it), its length, whether
// Long.parseLong(event_time) succeeded, and the parsed value.  The reference parses the time
// only after the join (CampaignProcessorCommon.java:58), so the outcome is stored, not tallied.
enum : u32 { PARK_LEN = KEY_WORDS, PARK_FLAGS = KEY_WORDS + 1, PARK_TIME = KEY_WORDS + 2, PARK_WORDS = KEY_WORDS + 4 };
enum : u32 { PARK_TIME_OK = 1u };
constexpr u32 PARK_KEY_STRIDE = MAX_KEY_BYTES;   // ysb_parked_keys' output: 56-byte-stride keys

YSB_HD void park_pack(u32* rec, const u32* kw, u32 len, bool time_ok, i64 t) {
    for (u32 k = 0; k < KEY_WORDS; ++k) rec[k] = kw[k];
    rec[PARK_LEN] = len;
    rec[PARK_FLAGS] = time_ok ? (u32)PARK_TIME_OK : 0u;
    rec[PARK_TIME] = (u32)(u64)t;
    rec[PARK_TIME + 1] = (u32)((u64)t >> 32);
}
YSB_HD bool park_time(const u32* rec, i64* t) {
    *t = (i64)(((u64)rec[PARK_TIME + 1] << 32) | (u64)rec[PARK_TIME]);
    return (rec[PARK_FLAGS] & PARK_TIME_OK) != 0;
}
YSB_HD bool park_same_key(const u32* a, const u32* b) {
    u32 d = a[PARK_LEN] ^ b[PARK_LEN];
    for (u32 k = 0; k < KEY_WORDS; ++k) d |= a[k] ^ b[k];
    return d == 0;
}

// Whether a view that reached the final miss verdict parks: its ad_id must be a possible map
// key (span_key true: at most 56 bytes) and, on a sharded context, belong to this rank's
// shard -- a foreign key stays foreign_shard.  h: key_hash of the key.
YSB_HD bool park_wanted(bool keyed, u32 h, u32 shard_rank, u32 shard_n) {
    return keyed && (shard_n <= 1u || key_shard(h, shard_n) == shard_rank);
}

// The device counters of a context's log (u32 words; PK_MINB and PK_DROPPED are 64 bits wide).
// PK_CLAIMED: views that claimed a slot; it passes the capacity by at most the waves that raced
// for the last slots, so records in the log = min(claimed, capacity).
enum : u32 { PK_CLAIMED = 0, PK_DISTINCT, PK_JOINED, PK_MISSED, PK_TIME_ERR, PK_PAD, PK_MINB, PK_DROPPED = 8, PK_COUNT_ = 10 };

// ---- distinct keys: an open-addressing table of record indices ---------------------------
// slots (a power of two, >= 2 x capacity) start EMPTY_SLOT.  Record i claims the first free
// slot of its key's linear probe with a compare-and-swap (cas(slot, i) -> the slot's previous
// value); a slot that names a record with an equal key makes i a duplicate, any other record
// is probed past.  Exactly one record per key comes out as its representative.
enum : u32 { PARK_REP = 0, PARK_DUP = 1, PARK_FULL = 2 };
YSB_HD u64 park_distinct_slots(u64 capacity) {
    u64 s = 2;
    while (s < 2 * capacity) s <<= 1;
    return s;
}
template <class Cas>
YSB_HD u32 park_distinct_insert(const u32* log, u32 i, u32 mask, Cas&& cas) {
    const u32* r = log + (u64)i * PARK_WORDS;
    const u32 h = key_hash(r, r[PARK_LEN]);
    for (u64 p = 0; p <= mask; ++p) {
        const u32 prev = cas((h + (u32)p) & mask, i);
        if (prev == EMPTY_SLOT) return PARK_REP;
        if (park_same_key(log + (u64)prev * PARK_WORDS, r)) return PARK_DUP;
    }
    return PARK_FULL;   // (never with slots >= 2 x records)
}

// ---- the resolve ------------------------------------------------------------------------
// What a record becomes once the tables have been asked again: a found ad is joined, and only
// then does its time count (a bad one is a time error, a good one is counted into its
// window); an ad still unknown is the reference's null from jedis.get, a join miss.
enum : u32 { PARK_R_COUNT = 0, PARK_R_TIME_ERR = 1, PARK_R_MISS = 2 };
YSB_HD u32 park_resolve_class(bool found, bool time_ok) {
    return !found ? (u32)PARK_R_MISS : time_ok ? (u32)PARK_R_COUNT : (u32)PARK_R_TIME_ERR;
}
// The ring base a resolve fixes when no batch has fixed one: the smallest bucket among the
// records it counts, under the auto-base kernels' rule (ysb_window.h).
YSB_HD i64 park_ring_base(i64 min_bucket, u32 ring_w) { return ring_base_for(min_bucket, ring_w); }

// ---- host model --------------------------------------------------------------------------
// The cycle on plain host data: miss() is the park site, distinct() the distinct kernel,
// resolve() the resolve kernels.  find(kw, len) -> campaign or EMPTY_SLOT is the general
// table's probe; add(campaign, bucket) the count of one view.
struct ParkTally {
    u64 parked = 0, dropped = 0, misses = 0, foreign = 0;          // the park sites
    u64 joined = 0, time_errors = 0, resolved_misses = 0;          // the resolves
};

struct ParkModel {
    u32 cap = 0, shard_rank = 0, shard_n = 1;
    std::vector<u32> log;   // records parked now
    ParkTally t;

    u64 parked_now() const { return log.size() / PARK_WORDS; }

    // A view with the final miss verdict.  keyed: its ad_id is at most 56 bytes (kw, len).
    void miss(bool keyed, const u32* kw, u32 len, bool time_ok, i64 time) {
        if (!park_wanted(keyed, keyed ? key_hash(kw, len) : 0u, shard_rank, shard_n)) {
            ++(keyed && shard_n > 1 ? t.foreign : t.misses);
            return;
        }
        if (parked_now() >= cap) {   // a full log: a join miss as without parking, and told
            ++t.misses;
            ++t.dropped;
            return;
        }
        log.resize(log.size() + PARK_WORDS);
        park_pack(&log[log.size() - PARK_WORDS], kw, len, time_ok, time);
        ++t.parked;
    }

    // The representatives' record indices (one per distinct key; order unspecified).
    std::vector<u32> distinct(u64 slots) const {
        std::vector<u32> tab(slots, EMPTY_SLOT), out;
        for (u32 i = 0; i < (u32)parked_now(); ++i) {
            const u32 r = park_distinct_insert(log.data(), i, (u32)(slots - 1), [&](u32 s, u32 v) {
                const u32 prev = tab[s];
                if (prev == EMPTY_SLOT) tab[s] = v;
                return prev;
            });
            if (r != PARK_DUP) out.push_back(i);
        }
        return out;
    }

    // The log against the map as it is now; the log is then empty.  The ring base, when not
    // set, comes from the records counted here.
    template <class Find, class Add>
    void resolve(Find&& find, Add&& add, const DivMagic& div, u32 ring_w, bool* ring_set, i64* ring_lo) {
        const u64 n = parked_now();
        std::vector<u32> camp(n);
        i64 minb = INT64_MAX;
        for (u64 i = 0; i < n; ++i) {
            const u32* r = &log[i * PARK_WORDS];
            i64 tv;
            const bool ok = park_time(r, &tv);
            camp[i] = find(r, r[PARK_LEN]);
            if (park_resolve_class(camp[i] != EMPTY_SLOT, ok) == PARK_R_COUNT) minb = std::min(minb, div_trunc(tv, div));
        }
        if (!*ring_set && minb != INT64_MAX) {
            *ring_lo = park_ring_base(minb, ring_w);
            *ring_set = true;
        }
        for (u64 i = 0; i < n; ++i) {
            const u32* r = &log[i * PARK_WORDS];
            i64 tv;
            const bool ok = park_time(r, &tv);
            switch (park_resolve_class(camp[i] != EMPTY_SLOT, ok)) {
            case PARK_R_MISS: ++t.resolved_misses; break;
            case PARK_R_TIME_ERR: ++t.joined; ++t.time_errors; break;
            default: ++t.joined; add(camp[i], div_trunc(tv, div));
            }
        }
        log.clear();
    }
};

}  // namespace ysb
