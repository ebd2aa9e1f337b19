// ysb_upsert.hip -- the join tables' own kernels: ysb_ad_map_upsert's three passes (entries
// added to the live general and cuckoo tables between two launches) and ysb_ad_map_lookup.
//
// This is HashMap.put on a live map -- RedisAdCampaignCache.execute's ad_to_campaign.put
// (RedisAdCampaignCache.java:23-35) and getAdCampaignMap's later-wins put
// (AdvertisingTopologyNative.java:47-56) -- done on the device.  The rules (the searches, the
// first-fit placement, the eviction chains) are ysb_admap.h's host/device routines, so
// tests/native/upsert_logic.cpp runs on the CPU what runs here.
//
// What makes it safe beside the scan's probes, which are untouched: the tables only gain
// entries (a slot or entry goes EMPTY_SLOT -> campaign once and is never freed), a new key
// claims the first free slot of its linear probe (no gap before it) and the first free entry
// of its first, else its second, slot or bucket (a key sits in its second bucket only while
// its first is full), and the host keeps the load factors a fresh load would have
// (upsert_fits).  The passes run on the compute stream, between the scans.
//
// Concurrency inside a pass.  The keys of a call are distinct (the host collapses
// duplicates), so in classify no two lanes write the same word.  In insert the only word two
// lanes ever contend on is a slot's or entry's campaign word, and every claim of it is an
// agent-scope compare-and-swap EMPTY_SLOT -> campaign (atomicCAS: device scope, so it is
// decided at the memory side for all eight XCDs).  A plain load of that word first spares the
// atomic on slots that are taken: it may be stale only the harmless way (it reads EMPTY_SLOT
// of a slot claimed meanwhile, and the swap then fails), never taken for a free one, as
// nothing is ever freed.  Key words are written by the claimant with plain stores and read
// by nobody in this pass: the keys are known absent and distinct, so no lane compares key
// words and a half-written neighbour cannot be mistaken for a match.  The kernel boundary
// publishes them to the next pass and to the scans.
#include "ysb_kernels.h"
#include "ysb_admap.h"

namespace ysb {

__device__ __forceinline__ void load_record(const u32* rec, u32 i, u32 (&r)[SLOT_WORDS]) {
    const uint4* p = reinterpret_cast<const uint4*>(rec + (u64)i * SLOT_WORDS);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint4 v = p[q];
        r[4 * q] = v.x;
        r[4 * q + 1] = v.y;
        r[4 * q + 2] = v.z;
        r[4 * q + 3] = v.w;
    }
}

__device__ __forceinline__ u32 lanes_below(u64 mask) {
    return (u32)__popcll(mask & ((1ull << (threadIdx.x & 63)) - 1ull));
}

// Pass 1, one lane per record: a known key's campaign is rewritten in its general slot and in
// its cuckoo slot or entry; a new key's record index is appended to fresh[] (a wave ballot,
// one atomic per wave and counter).
__global__ __launch_bounds__(AUX_TPB) void upsert_classify_kernel(const UpsertParams P) {
    const u32 i = blockIdx.x * AUX_TPB + threadIdx.x;
    bool fresh = false, fresh36 = false, known = false;
    if (i < P.n) {
        u32 r[SLOT_WORDS];
        load_record(P.rec, i, r);
        const i64 s = table_find(P.table, P.table_mask, r + 2, r[0]);
        if (s < 0) {
            fresh = true;
            fresh36 = r[0] == 36;
        } else {
            known = true;
            P.table[(u64)s * SLOT_WORDS + 1] = r[1];
            if (r[0] == 36) {
                u32 where;
                const u64 w = P.buckets ? cuckoo_find_buckets(P.ctable, P.ctable_mask, P.cseed, r + 2, &where)
                                        : cuckoo_find_slots(P.ctable, P.ctable_mask, P.cseed, r + 2, &where);
                if (w != CK_NONE) P.ctable[w] = r[1];
            }
        }
    }
    const u64 m = __ballot(fresh), m36 = __ballot(fresh36), mk = __ballot(known);
    u32 base = 0, base36 = 0;
    if ((threadIdx.x & 63) == 0) {
        if (m) base = atomicAdd(&P.ctr[UP_NEW], (u32)__popcll(m));
        if (m36) base36 = atomicAdd(&P.ctr[UP_NEW36], (u32)__popcll(m36));
        if (mk) atomicAdd(&P.ctr[UP_UPDATED], (u32)__popcll(mk));
    }
    base = __shfl(base, 0, 64);
    base36 = __shfl(base36, 0, 64);
    if (fresh) {
        // the sparse hook: of the call's new 36-byte keys those at odd positions stay
        const bool leave = P.sparse && fresh36 && !((base36 + lanes_below(m36)) & 1u);
        P.fresh[base + lanes_below(m)] = i | (leave ? UP_LEAVE_OUT : 0u);   // base + ... < P.n
    }
}

// Pass 2, one lane per new key.
__global__ __launch_bounds__(AUX_TPB) void upsert_insert_kernel(const UpsertParams P, u32 n_new) {
    const u32 j = blockIdx.x * AUX_TPB + threadIdx.x;
    if (j >= n_new) return;
    const u32 e = P.fresh[j], i = e & ~UP_LEAVE_OUT;
    u32 r[SLOT_WORDS];
    load_record(P.rec, i, r);
    // the general table: the first free slot of the key's linear probe (load <= 1/2: there is one)
    const u32 h = key_hash(r + 2, r[0]);
    for (u32 pr = 0; pr <= P.table_mask; ++pr) {
        u32* sl = P.table + (u64)((h + pr) & P.table_mask) * SLOT_WORDS;
        if (sl[1] != EMPTY_SLOT) continue;
        if (atomicCAS(sl + 1, (u32)EMPTY_SLOT, r[1]) != EMPTY_SLOT) continue;   // another key took it
        sl[0] = r[0];
#pragma unroll
        for (u32 k = 0; k < KEY_WORDS; ++k) sl[2 + k] = r[2 + k];
        break;
    }
    if (r[0] != 36) return;
    if (e & UP_LEAVE_OUT) {
        atomicAdd(&P.ctr[UP_LEFT_OUT], 1u);
        return;
    }
    u64 at = 0;
    const u32 where = cuckoo_first_fit(P.ctable_mask, P.buckets != 0, P.cseed, r + 2, [&](u64 w) {
        if (P.ctable[w] != EMPTY_SLOT) return true;
        return atomicCAS(P.ctable + w, (u32)EMPTY_SLOT, r[1]) != EMPTY_SLOT;
    }, &at);
    if (where == CK_OUT) {
        P.homeless[atomicAdd(&P.ctr[UP_HOMELESS], 1u)] = i;   // < n_new <= P.n entries
        return;
    }
#pragma unroll
    for (u32 k = 0; k < CKEY_WORDS; ++k) P.ctable[at + k] = r[2 + k];
    atomicAdd(&P.ctr[where == CK_FIRST ? UP_FIRST : UP_SECOND], 1u);
}

// Pass 3, one thread: the keys that found both slots / buckets full, through the builders'
// eviction chains (ysb_admap.h).  A key still in hand when the kicks run out is in the
// general table only: the host then marks the table partial.
__global__ void upsert_evict_kernel(const UpsertParams P) {
    const u32 nh = min(P.ctr[UP_HOMELESS], P.n);
    u64 rng = P.rng;
    u32 moved = 0, out = 0;
    for (u32 q = 0; q < nh; ++q) {
        const u32* r = P.rec + (u64)P.homeless[q] * SLOT_WORDS;
        const u32 where = P.buckets ? cuckoo_place_buckets(P.ctable, P.ctable_mask, P.cseed, r + 2, r[1], &rng)
                                    : cuckoo_place_slots(P.ctable, P.ctable_mask, P.cseed, r + 2, r[1]);
        ++(where == CK_OUT ? out : moved);
    }
    P.ctr[UP_MOVED] = moved;
    P.ctr[UP_LEFT_OUT] += out;
}

// ysb_ad_map_lookup, one lane per key: the cuckoo table by the scan's two-slot or bucket
// probe, then the general table by its linear probe.
__global__ __launch_bounds__(AUX_TPB) void admap_lookup_kernel(const UpsertParams P, u32* out_campaign, u32* out_where) {
    const u32 i = blockIdx.x * AUX_TPB + threadIdx.x;
    if (i >= P.n) return;
    u32 r[SLOT_WORDS];
    load_record(P.rec, i, r);
    u32 campaign = EMPTY_SLOT, where = 0;
    if (r[0] == 36) {
        const u64 w = P.buckets ? cuckoo_find_buckets(P.ctable, P.ctable_mask, P.cseed, r + 2, &where)
                                : cuckoo_find_slots(P.ctable, P.ctable_mask, P.cseed, r + 2, &where);
        if (w != CK_NONE) campaign = P.ctable[w];
        else where = 0;
    }
    if (!where) {
        const i64 s = table_find(P.table, P.table_mask, r + 2, r[0]);
        if (s >= 0) {
            campaign = P.table[(u64)s * SLOT_WORDS + 1];
            where = 3;
        }
    }
    out_campaign[i] = campaign;
    out_where[i] = where;
}

static dim3 lane_grid(u32 n) { return dim3((n + AUX_TPB - 1) / AUX_TPB); }

void launch_upsert_classify(const UpsertParams& p, hipStream_t s) {
    if (p.n) hipLaunchKernelGGL(upsert_classify_kernel, lane_grid(p.n), dim3(AUX_TPB), 0, s, p);
}
void launch_upsert_insert(const UpsertParams& p, u32 n_new, hipStream_t s) {
    if (n_new) hipLaunchKernelGGL(upsert_insert_kernel, lane_grid(n_new), dim3(AUX_TPB), 0, s, p, n_new);
}
void launch_upsert_evict(const UpsertParams& p, hipStream_t s) {
    hipLaunchKernelGGL(upsert_evict_kernel, dim3(1), dim3(1), 0, s, p);
}
void launch_admap_lookup(const UpsertParams& p, u32* out_campaign, u32* out_where, hipStream_t s) {
    if (p.n) hipLaunchKernelGGL(admap_lookup_kernel, lane_grid(p.n), dim3(AUX_TPB), 0, s, p, out_campaign, out_where);
}

}  // namespace ysb
