// ysb_parked.hip -- the parked views' own kernels (the rules: ysb_parked.h): the distinct keys
// of the log, so that the host asks Redis once per ad and not once per view, and the resolve,
// which walks the log against the join tables as they are after the host's upsert.
//
// This is the jedis.get half of RedisAdCampaignCache.execute (RedisAdCampaignCache.java:23-35):
// the park sites (defer_kernel and colcount_kernel, in the scan unit) append the views of
// unknown ads; the host fetches the distinct keys, looks them up, puts what it found with
// ysb_ad_map_upsert, and the resolve then counts every parked view exactly as the scan would
// have, had the ad been known: joined, then Long.parseLong's stored outcome, then global_add
// (ysb_ring_add.h: the ring, the out-of-ring map, the out_of_ring tally).  An ad the lookup did
// not know either is the reference's null: a join miss.
//
// All of it is cold: it runs once per batch of misses, over records that no other kernel
// touches meanwhile (the park sites ran before on the same stream, the next launch runs after).
#include "ysb_kernels.h"
#include "ysb_admap.h"
#include "ysb_ring_add.h"

namespace ysb {

__device__ __forceinline__ u32 lanes_below(u64 mask) {
    return (u32)__popcll(mask & ((1ull << (threadIdx.x & 63)) - 1ull));
}

// One lane per record.  The slot table holds record indices; a lane that loses the
// compare-and-swap compares its key with the record the slot names -- complete since an
// earlier kernel -- so no lane ever reads a key another lane is writing.  The representatives
// are compacted with one atomic per wave.
__global__ __launch_bounds__(AUX_TPB) void parked_distinct_kernel(const ParkParams K, u32 n, u32* slots, u32 mask,
                                                                  u8* out_keys, u32* out_lens) {
    const u32 i = blockIdx.x * AUX_TPB + threadIdx.x;
    bool rep = false;
    if (i < n)
        rep = park_distinct_insert(K.log, i, mask, [&](u32 s, u32 v) { return atomicCAS(slots + s, (u32)EMPTY_SLOT, v); }) !=
              PARK_DUP;
    const u64 m = __ballot(rep);
    u32 base = 0;
    if ((threadIdx.x & 63) == 0 && m) base = atomicAdd(&K.ctr[PK_DISTINCT], (u32)__popcll(m));
    base = __shfl(base, 0, 64);
    if (rep) {
        const u32 j = base + lanes_below(m);   // < n <= cap: one representative per record at most
        const u32* r = K.log + (u64)i * PARK_WORDS;
        u32* o = reinterpret_cast<u32*>(out_keys + (u64)j * PARK_KEY_STRIDE);
#pragma unroll
        for (u32 k = 0; k < KEY_WORDS; ++k) o[k] = r[k];
        out_lens[j] = r[PARK_LEN];
    }
}

// Resolve, pass 1: the general table's probe (it holds every key: defer_kernel's table), and
// the smallest bucket among the records that will be counted, for a ring without a base.
__global__ __launch_bounds__(AUX_TPB) void parked_probe_kernel(const ScanParams P, const ParkParams K, u32 n, u32* camp) {
    const u32 i = blockIdx.x * AUX_TPB + threadIdx.x;
    i64 b = INT64_MAX;
    if (i < n) {
        const u32* r = K.log + (u64)i * PARK_WORDS;
        const i64 s = table_find(P.table, P.table_mask, r, r[PARK_LEN]);
        const u32 c = s < 0 ? (u32)EMPTY_SLOT : P.table[(u64)s * SLOT_WORDS + 1];
        camp[i] = c;
        i64 tv;
        const bool ok = park_time(r, &tv);
        if (park_resolve_class(c != EMPTY_SLOT, ok) == PARK_R_COUNT) b = div_trunc(tv, P.div);
    }
    if (P.ring[1] != 0) return;   // the base is set: nothing to find
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const i64 x = __shfl_xor(b, o, 64);
        b = x < b ? x : b;
    }
    if ((threadIdx.x & 63) == 0 && b != INT64_MAX) atomicMin(reinterpret_cast<long long*>(&K.ctr[PK_MINB]), (long long)b);
}

// Pass 2, one thread: a ring that no batch has based yet is based on what this resolve counts.
__global__ void parked_base_kernel(const ParkParams K, u32 ring_w, i64* ring) {
    const i64 b = *reinterpret_cast<const long long*>(&K.ctr[PK_MINB]);
    if (ring[1] == 0 && b != INT64_MAX) {
        ring[0] = park_ring_base(b, ring_w);
        ring[1] = 1;
    }
}

// Pass 3: every record becomes what the scan would have made of it.
__global__ __launch_bounds__(AUX_TPB) void parked_count_kernel(const ScanParams P, const ParkParams K, u32 n,
                                                               const u32* camp) {
    const u32 i = blockIdx.x * AUX_TPB + threadIdx.x;
    const i64 ring_lo = P.ring[0];
    const bool ring_set = P.ring[1] != 0;
    Tally tl{0, 0, 0, 0, 0, 0, 0, 0};
    if (i < n) {
        const u32* r = K.log + (u64)i * PARK_WORDS;
        const u32 c = camp[i];
        i64 tv;
        const bool ok = park_time(r, &tv);
        const u32 cls = park_resolve_class(c != EMPTY_SLOT, ok);
        if (cls == PARK_R_MISS) {
            tl.miss++;
        } else {
            tl.join++;
            if (cls == PARK_R_TIME_ERR) {
                tl.terr++;
            } else {
                global_add(P, ring_lo, ring_set, c, div_trunc(tv, P.div), 1u, tl);
                *P.pend_dirty = 1u;   // the u64 ring holds pending counts now (the exchange reads it)
            }
        }
    }
    u32 sums[4] = {tl.join, tl.miss, tl.terr, tl.oor};
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sums[k] += __shfl_xor(sums[k], o, 64);
    if ((threadIdx.x & 63) == 0) {
        const u32 st[4] = {ST_JOINED, ST_MISSES, ST_TIME_ERR, ST_OUT_OF_RING};
        const u32 pk[4] = {PK_JOINED, PK_MISSED, PK_TIME_ERR, PK_COUNT_};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!sums[k]) continue;
            atomicAdd(&P.stats[st[k]], (unsigned long long)sums[k]);
            if (pk[k] != PK_COUNT_) atomicAdd(&K.ctr[pk[k]], sums[k]);
        }
    }
}

static dim3 lane_grid(u32 n) { return dim3((n + AUX_TPB - 1) / AUX_TPB); }

void launch_parked_distinct(const ParkParams& k, u32 n, u32* slots, u32 mask, u8* out_keys, u32* out_lens,
                            hipStream_t s) {
    if (n) hipLaunchKernelGGL(parked_distinct_kernel, lane_grid(n), dim3(AUX_TPB), 0, s, k, n, slots, mask, out_keys, out_lens);
}

void launch_parked_resolve(const ScanParams& sp, const ParkParams& k, u32 n, u32* camp, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(parked_probe_kernel, lane_grid(n), dim3(AUX_TPB), 0, s, sp, k, n, camp);
    hipLaunchKernelGGL(parked_base_kernel, dim3(1), dim3(1), 0, s, k, sp.ring_w, const_cast<i64*>(sp.ring));
    hipLaunchKernelGGL(parked_count_kernel, lane_grid(n), dim3(AUX_TPB), 0, s, sp, k, n, camp);
}

}  // namespace ysb
