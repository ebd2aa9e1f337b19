// ysb_ring_add.h -- one view (or v of them) counted into its (campaign, bucket) cell: the
// window ring when the bucket is live, else the exact out-of-ring map or its fallback list
// (global_add); in front of the ring, a workgroup's LDS window of counters (LdsWindow: the
// JSON / .tbl scan, the columnar count and the Arrow count step it the same way); and the
// ring's automatic base from a batch's first rows (commit_ring_base).  The window's and the
// base's rules are ysb_window.h's.  Device code shared by the scan unit (ysb_scan.hip and the
// headers it includes) and the parked views' resolve (ysb_parked.hip).
#pragma once
#include "ysb_kernels.h"
#include "ysb_window.h"

// diagnostic build (make variant; never used for results): LDS window counters never flushed
#ifndef YSB_DIAG_NO_FLUSH
#define YSB_DIAG_NO_FLUSH 0
#endif

namespace ysb {

// Per-thread tallies of a kernel (summed per wave into the stats array at its end).
struct Tally { u32 ev, view, join, miss, perr, terr, oor, frn; };

// Out-of-ring cell (c, b) += v in the device hash map; false if the key cannot express
// the bucket or 64 probes find no slot (the caller then appends to the fallback list).
__device__ __forceinline__ bool side_add(const ScanParams& P, u32 c, i64 b, u32 v) {
    const i64 half = (i64)1 << (63 - P.side_cbits);
    if (b < -half || b >= half) return false;
    const unsigned long long key = ((unsigned long long)(b + half) << P.side_cbits) | c;
    const u32 h = (u32)(mix64(key) >> 32);
    for (u32 i = 0; i < 64u && i <= P.side_mask; ++i) {
        SideSlot* sl = &P.side[(h + i) & P.side_mask];
        const unsigned long long k = atomicCAS(&sl->key, SIDE_EMPTY, key);
        if (k == SIDE_EMPTY || k == key) {
            if (k == SIDE_EMPTY) atomicAdd(P.side_used, 1u);
            atomicAdd(&sl->count, (unsigned long long)v);
            return true;
        }
    }
    return false;
}

// Adds v views to (campaign, bucket): the ring cell if the bucket is live, else the
// exact side map (or its fallback list).
__device__ __forceinline__ void global_add(const ScanParams& P, i64 ring_lo, bool ring_set,
                                           u32 c, i64 b, u32 v, Tally& t) {
    if (ring_set) {
        const i64 rel = b - ring_lo;
        if (rel >= 0 && rel < (i64)P.ring_w) {
            atomicAdd(&P.counts[(u64)c * P.ring_w + (u64)(b & (i64)(P.ring_w - 1))], (unsigned long long)v);
            return;
        }
    }
    t.oor += v;
    if (side_add(P, c, b, v)) return;
    const u32 idx = atomicAdd(P.ovf_count, 1u);
    if (idx < P.ovf_cap) {
        OvfEntry en;
        en.campaign = c; en.count = v; en.bucket = b;
        P.ovf[idx] = en;
    } else {
        atomicAdd(&P.stats[ST_OVF_DROPPED], (unsigned long long)v);
    }
}

// LDS window counters: every non-zero cell of the window at lbase to the ring.
__device__ __forceinline__ void flush_window(const ScanParams& P, u32* lcnt, u32 ncells, u32 WL, i64 lbase,
                                             i64 ring_lo, bool ring_set, Tally& tl) {
    for (u32 i = threadIdx.x; i < ncells; i += SCAN_TPB) {
        const u32 v = lcnt[i];
        if (v) {
            lcnt[i] = 0;
            if constexpr (!YSB_DIAG_NO_FLUSH)
                global_add(P, ring_lo, ring_set, i >> P.lds_wl_log2, lbase + (i64)(i & (WL - 1)), v, tl);
        }
    }
}

// A workgroup's LDS window over LDS of the caller's: lcnt, n_campaigns << lds_wl_log2 cells, and
// req, the two move requests (the largest bucket that fell ahead of the window; INT64_MIN:
// none), double-buffered by tile parity so that a tile's requests never meet the clearing of
// the previous tile's.  base / set / tseq are identical in every thread: each applies the same
// requests.  WL 0: the context has no window and count() counts into the ring.  Per tile:
// par = before_barrier(), the tile's barrier, after_barrier(par), count(par) per joined view, a
// barrier.
struct LdsWindow {
    u32* lcnt;
    i64* req;
    u32 WL, ncells;
    i64 ring_lo;
    bool ring_set;
    i64 base = 0;
    bool set = false;
    u32 tseq = 0;   // tiles stepped so far

    __device__ __forceinline__ LdsWindow(const ScanParams& P, u32* lcnt_, i64* req_)
        : lcnt(lcnt_), req(req_), WL(P.lds_wl), ncells(WL ? P.n_campaigns * WL : 0u), ring_lo(P.ring[0]),
          ring_set(P.ring[1] != 0) {}

    // cells zero, no request (requests false: the caller keeps something else in req's place)
    __device__ __forceinline__ void init(bool requests = true) {
        for (u32 i = threadIdx.x; i < ncells; i += SCAN_TPB) lcnt[i] = 0;
        if (requests && (int)threadIdx.x < 2) req[threadIdx.x] = INT64_MIN;
    }
    __device__ __forceinline__ void flush(const ScanParams& P, Tally& tl) {
        flush_window(P, lcnt, ncells, WL, base, ring_lo, ring_set, tl);
    }
    // The previous tile asked to move the window: flush it (its counts are all in, that tile's
    // end barrier saw to that) and re-centre, before this tile counts.
    // -> the tile's parity: its own requests go to req[par]
    __device__ __forceinline__ int before_barrier(const ScanParams& P, Tally& tl) {
        const int par = (int)(tseq++ & 1);
        if (WL) {
            const i64 r = req[par ^ 1];
            if (r != INT64_MIN) {
                if (set) flush(P, tl);
                base = window_base_for(r, WL);
                set = true;
            }
        }
        return par;
    }
    // every thread has read the previous tile's request
    __device__ __forceinline__ void after_barrier(int par) {
        if (threadIdx.x == 0) req[par ^ 1] = INT64_MIN;
    }
    // one joined view of a context with a window (WL != 0)
    __device__ __forceinline__ void add(const ScanParams& P, int par, u32 ci, i64 bucket, Tally& tl) {
        const i64 rel = bucket - base;
        if (window_holds(set, rel, WL)) {
            atomicAdd(&lcnt[(ci << P.lds_wl_log2) + (u32)rel], 1u);
        } else {
            global_add(P, ring_lo, ring_set, ci, bucket, 1u, tl);
            if (window_asks_move(set, rel, WL)) atomicMax(reinterpret_cast<long long*>(&req[par]), (long long)bucket);
        }
    }
    // ... of any context
    __device__ __forceinline__ void count(const ScanParams& P, int par, u32 ci, i64 bucket, Tally& tl) {
        if (WL) add(P, par, ci, bucket, tl);
        else global_add(P, ring_lo, ring_set, ci, bucket, 1u, tl);
    }
    // behind the last tile
    __device__ __forceinline__ void finish(const ScanParams& P, Tally& tl) {
        if (WL && set) flush(P, tl);
    }
};

// The ring's automatic base, one workgroup of AUX_TPB threads: b is the thread's bucket
// (INT64_MAX: its row counts nothing); the smallest one fixes the ring (ring_base_for).
__device__ __forceinline__ void commit_ring_base(i64 b, i64* ring, u32 ring_w) {
    __shared__ i64 scratch[AUX_TPB / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const i64 x = __shfl_xor(b, o, 64);
        b = x < b ? x : b;
    }
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
        i64 r = scratch[0];
        for (int w = 1; w < AUX_TPB / 64; ++w) r = scratch[w] < r ? scratch[w] : r;
        if (r != INT64_MAX) {
            ring[0] = ring_base_for(r, ring_w);
            ring[1] = 1;
        }
    }
}

}  // namespace ysb
