// ysb_count_columns.h -- Kernel 5: views counted straight from a batch in the fork's columnar
// hand-off layout (WindowedArrowFormatBolter, flink-benchmarks/.../
// AdvertisingTopologyNative.java:278-356; include/ysb_hip.h ysb_columns_layout): the consumer
// of what Kernel 4 (ysb_scan_columns.h) and the fork's bolter produce.  The filter -> join ->
// window-count chain (:115-119) on column contents: no parser, no deferred lines.
// Part of the scan kernel's translation unit: included at the end of ysb_scan.hip, whose
// code it shares rather than repeats -- cuckoo_slots36, bucket_find, probe, key_hash_dev,
// count_miss, park_append, the LDS window (LdsWindow, ysb_ring_add.h), flush_tally and div_trunc.
//
// It reads three of the seven columns: ad_id (36 B), event_type (4 B), event_time (8 B),
// 48 B per row, and with YSB_COL_VALIDITY one bitmap word per 64 rows.  The layout cuts
// event_type to four bytes, so the filter is "the four bytes equal `view`": a value such as
// `viewer` is a view here and not on the JSON path (a property of the fork's layout).
//
// Shape: one-wave workgroups, tiles of 64 rows, lane i takes row i.  A tile is contiguous in
// every column (2304 / 256 / 512 bytes, at least 16-byte aligned: column starts are pages,
// tiles start at multiples of 64 rows, the batch itself is 16-byte aligned), so the ad_id
// block is loaded with 16-byte coalesced loads two tiles ahead and staged into LDS at its own
// row stride of 9 dwords (odd: the lanes' reads of one key word fall in distinct banks), from
// where the view lanes read their nine key words.  Every load is a bounds-checked buffer load
// over the tile's rows only: a batch's last, partial tile loads no byte of a row >= n_rows.
#pragma once

namespace ysb {

constexpr int CC_KEY_DW = TILE_LINES * (int)CKEY_WORDS;     // 576 dwords: a tile's ad_id block
constexpr int CC_KEY_CHUNKS = CC_KEY_DW / 4;                // 144 16-byte chunks
constexpr int CC_CPT = (CC_KEY_CHUNKS + SCAN_TPB - 1) / SCAN_TPB;   // 3 per lane
constexpr int CC_LDS = CC_KEY_DW * 4 + LCNT_CAP * 4 + 16;   // keys | window counters | rebase requests
// Two waves per SIMD, each with two tiles in flight ahead of the one it probes.  Measured on
// 10M rows (profiles/AB_LOG.md "Columnar count"): 16 workgroups per CU with one tile ahead
// 0.261 ms, 24 per CU 0.312 (every workgroup ends in same-address tally and window-counter
// atomics: more workgroups, a longer tail), 8 per CU 0.231, 8 per CU with two tiles ahead 0.220,
// 4 per CU with two / four tiles ahead 0.295 / 0.269.
#ifndef YSB_COLCOUNT_WG_PER_CU
#define YSB_COLCOUNT_WG_PER_CU 8
#endif
constexpr int CC_WG_PER_CU = YSB_COLCOUNT_WG_PER_CU;
#ifndef YSB_COLCOUNT_PF
#define YSB_COLCOUNT_PF 2
#endif
constexpr int CC_PF = YSB_COLCOUNT_PF;                      // tiles in flight ahead of the one being probed
static_assert(CC_WG_PER_CU % 4 == 0 && CC_PF >= 1, "whole waves per SIMD");
static_assert((CC_LDS + 1279) / 1280 * 1280 * CC_WG_PER_CU <= 163840, "the workgroups fit one CU's LDS");
static_assert(TILE_LINES == 64 && SCAN_TPB == 64, "lane i takes row i; a tile's validity word is one u64");

// A tile's blocks on their way HBM -> registers (issued CC_PF tiles ahead).
struct ColTile {
    uint4 k[CC_CPT];    // the ad_id block's whole 16-byte chunks tid, tid + 64, tid + 128
    u32 ktail;          // dword tid past the whole chunks (a partial tile: 36 * count is no multiple of 16)
    u32 et;             // row tid's event_type
    u32 t0, t1;         // row tid's event_time as stored
    unsigned long long vw;   // the tile's validity word (YSB_COL_VALIDITY)
    u32 count;          // rows of the tile
};

// Tile t's loads.  Bounds-checked buffer loads over rows [0, count) of each block: lanes
// past them receive zeros and touch no memory.  t >= n_tiles: nothing is read.
__device__ __forceinline__ void cc_issue(const ColCountParams& C, u64 t, int tid, ColTile& o) {
    const bool live = t < C.n_tiles;
    const u64 first = live ? t * (u64)TILE_LINES : 0;
    const u64 rem = C.n_rows - first;
    const u32 count = !live ? 0u : rem < (u64)TILE_LINES ? (u32)rem : (u32)TILE_LINES;
    o.count = count;
    const u32 kbytes = count * 36u;
    const u32 whole = kbytes & ~15u;
    // (a 16-byte access that straddles num_records reads as zeros: whole chunks by b128,
    // the up to three dwords behind them by b32)
    const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<u8*>(C.cols + C.start[2] + first * 36u), 0, (int)whole, 0x00020000);
    const __amdgpu_buffer_rsrc_t rkt = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<u8*>(C.cols + C.start[2] + first * 36u), 0, (int)kbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t re = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<u8*>(C.cols + C.start[4] + first * 4u), 0, (int)(count * 4u), 0x00020000);
    const __amdgpu_buffer_rsrc_t rt = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<u8*>(C.cols + C.start[5] + first * 8u), 0, (int)(count * 8u), 0x00020000);
    o.et = __builtin_amdgcn_raw_buffer_load_b32(re, 4 * tid, 0, AUX_NT);
    o.vw = ~0ull;
    if (C.validity && live)   // word t < ceil(n_rows / 64); one address for the wave
        o.vw = reinterpret_cast<const unsigned long long*>(C.cols + C.start[7])[t];
#pragma unroll
    for (int j = 0; j < CC_CPT; ++j) {
        const auto v = __builtin_amdgcn_raw_buffer_load_b128(rk, 16 * (j * SCAN_TPB + tid), 0, AUX_NT);
        o.k[j] = make_uint4(v[0], v[1], v[2], v[3]);
    }
    o.ktail = __builtin_amdgcn_raw_buffer_load_b32(rkt, (int)whole + 4 * tid, 0, AUX_NT);
    const auto tv = __builtin_amdgcn_raw_buffer_load_b64(rt, 8 * tid, 0, AUX_NT);
    o.t0 = tv[0];
    o.t1 = tv[1];
}

// The 36-byte key's cuckoo probe (RedisJoinBolt, :461-474), split so that the caller can issue
// other loads between the probe's and their use.  Cache-resident slots: both at once.  HBM
// bucket table (SERIAL): the first bucket, the second only after a miss in a full first one.
template <bool SERIAL>
struct ColProbe {
    uint4 q[SERIAL ? (int)CB_Q : 6];
    u32 ib;
};

template <bool SERIAL>
__device__ __forceinline__ void cc_probe_issue(const ScanParams& P, const u32 (&kw)[CKEY_WORDS], ColProbe<SERIAL>& pr) {
    const uint4* ct4 = reinterpret_cast<const uint4*>(P.ctable);
    u32 ia, ib;
    cuckoo_slots36(kw, P.cseed, P.ctable_mask, &ia, &ib);
    pr.ib = ib;
    if constexpr (SERIAL) {
#pragma unroll
        for (int j = 0; j < (int)CB_Q; ++j) pr.q[j] = ct4[CB_Q * (u64)ia + j];
    } else {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            pr.q[j] = ct4[CSLOT_Q * (u64)ia + j];
            pr.q[3 + j] = ct4[CSLOT_Q * (u64)ib + j];
        }
    }
}

// The key's campaign, or EMPTY_SLOT.  A partial cuckoo table (YSB_F_SPARSE_FAST_JOIN, a failed
// placement, a sharded table) sends its misses to the general table in the same lane: the key
// is in registers, so there is no deferred list.  kw14: the key zero-padded to KEY_WORDS.
template <bool SERIAL>
__device__ __forceinline__ u32 cc_probe_finish(const ScanParams& P, const u32 (&kw14)[KEY_WORDS], ColProbe<SERIAL>& pr) {
    const u32* k = kw14;
    u32 ci;
    if constexpr (SERIAL) {
        const uint4* ct4 = reinterpret_cast<const uint4*>(P.ctable);
        bool full;
        ci = bucket_find(pr.q, k, full);
        if (ci == EMPTY_SLOT && full) {
#pragma unroll
            for (int j = 0; j < (int)CB_Q; ++j) pr.q[j] = ct4[CB_Q * (u64)pr.ib + j];
            ci = bucket_find(pr.q, k, full);
        }
    } else {
        const uint4 *a = pr.q, *b = pr.q + 3;
        const u32 da = (a[0].x ^ k[0]) | (a[0].y ^ k[1]) | (a[0].z ^ k[2]) | (a[0].w ^ k[3]) | (a[1].x ^ k[4]) |
                       (a[1].y ^ k[5]) | (a[1].z ^ k[6]) | (a[1].w ^ k[7]) | (a[2].x ^ k[8]);
        const u32 db = (b[0].x ^ k[0]) | (b[0].y ^ k[1]) | (b[0].z ^ k[2]) | (b[0].w ^ k[3]) | (b[1].x ^ k[4]) |
                       (b[1].y ^ k[5]) | (b[1].z ^ k[6]) | (b[1].w ^ k[7]) | (b[2].x ^ k[8]);
        ci = (da == 0u && a[2].y != EMPTY_SLOT) ? a[2].y : (db == 0u ? b[2].y : EMPTY_SLOT);
    }
    if (ci == EMPTY_SLOT && P.ctable_partial) {
        const int c = probe(P.table, P.table_mask, kw14, 36u);
        if (c >= 0) ci = (u32)c;
    }
    return ci;
}

// event_time as stored -> int64: little-endian, or MappedByteBuffer.putLong's big-endian
__device__ __forceinline__ i64 cc_time(u32 t0, u32 t1, u32 java_order) {
    if (java_order) {
        const u32 a = __builtin_bswap32(t1);
        t1 = __builtin_bswap32(t0);
        t0 = a;
    }
    return (i64)(((u64)t1 << 32) | (u64)t0);
}

// A view's join result, counted -- the columnar and the Arrow count's common tail.  The lane
// brings its campaign ci (EMPTY_SLOT: in no table), its key (keyed false: no possible map key)
// and Long.parseLong(event_time)'s outcome (tok, tv).  PARK (parking enabled, ysb_parked.h): a
// view whose ad is in no table is handed to the tile's park site in pl -- the key and the time
// are in registers -- instead of being counted as a join miss; the kernel calls park_append
// behind this with every lane of the wave (a view's lane or not).
template <bool PARK>
__device__ __forceinline__ void cc_count_view(const ScanParams& P, LdsWindow& win, int par, u32 ci, bool keyed,
                                              const u32 (&kw)[KEY_WORDS], u32 klen, bool tok, i64 tv, Tally& tl, ParkLane& pl) {
    if (PARK && ci == EMPTY_SLOT && park_wanted(keyed, keyed ? key_hash_dev(kw, klen) : 0u, P.shard_rank, P.shard_n)) {
        pl.want = true;
        pl.tok = tok;
#pragma unroll
        for (int k = 0; k < (int)KEY_WORDS; ++k) pl.kw[k] = kw[k];
        pl.klen = klen;
        pl.tv = tv;
    } else if (ci == EMPTY_SLOT) {
        count_miss(P, kw, klen, keyed, tl);   // a join miss, or a key of another shard
    } else {
        tl.join++;
        if (!tok) tl.terr++;   // CampaignProcessorCommon :58: the time is parsed after the join
        else win.count(P, par, ci, div_trunc(tv, P.div), tl);
    }
}

// One launch of kernel<SERIAL, PARK>: launch(std::bool_constant<SERIAL>, std::bool_constant<PARK>).
template <class Launch>
static void launch_serial_park(bool serial, bool park, Launch&& launch) {
    if (park) {
        if (serial) launch(std::true_type{}, std::true_type{});
        else launch(std::false_type{}, std::true_type{});
    } else {
        if (serial) launch(std::true_type{}, std::false_type{});
        else launch(std::false_type{}, std::false_type{});
    }
}
// whole rounds of resident workgroups over the tiles (each walks tiles blockIdx.x + k * grid)
static dim3 count_grid(u64 n_tiles, u64 resident) { return dim3((u32)(n_tiles < resident ? n_tiles : resident)); }

template <bool SERIAL, bool PARK>
__global__ __launch_bounds__(SCAN_TPB) __attribute__((amdgpu_waves_per_eu(CC_WG_PER_CU / 4)))
void colcount_kernel(const ColCountParams C, const ParkParams K) {
    const ScanParams& P = C.sp;
    __shared__ __attribute__((aligned(16))) u32 keys[CC_KEY_DW];
    __shared__ u32 lcnt[LCNT_CAP];
    __shared__ i64 req64[2];   // the LDS window's move requests
    const int tid = threadIdx.x;
    u64 t = blockIdx.x;
    if (t >= C.n_tiles) return;

    LdsWindow win(P, lcnt, req64);
    win.init();
    Tally tl{0, 0, 0, 0, 0, 0, 0, 0};

    // One tile: its blocks arrive in pre (issued CC_PF tiles ago); the tile CC_PF ahead is issued
    // into the same registers once these are in LDS.
    auto tile_step = [&](u64 t, ColTile& pre) {
        // ---- registers -> LDS: the ad_id block (chunks past the rows hold zeros) ----------
        const u32 whole_dw = (pre.count * 9u) & ~3u;
#pragma unroll
        for (int j = 0; j < CC_CPT; ++j) {
            const int k = j * SCAN_TPB + tid;
            if (j * SCAN_TPB + SCAN_TPB <= CC_KEY_CHUNKS || k < CC_KEY_CHUNKS) reinterpret_cast<uint4*>(keys)[k] = pre.k[j];
        }
        if ((u32)tid < pre.count * 9u - whole_dw) keys[whole_dw + tid] = pre.ktail;   // (after the zero chunk above)
        const u32 count = pre.count, et = pre.et, t0 = pre.t0, t1 = pre.t1;
        const unsigned long long vw = pre.vw;
        const int par = win.before_barrier(P, tl);
        __syncthreads();
        win.after_barrier(par);
        // ---- filter (EventFilterBolt on the cut value), the key, its probe -----------------
        const bool active = (u32)tid < count;
        const bool valid = active && ((vw >> tid) & 1ull);
        const bool view = valid && et == VIEW_W;
        tl.ev += active ? 1u : 0u;
        tl.perr += (active && !valid) ? 1u : 0u;   // the row the reference would have thrown on
        tl.view += view ? 1u : 0u;
        u32 kw[KEY_WORDS];
#pragma unroll
        for (int k = 0; k < (int)KEY_WORDS; ++k) kw[k] = 0u;
        ColProbe<SERIAL> pr;
#pragma unroll
        for (int j = 0; j < (int)(sizeof(pr.q) / sizeof(pr.q[0])); ++j) pr.q[j] = make_uint4(0, 0, 0, 0);
        pr.ib = 0;
        if (view) {
            u32 k9[CKEY_WORDS];
#pragma unroll
            for (int k = 0; k < (int)CKEY_WORDS; ++k) k9[k] = keys[tid * (int)CKEY_WORDS + k];
#pragma unroll
            for (int k = 0; k < (int)CKEY_WORDS; ++k) kw[k] = k9[k];
            cc_probe_issue<SERIAL>(P, k9, pr);
        }
        // ---- the next tile's blocks land while this one is probed and counted --------------
        cc_issue(C, t + (u64)CC_PF * gridDim.x, tid, pre);
        // ---- join result, bucket, count ------------------------------------------------------
        ParkLane pl;
        pl.want = false;
        if (view) {
            const u32 ci = cc_probe_finish<SERIAL>(P, kw, pr);
            // (a column time is an int64 already: no parse to fail)
            cc_count_view<PARK>(P, win, par, ci, true, kw, 36u, true, cc_time(t0, t1, C.java_order), tl, pl);
        }
        if constexpr (PARK) park_append(K, pl, tl);
        __syncthreads();   // the tile's keys are read and its counts are in before the next one
    };
    ColTile pre[CC_PF];
#pragma unroll
    for (int k = 0; k < CC_PF; ++k) cc_issue(C, t + (u64)k * gridDim.x, tid, pre[k]);
    for (; t < C.n_tiles; t += (u64)CC_PF * gridDim.x) {
#pragma unroll
        for (int k = 0; k < CC_PF; ++k) {
            const u64 tk = t + (u64)k * gridDim.x;
            if (tk >= C.n_tiles) break;
            tile_step(tk, pre[k]);
        }
    }
    win.finish(P, tl);
    flush_tally(P, tl, tid);
}

// Ring auto-base, the column form of ring_autobase_kernel: the smallest bucket among the joined
// views of rows [0, min(n_rows, 256)) fixes the ring at that bucket - W / 8.
template <bool SERIAL>
__global__ __launch_bounds__(AUX_TPB) void colcount_autobase_kernel(const ColCountParams C, i64* ring) {
    const ScanParams& P = C.sp;
    if (ring[1] != 0) return;
    const int tid = threadIdx.x;
    i64 b = INT64_MAX;
    if ((u64)tid < C.n_rows) {
        bool valid = true;
        if (C.validity)
            valid = (reinterpret_cast<const unsigned long long*>(C.cols + C.start[7])[tid >> 6] >> (tid & 63)) & 1ull;
        if (valid && reinterpret_cast<const u32*>(C.cols + C.start[4])[tid] == VIEW_W) {
            u32 kw[KEY_WORDS], k9[CKEY_WORDS];
#pragma unroll
            for (int k = 0; k < (int)KEY_WORDS; ++k) kw[k] = 0u;
#pragma unroll
            for (int k = 0; k < (int)CKEY_WORDS; ++k)
                kw[k] = k9[k] = reinterpret_cast<const u32*>(C.cols + C.start[2])[tid * (int)CKEY_WORDS + k];
            ColProbe<SERIAL> pr;
            cc_probe_issue<SERIAL>(P, k9, pr);
            if (cc_probe_finish<SERIAL>(P, kw, pr) != EMPTY_SLOT) {
                const u32* tw = reinterpret_cast<const u32*>(C.cols + C.start[5]) + 2 * tid;
                b = div_trunc(cc_time(tw[0], tw[1], C.java_order), P.div);
            }
        }
    }
    commit_ring_base(b, ring, P.ring_w);
}

// The out-of-ring map's fill level after the launch, for the host (what defer_kernel stores
// after a scan).
__global__ void colcount_used_kernel(const u32* side_used, u32* used_out) { *used_out = *side_used; }

void launch_colcount(const ColCountParams& p, int cus, hipStream_t s, const ParkParams* park) {
    if (p.n_rows == 0) return;
    const dim3 g = count_grid(p.n_tiles, (u64)(cus > 0 ? cus : 1) * (u64)CC_WG_PER_CU);
    launch_serial_park(p.sp.probe_serial, park, [&](auto serial, auto parked) {
        hipLaunchKernelGGL((colcount_kernel<decltype(serial)::value, decltype(parked)::value>), g, dim3(SCAN_TPB), 0, s, p,
                           park ? *park : ParkParams{});
    });
}

void launch_used_level(const ScanParams& sp, hipStream_t s) {
    if (!sp.used_out) return;
    hipLaunchKernelGGL(colcount_used_kernel, dim3(1), dim3(1), 0, s, sp.side_used, sp.used_out);
}

void launch_colcount_autobase(const ColCountParams& p, hipStream_t s) {
    if (p.n_rows == 0) return;
    const dim3 g(1), b(AUX_TPB);
    i64* ring = const_cast<i64*>(p.sp.ring);
    if (p.sp.probe_serial) hipLaunchKernelGGL(colcount_autobase_kernel<true>, g, b, 0, s, p, ring);
    else hipLaunchKernelGGL(colcount_autobase_kernel<false>, g, b, 0, s, p, ring);
}

}  // namespace ysb
