// ysb_scan_join.h -- Kernel 7: the join's output as ordered columns.  RedisJoinBolt.flatMap
// (flink-benchmarks/.../AdvertisingTopologyNative.java:460-474) emits a Tuple3(campaign_id,
// ad_id, event_time) for every view whose ad is in the map; these kernels give that stream for
// one device batch of lines or .tbl rows, in stream order, as columns in HBM: campaign index,
// source row, parsed event_time, whether it parsed, and with YSB_JOIN_KEYS the decoded ad_id.
// The layout, the scratch format and the rank / prefix / clip plan are ysb_join.h's (no HIP; its
// host model runs the same three steps on the CPU).
// Part of the scan kernel's translation unit: included at the end of ysb_scan.hip, whose code it
// shares rather than repeats -- the byte sources, the tile loader (TileInfo, issue_tile_loads,
// Kernel 4's col_tile_info and geometry), the vocabulary / canonical / .tbl stages, parse_line,
// tbl_split, line_sane, span_is_view, span_key, span_long, the probes (probe, Kernel 5's
// cc_probe_issue / cc_probe_finish), count_miss and flush_tally.
//
// Output order must not depend on scheduling and no workgroup waits for another -- no
// look-back, no spinning, no grid barrier -- so there are three launches:
//   a. join_kernel     one-wave workgroups, lane i takes line i of a 64-line tile staged in LDS
//                      (the next tile's loads in flight meanwhile).  The tile's joined mask is
//                      one ballot, a lane's rank the popcount of the mask below it; the tile's
//                      joined rows are assembled in LDS in rank order and written with 16-byte
//                      stores to the tile's block of the scratch area, its count to tile_count.
//   b. join_prefix_kernel  the exclusive prefix over tile_count (each workgroup sums what lies in
//                      front of its segment itself).
//   c. join_pack_kernel    tile t's rows to rows [prefix[t], prefix[t] + count) of every column,
//                      clipped at cap_rows: 16-byte stores over the aligned middle of each run,
//                      narrower ones only at its ragged ends.
#pragma once
#include "ysb_join.h"

namespace ysb {

static_assert(JOIN_TILE == TILE_LINES && TILE_LINES == SCAN_TPB, "lane i takes line i; the joined mask is one ballot");
static_assert(JOIN_KEY_STRIDE == PARK_KEY_STRIDE && JOIN_KEY_STRIDE == 4 * KEY_WORDS, "the key column is the tables' key form");

template <bool TBL>
struct JoinGeom {
    static constexpr int LDS = ColGeom<TBL>::CAP + 64 + (int)JOIN_TILE_BYTES_KEYS;   // tile | slack | the tile's block
    static constexpr int FIT = 163840 / ((LDS + 1279) / 1280 * 1280);
    static constexpr int WG_PER_CU = FIT < 8 ? FIT : 8;   // two waves per SIMD at most (amdgpu_waves_per_eu)
    // (the grid: one round of resident workgroups, each walking tiles blockIdx.x + k * grid; two
    // rounds were 4 % (JSON) to 9 % (.tbl) slower, profiles/AB_LOG.md "Kernel 7")
};

// What a lane knows of its line after filter, join and time parse.
struct JoinLane {
    bool joined, tok;
    u32 campaign, klen;
    i64 tv;
    u32 kw[KEY_WORDS];
};

// A parsed line's filter, join and time (the bolts after DeserializeBolt; finish_line's order,
// with the joined row kept instead of counted): the view's key through the general table, which
// holds every key of any length; a joined view whose time does not parse is still a row.
template <class S>
__device__ __forceinline__ void join_finish(const S& src, const Span& ad, const Span& et, const Span& tm,
                                            const ScanParams& P, Tally& t, JoinLane& o) {
    if (!span_is_view(src, et)) return;                      // EventFilterBolt
    t.view++;
    int c = -1;
    const bool keyed = span_key(src, ad, o.kw, o.klen);
    if (keyed) c = probe(P.table, P.table_mask, o.kw, o.klen);   // RedisJoinBolt
    if (c < 0) { count_miss(P, o.kw, o.klen, keyed, t); return; }
    t.join++;
    o.joined = true;
    o.campaign = (u32)c;
    o.tok = span_long(src, tm, o.tv);                        // CampaignProcessorCommon :58
    if (!o.tok) { t.terr++; o.tv = 0; }
}

// A line in any layout (process_line's steps).
template <class S>
__device__ __noinline__ void join_json_general(const S& src, int s, int e, const ScanParams& P, Tally& t, JoinLane& o) {
    KeepCount k;
    if (!parse_line(src, s, e, P.require_mask, k)) { t.perr++; return; }
    join_finish(src, k.ad, k.et, k.tm, P, t, o);
}

// Any .tbl row (process_tbl_line's steps).
template <class S>
__device__ __noinline__ void join_tbl_general(const S& src, int s, int e, const ScanParams& P, Tally& t, JoinLane& o) {
    int p[6];
    if (tbl_split(src, s, e, p) < 5) { t.perr++; return; }
    bool tail = p[5] > p[4] + 1;   // items[5] exists iff something other than '|' follows the fifth '|'
    for (int q = p[5]; !tail && q < e; ++q) tail = src.b(q) != '|';
    if (!tail) { t.perr++; return; }
    join_finish(src, Span{p[1] + 1, p[2], 0}, Span{p[3] + 1, p[4], 0}, Span{p[4] + 1, p[5], 0}, P, t, o);
}

// (two waves per SIMD, as Kernel 4: the general parser no generator line calls must not set
// the fast tier's register budget)
template <bool TBL, bool SERIAL>
__global__ __launch_bounds__(SCAN_TPB) __attribute__((amdgpu_waves_per_eu(2))) void join_kernel(const JoinParams J) {
    using G = ColGeom<TBL>;
    constexpr int CPT = G::CPT;
    __shared__ __attribute__((aligned(16))) u32 tile32[G::TILE_WORDS];
    __shared__ __attribute__((aligned(16))) u32 st[JOIN_TILE_BYTES_KEYS / 4];
    const ScanParams& P = J.sp;
    const ColParams& B = J.b;
    const int tid = threadIdx.x;
    const LdsSrc lsrc{tile32};
    u8* const st8 = reinterpret_cast<u8*>(st);
    Tally tl{0, 0, 0, 0, 0, 0, 0, 0};
    u32 n_fast = 0;
    if (tid < 16) tile32[G::CAP / 4 + tid] = 0u;   // the slack past a full tile

    uint4 pre[CPT];
    u32 pre_off = 0, pre_end = 0;
    u64 t = blockIdx.x;
    if (t >= B.n_tiles) return;
    const u32 tile_bytes = J.keys ? (u32)JOIN_TILE_BYTES_KEYS : (u32)JOIN_TILE_BYTES;
    TileInfo cur = col_tile_info<G::CAP>(B, t);
    issue_tile_loads(B.bytes, B.off, B.n, (u32)tid, cur, pre, pre_off, pre_end);
    for (; t < B.n_tiles; t += gridDim.x) {
        // ---- registers -> LDS (chunks past the staged bytes hold zeros) ----------------
#pragma unroll
        for (int j = 0; j < CPT; ++j) {
            const u32 k = (u32)(j * SCAN_TPB + tid);
            if (j * SCAN_TPB + SCAN_TPB <= G::CHUNKS || k < (u32)G::CHUNKS) reinterpret_cast<uint4*>(tile32)[k] = pre[j];
        }
        const TileInfo ti = cur;
        __syncthreads();
        // ---- this lane's line ------------------------------------------------------------
        const u64 line = ti.first + (u32)tid;
        const bool active = (u32)tid < ti.count;
        const u32 my_off = pre_off;
        const u32 my_end = line + 1 < B.n ? pre_end : (u32)B.nbytes;
        const bool sane = active && line_sane(my_off, my_end, B.nbytes);
        const bool in_lds = sane && ti.len != 0u && my_off >= ti.s0 && my_end <= ti.e;
        const int ls = (int)(my_off - ti.s0 + ti.delta), le = (int)(my_end - ti.s0 + ti.delta);
        tl.ev += active ? 1u : 0u;
        tl.perr += (active && !sane) ? 1u : 0u;   // offsets out of order or past the batch: no line to parse
        // ---- the fast tier: the generator's layout, proven to parse as org.json parses it ----
        bool fast = false, pend = false, tok = false, joined = false;
        u32 campaign = 0, klen = 36u;
        i64 tv = 0;
        u32 kw[KEY_WORDS];
#pragma unroll
        for (int k = 0; k < (int)KEY_WORDS; ++k) kw[k] = 0u;
        ColProbe<SERIAL> pr;
#pragma unroll
        for (int j = 0; j < (int)(sizeof(pr.q) / sizeof(pr.q[0])); ++j) pr.q[j] = make_uint4(0, 0, 0, 0);
        pr.ib = 0;
        if (in_lds) {
            CanonA ca;
            CanonB cb;
            cb.view = false;
            if constexpr (TBL) {
                fast = tbl_stage1(lsrc, ls, le, ca) && tbl_stage2(lsrc, ls, le, ca, cb);
            } else {
                fast = vocab_stage1<false>(lsrc, ls, le, ca) && vocab_stage2<false>(lsrc, ls, le, ca, cb);
                if (!fast) fast = canon_stage1<false>(lsrc, ls, le, ca) && canon_stage2<false>(lsrc, ls, le, ca, cb);
            }
            pend = fast && cb.view;                                           // EventFilterBolt
            if (pend) {
                // RedisJoinBolt's lookup of the 36 raw bytes, issued before the time parse and
                // the next tile's loads so that waiting for it never waits for them
                tl.view++;
#pragma unroll
                for (int k = 0; k < (int)CKEY_WORDS; ++k) kw[k] = ca.kw[k];
                cc_probe_issue<SERIAL>(P, ca.kw, pr);
                tok = cb.tlen <= 20 ? parse_digits_regs(cb.td, cb.tlen, tv)   // td: the time's first 20 bytes
                                    : parse_digits(lsrc, ls + ca.t0, ls + ca.t0 + cb.tlen, tv);
            }
        }
        // ---- the next tile's bytes land while this one is joined and written (issued before the
        // parse instead, Kernel 4's order, it measured the same) ----------------------------------
        if (t + gridDim.x < B.n_tiles) {
            cur = col_tile_info<G::CAP>(B, t + gridDim.x);
            issue_tile_loads(B.bytes, B.off, B.n, (u32)tid, cur, pre, pre_off, pre_end);
        }
        if (pend) {
            const u32 ci = cc_probe_finish<SERIAL>(P, kw, pr);
            if (ci == EMPTY_SLOT) {
                count_miss(P, kw, 36u, true, tl);   // dropped (:465-467), or a key of another shard
            } else {
                tl.join++;
                joined = true;
                campaign = ci;
                if (!tok) { tl.terr++; tv = 0; }    // still a row: the reference parses after the join
            }
        }
        // ---- any other line: the general parser in the same lane (a branch no generator line
        // takes; the hint keeps what is spilled around the call inside it, as in Kernel 4) ------
        if (__builtin_expect(sane && !fast, 0)) {
            JoinLane o;
            o.joined = o.tok = false;
            o.campaign = o.klen = 0u;
            o.tv = 0;
#pragma unroll
            for (int k = 0; k < (int)KEY_WORDS; ++k) o.kw[k] = 0u;
            Tally tg{0, 0, 0, 0, 0, 0, 0, 0};
            if (in_lds) {
                const LdsSrc3 s3{(lds_u32*)tile32};
                if (TBL) join_tbl_general(s3, ls, le, P, tg, o);
                else join_json_general(s3, ls, le, P, tg, o);
            } else {   // a line outside the staged tile (long lines, offsets out of order)
                const GlbSrc gs{B.bytes + my_off, (u64)(my_end - my_off)};
                const int len = (int)(my_end - my_off);
                if (TBL) join_tbl_general(gs, 0, len, P, tg, o);
                else join_json_general(gs, 0, len, P, tg, o);
            }
            tl.view += tg.view;
            tl.join += tg.join;
            tl.miss += tg.miss;
            tl.perr += tg.perr;
            tl.terr += tg.terr;
            tl.frn += tg.frn;
            if (o.joined) {
                joined = true;
                tok = o.tok;
                campaign = o.campaign;
                klen = o.klen;
                tv = o.tv;
#pragma unroll
                for (int k = 0; k < (int)KEY_WORDS; ++k) kw[k] = o.kw[k];
            }
        }
        // ---- the tile's joined rows in LDS, in rank order --------------------------------------
        const unsigned long long jm = __ballot(joined);
        const u32 cnt = (u32)__popcll(jm);
        n_fast += (u32)__popcll(__ballot(fast));
        if (joined) {
            const u32 r = __builtin_amdgcn_mbcnt_hi((u32)(jm >> 32), __builtin_amdgcn_mbcnt_lo((u32)jm, 0u));
            st[JOIN_S_CAMP / 4 + r] = campaign;
            st[JOIN_S_TIME / 4 + 2 * r] = (u32)(u64)tv;
            st[JOIN_S_TIME / 4 + 2 * r + 1] = (u32)((u64)tv >> 32);
            st8[JOIN_S_LANE + r] = join_lane_pack((u32)tid, tok);
            if (J.keys) {
                st8[JOIN_S_KLEN + r] = (u8)klen;
#pragma unroll
                for (int k = 0; k < (int)KEY_WORDS; ++k) st[JOIN_S_KEY / 4 + r * KEY_WORDS + k] = kw[k];
            }
        }
        __syncthreads();
        // ---- LDS -> the tile's block of the scratch area: rows [0, cnt) of every array, whole
        // 16-byte vectors (a vector's bytes past the rows stay inside the array) -------------------
        u8* blk = J.scratch + t * (u64)tile_bytes;
        auto put = [&](u32 at, u32 bytes) {
            const u32 nv = (bytes + 15u) >> 4;
            for (u32 k = (u32)tid; k < nv; k += SCAN_TPB)
                reinterpret_cast<uint4*>(blk + at)[k] = reinterpret_cast<const uint4*>(st8 + at)[k];
        };
        put(JOIN_S_CAMP, cnt * 4u);
        put(JOIN_S_TIME, cnt * 8u);
        put(JOIN_S_LANE, cnt);
        if (J.keys) {
            put(JOIN_S_KLEN, cnt);
            put(JOIN_S_KEY, cnt * JOIN_KEY_STRIDE);
        }
        if (tid == 0) J.tile_count[t] = cnt;
        // (the next iteration's barrier orders these reads of st before its rewrite; the
        // barrier above ordered every read of the tile before the next one is stored)
    }
    flush_tally(P, tl, tid);   // P.stats: the call's own tallies -- one atomic per counter and workgroup
    if (tid == 0 && n_fast) atomicAdd(&P.stats[ST_COUNT_], (unsigned long long)n_fast);
}

// ---- b: the exclusive prefix over tile_count.  Workgroup g owns tiles [g, g + 1) x JOIN_PREFIX_SEG
// and waits for nobody: it sums every count in front of its segment itself (16-byte loads of a
// few hundred KiB that stay in L2), then scans the segment in rounds of one value per thread.
// One workgroup over the whole array (split_prefix_kernel's shape, a run of values per thread)
// took 0.26 ms for the 156,250 tiles of 10M lines: profiles/AB_LOG.md "Kernel 7". ---------------
constexpr int JOIN_PREFIX_TPB = 1024;
constexpr int JOIN_PREFIX_ROUNDS = 4;
constexpr int JOIN_PREFIX_SEG = JOIN_PREFIX_ROUNDS * JOIN_PREFIX_TPB;
__global__ __launch_bounds__(JOIN_PREFIX_TPB) void join_prefix_kernel(const u32* count, u32* prefix, u64 n_tiles) {
    __shared__ u32 wsum[JOIN_PREFIX_TPB / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 seg = (u64)blockIdx.x * JOIN_PREFIX_SEG;   // (< n_tiles; count is 16-byte aligned)
    u32 s = 0;
    for (u64 i = (u64)tid; i < seg / 4; i += JOIN_PREFIX_TPB) {
        const uint4 v = reinterpret_cast<const uint4*>(count)[i];
        s += v.x + v.y + v.z + v.w;
    }
    s = wave_sum(s);
    if (lane == 0) wsum[wave] = s;
    __syncthreads();
    u32 base = 0;   // the total is at most the batch's lines: < 2^32
    for (int w = 0; w < JOIN_PREFIX_TPB / 64; ++w) base += wsum[w];
    __syncthreads();
    for (int r = 0; r < JOIN_PREFIX_ROUNDS; ++r) {
        const u64 i = seg + (u64)(r * JOIN_PREFIX_TPB + tid);
        const u32 c = i < n_tiles ? count[i] : 0u;
        u32 inc = c;   // inclusive scan within the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const u32 x = __shfl_up(inc, o, 64);
            if (lane >= o) inc += x;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        u32 pre = base + inc - c, total = 0;
        for (int w = 0; w < JOIN_PREFIX_TPB / 64; ++w) {
            pre += w < wave ? wsum[w] : 0u;
            total += wsum[w];
        }
        if (i < n_tiles) prefix[i] = pre;
        base += total;
        __syncthreads();   // the waves' sums are read before the next round's
    }
}

// ---- c: the rows into the columns --------------------------------------------------------
// bytes [at, at + bytes) of the column at col (16-byte aligned) from the LDS words src (the
// run's bytes from src's byte 0 on; readable one vector past them): 16-byte stores over the
// aligned middle (join_span), stores of `unit` bytes (4: at and bytes are multiples of 4; or 1)
// at the ragged ends.
__device__ __forceinline__ void join_emit(u8* col, u64 at, u32 bytes, const u32* src, u32 unit, int tid) {
    u64 a16, b16;
    join_span(at, bytes, &a16, &b16);
    const WordSrc<const u32*> ws{src};
    const u32 nv = (u32)((b16 - a16) >> 4), head = (u32)(a16 - at);
    for (u32 k = (u32)tid; k < nv; k += SCAN_TPB) {
        const int s = (int)(head + 16u * k);
        reinterpret_cast<uint4*>(col + a16)[k] = make_uint4(ws.load4(s), ws.load4(s + 4), ws.load4(s + 8), ws.load4(s + 12));
    }
    // the ends: fewer than 16 bytes each
    const u32 tail = (u32)(at + bytes - b16);
    if (unit == 4u) {
        if ((u32)tid < head / 4u) *reinterpret_cast<u32*>(col + at + 4u * tid) = ws.load4(4 * tid);
        if ((u32)tid < tail / 4u) *reinterpret_cast<u32*>(col + b16 + 4u * tid) = ws.load4((int)(b16 - at) + 4 * tid);
    } else {
        if ((u32)tid < head) col[at + tid] = (u8)ws.b(tid);
        if ((u32)tid < tail) col[b16 + tid] = (u8)ws.b((int)(b16 - at) + tid);
    }
}

constexpr int JOIN_PACK_WG_PER_CU = 16;
__global__ __launch_bounds__(SCAN_TPB) void join_pack_kernel(const JoinParams J) {
    // the tile's block, then its rows' source rows and time_ok bytes; a vector of slack behind each
    __shared__ __attribute__((aligned(16))) u32 blk[JOIN_TILE_BYTES_KEYS / 4 + 4];
    __shared__ __attribute__((aligned(16))) u32 rows[JOIN_TILE + 4];
    __shared__ __attribute__((aligned(16))) u32 okw[JOIN_TILE / 4 + 4];
    const int tid = threadIdx.x;
    const u32 tile_bytes = J.keys ? (u32)JOIN_TILE_BYTES_KEYS : (u32)JOIN_TILE_BYTES;
    u8* const blk8 = reinterpret_cast<u8*>(blk);
    for (u64 t = blockIdx.x; t < J.b.n_tiles; t += gridDim.x) {
        const JoinRun run = join_run(J.prefix[t], J.tile_count[t], J.cap_rows);
        if (run.count == 0u) continue;   // (uniform: nothing joined, or the tile lies past cap_rows)
        const u8* sb = J.scratch + t * (u64)tile_bytes;
        auto get = [&](u32 at, u32 bytes) {
            const u32 nv = (bytes + 15u) >> 4;
            for (u32 k = (u32)tid; k < nv; k += SCAN_TPB)
                reinterpret_cast<uint4*>(blk8 + at)[k] = reinterpret_cast<const uint4*>(sb + at)[k];
        };
        get(JOIN_S_CAMP, run.count * 4u);
        get(JOIN_S_TIME, run.count * 8u);
        get(JOIN_S_LANE, run.count);
        if (J.keys) {
            get(JOIN_S_KLEN, run.count);
            get(JOIN_S_KEY, run.count * JOIN_KEY_STRIDE);
        }
        __syncthreads();
        if ((u32)tid < run.count) {
            const u32 b = blk8[JOIN_S_LANE + tid];
            rows[tid] = join_lane_row(t, b);
            reinterpret_cast<u8*>(okw)[tid] = join_lane_ok(b);
        }
        __syncthreads();
        u8* const out = J.b.out;
        join_emit(out + J.b.start[JC_CAMPAIGN], run.first * 4u, run.count * 4u, blk + JOIN_S_CAMP / 4, 4u, tid);
        join_emit(out + J.b.start[JC_ROW], run.first * 4u, run.count * 4u, rows, 4u, tid);
        join_emit(out + J.b.start[JC_TIME], run.first * 8u, run.count * 8u, blk + JOIN_S_TIME / 4, 4u, tid);
        join_emit(out + J.b.start[JC_TIME_OK], run.first, run.count, okw, 1u, tid);
        if (J.keys) {
            join_emit(out + J.b.start[JC_KEY], run.first * JOIN_KEY_STRIDE, run.count * JOIN_KEY_STRIDE, blk + JOIN_S_KEY / 4, 4u, tid);
            join_emit(out + J.b.start[JC_KEY_LEN], run.first, run.count, blk + JOIN_S_KLEN / 4, 1u, tid);
        }
        __syncthreads();   // the block is read before the next tile's overwrites it
    }
}

u32 join_max_grid(int cus, bool tbl) {
    const u64 per_cu = tbl ? JoinGeom<true>::WG_PER_CU : JoinGeom<false>::WG_PER_CU;
    return (u32)((u64)(cus > 0 ? cus : 1) * per_cu);
}

u32 join_grid(u64 n_tiles, int cus, bool tbl) {
    const u64 want = join_max_grid(cus, tbl);
    return (u32)(n_tiles < want ? n_tiles : want);
}

void launch_join(const JoinParams& p, int cus, hipStream_t s) {
    if (p.b.n == 0) return;
    const dim3 g(join_grid(p.b.n_tiles, cus, p.b.tbl != 0)), b(SCAN_TPB);
    if (p.b.tbl) {
        if (p.sp.probe_serial) hipLaunchKernelGGL((join_kernel<true, true>), g, b, 0, s, p);
        else hipLaunchKernelGGL((join_kernel<true, false>), g, b, 0, s, p);
    } else {
        if (p.sp.probe_serial) hipLaunchKernelGGL((join_kernel<false, true>), g, b, 0, s, p);
        else hipLaunchKernelGGL((join_kernel<false, false>), g, b, 0, s, p);
    }
}

void launch_join_prefix(const JoinParams& p, hipStream_t s) {
    if (p.b.n == 0) return;
    const dim3 g((u32)((p.b.n_tiles + JOIN_PREFIX_SEG - 1) / JOIN_PREFIX_SEG)), b(JOIN_PREFIX_TPB);
    hipLaunchKernelGGL(join_prefix_kernel, g, b, 0, s, p.tile_count, p.prefix, p.b.n_tiles);
}

void launch_join_pack(const JoinParams& p, int cus, hipStream_t s) {
    if (p.b.n == 0 || p.cap_rows == 0) return;
    const u64 want = (u64)(cus > 0 ? cus : 1) * JOIN_PACK_WG_PER_CU;
    const dim3 g((u32)(p.b.n_tiles < want ? p.b.n_tiles : want)), b(SCAN_TPB);
    hipLaunchKernelGGL(join_pack_kernel, g, b, 0, s, p);
}

}  // namespace ysb
