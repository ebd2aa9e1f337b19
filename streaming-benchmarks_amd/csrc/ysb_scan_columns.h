// ysb_scan_columns.h -- Kernel 4: a batch of event lines decoded into the fork's columnar
// hand-off layout (WindowedArrowFormatBolter, flink-benchmarks/.../
// AdvertisingTopologyNative.java:278-356): seven fixed-stride columns of widths
// {36,36,36,4,4,8,8} -- user_id, page_id, ad_id, ad_type, event_type, the parsed
// event_time and a stamp -- each starting on a 4096-byte page (:291-302), plus an
// Arrow-style validity bitmap behind them (include/ysb_hip.h ysb_columns_layout).
// Part of the scan kernel's translation unit: included at the end of ysb_scan.hip, whose
// code it shares rather than repeats -- the byte sources, the canonical / vocabulary tiers,
// tbl_stage1/2, decode_str, the org.json machine (parse_line, here keeping all seven
// values: KeepAll), the .tbl row split (tbl_split), the per-line sanity test (line_sane)
// and the tile loader (TileInfo, tile_lines / tile_bytes, issue_tile_loads).
//
// Shape: one-wave workgroups, one line per lane, tiles of 64 lines staged into LDS (the
// next tile's bytes are loaded into registers while this one is parsed).  Lane i takes line
// i of the tile, so the tile's validity word is one ballot.  A fast tier takes the
// generator's JSON layout (vocab_stage1/2, then canon_stage1/2: both prove the line parses
// exactly as org.json parses it and locate every value) and the generator's .tbl rows
// (tbl_stage1/2); every other line runs through the general parser in the same lane
// (parse_line or tbl_split; lines outside the staged tile through GlbSrc).  The 64 rows of a
// tile are contiguous in every column (2304 / 256 / 512 bytes, 128-byte aligned), so each
// column's block is assembled in LDS and written with 16-byte stores, whole lines for a
// full tile.
#pragma once

namespace ysb {

// ---------------------------------------------------------------------------
// One decoded row: what WindowedArrowFormatBolter.flatMap puts per tuple (:323-334).
// ---------------------------------------------------------------------------
constexpr int COL_ROW_BYTES = 3 * 36 + 4 + 4 + 8 + 8;   // 132
constexpr int COL_USER = 13, COL_PAGE = 64;             // value offsets in the generator's JSON layout
static_assert(COL_USER == sizeof(YSB_P0) - 1 && COL_PAGE == COL_USER + 36 + (int)sizeof(YSB_P1) - 1 &&
                  CanonGeo<false>::AD == COL_PAGE + 36 + (int)sizeof(YSB_P2) - 1 &&
                  CanonGeo<false>::PREFIX == CanonGeo<false>::AD + 36 + (int)sizeof(YSB_P3) - 1,
              "value offsets of the generator's layout");

struct ColRow {
    u32 id[3][9];   // user_id, page_id, ad_id: the first 36 bytes
    u32 at, et;     // ad_type, event_type: the first 4 bytes
    i64 tv;         // Long.parseLong(event_time)
};

// The first 4 * N bytes of a String value (put(bytes, 0, entry_len) throws on a shorter
// array: false).  Escaped values are decoded (decode_str) only as far as needed.
template <class S, int N>
__device__ __forceinline__ bool span_prefix(const S& src, const Span& v, u32 (&w)[N]) {
    if (!v.esc) {
        if (v.e - v.s < 4 * N) return false;
#pragma unroll
        for (int k = 0; k < N; ++k) w[k] = src.load4(v.s + 4 * k);
        return true;
    }
    u8 buf[4 * N + 4];
    if (decode_str(src, v.s, v.e, buf, 4 * N) < 4 * N) return false;
#pragma unroll
    for (int k = 0; k < N; ++k)
        w[k] = (u32)buf[4 * k] | ((u32)buf[4 * k + 1] << 8) | ((u32)buf[4 * k + 2] << 16) | ((u32)buf[4 * k + 3] << 24);
    return true;
}

// The row of six String spans (user_id .. event_time): every value long enough for its
// column and the time a long.
template <class S>
__device__ __forceinline__ bool row_of_spans(const S& src, const Span* sp, ColRow& r) {
    u32 a[1], b[1];
    bool ok = span_prefix<S, 9>(src, sp[0], r.id[0]);
    ok = ok && span_prefix<S, 9>(src, sp[1], r.id[1]);
    ok = ok && span_prefix<S, 9>(src, sp[2], r.id[2]);
    ok = ok && span_prefix<S, 1>(src, sp[3], a) && span_prefix<S, 1>(src, sp[4], b);
    ok = ok && span_long(src, sp[5], r.tv);
    if (ok) {
        r.at = a[0];
        r.et = b[0];
    }
    return ok;
}

// A line in any layout: new JSONObject(line) + getString of the required keys.
template <class S>
__device__ __noinline__ bool col_json_general(const S& src, int s, int e, u32 require, ColRow& r) {
    KeepAll k;
    if (!parse_line(src, s, e, require, k)) return false;
    return row_of_spans(src, k.sp, r);
}

// Any .tbl row: readLine's terminator stripped, items = line.split("\\|") (MockWindowedFlatMap,
// :197-226).  items[0..5] lie between the first six '|' (the sixth, or the end of the line);
// items[5] exists iff it is not empty or a later item is not -- an empty one is no long either
// way, so the row is valid iff the five values are long enough and items[5] parses.
template <class S>
__device__ __noinline__ bool col_tbl_general(const S& src, int s, int e, ColRow& r) {
    int p[6];
    if (tbl_split(src, s, e, p) < 5) return false;
    const Span sp[6] = {{s, p[0], 0},        {p[0] + 1, p[1], 0}, {p[1] + 1, p[2], 0},
                        {p[2] + 1, p[3], 0}, {p[3] + 1, p[4], 0}, {p[4] + 1, p[5], 0}};
    return row_of_spans(src, sp, r);
}

template <bool TBL>
struct ColGeom {
    static constexpr int CAP = Geom<TBL>::CAP;            // the scan's tile capacity
    static constexpr int CHUNKS = CAP / 16;
    static constexpr int CPT = (CHUNKS + SCAN_TPB - 1) / SCAN_TPB;
    static constexpr int TILE_WORDS = (CAP + 64) / 4;     // 64 B slack for reads past a tile
    static constexpr int LDS = CAP + 64 + TILE_LINES * COL_ROW_BYTES;
    static constexpr int WG_PER_CU = 163840 / ((LDS + 1279) / 1280 * 1280);
};
static_assert(TILE_LINES == 64, "a tile's validity word is one 64-lane ballot");

// Tile t (< P.n_tiles) of the batch by the scan's tile_info, its two bounds straight from
// P.off (one wave per workgroup: no LDS copy of them).  len == 0: nothing staged (offsets
// out of order or past the batch), every line from HBM.
template <int CAP>
__device__ __forceinline__ TileInfo col_tile_info(const ColParams& P, u64 t) {
    const u64 first = t * TILE_LINES, next = first + TILE_LINES;
    const u32 tb[2] = {P.off[first], next < P.n ? P.off[next] : (u32)P.nbytes};   // (nbytes < 4 GiB)
    return tile_info<CAP>(P, t, t, tb);
}

// column c's width, and the dword offset of its block of a tile in the LDS staging area
__host__ __device__ constexpr int col_w(int c) { return c < 3 ? 36 : c < 5 ? 4 : 8; }
__host__ __device__ constexpr int col_st(int c) {
    int o = 0;
    for (int k = 0; k < c; ++k) o += col_w(k) * TILE_LINES / 4;
    return o;
}
static_assert(col_st(7) * 4 == TILE_LINES * COL_ROW_BYTES, "the staging area holds a tile's rows");

// (two waves per SIMD: without the bound the JSON instantiation took 256 VGPRs + 14 AGPRs,
// one wave per SIMD, for the general parser no generator line calls; profiles/AB_LOG.md)
template <bool TBL>
__global__ __launch_bounds__(SCAN_TPB) __attribute__((amdgpu_waves_per_eu(2))) void columns_kernel(const ColParams P) {
    using G = ColGeom<TBL>;
    constexpr int CPT = G::CPT;
    __shared__ __attribute__((aligned(16))) u32 tile32[G::TILE_WORDS];
    __shared__ __attribute__((aligned(16))) u32 st[TILE_LINES * COL_ROW_BYTES / 4];
    const int tid = threadIdx.x;
    const LdsSrc lsrc{tile32};
    u32 n_valid = 0, n_fast = 0;
    if (tid < 16) tile32[G::CAP / 4 + tid] = 0u;   // the slack past a full tile

    // a tile's bytes and line offsets HBM -> registers by the scan's loader; lane i receives
    // line i's offsets
    uint4 pre[CPT];
    u32 pre_off = 0, pre_end = 0;
    u64 t = blockIdx.x;
    if (t >= P.n_tiles) return;
    TileInfo cur = col_tile_info<G::CAP>(P, t);
    issue_tile_loads(P.bytes, P.off, P.n, (u32)tid, cur, pre, pre_off, pre_end);
    for (; t < P.n_tiles; t += gridDim.x) {
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
        const u32 my_end = line + 1 < P.n ? pre_end : (u32)P.nbytes;
        // the next tile's bytes land while this one is parsed
        if (t + gridDim.x < P.n_tiles) {
            cur = col_tile_info<G::CAP>(P, t + gridDim.x);
            issue_tile_loads(P.bytes, P.off, P.n, (u32)tid, cur, pre, pre_off, pre_end);
        }
        const bool sane = active && line_sane(my_off, my_end, P.nbytes);
        const bool in_lds = sane && ti.len != 0u && my_off >= ti.s0 && my_end <= ti.e;
        const int ls = (int)(my_off - ti.s0 + ti.delta), le = (int)(my_end - ti.s0 + ti.delta);
        ColRow r;
        r.tv = 0;
        bool valid = false, fast = false;
        if (in_lds) {
            CanonA ca;
            CanonB cb;
            if constexpr (TBL) {
                fast = tbl_stage1(lsrc, ls, le, ca) && tbl_stage2(lsrc, ls, le, ca, cb);
                if (fast) {
                    // '|' at 36, 73, 110, e3, e4 and none after: exactly six items
                    load_span(lsrc, ls, r.id[0]);
                    load_span(lsrc, ls + 37, r.id[1]);
#pragma unroll
                    for (int k = 0; k < 9; ++k) r.id[2][k] = ca.kw[k];
                    r.at = lsrc.load4(ls + 111);
                    r.et = lsrc.load4(ls + ca.e3 + 1);
                    valid = ca.e3 - 111 >= 4 && ca.e4 - ca.e3 - 1 >= 4 &&
                            (cb.tlen <= 20 ? parse_digits_regs(cb.td, cb.tlen, r.tv)
                                           : parse_digits(lsrc, ls + ca.t0, ls + ca.t0 + cb.tlen, r.tv));
                }
            } else {
                using CG = CanonGeo<false>;
                fast = vocab_stage1<false>(lsrc, ls, le, ca) && vocab_stage2<false>(lsrc, ls, le, ca, cb);
                if (!fast) fast = canon_stage1<false>(lsrc, ls, le, ca) && canon_stage2<false>(lsrc, ls, le, ca, cb);
                if (fast) {
                    // the seven keys in the generator's order, every value free of quotes,
                    // backslashes and control bytes: the String values are the raw bytes
                    load_span(lsrc, ls + COL_USER, r.id[0]);
                    load_span(lsrc, ls + COL_PAGE, r.id[1]);
#pragma unroll
                    for (int k = 0; k < 9; ++k) r.id[2][k] = ca.kw[k];
                    r.at = lsrc.load4(ls + CG::PREFIX);
                    r.et = lsrc.load4(ls + ca.e3 + CG::SEP);
                    valid = ca.e3 - CG::PREFIX >= 4 && ca.e4 - ca.e3 - CG::SEP >= 4 &&
                            (cb.tlen <= 20 ? parse_digits_regs(cb.td, cb.tlen, r.tv)   // td: the time's first 20 bytes
                                           : parse_digits(lsrc, ls + ca.t0, ls + ca.e5, r.tv));
                }
            }
        }
        // (a branch no generator line takes.  The hint keeps what the kernel spills around
        // the general parser's call inside the branch: without it the JSON fast tier took
        // 1.40 ms for 0.92, profiles/AB_LOG.md "Scan unit de-duplication")
        if (__builtin_expect(sane && !fast, 0)) {
            if (in_lds) {
                const LdsSrc3 s3{(lds_u32*)tile32};
                valid = TBL ? col_tbl_general(s3, ls, le, r) : col_json_general(s3, ls, le, P.require_mask, r);
            } else {   // a line outside the staged tile (long lines, offsets out of order)
                const GlbSrc gs{P.bytes + my_off, (u64)(my_end - my_off)};
                const int len = (int)(my_end - my_off);
                valid = TBL ? col_tbl_general(gs, 0, len, r) : col_json_general(gs, 0, len, P.require_mask, r);
            }
        }
        // ---- the tile's column blocks in LDS ---------------------------------------------
        u32 t0 = (u32)(u64)r.tv, t1 = (u32)((u64)r.tv >> 32);
        u32 m0 = (u32)(u64)P.stamp, m1 = (u32)((u64)P.stamp >> 32);
        if (P.java_order) {   // MappedByteBuffer.putLong: big-endian
            const u32 a = __builtin_bswap32(t1), b = __builtin_bswap32(m1);
            t1 = __builtin_bswap32(t0);
            t0 = a;
            m1 = __builtin_bswap32(m0);
            m0 = b;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int k = 0; k < 9; ++k) st[col_st(c) + tid * 9 + k] = valid ? r.id[c][k] : 0u;
        st[col_st(3) + tid] = valid ? r.at : 0u;
        st[col_st(4) + tid] = valid ? r.et : 0u;
        st[col_st(5) + 2 * tid] = valid ? t0 : 0u;
        st[col_st(5) + 2 * tid + 1] = valid ? t1 : 0u;
        st[col_st(6) + 2 * tid] = valid ? m0 : 0u;
        st[col_st(6) + 2 * tid + 1] = valid ? m1 : 0u;
        const unsigned long long vm = __ballot(valid), fm = __ballot(fast);
        n_valid += (u32)__popcll(vm);
        n_fast += (u32)__popcll(fm);
        __syncthreads();
        // ---- LDS -> HBM: rows [first, first + count) of every column, 16 bytes per lane ---
#pragma unroll
        for (int c = 0; c < 7; ++c) {
            u8* dst = P.out + P.start[c] + ti.first * (u64)col_w(c);   // 16-byte aligned
            const u32 bytes = ti.count * (u32)col_w(c);
            const u32 full = bytes >> 4, tail = (bytes & 15u) >> 2;
            for (u32 k = (u32)tid; k < full; k += SCAN_TPB)
                reinterpret_cast<uint4*>(dst)[k] = reinterpret_cast<const uint4*>(st + col_st(c))[k];
            if ((u32)tid < tail)   // a batch's last, partial tile
                reinterpret_cast<u32*>(dst)[4 * full + tid] = st[col_st(c) + 4 * full + tid];
        }
        if (tid == 0) reinterpret_cast<unsigned long long*>(P.out + P.start[7])[ti.first / TILE_LINES] = vm;
        // (the next iteration's barrier orders these reads of st before its rewrite; the
        // barrier above ordered every read of the tile before the next one is stored)
    }
    if (tid == 0) {
        if (n_valid) atomicAdd(&P.info[0], (unsigned long long)n_valid);
        if (n_fast) atomicAdd(&P.info[1], (unsigned long long)n_fast);
    }
}

void launch_columns(const ColParams& p, int cus, hipStream_t s) {
    if (p.n == 0) return;
    const int per_cu = p.tbl ? ColGeom<true>::WG_PER_CU : ColGeom<false>::WG_PER_CU;
    const u64 want = (u64)(cus > 0 ? cus : 1) * (u64)per_cu;
    const dim3 g((u32)(p.n_tiles < want ? p.n_tiles : want)), b(SCAN_TPB);
    if (p.tbl) hipLaunchKernelGGL(columns_kernel<true>, g, b, 0, s, p);
    else hipLaunchKernelGGL(columns_kernel<false>, g, b, 0, s, p);
}

}  // namespace ysb
