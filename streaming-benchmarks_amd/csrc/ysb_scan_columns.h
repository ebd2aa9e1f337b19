// ysb_scan_columns.h -- Kernel 4: a batch of event lines decoded into the fork's columnar
// hand-off layout (WindowedArrowFormatBolter, flink-benchmarks/.../
// AdvertisingTopologyNative.java:278-356): seven fixed-stride columns of widths
// {36,36,36,4,4,8,8} -- user_id, page_id, ad_id, ad_type, event_type, the parsed
// event_time and a stamp -- each starting on a 4096-byte page (:291-302), plus an
// Arrow-style validity bitmap behind them (include/ysb_hip.h ysb_columns_layout).
// Part of the scan kernel's translation unit: included at the end of ysb_scan.hip, after
// the byte sources, the canonical / vocabulary tiers, tbl_stage1/2, decode_str and the
// org.json machine, none of which it changes.
//
// Shape: one-wave workgroups, one line per lane, tiles of 64 lines staged into LDS (the
// next tile's bytes are loaded into registers while this one is parsed).  Lane i takes line
// i of the tile, so the tile's validity word is one ballot.  A fast tier takes the
// generator's JSON layout (vocab_stage1/2, then canon_stage1/2: both prove the line parses
// exactly as org.json parses it and locate every value) and the generator's .tbl rows
// (tbl_stage1/2); every other line runs through the general parser in the same lane
// (parse_line_all below; lines outside the staged tile through GlbSrc).  The 64 rows of a
// tile are contiguous in every column (2304 / 256 / 512 bytes, 128-byte aligned), so each
// column's block is assembled in LDS and written with 16-byte stores, whole lines for a
// full tile.
#pragma once

namespace ysb {

// ---------------------------------------------------------------------------
// parse_line (ysb_orgjson.h) with the String value of every key DeserializeBolt reads:
// sp[k] is the span of key bit k (0 user_id .. 5 event_time, 6 ip_address).  The same
// machine, state for state; only the value capture differs.
// ---------------------------------------------------------------------------
template <class S>
__device__ __noinline__ bool parse_line_all(const S& src, int s, int e, u32 require, Span (&sp)[7]) {
    int end = e;                                                           // NUL: end of input
    for (int q = s & ~3; q < e; q += 4) {                                  // word at a time
        const u32 w = src.load4(q);
        const u32 z = (w - 0x01010101u) & ~w & 0x80808080u;                // a zero byte (exact for the lowest)
        if (z == 0u) continue;
        int k = 0;
        for (; k < 4; ++k) {
            const int pos = q + k;
            if (pos >= s && pos < e && ((w >> (8 * k)) & 0xFFu) == 0u) break;
        }
        if (k < 4) { end = q + k; break; }
    }
    OjTok<S> t{src, s, end, false, -1, 0u};
    if (t.clean() != '{') return false;                                    // must begin with '{'
    int open[OJ_MAX_DEPTH + 1];                                            // each open container's bracket
    u8 role[OJ_MAX_DEPTH + 1];
    int depth = 1;
    open[1] = t.p - 1;
    role[1] = OJR_TOP;
    int state = OJS_KEY, kpos = 0;
    OjKey key{OJK_RAW, 0, 0};
    u32 kid = 0, seen = 0;
    u32 khash[OJ_TOP_KEYS];   // the top-level object's key hashes so far
    int ntop = 0;
    for (;;) {
        OjVal v;
        u8 nested = 0;          // != 0: v opened a container in this role
        bool closed = false;    // the innermost container closed
        int c;
        switch (state) {
        case OJS_KEY:                                                      // a key, or '}'
            c = t.clean();
            if (c < 0) return false;                                       // must end with '}'
            if (c == '}') { closed = true; break; }
            t.back();
            kpos = t.p;
            if (!oj_value(t, v)) return false;
            if (v.kind == OJV_OBJ || v.kind == OJV_ARR) { nested = OJR_KEY; break; }
            kid = 0;
            if (v.kind == OJV_STR) {
                key = OjKey{OJK_STR, v.a, v.b};
                if (depth == 1) kid = v.esc ? match_key_esc(src, v.a, v.b) : match_key_raw(src, v.a, v.b - v.a);
            } else {
                const int k = oj_token_kind(src, v.a, v.b);
                key = OjKey{k == OJ_TRUE ? OJK_TRUE : k == OJ_FALSE ? OJK_FALSE : k == OJ_NULL ? OJK_NULL : OJK_RAW,
                            v.a, v.b};
                if (depth == 1 && key.kind == OJK_RAW) kid = match_key_raw(src, v.a, v.b - v.a);
            }
            state = OJS_COLON;
            continue;
        case OJS_COLON:
            if (t.clean() != ':') return false;                            // Expected a ':' after a key
            if (depth == 1 && ntop < OJ_TOP_KEYS) {
                // top level: compare hashes with the earlier keys', re-walk only on a hit
                const u32 h = oj_key_hash(src, key);
                bool hit = false;
#pragma unroll
                for (int k = 0; k < OJ_TOP_KEYS; ++k) hit |= k < ntop && khash[k] == h;
                if (hit && oj_dup_key(src, open[depth], kpos, end, key)) return false;   // Duplicate key
#pragma unroll
                for (int k = 0; k < OJ_TOP_KEYS; ++k)
                    if (k == ntop) khash[k] = h;
                ++ntop;
            } else if (oj_dup_key(src, open[depth], kpos, end, key)) {
                return false;                                                   // Duplicate key
            }
            state = OJS_VALUE;
            continue;
        case OJS_VALUE:
            if (!oj_value(t, v)) return false;
            if (v.kind == OJV_OBJ || v.kind == OJV_ARR) { kid = 0; nested = OJR_VALUE; break; }
            if (kid && (v.kind == OJV_STR || oj_token_kind(src, v.a, v.b) == OJ_STR)) {   // getString
                const Span val{v.a, v.b, v.kind == OJV_STR ? v.esc : 0};
#pragma unroll
                for (int k = 0; k < 7; ++k)
                    if (kid == (1u << k)) sp[k] = val;
                seen |= kid;
            }
            kid = 0;
            state = OJS_OSEP;
            continue;
        case OJS_OSEP:                                                     // ',' / ';' / '}'
            c = t.clean();
            if (c == ',' || c == ';') {
                if (t.clean() == '}') { closed = true; break; }
                if (!t.back()) return false;
                state = OJS_KEY;
                continue;
            }
            if (c == '}') { closed = true; break; }
            return false;                                                  // Expected a ',' or '}'
        case OJS_AFIRST:
            c = t.clean();
            if (c == ']') { closed = true; break; }
            if (!t.back()) return false;
            state = OJS_AELEM;
            continue;
        case OJS_AELEM:
            c = t.clean();
            if (!t.back()) return false;
            if (c == ',') { state = OJS_ASEP; continue; }                  // an empty slot: NULL
            if (!oj_value(t, v)) return false;
            if (v.kind == OJV_OBJ || v.kind == OJV_ARR) { nested = OJR_ELEM; break; }
            state = OJS_ASEP;
            continue;
        default:                                                           // OJS_ASEP
            c = t.clean();
            if (c == ',') {
                if (t.clean() == ']') { closed = true; break; }
                if (!t.back()) return false;
                state = OJS_AELEM;
                continue;
            }
            if (c == ']') { closed = true; break; }
            return false;                                                  // Expected a ',' or ']'
        }
        if (nested) {
            if (++depth > OJ_MAX_DEPTH) return false;
            open[depth] = v.a;
            role[depth] = nested;
            state = v.kind == OJV_OBJ ? OJS_KEY : OJS_AFIRST;
            continue;
        }
        if (closed) {
            const u8 r = role[depth];
            const int op = open[depth];
            if (--depth == 0) return (seen & require) == require;          // nothing after '}' is read
            if (r == OJR_KEY) {                                            // toString() of a container
                key = OjKey{OJK_RAW, op, t.p};
                kpos = op;
                kid = 0;
                state = OJS_COLON;
            } else {
                state = r == OJR_VALUE ? OJS_OSEP : OJS_ASEP;
            }
        }
    }
}

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
    Span sp[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) sp[k] = Span{0, 0, 0};
    if (!parse_line_all(src, s, e, require, sp)) return false;
    return row_of_spans(src, sp, r);
}

// Any .tbl row: readLine's terminator stripped, items = line.split("\\|") (MockWindowedFlatMap,
// :197-226).  items[0..5] lie between the first six '|' (the sixth, or the end of the line);
// items[5] exists iff it is not empty or a later item is not -- an empty one is no long either
// way, so the row is valid iff the five values are long enough and items[5] parses.
template <class S>
__device__ __noinline__ bool col_tbl_general(const S& src, int s, int e, ColRow& r) {
    if (e > s && src.b(e - 1) == '\n') --e;
    if (e > s && src.b(e - 1) == '\r') --e;
    int p[6];
    int k = 0;
    for (int q = s; q < e && k < 6; ++q)
        if (src.b(q) == '|') p[k++] = q;
    if (k < 5) return false;
    if (k == 5) p[5] = e;
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

struct ColTile {
    u64 first;     // first line
    u32 count;     // lines
    u32 s0;        // byte offset of the first line
    u32 delta;     // s0 - 16-byte aligned base
    u32 len;       // bytes staged from the aligned base (0: nothing)
    u32 e;         // end of the staged bytes
};

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

    // the tile's bounds (wave-uniform), then its bytes and line offsets HBM -> registers by
    // bounds-checked buffer loads, as the scan's issue_tile_loads reads them (chunks past the
    // staged bytes and offsets past the batch read zeros; the range is the tile rounded up
    // to 16 bytes, which never leaves the batch's last page)
    auto issue = [&](u64 t, ColTile& ti, uint4 (&pre)[CPT], u32& p_off, u32& p_end) {
        ti = ColTile{t * TILE_LINES, 0u, 0u, 0u, 0u, 0u};
        if (ti.first < P.n) {
            const u64 rem = P.n - ti.first;
            ti.count = rem < (u64)TILE_LINES ? (u32)rem : (u32)TILE_LINES;
            const u32 s0 = (u32)__builtin_amdgcn_readfirstlane((int)P.off[ti.first]);
            const u64 e = ti.first + ti.count < P.n
                              ? (u64)(u32)__builtin_amdgcn_readfirstlane((int)P.off[ti.first + ti.count])
                              : P.nbytes;
            ti.s0 = s0;
            ti.delta = s0 & 15u;   // P.bytes is 16-byte aligned
            if ((u64)s0 <= e && e <= P.nbytes) {
                const u64 len = e - s0 + ti.delta;
                ti.len = (u32)(len < (u64)G::CAP ? len : (u64)G::CAP);
            }
            ti.e = s0 - ti.delta + ti.len;
        }
        const u8* tbase = P.bytes + ((u64)ti.s0 - ti.delta);   // (len 0: nothing is read)
        const __amdgpu_buffer_rsrc_t rb =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<u8*>(tbase), 0, (int)((ti.len + 15u) & ~15u), 0x00020000);
#pragma unroll
        for (int j = 0; j < CPT; ++j) {
            const auto v = __builtin_amdgcn_raw_buffer_load_b128(rb, 16 * (j * SCAN_TPB + tid), 0, AUX_NT);
            pre[j] = make_uint4(v[0], v[1], v[2], v[3]);
        }
        const u64 f = ti.first < P.n ? ti.first : P.n;
        const u64 left = P.n - f;
        const u32 nrec = (u32)((u64)ti.count + 1u < left ? (u64)ti.count + 1u : left) * 4u;   // the last line's end included
        const __amdgpu_buffer_rsrc_t ro =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<u32*>(P.off + f), 0, (int)nrec, 0x00020000);
        p_off = __builtin_amdgcn_raw_buffer_load_b32(ro, 4 * tid, 0, 0);
        p_end = __builtin_amdgcn_raw_buffer_load_b32(ro, 4 * tid + 4, 0, 0);   // 0 past the batch end
    };

    ColTile cur;
    uint4 pre[CPT];
    u32 pre_off = 0, pre_end = 0;
    u64 t = blockIdx.x;
    if (t >= P.n_tiles) return;
    issue(t, cur, pre, pre_off, pre_end);
    for (; t < P.n_tiles; t += gridDim.x) {
        // ---- registers -> LDS (chunks past the staged bytes hold zeros) ----------------
#pragma unroll
        for (int j = 0; j < CPT; ++j) {
            const u32 k = (u32)(j * SCAN_TPB + tid);
            if (j * SCAN_TPB + SCAN_TPB <= G::CHUNKS || k < (u32)G::CHUNKS) reinterpret_cast<uint4*>(tile32)[k] = pre[j];
        }
        const ColTile ti = cur;
        __syncthreads();
        // ---- this lane's line ------------------------------------------------------------
        const u64 line = ti.first + (u32)tid;
        const bool active = (u32)tid < ti.count;
        const u32 my_off = pre_off;
        const u32 my_end = line + 1 < P.n ? pre_end : (u32)P.nbytes;
        // the next tile's bytes land while this one is parsed
        if (t + gridDim.x < P.n_tiles) issue(t + gridDim.x, cur, pre, pre_off, pre_end);
        const bool sane = active && my_off <= my_end && (u64)my_end <= P.nbytes && my_end - my_off <= 0x7FFFFFFFu;
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
        if (sane && !fast) {
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
