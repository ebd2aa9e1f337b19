// ysb_count_arrow.h -- Kernel 6: views counted straight from an Apache Arrow record batch
// (ysb_submit_arrow*, include/ysb_hip.h "Arrow record batches"; the row rule: ysb_arrow.h).
// Part of the scan kernel's translation unit: included at the end of ysb_scan.hip, behind
// ysb_count_columns.h, whose probe (cc_probe_issue / cc_probe_finish) it shares together with
// the scan's own span_is_view, span_key, parse_digits, parse_digits_regs, load_span, probe,
// key_hash_dev, count_miss, the count tail (cc_count_view), the LDS window, flush_tally and div_trunc.
//
// Shape, after colcount_kernel: one-wave workgroups, tiles of 64 rows, lane i takes row i.
// Rows are not at a fixed stride, so a tile is loaded in two dependent steps, both ahead of its
// turn.  A: per string column the tile's 65 offsets (aligned words i, 64 and 65 of the tile's
// offsets, realigned with v_alignbyte: the caller's pointers have any alignment), the bitmap
// byte of each lane's row, the int64 time or the dictionary index.  B, once A is there: the
// byte span [off[first], off[first + count]) of each string column -- contiguous -- with
// 16-byte bounds-checked loads from the dword-aligned address below its start, staged into LDS
// when the tile's turn comes; each lane then reads its own values from LDS through the scan's
// realigning readers.  Tile t's turn issues B of tile t + AC_PF * grid and A of tile
// t + 2 * AC_PF * grid between its probe's loads and their use.
//
// A tile goes through LDS only if every row's offsets obey the rule and each span fits its cap
// (AC_*_BYTES: 48 bytes of id, 16 of type and 16 of time per row on average; the generator's rows
// are 36, <= 8 and 13).  Any other tile takes the per-lane path (ar_lane_row): each lane loads
// its own row with bounds-checked dword loads.  Which path a tile takes is uniform across the
// wave.  Every access to a caller's buffer is a buffer load over that buffer's stated bytes
// widened to whole dwords, so an offset that lies is never followed (rule 2 rejects the row
// from the offsets alone) and a load past the rows returns zeros without touching memory.
#pragma once

#include "ysb_arrow.h"

namespace ysb {

constexpr int AC_KEY_BYTES = 3072, AC_TY_BYTES = 1024, AC_TM_BYTES = 1024;   // a tile's staged span, at most
constexpr int AC_SLACK = 64;   // a lane's realigned reads end within 60 bytes of its value's start
constexpr int AC_KEY_DW = 0;
constexpr int AC_TY_DW = AC_KEY_DW + (AC_KEY_BYTES + AC_SLACK) / 4;
constexpr int AC_TM_DW = AC_TY_DW + (AC_TY_BYTES + AC_SLACK) / 4;
constexpr int AC_STAGE_DW = AC_TM_DW + (AC_TM_BYTES + AC_SLACK) / 4;
constexpr int AC_KEY_CPT = AC_KEY_BYTES / 16 / SCAN_TPB;   // 16-byte chunks per lane: 3, 1, 1
constexpr int AC_LDS = AC_STAGE_DW * 4 + LCNT_CAP * 4 + 16;   // spans | window counters | rebase requests
#ifndef YSB_ARROWCOUNT_WG_PER_CU
#define YSB_ARROWCOUNT_WG_PER_CU 8
#endif
constexpr int AC_WG_PER_CU = YSB_ARROWCOUNT_WG_PER_CU;
constexpr int AC_PF = 2;   // tiles whose spans are in flight ahead of the one being probed
static_assert(AC_KEY_BYTES % (16 * SCAN_TPB) == 0 && AC_TY_BYTES == 16 * SCAN_TPB && AC_TM_BYTES == 16 * SCAN_TPB,
              "whole chunks per lane");
static_assert(AC_WG_PER_CU % 4 == 0, "whole waves per SIMD");
static_assert((AC_LDS + 1279) / 1280 * 1280 * AC_WG_PER_CU <= 163840, "the workgroups fit one CU's LDS");
static_assert(AC_TY_DW % 4 == 0 && AC_TM_DW % 4 == 0, "16-byte LDS stores");
static_assert(TILE_LINES == 64 && SCAN_TPB == 64, "lane i takes row i");

// A caller's buffer [p, p + bytes) as a byte source: a buffer resource from the dword-aligned
// address at or below p over the bytes widened to whole dwords.  Positions count from that
// address: byte x of the buffer is position lead + x.  Out-of-range dwords read as zero.
struct ArSrc {
    __amdgpu_buffer_rsrc_t r;
    __device__ __forceinline__ u32 dw(int p) const { return __builtin_amdgcn_raw_buffer_load_b32(r, p, 0, 0); }
    __device__ __forceinline__ u32 b(int p) const { return (dw(p & ~3) >> ((p & 3) << 3)) & 0xFFu; }
    __device__ __forceinline__ u32 load4(int p) const {
        const u32 lo = dw(p & ~3), hi = dw((p & ~3) + 4);
        return __builtin_amdgcn_alignbyte(hi, lo, (u32)(p & 3));
    }
};
__device__ __forceinline__ ArSrc ar_src(const u8* p, u32 bytes, u32& lead) {   // (p, bytes: wave-uniform)
    lead = (u32)(reinterpret_cast<u64>(p) & 3u);
    const u32 n = (p && bytes) ? (lead + bytes + 3u) & ~3u : 0u;
    return ArSrc{__builtin_amdgcn_make_buffer_rsrc(const_cast<u8*>(p) - lead, 0, (int)n, 0x00020000)};
}

// The bitmap byte that holds bit bit0 + i, i < cnt (bit0, cnt uniform); 0xFF without a bitmap.
__device__ __forceinline__ u32 ar_bit_byte(const u8* bm, u64 bit0, u32 cnt, u32 i) {
    if (!bm) return 0xFFu;
    const u32 sh = (u32)(bit0 & 7);
    u32 lead;
    const ArSrc s = ar_src(bm + (bit0 >> 3), cnt ? (sh + cnt + 7u) >> 3 : 0u, lead);
    return s.b((int)(lead + ((sh + i) >> 3)));
}

// What a row hands to the join: rule 2's verdict, rule 3's, the key in the tables' form
// (keyed: at most 56 bytes) and the time's parse outcome.
struct ArRow {
    u32 why;
    bool view, keyed, tok;
    u32 klen;
    i64 tv;
    u32 kw[KEY_WORDS];
};

// The launch's buffers that every tile reads through one resource.
struct ArBufs {
    ArSrc ad, ty, tm, doffs, dval;   // the three columns' string bytes; the dictionary's offsets and bitmap
    u32 lad, lty, ltm, ldoffs, ldval;
};
__device__ __forceinline__ void ar_bufs(const ArrowCountParams& C, ArBufs& B) {
    const int y = C.type_dict ? (int)AR_DICTV : (int)AR_TYPE;
    B.ad = ar_src(C.data[AR_AD], C.end[AR_AD] - C.first[AR_AD], B.lad);
    B.ty = ar_src(C.data[y], C.end[y] - C.first[y], B.lty);
    B.tm = ar_src(C.time_i64 ? nullptr : C.data[AR_TIME], C.end[AR_TIME] - C.first[AR_TIME], B.ltm);
    B.doffs = ar_src(C.type_dict ? C.offs[AR_DICTV] + 4 * C.elem[AR_DICTV] : nullptr, (C.dict_len + 1u) * 4u, B.ldoffs);
    B.dval = ar_src(C.type_dict && C.val[AR_DICTV] ? C.val[AR_DICTV] + (C.val_off[AR_DICTV] >> 3) : nullptr,
                    (u32)(((C.val_off[AR_DICTV] & 7) + C.dict_len + 7u) >> 3), B.ldval);
}

// A dictionary-encoded event_type: index -> the value's offsets in the dictionary's bytes (rule
// 2: the index's range, the value's bit, its offsets).  The dictionary is small: cache-resident.
__device__ __forceinline__ u32 ar_dict_value(const ArrowCountParams& C, const ArBufs& B, u32 idx, u32& y0, u32& y1) {
    if (!arrow_index_ok(idx, C.dict_len)) return AR_DICT;
    if (C.val[AR_DICTV]) {
        const u32 bit = (u32)(C.val_off[AR_DICTV] & 7) + idx;
        if (!arrow_bit(B.dval.b((int)(B.ldval + (bit >> 3))), bit)) return AR_NULL;
    }
    y0 = B.doffs.load4((int)(B.ldoffs + 4u * idx));
    y1 = B.doffs.load4((int)(B.ldoffs + 4u * idx + 4u));
    return arrow_span_ok(y0, y1, C.first[AR_DICTV], C.end[AR_DICTV]) ? (u32)AR_OK : (u32)AR_OFFSETS;
}

// The per-lane path: row row0 + i (i < cnt; row0, cnt uniform) by the lane's own loads alone.
__device__ __forceinline__ void ar_lane_row(const ArrowCountParams& C, const ArBufs& B, u64 row0, u32 cnt, u32 i, ArRow& o) {
    o.why = AR_OK;
    o.view = o.keyed = o.tok = false;
    o.klen = 0;
    o.tv = 0;
    u32 bits = ar_bit_byte(C.sval, C.sval_off + row0, cnt, i) >> ((C.sval_off + row0 + i) & 7);
#pragma unroll
    for (int c = 0; c < 3; ++c) bits &= ar_bit_byte(C.val[c], C.val_off[c] + row0, cnt, i) >> ((C.val_off[c] + row0 + i) & 7);
    if (!(bits & 1u)) o.why = AR_NULL;
    u32 off[3][2] = {{0, 0}, {0, 0}, {0, 0}};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if ((c == (int)AR_TYPE && C.type_dict) || (c == (int)AR_TIME && C.time_i64)) continue;
        u32 lead;
        const ArSrc s = ar_src(C.offs[c] + 4 * (C.elem[c] + row0), cnt ? (cnt + 1u) * 4u : 0u, lead);
        off[c][0] = s.load4((int)(lead + 4u * i));
        off[c][1] = s.load4((int)(lead + 4u * i + 4u));
    }
    if (C.type_dict) {
        u32 lead;
        const ArSrc s = ar_src(C.data[AR_TYPE] + 4 * (C.elem[AR_TYPE] + row0), cnt * 4u, lead);
        const u32 idx = s.load4((int)(lead + 4u * i));
        if (o.why == AR_OK) o.why = ar_dict_value(C, B, idx, off[AR_TYPE][0], off[AR_TYPE][1]);
    }
    const int y = C.type_dict ? (int)AR_DICTV : (int)AR_TYPE;
    if (o.why == AR_OK &&
        !(arrow_span_ok(off[AR_AD][0], off[AR_AD][1], C.first[AR_AD], C.end[AR_AD]) &&
          arrow_span_ok(off[AR_TYPE][0], off[AR_TYPE][1], C.first[y], C.end[y]) &&
          (C.time_i64 || arrow_span_ok(off[AR_TIME][0], off[AR_TIME][1], C.first[AR_TIME], C.end[AR_TIME]))))
        o.why = AR_OFFSETS;
    if (o.why != AR_OK || i >= cnt) return;
    const int py = (int)(B.lty + (off[AR_TYPE][0] - C.first[y]));
    o.view = span_is_view(B.ty, Span{py, py + (int)(off[AR_TYPE][1] - off[AR_TYPE][0]), 0});
    if (!o.view) return;
    const int pa = (int)(B.lad + (off[AR_AD][0] - C.first[AR_AD]));
    o.keyed = span_key(B.ad, Span{pa, pa + (int)(off[AR_AD][1] - off[AR_AD][0]), 0}, o.kw, o.klen);
    if (C.time_i64) {
        u32 lead;
        const ArSrc s = ar_src(C.data[AR_TIME] + 8 * (C.elem[AR_TIME] + row0), cnt * 8u, lead);
        const u32 t0 = s.load4((int)(lead + 8u * i)), t1 = s.load4((int)(lead + 8u * i + 4u));
        o.tv = (i64)(((u64)t1 << 32) | (u64)t0);
        o.tok = true;
    } else {
        const int pm = (int)(B.ltm + (off[AR_TIME][0] - C.first[AR_TIME]));
        o.tok = parse_digits(B.tm, pm, pm + (int)(off[AR_TIME][1] - off[AR_TIME][0]), o.tv);
    }
}

// ---- the staged path's two load steps -------------------------------------------------------
// A: what tells where a tile's bytes are (issued 2 * AC_PF tiles ahead).
struct ArTileA {
    u32 ad[3], ty[3], tm[3];   // a string column: aligned words tid, 64 and 65 of the tile's offsets;
                               // ty[0..1]: the index's aligned words; tm[0..2]: the int64 time's
    u32 vb;                    // the row's bit at struct level and in the three columns, ANDed (bit 0)
    u32 count;
};
// B: the tile's spans on their way HBM -> registers (issued AC_PF tiles ahead), and its rows.
struct ArTileB {
    uint4 k[AC_KEY_CPT], y, m;
    u32 kt, yt, mt;            // the dwords behind the whole chunks (lanes 0..2)
    u32 a0, a1, y0, y1, m0, m1;   // the row's offsets (y0: a dictionary index; m0, m1: an int64 time)
    bool nul;
    u32 count;
    bool staged;               // uniform
    u32 nda, ndy, ndm;         // uniform: dwords staged per column
    u32 pa, py, pm;            // uniform: LDS byte position of offset 0 (position of o: p + o, mod 2^32)
};

__device__ __forceinline__ void ar_issue_offs(const u8* offs, u64 elem0, u32 count, int tid, u32 (&w)[3]) {
    u32 lead;
    const ArSrc s = ar_src(offs + 4 * elem0, count ? (count + 1u) * 4u : 0u, lead);
    w[0] = __builtin_amdgcn_raw_buffer_load_b32(s.r, 4 * tid, 0, AUX_NT);
    w[1] = __builtin_amdgcn_raw_buffer_load_b32(s.r, 4 * 64, 0, AUX_NT);
    w[2] = __builtin_amdgcn_raw_buffer_load_b32(s.r, 4 * 65, 0, AUX_NT);
}

// Tile t's step A.  t >= n_tiles: nothing is read.
__device__ __forceinline__ void ar_issue_a(const ArrowCountParams& C, u64 t, int tid, ArTileA& o) {
    const bool live = t < C.n_tiles;
    const u64 first = live ? t * (u64)TILE_LINES : 0;
    const u64 rem = C.n_rows - first;
    const u32 count = !live ? 0u : rem < (u64)TILE_LINES ? (u32)rem : (u32)TILE_LINES;
    o.count = count;
    ar_issue_offs(C.offs[AR_AD], C.elem[AR_AD] + first, count, tid, o.ad);
    if (C.type_dict) {
        u32 lead;
        const ArSrc s = ar_src(C.data[AR_TYPE] + 4 * (C.elem[AR_TYPE] + first), count * 4u, lead);
        o.ty[0] = s.dw(4 * tid);
        o.ty[1] = s.dw(4 * tid + 4);
        o.ty[2] = 0;
    } else {
        ar_issue_offs(C.offs[AR_TYPE], C.elem[AR_TYPE] + first, count, tid, o.ty);
    }
    if (C.time_i64) {
        u32 lead;
        const ArSrc s = ar_src(C.data[AR_TIME] + 8 * (C.elem[AR_TIME] + first), count * 8u, lead);
        o.tm[0] = s.dw(8 * tid);
        o.tm[1] = s.dw(8 * tid + 4);
        o.tm[2] = s.dw(8 * tid + 8);
    } else {
        ar_issue_offs(C.offs[AR_TIME], C.elem[AR_TIME] + first, count, tid, o.tm);
    }
    u32 bits = ar_bit_byte(C.sval, C.sval_off + first, count, (u32)tid) >> ((C.sval_off + first + (u64)tid) & 7);
#pragma unroll
    for (int c = 0; c < 3; ++c)
        bits &= ar_bit_byte(C.val[c], C.val_off[c] + first, count, (u32)tid) >> ((C.val_off[c] + first + (u64)tid) & 7);
    o.vb = bits;
}

// the lane's offsets off[tid], off[tid + 1] from step A's aligned words
__device__ __forceinline__ void ar_offs_of(const u8* offs, const u32 (&w)[3], int tid, u32& o0, u32& o1) {
    const u32 lead = (u32)(reinterpret_cast<u64>(offs) & 3u);
    const u32 nx = __shfl_down(w[0], 1, 64);
    o0 = __builtin_amdgcn_alignbyte(tid == 63 ? w[1] : nx, w[0], lead);
    const u32 n0 = __shfl_down(o0, 1, 64);
    o1 = tid == 63 ? __builtin_amdgcn_alignbyte(w[2], w[1], lead) : n0;
}

// A string column's span [s, e) of a staged tile: CPT whole 16-byte chunks per lane from the
// dword-aligned address below its start, the up to three dwords behind them by lanes 0..2.
// go false (or an empty span): nothing is read.  nd <- the dwords staged, p0 <- the LDS byte
// position of offset 0 when the span is staged at dword `at`.
template <int CPT>
__device__ __forceinline__ void ar_issue_span(const u8* data, u32 first, u32 s, u32 e, bool go, int at, int tid,
                                              uint4 (&k)[CPT], u32& tail, u32& nd, u32& p0) {
    const u8* addr = data + (s - first);
    const u32 l = (u32)(reinterpret_cast<u64>(addr) & 3u);
    nd = (go && e > s) ? (l + (e - s) + 3u) >> 2 : 0u;
    const u32 whole = (nd * 4u) & ~15u;
    p0 = (u32)at * 4u + l - s;
    const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc(const_cast<u8*>(addr) - l, 0, (int)whole, 0x00020000);
    const __amdgpu_buffer_rsrc_t rt = __builtin_amdgcn_make_buffer_rsrc(const_cast<u8*>(addr) - l, 0, (int)(nd * 4u), 0x00020000);
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
        const auto v = __builtin_amdgcn_raw_buffer_load_b128(rk, 16 * (j * SCAN_TPB + tid), 0, AUX_NT);
        k[j] = make_uint4(v[0], v[1], v[2], v[3]);
    }
    tail = __builtin_amdgcn_raw_buffer_load_b32(rt, (int)whole + 4 * tid, 0, AUX_NT);
}

// Step B of the tile whose step A is in `a`: the rows' offsets, the verdict staged / per-lane,
// and a staged tile's span loads.
__device__ __forceinline__ void ar_issue_b(const ArrowCountParams& C, const ArTileA& a, int tid, ArTileB& o) {
    const u32 count = a.count;
    o.count = count;
    o.nul = !(a.vb & 1u);
    ar_offs_of(C.offs[AR_AD], a.ad, tid, o.a0, o.a1);
    bool ok = arrow_span_ok(o.a0, o.a1, C.first[AR_AD], C.end[AR_AD]);
    if (C.type_dict) {
        o.y0 = __builtin_amdgcn_alignbyte(a.ty[1], a.ty[0], (u32)(reinterpret_cast<u64>(C.data[AR_TYPE]) & 3u));
        o.y1 = 0;
    } else {
        ar_offs_of(C.offs[AR_TYPE], a.ty, tid, o.y0, o.y1);
        ok = ok && arrow_span_ok(o.y0, o.y1, C.first[AR_TYPE], C.end[AR_TYPE]);
    }
    if (C.time_i64) {
        const u32 lead = (u32)(reinterpret_cast<u64>(C.data[AR_TIME]) & 3u);
        o.m0 = __builtin_amdgcn_alignbyte(a.tm[1], a.tm[0], lead);
        o.m1 = __builtin_amdgcn_alignbyte(a.tm[2], a.tm[1], lead);
    } else {
        ar_offs_of(C.offs[AR_TIME], a.tm, tid, o.m0, o.m1);
        ok = ok && arrow_span_ok(o.m0, o.m1, C.first[AR_TIME], C.end[AR_TIME]);
    }
    bool staged = count > 0 && __ballot(!ok && (u32)tid < count) == 0ull;
    const int last = count ? (int)count - 1 : 0;
    const u32 sa = __builtin_amdgcn_readfirstlane(o.a0), ea = __builtin_amdgcn_readfirstlane(__shfl(o.a1, last, 64));
    const u32 sy = __builtin_amdgcn_readfirstlane(o.y0), ey = __builtin_amdgcn_readfirstlane(__shfl(o.y1, last, 64));
    const u32 sm = __builtin_amdgcn_readfirstlane(o.m0), em = __builtin_amdgcn_readfirstlane(__shfl(o.m1, last, 64));
    // (a span's dwords: its bytes plus the up to three in front of it in its first dword)
    staged = staged && (ea - sa) + 3u <= (u32)AC_KEY_BYTES - 4u;
    if (!C.type_dict) staged = staged && (ey - sy) + 3u <= (u32)AC_TY_BYTES - 4u;
    if (!C.time_i64) staged = staged && (em - sm) + 3u <= (u32)AC_TM_BYTES - 4u;
    o.staged = staged;
    ar_issue_span<AC_KEY_CPT>(C.data[AR_AD], C.first[AR_AD], sa, ea, staged, AC_KEY_DW, tid, o.k, o.kt, o.nda, o.pa);
    uint4 y1[1], m1[1];
    ar_issue_span<1>(C.data[AR_TYPE], C.first[AR_TYPE], sy, ey, staged && !C.type_dict, AC_TY_DW, tid, y1, o.yt, o.ndy, o.py);
    ar_issue_span<1>(C.data[AR_TIME], C.first[AR_TIME], sm, em, staged && !C.time_i64, AC_TM_DW, tid, m1, o.mt, o.ndm, o.pm);
    o.y = y1[0];
    o.m = m1[0];
}

// registers -> LDS: a staged span's chunks (those past the span hold zeros) and tail dwords
template <int CPT>
__device__ __forceinline__ void ar_stage(u32* stage, int at, const uint4 (&k)[CPT], u32 tail, u32 nd, int tid) {
#pragma unroll
    for (int j = 0; j < CPT; ++j) reinterpret_cast<uint4*>(stage + at)[j * SCAN_TPB + tid] = k[j];
    const u32 whole_dw = nd & ~3u;
    if ((u32)tid < nd - whole_dw) stage[at + (int)whole_dw + tid] = tail;   // (after the zero chunk above)
}

template <bool SERIAL, bool PARK>
__global__ __launch_bounds__(SCAN_TPB) __attribute__((amdgpu_waves_per_eu(AC_WG_PER_CU / 4)))
void arrowcount_kernel(const ArrowCountParams C, const ParkParams K) {
    const ScanParams& P = C.sp;
    __shared__ __attribute__((aligned(16))) u32 stage[AC_STAGE_DW];
    __shared__ u32 lcnt[LCNT_CAP];
    __shared__ i64 req64[2];   // the LDS window's move requests
    const int tid = threadIdx.x;
    u64 t = blockIdx.x;
    if (t >= C.n_tiles) return;

    LdsWindow win(P, lcnt, req64);
    win.init();
    Tally tl{0, 0, 0, 0, 0, 0, 0, 0};
    u32 inv_null = 0, inv_offs = 0, inv_dict = 0, lane_tiles = 0;
    ArBufs B;
    ar_bufs(C, B);
    const LdsSrc lds{stage};

    auto tile_step = [&](u64 t, ArTileA& nxt, ArTileB& cur) {
        // ---- registers -> LDS: the tile's spans ---------------------------------------------
        const u32 count = cur.count;
        const bool staged = cur.staged, nul = cur.nul;
        const u32 a0 = cur.a0, a1 = cur.a1, y0 = cur.y0, y1 = cur.y1, m0 = cur.m0, m1 = cur.m1;
        const u32 pa = cur.pa, py = cur.py, pm = cur.pm;
        if (staged) {
            ar_stage<AC_KEY_CPT>(stage, AC_KEY_DW, cur.k, cur.kt, cur.nda, tid);
            if (!C.type_dict) { const uint4 v[1] = {cur.y}; ar_stage<1>(stage, AC_TY_DW, v, cur.yt, cur.ndy, tid); }
            if (!C.time_i64) { const uint4 v[1] = {cur.m}; ar_stage<1>(stage, AC_TM_DW, v, cur.mt, cur.ndm, tid); }
        }
        const int par = win.before_barrier(P, tl);
        __syncthreads();
        win.after_barrier(par);
        // ---- rules 2 and 3, the key, the time -------------------------------------------------
        const bool active = (u32)tid < count;
        ArRow r;
        r.why = AR_OK;
        r.view = r.keyed = r.tok = false;
        r.klen = 0;
        r.tv = 0;
#pragma unroll
        for (int k = 0; k < (int)KEY_WORDS; ++k) r.kw[k] = 0u;
        if (staged) {
            u32 ys = y0, ye = y1;
            if (nul) r.why = AR_NULL;
            else if (C.type_dict) r.why = ar_dict_value(C, B, y0, ys, ye);
            if (active && r.why == AR_OK) {
                if (C.type_dict) {
                    const int p = (int)(B.lty + (ys - C.first[AR_DICTV]));
                    r.view = span_is_view(B.ty, Span{p, p + (int)(ye - ys), 0});
                } else {
                    r.view = span_is_view(lds, Span{(int)(py + ys), (int)(py + ye), 0});
                }
            }
            if (r.view) {
                r.keyed = span_key(lds, Span{(int)(pa + a0), (int)(pa + a1), 0}, r.kw, r.klen);
                if (C.time_i64) {
                    r.tv = (i64)(((u64)m1 << 32) | (u64)m0);
                    r.tok = true;
                } else {
                    const int ps = (int)(pm + m0), len = (int)(m1 - m0);
                    if (len <= 20) {
                        u32 td[5];
                        load_span(lds, ps, td);
                        r.tok = parse_digits_regs(td, len, r.tv);
                    } else {
                        r.tok = parse_digits(lds, ps, ps + len, r.tv);
                    }
                }
            }
        } else {
            ar_lane_row(C, B, t * (u64)TILE_LINES, count, (u32)tid, r);
            lane_tiles += count ? 1u : 0u;
        }
        const bool bad = active && r.why != AR_OK;
        const bool view = active && r.why == AR_OK && r.view;
        inv_null += (bad && r.why == AR_NULL) ? 1u : 0u;
        inv_offs += (bad && r.why == AR_OFFSETS) ? 1u : 0u;
        inv_dict += (bad && r.why == AR_DICT) ? 1u : 0u;
        tl.ev += active ? 1u : 0u;
        tl.perr += bad ? 1u : 0u;   // the row the reference would have thrown on
        tl.view += view ? 1u : 0u;
        const bool k36 = view && r.keyed && r.klen == 36u;
        ColProbe<SERIAL> pr;
#pragma unroll
        for (int j = 0; j < (int)(sizeof(pr.q) / sizeof(pr.q[0])); ++j) pr.q[j] = make_uint4(0, 0, 0, 0);
        pr.ib = 0;
        if (k36) {
            u32 k9[CKEY_WORDS];
#pragma unroll
            for (int k = 0; k < (int)CKEY_WORDS; ++k) k9[k] = r.kw[k];
            cc_probe_issue<SERIAL>(P, k9, pr);
        }
        // ---- the tiles ahead: B of the next one of this slot, A of the one after ----------------
        ar_issue_b(C, nxt, tid, cur);
        ar_issue_a(C, t + 2ull * AC_PF * gridDim.x, tid, nxt);
        // ---- join result, bucket, count ------------------------------------------------------
        ParkLane pl;
        pl.want = false;
        if (view) {
            u32 ci = EMPTY_SLOT;
            if (k36) {
                ci = cc_probe_finish<SERIAL>(P, r.kw, pr);
            } else if (r.keyed) {
                const int c = probe(P.table, P.table_mask, r.kw, r.klen);
                if (c >= 0) ci = (u32)c;
            }
            cc_count_view<PARK>(P, win, par, ci, r.keyed, r.kw, r.klen, r.tok, r.tv, tl, pl);
        }
        if constexpr (PARK) park_append(K, pl, tl);
        __syncthreads();   // the tile's spans are read and its counts are in before the next one
    };
    ArTileA ta[AC_PF];
    ArTileB tb[AC_PF];
#pragma unroll
    for (int k = 0; k < AC_PF; ++k) ar_issue_a(C, t + (u64)k * gridDim.x, tid, ta[k]);
#pragma unroll
    for (int k = 0; k < AC_PF; ++k) {
        ar_issue_b(C, ta[k], tid, tb[k]);
        ar_issue_a(C, t + (u64)(k + AC_PF) * gridDim.x, tid, ta[k]);
    }
    for (; t < C.n_tiles; t += (u64)AC_PF * gridDim.x) {
#pragma unroll
        for (int k = 0; k < AC_PF; ++k) {
            const u64 tk = t + (u64)k * gridDim.x;
            if (tk >= C.n_tiles) break;
            tile_step(tk, ta[k], tb[k]);
        }
    }
    win.finish(P, tl);
    flush_tally(P, tl, tid);
    const u32 sums[3] = {wave_sum(inv_null), wave_sum(inv_offs), wave_sum(inv_dict)};
    if (tid == 0) {
        if (lane_tiles) atomicAdd(&C.info[0], (unsigned long long)lane_tiles);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (sums[k]) atomicAdd(&C.info[1 + k], (unsigned long long)sums[k]);
    }
}

// Ring auto-base, the Arrow form of colcount_autobase_kernel: the smallest bucket among the
// counted views of rows [0, min(n_rows, 256)) fixes the ring at that bucket - W / 8.
template <bool SERIAL>
__global__ __launch_bounds__(AUX_TPB) void arrowcount_autobase_kernel(const ArrowCountParams C, i64* ring) {
    const ScanParams& P = C.sp;
    if (ring[1] != 0) return;
    const int tid = threadIdx.x;
    const u32 cnt = C.n_rows < (u64)AUX_TPB ? (u32)C.n_rows : (u32)AUX_TPB;
    i64 b = INT64_MAX;
    ArBufs B;
    ar_bufs(C, B);
    ArRow r;
#pragma unroll
    for (int k = 0; k < (int)KEY_WORDS; ++k) r.kw[k] = 0u;
    ar_lane_row(C, B, 0, cnt, (u32)tid, r);
    if ((u32)tid < cnt && r.why == AR_OK && r.view && r.keyed && r.tok) {
        u32 ci = EMPTY_SLOT;
        if (r.klen == 36u) {
            u32 k9[CKEY_WORDS];
#pragma unroll
            for (int k = 0; k < (int)CKEY_WORDS; ++k) k9[k] = r.kw[k];
            ColProbe<SERIAL> pr;
            cc_probe_issue<SERIAL>(P, k9, pr);
            ci = cc_probe_finish<SERIAL>(P, r.kw, pr);
        } else {
            const int c = probe(P.table, P.table_mask, r.kw, r.klen);
            if (c >= 0) ci = (u32)c;
        }
        if (ci != EMPTY_SLOT) b = div_trunc(r.tv, P.div);
    }
    commit_ring_base(b, ring, P.ring_w);
}

u32 arrowcount_resident_grid(int cus) { return (u32)(cus > 0 ? cus : 1) * (u32)AC_WG_PER_CU; }

void launch_arrowcount(const ArrowCountParams& p, int cus, hipStream_t s, const ParkParams* park) {
    if (p.n_rows == 0) return;
    const dim3 g = count_grid(p.n_tiles, arrowcount_resident_grid(cus));
    launch_serial_park(p.sp.probe_serial, park, [&](auto serial, auto parked) {
        hipLaunchKernelGGL((arrowcount_kernel<decltype(serial)::value, decltype(parked)::value>), g, dim3(SCAN_TPB), 0, s, p,
                           park ? *park : ParkParams{});
    });
}

void launch_arrowcount_autobase(const ArrowCountParams& p, hipStream_t s) {
    if (p.n_rows == 0) return;
    const dim3 g(1), b(AUX_TPB);
    i64* ring = const_cast<i64*>(p.sp.ring);
    if (p.sp.probe_serial) hipLaunchKernelGGL(arrowcount_autobase_kernel<true>, g, b, 0, s, p, ring);
    else hipLaunchKernelGGL(arrowcount_autobase_kernel<false>, g, b, 0, s, p, ring);
}

}  // namespace ysb
