// ysb_lz4.hip -- LZ4 batches decoded on the GPU (ysb_submit_raw_lz4, ysb_lz4_decode_device;
// the format, its ONE sequence reader and the host model: ysb_lz4.h).  This is the codec a
// source otherwise runs on a CPU in front of FileBasedDataSource.run
// (AdvertisingTopologyNative.java:144-165) or inside a Kafka consumer: here the compressed
// blocks cross PCIe and are decoded where the lines are split and scanned.
//
// Two decode kernels, picked by the batch's largest block (launch_lz4_decode): the one described
// here for blocks up to 16 KiB, and for larger ones a pipeline of four waves per block
// (lz4_decode_wide_kernel, below).  Behind them the standard frames' measure pass and
// descriptor scan (ysb_lz4_frame.h).
//
// One wave per block, one block per workgroup; the batch's parallelism is across its blocks.
// A block's sequences are walked serially by the whole wave: every position and length is
// wave-uniform (the reader's bytes come out of a 64-byte register window through readlane),
// the copies are lane-parallel.
//
// The block is decoded IN LDS, not in global memory: a match reads bytes that the same wave
// has just written, often a few bytes back, and LDS gives that a defined order (a wave's LDS
// instructions complete in issue order; __syncthreads() -- a wave barrier plus the LDS wait in
// a one-wave workgroup -- stands between every write and a read that may see it), at LDS
// latency per sequence instead of a global round trip.  The window holds the output from its
// start and the compressed bytes at its end (in place: ysb_lz4.h lz4_margin says why the write
// front never reaches the read front for a block the reader accepts; both checks are made
// anyway and make the block bad).  The launch sizes the window for the batch's largest block,
// so small blocks keep many waves per CU (of 160 KiB LDS: 8 KiB blocks 19, 16 KiB blocks 9,
// 64 KiB blocks 2) -- the kernel's time is per-sequence latency, so its rate follows that
// number (DESIGN.md, LZ4 batches: why the tools default to 8 KiB blocks).
//
// Global memory is touched at the two ends only.  In: the block's compressed bytes, 16-byte
// vector loads between the first and last 16-byte boundary INSIDE [in, in + comp) and single
// bytes at the edges, so nothing past comp_bytes is read (the batch's last block may end where
// the allocation ends).  Out: the same shape with stores, so no dword or vector that a
// neighbouring block's wave may store into is ever read-modify-written -- a block's output
// starts and ends at any byte address.  A bad block stores nothing at all and records its
// index; a stored block is copied byte by byte.
#include "ysb_kernels.h"
#include "ysb_lz4.h"
#include "ysb_lz4_frame.h"
#include "ysb_lz4_device.h"

namespace ysb {

// The reader's input: the compressed bytes in LDS at lds[base + pos], 64 at a time in one
// register per lane.  byte() is wave-uniform: pos is, and readlane broadcasts one lane's byte.
struct Lz4WaveIn {
    const u8* lds;
    u32 base, comp, lane;
    u32 win_pos, win;
    __device__ __forceinline__ u32 byte(u32 pos) {
        if (pos - win_pos >= 64u) {   // (win_pos starts at 2^31: no pos is within 64 of it)
            win_pos = pos;
            const u32 i = pos + lane;
            win = lds[base + (i < comp ? i : comp - 1)];
        }
        return (u32)__builtin_amdgcn_readlane((int)win, (int)(pos - win_pos));
    }
};

__global__ __launch_bounds__(LZ4_TPB) void lz4_decode_kernel(const Lz4Params P) {
    extern __shared__ __align__(16) u8 lz4_lds[];
    u8* lds = lz4_lds;
    const u32 lane = threadIdx.x;
    const Lz4Desc d = P.desc[blockIdx.x];
    const ysb_lz4_block e{d.comp, d.raw};
    const u32 comp = lz4_entry_comp(e), raw = d.raw;
    const u8* gin = P.in + d.in_off;
    u8* gout = P.out + d.out_off;
    if (P.skip_above && raw > P.skip_above) return;   // (the whole workgroup: the other launch's block)
    if (d.comp & P.skip_tag) return;                  // (... or another codec's: ysb_snappy.hip)
    // (the host has checked every entry: lz4_check_dir; a launch sized for max_raw must not
    // meet a larger block all the same)
    bool bad = !lz4_entry_ok(e) || raw > P.max_raw;
    if (!bad && (d.comp & LZ4_STORED)) {
        bad = !lz4_stored_ok(e);
        if (!bad)
            for (u32 j = lane; j < raw; j += LZ4_TPB) gout[j] = gin[j];
    } else if (!bad) {
        const u32 W = lz4_window(raw);
        bad = comp > W;
        if (!bad) {
            // output byte i at lds[ob + i], input byte j at lds[ib + j]; ob and ib congruent to
            // the global addresses mod 16; ib - ob >= W - comp; ib + comp <= 31 + W
            const u32 ob = (u32)(reinterpret_cast<uintptr_t>(gout) & 15);
            u32 ib = 16 + W - comp;
            ib += ((u32)(reinterpret_cast<uintptr_t>(gin) & 15) - ib) & 15;
            lz4_move<true>(lds, ib, const_cast<u8*>(gin), comp, lane);
            __syncthreads();
            Lz4WaveIn in{lds, ib, comp, lane, 0x80000000u, 0u};
            u32 ip = 0, op = 0;
            for (;;) {
                Lz4Seq s;
                const u32 r = lz4_read_seq(in, ip, comp, op, raw, &s);
                if (r == LZ4_SEQ_BAD) { bad = true; break; }
                // the literals, forwards: in place as long as the write front is not ahead
                if (ob + op > ib + s.lit_pos) { bad = true; break; }
                for (u32 at = 0; at < s.lit_len; at += LZ4_TPB) {
                    const u32 k = at + lane;
                    u8 b = 0;
                    if (k < s.lit_len) b = lds[ib + s.lit_pos + k];
                    if (k < s.lit_len) lds[ob + op + k] = b;
                }
                op += s.lit_len;
                if (r == LZ4_SEQ_LAST) break;
                // the match must not overwrite input that is still to be read
                if (ob + op + s.match_len > ib + s.next) { bad = true; break; }
                __syncthreads();   // the literals just written may be the match's source
                const u32 dst = ob + op, src = dst - s.offset;
                if (s.offset >= LZ4_TPB || s.match_len <= s.offset) {
                    // 64 bytes at a time: a chunk's source lies wholly behind the chunk (the
                    // offset is at least a chunk, or the match does not overlap itself)
                    for (u32 at = 0; at < s.match_len; at += LZ4_TPB) {
                        const u32 k = at + lane;
                        if (k < s.match_len) lds[dst + k] = lds[src + k];
                        __syncthreads();   // the next chunk may read this one
                    }
                } else {
                    // an overlapping match replicates the `offset` bytes before it:
                    // dst[k] = src[k % offset], every source byte written before the match
                    u32 m = lane % s.offset;
                    const u32 step = LZ4_TPB % s.offset;
                    for (u32 at = 0; at < s.match_len; at += LZ4_TPB) {
                        const u32 k = at + lane;
                        if (k < s.match_len) lds[dst + k] = lds[src + m];
                        m += step;
                        if (m >= s.offset) m -= s.offset;
                    }
                    __syncthreads();
                }
                op += s.match_len;
                ip = s.next;
            }
            if (!bad) {
                __syncthreads();
                lz4_move<false>(lds, ob, gout, raw, lane);
            }
        }
    }
    if (bad && lane == 0) {
        atomicMin(&P.bad[0], blockIdx.x);
        atomicAdd(&P.bad[1], 1u);
        if (P.block_bad) P.block_bad[blockIdx.x] = 1u;
    }
}

// ---- the several-wave decoder: large blocks ------------------------------------------------
// At 64 KiB the one-wave kernel keeps two waves per CU, and each pays its LDS round trips and
// barriers per sequence with nothing to hide them behind.  Here a workgroup of four waves
// decodes a block as a three-stage pipeline over batches of LZ4W_BATCH sequences, one
// __syncthreads() per stage:
//   wave 0     parses batch s into records in LDS (the same lz4_read_seq; its bytes stream from
//              global memory through a prefetched register window: Lz4GlobalIn);
//   waves 2, 3 copy the literals of batch s - 1 from global memory into the output block in LDS,
//              in any order: they read input only, and no earlier match reads their destination;
//   wave 1     runs the matches of batch s - 2 in sequence order.  Their sources are literals
//              of batches <= s - 2 (complete one barrier ago) and earlier matches, which this
//              same wave wrote: a wave's LDS instructions complete in issue order, and
//              lz4_wave_sync() keeps the compiler from moving a read above the write it may see.
// So the block's time is the slower of the parse and the match chain instead of their sum plus
// the literals.  Every wave runs every stage's barrier: the stage count is not known ahead, so
// the "this was the last batch" flag is read from LDS (fin[], written two stages before it is
// read, overwritten one stage after), as is the parser's verdict (stop[], read behind the
// barrier of the stage that wrote it, overwritten three stages later).  The
// in-place trick does not carry over -- the input is not in LDS --, so the window is the output
// block alone: two workgroups per CU at 64 KiB.  Every LDS index is ob + an output position
// below raw, by the reader's checks; a bad block leaves the loop before anything is stored.
constexpr u32 LZ4W_TPB = 256;

__global__ __launch_bounds__(LZ4W_TPB) void lz4_decode_wide_kernel(const Lz4Params P) {
    extern __shared__ __align__(16) u8 lz4_lds[];
    u8* lds = lz4_lds;
    const u32 tid = threadIdx.x, lane = tid & 63;
    const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const Lz4Desc d = P.desc[blockIdx.x];
    const ysb_lz4_block e{d.comp, d.raw};
    const u32 comp = lz4_entry_comp(e), raw = d.raw;
    const u8* gin = P.in + d.in_off;
    u8* gout = P.out + d.out_off;
    if (P.skip_upto && raw <= P.skip_upto) return;   // (the whole workgroup: the other launch's block)
    if (d.comp & P.skip_tag) return;                 // (... or another codec's: ysb_snappy.hip)
    bool bad = !lz4_entry_ok(e) || raw > P.max_raw;
    if (!bad && (d.comp & LZ4_STORED)) {
        bad = !lz4_stored_ok(e);
        if (!bad)
            for (u32 j = tid; j < raw; j += LZ4W_TPB) gout[j] = gin[j];
    } else if (!bad && comp == 0) {
        bad = true;
    } else if (!bad) {
        const u32 ob = (u32)(reinterpret_cast<uintptr_t>(gout) & 15);   // output byte i at lds[ob + i]
        u32* rec = reinterpret_cast<u32*>(lds + lz4_wide_out_bytes(P.max_raw));   // [3][LZ4W_FIELDS][LZ4W_BATCH]
        u32* cnt = rec + 3 * LZ4W_FIELDS * LZ4W_BATCH;   // [3] records of a batch
        u32* fin = cnt + 3;                              // [3] the batch holds the block's last sequence
        u32* stop = cnt + 6;                             // [3] the parser met a bad sequence in the batch
        if (tid < 9) cnt[tid] = 0;
        __syncthreads();
        Lz4GlobalIn in;
        if (wave == 0) in.init(gin, comp, lane);
        u32 ip = 0, op = 0;
        bool parsed = false;   // (wave 0) the last or a bad sequence has been read
        for (u32 s = 0;; ++s) {
            const u32 b0 = s % 3, b1 = (s + 2) % 3, b2 = (s + 1) % 3;   // the buffers of batches s, s - 1, s - 2
            const u32 last = s >= 2 ? fin[b2] : 0u;   // read BEFORE this stage's barrier: wave 0 rewrites it behind it
            if (wave == 0) {
                u32 n = 0, f = 0, pbad = 0;
                u32 r_lp = 0, r_ll = 0, r_op = 0, r_off = 0, r_ml = 0;   // lane i: record i
                while (!parsed && n < LZ4W_BATCH) {
                    Lz4Seq q;
                    const u32 r = lz4_read_seq(in, ip, comp, op, raw, &q);
                    if (r == LZ4_SEQ_BAD) { pbad = 1; break; }
                    if (lane == n) { r_lp = q.lit_pos; r_ll = q.lit_len; r_op = op; r_off = q.offset; r_ml = q.match_len; }
                    ++n;
                    op += q.lit_len;
                    if (r == LZ4_SEQ_LAST) { f = 1; break; }
                    op += q.match_len;
                    ip = q.next;
                }
                parsed = parsed || f || pbad;
                u32* R = rec + b0 * LZ4W_FIELDS * LZ4W_BATCH;
                if (lane < n) {
                    R[0 * LZ4W_BATCH + lane] = r_lp;
                    R[1 * LZ4W_BATCH + lane] = r_ll;
                    R[2 * LZ4W_BATCH + lane] = r_op;
                    R[3 * LZ4W_BATCH + lane] = r_off;
                    R[4 * LZ4W_BATCH + lane] = r_ml;
                }
                if (lane == 0) {
                    cnt[b0] = n;
                    fin[b0] = f;
                    stop[b0] = pbad;
                }
            } else if (wave == 1) {
                if (s >= 2) {
                    const u32* R = rec + b2 * LZ4W_FIELDS * LZ4W_BATCH;
                    const u32 n = cnt[b2];
                    u32 v_at = 0, v_off = 0, v_ml = 0;
                    if (lane < n) {
                        v_at = ob + R[2 * LZ4W_BATCH + lane] + R[1 * LZ4W_BATCH + lane];   // behind the literals
                        v_off = R[3 * LZ4W_BATCH + lane];
                        v_ml = R[4 * LZ4W_BATCH + lane];
                    }
                    for (u32 i = 0; i < n; ++i) {
                        const u32 ml = (u32)__builtin_amdgcn_readlane((int)v_ml, (int)i);
                        if (!ml) continue;   // the last sequence has no match
                        const u32 off = (u32)__builtin_amdgcn_readlane((int)v_off, (int)i);
                        const u32 dst = (u32)__builtin_amdgcn_readlane((int)v_at, (int)i), src = dst - off;
                        if (off >= 64u || ml <= off) {
                            // 64 bytes at a time: a chunk's source lies wholly behind the chunk
                            for (u32 at = 0; at < ml; at += 64u) {
                                const u32 k = at + lane;
                                if (k < ml) lds[dst + k] = lds[src + k];
                                lz4_wave_sync();   // the next chunk, or the next match, may read this one
                            }
                        } else {
                            // an overlapping match replicates the `off` bytes before it
                            u32 m = lane % off;
                            const u32 step = 64u % off;
                            for (u32 at = 0; at < ml; at += 64u) {
                                const u32 k = at + lane;
                                if (k < ml) lds[dst + k] = lds[src + m];
                                m += step;
                                if (m >= off) m -= off;
                            }
                            lz4_wave_sync();
                        }
                    }
                }
            } else if (s >= 1) {
                const u32* R = rec + b1 * LZ4W_FIELDS * LZ4W_BATCH;
                const u32 n = cnt[b1], t = tid - 128u;   // 128 threads
                // short runs: eight lanes per record, sixteen records at a time
                for (u32 i = t / 8; i < n; i += 16) {
                    const u32 ll = R[1 * LZ4W_BATCH + i];
                    if (ll <= 32u) {
                        const u32 lp = R[0 * LZ4W_BATCH + i], o = ob + R[2 * LZ4W_BATCH + i];
                        for (u32 k = t & 7; k < ll; k += 8) lds[o + k] = gin[lp + k];
                    }
                }
                // long runs: all 128 lanes on one record after the other
                const u32 my_ll = lane < n ? R[1 * LZ4W_BATCH + lane] : 0u;
                for (unsigned long long m = __ballot(my_ll > 32u); m; m &= m - 1) {
                    const u32 i = (u32)__builtin_ctzll(m);
                    const u32 ll = R[1 * LZ4W_BATCH + i], lp = R[0 * LZ4W_BATCH + i], o = ob + R[2 * LZ4W_BATCH + i];
                    for (u32 k = t; k < ll; k += 128u) lds[o + k] = gin[lp + k];
                }
            }
            __syncthreads();
            // (this stage's words: wave 0, at most one stage ahead, writes another buffer's meanwhile)
            if (stop[b0]) { bad = true; break; }
            if (last) break;
        }
        if (!bad) lz4_move<false, LZ4W_TPB>(lds, ob, gout, raw, tid);
    }
    if (bad && tid == 0) {
        atomicMin(&P.bad[0], blockIdx.x);
        atomicAdd(&P.bad[1], 1u);
        if (P.block_bad) P.block_bad[blockIdx.x] = 1u;
    }
}

hipError_t launch_lz4_decode(const Lz4Params& p, hipStream_t s) {
    if (!p.n_blocks) return hipSuccess;
    const bool wide = lz4_pick_decoder(p.max_raw, p.decoder) == YSB_LZ4_DECODER_WIDE;
    const u32 lds = wide ? lz4_wide_lds_bytes(p.max_raw) : lz4_lds_bytes(p.max_raw);
    // (above 64 KiB of dynamic LDS the kernel must be told, on the current device: the largest
    // block's window is 66,096 B, the several-wave kernel's 69,456 B)
    if (lds > 65536u) {
        const hipError_t e = wide ? hipFuncSetAttribute(reinterpret_cast<const void*>(lz4_decode_wide_kernel),
                                                        hipFuncAttributeMaxDynamicSharedMemorySize,
                                                        (int)lz4_wide_lds_bytes(LZ4_MAX_RAW))
                                  : hipFuncSetAttribute(reinterpret_cast<const void*>(lz4_decode_kernel),
                                                        hipFuncAttributeMaxDynamicSharedMemorySize,
                                                        (int)lz4_lds_bytes(LZ4_MAX_RAW));
        if (e != hipSuccess) return e;
    }
    if (wide) hipLaunchKernelGGL(lz4_decode_wide_kernel, dim3(p.n_blocks), dim3(LZ4W_TPB), lds, s, p);
    else hipLaunchKernelGGL(lz4_decode_kernel, dim3(p.n_blocks), dim3(LZ4_TPB), lds, s, p);
    return hipGetLastError();
}

// ---- standard frames: the measure pass and the descriptors (ysb_lz4_frame.h) -----------------
// A frame block's raw size is not recorded, so it is found here: one wave per block walks the
// tokens alone -- lz4_measure_walk, the host model's function, over Lz4GlobalIn -- and copies
// nothing.  No LDS and few registers: many waves per CU, which is what hides a walk's latency.
constexpr u32 LZ4M_TPB = 256;   // four waves, four blocks

__global__ __launch_bounds__(LZ4M_TPB) void lz4_measure_kernel(const u8* base, const Lz4FrameBlock* blocks, u32 n_blocks,
                                                               u32* raw_out, u32 skip_tag) {
    const u32 lane = threadIdx.x & 63;
    const u32 blk = (u32)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (LZ4M_TPB / 64) + (threadIdx.x >> 6)));
    if (blk >= n_blocks) return;
    const Lz4FrameBlock e = blocks[blk];
    if (e.comp & skip_tag) return;   // another codec's block: its raw size is not this kernel's to write
    const u32 comp = e.comp & ~LZ4_STORED;
    u32 raw = 0;
    if (e.comp & LZ4_STORED) {
        raw = comp <= LZ4_MAX_RAW ? comp : 0u;
    } else if (comp) {
        Lz4GlobalIn in;
        in.init(base + e.offset, comp, lane);
        raw = lz4_measure_walk(in, comp);
    }
    if (lane == 0) raw_out[blk] = raw;
}

hipError_t launch_lz4_measure(const u8* base, const Lz4FrameBlock* blocks, u32 n_blocks, u32* raw, hipStream_t s, u32 skip_tag) {
    if (!n_blocks) return hipSuccess;
    const u32 per = LZ4M_TPB / 64;
    hipLaunchKernelGGL(lz4_measure_kernel, dim3((n_blocks + per - 1) / per), dim3(LZ4M_TPB), 0, s, base, blocks, n_blocks, raw, skip_tag);
    return hipGetLastError();
}

// The decode kernels' descriptors from the measured sizes: an exclusive prefix over the blocks,
// 256 at a time, by one workgroup (a batch holds a few thousand blocks at the most).
__global__ __launch_bounds__(256) void lz4_frame_desc_kernel(const Lz4FrameBlock* blocks, const u32* raw, u32 n_blocks,
                                                             u64 carry, const u64* d_carry, Lz4Desc* desc, u64* total) {
    __shared__ u32 scan[256];
    const u32 tid = threadIdx.x;
    if (d_carry) carry = *d_carry <= LZ4_CARRY_MAX ? *d_carry : 0;   // (never above it: the carry kernel's rule)
    u64 run = carry;
    for (u32 at = 0; at < n_blocks; at += 256) {
        const u32 i = at + tid;
        const u32 mine = i < n_blocks ? raw[i] : 0u;
        scan[tid] = mine;
        __syncthreads();
        for (u32 step = 1; step < 256; step <<= 1) {
            const u32 add = tid >= step ? scan[tid - step] : 0u;
            __syncthreads();
            scan[tid] += add;
            __syncthreads();
        }
        if (i < n_blocks) {
            const Lz4FrameBlock b = blocks[i];
            desc[i] = Lz4Desc{b.offset, run + (scan[tid] - mine), b.comp, mine};
        }
        run += scan[255];
        __syncthreads();
    }
    if (tid == 0) *total = run - carry;
}

hipError_t launch_lz4_frame_descs(const Lz4FrameBlock* blocks, const u32* raw, u32 n_blocks, u64 carry, Lz4Desc* desc,
                                  u64* total, hipStream_t s, const u64* d_carry) {
    hipLaunchKernelGGL(lz4_frame_desc_kernel, dim3(1), dim3(256), 0, s, blocks, raw, n_blocks, carry, d_carry, desc, total);
    return hipGetLastError();
}

// The carry of a stream of frame batches on the device (launch_lz4_frame_carry; the rule is
// lz4f_carry_cut's, which tests/native/lz4_frame_logic.cpp models over whole streams): a cut
// candidate e -- byte e - 1 a '\n', or a '\r' that is not the batch's last byte -- is searched
// from the end backwards, 1024 positions at a time, no further than LZ4_CARRY_MAX bytes.
__global__ __launch_bounds__(256) void lz4_frame_carry_kernel(u8* out, u8* carry, Lz4FrameHead* head, u32 more) {
    __shared__ unsigned long long best;
    const u32 tid = threadIdx.x;
    u64* clen = reinterpret_cast<u64*>(carry);
    u8* cbytes = carry + LZ4_CARRY_HEAD;
    const u64 cin = *clen <= LZ4_CARRY_MAX ? *clen : 0;
    const u64 total = cin + head->raw_total;
    const bool dropped = head->bad[1] != 0;
    for (u64 j = tid; j < cin; j += 256) out[j] = cbytes[j];
    if (tid == 0) best = 0;
    __syncthreads();   // the carry is read (and in `out`, for the search) before it is rewritten
    u64 cut = total;
    u32 overflow = 0;
    if (more && !dropped) {
        const u64 lo = total > LZ4_CARRY_MAX ? total - LZ4_CARRY_MAX - 1 : 0;   // a cut at or below lo leaves too much
        u64 hi = total;
        cut = 0;
        bool found = false;
        while (hi > lo && !found) {
            const u64 from = hi - lo > 1024 ? hi - 1024 : lo;   // candidates e in (from, hi]
            for (u64 e = from + 1 + tid; e <= hi; e += 256) {
                const u8 c = out[e - 1];
                if (c == '\n' || (c == '\r' && e < total)) atomicMax(&best, (unsigned long long)e);
            }
            __syncthreads();
            found = best != 0;
            if (found) cut = best;
            __syncthreads();
            hi = from;
        }
        if (!found && total > LZ4_CARRY_MAX) overflow = 1;   // (else: no terminator at all, everything is carried)
    }
    const bool drop = dropped || overflow;
    const u64 keep = drop ? 0 : total - cut;   // <= LZ4_CARRY_MAX
    for (u64 j = tid; j < keep; j += 256) cbytes[j] = out[cut + j];
    if (tid == 0) {
        *clen = keep;
        head->nbytes = drop ? 0 : cut;
        head->carry_in = (u32)cin;
        head->carry_out = (u32)keep;
        head->overflow = overflow;
    }
}

hipError_t launch_lz4_frame_carry(u8* out, u8* carry, Lz4FrameHead* head, u32 more, hipStream_t s) {
    hipLaunchKernelGGL(lz4_frame_carry_kernel, dim3(1), dim3(256), 0, s, out, carry, head, more);
    return hipGetLastError();
}

}  // namespace ysb
