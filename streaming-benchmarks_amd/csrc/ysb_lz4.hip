// ysb_lz4.hip -- LZ4 batches decoded on the GPU (ysb_submit_raw_lz4, ysb_lz4_decode_device;
// the format, its ONE sequence reader and the host model: ysb_lz4.h).  This is the codec a
// source otherwise runs on a CPU in front of FileBasedDataSource.run
// (AdvertisingTopologyNative.java:144-165) or inside a Kafka consumer: here the compressed
// blocks cross PCIe and are decoded where the lines are split and scanned.
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

namespace ysb {

constexpr u32 LZ4_TPB = 64;   // one wave

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

// n bytes between global memory and the LDS window, lds_at congruent to g mod 16: vectors
// between the 16-byte boundaries inside [g, g + n), bytes at the edges.
template <bool TO_LDS>
__device__ __forceinline__ void lz4_move(u8* lds, u32 lds_at, u8* g, u32 n, u32 lane) {
    const u32 mis = (u32)(reinterpret_cast<uintptr_t>(g) & 15);
    u32 head = (16 - mis) & 15;
    if (head > n) head = n;
    const u32 nvec = (n - head) / 16, tail = head + nvec * 16;
    for (u32 j = lane; j < head; j += LZ4_TPB) {
        if (TO_LDS) lds[lds_at + j] = g[j];
        else g[j] = lds[lds_at + j];
    }
    for (u32 v = lane; v < nvec; v += LZ4_TPB) {
        uint4* l = reinterpret_cast<uint4*>(lds + lds_at + head + v * 16);
        uint4* m = reinterpret_cast<uint4*>(g + head + v * 16);
        if (TO_LDS) *l = *m;
        else *m = *l;
    }
    for (u32 j = tail + lane; j < n; j += LZ4_TPB) {
        if (TO_LDS) lds[lds_at + j] = g[j];
        else g[j] = lds[lds_at + j];
    }
}

__global__ __launch_bounds__(LZ4_TPB) void lz4_decode_kernel(const Lz4Params P) {
    extern __shared__ __align__(16) u8 lz4_lds[];
    u8* lds = lz4_lds;
    const u32 lane = threadIdx.x;
    const Lz4Desc d = P.desc[blockIdx.x];
    const ysb_lz4_block e{d.comp, d.raw};
    const u32 comp = lz4_entry_comp(e), raw = d.raw;
    const u8* gin = P.in + d.in_off;
    u8* gout = P.out + d.out_off;
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
    }
}

hipError_t launch_lz4_decode(const Lz4Params& p, hipStream_t s) {
    if (!p.n_blocks) return hipSuccess;
    const u32 lds = lz4_lds_bytes(p.max_raw);
    // (above 64 KiB of dynamic LDS the kernel must be told, on the current device: the largest
    // block's window is 66,096 B)
    if (lds > 65536u) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(lz4_decode_kernel),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lz4_lds_bytes(LZ4_MAX_RAW));
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(lz4_decode_kernel, dim3(p.n_blocks), dim3(LZ4_TPB), lds, s, p);
    return hipGetLastError();
}

}  // namespace ysb
