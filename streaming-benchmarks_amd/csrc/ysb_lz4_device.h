// ysb_lz4_device.h -- what the block decoders' kernels share (ysb_lz4.hip, ysb_snappy.hip): the
// move between global memory and an LDS window with its edge rule, the reader's input streamed
// from global memory through a register window, and the fence between one wave's LDS write and
// another lane's read of it.  Device code only.
#pragma once
#include "ysb_kernels.h"

namespace ysb {

constexpr u32 LZ4_TPB = 64;   // one wave

// n bytes between global memory and the LDS window, lds_at congruent to g mod 16: vectors
// between the 16-byte boundaries inside [g, g + n), bytes at the edges.
// (NT threads take part; `lane` is the thread's index among them)
template <bool TO_LDS, u32 NT = LZ4_TPB>
__device__ __forceinline__ void lz4_move(u8* lds, u32 lds_at, u8* g, u32 n, u32 lane) {
    const u32 mis = (u32)(reinterpret_cast<uintptr_t>(g) & 15);
    u32 head = (16 - mis) & 15;
    if (head > n) head = n;
    const u32 nvec = (n - head) / 16, tail = head + nvec * 16;
    for (u32 j = lane; j < head; j += NT) {
        if (TO_LDS) lds[lds_at + j] = g[j];
        else g[j] = lds[lds_at + j];
    }
    for (u32 v = lane; v < nvec; v += NT) {
        uint4* l = reinterpret_cast<uint4*>(lds + lds_at + head + v * 16);
        uint4* m = reinterpret_cast<uint4*>(g + head + v * 16);
        if (TO_LDS) *l = *m;
        else *m = *l;
    }
    for (u32 j = tail + lane; j < n; j += NT) {
        if (TO_LDS) lds[lds_at + j] = g[j];
        else g[j] = lds[lds_at + j];
    }
}

// The reader's input straight from global memory: 256 bytes at a time, one aligned dword per
// lane, and the next 256 already in flight (a refill waits for a load issued a window ago, not
// for a fresh one).  Only dwords that hold at least one of the block's bytes are loaded -- an
// aligned dword never crosses a page, so nothing is touched that the block's own bytes do not
// make accessible.  byte() is wave-uniform, positions only grow.
struct Lz4GlobalIn {
    const u32* base4;
    u32 mis, ndw, lane;
    u32 win_pos, cur, nxt;
    __device__ __forceinline__ u32 load(u32 wp) const {
        const u32 i = wp / 4 + lane;
        return base4[i < ndw ? i : ndw - 1];
    }
    __device__ __forceinline__ void init(const u8* g, u32 comp, u32 lane_) {   // comp >= 1
        mis = (u32)(reinterpret_cast<uintptr_t>(g) & 3);
        base4 = reinterpret_cast<const u32*>(g - mis);
        ndw = (mis + comp + 3) / 4;
        lane = lane_;
        win_pos = 0;
        cur = load(0);
        nxt = load(256);
    }
    __device__ __forceinline__ u32 byte(u32 pos) {
        u32 rel = pos + mis - win_pos;
        if (rel >= 256u) {
            if (rel < 512u) {
                cur = nxt;
                win_pos += 256;
            } else {   // a long run of literals was stepped over
                win_pos = (pos + mis) & ~3u;
                cur = load(win_pos);
            }
            nxt = load(win_pos + 256);
            rel = pos + mis - win_pos;
        }
        const u32 w = (u32)__builtin_amdgcn_readlane((int)cur, (int)(rel >> 2));
        return (w >> ((rel & 3) * 8)) & 0xFFu;
    }
};

// between an LDS write of this wave and a read of it by another lane of the same wave
__device__ __forceinline__ void lz4_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

}  // namespace ysb
