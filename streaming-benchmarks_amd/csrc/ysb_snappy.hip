// ysb_snappy.hip -- snappy blocks decoded on the GPU (the blocks of snappy-compressed Kafka
// record batches: ysb_kafka_lz4.h; the format, its ONE element reader and the host model:
// ysb_snappy.h).  Two kernels beside the LZ4 ones in a compressed Kafka call's chain, for the
// blocks tagged YSB_SNAPPY_BLOCK alone (the LZ4 kernels skip those, these skip the rest):
//
//   snappy_preamble_kernel  a thread per block reads the block's own raw size -- what
//                           lz4_measure_kernel has to walk a whole LZ4 block for -- into raw[i], 0
//                           for a preamble that is bad, 0 or above 65536.
//   snappy_decode_kernel    one wave per block, one block per workgroup; the elements are walked
//                           serially by the whole wave, every position and length wave-uniform,
//                           the copies lane-parallel.  An element is at most 64 bytes of copy: one
//                           wave-wide LDS read and one write, an overlapping copy as
//                           dst[k] = src[k mod offset].
//
// Where the bytes are.  The OUTPUT block is decoded in LDS, as in ysb_lz4.hip: a copy reads bytes
// the same wave has just written, and a __syncthreads() (one wave: the LDS wait) stands between
// every write and a read that may see it.  The INPUT is not in LDS.  A snappy block may outgrow
// its raw bytes (65536 random bytes take 65542; the format's bound is raw + raw / 6 + 32), so
// lz4_decode_kernel's in-place window, whose write front provably stays behind its read front,
// does not carry over; and a separate input area of the bound's size beside the output would take
// 139 KiB at 64 KiB blocks, one wave per CU of 160 KiB LDS.  So the compressed bytes are streamed
// from global memory through a prefetched register window (Lz4GlobalIn, ysb_lz4_device.h) and
// the literals are copied from global memory straight into the output block: the window is the
// output alone, 2 workgroups per CU at 64 KiB blocks, 4 at the Java client's 32 KiB chunks, and
// more for smaller batches (the launch sizes it by the largest preamble the host read).
//
// Malformed input cannot fault or hang, for any bytes:
//   the block's extent [offset, offset + comp) is the host's (kafka_lz4_entries checked it against
//   the buffer and comp <= SNAPPY_MAX_COMP); the reader's input loads only aligned dwords that
//   hold at least one byte of it, and a literal's bytes are input positions the reader has checked
//   against comp -- nothing past comp_bytes is read;
//   `raw` is the planned size, at most P.max_raw (else the block is bad before anything is
//   touched), and the preamble must repeat it (mapped memory may have changed since the preamble
//   kernel ran); every LDS index is ob + an output position below raw by the reader's checks
//   (len <= raw - op, offset <= op), ob < 16, and the launch holds 16 + max_raw bytes;
//   every element consumes its tag at least, so the walk over comp bytes ends;
//   the global stores follow lz4_move's rule inside [out_off, out_off + raw), which the plan keeps
//   inside the inflated buffer: no 16-byte vector shared with a neighbouring block is
//   read-modify-written.  A bad block stores nothing at all and records itself in block_bad[]
//   and bad[0..1], as the LZ4 decoders do.
#include <atomic>

#include "ysb_kernels.h"
#include "ysb_lz4_device.h"
#include "ysb_snappy.h"

namespace ysb {

struct SnappyGlobalBytes {
    const u8* p;
    __device__ __forceinline__ u32 byte(u32 pos) const { return p[pos]; }
};

__global__ __launch_bounds__(256) void snappy_preamble_kernel(const u8* base, const Lz4FrameBlock* blocks, u32 n_blocks,
                                                              u32* raw_out) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_blocks) return;
    const Lz4FrameBlock e = blocks[i];
    if (!(e.comp & SNAPPY_BLOCK)) return;   // an LZ4 or stored block: lz4_measure_kernel's
    const u32 comp = e.comp & SNAPPY_LEN_MASK;
    SnappyGlobalBytes in{base + e.offset};
    raw_out[i] = (comp && comp <= SNAPPY_MAX_COMP) ? snappy_block_raw(in, comp, nullptr) : 0u;
}

hipError_t launch_snappy_preamble(const u8* base, const Lz4FrameBlock* blocks, u32 n_blocks, u32* raw, hipStream_t s) {
    if (!n_blocks) return hipSuccess;
    hipLaunchKernelGGL(snappy_preamble_kernel, dim3((n_blocks + 255) / 256), dim3(256), 0, s, base, blocks, n_blocks, raw);
    return hipGetLastError();
}

__global__ __launch_bounds__(LZ4_TPB) void snappy_decode_kernel(const Lz4Params P) {
    extern __shared__ __align__(16) u8 snappy_lds[];
    u8* lds = snappy_lds;
    const u32 lane = threadIdx.x;
    const Lz4Desc d = P.desc[blockIdx.x];
    if (!(d.comp & SNAPPY_BLOCK)) return;   // (the whole workgroup: the LZ4 kernels' block)
    const u32 comp = d.comp & SNAPPY_LEN_MASK, raw = d.raw;
    const u8* gin = P.in + d.in_off;
    u8* gout = P.out + d.out_off;
    // (raw 0: the preamble kernel's or the plan's verdict -- a block of a bad batch)
    bool bad = raw == 0 || raw > P.max_raw || raw > SNAPPY_MAX_RAW || comp == 0 || comp > SNAPPY_MAX_COMP;
    if (!bad) {
        const u32 ob = (u32)(reinterpret_cast<uintptr_t>(gout) & 15);   // output byte i at lds[ob + i]
        Lz4GlobalIn in;
        in.init(gin, comp, lane);
        u32 ip = 0, op = 0;
        bad = snappy_block_raw(in, comp, &ip) != raw;
        while (!bad && ip < comp) {
            SnappyEl e;
            if (snappy_read_el(in, ip, comp, op, raw, &e) != SNAPPY_EL_OK) {
                bad = true;
                break;
            }
            const u32 dst = ob + op;
            if (e.offset == 0) {
                // a literal: input only, and nothing written so far lies at or behind dst
                for (u32 at = 0; at < e.len; at += LZ4_TPB) {
                    const u32 k = at + lane;
                    if (k < e.len) lds[dst + k] = gin[e.pos + k];
                }
            } else {
                __syncthreads();   // the bytes just written may be the copy's source
                // at most 64 bytes: every lane reads before any writes (a wave's LDS instructions
                // complete in issue order), and every source byte lies in front of dst
                u8 b = 0;
                if (lane < e.len) b = lds[dst - e.offset + (e.offset >= LZ4_TPB ? lane : lane % e.offset)];
                if (lane < e.len) lds[dst + lane] = b;
            }
            op += e.len;
            ip = e.next;
        }
        if (!bad && op != raw) bad = true;   // the input ended with the output short
        if (!bad) {
            __syncthreads();
            lz4_move<false>(lds, ob, gout, raw, lane);
        }
    }
    if (bad && lane == 0) {
        atomicMin(&P.bad[0], blockIdx.x);
        atomicAdd(&P.bad[1], 1u);
        if (P.block_bad) P.block_bad[blockIdx.x] = 1u;
    }
}

hipError_t launch_snappy_decode(const Lz4Params& p, hipStream_t s) {
    if (!p.n_blocks) return hipSuccess;
    const u32 max_raw = p.max_raw < SNAPPY_MAX_RAW ? p.max_raw : SNAPPY_MAX_RAW;
    const u32 lds = snappy_lds_bytes(max_raw);
    // (above 64 KiB of dynamic LDS the kernel must be told, on the current device: once per device)
    if (lds > 65536u) {
        static std::atomic<unsigned long long> told{0};
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        const unsigned long long bit = 1ull << (dev & 63);
        if (dev >= 64 || !(told.load(std::memory_order_acquire) & bit)) {
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(snappy_decode_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)snappy_lds_bytes(SNAPPY_MAX_RAW));
            if (e != hipSuccess) return e;
            told.fetch_or(bit, std::memory_order_release);
        }
    }
    hipLaunchKernelGGL(snappy_decode_kernel, dim3(p.n_blocks), dim3(LZ4_TPB), lds, s, p);
    return hipGetLastError();
}

}  // namespace ysb
