// ysb_replay_lz4.hpp -- the streaming mode's replay cycle in compressed form, as host data (no
// library call, no HIP: the format and the host codec are csrc/ysb_lz4.h's): every batch of a
// ReplayCycle compressed on its own into line-aligned LZ4 blocks that never span batches, the
// blocks of all batches in one anonymous mapping (what --stream-lz4 registers in place of the
// raw cycle), one directory, and per batch where its blocks lie.  A batch's blocks decode to
// exactly the batch's bytes of cycle 0, so the cycle's line offsets and rebase table hold for
// the decoded batch as they hold for the raw one.  tests/native/lz4_cycle_logic.cpp.
#pragma once

#include "../csrc/ysb_lz4.h"
#include "ysb_replay.hpp"

namespace ysb {
namespace topology {

// the largest block size at which the decode outruns the link (DESIGN.md, LZ4 batches)
constexpr uint32_t STREAM_LZ4_BLOCK = 8192;

struct Lz4Cycle {
    uint8_t* bytes = nullptr;
    uint64_t reserved = 0;           // bytes mapped (virtual)
    uint64_t used = 0;               // bytes written, slack included (what is registered)
    uint32_t blockBytes = 0;
    uint64_t compBytes = 0, rawBytes = 0;   // the blocks' bytes and what they decode to, all batches
    std::vector<ysb_lz4_block> dir;  // every batch's entries, in batch order
    struct Batch {
        uint64_t firstBlock, blocks; // dir[firstBlock, firstBlock + blocks)
        uint64_t off, nbytes;        // its blocks back to back: [off, off + nbytes) of `bytes`
    };
    std::vector<Batch> batches;      // batches[k] is ReplayCycle::batches[k] compressed
    Lz4Cycle() = default;
    Lz4Cycle(const Lz4Cycle&) = delete;
    Lz4Cycle& operator=(const Lz4Cycle&) = delete;
    ~Lz4Cycle() {
        if (bytes) munmap(bytes, reserved);
    }
};

// Compresses the cycle batch by batch on the pool: the blocks' ranges first (line-aligned cuts
// depend on the data), then, pool.size() batches at a time, every batch into a scratch buffer of
// its thread and from there to its place behind the batch before it (each batch BATCH_ALIGN
// aligned) -- the mapping's pages are written by the pool's threads only, and only where
// compressed bytes end up (first touch: on their NUMA node).
inline void compress_cycle(const ReplayCycle& c, uint32_t blockBytes, Lz4Cycle& z, WorkerPool& pool) {
    if (blockBytes < 1 || blockBytes > LZ4_MAX_RAW) throw std::runtime_error("the LZ4 block size must be in 1..65536");
    if (!c.bytes) throw std::runtime_error("compress_cycle: the raw cycle is gone");
    const size_t B = c.batches.size();
    const unsigned T = pool.size();
    z.blockBytes = blockBytes;
    z.batches.assign(B, Lz4Cycle::Batch{0, 0, 0, 0});
    std::vector<std::vector<uint32_t>> len(B);   // per batch: its blocks' raw sizes
    pool.run(T, [&](unsigned t) {
        for (size_t k = t; k < B; k += T) {
            const ReplayCycle::Batch& b = c.batches[k];
            for (uint64_t at = 0; at < b.nbytes;) {
                const uint64_t e = lz4_block_end(c.bytes + b.off, b.nbytes, at, blockBytes, true);
                len[k].push_back((uint32_t)(e - at));
                at = e;
            }
        }
    });
    uint64_t blocks = 0, bound = 0;
    std::vector<uint64_t> cap(B, 0);
    for (size_t k = 0; k < B; ++k) {
        z.batches[k].firstBlock = blocks;
        z.batches[k].blocks = len[k].size();
        blocks += len[k].size();
        for (uint32_t n : len[k]) cap[k] += lz4_compress_bound(n);
        bound += cap[k] + BATCH_ALIGN;
        z.rawBytes += c.batches[k].nbytes;
    }
    z.dir.assign(blocks, ysb_lz4_block{0, 0});
    z.reserved = bound + (1u << 20);
    void* m = mmap(nullptr, z.reserved, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (m == MAP_FAILED) throw std::runtime_error("compressed replay cycle: mmap failed");
    z.bytes = static_cast<uint8_t*>(m);
    madvise(z.bytes, z.reserved, MADV_HUGEPAGE);
    std::vector<std::vector<uint8_t>> scratch(T);
    uint64_t pos = 0;
    for (size_t k0 = 0; k0 < B; k0 += T) {
        const unsigned n = (unsigned)std::min<size_t>(T, B - k0);
        pool.run(n, [&](unsigned t) {
            const size_t k = k0 + t;
            const ReplayCycle::Batch& b = c.batches[k];
            Lz4Cycle::Batch& zb = z.batches[k];
            if (scratch[t].size() < cap[k]) scratch[t].resize(cap[k]);
            uint64_t at = 0, o = 0;
            for (uint64_t i = 0; i < zb.blocks; ++i) {
                const ysb_lz4_block e = lz4_pack_block(c.bytes + b.off + at, len[k][i], scratch[t].data() + o, true);
                z.dir[zb.firstBlock + i] = e;
                at += len[k][i];
                o += lz4_entry_comp(e);
            }
            zb.nbytes = o;
        });
        for (unsigned t = 0; t < n; ++t) {   // each behind the one before it
            Lz4Cycle::Batch& zb = z.batches[k0 + t];
            pos = (pos + BATCH_ALIGN - 1) / BATCH_ALIGN * BATCH_ALIGN;
            zb.off = pos;
            pos += zb.nbytes;
            z.compBytes += zb.nbytes;
        }
        pool.run(n, [&](unsigned t) {
            const Lz4Cycle::Batch& zb = z.batches[k0 + t];
            std::memcpy(z.bytes + zb.off, scratch[t].data(), zb.nbytes);
        });
    }
    z.used = pos + BATCH_ALIGN;   // slack: a batch's copy reads up to 15 bytes past its end
}

// Batch k decoded by the host model into dst (ReplayCycle::batches[k].nbytes bytes): the bytes
// of cycle 0.  false if a block breaks the format or the sizes do not add up.
inline bool decode_batch(const Lz4Cycle& z, size_t k, uint64_t rawBytes, uint8_t* dst) {
    const Lz4Cycle::Batch& zb = z.batches[k];
    uint64_t raw = 0;
    if (lz4_check_dir(z.dir.data() + zb.firstBlock, (uint32_t)zb.blocks, zb.nbytes, &raw, nullptr) != LZ4_DIR_OK) return false;
    if (raw != rawBytes) return false;
    return lz4_decode_batch(z.bytes + zb.off, z.dir.data() + zb.firstBlock, (uint32_t)zb.blocks, dst) == LZ4_NO_BAD;
}

// The host restatement of what the device does with batch k of cycle `cycle`: the decode, then
// the rebase on the decoded bytes (ysb_split.hip rebase_kernel; fill_batch's digits).  The raw
// cycle's index (start, timeAt) is used, its bytes are not.
inline bool fill_batch_lz4(const ReplayCycle& c, const Lz4Cycle& z, size_t k, uint64_t cycle, int64_t cycleMs, uint8_t* dst) {
    const ReplayCycle::Batch& b = c.batches[k];
    if (!decode_batch(z, k, b.nbytes, dst)) return false;
    const int64_t shift = (int64_t)cycle * (cycleMs / BUCKET_MS);
    if (!shift) return true;
    for (uint64_t i = b.a; i < b.b; ++i) {
        int64_t v = c.upperMin + (int64_t)(c.timeAt[i] >> 16) + shift;
        uint8_t* p = dst + (c.start[i] - b.off) + (c.timeAt[i] & 0xFFFFu);
        for (int d = 8; d >= 0; --d) {
            p[d] = (uint8_t)('0' + v % 10);
            v /= 10;
        }
    }
    return true;
}

}  // namespace topology
}  // namespace ysb
