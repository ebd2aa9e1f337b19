// Host-side checks of the streaming replay's compressed cycle (host/ysb_replay_lz4.hpp over
// host/ysb_replay.hpp and csrc/ysb_lz4.h; no library, no GPU): small generated cycles whose
// batches close by time and by slot bytes, compressed at block sizes 64 B, 4 KiB and 64 KiB.
// Every batch's blocks decode (the host model) to exactly the batch's bytes; blocks end behind a
// line terminator and never span batches; the per-batch ranges and the directory are consistent;
// decoded sizes stay within the slot; the decode followed by the host rebase equals fill_batch
// for cycles 0, 1 and 7 -- also after the raw bytes are released.
// Built and run by tests/test_lz4_cycle_logic.py with g++ alone, plain and under the sanitizers.
#include <cinttypes>
#include <cstdio>
#include <string>
#include <vector>

#include "ysb_replay_lz4.hpp"

using namespace ysb;
using namespace ysb::topology;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { if (++fails <= 40) std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); } } while (0)

static const int64_t T0 = 1699999990000LL;   // bucket 169999999: one cycle of 10 s carries through all nine digits
static const int64_t CYCLE_MS = 10000;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}
static std::string hex(size_t n) {   // what a UUID looks like to a compressor
    std::string s;
    for (size_t i = 0; i < n; ++i) s += "0123456789abcdef"[rnd() & 15];
    return s;
}

// An event line of the generator's shape: ids that do not compress, keys that do.
static std::string make_line(int i, int64_t timeMs) {
    static const char* TYPES[] = {"view", "click", "purchase"};
    char d[32];
    std::snprintf(d, sizeof d, "%013" PRId64, timeMs);
    return "{\"user_id\": \"" + hex(8 + i % 29) + "\", \"page_id\": \"" + hex(36) + "\", \"ad_id\": \"" + hex(36) +
           "\", \"ad_type\": \"banner78\", \"event_type\": \"" + TYPES[i % 3] + "\", \"event_time\": \"" + d +
           "\", \"ip_address\": \"1.2.3.4\"}\n";
}

struct Lines {
    std::vector<uint8_t> bytes;
    std::vector<uint32_t> off;   // n + 1
    uint64_t maxLine = 0;
};

// n lines, one per 2 ms (500 events/s); lines 300..699 carry long user ids so that their batches
// close by bytes, the others' by time.
static Lines gen_lines(int n) {
    Lines l;
    l.off.push_back(0);
    for (int i = 0; i < n; ++i) {
        const int64_t t = T0 + i * 2 + (i * 37) % 101 - 50 + (i == 77 ? -155000 : 0) + (i == 901 ? 25000 : 0);
        std::string s = make_line(i, t);
        if (i >= 300 && i < 700) s.insert(13, hex(150 + i % 61));
        l.bytes.insert(l.bytes.end(), s.begin(), s.end());
        l.off.push_back((uint32_t)l.bytes.size());
        l.maxLine = std::max<uint64_t>(l.maxLine, s.size());
    }
    return l;
}

static void build(ReplayCycle& c, const Lines& l, int64_t batchMs, uint64_t slot, size_t piece, WorkerPool& pool) {
    const size_t n = l.off.size() - 1;
    CycleBuilder b(c);
    b.begin(n, l.maxLine, T0, 500, batchMs, slot);
    for (size_t a = 0; a < n; a += piece) {
        const size_t e = std::min(n, a + piece);
        std::vector<uint32_t> off(l.off.begin() + a, l.off.begin() + e + 1);
        for (uint32_t& o : off) o -= l.off[a];
        b.add(a, e - a, l.bytes.data() + l.off[a], off.data(), pool);
    }
    b.finish(pool);
}

static bool terminator_in(const uint8_t* p, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i)
        if (p[i] == '\n' || p[i] == '\r') return true;
    return false;
}

static void check_cycle(const Lines& l, int64_t batchMs, uint64_t slot, uint32_t block, unsigned threads) {
    WorkerPool pool(threads);
    ReplayCycle c;
    build(c, l, batchMs, slot, 700, pool);
    Lz4Cycle z;
    compress_cycle(c, block, z, pool);
    const size_t B = c.batches.size();
    CHECK(B >= 8 && z.batches.size() == B && z.blockBytes == block);
    uint64_t byTime = 0, byBytes = 0;
    for (size_t k = 0; k + 1 < B; ++k) {
        const ReplayCycle::Batch& b = c.batches[k];
        const bool y = b.nbytes + (l.off[b.b + 1] - l.off[b.b]) > slot;
        byBytes += y;
        byTime += !y;
    }
    CHECK(byTime >= 3 && byBytes >= 3);   // both ways a batch closes
    // the ranges and the directory
    uint64_t blocks = 0, end = 0, comp = 0, raw = 0, stored = 0, multi = 0;
    std::vector<uint8_t> got(slot + 64), want(slot + 64);
    std::vector<std::vector<uint8_t>> kept[3];
    const uint64_t cycles[3] = {0, 1, 7};
    for (size_t k = 0; k < B; ++k) {
        const ReplayCycle::Batch& b = c.batches[k];
        const Lz4Cycle::Batch& zb = z.batches[k];
        CHECK(zb.firstBlock == blocks && zb.blocks >= 1 && zb.firstBlock + zb.blocks <= z.dir.size());
        CHECK(zb.off % BATCH_ALIGN == 0 && zb.off == (end + BATCH_ALIGN - 1) / BATCH_ALIGN * BATCH_ALIGN);
        multi += zb.blocks > 1;
        uint64_t cb = 0, rb = 0;
        for (uint64_t i = 0; i < zb.blocks; ++i) {
            const ysb_lz4_block& e = z.dir[zb.firstBlock + i];
            CHECK(e.raw_bytes >= 1 && e.raw_bytes <= block);
            // a block ends behind a line terminator -- or holds none at all (a line longer than
            // the block: cut where it is); the batch's last block ends where the batch ends
            const uint8_t* p = c.bytes + b.off + rb;
            const bool last = i + 1 == zb.blocks;
            CHECK(p[e.raw_bytes - 1] == '\n' || (!last && e.raw_bytes == block && !terminator_in(p, block)));
            if (block >= 4096) CHECK(p[e.raw_bytes - 1] == '\n');
            if (e.comp_bytes & LZ4_STORED) {
                ++stored;
                CHECK(lz4_entry_comp(e) == e.raw_bytes);
            }
            cb += lz4_entry_comp(e);
            rb += e.raw_bytes;
        }
        CHECK(cb == zb.nbytes);                       // the batch's range is its blocks back to back
        CHECK(rb == b.nbytes && rb <= slot);          // they decode to the batch, within the slot: none spans batches
        blocks += zb.blocks;
        end = zb.off + zb.nbytes;
        comp += cb;
        raw += rb;
        // the decode: exactly the batch's bytes, nothing past them
        std::fill(got.begin(), got.end(), (uint8_t)0xA5);
        CHECK(decode_batch(z, k, b.nbytes, got.data()));
        CHECK(std::memcmp(got.data(), c.bytes + b.off, b.nbytes) == 0);
        CHECK(got[b.nbytes] == 0xA5 && got[b.nbytes + 63] == 0xA5);
        CHECK(!decode_batch(z, k, b.nbytes + 1, got.data()));
        // decode + rebase against the raw cycle's fill_batch
        for (int ci = 0; ci < 3; ++ci) {
            CHECK(fill_batch_lz4(c, z, k, cycles[ci], CYCLE_MS, got.data()));
            CHECK(fill_batch(c, b, cycles[ci], CYCLE_MS, want.data(), pool, threads) == b.nbytes);
            CHECK(std::memcmp(got.data(), want.data(), b.nbytes) == 0);
            kept[ci].emplace_back(want.begin(), want.begin() + b.nbytes);
        }
        if (k == 0) {   // a rebased batch differs from cycle 0's in its digits only
            CHECK(kept[1][0] != kept[0][0] && kept[2][0] != kept[1][0]);
        }
    }
    CHECK(blocks == z.dir.size() && comp == z.compBytes && raw == z.rawBytes);
    CHECK(z.used == end + BATCH_ALIGN && z.used <= z.reserved);
    if (block == 64) CHECK(stored > 0);                            // 64 bytes of mostly hex ids do not shrink
    if (block == 4096) CHECK(multi >= B / 2 && z.compBytes < z.rawBytes);
    if (block == 65536) CHECK(blocks == B);                        // a batch below 64 KiB is one block
    // a corrupted block is found by the host model
    {
        const Lz4Cycle::Batch& zb = z.batches[B / 2];
        const ysb_lz4_block keep = z.dir[zb.firstBlock];
        z.dir[zb.firstBlock].raw_bytes = keep.raw_bytes + 1;
        CHECK(!decode_batch(z, B / 2, c.batches[B / 2].nbytes, got.data()));
        z.dir[zb.firstBlock] = keep;
        CHECK(decode_batch(z, B / 2, c.batches[B / 2].nbytes, got.data()));
    }
    // the raw bytes released (what the GPU run does once its tables are on the device): the
    // index and the compressed cycle still give every cycle's bytes
    c.releaseBytes();
    CHECK(c.bytes == nullptr && c.lines() == l.off.size() - 1);
    for (size_t k = 0; k < B; ++k)
        for (int ci = 0; ci < 3; ++ci) {
            CHECK(fill_batch_lz4(c, z, k, cycles[ci], CYCLE_MS, got.data()));
            CHECK(std::memcmp(got.data(), kept[ci][k].data(), kept[ci][k].size()) == 0);
        }
    bool threw = false;
    try {
        Lz4Cycle z2;
        compress_cycle(c, block, z2, pool);
    } catch (const std::exception&) {
        threw = true;
    }
    CHECK(threw);
}

static void test_block_size_rule() {
    WorkerPool pool(2);
    const Lines l = gen_lines(50);
    ReplayCycle c;
    build(c, l, 50, 1 << 20, 50, pool);
    for (uint32_t bad : {0u, 65537u}) {
        bool threw = false;
        try {
            Lz4Cycle z;
            compress_cycle(c, bad, z, pool);
        } catch (const std::exception&) {
            threw = true;
        }
        CHECK(threw);
    }
}

int main() {
    const Lines l = gen_lines(1000);
    // 50 ms of emission time is 25 lines (~6 KB); the long lines' batches reach 8000 B first
    for (uint32_t block : {64u, 4096u, 65536u})
        for (unsigned threads : {1u, 3u}) check_cycle(l, 50, 8000, block, threads);
    // 64 KiB slots: batches of several 4 KiB blocks closed by time only would miss the byte rule,
    // so a second shape closes by bytes at 40 000 B with 250 ms batches
    check_cycle(l, 250, 40000, 4096, 3);
    check_cycle(l, 250, 40000, 65536, 2);
    test_block_size_rule();
    if (fails) {
        std::printf("%d checks failed\n", fails);
        return 1;
    }
    std::printf("lz4_cycle_logic OK\n");
    return 0;
}
