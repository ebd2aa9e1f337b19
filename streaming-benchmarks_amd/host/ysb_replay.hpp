// ysb_replay.hpp -- the streaming mode's replay cycle as host data (no library call): the
// lines of one cycle of event time laid out batch by batch, each line's event_time digits
// located, and the host restatement of the device rebase.  tests/native/stream_logic.cpp.
#pragma once

#include <sys/mman.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "worker_pool.hpp"

namespace ysb {
namespace topology {

constexpr int64_t BUCKET_MS = 10000;       // CampaignProcessorCommon.java:28 (time_divisor)
constexpr uint64_t BATCH_ALIGN = 64;       // each batch's first byte (ysb_submit_raw_mapped: >= 16)
constexpr int64_t LEAD_SLACK = 16;         // buckets below t0's a line may fall in (skew, late events)

// One cycle of the replay: the generator's lines over cycleMs of event time in one anonymous
// mapping (each batch 64-byte aligned, the lines of a batch back to back), and the batches the
// cycle is released in.
struct ReplayCycle {
    uint8_t* bytes = nullptr;
    uint64_t reserved = 0;           // bytes mapped (virtual)
    uint64_t used = 0;               // bytes written, slack included (what is registered)
    std::vector<uint64_t> start;     // n line starts in `bytes`
    // per line: offset of its 13 time digits within the line | (leading nine digits - upperMin) << 16
    // (the encoding ysb_rebase_table consumes)
    std::vector<uint32_t> timeAt;
    int64_t upperMin = 0;
    uint32_t nUpper = 0;
    struct Batch {
        uint64_t a, b;               // lines [a, b)
        uint64_t off, nbytes;        // its bytes: [off, off + nbytes) of `bytes`
        int64_t releaseMs;           // nominal emission time of line b - 1 (cycle 0)
        int64_t maxTimeMs;           // the largest event_time in it (cycle 0)
    };
    std::vector<Batch> batches;
    uint64_t lines() const { return start.size(); }
    // The bytes given back (a compressed replay keeps the cycle's blocks, not its lines); the
    // index and the batches stay.
    void releaseBytes() {
        if (bytes) munmap(bytes, reserved);
        bytes = nullptr;
        reserved = 0;
    }
    ReplayCycle() = default;
    ReplayCycle(const ReplayCycle&) = delete;
    ReplayCycle& operator=(const ReplayCycle&) = delete;
    ~ReplayCycle() {
        if (bytes) munmap(bytes, reserved);
    }
};

// 13 decimal digits at p; -1 if one of them is no digit.
inline int64_t read13(const uint8_t* p) {
    int64_t v = 0;
    for (int d = 0; d < 13; ++d) {
        if (p[d] < '0' || p[d] > '9') return -1;
        v = v * 10 + (p[d] - '0');
    }
    return v;
}

// Where a line's "event_time": "<13 digits>" sits: the digits' offset within the line and
// their bucket (leading nine digits) relative to `base`; or what is wrong with the line.
struct EventTimeAt {
    const char* error;               // nullptr: found
    uint32_t offset, bucket;
};
inline EventTimeAt locate_event_time(const uint8_t* l, uint64_t len, int64_t base) {
    static const char KEY[] = "\"event_time\"";
    const void* k = memmem(l, len, KEY, sizeof KEY - 1);
    uint64_t p = k ? (uint64_t)((const uint8_t*)k - l) + sizeof KEY - 1 : len;
    while (p < len && (l[p] == ' ' || l[p] == ':')) ++p;
    if (p < len && l[p] == '"') ++p;
    if (p + 13 >= len || l[p + 13] != '"' || p > 0xFFFF) return {"no 13-digit event_time", 0, 0};
    const int64_t v = read13(l + p);
    if (v < 0) return {"event_time", 0, 0};
    const int64_t kk = v / BUCKET_MS - base;
    if (kk < 0 || kk > 0xFFFF) return {"event_time out of the cycle's range", 0, 0};
    return {nullptr, (uint32_t)p, (uint32_t)kk};
}

// Lays a cycle out from pieces of generated lines: batches close at batchMs of nominal emission
// time or a slot's bytes, whichever comes first.  The pages are written by the calling threads
// (first touch: on their NUMA node).
class CycleBuilder {
public:
    explicit CycleBuilder(ReplayCycle& c) : c_(c) {}
    // n lines of at most maxLine bytes; line i is emitted at t0Ms + i * 1000 / eventsPerSec
    void begin(uint64_t n, uint64_t maxLine, int64_t t0Ms, uint64_t eventsPerSec, int64_t batchMs, uint64_t slotBytes) {
        if (n == 0) throw std::runtime_error("empty replay cycle");
        n_ = n, t0Ms_ = t0Ms, eventsPerSec_ = eventsPerSec, batchMs_ = batchMs, slotBytes_ = slotBytes;
        c_.reserved = n * (maxLine + BATCH_ALIGN) + (1u << 20);
        void* m = mmap(nullptr, c_.reserved, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (m == MAP_FAILED) throw std::runtime_error("replay cycle: mmap failed");
        c_.bytes = static_cast<uint8_t*>(m);
        madvise(c_.bytes, c_.reserved, MADV_HUGEPAGE);
        c_.start.assign(n, 0);
        c_.timeAt.assign(n, 0);
        c_.upperMin = t0Ms / BUCKET_MS - LEAD_SLACK;
    }
    // lines [first, first + count): line first + j is bytes[off[j], off[j + 1])
    void add(uint64_t first, uint64_t count, const uint8_t* bytes, const uint32_t* off, WorkerPool& pool) {
        // the layout: sequential (batch boundaries depend on the lines before), positions only
        for (uint64_t j = 0; j < count; ++j) {
            const uint64_t i = first + j, len = off[j + 1] - off[j];
            if (open_ && (nominal(i) >= lim_ || pos_ + len - cur_.off > slotBytes_)) close(i);
            if (!open_) {
                pos_ = (pos_ + BATCH_ALIGN - 1) / BATCH_ALIGN * BATCH_ALIGN;
                cur_ = ReplayCycle::Batch{i, i, pos_, 0, 0, INT64_MIN};
                lim_ = nominal(i) + batchMs_;
                open_ = true;
                if (len > slotBytes_) throw std::runtime_error("a replay line is longer than the slot");
            }
            c_.start[i] = pos_;
            pos_ += len;
        }
        // the bytes and the time index: in parallel; a thread stops at its first bad line
        std::vector<std::string> err(pool.size());
        std::vector<uint32_t> kmax(pool.size(), 0);
        pool.run(pool.size(), [&](unsigned t) {
            const uint64_t ja = count * t / pool.size(), jb = count * (t + 1) / pool.size();
            for (uint64_t j = ja; j < jb; ++j) {
                const uint64_t i = first + j, len = off[j + 1] - off[j];
                std::memcpy(c_.bytes + c_.start[i], bytes + off[j], len);
                const EventTimeAt at = locate_event_time(bytes + off[j], len, c_.upperMin);
                if (at.error) {
                    err[t] = "line " + std::to_string(i) + ": " + at.error;
                    return;
                }
                c_.timeAt[i] = at.offset | (at.bucket << 16);
                kmax[t] = std::max(kmax[t], at.bucket);
            }
        });
        for (const auto& e : err)
            if (!e.empty()) throw std::runtime_error("replay cycle: " + e);
        kmax_ = std::max(kmax_, *std::max_element(kmax.begin(), kmax.end()));
    }
    void finish(WorkerPool& pool) {
        if (open_) close(n_);
        c_.used = pos_ + BATCH_ALIGN;     // slack: a batch's copy reads up to 15 bytes past its end
        c_.nUpper = 1 + kmax_;
        // each batch's largest event_time (cycle 0): from the index, in parallel over batches
        pool.run(pool.size(), [&](unsigned t) {
            for (size_t k = t; k < c_.batches.size(); k += pool.size()) {
                ReplayCycle::Batch& b = c_.batches[k];
                for (uint64_t i = b.a; i < b.b; ++i)
                    b.maxTimeMs = std::max(b.maxTimeMs, read13(c_.bytes + c_.start[i] + (c_.timeAt[i] & 0xFFFFu)));
            }
        });
    }

private:
    ReplayCycle& c_;
    uint64_t n_ = 0, eventsPerSec_ = 1, slotBytes_ = 0;
    int64_t t0Ms_ = 0, batchMs_ = 0;
    uint64_t pos_ = 0;                // write position in c_.bytes
    bool open_ = false;
    ReplayCycle::Batch cur_{};
    int64_t lim_ = 0;
    uint32_t kmax_ = 0;
    int64_t nominal(uint64_t i) const { return t0Ms_ + (int64_t)((i * 1000ull) / eventsPerSec_); }
    void close(uint64_t b) {
        cur_.b = b;
        cur_.nbytes = pos_ - cur_.off;
        cur_.releaseMs = nominal(b - 1);
        c_.batches.push_back(cur_);
        open_ = false;
    }
};

// The host restatement of the device rebase (ysb_split.hip rebase_kernel): batch b of cycle
// `cycle` copied into dst with every line's nine leading event_time digits moved by
// cycle * cycleMs / 10 000 buckets (the four trailing digits do not change), on
// min(T, pool, nbytes >> 22) threads (at least one).  The copy replay's fill and the CPU checks.
inline uint64_t fill_batch(const ReplayCycle& c, const ReplayCycle::Batch& b, uint64_t cycle, int64_t cycleMs,
                           uint8_t* dst, WorkerPool& pool, unsigned T) {
    const int64_t shift = (int64_t)cycle * (cycleMs / BUCKET_MS);
    std::vector<char> table(9ull * c.nUpper);
    for (uint32_t k = 0; k < c.nUpper; ++k) {
        int64_t v = c.upperMin + k + shift;
        for (int d = 8; d >= 0; --d) {
            table[9ull * k + d] = (char)('0' + v % 10);
            v /= 10;
        }
    }
    const uint64_t lines = b.b - b.a;
    const unsigned tn = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(std::min(T, pool.size()), b.nbytes >> 22));
    pool.run(tn, [&](unsigned t) {
        const uint64_t la = b.a + lines * t / tn, lb = b.a + lines * (t + 1) / tn;
        const uint64_t pa = c.start[la], pb = lb < b.b ? c.start[lb] : b.off + b.nbytes;
        std::memcpy(dst + (pa - b.off), c.bytes + pa, pb - pa);
        if (shift)
            for (uint64_t i = la; i < lb; ++i)
                std::memcpy(dst + (c.start[i] - b.off) + (c.timeAt[i] & 0xFFFFu), &table[9ull * (c.timeAt[i] >> 16)], 9);
    });
    return b.nbytes;
}

}  // namespace topology
}  // namespace ysb
