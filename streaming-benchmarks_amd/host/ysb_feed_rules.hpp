// ysb_feed_rules.hpp -- what the streaming mode's feeders and their coordinator share (no
// library call): the replay clock, the start/stop/final handshake's flags, and the pure rules
// of the watermark and of the ring following it.  tests/native/stream_logic.cpp.
#pragma once

#include <atomic>
#include <chrono>
#include <cstdint>
#include <optional>

#include "ysb_replay.hpp"

namespace ysb {
namespace topology {

inline double wall_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Event time runs `speedup` times faster than the wall clock, from t0Ms at wall0.
struct ReplayClock {
    double wall0 = 0;
    int64_t t0Ms = 0;
    double speedup = 1;
    int64_t at(double wall) const { return t0Ms + (int64_t)((wall - wall0) * 1000.0 * speedup); }
    int64_t now() const { return at(wall_s()); }
    double wallOf(int64_t eventMs) const { return wall0 + (double)(eventMs - t0Ms) / (1000.0 * speedup); }
};

// The coordinator's side of the handshake: it counts the flushes asked for, stops the input at
// stopAt, and after every feeder's ysb_sync asks for the final flush.
struct FeedControl {
    std::atomic<int64_t> flushReq{0};
    std::atomic<bool> stop{false}, final{false}, failed{false};
    ReplayClock clock;
    double stopAt = 0;                // wall: no batch is submitted from here on
};

// A shard's watermark: the largest event_time submitted minus the out-of-orderness bound.
inline int64_t watermark_of(int64_t maxTime, int64_t oooMs) {
    return maxTime == INT64_MIN ? INT64_MIN : maxTime - oooMs;
}

// The ring follows the shard's watermark: when the newest bucket comes within 8 of the end of
// a ring of W buckets from ringLo, the base to move it to (8 buckets below the watermark's) --
// if that moves it forward.
inline std::optional<int64_t> ring_follow(int64_t maxTime, int64_t ringLo, uint32_t W, int64_t oooMs) {
    if (maxTime == INT64_MIN) return std::nullopt;
    if (maxTime / BUCKET_MS + 8 < ringLo + (int64_t)W) return std::nullopt;
    const int64_t lo = (maxTime - oooMs) / BUCKET_MS - 8;
    if (lo <= ringLo) return std::nullopt;
    return lo;
}

}  // namespace topology
}  // namespace ysb
