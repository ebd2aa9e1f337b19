// ysb_flush_merge.hpp -- the streaming mode's sink side (no library call): the shards' flushes
// merged by index, written in order by one thread, and the bookkeeping of which flush closes
// which window.  tests/native/stream_logic.cpp.
#pragma once

#include <algorithm>
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <functional>
#include <map>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "ysb_replay.hpp"
#include "ysb_topology.hpp"

namespace ysb {
namespace topology {

// One flush as the sink sees it: every shard's deltas, the watermark at its begin and the
// replay-clock time it is written at (the writer's "now", CampaignProcessorCommon.java:84).
struct FlushRows {
    int64_t index = 0;
    int64_t watermarkMs = 0;
    std::vector<WindowDelta> rows;
};

// sink(flush, nowMs): writes one flush's rows with the replay clock's now (ms).
using FlushSink = std::function<void(const FlushRows&, int64_t nowMs)>;

// Which flush closes which window, and the two latency samples.  A window is closed by the
// first flush whose watermark has passed its end (10 s after its start), at or after the flush
// that first shows it; once.  Single-threaded; `nowMs` is the time the flush was written at.
class WindowCloser {
public:
    std::vector<double> closeMs;      // per closed window: write time - window end
    std::vector<double> cwMs;         // per campaign of it: its last write - window start (get-stats)
    std::set<int64_t> seen, closed;
    void onFlush(const FlushRows& f, int64_t nowMs) {
        for (const WindowDelta& d : f.rows) {
            lastWrite_[{d.campaign, d.windowMs}] = nowMs;
            windowCampaigns_[d.windowMs].insert(d.campaign);
            seen.insert(d.windowMs);
        }
        for (int64_t w : seen) {
            if (closed.count(w) || w + BUCKET_MS > f.watermarkMs) continue;
            closed.insert(w);
            closeMs.push_back((double)(nowMs - (w + BUCKET_MS)));
            for (const std::string& c : windowCampaigns_[w]) cwMs.push_back((double)(lastWrite_[{c, w}] - w));
        }
    }

private:
    std::map<std::pair<std::string, int64_t>, int64_t> lastWrite_;   // (campaign, window_ms) -> time_updated
    std::map<int64_t, std::set<std::string>> windowCampaigns_;
};

// Merged flushes written in order by one thread (the flusher's writes).  An empty flush is
// counted but not handed to the sink; after a sink exception the queue is dropped and finish()
// throws "sink: ..." once.
class SinkThread {
public:
    SinkThread(const FlushSink& sink, std::function<int64_t()> clock) : sink_(sink), clock_(std::move(clock)) {
        th_ = std::thread([this] { loop(); });
    }
    ~SinkThread() {
        try {
            finish();
        } catch (...) {   // (an error the explicit finish would have reported)
        }
    }
    void push(FlushRows&& f) {
        {
            std::lock_guard<std::mutex> g(m_);
            q_.push_back(std::move(f));
        }
        cv_.notify_one();
    }
    void finish() {
        {
            std::lock_guard<std::mutex> g(m_);
            if (done_) return;
            done_ = true;
        }
        cv_.notify_one();
        th_.join();
        if (!error_.empty()) throw std::runtime_error("sink: " + error_);
    }
    // (the sink thread's own until finish() returned)
    uint64_t rows = 0, flushes = 0;
    WindowCloser windows;

private:
    FlushSink sink_;
    std::function<int64_t()> clock_;
    std::thread th_;
    std::mutex m_;
    std::condition_variable cv_;
    std::deque<FlushRows> q_;
    bool done_ = false;
    std::string error_;
    void loop() {
        for (;;) {
            FlushRows f;
            {
                std::unique_lock<std::mutex> g(m_);
                cv_.wait(g, [this] { return done_ || !q_.empty(); });
                if (q_.empty()) return;
                f = std::move(q_.front());
                q_.pop_front();
            }
            try {
                const int64_t now = clock_();
                if (!f.rows.empty()) sink_(f, now);
                rows += f.rows.size();
                ++flushes;
                windows.onFlush(f, now);
            } catch (const std::exception& e) {
                std::lock_guard<std::mutex> g(m_);
                error_ = e.what();
                q_.clear();
                return;
            }
        }
    }
};

// The shards' flushes merged by index: a flush goes to the sink once every shard delivered it,
// in index order, its watermark the minimum of the shards' (each taken at that shard's begin).
class FlushMerger {
public:
    FlushMerger(SinkThread& st, int shards) : st_(st), shards_(shards) {}
    void deliver(int64_t index, int64_t watermark, std::vector<WindowDelta>&& rows) {
        std::lock_guard<std::mutex> g(m_);
        Pending& p = pend_[index];
        if (p.left < 0) {
            p.left = shards_;
            p.f.index = index;
            p.f.watermarkMs = INT64_MAX;
        }
        p.f.watermarkMs = std::min(p.f.watermarkMs, watermark);
        for (auto& r : rows) p.f.rows.push_back(std::move(r));
        --p.left;
        while (!pend_.empty() && pend_.begin()->first == next_ && pend_.begin()->second.left == 0) {
            st_.push(std::move(pend_.begin()->second.f));
            pend_.erase(pend_.begin());
            ++next_;
        }
    }
    bool empty() {
        std::lock_guard<std::mutex> g(m_);
        return pend_.empty();
    }

private:
    struct Pending {
        int left = -1;
        FlushRows f;
    };
    SinkThread& st_;
    const int shards_;
    std::mutex m_;
    std::map<int64_t, Pending> pend_;
    int64_t next_ = 0;
};

}  // namespace topology
}  // namespace ysb
