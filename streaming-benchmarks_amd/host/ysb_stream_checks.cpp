// ysb_stream_checks.cpp -- the streaming mode's CPU checks (no GPU), each a JSON line:
// --stream-self-check, --stream-feed-check, --stream-merge-check.
#include <atomic>
#include <cstdio>
#include <random>

#include "ysb_feed_rules.hpp"
#include "ysb_stream.hpp"

namespace ysb {
namespace topology {

// The replay: a cycle from the host generator, each batch of each of `cycles` rebased into a
// buffer (fill_batch) and compared byte for byte with the host generator's own lines of that
// cycle (t0 moved by cycle * cycleMs).  With streamLz4 the cycle is compressed first and each
// batch comes out of its blocks instead (fill_batch_lz4: the host model's decode, then the
// rebase on the decoded bytes), and for cycle 0 the decode alone is compared with fill_batch's bytes.
std::string replaySelfCheck(const StreamOptions& o, const std::vector<uint64_t>& cycles) {
    const ysb_gen_params g = shard_gen(o, 1);
    const unsigned T = default_threads(o);
    WorkerPool pool(T);
    ReplayCycle c;
    build_cycle(nullptr, g, o, c, pool);
    Lz4Cycle z;
    if (o.streamLz4) compress_cycle(c, o.lz4Block, z, pool);
    std::vector<uint8_t> buf(o.slotBytes + 64), ref(o.slotBytes + 64);
    std::vector<uint32_t> off(c.lines() + 1);
    uint64_t lines = 0, bad = 0, batches = 0, misaligned = 0, lz4_bad = 0;
    for (size_t k = 0; o.streamLz4 && k < c.batches.size(); ++k) {   // the decode alone against cycle 0's bytes
        const ReplayCycle::Batch& b = c.batches[k];
        fill_batch(c, b, 0, o.cycleMs, ref.data(), pool, T);
        if (!decode_batch(z, k, b.nbytes, buf.data()) || std::memcmp(buf.data(), ref.data(), b.nbytes) != 0) ++lz4_bad;
    }
    for (uint64_t cy : cycles) {
        ysb_gen_params gc = g;
        gc.t0_ms = o.t0Ms + (int64_t)cy * o.cycleMs;   // the generator's own lines of that cycle
        for (const auto& b : c.batches) {
            uint64_t nb = b.nbytes;
            if (!o.streamLz4) nb = fill_batch(c, b, cy, o.cycleMs, buf.data(), pool, T);
            else if (!fill_batch_lz4(c, z, (size_t)(&b - c.batches.data()), cy, o.cycleMs, buf.data())) nb = 0;
            uint64_t rb = 0;
            if (ysb_gen_events_host(&gc, b.a, b.b - b.a, ref.data(), ref.size(), off.data(), &rb) != YSB_OK)
                throw std::runtime_error("ysb_gen_events_host failed");
            if (rb != nb || std::memcmp(buf.data(), ref.data(), nb) != 0) ++bad;
            misaligned += (b.off % BATCH_ALIGN) != 0;
            lines += b.b - b.a;
            ++batches;
        }
    }
    char o2[640];
    std::snprintf(o2, sizeof o2, "{\"mode\": \"stream-self-check\", \"lines_per_cycle\": %llu, \"batches\": %llu, "
                  "\"lines\": %llu, \"mismatched_batches\": %llu, \"misaligned_batches\": %llu, \"upper_values\": %u, "
                  "\"stream_lz4\": %s, \"lz4_block\": %u, \"lz4_blocks\": %zu, \"lz4_comp_bytes\": %llu, "
                  "\"lz4_raw_bytes\": %llu, \"lz4_mismatched_batches\": %llu}",
                  (unsigned long long)c.lines(), (unsigned long long)batches, (unsigned long long)lines,
                  (unsigned long long)bad, (unsigned long long)misaligned, c.nUpper, o.streamLz4 ? "true" : "false",
                  o.streamLz4 ? o.lz4Block : 0u, z.dir.size(), (unsigned long long)z.compBytes,
                  (unsigned long long)z.rawBytes, (unsigned long long)lz4_bad);
    return o2;
}

// The copy feeders: `shards` host cycles, each shard's feeder on a thread of its own filling
// its slot buffer as fast as it can for `seconds` (memcpy + digit patch); the aggregate
// events/s.  (The mapped feeder has no per-byte host work: its cost per batch is the submit
// call, measured by the GPU run.)
std::string feedCheck(const StreamOptions& o, double seconds) {
    // every shard: its own cycle (its own event stream), built and fed on a thread of its own
    const int S = o.shards;
    std::vector<std::unique_ptr<ReplayCycle>> cyc(S);
    std::vector<std::thread> th;
    std::vector<std::string> err(S);
    // streamLz4: every shard's cycle compressed as the GPU run compresses it, and every batch's
    // blocks decoded by the host model against fill_batch's bytes of cycle 0
    std::vector<uint64_t> lz4_bad(S, 0), lz4_comp(S, 0), lz4_raw(S, 0);
    for (int s = 0; s < S; ++s)
        th.emplace_back([&, s] {
            try {
                WorkerPool pool(default_threads(o));
                cyc[s].reset(new ReplayCycle());
                build_cycle(nullptr, shard_gen(o, 1 + (uint32_t)s), o, *cyc[s], pool);
                if (o.streamLz4) {
                    Lz4Cycle z;
                    compress_cycle(*cyc[s], o.lz4Block, z, pool);
                    std::vector<uint8_t> got(o.slotBytes + 64), want(o.slotBytes + 64);
                    for (size_t k = 0; k < cyc[s]->batches.size(); ++k) {
                        const ReplayCycle::Batch& b = cyc[s]->batches[k];
                        fill_batch(*cyc[s], b, 0, o.cycleMs, want.data(), pool, pool.size());
                        if (!decode_batch(z, k, b.nbytes, got.data()) || std::memcmp(got.data(), want.data(), b.nbytes) != 0)
                            ++lz4_bad[s];
                    }
                    lz4_comp[s] = z.compBytes;
                    lz4_raw[s] = z.rawBytes;
                }
            } catch (const std::exception& e) {
                err[s] = e.what();
            }
        });
    for (auto& t : th) t.join();
    th.clear();
    for (const auto& e : err)
        if (!e.empty()) throw std::runtime_error(e);
    // every feeder fills its own slot buffer as fast as it can (one thread each)
    std::vector<uint64_t> ev(S, 0);
    std::atomic<int> ready{0};
    std::atomic<bool> go{false};
    std::vector<double> el(S, 0);
    for (int s = 0; s < S; ++s)
        th.emplace_back([&, s] {
            const ReplayCycle& c = *cyc[s];
            std::vector<uint8_t> slot(o.slotBytes + 64);
            WorkerPool pool(1);
            ++ready;
            while (!go.load()) std::this_thread::yield();
            const double t0 = wall_s();
            uint64_t cycle = 0, next = 0, events = 0;
            while (wall_s() - t0 < seconds) {
                const ReplayCycle::Batch& b = c.batches[next];
                fill_batch(c, b, cycle, o.cycleMs, slot.data(), pool, 1);
                events += b.b - b.a;
                if (++next == c.batches.size()) {
                    next = 0;
                    ++cycle;
                }
            }
            el[s] = wall_s() - t0;
            ev[s] = events;
        });
    while (ready.load() < S) std::this_thread::yield();
    go = true;
    for (auto& t : th) t.join();
    uint64_t total = 0;
    double mx = 0;
    for (int s = 0; s < S; ++s) {
        total += ev[s];
        mx = std::max(mx, el[s]);
    }
    const double rate = mx > 0 ? (double)total / mx : 0;
    const double lineBytes = (double)(cyc[0]->used) / (double)cyc[0]->lines();
    uint64_t zbad = 0, zcomp = 0, zraw = 0;
    for (int s = 0; s < S; ++s) zbad += lz4_bad[s], zcomp += lz4_comp[s], zraw += lz4_raw[s];
    char out[768];
    std::snprintf(out, sizeof out, "{\"mode\": \"stream-feed-check\", \"shards\": %d, \"seconds\": %.2f, "
                  "\"lines_per_cycle\": %llu, \"batches_per_cycle\": %zu, \"copy_events_per_s\": %.1f, "
                  "\"copy_GBs\": %.2f, \"hardware_threads\": %u, \"stream_lz4\": %s, \"lz4_block\": %u, "
                  "\"lz4_comp_bytes\": %llu, \"lz4_raw_bytes\": %llu, \"lz4_mismatched_batches\": %llu}",
                  S, seconds, (unsigned long long)cyc[0]->lines(), cyc[0]->batches.size(), rate,
                  rate * lineBytes / 1e9, std::thread::hardware_concurrency(), o.streamLz4 ? "true" : "false",
                  o.streamLz4 ? o.lz4Block : 0u, (unsigned long long)zcomp, (unsigned long long)zraw,
                  (unsigned long long)zbad);
    return out;
}

// The shards' flush merge: `shards` threads deliver `flushes` flushes each, at random moments,
// with jittered watermarks and one delta row per flush, through the runner's own merger and
// sink thread.  The sink must see every index once, in order, with every shard's rows and the
// minimum of the shards' watermarks; the windows it closes are exactly those the merged
// watermarks pass ("ok": true|false).
std::string mergeCheck(int shards, int flushes, uint64_t seed) {
    if (shards < 1 || flushes < 1) throw std::runtime_error("mergeCheck: shards and flushes must be >= 1");
    const int64_t W0 = 1700000000000LL, STEP = 2500;
    std::vector<std::vector<int64_t>> wm(shards, std::vector<int64_t>(flushes));
    std::mt19937_64 rng(seed);
    for (int s = 0; s < shards; ++s)
        for (int i = 0; i < flushes; ++i) wm[s][i] = W0 + i * STEP - (int64_t)(rng() % 3001);
    std::vector<FlushRows> got;
    std::mutex gm;
    int64_t fake_now = W0;
    std::set<int64_t> closed;
    {
        SinkThread st([&](const FlushRows& f, int64_t) {
            std::lock_guard<std::mutex> g(gm);
            got.push_back(f);
        }, [&]() { return fake_now; });
        FlushMerger merger(st, shards);
        std::vector<std::thread> th;
        for (int s = 0; s < shards; ++s)
            th.emplace_back([&, s]() {
                std::mt19937_64 r(seed * 977 + (uint64_t)s);
                for (int i = 0; i < flushes; ++i) {
                    std::this_thread::sleep_for(std::chrono::microseconds(r() % 300));
                    const int64_t w = (W0 + i * STEP) / BUCKET_MS * BUCKET_MS;
                    std::vector<WindowDelta> rows{{"c" + std::to_string(s), w, (uint64_t)(s + 1)}};
                    merger.deliver(i, wm[s][i], std::move(rows));
                }
            });
        for (auto& t : th) t.join();
        st.finish();
        closed = st.windows.closed;
    }
    // the expectation: in index order, min watermark, every shard's row; windows closed by the
    // first flush (at or after the one that first shows them) whose watermark passes their end
    bool inOrder = (int)got.size() == flushes, wmMin = true, rowsOk = true;
    std::set<int64_t> seen, want;
    for (int i = 0; i < (int)got.size(); ++i) {
        const FlushRows& f = got[i];
        inOrder = inOrder && f.index == i;
        int64_t m = INT64_MAX;
        for (int s = 0; s < shards; ++s) m = std::min(m, wm[s][std::min<int64_t>(f.index, flushes - 1)]);
        wmMin = wmMin && f.watermarkMs == m;
        std::set<std::string> cs;
        for (const WindowDelta& d : f.rows) cs.insert(d.campaign);
        rowsOk = rowsOk && (int)f.rows.size() == shards && (int)cs.size() == shards;
        for (const WindowDelta& d : f.rows) seen.insert(d.windowMs);
        for (int64_t w : seen)
            if (w + BUCKET_MS <= f.watermarkMs) want.insert(w);
    }
    const bool ok = inOrder && wmMin && rowsOk && closed == want && !want.empty();
    char b[320];
    std::snprintf(b, sizeof b,
                  "{\"mode\": \"stream-merge-check\", \"shards\": %d, \"flushes\": %d, \"delivered\": %zu, "
                  "\"in_order\": %s, \"watermark_min\": %s, \"rows\": %s, \"closed\": %zu, \"closed_expected\": %zu, "
                  "\"ok\": %s}",
                  shards, flushes, got.size(), inOrder ? "true" : "false", wmMin ? "true" : "false",
                  rowsOk ? "true" : "false", closed.size(), want.size(), ok ? "true" : "false");
    return b;
}

}  // namespace topology
}  // namespace ysb
