// Host-side checks of the native runner's streaming mode where it needs no library and no GPU
// (host/ysb_replay.hpp, ysb_flush_merge.hpp, ysb_feed_rules.hpp): the replay cycle's batch
// layout and event_time index from hand-written lines, the index's rejections, the host
// rebase against the digits worked out here, which flush closes which window, the flush merge
// and the sink thread's error path, the replay clock and the ring-follow rule.
// Built and run by tests/test_capi.py with g++ (no GPU, no library).
#include <cinttypes>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "ysb_feed_rules.hpp"
#include "ysb_flush_merge.hpp"
#include "ysb_replay.hpp"

using namespace ysb::topology;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { if (++fails <= 40) std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); } } while (0)

static const int64_t T0 = 1699999990000LL;   // bucket 169999999: one cycle of 10 s carries through all nine digits

// A JSON-looking line: a prefix of `prefix` bytes, the key, 13 digits (or `digits` verbatim), a tail.
struct Line {
    std::string text;
    uint32_t digitsAt = 0;
    int64_t timeMs = 0;
};
static Line make_line(size_t prefix, int64_t timeMs, size_t tail, const char* digits = nullptr, bool key = true) {
    Line l;
    l.timeMs = timeMs;
    l.text = "{\"user_id\": \"" + std::string(prefix, 'u') + "\", " + (key ? "\"event_time\"" : "\"event_tome\"") + ": \"";
    l.digitsAt = (uint32_t)l.text.size();
    char d[32];
    std::snprintf(d, sizeof d, "%013" PRId64, timeMs);
    l.text += digits ? digits : d;
    l.text += "\", \"ip_address\": \"" + std::string(tail, '1') + "\"}\n";
    return l;
}

struct Piece {
    std::vector<uint8_t> bytes;
    std::vector<uint32_t> off;
};
static Piece pack(const std::vector<Line>& lines, size_t a, size_t b) {
    Piece p;
    p.off.push_back(0);
    for (size_t i = a; i < b; ++i) {
        p.bytes.insert(p.bytes.end(), lines[i].text.begin(), lines[i].text.end());
        p.off.push_back((uint32_t)p.bytes.size());
    }
    return p;
}

// Builds a cycle from `lines` in pieces of `piece` lines; the error text, or "" if it was built.
static std::string build(ReplayCycle& c, const std::vector<Line>& lines, int64_t t0, uint64_t eps, int64_t batchMs,
                         uint64_t slot, size_t piece, WorkerPool& pool) {
    uint64_t maxLine = 0;
    for (const Line& l : lines) maxLine = std::max<uint64_t>(maxLine, l.text.size());
    try {
        CycleBuilder b(c);
        b.begin(lines.size(), maxLine, t0, eps, batchMs, slot);
        for (size_t a = 0; a < lines.size(); a += piece) {
            const size_t e = std::min(lines.size(), a + piece);
            const Piece p = pack(lines, a, e);
            b.add(a, e - a, p.bytes.data(), p.off.data(), pool);
        }
        b.finish(pool);
    } catch (const std::exception& e) {
        return e.what();
    }
    return "";
}

static void test_layout() {
    // one line per 2 ms; 120 short lines (a 50 ms batch of them is ~2.7 KB: closes by time),
    // then 180 long ones (~330 B: 4 KiB closes by bytes first), then short ones again
    const uint64_t EPS = 500, SLOT = 4096;
    const int64_t BATCH_MS = 50;
    std::vector<Line> lines;
    for (int i = 0; i < 400; ++i) {
        const bool longLine = i >= 120 && i < 300;
        const int64_t t = T0 + i * 2 + (i * 37) % 101 - 50 + (i == 77 ? -155000 : 0) + (i == 301 ? 25000 : 0);
        lines.push_back(make_line(longLine ? 200 + i % 61 : i % 23, t, longLine ? 40 : i % 7));
    }
    auto nominal = [&](uint64_t i) { return T0 + (int64_t)(i * 1000 / EPS); };
    WorkerPool pool(3);
    ReplayCycle c;
    CHECK(build(c, lines, T0, EPS, BATCH_MS, SLOT, 150, pool) == "");
    CHECK(c.lines() == 400 && !c.batches.empty());
    CHECK(c.upperMin == T0 / 10000 - 16);
    uint64_t expectA = 0, end = 0, byTime = 0, byBytes = 0;
    int64_t maxBucket = 0;
    for (size_t k = 0; k < c.batches.size(); ++k) {
        const ReplayCycle::Batch& b = c.batches[k];
        CHECK(b.a == expectA && b.b > b.a);
        expectA = b.b;
        CHECK(b.off % 64 == 0 && b.off == (end + 63) / 64 * 64);
        CHECK(b.nbytes <= SLOT);
        CHECK(b.releaseMs == nominal(b.b - 1));
        uint64_t pos = b.off;
        int64_t mx = INT64_MIN;
        for (uint64_t i = b.a; i < b.b; ++i) {
            const Line& l = lines[i];
            CHECK(c.start[i] == pos);                                     // back to back
            CHECK(std::memcmp(c.bytes + pos, l.text.data(), l.text.size()) == 0);
            CHECK(nominal(i) < nominal(b.a) + BATCH_MS);                    // no line past the batch's time ...
            pos += l.text.size();
            CHECK(pos - b.off <= SLOT);                                   // ... or its bytes
            mx = std::max(mx, l.timeMs);
            CHECK((c.timeAt[i] & 0xFFFFu) == l.digitsAt);
            CHECK((int64_t)(c.timeAt[i] >> 16) == l.timeMs / 10000 - c.upperMin);
            maxBucket = std::max(maxBucket, l.timeMs / 10000 - c.upperMin);
        }
        CHECK(b.nbytes == pos - b.off);
        CHECK(b.maxTimeMs == mx);
        end = pos;
        if (b.b < 400) {   // why it closed: the next line's time, or its bytes
            const bool t = nominal(b.b) >= nominal(b.a) + BATCH_MS, y = b.nbytes + lines[b.b].text.size() > SLOT;
            CHECK(t || y);
            byTime += t;
            byBytes += y && !t;
        }
    }
    CHECK(expectA == 400);
    CHECK(byTime >= 3 && byBytes >= 3);
    CHECK(c.used == end + 64);
    CHECK(c.nUpper == (uint32_t)maxBucket + 1 && maxBucket == 16 + 2);   // line 301: 2.5 buckets after t0
    CHECK((c.timeAt[77] >> 16) == 0);                                   // 16 buckets below t0's: the lowest accepted
}

static void test_rejections() {
    WorkerPool pool(3);
    auto base = [] {
        std::vector<Line> v;
        for (int i = 0; i < 30; ++i) v.push_back(make_line(i % 5, T0 + i, 3));
        return v;
    };
    auto error_of = [&](std::vector<Line> v, uint64_t slot = 1 << 20) {
        ReplayCycle c;
        return build(c, v, T0, 1000, 10, slot, 16, pool);
    };
    CHECK(error_of(base()) == "");
    std::vector<Line> v = base();
    v[13] = make_line(300, T0 + 13, 3);
    CHECK(error_of(v, 256) == "a replay line is longer than the slot");
    v = base();
    v[21] = make_line(2, T0, 3, nullptr, false);
    CHECK(error_of(v) == "replay cycle: line 21: no 13-digit event_time");
    v = base();
    v[4] = make_line(2, T0, 3, "169999999000");
    CHECK(error_of(v) == "replay cycle: line 4: no 13-digit event_time");
    v = base();
    v[17] = make_line(2, T0, 3, "16999999x0000");
    CHECK(error_of(v) == "replay cycle: line 17: event_time");
    v = base();
    v[29] = make_line(0xFFFF, T0, 3);                       // the digits sit past offset 0xFFFF
    CHECK(v[29].digitsAt > 0xFFFF);
    CHECK(error_of(v) == "replay cycle: line 29: no 13-digit event_time");
    v[29] = make_line(0xFFFF - (v[29].digitsAt - 0xFFFF), T0, 3);
    CHECK(v[29].digitsAt == 0xFFFF && error_of(v) == "");   // at 0xFFFF: accepted
    v = base();
    v[9] = make_line(2, T0 - 160001, 3);                    // 17 buckets below t0's
    CHECK(error_of(v) == "replay cycle: line 9: event_time out of the cycle's range");
    v[9] = make_line(2, T0 - 160000, 3);
    CHECK(error_of(v) == "");
    v = base();
    v[0] = make_line(2, T0 + (0x10000 - 16) * 10000LL, 3);  // bucket index 0x10000
    CHECK(error_of(v) == "replay cycle: line 0: event_time out of the cycle's range");
    v[0] = make_line(2, T0 + (0xFFFF - 16) * 10000LL + 9999, 3);
    CHECK(error_of(v) == "");
    ReplayCycle c;
    CHECK(build(c, {}, T0, 1000, 10, 1 << 20, 16, pool) == "empty replay cycle");
}

// dst against the batch's source lines: only the nine leading digits may differ, and they read
// bucket + cycle * cycleMs / 10 000
static void check_rebased(const std::vector<Line>& lines, const ReplayCycle::Batch& b, const std::vector<uint8_t>& dst,
                          uint64_t cycle, int64_t cycleMs) {
    uint64_t pos = 0;
    for (uint64_t i = b.a; i < b.b; ++i) {
        std::string want = lines[i].text;
        char d[16];
        std::snprintf(d, sizeof d, "%09" PRId64, lines[i].timeMs / 10000 + (int64_t)cycle * (cycleMs / 10000));
        want.replace(lines[i].digitsAt, 9, d);
        if (std::memcmp(dst.data() + pos, want.data(), want.size()) != 0) {
            CHECK(!"a rebased line differs");
            return;
        }
        pos += want.size();
    }
    CHECK(pos == b.nbytes);
}

static void test_rebase() {
    WorkerPool pool(2);
    {
        std::vector<Line> lines;
        for (int i = 0; i < 500; ++i) lines.push_back(make_line(i % 19, T0 + i * 20 + (i * 37) % 101 - 50, i % 5));
        ReplayCycle c;
        CHECK(build(c, lines, T0, 50, 100, 1 << 20, 200, pool) == "");
        CHECK(c.batches.size() > 10);
        std::vector<uint8_t> dst((1 << 20) + 64);
        for (uint64_t cycle : {0ull, 1ull, 7ull, 1000ull})
            for (const auto& b : c.batches) {
                std::fill(dst.begin(), dst.end(), 0xEE);
                CHECK(fill_batch(c, b, cycle, 10000, dst.data(), pool, 2) == b.nbytes);
                if (cycle == 0) CHECK(std::memcmp(dst.data(), c.bytes + b.off, b.nbytes) == 0);
                check_rebased(lines, b, dst, cycle, 10000);
                CHECK(dst[b.nbytes] == 0xEE);
            }
        // the carry: 169999999 -> 170000000 at cycle 1
        fill_batch(c, c.batches[0], 1, 10000, dst.data(), pool, 2);
        CHECK(lines[1].timeMs / 10000 == 169999999 && std::memcmp(dst.data() + lines[0].text.size() + lines[1].digitsAt, "170000000", 9) == 0);
    }
    {   // one batch of >= 8 MiB: the copy splits over two threads, at a line boundary
        std::vector<Line> lines;
        for (int i = 0; i < 40000; ++i) lines.push_back(make_line(150 + i % 41, T0 + i / 4, 10));
        ReplayCycle c;
        CHECK(build(c, lines, T0, 4000, 1 << 30, 16 << 20, 1 << 14, pool) == "");
        CHECK(c.batches.size() == 1 && (c.batches[0].nbytes >> 22) >= 2);
        std::vector<uint8_t> dst((16 << 20) + 64, 0xEE);
        fill_batch(c, c.batches[0], 7, 20000, dst.data(), pool, 2);
        check_rebased(lines, c.batches[0], dst, 7, 20000);
        CHECK(dst[c.batches[0].nbytes] == 0xEE);
    }
}

static FlushRows flush(int64_t index, int64_t wm, std::vector<WindowDelta> rows) {
    FlushRows f;
    f.index = index;
    f.watermarkMs = wm;
    f.rows = std::move(rows);
    return f;
}

static void test_window_closer() {
    const int64_t W = 1700000000000LL, W1 = W + 10000, W2 = W + 20000;
    WindowCloser wc;
    wc.onFlush(flush(0, W + 5000, {{"a", W, 1}, {"b", W, 1}}), W + 1000);
    wc.onFlush(flush(1, W + 9999, {{"a", W, 2}}), W + 9000);
    CHECK(wc.closed.empty() && wc.closeMs.empty() && wc.seen.count(W));
    wc.onFlush(flush(2, W + 10000, {}), W + 10500);                 // the first watermark at its end
    CHECK(wc.closed == std::set<int64_t>{W});
    CHECK(wc.closeMs == std::vector<double>{500.0});
    CHECK((wc.cwMs == std::vector<double>{9000.0, 1000.0}));        // a's last write, b's
    wc.onFlush(flush(3, W + 30000, {{"a", W, 1}}), W + 12000);      // a late row; the watermark is past W1's end
    CHECK(wc.closeMs.size() == 1 && wc.cwMs.size() == 2 && wc.closed.size() == 1);   // W1 not shown yet
    wc.onFlush(flush(4, W + 30000, {{"c", W1, 5}}), W + 31000);     // shown: closed by this flush
    CHECK((wc.closed == std::set<int64_t>{W, W1}));
    CHECK((wc.closeMs == std::vector<double>{500.0, 11000.0}));
    CHECK((wc.cwMs == std::vector<double>{9000.0, 1000.0, 21000.0}));
    wc.onFlush(flush(5, INT64_MIN, {{"c", W2, 1}}), W + 32000);     // no watermark yet: closes nothing
    CHECK(wc.closed.size() == 2 && wc.seen.size() == 3 && wc.closeMs.size() == 2);
}

static void test_merge_scripted() {
    std::vector<FlushRows> got;
    SinkThread st([&](const FlushRows& f, int64_t) { got.push_back(f); }, [] { return (int64_t)0; });
    FlushMerger m(st, 3);
    auto wm = [](int shard, int64_t i) { return 1000 * i - 10 * ((shard + i) % 3); };
    auto deliver = [&](int shard, int64_t i) { m.deliver(i, wm(shard, i), {{"s" + std::to_string(shard), i * 10000, (uint64_t)shard + 1}}); };
    for (int64_t i : {0, 1, 2, 3}) deliver(0, i);   // shard 0 runs ahead
    deliver(2, 1);                                   // shard 2 out of index order
    deliver(2, 0);
    deliver(1, 0);                                   // completes 0
    deliver(1, 2);
    deliver(1, 1);                                   // completes 1
    deliver(2, 3);
    deliver(2, 2);                                   // completes 2
    CHECK(!m.empty());
    deliver(1, 3);
    CHECK(m.empty());
    st.finish();
    CHECK(got.size() == 4 && st.flushes == 4 && st.rows == 12);
    for (size_t i = 0; i < got.size(); ++i) {
        CHECK(got[i].index == (int64_t)i);
        CHECK(got[i].watermarkMs == std::min({wm(0, i), wm(1, i), wm(2, i)}));
        std::set<std::string> who;
        for (const WindowDelta& d : got[i].rows) who.insert(d.campaign);
        CHECK(got[i].rows.size() == 3 && who.size() == 3);
    }
}

// (timing-dependent: the interleaving of the deliveries; the expectation is not)
static void test_merge_threaded() {
    const int S = 3, F = 100;
    const int64_t W0 = 1700000000000LL, STEP = 2500;
    std::vector<std::vector<int64_t>> wm(S, std::vector<int64_t>(F));
    std::mt19937_64 rng(7);
    for (auto& v : wm)
        for (int i = 0; i < F; ++i) v[i] = W0 + i * STEP - (int64_t)(rng() % 3001);
    std::vector<FlushRows> got;
    SinkThread st([&](const FlushRows& f, int64_t) { got.push_back(f); }, [&] { return W0; });
    FlushMerger m(st, S);
    std::vector<std::thread> th;
    for (int s = 0; s < S; ++s)
        th.emplace_back([&, s] {
            std::mt19937_64 r(977 + s);
            for (int i = 0; i < F; ++i) {
                std::this_thread::sleep_for(std::chrono::microseconds(r() % 200));
                m.deliver(i, wm[s][i], {{"c" + std::to_string(s), (W0 + i * STEP) / 10000 * 10000, 1}});
            }
        });
    for (auto& t : th) t.join();
    st.finish();
    CHECK((int)got.size() == F && m.empty());
    std::set<int64_t> seen, want;
    for (int i = 0; i < (int)got.size(); ++i) {
        CHECK(got[i].index == i && got[i].rows.size() == (size_t)S);
        CHECK(got[i].watermarkMs == std::min({wm[0][i], wm[1][i], wm[2][i]}));
        for (const WindowDelta& d : got[i].rows) seen.insert(d.windowMs);
        for (int64_t w : seen)
            if (w + 10000 <= got[i].watermarkMs) want.insert(w);
    }
    CHECK(st.windows.closed == want && !want.empty());
}

static void test_sink_errors() {
    int calls = 0;
    auto sink = [&](const FlushRows&, int64_t) {
        if (++calls == 3) throw std::runtime_error("boom");
    };
    {
        SinkThread st(sink, [] { return (int64_t)0; });
        st.push(flush(0, 0, {}));                    // empty: counted, not handed to the sink
        for (int i = 1; i <= 5; ++i) st.push(flush(i, 0, {{"a", 0, 1}}));
        std::string what;
        try {
            st.finish();
        } catch (const std::exception& e) {
            what = e.what();
        }
        CHECK(what == "sink: boom" && calls == 3 && st.flushes == 3 && st.rows == 2);
        st.push(flush(6, 0, {{"a", 0, 1}}));         // returns; nothing reads it
        st.finish();                                 // throws once only
        CHECK(calls == 3);
    }
    calls = 0;
    {
        SinkThread st(sink, [] { return (int64_t)0; });
        for (int i = 0; i < 5; ++i) st.push(flush(i, 0, {{"a", 0, 1}}));
    }   // the destructor swallows the error and does not hang
    CHECK(calls == 3);
}

static void test_clock_and_ring() {
    const ReplayClock c{wall_s() - 5.0, T0, 32.0};   // running: now() truncates downwards
    for (int64_t e : {T0, T0 + 1, T0 + 999, T0 + 123457, T0 + 86400000}) {
        const int64_t back = c.at(c.wallOf(e));      // truncation: within 1 ms of event time
        CHECK(back == e || back == e - 1);
    }
    const double w0 = wall_s(), w = c.wallOf(c.now()), w1 = wall_s();
    CHECK(w <= w1 + 1e-9 && w >= w0 - 1e-3 / 32 - 1e-9);
    CHECK(c.at(c.wall0) == T0 && c.wallOf(T0) == c.wall0);

    const int64_t lo = T0 / 10000 - 8, OOO = 100;
    CHECK(watermark_of(INT64_MIN, OOO) == INT64_MIN && watermark_of(T0, OOO) == T0 - OOO);
    CHECK(!ring_follow(INT64_MIN, lo, 64, OOO));
    CHECK(!ring_follow((lo + 64 - 9) * 10000 + 9999, lo, 64, OOO));   // newest bucket + 8 still inside
    const int64_t mt = (lo + 64 - 8) * 10000;                         // newest bucket + 8 at the ring's end
    CHECK(ring_follow(mt, lo, 64, OOO) == (mt - OOO) / 10000 - 8);
    CHECK(ring_follow(mt + 50, lo, 64, 0) == lo + 64 - 16);
    CHECK(!ring_follow(lo * 10000, lo, 8, OOO));                      // the target would move the base back
    CHECK(!ring_follow((lo + 8) * 10000 + 50, lo, 8, OOO));           // ... or leave it (ooo: one bucket lower)
    CHECK(ring_follow((lo + 9) * 10000 + 500, lo, 8, OOO) == lo + 1);
}

int main() {
    test_layout();
    test_rejections();
    test_rebase();
    test_window_closer();
    test_merge_scripted();
    test_merge_threaded();
    test_sink_errors();
    test_clock_and_ring();
    if (fails) {
        std::printf("%d failure(s)\n", fails);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
