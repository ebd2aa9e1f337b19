// ysb_stream.cpp -- implementation of ysb_stream.hpp (the runner's streaming mode): the GPU
// driving, one context per shard through the C ABI, and the feeders' coordinator.
#include "ysb_stream.hpp"

#include <pthread.h>
#include <sched.h>
#include <time.h>

#include <algorithm>
#include <stdexcept>
#include <thread>

#include "worker_pool.hpp"
#include "ysb_feed_rules.hpp"

namespace ysb {
namespace topology {

namespace {

double thread_cpu_s() {
    timespec ts{};
    clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

constexpr uint64_t GEN_PIECE = 2u << 20;   // events per generator call

void check_ctx(int rc, ysb_ctx* c, const char* what) {
    if (rc != YSB_OK) throw std::runtime_error(std::string(what) + ": " + ysb_last_error(c));
}

// Pins the calling thread to `cpus` (threads it creates inherit the mask); false if it could not.
bool pin_to(const std::vector<int>& cpus) {
    if (cpus.empty()) return false;
    cpu_set_t set;
    CPU_ZERO(&set);
    for (int c : cpus) CPU_SET(c, &set);
    return pthread_setaffinity_np(pthread_self(), sizeof set, &set) == 0;
}

// `bytes` of a context's device memory.
struct DeviceBuf {
    ysb_ctx* ctx;
    void* p = nullptr;
    DeviceBuf(ysb_ctx* c, uint64_t bytes) : ctx(c) { check_ctx(ysb_device_alloc(c, bytes, &p), c, "ysb_device_alloc"); }
    DeviceBuf(const DeviceBuf&) = delete;
    DeviceBuf& operator=(const DeviceBuf&) = delete;
    ~DeviceBuf() { ysb_device_free(ctx, p); }
};

struct CtxClose {
    void operator()(ysb_ctx* c) const { ysb_close(c); }
};

void append_deltas(const std::vector<ysb_count>& rows, uint64_t n, const std::vector<std::string>& campaigns,
                   std::vector<WindowDelta>& out) {
    out.reserve(out.size() + n);
    for (uint64_t i = 0; i < n; ++i) out.push_back({campaigns[rows[i].campaign], rows[i].window_ms, rows[i].count});
}

}  // namespace

unsigned default_threads(const StreamOptions& o) {
    const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    return o.threads ? o.threads : std::max(1u, hw / (unsigned)std::max(1, o.shards));
}

int gpuNumaNode(int device) { return ysb_device_numa_node(device); }

std::vector<int> nodeCpus(int node) {
    std::vector<int> out;
    if (node < 0) return out;
    FILE* f = std::fopen(("/sys/devices/system/node/node" + std::to_string(node) + "/cpulist").c_str(), "r");
    if (!f) return out;
    char buf[4096] = {0};
    const size_t n = std::fread(buf, 1, sizeof buf - 1, f);
    std::fclose(f);
    buf[n] = 0;
    cpu_set_t allowed;
    CPU_ZERO(&allowed);
    if (sched_getaffinity(0, sizeof allowed, &allowed) != 0) return out;
    for (char* p = buf; *p;) {   // "0-23,96-119"
        char* e = nullptr;
        const long a = std::strtol(p, &e, 10);
        if (e == p) break;
        long b = a;
        if (*e == '-') {
            p = e + 1;
            b = std::strtol(p, &e, 10);
        }
        for (long c = a; c <= b && c < CPU_SETSIZE; ++c)
            if (CPU_ISSET((int)c, &allowed)) out.push_back((int)c);
        p = *e == ',' ? e + 1 : e;
        if (*p == '\n') break;
    }
    return out;
}

// Members are destroyed last to first: the device buffer is freed, then the context closed
// (ysb_close unregisters the cycle), then the cycle unmapped.  A shard's feeder thread is
// joined before that (~Feeder, in run()).
struct StreamingJob::Shard {
    int index = 0, device = 0, node = -1;
    std::vector<int> cpus;
    bool pinned = false;
    ysb_gen_params gen{};
    std::vector<uint32_t> subset;
    double prepareS = 0, registerS = 0;
    std::string error;
    ReplayCycle cyc;
    Lz4Cycle z;                           // (--stream-lz4) the cycle compressed: what is registered
    std::unique_ptr<ysb_ctx, CtxClose> ctx;
    std::unique_ptr<DeviceBuf> lineOff;   // (mapped) every line's offset within its batch, in HBM
    uint8_t* slot[2] = {nullptr, nullptr};
    int64_t ringBase = 0;
};

StreamingJob::StreamingJob(const StreamOptions& o) : o_(o) {
    if (o_.cycleMs <= 0 || o_.cycleMs % BUCKET_MS) throw std::runtime_error("the replay cycle must be a multiple of 10 000 ms");
    if (o_.t0Ms % BUCKET_MS) throw std::runtime_error("t0 must be a multiple of 10 000 ms");
    if (o_.shards < 1 || o_.eventRate < 1 || o_.speedup <= 0) throw std::runtime_error("bad stream options");
    if (o_.skew < 0 || o_.skew > 2) throw std::runtime_error("skew must be 0 (off), 1 (skew + late events) or 2 (skew only)");
    if (o_.streamLz4 && o_.replay == StreamOptions::COPY) throw std::runtime_error("a compressed replay is read in place: not with the copy replay");
    if (o_.streamLz4 && (o_.lz4Block < 1 || o_.lz4Block > YSB_LZ4_MAX_RAW)) throw std::runtime_error("the LZ4 block size must be in 1..65536");
}

StreamingJob::~StreamingJob() = default;

void build_cycle(ysb_ctx* ctx, const ysb_gen_params& g, const StreamOptions& o, ReplayCycle& c, WorkerPool& pool) {
    const uint64_t n = (uint64_t)(o.eventRate * (double)o.cycleMs / 1000.0);
    CycleBuilder builder(c);
    const uint64_t maxLine = n ? ysb_gen_max_line_bytes(&g) : 0;
    builder.begin(n, maxLine, g.t0_ms, g.events_per_sec, o.batchMs, o.slotBytes);
    const uint64_t piece = std::min<uint64_t>(n, GEN_PIECE);
    std::unique_ptr<DeviceBuf> d_b, d_o;
    if (ctx) {
        d_b = std::make_unique<DeviceBuf>(ctx, piece * maxLine + 64);
        d_o = std::make_unique<DeviceBuf>(ctx, piece * 4 + 64);
    }
    std::vector<uint8_t> hbuf(piece * maxLine + 64);
    std::vector<uint32_t> off(piece + 1);
    for (uint64_t first = 0; first < n; first += piece) {
        const uint64_t count = std::min(piece, n - first);
        uint64_t nb = 0;
        if (ctx) {
            check_ctx(ysb_gen_events_device(ctx, &g, first, count, (uint8_t*)d_b->p, piece * maxLine, (uint32_t*)d_o->p, &nb),
                      ctx, "ysb_gen_events_device");
            check_ctx(ysb_memcpy_d2h(ctx, hbuf.data(), d_b->p, nb), ctx, "ysb_memcpy_d2h");
            check_ctx(ysb_memcpy_d2h(ctx, off.data(), d_o->p, count * 4), ctx, "ysb_memcpy_d2h");
        } else if (ysb_gen_events_host_mt(&g, first, count, hbuf.data(), hbuf.size(), off.data(), &nb, pool.size()) != YSB_OK) {
            throw std::runtime_error(std::string("ysb_gen_events_host_mt: ") + ysb_last_error(nullptr));
        }
        off[count] = (uint32_t)nb;
        builder.add(first, count, hbuf.data(), off.data(), pool);
    }
    builder.finish(pool);
}

ysb_gen_params shard_gen(const StreamOptions& o, uint32_t stream) {
    ysb_gen_params g;
    ysb_gen_default(&g);
    g.seed = o.seed;
    g.n_campaigns = o.campaigns;
    g.ads_per_campaign = o.adsPerCampaign;
    g.t0_ms = o.t0Ms;
    g.events_per_sec = (uint64_t)o.eventRate;
    g.with_skew = (uint32_t)o.skew;
    g.event_stream = stream;
    return g;
}

void StreamingJob::prepare() {
    ysb_gen_params g = shard_gen(o_, 0);
    std::vector<char> cid(36ull * o_.campaigns), aid(36ull * o_.campaigns * o_.adsPerCampaign);
    if (ysb_gen_ids(&g, cid.data(), aid.data()) != YSB_OK) throw std::runtime_error("ysb_gen_ids failed");
    const uint64_t A = (uint64_t)o_.campaigns * o_.adsPerCampaign;
    for (uint32_t c = 0; c < o_.campaigns; ++c) campaigns_.emplace_back(&cid[36ull * c], 36);
    for (uint64_t a = 0; a < A; ++a) ads_.emplace_back(&aid[36 * a], 36);
    const int ndev = std::max(1, ysb_device_count());
    std::vector<const char*> keys(A);
    std::vector<uint32_t> camp(A);
    for (uint64_t a = 0; a < A; ++a) {
        keys[a] = ads_[a].data();
        camp[a] = (uint32_t)(a / o_.adsPerCampaign);
    }
    for (int s = 0; s < o_.shards; ++s) {
        shards_.push_back(std::make_unique<Shard>());
        Shard& sh = *shards_.back();
        sh.index = s;
        sh.device = (o_.device + s) % ndev;
        sh.node = gpuNumaNode(sh.device);
        if (o_.pinNuma) sh.cpus = nodeCpus(sh.node);
    }
    // every shard prepared on a thread of its own, on its GPU's NUMA node
    std::vector<std::thread> th;
    for (auto& sh : shards_)
        th.emplace_back([&, s = sh.get()] {
            try {
                prepareShard(*s, keys, camp);
            } catch (const std::exception& e) {
                s->error = e.what();
            }
        });
    for (auto& t : th) t.join();
    for (auto& sh : shards_)
        if (!sh->error.empty()) throw std::runtime_error("shard " + std::to_string(sh->index) + ": " + sh->error);
}

// The shard's context, its cycle (generated on its GPU, its pages first touched on the calling
// thread's node: pinned before the pool is created, whose threads inherit the mask), the cycle
// registered with the context.
void StreamingJob::prepareShard(Shard& sh, const std::vector<const char*>& keys, const std::vector<uint32_t>& camp) {
    const double t0 = wall_s();
    sh.pinned = pin_to(sh.cpus);
    WorkerPool pool(default_threads(o_));
    ysb_config cfg;
    ysb_config_default(&cfg);
    cfg.n_campaigns = o_.campaigns;
    cfg.window_ring = o_.windowRing;
    cfg.max_batch_bytes = o_.slotBytes;
    cfg.max_batch_events = o_.slotBytes / 64;
    cfg.ring_base_bucket = o_.t0Ms / BUCKET_MS - 8;
    cfg.flags = o_.timing ? YSB_F_TIMING : 0u;
    ysb_ctx* ctx = nullptr;
    if (ysb_open(&ctx, sh.device, &cfg) != YSB_OK) throw std::runtime_error(std::string("ysb_open: ") + ysb_last_error(nullptr));
    sh.ctx.reset(ctx);
    sh.ringBase = cfg.ring_base_bucket;
    check_ctx(ysb_load_ad_map(ctx, keys.data(), nullptr, camp.data(), keys.size()), ctx, "ysb_load_ad_map");
    for (int k = 0; k < 2; ++k) check_ctx(ysb_slot_buffers(ctx, k, &sh.slot[k], nullptr), ctx, "ysb_slot_buffers");
    // the shard's own event stream over its ad_id shard (ysb_ad_shard), as bench.py's ranks
    sh.gen = shard_gen(o_, 1 + (uint32_t)sh.index);
    if (o_.shards > 1) {
        for (uint64_t a = 0; a < ads_.size(); ++a)
            if (ysb_ad_shard(ads_[a].data(), 36, (uint32_t)o_.shards) == (uint32_t)sh.index) sh.subset.push_back((uint32_t)a);
        sh.gen.ad_subset = sh.subset.data();
        sh.gen.n_ad_subset = (uint32_t)sh.subset.size();
    }
    build_cycle(ctx, sh.gen, o_, sh.cyc, pool);
    // --stream-lz4: every batch compressed on its own on the shard's pool (its pages on this node)
    if (o_.streamLz4) compress_cycle(sh.cyc, o_.lz4Block, sh.z, pool);
    const double t1 = wall_s();
    if (o_.replay != StreamOptions::COPY) {
        // the compressed cycle is registered, the raw one is not
        uint8_t* const base = o_.streamLz4 ? sh.z.bytes : sh.cyc.bytes;
        const uint64_t used = o_.streamLz4 ? sh.z.used : sh.cyc.used;
        check_ctx(ysb_host_register(ctx, base, (used + 4095) / 4096 * 4096), ctx, "ysb_host_register");
        check_ctx(ysb_rebase_table(ctx, sh.cyc.timeAt.data(), sh.cyc.lines(), sh.cyc.upperMin), ctx, "ysb_rebase_table");
    }
    if (o_.replay == StreamOptions::MAPPED) {   // the line offsets, once for every cycle
        std::vector<uint32_t> lo(sh.cyc.lines());
        for (const auto& b : sh.cyc.batches)
            for (uint64_t i = b.a; i < b.b; ++i) lo[i] = (uint32_t)(sh.cyc.start[i] - b.off);
        sh.lineOff = std::make_unique<DeviceBuf>(ctx, lo.size() * 4 + 64);
        check_ctx(ysb_memcpy_h2d(ctx, sh.lineOff->p, lo.data(), lo.size() * 4), ctx, "ysb_memcpy_h2d");
    }
    // the raw lines are not needed again: the line offsets and the rebase table are on the device
    if (o_.streamLz4) sh.cyc.releaseBytes();
    sh.registerS = wall_s() - t1;
    sh.prepareS = wall_s() - t0;
}

// One feeder per shard, on a thread of its own that owns the shard's context: it releases the
// shard's batches on the replay clock, begins and takes the shard's flushes (at most 4
// outstanding), and moves the shard's ring.
class StreamingJob::Feeder {
public:
    Feeder(Shard& s, const StreamOptions& o, FeedControl& ctl, FlushMerger& merger, const std::vector<std::string>& campaigns)
        : s_(s), ctx_(s.ctx.get()), o_(o), ctl_(ctl), merger_(merger), campaigns_(campaigns), ringLo_(s.ringBase) {}
    ~Feeder() {
        if (!th_.joinable()) return;
        ctl_.failed = true;   // (the coordinator is unwinding: no final flush)
        ctl_.stop = true;
        th_.join();
    }
    void start() { th_ = std::thread([this] { run(); }); }
    void join() { th_.join(); }
    int64_t watermark() const { return watermark_of(maxTime_, o_.oooMs); }

    std::atomic<bool> synced{false};
    std::string error;
    uint64_t cycle = 0, next = 0;    // the next batch: cyc.batches[next] of cycle `cycle`
    uint64_t events = 0, batches = 0, ringAdvances = 0, slowSubmits = 0;
    double submitMs = 0, slowMs = 0, slowMaxMs = 0, maxBehindMs = 0, cpuS = 0;
    double firstSubmit = 0, lastSubmit = 0, doneAt = 0;

private:
    Shard& s_;
    ysb_ctx* const ctx_;
    const StreamOptions& o_;
    FeedControl& ctl_;
    FlushMerger& merger_;
    const std::vector<std::string>& campaigns_;
    std::unique_ptr<WorkerPool> pool_;
    int cur_ = 0;
    int64_t maxTime_ = INT64_MIN;
    std::deque<std::pair<int64_t, int64_t>> flushes_;   // outstanding: (flush index, watermark at its begin)
    int64_t flushBegun_ = 0, ringLo_;
    std::thread th_;

    void check(int rc, const char* what) const { check_ctx(rc, ctx_, what); }
    // the wall time the next batch is due at
    double dueWall() const { return ctl_.clock.wallOf(s_.cyc.batches[next].releaseMs + (int64_t)cycle * o_.cycleMs); }
    bool submitNext();
    void beginFlushes();
    void takeFlushes(bool wait);
    void followRing();
    void run();
};

// Submits the next batch if it is due and the input has not stopped; false if it did not.
bool StreamingJob::Feeder::submitNext() {
    const double w = wall_s(), due = dueWall();
    if (w < due || w >= ctl_.stopAt) return false;
    const ReplayCycle::Batch& b = s_.cyc.batches[next];
    maxBehindMs = std::max(maxBehindMs, (w - due) * 1e3);
    const double t0 = wall_s();
    const ysb_rebase rb{b.a, (int64_t)cycle * (o_.cycleMs / BUCKET_MS)};
    if (o_.streamLz4) {   // the batch's blocks in place; mapped: the cycle's HBM line offsets, mapped-raw: the GPU split
        const Lz4Cycle::Batch& zb = s_.z.batches[next];
        const bool offs = o_.replay == StreamOptions::MAPPED;
        check(ysb_submit_lz4_mapped(ctx_, cur_, s_.z.bytes + zb.off, zb.nbytes, s_.z.dir.data() + zb.firstBlock,
                                    (uint32_t)zb.blocks, offs ? (uint32_t*)s_.lineOff->p + b.a : nullptr,
                                    offs ? b.b - b.a : 0, &rb),
              "ysb_submit_lz4_mapped");
    } else if (o_.replay == StreamOptions::MAPPED) {
        check(ysb_submit_mapped(ctx_, cur_, s_.cyc.bytes + b.off, b.nbytes, (uint32_t*)s_.lineOff->p + b.a, b.b - b.a, &rb),
              "ysb_submit_mapped");
    } else if (o_.replay == StreamOptions::MAPPED_RAW) {
        check(ysb_submit_raw_mapped(ctx_, cur_, s_.cyc.bytes + b.off, b.nbytes, &rb), "ysb_submit_raw_mapped");
    } else {
        check(ysb_wait(ctx_, cur_), "ysb_wait");   // the slot's last copy is done
        const uint64_t nb = fill_batch(s_.cyc, b, cycle, o_.cycleMs, s_.slot[cur_], *pool_, pool_->size());
        check(ysb_submit_raw(ctx_, cur_, s_.slot[cur_], nb), "ysb_submit_raw");
    }
    const double t1 = wall_s(), dt = (t1 - t0) * 1e3;
    submitMs += dt;
    if (dt > 1.0) {
        ++slowSubmits;
        slowMs += dt;
        slowMaxMs = std::max(slowMaxMs, dt);
    }
    if (!firstSubmit) firstSubmit = t0;
    lastSubmit = t1;
    maxTime_ = std::max(maxTime_, b.maxTimeMs + (int64_t)cycle * o_.cycleMs);
    events += b.b - b.a;
    ++batches;
    cur_ ^= 1;
    if (++next == s_.cyc.batches.size()) {
        next = 0;
        ++cycle;
    }
    return true;
}

void StreamingJob::Feeder::beginFlushes() {
    const int64_t want = ctl_.flushReq.load();
    while (flushBegun_ < want) {
        if (flushes_.size() == 4) takeFlushes(true);   // at most 4 outstanding: the oldest first
        check(ysb_flush_begin(ctx_, INT64_MIN, INT64_MAX), "ysb_flush_begin");
        flushes_.push_back({flushBegun_++, watermark()});
    }
}

void StreamingJob::Feeder::takeFlushes(bool wait) {
    while (!flushes_.empty()) {
        uint64_t n = 0;
        int more = 0;
        const int rc = ysb_flush_end(ctx_, wait ? 1 : 0, nullptr, 0, &n, &more);
        if (rc == YSB_PENDING) break;
        check(rc, "ysb_flush_end");
        std::vector<ysb_count> rows(std::max<uint64_t>(n, 1));
        check(ysb_flush_end(ctx_, 1, rows.data(), n, &n, &more), "ysb_flush_end");
        std::vector<WindowDelta> d;
        append_deltas(rows, n, campaigns_, d);
        merger_.deliver(flushes_.front().first, flushes_.front().second, std::move(d));
        flushes_.pop_front();
    }
}

// A synchronous move of the ring (rare), after taking the outstanding flushes.
void StreamingJob::Feeder::followRing() {
    const std::optional<int64_t> lo = ring_follow(maxTime_, ringLo_, o_.windowRing, o_.oooMs);
    if (!lo) return;
    takeFlushes(true);
    check(ysb_ring_advance(ctx_, *lo), "ysb_ring_advance");
    ringLo_ = *lo;
    ++ringAdvances;
}

void StreamingJob::Feeder::run() {
    const double cpu0 = thread_cpu_s();
    try {
        pin_to(s_.cpus);   // before the pool: its threads inherit the mask
        pool_ = std::make_unique<WorkerPool>(o_.replay == StreamOptions::COPY ? default_threads(o_) : 1u);
        ysb_copy_time(ctx_, nullptr, nullptr, nullptr);   // reset the copy timing
        check(ysb_wait(ctx_, 0), "ysb_wait");
        while (!ctl_.stop.load()) {
            const bool any = submitNext();
            beginFlushes();
            takeFlushes(false);
            followRing();
            if (!any) {
                // sleep until the next batch is due (at most 200 us: flushes to begin / take)
                const double nd = dueWall() - wall_s();
                if (nd > 20e-6) std::this_thread::sleep_for(std::chrono::microseconds((int64_t)std::min(200.0, nd * 1e6 - 10)));
            }
        }
        // end of input: every batch counted, then the final flush the coordinator asks for
        check(ysb_sync(ctx_), "ysb_sync");
        doneAt = wall_s();
        synced = true;
        while (!ctl_.final.load() && !ctl_.failed.load()) std::this_thread::sleep_for(std::chrono::microseconds(100));
        if (!ctl_.failed.load()) {
            beginFlushes();
            takeFlushes(true);
        }
    } catch (const std::exception& e) {
        error = e.what();
        ctl_.failed = true;
        synced = true;
    }
    cpuS = thread_cpu_s() - cpu0;
}

// The coordinator: start the feeders, tick the flusher, stop, final flush, drain, report.
StreamReport StreamingJob::run(const FlushSink& sink) {
    FeedControl ctl;
    ctl.clock = ReplayClock{wall_s() + 0.1, o_.t0Ms, o_.speedup};   // starts 100 ms from now (feeders started)
    ctl.stopAt = ctl.clock.wall0 + o_.seconds;
    SinkThread st(sink, [&ctl] { return ctl.clock.now(); });
    FlushMerger merger(st, (int)shards_.size());
    std::vector<std::unique_ptr<Feeder>> feeders;
    for (auto& s : shards_) feeders.push_back(std::make_unique<Feeder>(*s, o_, ctl, merger, campaigns_));
    for (auto& f : feeders) f->start();

    // the flusher's clock (CampaignProcessorCommon.java:45: every flushMs)
    int64_t nextFlush = o_.t0Ms + o_.flushMs;
    while (wall_s() < ctl.stopAt && !ctl.failed.load()) {
        if (ctl.clock.now() >= nextFlush) {
            ++ctl.flushReq;
            nextFlush += o_.flushMs;
        }
        std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
    ctl.stop = true;
    for (auto& f : feeders)
        while (!f->synced.load()) std::this_thread::sleep_for(std::chrono::microseconds(100));
    ++ctl.flushReq;   // the last flush: everything submitted
    ctl.final = true;
    for (auto& f : feeders) f->join();
    for (size_t i = 0; i < feeders.size(); ++i)
        if (!feeders[i]->error.empty()) throw std::runtime_error("shard " + std::to_string(i) + ": " + feeders[i]->error);
    if (!merger.empty()) throw std::runtime_error("a flush was not delivered by every shard");

    // a drain for anything outside the ring (the side list); the watermark stays where the input stopped
    FlushRows last;
    last.index = ctl.flushReq.load();
    last.watermarkMs = INT64_MAX;
    for (size_t i = 0; i < feeders.size(); ++i) {
        ysb_ctx* ctx = shards_[i]->ctx.get();
        last.watermarkMs = std::min(last.watermarkMs, feeders[i]->watermark());
        uint64_t n = 0;
        check_ctx(ysb_drain(ctx, INT64_MIN, INT64_MAX, 0, nullptr, 0, &n), ctx, "ysb_drain");
        std::vector<ysb_count> rows(std::max<uint64_t>(n, 1));
        check_ctx(ysb_drain(ctx, INT64_MIN, INT64_MAX, 1, rows.data(), n, &n), ctx, "ysb_drain");
        append_deltas(rows, n, campaigns_, last.rows);
    }
    const int64_t finalWm = last.watermarkMs;
    st.push(std::move(last));
    st.finish();
    StreamReport rep = report(feeders, st);
    rep.finalWatermarkMs = finalWm;
    return rep;
}

StreamReport StreamingJob::report(const std::vector<std::unique_ptr<Feeder>>& feeders, const SinkThread& st) const {
    StreamReport rep;
    rep.linesPerCycle = shards_[0]->cyc.lines();
    double first = 0, lastSubmit = 0, done = 0;
    for (size_t i = 0; i < feeders.size(); ++i) {
        const Shard& s = *shards_[i];
        const Feeder& f = *feeders[i];
        ShardReport sr;
        sr.device = s.device;
        sr.numaNode = s.node;
        sr.pinned = s.pinned;
        sr.events = f.events;
        sr.batches = f.batches;
        sr.cycles = f.cycle;
        sr.partialLines = f.next ? s.cyc.batches[f.next].a : 0;
        sr.submitMs = f.submitMs;
        sr.feederCpuS = f.cpuS;
        sr.maxBehindMs = f.maxBehindMs;
        sr.ringAdvances = f.ringAdvances;
        sr.replayGB = (double)(o_.streamLz4 ? s.z.used : s.cyc.used) / 1e9;   // what is resident
        rep.lz4CompBytesPerCycle += s.z.compBytes;
        rep.lz4RawBytesPerCycle += s.z.rawBytes;
        rep.lz4BlocksPerCycle += s.z.dir.size();
        sr.prepareS = s.prepareS;
        sr.registerS = s.registerS;
        rep.shards.push_back(sr);
        rep.events += f.events;
        rep.batches += f.batches;
        rep.cycles.push_back(f.cycle);
        rep.partialLines.push_back(sr.partialLines);
        rep.slotWaits += f.slowSubmits;
        rep.slotWaitMs += f.slowMs;
        rep.slotWaitMaxMs = std::max(rep.slotWaitMaxMs, f.slowMaxMs);
        rep.maxBehindMs = std::max(rep.maxBehindMs, f.maxBehindMs);
        rep.ringAdvances += f.ringAdvances;
        if (f.firstSubmit && (!first || f.firstSubmit < first)) first = f.firstSubmit;
        lastSubmit = std::max(lastSubmit, f.lastSubmit);
        done = std::max(done, f.doneAt);
        double ms = 0;
        uint64_t copies = 0, bytes = 0;
        check_ctx(ysb_copy_time(s.ctx.get(), &ms, &copies, &bytes), s.ctx.get(), "ysb_copy_time");
        rep.copyMs += ms;
        rep.copyBytes += bytes;
        ysb_stats x;
        check_ctx(ysb_stats_get(s.ctx.get(), &x), s.ctx.get(), "ysb_stats_get");
        rep.overflowDropped += x.overflow_dropped;
        rep.parseErrors += x.parse_errors;
        rep.joinMisses += x.join_misses;
    }
    // every submitted event counted, from the first submit to the last shard's ysb_sync
    rep.wallSeconds = first ? done - first : 0;
    rep.eventsPerSecond = rep.wallSeconds > 0 ? (double)rep.events / rep.wallSeconds : 0;
    rep.submitEventsPerSecond = lastSubmit > first ? (double)rep.events / (lastSubmit - first) : 0;
    rep.targetEventsPerSecond = o_.eventRate * o_.speedup * (double)shards_.size();
    rep.copyGBs = rep.copyMs > 0 ? (double)rep.copyBytes / (rep.copyMs * 1e-3) / 1e9 : 0;
    rep.copyBusyFrac = rep.wallSeconds > 0 ? rep.copyMs * 1e-3 / rep.wallSeconds / (double)shards_.size() : 0;
    {   // measured when the copies were timed, the cycle's own figure otherwise
        uint64_t cyc_bytes = 0, cyc_lines = 0;
        for (const auto& s : shards_) {
            cyc_lines += s->cyc.lines();
            if (o_.streamLz4) cyc_bytes += s->z.compBytes;
            else for (const auto& b : s->cyc.batches) cyc_bytes += b.nbytes;
        }
        rep.pcieBytesPerEvent = rep.copyBytes && rep.events ? (double)rep.copyBytes / (double)rep.events
                                                            : cyc_lines ? (double)cyc_bytes / (double)cyc_lines : 0;
    }
    rep.flushes = st.flushes;
    rep.rowsWritten = st.rows;
    rep.closeReplayMs = st.windows.closeMs;
    rep.cwReplayMs = st.windows.cwMs;
    rep.openAtEnd = st.windows.seen.size() - st.windows.closed.size();
    return rep;
}

}  // namespace topology
}  // namespace ysb
