// ysb_topology -- the native drop-in for `flink run ... AdvertisingTopologyNative
// --confPath conf/benchmarkConf.yaml` (flink-benchmarks/.../AdvertisingTopologyNative.java:
// 58-142): reads the same YAML keys, the same ad map and events files, runs the chain on
// one GPU, and writes the (campaign, window) counts to Redis in the reference's schema
// (or to a CSV file).
//
//   ysb_topology --confPath PATH --columns [--device N] [--format json|tbl] [--require-ip]
//   ysb_topology --confPath PATH --from-columns [--device N] [--sink ...] [--window-ring W]
//   ysb_topology --confPath PATH [--device N] [--sink none|csv:FILE|redis[:HOST[:PORT]]]
//                [--format json|tbl] [--flush-ms MS] [--batch-mb MB | --batch-bytes B] [--batch-events N]
//                [--window-ring W] [--require-ip] [--dry-run] [--print-config]
//                [--replay-rows CSV] [--host-split] [--repeat K] [--io-threads T] [--io mmap|pread]
//
// --dry-run reads the config, the map and the events file (FileBasedDataSource) without a
// GPU and reports what it found; --replay-rows writes the (campaign_id,window_ms,count)
// rows of a CSV through the sink without a GPU (the Redis writer on its own).  The events
// file is read as raw lines and the GPU finds the line starts (ysb_submit_raw); --host-split
// splits the lines on the host instead (ysb_submit with offsets).  --repeat K reads the file
// K times (a replay source; the counts are K times the file's).  --lz4 reads events_path as a
// compressed replay file through the slots; --lz4 --io mapped maps it instead and hands runs of
// its blocks over where they lie (ysb_submit_lz4_mapped); a standard LZ4 frame file (ysb_gen
// --lz4-frame, lz4 -B4 -BI) is told by its magic and fed with ysb_submit_lz4_blocks(_mapped).  The last stdout line is a JSON
// summary.
#include <algorithm>
#include <chrono>
#include <memory>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ysb_stream.hpp"
#include "ysb_topology.hpp"

using namespace ysb::topology;

namespace {

struct Args {
    std::string conf, sink = "none", format, replay;
    int device = 0;
    long long flush_ms = 1000;                  // CampaignProcessorCommon's flusher period (:45)
    long long batch_bytes = 256ll << 20, batch_events = 1 << 20;
    unsigned window_ring = 1024;
    bool require_ip = false, dry = false, print_config = false, host_split = false;
    bool columns = false;                       // --columns: the columnar chain (:106-109)
    bool from_columns = false;                  // --from-columns: count <shared_file>_<k> images
    long long repeat = 1;
    unsigned io_threads = 0;
    bool io_mmap = true;
    // --io mapped: the mapping registered, batches read in place by the GPU; auto (the default):
    // that whenever the GPU splits the lines and the slots' copy is the copy kernel's, with
    // slot copies out of the mapping if the registration is refused
    std::string io = "auto";
    bool h2d_sdma = false;
    // --join-redis: the join as a cache in front of Redis (RedisAdCampaignCache): views of ads the
    // map does not hold are parked, looked up with GET after each batch, upserted and resolved
    bool join_redis = false;
    long long park_capacity = 1 << 20;
    // --lz4: events_path is a compressed replay file (ysb_gen --lz4): runs of whole LZ4 blocks go
    // over PCIe as they are and are decoded on the GPU (ysb_submit_raw_lz4)
    bool lz4 = false;
    // --kafka: events_path is a partition's log segment (ysb_gen --kafka): runs of whole record
    // batches go over PCIe framed and are unframed on the GPU (ysb_submit_kafka)
    bool kafka = false;
    // --kafka-codec lz4: the segment's batches may be LZ4-compressed (attributes codec 3; ysb_gen
    // --kafka --kafka-codec lz4): inflated on the GPU in front of the unframing (ysb_submit_kafka_lz4).
    // --kafka-codec snappy: they may be snappy too (codec 2; ysb_gen --kafka --kafka-codec snappy), in
    // either framing: ysb_kafka_index_lz4 with YSB_KAFKA_ACCEPT_SNAPPY and ysb_kafka_set_codecs.
    // Without it a compressed segment is refused, as before.
    std::string kafka_codec;
    // --kafka-check-crc device|host|off: every data batch's CRC-32C verified on the GPU in front of
    // its records (ysb_kafka_set_crc; the control batches the index skips on the host), or all of
    // them on the host at index time (a pass over the bytes), or not at all (the default)
    std::string kafka_check_crc = "off";
    // streaming mode (configs[4]): --stream plus its options (ysb_stream.hpp)
    bool stream = false;
    StreamOptions so;
    std::string stream_csv;   // per-(campaign, window) totals of everything written
    bool self_check = false;  // --stream-self-check: the replay's rebasing on the CPU, no GPU
    bool feed_check = false;  // --stream-feed-check: the feeders' host rate on the CPU, no GPU
    bool merge_check = false; // --stream-merge-check: the shards' flush merge on the CPU, no GPU
    int merge_flushes = 400;
    double feed_seconds = 2;
};

void usage() {
    std::fprintf(stderr,
                 "usage: ysb_topology --confPath PATH [--device N] [--sink none|csv:FILE|redis[:HOST[:PORT]]]\n"
                 "       [--format json|tbl] [--flush-ms MS] [--batch-mb MB | --batch-bytes B] [--batch-events N]\n"
                 "       [--window-ring W] [--require-ip] [--dry-run] [--print-config] [--replay-rows CSV]\n"
                 "       [--host-split] [--repeat K] [--io-threads T] [--io auto|mapped|mmap|pread]\n"
                 "       [--h2d-sdma] [--join-redis [--park-capacity N]] [--lz4] [--kafka [--kafka-codec lz4|snappy]\n"
                 "       [--kafka-check-crc device|host|off]]\n"
                 "   or: ysb_topology --confPath PATH --columns [--device N] [--format json|tbl] [--require-ip]\n"
                 "       [--batch-mb MB | --batch-bytes B]   (window.size rows per <shared_file>_<k>)\n"
                 "   or: ysb_topology --confPath PATH --from-columns [--device N] [--sink none|csv:FILE|redis[:HOST[:PORT]]]\n"
                 "                    [--window-ring W]\n"
                 "   or: ysb_topology --stream [--sink none|csv:FILE|redis[:HOST[:PORT]]] [--shards N] [--device D]\n"
                 "       [--seed S] [--campaigns C] [--ads-per-campaign A] [--event-rate E] [--speedup F]\n"
                 "       [--cycle-ms MS] [--flush-ms MS] [--batch-ms MS] [--ooo-ms MS] [--seconds S]\n"
                 "       [--batch-mb MB] [--window-ring W] [--skew 0|1|2] [--io-threads T] [--totals CSV]\n"
                 "       [--replay mapped|mapped-raw|copy] [--no-numa] [--no-timing] [--stream-lz4 [--lz4-block N]]\n"
                 "   or: ysb_topology --stream-self-check | --stream-feed-check [--shards N] [--feed-seconds S] ...\n"
                 "   or: ysb_topology --stream-merge-check [--shards N] [--merge-flushes F] [--seed S]\n");
}

Args parse(int argc, char** argv) {
    Args a;
    for (int i = 1; i < argc; ++i) {
        const std::string k = argv[i];
        auto val = [&]() -> std::string {
            if (i + 1 >= argc) { usage(); std::exit(2); }
            return argv[++i];
        };
        if (k == "--confPath") a.conf = val();
        else if (k == "--device") a.device = std::atoi(val().c_str());
        else if (k == "--sink") a.sink = val();
        else if (k == "--format") a.format = val();
        else if (k == "--flush-ms") a.flush_ms = std::atoll(val().c_str());
        else if (k == "--batch-mb") a.batch_bytes = (long long)std::atoll(val().c_str()) << 20;
        else if (k == "--batch-bytes") a.batch_bytes = std::atoll(val().c_str());
        else if (k == "--batch-events") a.batch_events = std::atoll(val().c_str());
        else if (k == "--window-ring") a.window_ring = (unsigned)std::atoll(val().c_str());
        else if (k == "--require-ip") a.require_ip = true;
        else if (k == "--dry-run") a.dry = true;
        else if (k == "--print-config") a.print_config = true;
        else if (k == "--replay-rows") a.replay = val();
        else if (k == "--host-split") a.host_split = true;
        else if (k == "--repeat") a.repeat = std::max(1ll, std::atoll(val().c_str()));
        else if (k == "--io-threads") a.io_threads = (unsigned)std::atoll(val().c_str());
        else if (k == "--io") {
            const std::string m = val();
            if (m != "mmap" && m != "pread" && m != "mapped" && m != "auto") { usage(); std::exit(2); }
            a.io_mmap = m != "pread";
            a.io = m;
        }
        else if (k == "--h2d-sdma") a.h2d_sdma = true;
        else if (k == "--join-redis") a.join_redis = true;
        else if (k == "--park-capacity") a.park_capacity = std::max(1ll, std::atoll(val().c_str()));
        else if (k == "--lz4") a.lz4 = true;
        else if (k == "--kafka") a.kafka = true;
        else if (k == "--kafka-check-crc") {
            a.kafka_check_crc = val();
            if (a.kafka_check_crc != "device" && a.kafka_check_crc != "host" && a.kafka_check_crc != "off") {
                std::fprintf(stderr, "--kafka-check-crc %s: device, host or off\n", a.kafka_check_crc.c_str());
                std::exit(2);
            }
        } else if (k == "--kafka-codec") {
            a.kafka_codec = val();
            if (a.kafka_codec != "lz4" && a.kafka_codec != "snappy") {
                std::fprintf(stderr, "--kafka-codec %s: lz4 and snappy are the codecs that are read (gzip and zstd are not)\n",
                             a.kafka_codec.c_str());
                std::exit(2);
            }
        }
        else if (k == "--columns") a.columns = true;
        else if (k == "--from-columns") a.from_columns = true;
        else if (k == "--stream") a.stream = true;
        else if (k == "--stream-self-check") { a.stream = true; a.self_check = true; }
        else if (k == "--shards") a.so.shards = std::atoi(val().c_str());
        else if (k == "--seed") a.so.seed = std::strtoull(val().c_str(), nullptr, 10);
        else if (k == "--campaigns") a.so.campaigns = (uint32_t)std::atoll(val().c_str());
        else if (k == "--ads-per-campaign") a.so.adsPerCampaign = (uint32_t)std::atoll(val().c_str());
        else if (k == "--event-rate") a.so.eventRate = std::atof(val().c_str());
        else if (k == "--speedup") a.so.speedup = std::atof(val().c_str());
        else if (k == "--cycle-ms") a.so.cycleMs = std::atoll(val().c_str());
        else if (k == "--batch-ms") a.so.batchMs = std::atoll(val().c_str());
        else if (k == "--ooo-ms") a.so.oooMs = std::atoll(val().c_str());
        else if (k == "--seconds") a.so.seconds = std::atof(val().c_str());
        else if (k == "--skew") a.so.skew = std::atoi(val().c_str());
        else if (k == "--totals") a.stream_csv = val();
        else if (k == "--stream-feed-check") { a.stream = true; a.feed_check = true; }
        else if (k == "--feed-seconds") a.feed_seconds = std::atof(val().c_str());
        else if (k == "--stream-merge-check") { a.stream = true; a.merge_check = true; }
        else if (k == "--merge-flushes") a.merge_flushes = std::atoi(val().c_str());
        else if (k == "--no-numa") a.so.pinNuma = false;
        else if (k == "--no-timing") a.so.timing = false;
        else if (k == "--stream-lz4") a.so.streamLz4 = true;
        else if (k == "--lz4-block") {
            const long long n = std::atoll(val().c_str());
            if (n < 1 || n > (long long)YSB_LZ4_MAX_RAW) {
                std::fprintf(stderr, "--lz4-block must be in 1..65536\n");
                std::exit(2);
            }
            a.so.lz4Block = (uint32_t)n;
        }
        else if (k == "--replay") {
            const std::string m = val();
            if (m != "mapped" && m != "mapped-raw" && m != "copy") { usage(); std::exit(2); }
            a.so.replay = m == "mapped" ? StreamOptions::MAPPED : m == "mapped-raw" ? StreamOptions::MAPPED_RAW
                                                                                    : StreamOptions::COPY;
        }
        else { usage(); std::exit(2); }
    }
    if (a.join_redis && (a.stream || a.columns || a.from_columns)) {
        std::fprintf(stderr, "--join-redis is batch mode's (the counting chain over events_path): not with --stream, "
                             "--columns or --from-columns\n");
        std::exit(2);
    }
    if (a.so.streamLz4 && !a.stream) {
        std::fprintf(stderr, "--stream-lz4 compresses the streaming replay's cycle: only with --stream\n");
        std::exit(2);
    }
    if (a.so.streamLz4 && a.so.replay == StreamOptions::COPY) {
        std::fprintf(stderr, "--stream-lz4 is read in place from the registered cycle: not with --replay copy "
                             "(--replay mapped or mapped-raw)\n");
        std::exit(2);
    }
    if (a.kafka && (a.stream || a.columns || a.from_columns || a.lz4 || a.host_split)) {
        std::fprintf(stderr, "--kafka reads events_path as a log segment of record batches in batch mode: not with --stream, "
                             "--columns, --from-columns, --lz4 or --host-split\n");
        std::exit(2);
    }
    if (a.kafka_check_crc != "off" && !a.kafka) {
        std::fprintf(stderr, "--kafka-check-crc verifies a log segment's batches: only with --kafka\n");
        std::exit(2);
    }
    if (!a.kafka_codec.empty() && !a.kafka) {
        std::fprintf(stderr, "--kafka-codec names the codec of a log segment's batches: only with --kafka\n");
        std::exit(2);
    }
    if (a.lz4 && a.stream) {
        std::fprintf(stderr, "--lz4 reads events_path as a compressed replay file in batch mode: not with --stream\n");
        std::exit(2);
    }
    if (a.lz4 && a.columns) {
        std::fprintf(stderr, "--lz4 feeds the counting chain: not with --columns (the columnar decode reads plain lines)\n");
        std::exit(2);
    }
    if (a.lz4 && a.from_columns) {
        std::fprintf(stderr, "--lz4 feeds the counting chain: not with --from-columns (column images are not compressed)\n");
        std::exit(2);
    }
    if (a.stream && a.columns) {
        std::fprintf(stderr, "--columns reads events_path in batch mode: not with --stream\n");
        std::exit(2);
    }
    if (a.from_columns && (a.stream || a.columns)) {
        std::fprintf(stderr, "--from-columns counts the images --columns wrote: not with --stream or --columns\n");
        std::exit(2);
    }
    if (a.stream) {   // the generator's ids and events: no config file needed
        a.so.device = a.device;
        a.so.flushMs = a.flush_ms;
        a.so.slotBytes = (uint64_t)a.batch_bytes;
        a.so.windowRing = a.window_ring == 1024 ? 64 : a.window_ring;
        a.so.threads = a.io_threads;
        return a;
    }
    if (a.conf.empty()) {   // ParameterTool.getRequired("confPath")
        std::fprintf(stderr, "No data for required key 'confPath'\n");
        std::exit(2);
    }
    return a;
}

std::string json_str(const std::string& s) {
    std::string o = "\"";
    for (char c : s) {
        if (c == '"' || c == '\\') o += '\\';
        if ((unsigned char)c < 0x20) { char b[8]; std::snprintf(b, sizeof b, "\\u%04x", c); o += b; continue; }
        o += c;
    }
    return o + "\"";
}

double now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// --sink none | csv:FILE | redis[:HOST[:PORT]] (the host defaults to the config's redis.host);
// false (after the usage text) for anything else.
// The job's Redis: the conf's redis.host (Utils.java), port 6379, unless --sink redis:HOST[:PORT]
// names another (the sink and --join-redis talk to the same server, as the reference's bolts do).
void redis_address(const Args& a, const Config& conf, std::string* host, int* port) {
    *host = conf.get("redis.host", "localhost");
    *port = 6379;
    const std::string rest = a.sink.rfind("redis", 0) == 0 && a.sink.size() > 6 ? a.sink.substr(6) : "";
    if (!rest.empty()) {
        const size_t c = rest.rfind(':');
        *host = c == std::string::npos ? rest : rest.substr(0, c);
        if (c != std::string::npos) *port = std::atoi(rest.c_str() + c + 1);
    }
}

bool open_sink(const Args& a, const Config& conf, std::unique_ptr<RedisWindowWriter>& redis, std::string& csv_path) {
    if (a.sink.rfind("redis", 0) == 0) {
        std::string host;
        int port;
        redis_address(a, conf, &host, &port);
        redis.reset(new RedisWindowWriter(host, port));
    } else if (a.sink.rfind("csv:", 0) == 0) {
        csv_path = a.sink.substr(4);
    } else if (a.sink != "none") {
        usage();
        return false;
    }
    return true;
}

int run(const Args& a) {
    const Config conf = Config::findAndReadConfigFile(a.conf, true);
    if (a.print_config) {
        std::string o = "{";
        bool first = true;
        for (const auto& kv : conf.scalars()) {
            o += (first ? "" : ", ") + json_str(kv.first) + ": " + json_str(kv.second);
            first = false;
        }
        for (const auto& kv : conf.lists()) {
            o += (first ? "" : ", ") + json_str(kv.first) + ": [";
            for (size_t i = 0; i < kv.second.size(); ++i) o += (i ? ", " : "") + json_str(kv.second[i]);
            o += "]";
            first = false;
        }
        std::printf("%s}\n", o.c_str());
    }
    // getAdCampaignMap(conf.get("ad_to_campaign_path")) (:67)
    // -- or, with --join-redis, RedisAdCampaignCache's cold HashMap: the file may be empty or
    // absent, and the campaign index space is its campaigns joined with Redis' `campaigns` set
    AdCampaignMap map = a.join_redis ? AdCampaignMap::fromFileOrEmpty(conf.get("ad_to_campaign_path", ""))
                                     : AdCampaignMap::fromFile(conf.get("ad_to_campaign_path"));
    std::unique_ptr<RedisAdLookup> lookup;
    if (a.join_redis && !a.dry && a.replay.empty()) {
        std::string host;
        int port;
        redis_address(a, conf, &host, &port);
        lookup.reset(new RedisAdLookup(host, port));
        for (const std::string& c : lookup->campaigns()) map.addCampaign(c);
    }
    const std::string events = conf.get("events_path");
    // (a compressed replay file is named after what it holds: events.tbl.lz4)
    const std::string named = a.lz4 && events.size() > 4 && events.compare(events.size() - 4, 4, ".lz4") == 0
                                  ? events.substr(0, events.size() - 4) : events;
    const bool tbl = a.format.empty() ? (named.size() > 4 && named.compare(named.size() - 4, 4, ".tbl") == 0)
                                      : a.format == "tbl";
    if (!a.format.empty() && a.format != "json" && a.format != "tbl") { usage(); return 2; }

    GpuAdCampaignOperator::Options o;
    o.device = a.device;
    o.windowRing = a.window_ring;
    o.batchBytes = (uint64_t)a.batch_bytes;
    o.batchEvents = (uint64_t)a.batch_events;
    o.tbl = tbl;
    o.requireIp = a.require_ip;
    o.gpuSplit = !a.host_split;
    o.h2dSdma = a.h2d_sdma;
    o.mappedIo = !a.lz4 && !a.kafka && (a.io == "mapped" || (a.io == "auto" && o.gpuSplit && !o.h2dSdma));
    o.parkCapacity = lookup ? (uint64_t)a.park_capacity : 0;
    if (a.io == "mapped" && !o.gpuSplit) {
        std::fprintf(stderr, "--io mapped reads raw lines in place: not with --host-split\n");
        return 2;
    }

    FileBasedDataSource src(events, a.io_threads, a.io_mmap);
    const double t0 = now_s();
    if (a.dry && a.io == "mapped") {   // the mapped source's ranges alone: whole lines, every byte once
        uint64_t nb, bytes = 0, batches = 0, cut = 0;
        const uint8_t* p = nullptr;
        while ((nb = src.nextMapped(o.batchBytes, &p)) > 0) {
            if (p != src.mapping() + bytes) throw std::runtime_error("mapped ranges not back to back");
            const uint8_t last = p[nb - 1];
            if (last != '\n' && last != '\r') ++cut;   // only the file's last line may lack its terminator
            bytes += nb;
            ++batches;
        }
        std::printf("{\"mode\": \"dry-run\", \"io\": \"mapped\", \"bytes\": %llu, \"batches\": %llu, "
                    "\"unterminated\": %llu}\n",
                    (unsigned long long)bytes, (unsigned long long)batches, (unsigned long long)cut);
        return 0;
    }
    if (a.dry) {   // host half only: map + source, no device
        std::vector<uint8_t> buf(o.batchBytes);
        std::vector<uint32_t> off(o.batchEvents);
        uint64_t n, nb, bytes = 0, batches = 0;
        while ((n = src.fill(buf.data(), buf.size(), off.data(), off.size(), &nb)) > 0) {
            bytes += nb;
            ++batches;
        }
        std::printf("{\"mode\": \"dry-run\", \"ads\": %zu, \"campaigns\": %zu, \"events\": %llu, \"bytes\": %llu, "
                    "\"batches\": %llu, \"format\": \"%s\"}\n",
                    map.ads.size(), map.campaigns.size(), (unsigned long long)src.linesRead(),
                    (unsigned long long)bytes, (unsigned long long)batches, tbl ? "tbl" : "json");
        return 0;
    }

    std::unique_ptr<RedisWindowWriter> redis;
    CsvWindowSink csv;
    std::string csv_path;
    if (!open_sink(a, conf, redis, csv_path)) return 2;

    if (!a.replay.empty()) {   // the sink alone: rows from a CSV, one flush
        std::vector<WindowDelta> d;
        const std::vector<std::string> lines = readLines(readFile(a.replay));
        for (size_t i = 1; i < lines.size(); ++i) {
            const std::vector<std::string> f = javaSplit(lines[i], ',');
            if (f.size() != 3) throw std::runtime_error("bad row line " + std::to_string(i + 1));
            d.push_back({f[0], std::stoll(f[1]), std::stoull(f[2])});
        }
        if (redis) redis->writeWindows(d);
        if (!csv_path.empty()) {
            csv.add(d);
            csv.write(csv_path);
        }
        std::printf("{\"mode\": \"replay-rows\", \"rows\": %zu, \"round_trips\": %llu}\n", d.size(),
                    (unsigned long long)(redis ? redis->roundTrips() : 0));
        return 0;
    }

    GpuAdCampaignOperator op(map, o);
    op.open();
    if (o.mappedIo && a.io == "auto" && !src.mapping()) o.mappedIo = false;   // nothing mapped (empty file)
    if (o.mappedIo) {
        try {
            op.registerSource(src);
        } catch (const std::exception& e) {
            if (a.io == "mapped") throw;
            std::fprintf(stderr, "note: the events file's mapping cannot be read in place (%s): slot copies\n",
                         e.what());
            o.mappedIo = false;
        }
    }
    // --lz4 --io mapped: the container's mapping (the source's) registered; a refused
    // registration falls back to the slot path, as the uncompressed runner's does
    bool lz4_mapped = a.lz4 && a.io == "mapped";
    if (lz4_mapped) {
        try {
            op.registerSource(src);
        } catch (const std::exception& e) {
            std::fprintf(stderr, "note: the container's mapping cannot be read in place (%s): slot copies\n", e.what());
            lz4_mapped = false;
        }
    }
    const double t_open = now_s();   // the stream itself: from the first read to close
    uint64_t rows = 0, flushes = 0;
    auto flush = [&]() {
        const std::vector<WindowDelta> d = op.flushWindows();
        rows += d.size();
        ++flushes;
        if (redis) redis->writeWindows(d);
        if (!csv_path.empty()) csv.add(d);
    };
    double last_flush = now_s();
    // --lz4: the container's blocks in runs that fit a slot, compressed and decoded; the
    // line-aligned flag makes every run a batch of whole lines
    // --lz4 --io mapped: the container is mapped (the source's mapping), not read, and every
    // run is read where it lies (ysb_submit_lz4_mapped)
    // A standard LZ4 frame (lz4 -B4 -BI, ysb_gen --lz4-frame), told from the container by its
    // magic: indexed on the host (one size word per block), fed in runs of blocks that fit a
    // slot (the span and (blocks + 1) x 64 KiB), YSB_LZ4F_MORE on all batches but the last --
    // frame blocks end mid-line, the device carries the unfinished line to the next batch.
    std::string lz4_file;
    Lz4Container lz4;
    std::vector<ysb_lz4_frame_block> frame;
    const uint8_t* frame_bytes = nullptr;
    bool is_frame = false;
    if (a.lz4) {
        if (!lz4_mapped) lz4_file = readFile(events);
        const uint8_t* fb = lz4_mapped ? src.mapping() : reinterpret_cast<const uint8_t*>(lz4_file.data());
        const uint64_t fn = lz4_mapped ? src.fileBytes() : lz4_file.size();
        is_frame = fn >= 4 && fb[1] == (fb[0] == 0x04 ? 0x22 : 0x2A) && fb[2] == 0x4D && fb[3] == 0x18 &&
                   (fb[0] == 0x04 || (fb[0] & 0xF0) == 0x50);
        if (is_frame) {
            uint64_t n = 0;
            ysb_lz4_frame_summary sum{};
            int rc = ysb_lz4_frame_index(fb, fn, nullptr, 0, &n, &sum);
            if (rc && rc != YSB_ERR_CAPACITY) throw std::runtime_error(events + ": " + ysb_last_error(nullptr));
            frame.resize(n);
            if (n && ysb_lz4_frame_index(fb, fn, frame.data(), n, &n, &sum))
                throw std::runtime_error(events + ": " + ysb_last_error(nullptr));
            frame_bytes = fb;
            lz4.rawBytes = sum.content_bytes;   // (what the frames state; 0 if none does)
        } else if (lz4_mapped) {
            lz4 = Lz4Container::parse(src.mapping(), src.fileBytes(), events);
        } else {
            lz4 = Lz4Container::parse(lz4_file, events);
        }
    }
    if (a.lz4 && !is_frame) {
        if (!lz4.lineAligned)
            throw std::runtime_error(events + ": its blocks are not line-aligned (ysb_gen --lz4 writes them so): "
                                     "a run of blocks would cut lines");
    }
    uint64_t lz4_comp = 0;
    // --kafka: the segment's index (one 61-byte header per batch) and runs of whole batches that
    // fit a slot's bytes and lines; --io mapped: read where they lie in the registered mapping
    bool kafka_mapped = a.kafka && a.io == "mapped";
    uint64_t kafka_framed = 0, kafka_records = 0, kafka_batches = 0;
    if (kafka_mapped) {
        try {
            op.registerSource(src);
        } catch (const std::exception& e) {
            std::fprintf(stderr, "note: the segment's mapping cannot be read in place (%s): slot copies\n", e.what());
            kafka_mapped = false;
        }
    }
    uint64_t kafka_compressed = 0, kafka_inflated = 0;
    const bool kafka_snappy = a.kafka_codec == "snappy";
    const uint32_t kafka_index_flags = (a.kafka_check_crc == "host" ? YSB_KAFKA_CHECK_CRC
                                        : a.kafka_check_crc == "device" ? YSB_KAFKA_CHECK_CRC_CONTROL : 0u) |
                                       (kafka_snappy ? YSB_KAFKA_ACCEPT_SNAPPY : 0u);
    if (a.kafka && kafka_snappy) op.setKafkaCodecs(YSB_KAFKA_CODECS_DEFAULT | YSB_KAFKA_CODECS_SNAPPY);
    if (a.kafka && a.kafka_check_crc == "device") op.setKafkaCrc(YSB_KAFKA_CRC_DEVICE);
    if (a.kafka && !a.kafka_codec.empty()) {
        // the three arrays of ysb_kafka_index_lz4; runs of whole batches by the slot's bytes and lines
        // and by the bound on what they inflate to (ysb_kafka_inflate_bounds: 64 KiB per block, a
        // snappy block what its preamble says)
        std::string file;
        if (!kafka_mapped) file = readFile(events);
        const uint8_t* fb = kafka_mapped ? src.mapping() : reinterpret_cast<const uint8_t*>(file.data());
        const uint64_t fn = kafka_mapped ? src.fileBytes() : file.size();
        ysb_kafka_lz4_summary sum{};
        int rc = ysb_kafka_index_lz4(fb, fn, kafka_index_flags, nullptr, nullptr, 0, nullptr, 0, &sum);
        if (rc && rc != YSB_ERR_CAPACITY) throw std::runtime_error(events + ": " + ysb_last_error(nullptr));
        std::vector<ysb_kafka_batch> idx(sum.n_batches);
        std::vector<ysb_kafka_frame> frames(sum.n_batches);
        std::vector<ysb_lz4_frame_block> blocks(sum.blocks);
        if (sum.n_batches && ysb_kafka_index_lz4(fb, fn, kafka_index_flags, idx.data(), frames.data(), idx.size(), blocks.data(), blocks.size(), &sum))
            throw std::runtime_error(events + ": " + ysb_last_error(nullptr));
        if (sum.consumed != fn)
            std::fprintf(stderr, "note: %llu bytes behind the segment's last whole batch are left alone\n",
                         (unsigned long long)(fn - sum.consumed));
        const uint64_t max_lines = std::max<uint64_t>(o.batchEvents, o.batchBytes / 32);
        std::vector<uint64_t> inflates_to(idx.size());
        if (!idx.empty() && ysb_kafka_inflate_bounds(fb, fn, idx.data(), frames.data(), idx.size(), blocks.data(), blocks.size(), inflates_to.data()))
            throw std::runtime_error(events + ": " + ysb_last_error(nullptr));
        std::vector<ysb_kafka_batch> rel;
        std::vector<ysb_kafka_frame> relf;
        std::vector<ysb_lz4_frame_block> relb;
        for (long long rep = 0; rep < a.repeat; ++rep) {
            for (uint64_t b = 0; b < idx.size();) {
                const uint64_t start = idx[b].records_off - 61;
                uint64_t e = b, recs = 0, nblk = 0, infl = 0;
                while (e < idx.size() && idx[e].records_off + idx[e].records_bytes - start <= o.batchBytes &&
                       recs + idx[e].n_records <= max_lines && infl + inflates_to[e] <= o.batchBytes) {
                    recs += idx[e].n_records;
                    nblk += frames[e].n_blocks;
                    infl += inflates_to[e];
                    ++e;
                }
                if (e == b) throw std::runtime_error(events + ": batch " + std::to_string(b) + " exceeds the slot (--batch-mb; "
                                                     "a compressed batch needs 65536 bytes per block)");
                const uint64_t span = idx[e - 1].records_off + idx[e - 1].records_bytes - start;
                rel.assign(idx.begin() + (ptrdiff_t)b, idx.begin() + (ptrdiff_t)e);
                relf.assign(frames.begin() + (ptrdiff_t)b, frames.begin() + (ptrdiff_t)e);
                const uint64_t fb0 = frames[b].first_block;
                relb.assign(blocks.begin() + (ptrdiff_t)fb0, blocks.begin() + (ptrdiff_t)(fb0 + nblk));
                for (ysb_kafka_batch& k : rel) {
                    k.records_off -= start;
                    k.first_record -= idx[b].first_record;
                }
                for (ysb_kafka_frame& f : relf) {
                    f.first_block -= fb0;
                    kafka_compressed += f.codec ? 1 : 0;
                }
                for (ysb_lz4_frame_block& k : relb) k.offset -= start;
                op.submitKafkaLz4(fb + start, span, rel.data(), relf.data(), rel.size(), relb.data(), relb.size(), kafka_mapped);
                kafka_framed += span;
                kafka_records += recs;
                kafka_batches += e - b;
                b = e;
                if (lookup) op.resolveParked(*lookup);
                if (a.flush_ms > 0 && (now_s() - last_flush) * 1000.0 >= (double)a.flush_ms) {
                    flush();
                    last_flush = now_s();
                }
            }
        }
        kafka_inflated = op.kafkaLz4Info().inflated_total;
    } else if (a.kafka) {
        std::string file;
        if (!kafka_mapped) file = readFile(events);
        const uint8_t* fb = kafka_mapped ? src.mapping() : reinterpret_cast<const uint8_t*>(file.data());
        const uint64_t fn = kafka_mapped ? src.fileBytes() : file.size();
        ysb_kafka_summary sum{};
        int rc = ysb_kafka_index(fb, fn, kafka_index_flags, nullptr, 0, &sum);
        if (rc && rc != YSB_ERR_CAPACITY) throw std::runtime_error(events + ": " + ysb_last_error(nullptr));
        std::vector<ysb_kafka_batch> idx(sum.n_batches);
        if (sum.n_batches && ysb_kafka_index(fb, fn, kafka_index_flags, idx.data(), idx.size(), &sum))
            throw std::runtime_error(events + ": " + ysb_last_error(nullptr));
        if (sum.consumed != fn)
            std::fprintf(stderr, "note: %llu bytes behind the segment's last whole batch are left alone\n",
                         (unsigned long long)(fn - sum.consumed));
        const uint64_t max_lines = std::max<uint64_t>(o.batchEvents, o.batchBytes / 32);
        std::vector<ysb_kafka_batch> rel;
        for (long long rep = 0; rep < a.repeat; ++rep) {
            for (uint64_t b = 0; b < idx.size();) {
                const uint64_t start = idx[b].records_off - 61;
                uint64_t e = b, recs = 0;
                while (e < idx.size() && idx[e].records_off + idx[e].records_bytes - start <= o.batchBytes &&
                       recs + idx[e].n_records <= max_lines) recs += idx[e++].n_records;
                if (e == b) throw std::runtime_error(events + ": batch " + std::to_string(b) + " exceeds the slot (--batch-mb)");
                const uint64_t span = idx[e - 1].records_off + idx[e - 1].records_bytes - start;
                rel.assign(idx.begin() + (ptrdiff_t)b, idx.begin() + (ptrdiff_t)e);
                for (ysb_kafka_batch& k : rel) {
                    k.records_off -= start;
                    k.first_record -= idx[b].first_record;
                }
                op.submitKafka(fb + start, span, rel.data(), rel.size(), kafka_mapped);
                kafka_framed += span;
                kafka_records += recs;
                kafka_batches += e - b;
                b = e;
                if (lookup) op.resolveParked(*lookup);
                if (a.flush_ms > 0 && (now_s() - last_flush) * 1000.0 >= (double)a.flush_ms) {
                    flush();
                    last_flush = now_s();
                }
            }
        }
    }
    for (long long rep = 0; is_frame && rep < a.repeat; ++rep) {
        for (uint64_t b = 0; b < frame.size();) {
            uint64_t e = b;
            auto end_of = [&](uint64_t i) { return frame[i].offset + (frame[i].comp_bytes & ~YSB_LZ4_STORED); };
            while (e < frame.size() && end_of(e) - frame[b].offset <= o.batchBytes && (e - b + 2) * 65536ull <= o.batchBytes) ++e;
            if (e == b) throw std::runtime_error(events + ": block " + std::to_string(b) + " exceeds the slot (--batch-mb)");
            op.submitLz4Blocks(frame_bytes, frame.data() + b, (uint32_t)(e - b), e < frame.size(), lz4_mapped);
            lz4_comp += end_of(e - 1) - frame[b].offset;
            b = e;
            if (lookup) op.resolveParked(*lookup);
            if (a.flush_ms > 0 && (now_s() - last_flush) * 1000.0 >= (double)a.flush_ms) {
                flush();
                last_flush = now_s();
            }
        }
    }
    for (long long rep = 0; a.lz4 && !is_frame && rep < a.repeat; ++rep) {
        for (uint64_t b = 0; b < lz4.nBlocks;) {
            uint64_t e = b, comp = 0, raw = 0;
            while (e < lz4.nBlocks && comp + (lz4.dir[e].comp_bytes & ~YSB_LZ4_STORED) <= o.batchBytes &&
                   raw + lz4.dir[e].raw_bytes <= o.batchBytes && e - b < 0xFFFFFFFFull) {
                comp += lz4.dir[e].comp_bytes & ~YSB_LZ4_STORED;
                raw += lz4.dir[e].raw_bytes;
                ++e;
            }
            if (e == b) throw std::runtime_error(events + ": block " + std::to_string(b) + " exceeds the slot (--batch-mb)");
            if (lz4_mapped) op.submitLz4Mapped(lz4.blocks + lz4.blockStart(b), comp, lz4.dir + b, (uint32_t)(e - b));
            else op.submitLz4(lz4.blocks + lz4.blockStart(b), comp, lz4.dir + b, (uint32_t)(e - b));
            lz4_comp += comp;
            b = e;
            if (lookup) op.resolveParked(*lookup);
            if (a.flush_ms > 0 && (now_s() - last_flush) * 1000.0 >= (double)a.flush_ms) {
                flush();
                last_flush = now_s();
            }
        }
    }
    for (long long rep = 0; !a.lz4 && !a.kafka && rep < a.repeat; ++rep) {
        if (rep) src.rewind();
        while (o.mappedIo ? op.submitMapped(src) > 0 : (o.gpuSplit ? op.fillFromRaw(src) : op.fillFrom(src)) > 0) {
            if (!o.mappedIo) op.submit();
            if (lookup) op.resolveParked(*lookup);   // the batch's misses: GET, put, count
            if (a.flush_ms > 0 && (now_s() - last_flush) * 1000.0 >= (double)a.flush_ms) {
                flush();
                last_flush = now_s();
            }
        }
        op.submit();   // a last partial slot
        if (lookup) op.resolveParked(*lookup);
    }
    op.close();
    const double el_stream = now_s() - t_open;
    flush();
    const double el = now_s() - t0;
    if (!csv_path.empty()) csv.write(csv_path);
    const ysb_stats s = op.stats();
    double copy_ms = 0;
    uint64_t copies = 0, copy_bytes = 0;
    op.copyTime(&copy_ms, &copies, &copy_bytes);
    std::printf("{\"mode\": \"gpu\", \"events\": %llu, \"views\": %llu, \"joined\": %llu, \"join_misses\": %llu, "
                "\"parse_errors\": %llu, \"time_errors\": %llu, \"out_of_ring\": %llu, \"overflow_dropped\": %llu, "
                "\"batches\": %llu, \"rows_written\": %llu, \"flushes\": %llu, \"seconds\": %.3f, "
                "\"events_per_s\": %.1f, \"stream_seconds\": %.3f, \"stream_events_per_s\": %.1f, "
                "\"bytes\": %llu, \"stream_GBs\": %.2f, \"line_split\": \"%s\", \"repeat\": %lld, "
                "\"format\": \"%s\", \"sink\": %s, \"h2d\": \"%s\", \"copy_GBs\": %.2f, \"copy_busy_frac\": %.4f, "
                "\"fill_s\": %.3f, \"slot_wait_s\": %.3f, \"join_redis\": %s, \"parked_keys\": %llu, "
                "\"parked_found\": %llu, \"parked_joined\": %llu, \"parked_missed\": %llu, \"join_round_trips\": %llu, "
                "\"lz4\": %s, \"lz4_comp_bytes\": %llu, \"lz4_raw_bytes\": %llu, \"lz4_io\": \"%s\", "
                "\"kafka\": %s, \"kafka_framed_bytes\": %llu, \"kafka_records\": %llu, \"kafka_batches\": %llu, "
                "\"kafka_io\": \"%s\", \"kafka_codec\": \"%s\", \"kafka_compressed_batches\": %llu, "
                "\"kafka_inflated_bytes\": %llu}\n",
                (unsigned long long)s.events, (unsigned long long)s.views, (unsigned long long)s.joined,
                (unsigned long long)s.join_misses, (unsigned long long)s.parse_errors,
                (unsigned long long)s.time_errors, (unsigned long long)s.out_of_ring,
                (unsigned long long)s.overflow_dropped, (unsigned long long)s.batches, (unsigned long long)rows,
                (unsigned long long)flushes, el, el > 0 ? (double)s.events / el : 0.0, el_stream,
                el_stream > 0 ? (double)s.events / el_stream : 0.0, (unsigned long long)src.bytesRead(),
                el_stream > 0 ? (double)src.bytesRead() / el_stream / 1e9 : 0.0, o.gpuSplit ? "gpu" : "host",
                a.repeat, tbl ? "tbl" : "json",
                json_str(a.sink).c_str(), a.h2d_sdma ? "sdma" : o.mappedIo ? "mapped" : "kernel",
                copy_ms > 0 ? (double)copy_bytes / (copy_ms * 1e-3) / 1e9 : 0.0,
                el_stream > 0 ? copy_ms * 1e-3 / el_stream : 0.0, op.fillSeconds(), op.waitSeconds(),
                lookup ? "true" : "false", (unsigned long long)op.parkedTotals().keys,
                (unsigned long long)op.parkedTotals().found, (unsigned long long)op.parkedTotals().joined,
                (unsigned long long)op.parkedTotals().missed, (unsigned long long)(lookup ? lookup->roundTrips() : 0),
                a.lz4 ? "true" : "false", (unsigned long long)lz4_comp,
                (unsigned long long)(a.lz4 ? lz4.rawBytes * (uint64_t)a.repeat : 0),
                !a.lz4 ? "" : lz4_mapped ? "mapped" : "slot", a.kafka ? "true" : "false",
                (unsigned long long)kafka_framed, (unsigned long long)kafka_records, (unsigned long long)kafka_batches,
                !a.kafka ? "" : kafka_mapped ? "mapped" : "slot", a.kafka_codec.c_str(),
                (unsigned long long)kafka_compressed, (unsigned long long)kafka_inflated);
    return s.overflow_dropped ? 3 : 0;
}

// --columns: the reference's commented chain (AdvertisingTopologyNative.java:106-109) instead
// of the counting chain -- countWindowAll(window.size) over the events file's rows, each
// window decoded on the GPU into WindowedArrowFormatBolter's columnar image (:278-356) and
// written to <shared_file>_<k> (:317) as the reference's mapping would hold it: image_bytes
// long, longs big-endian (MappedByteBuffer.putLong), stamp 10 (:333), padding zero.  A trailing
// partial window is never written (the count window does not fire).  A row the reference
// would have thrown on fails the job.
int run_columns(const Args& a) {
    const Config conf = Config::findAndReadConfigFile(a.conf, true);
    const std::string events = conf.get("events_path");
    const std::string shared = conf.get("shared_file");
    const long long window = conf.getLong("window.size");
    if (window <= 0 || window > 0x7FFFFFFFll) throw std::runtime_error("window.size must be in [1, 2^31 - 1]");
    if (!a.format.empty() && a.format != "json" && a.format != "tbl") { usage(); return 2; }
    const bool tbl = a.format.empty() ? (events.size() > 4 && events.compare(events.size() - 4, 4, ".tbl") == 0)
                                      : a.format == "tbl";
    ysb_columns_layout lay;
    if (ysb_columns_layout_of((uint64_t)window, &lay)) throw std::runtime_error("ysb_columns_layout_of failed");

    ysb_config cfg;
    ysb_config_default(&cfg);
    cfg.n_campaigns = 1;   // the decode uses no join table and no ring
    cfg.window_ring = 16;
    cfg.max_ads = 1;
    cfg.max_batch_events = 64;
    cfg.max_batch_bytes = 1 << 16;
    cfg.overflow_capacity = 16;
    cfg.flags = YSB_F_LAYOUT_FIXED | (tbl ? YSB_F_FORMAT_TBL : 0u) | (a.require_ip ? YSB_F_REQUIRE_IP : 0u);
    ysb_ctx* ctx = nullptr;
    if (ysb_open(&ctx, a.device, &cfg)) throw std::runtime_error(std::string("ysb_open: ") + ysb_last_error(nullptr));
    auto chk = [&](int rc, const char* what) {
        if (rc) {
            const std::string msg = std::string(what) + ": " + ysb_last_error(ctx);
            ysb_close(ctx);
            throw std::runtime_error(msg);
        }
    };
    const uint64_t cap = (uint64_t)a.batch_bytes;
    void *d_bytes = nullptr, *d_off = nullptr, *d_out = nullptr;
    chk(ysb_device_alloc(ctx, cap, &d_bytes), "ysb_device_alloc");
    chk(ysb_device_alloc(ctx, 4 * (uint64_t)window, &d_off), "ysb_device_alloc");
    chk(ysb_device_alloc(ctx, lay.start[8], &d_out), "ysb_device_alloc");
    std::vector<uint8_t> image(lay.start[8], 0);   // a fresh mapping is zero
    chk(ysb_memcpy_h2d(ctx, d_out, image.data(), image.size()), "ysb_memcpy_h2d");

    FileBasedDataSource src(events, a.io_threads, a.io_mmap);
    std::vector<uint8_t> wbytes(cap), buf(cap);
    std::vector<uint32_t> woff((size_t)window), off((size_t)window);
    uint64_t have = 0, used = 0, files = 0, rows = 0;
    double kernel_ms = 0;
    const double t0 = now_s();
    for (;;) {
        uint64_t nb = 0;
        const uint64_t n = src.fill(buf.data(), cap - used, off.data(), (uint64_t)window - have, &nb);
        if (n == 0) break;
        std::memcpy(wbytes.data() + used, buf.data(), nb);
        for (uint64_t i = 0; i < n; ++i) woff[have + i] = (uint32_t)(used + off[i]);
        have += n;
        used += nb;
        if (have < (uint64_t)window) {
            if (used >= cap) {
                ysb_close(ctx);
                throw std::runtime_error("a window of " + std::to_string(window) + " rows exceeds --batch-bytes");
            }
            continue;
        }
        chk(ysb_memcpy_h2d(ctx, d_bytes, wbytes.data(), used), "ysb_memcpy_h2d");
        chk(ysb_memcpy_h2d(ctx, d_off, woff.data(), 4 * have), "ysb_memcpy_h2d");
        ysb_decode_info info;
        chk(ysb_decode_columns_device(ctx, (const uint8_t*)d_bytes, used, (const uint32_t*)d_off, have, (uint8_t*)d_out,
                                      (uint64_t)window, 10, YSB_COL_JAVA_ORDER, &info),
            "ysb_decode_columns_device");
        kernel_ms += info.kernel_ms;
        chk(ysb_memcpy_d2h(ctx, image.data(), d_out, image.size()), "ysb_memcpy_d2h");
        if (info.valid != info.rows) {   // the reference's flatMap throws: the job fails
            uint64_t bad = 0;
            while (bad < have && ((image[lay.start[7] + bad / 8] >> (bad % 8)) & 1)) ++bad;
            ysb_close(ctx);
            throw std::runtime_error("--columns: " + shared + "_" + std::to_string(files) + " (file index " +
                                     std::to_string(files) + "), row " + std::to_string(bad) + " (line " +
                                     std::to_string(rows + bad + 1) + " of " + events +
                                     "): a row the reference throws on (" +
                                     std::to_string(info.rows - info.valid) + " in this window)");
        }
        const std::string path = shared + "_" + std::to_string(files);
        std::FILE* f = std::fopen(path.c_str(), "wb");
        if (!f || std::fwrite(image.data(), 1, lay.image_bytes, f) != lay.image_bytes || std::fclose(f) != 0) {
            ysb_close(ctx);
            throw std::runtime_error("cannot write " + path);
        }
        ++files;
        rows += have;
        have = used = 0;
    }
    for (void* p : {d_bytes, d_off, d_out}) ysb_device_free(ctx, p);
    ysb_close(ctx);
    const double el = now_s() - t0;
    std::printf("{\"mode\": \"columns\", \"files\": %llu, \"rows\": %llu, \"dropped_tail_rows\": %llu, "
                "\"window_size\": %lld, \"image_bytes\": %llu, \"kernel_ms\": %.3f, \"seconds\": %.3f, "
                "\"format\": \"%s\", \"shared_file\": %s}\n",
                (unsigned long long)files, (unsigned long long)rows, (unsigned long long)have, window,
                (unsigned long long)lay.image_bytes, kernel_ms, el, tbl ? "tbl" : "json", json_str(shared).c_str());
    return 0;
}

// --from-columns: the consumer of --columns -- the accelerator behind WindowedArrowFormatBolter
// (AdvertisingTopologyNative.java:278-356).  Loads ad_to_campaign_path, reads <shared_file>_0,
// _1, ... up to the first missing index, each the image_bytes of window.size rows with big-endian
// longs and no validity bitmap (the reference's mapping), counts them through the filter -> join
// -> window-count chain (:115-119) from their columns (ysb_submit_columns, slots 0 and 1
// alternating) and flushes to the sink as the batch mode does.  A file of another size fails
// the job, naming it.
int run_from_columns(const Args& a) {
    const Config conf = Config::findAndReadConfigFile(a.conf, true);
    const AdCampaignMap map = AdCampaignMap::fromFile(conf.get("ad_to_campaign_path"));
    const std::string shared = conf.get("shared_file");
    const long long window = conf.getLong("window.size");
    if (window <= 0 || window > 0x7FFFFFFFll) throw std::runtime_error("window.size must be in [1, 2^31 - 1]");
    ysb_columns_layout lay;
    if (ysb_columns_layout_of((uint64_t)window, &lay)) throw std::runtime_error("ysb_columns_layout_of failed");
    std::unique_ptr<RedisWindowWriter> redis;
    CsvWindowSink csv;
    std::string csv_path;
    if (!open_sink(a, conf, redis, csv_path)) return 2;

    GpuAdCampaignOperator::Options o;
    o.device = a.device;
    o.windowRing = a.window_ring;
    o.batchBytes = lay.image_bytes;
    o.batchEvents = 64;   // (the slots' line offsets are not used)
    o.h2dSdma = a.h2d_sdma;
    const double t0 = now_s();
    GpuAdCampaignOperator op(map, o);
    op.open();
    uint64_t files = 0, rows = 0, flushes = 0;
    auto flush = [&]() {
        const std::vector<WindowDelta> d = op.flushWindows();
        rows += d.size();
        ++flushes;
        if (redis) redis->writeWindows(d);
        if (!csv_path.empty()) csv.add(d);
    };
    double last_flush = now_s();
    for (;; ++files) {
        const std::string path = shared + "_" + std::to_string(files);
        std::FILE* f = std::fopen(path.c_str(), "rb");
        if (!f) break;   // the first missing index ends the job
        std::fclose(f);
        op.submitColumnsFile(path, (uint64_t)window);
        if (a.flush_ms > 0 && (now_s() - last_flush) * 1000.0 >= (double)a.flush_ms) {
            flush();
            last_flush = now_s();
        }
    }
    op.close();
    flush();
    const double el = now_s() - t0;
    if (!csv_path.empty()) csv.write(csv_path);
    const ysb_stats s = op.stats();
    std::printf("{\"mode\": \"from_columns\", \"files\": %llu, \"rows\": %llu, \"views\": %llu, \"joined\": %llu, "
                "\"join_misses\": %llu, \"out_of_ring\": %llu, \"overflow_dropped\": %llu, \"batches\": %llu, "
                "\"rows_written\": %llu, \"flushes\": %llu, \"window_size\": %lld, \"image_bytes\": %llu, "
                "\"bytes_read_per_row\": 48, \"seconds\": %.3f, \"rows_per_s\": %.1f, \"sink\": %s, "
                "\"shared_file\": %s}\n",
                (unsigned long long)files, (unsigned long long)s.events, (unsigned long long)s.views,
                (unsigned long long)s.joined, (unsigned long long)s.join_misses, (unsigned long long)s.out_of_ring,
                (unsigned long long)s.overflow_dropped, (unsigned long long)s.batches, (unsigned long long)rows,
                (unsigned long long)flushes, window, (unsigned long long)lay.image_bytes, el,
                el > 0 ? (double)s.events / el : 0.0, json_str(a.sink).c_str(), json_str(shared).c_str());
    return s.overflow_dropped ? 3 : 0;
}

double pct(std::vector<double> v, double q) {
    if (v.empty()) return 0;
    std::sort(v.begin(), v.end());
    const double pos = q / 100.0 * (double)(v.size() - 1);
    const size_t lo = (size_t)pos, hi = std::min(v.size() - 1, lo + 1);
    return v[lo] + (v[hi] - v[lo]) * (pos - (double)lo);
}

std::string dist(const std::vector<double>& v, double scale) {
    char b[256];
    std::snprintf(b, sizeof b, "{\"n\": %zu, \"p50\": %.1f, \"p99\": %.1f, \"max\": %.1f}", v.size(),
                  pct(v, 50) * scale, pct(v, 99) * scale, v.empty() ? 0.0 : *std::max_element(v.begin(), v.end()) * scale);
    return b;
}

// Streaming mode (BASELINE configs[4]): ysb_stream.hpp.
int run_stream(const Args& a) {
    StreamingJob job(a.so);
    const double t0 = now_s();
    job.prepare();
    const double prep_s = now_s() - t0;
    std::unique_ptr<RedisWindowWriter> redis;
    if (a.sink.rfind("redis", 0) == 0) {
        std::string host = "localhost";
        int port = 6379;
        const std::string rest = a.sink.size() > 6 ? a.sink.substr(6) : "";
        if (!rest.empty()) {
            const size_t c = rest.rfind(':');
            host = c == std::string::npos ? rest : rest.substr(0, c);
            if (c != std::string::npos) port = std::atoi(rest.c_str() + c + 1);
        }
        redis.reset(new RedisWindowWriter(host, port));
    } else if (a.sink != "none" && a.sink.rfind("csv:", 0) != 0) {
        usage();
        return 2;
    }
    CsvWindowSink totals;
    const std::string csv_path = a.sink.rfind("csv:", 0) == 0 ? a.sink.substr(4) : a.stream_csv;
    const StreamReport r = job.run([&](const FlushRows& f, int64_t now) {
        if (redis) redis->writeWindows(f.rows, now);
        totals.add(f.rows);
    });
    if (!csv_path.empty()) totals.write(csv_path);
    const double f = 1.0 / a.so.speedup;   // replay ms -> wall ms
    std::string cyc = "[", part = "[";
    for (size_t i = 0; i < r.cycles.size(); ++i) {
        cyc += (i ? ", " : "") + std::to_string(r.cycles[i]);
        part += (i ? ", " : "") + std::to_string(r.partialLines[i]);
    }
    cyc += "]";
    part += "]";
    std::string per = "[";
    for (size_t i = 0; i < r.shards.size(); ++i) {
        const ShardReport& s = r.shards[i];
        char b[512];
        std::snprintf(b, sizeof b, "%s{\"device\": %d, \"numa_node\": %d, \"feeder_pinned\": %s, \"events\": %llu, "
                      "\"batches\": %llu, \"submit_ms\": %.1f, \"feeder_cpu_s\": %.3f, \"max_behind_ms\": %.2f, "
                      "\"ring_advances\": %llu, \"replay_GB\": %.2f, \"prepare_s\": %.2f, \"register_s\": %.2f}",
                      i ? ", " : "", s.device, s.numaNode, s.pinned ? "true" : "false", (unsigned long long)s.events,
                      (unsigned long long)s.batches, s.submitMs, s.feederCpuS, s.maxBehindMs,
                      (unsigned long long)s.ringAdvances, s.replayGB, s.prepareS, s.registerS);
        per += b;
    }
    per += "]";
    std::printf("{\"mode\": \"stream\", \"replay\": \"%s\", \"shards\": %d, \"events\": %llu, \"batches\": %llu, "
                "\"wall_s\": %.3f, \"submit_events_per_s\": %.1f, \"per_shard\": %s, "
                "\"events_per_s\": %.1f, \"target_events_per_s\": %.1f, \"copy_GBs\": %.2f, \"copy_busy_frac\": %.4f, "
                "\"slot_waits\": %llu, \"slot_wait_ms\": %.2f, \"slot_wait_max_ms\": %.3f, \"max_behind_ms\": %.2f, "
                "\"flushes\": %llu, \"rows_written\": %llu, \"ring_advances\": %llu, "
                "\"window_close_ms\": %s, \"window_close_wall_ms\": %s, \"get_stats_ms\": %s, "
                "\"get_stats_wall_ms_after_window_end\": %s, \"open_at_end\": %llu, \"final_watermark_ms\": %lld, "
                "\"speedup\": %.3f, \"event_rate\": %.1f, \"cycle_ms\": %lld, \"flush_ms\": %lld, \"batch_ms\": %lld, "
                "\"ooo_ms\": %lld, \"skew\": %d, \"seed\": %llu, \"campaigns\": %u, \"ads_per_campaign\": %u, "
                "\"t0_ms\": %lld, \"lines_per_cycle\": %llu, \"cycles\": %s, \"partial_lines\": %s, "
                "\"overflow_dropped\": %llu, \"parse_errors\": %llu, \"join_misses\": %llu, \"prepare_s\": %.2f, "
                "\"sink\": %s, \"stream_lz4\": %s, \"lz4_block\": %u, \"lz4_comp_bytes_per_cycle\": %llu, "
                "\"lz4_raw_bytes_per_cycle\": %llu, \"lz4_blocks_per_cycle\": %llu, \"pcie_bytes_per_event\": %.2f}\n",
                a.so.replay == StreamOptions::MAPPED ? "mapped" : a.so.replay == StreamOptions::MAPPED_RAW ? "mapped-raw" : "copy",
                a.so.shards, (unsigned long long)r.events, (unsigned long long)r.batches,
                r.wallSeconds, r.submitEventsPerSecond, per.c_str(), r.eventsPerSecond,
                r.targetEventsPerSecond, r.copyGBs, r.copyBusyFrac, (unsigned long long)r.slotWaits, r.slotWaitMs,
                r.slotWaitMaxMs, r.maxBehindMs, (unsigned long long)r.flushes, (unsigned long long)r.rowsWritten,
                (unsigned long long)r.ringAdvances, dist(r.closeReplayMs, 1.0).c_str(), dist(r.closeReplayMs, f).c_str(),
                dist(r.cwReplayMs, 1.0).c_str(),
                dist([&] { std::vector<double> v; for (double x : r.cwReplayMs) v.push_back(x - 10000.0); return v; }(), f).c_str(),
                (unsigned long long)r.openAtEnd, (long long)r.finalWatermarkMs, a.so.speedup, a.so.eventRate, (long long)a.so.cycleMs,
                (long long)a.so.flushMs, (long long)a.so.batchMs, (long long)a.so.oooMs, a.so.skew,
                (unsigned long long)a.so.seed, a.so.campaigns, a.so.adsPerCampaign, (long long)a.so.t0Ms,
                (unsigned long long)r.linesPerCycle, cyc.c_str(), part.c_str(), (unsigned long long)r.overflowDropped,
                (unsigned long long)r.parseErrors, (unsigned long long)r.joinMisses, prep_s, json_str(a.sink).c_str(),
                a.so.streamLz4 ? "true" : "false", a.so.streamLz4 ? a.so.lz4Block : 0u,
                (unsigned long long)r.lz4CompBytesPerCycle, (unsigned long long)r.lz4RawBytesPerCycle,
                (unsigned long long)r.lz4BlocksPerCycle, r.pcieBytesPerEvent);
    return r.overflowDropped ? 3 : 0;
}

}  // namespace

int main(int argc, char** argv) {
    const Args a = parse(argc, argv);
    if (ysb_abi_version() != YSB_ABI_VERSION || ysb_exchange_info_size() != sizeof(ysb_exchange_info)) {
        std::fprintf(stderr, "ysb_topology: libysb_hip.so has ABI %d, this runner was built for ABI %d: rebuild\n",
                     ysb_abi_version(), YSB_ABI_VERSION);
        return 2;
    }
    try {
        if (a.self_check) {
            std::printf("%s\n", replaySelfCheck(a.so, {0, 1, 2, 7, 1000}).c_str());
            return 0;
        }
        if (a.feed_check) {
            std::printf("%s\n", feedCheck(a.so, a.feed_seconds).c_str());
            return 0;
        }
        if (a.merge_check) {
            const std::string r = mergeCheck(a.so.shards, a.merge_flushes, a.so.seed);
            std::printf("%s\n", r.c_str());
            return r.find("\"ok\": true") != std::string::npos ? 0 : 1;
        }
        if (a.stream) return run_stream(a);
        if (a.columns) return run_columns(a);
        if (a.from_columns) return run_from_columns(a);
        return run(a);
    } catch (const std::exception& e) {   // the job fails, as the reference's uncaught exceptions do
        std::fprintf(stderr, "ysb_topology: %s\n", e.what());
        return 1;
    }
}
