// ysb_gen -- file-dump mode of the data/ generator (data/src/setup/core.clj:239-248
// -s, and write-to-kafka :61-98 which the reference leaves unwired at :246).
//
//   ysb_gen -d DIR [-n EVENTS] [--seed S] [--campaigns C] [--ads-per-campaign A]
//           [--rate EVENTS_PER_SEC] [--t0 MS] [--with-skew] [--users K]
//           [--shards K] [--tbl] [--lz4 [--lz4-block N] | --lz4-frame] [--kafka [--kafka-batch BYTES] [--kafka-codec lz4|snappy [--kafka-snappy-framing xerial|raw]]]
//
// Writes campaign-ids.txt, ad-ids.txt, ad-to-campaign-ids.txt (JSON map lines),
// ad-to-campaign.csv (the fork's CSV map) and kafka-json.txt into DIR; with --shards K
// kafka-json.<r>.txt per ad_id-hash shard instead; with --tbl also events.tbl, the
// fork's pipe-delimited rows (conf/benchmarkConf.yaml:6); with --lz4 also kafka-json.txt.lz4
// (and events.tbl.lz4): the same bytes as a compressed replay file of line-aligned LZ4 blocks
// of N bytes (default 8192; include/ysb_hip.h ysb_lz4_file_header) for ysb_topology --lz4.
// With --lz4-frame the .lz4 files are standard LZ4 frames instead (independent 64 KiB blocks,
// content size set: any LZ4 tool reads them, and so does ysb_topology --lz4).
// With --kafka also kafka-json.log: the same events as a partition's log segment -- Kafka record
// batches (message format v2) of at most BYTES bytes (default 16384, a producer's batch.size),
// each event one record's value without its line terminator, as write-to-kafka (core.clj:61-98)
// sends it -- for ysb_topology --kafka.  With --kafka-codec lz4 each batch's records are one
// standard LZ4 frame (attributes codec 3, what compression.type=lz4 puts on the wire), for
// ysb_topology --kafka --kafka-codec lz4.  With --kafka-codec snappy they are snappy (attributes
// codec 2): the Java client's xerial stream of 32 KiB chunks, or with --kafka-snappy-framing raw
// one raw block per batch as librdkafka writes it (--kafka-batch at most 65536) -- for
// ysb_topology --kafka --kafka-codec snappy.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ysb_hip.h"

int main(int argc, char** argv) {
    ysb_gen_params p;
    ysb_gen_default(&p);
    p.events_per_sec = 100;   // catch-up mode: one event per 10 ms (core.clj:95)
    unsigned long long n = 10000000ULL;   // kafka-event-count (core.clj:17)
    const char* dir = nullptr;
    unsigned shards = 0;
    bool tbl = false, lz4 = false, lz4_frame = false;
    unsigned lz4_block = 8192;
    bool kafka = false;
    unsigned kafka_batch = 16384;
    unsigned kafka_codec = 0;     // --kafka-codec lz4: each batch's records as one LZ4 frame (attributes codec 3);
                                  //   snappy: as a xerial stream or one raw block (codec 2)
    unsigned kafka_snappy_framing = YSB_KAFKA_SNAPPY_XERIAL;
    for (int i = 1; i < argc; ++i) {
        auto val = [&]() -> const char* {
            if (i + 1 >= argc) { std::fprintf(stderr, "missing value for %s\n", argv[i]); std::exit(2); }
            return argv[++i];
        };
        if (!std::strcmp(argv[i], "-d")) dir = val();
        else if (!std::strcmp(argv[i], "-n")) n = std::strtoull(val(), nullptr, 10);
        else if (!std::strcmp(argv[i], "--seed")) p.seed = std::strtoull(val(), nullptr, 10);
        else if (!std::strcmp(argv[i], "--campaigns")) p.n_campaigns = (unsigned)std::strtoul(val(), nullptr, 10);
        else if (!std::strcmp(argv[i], "--ads-per-campaign")) p.ads_per_campaign = (unsigned)std::strtoul(val(), nullptr, 10);
        else if (!std::strcmp(argv[i], "--rate")) p.events_per_sec = std::strtoull(val(), nullptr, 10);
        else if (!std::strcmp(argv[i], "--t0")) p.t0_ms = std::strtoll(val(), nullptr, 10);
        else if (!std::strcmp(argv[i], "--with-skew")) p.with_skew = 1;
        else if (!std::strcmp(argv[i], "--users")) p.n_users = (unsigned)std::strtoul(val(), nullptr, 10);
        else if (!std::strcmp(argv[i], "--shards")) shards = (unsigned)std::strtoul(val(), nullptr, 10);
        else if (!std::strcmp(argv[i], "--tbl")) tbl = true;
        else if (!std::strcmp(argv[i], "--lz4")) lz4 = true;
        else if (!std::strcmp(argv[i], "--lz4-frame")) lz4 = lz4_frame = true;
        else if (!std::strcmp(argv[i], "--lz4-block")) lz4_block = (unsigned)std::strtoul(val(), nullptr, 10);
        else if (!std::strcmp(argv[i], "--kafka")) kafka = true;
        else if (!std::strcmp(argv[i], "--kafka-batch")) kafka_batch = (unsigned)std::strtoul(val(), nullptr, 10);
        else if (!std::strcmp(argv[i], "--kafka-codec")) {
            const char* v = val();
            if (std::strcmp(v, "lz4") && std::strcmp(v, "snappy")) {
                std::fprintf(stderr, "ysb_gen: --kafka-codec %s: lz4 and snappy are the codecs that are written\n", v);
                return 2;
            }
            kafka_codec = std::strcmp(v, "lz4") ? YSB_KAFKA_CODEC_SNAPPY : YSB_KAFKA_CODEC_LZ4;
        }
        else if (!std::strcmp(argv[i], "--kafka-snappy-framing")) {
            const char* v = val();
            if (std::strcmp(v, "xerial") && std::strcmp(v, "raw")) { std::fprintf(stderr, "ysb_gen: --kafka-snappy-framing %s: xerial or raw\n", v); return 2; }
            kafka_snappy_framing = std::strcmp(v, "raw") ? YSB_KAFKA_SNAPPY_XERIAL : YSB_KAFKA_SNAPPY_RAW;
        }
        else { std::fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
    }
    if (!dir) { std::fprintf(stderr, "usage: ysb_gen -d DIR [-n EVENTS] [options]\n"); return 2; }
    int rc = shards > 1 ? ysb_gen_dump_shards(&p, n, dir, shards) : ysb_gen_dump(&p, n, dir);
    if (rc) { std::fprintf(stderr, "ysb_gen: %s\n", ysb_last_error(nullptr)); return 1; }
    if (tbl) {   // events.tbl: the same events as .tbl rows (generator format YSB_GEN_TBL)
        ysb_gen_params q = p;
        q.format = YSB_GEN_TBL;
        rc = ysb_gen_dump(&q, n, dir);
        if (rc) { std::fprintf(stderr, "ysb_gen: %s\n", ysb_last_error(nullptr)); return 1; }
    }
    if (lz4) {
        if (shards > 1) { std::fprintf(stderr, "ysb_gen: --lz4 compresses kafka-json.txt / events.tbl: not with --shards\n"); return 2; }
        for (const char* name : {"kafka-json.txt", "events.tbl"}) {
            if (!tbl && name[0] == 'e') continue;
            const std::string path = std::string(dir) + "/" + name;
            std::vector<uint8_t> data;
            FILE* f = std::fopen(path.c_str(), "rb");
            if (!f) { std::fprintf(stderr, "ysb_gen: cannot read %s\n", path.c_str()); return 1; }
            uint8_t buf[1 << 16];
            for (size_t k; (k = std::fread(buf, 1, sizeof buf, f)) > 0;) data.insert(data.end(), buf, buf + k);
            std::fclose(f);
            // --lz4-frame: one standard LZ4 frame of independent 64 KiB blocks (what lz4 -B4 -BI writes)
            rc = lz4_frame ? ysb_lz4_frame_write((path + ".lz4").c_str(), data.data(), data.size(), 65536, 16)
                           : ysb_lz4_write_file((path + ".lz4").c_str(), data.data(), data.size(), lz4_block, 1, 1, 16);
            if (rc) { std::fprintf(stderr, "ysb_gen: %s\n", ysb_last_error(nullptr)); return 1; }
        }
    }
    if (kafka) {
        if (shards > 1) { std::fprintf(stderr, "ysb_gen: --kafka frames kafka-json.txt: not with --shards\n"); return 2; }
        const std::string path = std::string(dir) + "/kafka-json.txt";
        FILE* f = std::fopen(path.c_str(), "rb");
        if (!f) { std::fprintf(stderr, "ysb_gen: cannot read %s\n", path.c_str()); return 1; }
        // the values back to back: every line without its terminator
        std::vector<uint8_t> data;
        std::vector<uint32_t> off;
        uint8_t buf[1 << 16];
        bool at_start = true;
        for (size_t k; (k = std::fread(buf, 1, sizeof buf, f)) > 0;)
            for (size_t j = 0; j < k; ++j) {
                if (buf[j] == '\n') { at_start = true; continue; }
                if (at_start) {
                    if (data.size() > 0xFFFFFFFFull) { std::fprintf(stderr, "ysb_gen: --kafka takes up to 4 GiB of values\n"); return 1; }
                    off.push_back((uint32_t)data.size());
                    at_start = false;
                }
                data.push_back(buf[j]);
            }
        std::fclose(f);
        ysb_kafka_pack_opts o{};
        o.batch_bytes = kafka_batch;
        o.codec = kafka_codec;
        o.snappy_framing = kafka_snappy_framing;
        o.base_timestamp = p.t0_ms;
        rc = ysb_kafka_write_file((std::string(dir) + "/kafka-json.log").c_str(), data.data(), data.size(), off.data(), off.size(), &o);
        if (rc) { std::fprintf(stderr, "ysb_gen: %s\n", ysb_last_error(nullptr)); return 1; }
    }
    return 0;
}
