// ysb_topology.hpp -- the C++ host side above the C ABI (include/ysb_hip.h): the
// reference's Flink job (flink-benchmarks/src/main/java/flink/benchmark/
// AdvertisingTopologyNative.java:58-142) restated with the reference's class names,
// argument meanings and error behaviour, driving the GPU operator instead of the
// per-record Java chain.
//
//   Config::findAndReadConfigFile   benchmark.common.Utils.findAndReadConfigFile (Utils.java:29-63)
//   AdCampaignMap                   AdvertisingTopologyNative.getAdCampaignMap (:47-56) and the
//                                   generator's JSON map lines (data/src/setup/core.clj:58)
//   FileBasedDataSource             FileBasedDataSource.run (:144-165): readLine over events_path
//   GpuAdCampaignOperator           DeserializeBolt -> EventFilterBolt -> project -> RedisJoinBolt
//                                   -> keyBy -> CampaignProcessor (:111-119 / :122-138), one operator
//   RedisWindowWriter               CampaignProcessorCommon.writeWindow (CampaignProcessorCommon.java:69-89)
//                                   / AdvertisingSpark.writeWindow (AdvertisingSpark.scala:184-208)
//
// Errors surface as exceptions (std::runtime_error) where the reference's Java code
// throws; records the reference would have dropped are dropped and counted.
#pragma once

#include <cstdint>
#include <cstdio>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "ysb_hip.h"

namespace ysb {
namespace topology {

// ---- configuration ---------------------------------------------------------------------
// The YAML subset conf/benchmarkConf.yaml uses: `key: scalar`, `key:` followed by
// `- item` lines, `#` comments, single/double-quoted scalars.
class Config {
public:
    static Config findAndReadConfigFile(const std::string& path, bool mustExist);
    static Config parse(const std::string& text);
    bool has(const std::string& key) const;
    const std::string& get(const std::string& key) const;          // throws when missing
    std::string get(const std::string& key, const std::string& dflt) const;
    long long getLong(const std::string& key) const;               // throws when missing / not a number
    const std::vector<std::string>& getList(const std::string& key) const;
    const std::map<std::string, std::string>& scalars() const { return scalars_; }
    const std::map<std::string, std::vector<std::string>>& lists() const { return lists_; }

private:
    std::map<std::string, std::string> scalars_;
    std::map<std::string, std::vector<std::string>> lists_;
};

// java.io.BufferedReader.readLine over a whole text: "\n", "\r\n" and "\r" end a line.
std::vector<std::string> readLines(const std::string& text);
// java.lang.String.split(one literal char, limit 0): trailing empty items dropped.
std::vector<std::string> javaSplit(const std::string& s, char sep);
std::string readFile(const std::string& path);

// ---- ad -> campaign map -------------------------------------------------------------------
struct AdCampaignMap {
    std::vector<std::string> campaigns;                 // campaign index -> UUID
    std::vector<std::string> ads;                       // distinct ads, first-appearance order
    std::vector<uint32_t> adCampaign;                   // ads[i] -> campaign index
    // CSV `ad,campaign` (split(","); kv[0] -> kv[1]; a later duplicate wins; a line with
    // fewer than two items throws, as ArrayIndexOutOfBounds does) or JSON map lines
    // `{ "AD": "CAMPAIGN"}` (merged left to right, core.clj:104-106): chosen by content.
    static AdCampaignMap fromFile(const std::string& path);
    static AdCampaignMap fromCsv(const std::string& text);
    static AdCampaignMap fromJsonLines(const std::string& text);
    // --join-redis: the file may be absent or empty -- the cold cache of
    // RedisAdCampaignCache.prepare() (RedisAdCampaignCache.java:19-21)
    static AdCampaignMap fromFileOrEmpty(const std::string& path);
    // A campaign without an ad yet (the `campaigns` set, core.clj:213): its index, added if new.
    uint32_t addCampaign(const std::string& campaign);
    // The index of a campaign UUID, -1 if it is not in the index space.
    int64_t campaignOf(const std::string& campaign) const;

private:
    std::unordered_map<std::string, uint32_t> campaignIndex_, adIndex_;
    void put(const std::string& ad, const std::string& campaign);
};

// ---- event source ----------------------------------------------------------------------------
// Threads that stay up for the source's lifetime: run(n, f) calls f(t) for t in [0, n) on
// n threads (the caller's is t = 0) and returns when all are done.
class WorkerPool;

// The events file as complete lines ('\n'-terminated; the last line may lack it), read
// in large blocks straight into a caller buffer, by parallel preads of a persistent pool;
// a partial line at the end of a block is carried into the next one.  Empty lines are
// records, as readLine returns them.
class FileBasedDataSource {
public:
    // threads: readers/splitters per block (0 = min(16, hardware threads)).  mmap: read by
    // parallel copies out of a read-only mapping of the file (no syscall per piece) instead of
    // parallel preads.
    explicit FileBasedDataSource(const std::string& path, unsigned threads = 0, bool mmap = true);
    ~FileBasedDataSource();
    FileBasedDataSource(const FileBasedDataSource&) = delete;
    FileBasedDataSource& operator=(const FileBasedDataSource&) = delete;
    // Fills buf (cap bytes) with whole lines and off (maxLines) with their offsets;
    // returns the number of lines (0 = end of file).  Throws if one line exceeds cap.
    uint64_t fill(uint8_t* buf, uint64_t cap, uint32_t* off, uint64_t maxLines, uint64_t* nbytes);
    // The same without the line split: buf receives whole lines, the return value is their
    // bytes (0 = end of file); the GPU finds the line starts (ysb_submit_raw).
    uint64_t fillRaw(uint8_t* buf, uint64_t cap);
    // Zero-copy (mmap mode only): the next whole lines, at most cap bytes, where they lie in the
    // mapping -- *p points into it, the return value is their bytes (0 = end of file).  The
    // GPU reads them in place (ysb_submit_raw_mapped) once the mapping is registered.
    uint64_t nextMapped(uint64_t cap, const uint8_t** p);
    // The mapping (NULL without mmap) and its registrable length (whole pages).
    const uint8_t* mapping() const { return map_; }
    uint64_t mappingBytes() const;
    uint64_t fileBytes() const { return size_; }
    // Back to the file's start (a replay source read again).
    void rewind();
    uint64_t linesRead() const { return lines_; }
    uint64_t bytesRead() const { return bytes_; }

private:
    int fd_ = -1;
    const uint8_t* map_ = nullptr;      // the file mapped read-only (mmap mode)
    uint64_t size_ = 0;
    uint64_t pos_ = 0;                  // file offset of the next read
    unsigned threads_ = 1;
    std::unique_ptr<WorkerPool> pool_;
    std::vector<uint8_t> carry_;
    bool eof_ = false;
    uint64_t lines_ = 0, bytes_ = 0;
    uint64_t readBlock(uint8_t* buf, uint64_t cap);   // carry + file bytes into buf: bytes held
    uint64_t completeEnd(const uint8_t* buf, uint64_t have, bool anyCr) const;
};

// ---- the join's Redis (--join-redis) ----------------------------------------------------------
// What RedisAdCampaignCache asks Redis (RedisAdCampaignCache.java:23-35): jedis.get(ad_id), the
// `<ad_id> -> campaign_id` strings the generator SET (core.clj:160), and the `campaigns` set it
// SADDed (core.clj:213), which is the campaign index space.
class RespClient;   // RESP2 over a TCP socket
class RedisAdLookup {
public:
    RedisAdLookup(const std::string& host, int port);
    ~RedisAdLookup();
    std::vector<std::string> campaigns();                                  // SMEMBERS campaigns
    // one pipelined GET per key: {found, campaign_id}
    std::vector<std::pair<bool, std::string>> get(const std::vector<std::string>& adIds);
    uint64_t roundTrips() const { return trips_; }

private:
    std::unique_ptr<RespClient> r_;
    uint64_t trips_ = 0;
};

// One (campaign, window) delta: what writeWindow HINCRBYs into seen_count.
struct WindowDelta {
    std::string campaign;
    int64_t windowMs;
    uint64_t count;
};

// ---- the operator -------------------------------------------------------------------------------
class GpuAdCampaignOperator {
public:
    struct Options {
        int device = 0;
        int64_t timeDivisorMs = 10000;      // CampaignProcessorCommon.java:28
        uint32_t windowRing = 1024;
        uint64_t batchBytes = 256ull << 20;
        uint64_t batchEvents = 1ull << 20;
        bool tbl = false;                   // MockWindowedFlatMap's .tbl rows (:197-226)
        bool requireIp = false;             // Storm/Spark's 7-field deserializer
        bool gpuSplit = true;               // fillFromRaw + ysb_submit_raw: line starts found on the GPU
        bool h2dSdma = false;               // YSB_F_H2D_SDMA: the slot's H2D by the DMA engine (default: a copy kernel)
        bool mappedIo = false;              // the source's mapping registered, batches read in place (--io mapped)
        uint64_t parkCapacity = 0;          // --join-redis: views of unknown ads parked (ysb_parked_enable), 0 = off
    };
    GpuAdCampaignOperator(const AdCampaignMap& map, const Options& o);
    ~GpuAdCampaignOperator();
    GpuAdCampaignOperator(const GpuAdCampaignOperator&) = delete;
    GpuAdCampaignOperator& operator=(const GpuAdCampaignOperator&) = delete;

    void open();                                           // RichFlatMapFunction.open
    void flatMap(const char* line, uint64_t len);          // one record
    uint64_t fillFrom(FileBasedDataSource& src);           // a slot's worth of records, zero-copy
    uint64_t fillFromRaw(FileBasedDataSource& src);        // the same as raw lines (bytes returned)
    void registerSource(FileBasedDataSource& src);         // pin + map the source's mapping (mappedIo)
    uint64_t submitMapped(FileBasedDataSource& src);       // the next whole lines, read in place: bytes
    void submit();                                         // hand the open slot to the GPU
    // a batch of whole lines as LZ4 blocks (ysb_submit_raw_lz4): copied into the open slot's
    // pinned buffer compressed, decoded on the GPU
    void submitLz4(const uint8_t* blocks, uint64_t compBytes, const ysb_lz4_block* dir, uint32_t nBlocks);
    // the same read where the blocks lie, in the registered mapping of the container
    // (ysb_submit_lz4_mapped after registerSource): no copy into a slot
    void submitLz4Mapped(const uint8_t* blocks, uint64_t compBytes, const ysb_lz4_block* dir, uint32_t nBlocks);
    // A run of a standard LZ4 frame's blocks (ysb_lz4_frame_index's entries over `file`) as one
    // batch: through the slot, or (mapped) read where they lie in the registered mapping.  more:
    // the batch's unfinished last line is carried in front of the next one (YSB_LZ4F_MORE).
    void submitLz4Blocks(const uint8_t* file, const ysb_lz4_frame_block* blocks, uint32_t nBlocks, bool more, bool mapped);
    // A run of whole Kafka record batches (ysb_kafka_index's entries, records_off relative to
    // `bytes`, first_record running from 0) as one batch: through the slot, or (mapped) read where
    // it lies in the registered mapping.
    void submitKafka(const uint8_t* bytes, uint64_t nbytes, const ysb_kafka_batch* batches, uint64_t nBatches, bool mapped);
    // ysb_kafka_set_crc: the Kafka submits verify every batch's CRC-32C on the GPU (a batch whose
    // CRC differs drops its slot batch: the sticky error is thrown by the call that meets it)
    void setKafkaCrc(int mode);
    // ysb_kafka_set_codecs: which codecs the compressed Kafka submits take (YSB_KAFKA_CODECS_*)
    void setKafkaCodecs(uint32_t mask);
    // The same for batches that may be LZ4-compressed (ysb_kafka_index_lz4's three arrays, offsets
    // relative to `bytes`): inflated on the GPU in front of the unframing (ysb_submit_kafka_lz4).
    void submitKafkaLz4(const uint8_t* bytes, uint64_t nbytes, const ysb_kafka_batch* batches, const ysb_kafka_frame* frames,
                        uint64_t nBatches, const ysb_lz4_frame_block* blocks, uint64_t nBlocks, bool mapped);
    // ysb_kafka_lz4_info: the last compressed call and the inflated bytes of all (waits for everything)
    ysb_kafka_lz4_desc kafkaLz4Info();
    // One file image of WindowedArrowFormatBolter (<shared_file>_<k>, :303-317) of `rows` rows
    // counted from its columns (ysb_submit_columns, longs big-endian): only the ranges the count
    // reads are read from the file, straight into the open slot.  Throws, naming the file, if
    // its size is not the layout's image_bytes.
    void submitColumnsFile(const std::string& path, uint64_t rows);
    // --join-redis, after a batch: everything submitted is waited for, the distinct ads of the
    // parked views are asked of Redis (pipelined GETs), the ads found are put into the live map
    // (ysb_ad_map_upsert) and the parked views resolved.  A GET that names a campaign outside the
    // index space (the map file's campaigns and the `campaigns` set at start-up) throws, naming it.
    struct Parked {
        uint64_t keys = 0, found = 0, joined = 0, missed = 0;
    };
    Parked resolveParked(RedisAdLookup& redis);
    const Parked& parkedTotals() const { return parked_; }
    std::vector<WindowDelta> flushWindows();               // CampaignProcessorCommon.flushWindows (:91-98)
    void close();                                          // RichFlatMapFunction.close
    ysb_stats stats();
    uint64_t submittedEvents() const { return submitted_; }
    // host seconds spent filling slots (fillFrom / fillFromRaw) and waiting for a slot's H2D
    double fillSeconds() const { return fillS_; }
    double waitSeconds() const { return waitS_; }
    // the slots' H2D: total ms, copies and bytes (YSB_F_TIMING, ysb_copy_time)
    void copyTime(double* ms, uint64_t* copies, uint64_t* bytes);

private:
    const AdCampaignMap& map_;
    Options o_;
    ysb_ctx* ctx_ = nullptr;
    double fillS_ = 0, waitS_ = 0;
    uint8_t* bytes_[2] = {nullptr, nullptr};
    uint32_t* off_[2] = {nullptr, nullptr};
    int cur_ = 0;
    uint64_t fillBytes_ = 0, fillEvents_ = 0, submitted_ = 0, rawBytes_ = 0;
    Parked parked_;
    void check(int rc, const char* what);
};

// A compressed replay file (include/ysb_hip.h ysb_lz4_file_header: header, directory, blocks)
// as a view into its bytes.  parse throws, naming the file, for anything that is not one.
struct Lz4Container {
    bool lineAligned = false;
    uint64_t nBlocks = 0, rawBytes = 0;
    const ysb_lz4_block* dir = nullptr;
    const uint8_t* blocks = nullptr;
    std::vector<uint64_t> start;                            // block i's first byte in blocks; [nBlocks]: their size
    uint64_t blockStart(uint64_t i) const { return start[i]; }
    static Lz4Container parse(const uint8_t* file, uint64_t size, const std::string& name);
    static Lz4Container parse(const std::string& file, const std::string& name) {
        return parse(reinterpret_cast<const uint8_t*>(file.data()), file.size(), name);
    }
};

// ---- output -------------------------------------------------------------------------------------------

class RedisWindowWriter {
public:
    RedisWindowWriter(const std::string& host, int port);
    ~RedisWindowWriter();
    // writeWindow for every delta of one flush, in two pipelined round trips; time_updated is
    // nowMs (the wall clock when negative; a streaming replay passes its replay clock).
    void writeWindows(const std::vector<WindowDelta>& rows, int64_t nowMs = -1);
    uint64_t roundTrips() const { return trips_; }

private:
    std::unique_ptr<RespClient> r_;
    std::map<std::pair<std::string, std::string>, std::string> windowUuid_;
    std::map<std::string, std::string> listUuid_;
    uint64_t trips_ = 0;
};

// Totals per (campaign, window) written as `campaign_id,window_ms,count` lines.
class CsvWindowSink {
public:
    void add(const std::vector<WindowDelta>& rows);
    void write(const std::string& path) const;
    uint64_t windows() const { return totals_.size(); }

private:
    std::map<std::pair<std::string, int64_t>, uint64_t> totals_;
};

std::string randomUuid();

}  // namespace topology
}  // namespace ysb
