/*
 * ysb_hip.h -- C ABI of the MI355X-native YSB advertising hot path.
 *
 * One library (libysb_hip.so) replaces the Flink operator chain
 *   DeserializeBolt -> EventFilterBolt -> project(ad_id, event_time)
 *   -> RedisJoinBolt -> keyBy(campaign) -> CampaignProcessor/CampaignProcessorCommon
 * of the reference (flink-benchmarks/src/main/java/flink/benchmark/
 * AdvertisingTopologyNative.java:111-138) with hand-written gfx950 kernels.
 * Every entry point below names the reference interface it stands in for.
 *
 * Conventions
 *   - plain C, no exceptions cross the ABI; every call returns an int status,
 *     0 = YSB_OK, negative = error; ysb_last_error(ctx) explains the last one.
 *   - one ysb_ctx per Flink subtask and per GPU; calls on one ctx are not
 *     concurrent (the reference's operators are single-threaded per subtask).
 *   - counts are exact 64-bit integers (the reference's Window.seenCount is a
 *     java.lang.Long, streaming-benchmark-common/.../Window.java:9).
 */
#ifndef YSB_HIP_H
#define YSB_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: ysb_stats.foreign_shard, YSB_F_STRICT, ysb_load_ad_map(_packed)_shard, the
 *    range-limited exchange (ysb_group_exchange_info / ysb_exchange_plan),
 *    ysb_group_checksum, layout selection on by default (YSB_F_LAYOUT_FIXED turns it off),
 *    ysb_sync's sticky YSB_ERR_CAPACITY, the collective ysb_ring_advance after
 *    ysb_group_init, ysb_gen_params.variant
 * 3: raw batches with the line split on the GPU (ysb_submit_raw, ysb_split_lines_device),
 *    ysb_slot_capacity, ysb_copy_time; device batches' layout sampled in stream order
 * 4: ysb_device_count; a busy stream's device batches take the sampled layout only when two
 *    samples agree (else the per-tile dispatch, never a host wait for the launch queued
 *    last); a raw batch that cannot launch is a sticky error (ysb_stream returns NULL);
 *    raw batches hold at most max(max_batch_events, max_batch_bytes / 32) lines
 * 5: ysb_device_sync, ysb_device_numa_node; batches read in place from caller-registered host
 *    memory (ysb_host_register; raw lines: ysb_submit_raw_mapped; offsets in device memory:
 *    ysb_submit_mapped) with the replay's event-time rebasing on the device
 *    (ysb_rebase_table); ysb_exchange_info_size (the struct grew in ABI 4: a caller
 *    checks the size it was built with); YSB_F_TIMING's event records are folded into running
 *    totals, so a caller that never reads them keeps a bounded number
 * 6: ysb_record_info / ysb_record_desc_size (the last record-mode launch's plan, sub-buffer
 *    fill and partition runs, read-only) */
#define YSB_ABI_VERSION 6

/* status codes */
#define YSB_OK            0
#define YSB_ERR_ARG      (-1)  /* bad argument / size                      */
#define YSB_ERR_HIP      (-2)  /* HIP runtime failure                      */
#define YSB_ERR_STATE    (-3)  /* call not valid in the current state      */
#define YSB_ERR_CAPACITY (-4)  /* batch, table or output buffer too small  */
#define YSB_ERR_FORMAT   (-5)  /* malformed ad map / config, or a batch
                                  with a bad LZ4 block (dropped whole)     */
#define YSB_ERR_RCCL     (-6)  /* RCCL failure                             */
#define YSB_ERR_NOMEM    (-7)  /* host or device allocation failed         */
#define YSB_ERR_DATA     (-8)  /* strict mode: the batch held records the
                                  reference would have thrown on           */
#define YSB_PENDING        1   /* ysb_flush_end(wait = 0): not complete yet (not an error) */

/* ysb_config.flags */
#define YSB_F_TIMING       0x1u /* record HIP events around every scan launch */
#define YSB_F_REQUIRE_IP   0x2u /* also require a string "ip_address" (the Storm/
                                   Spark deserializers read 7 fields:
                                   storm-benchmarks/.../AdvertisingTopology.java:56-62,
                                   AdvertisingSpark.scala:124-134; Flink reads 6:
                                   AdvertisingTopologyNative.java:267-272)      */
#define YSB_F_NO_LDS_COUNT 0x4u /* disable the per-workgroup LDS window counters
                                   (every joined view becomes a global atomic)   */
#define YSB_F_FORMAT_TBL  0x10u /* batches are the fork's pipe-delimited .tbl lines
                                   user_id|page_id|ad_id|ad_type|event_type|event_time
                                   (MockWindowedFlatMap, AdvertisingTopologyNative.java:
                                   197-226) instead of JSON                       */
#define YSB_F_RECORD_COUNT 0x20u /* count joined views in record mode wherever possible (the
                                   default: only for rings >= 1M cells and launches >= 1M
                                   events without LDS window counters; ysb_path_time).
                                   Record mode needs the HBM-resident join table (the
                                   bucket layout ysb_load_ad_map builds for tables beyond
                                   64 MB): with a cache-resident table the flag has no
                                   effect.  ysb_path_time's record_launches tells which
                                   launches used it.                                    */
#define YSB_F_NO_RECORD_COUNT 0x40u /* never: one global atomic per joined view             */
#define YSB_F_COMPACT_FIRST 0x80u /* layout hint: JSON lines are expected as compact JSON
                                   ({"user_id":"...","page_id":...} -- no space after ':'
                                   or ','); the scan tries that layout first and the
                                   generator's (core.clj:90-96) as a later tier.  Counts
                                   are identical either way; only the speed differs.
                                   Every join-table layout (since ABI 3 also the HBM-
                                   resident table's serial-probe / record-mode kernels). */
#define YSB_F_FLAT_FIRST 0x100u /* layout hint: JSON lines are flat objects in any key
                                   order or spacing (another producer's serializer); the
                                   scan parses every line with its flat-object tier first
                                   (generator-layout lines too, a little slower than their
                                   own path) -- unless a batch's first line names one key
                                   order of DeserializeBolt's keys with one spacing: then
                                   the learned-order instantiation, which sends lines off
                                   that order to the same flat tier (without
                                   YSB_F_LAYOUT_FIXED).  Counts are identical; takes
                                   precedence over YSB_F_COMPACT_FIRST.  Every join-table
                                   layout (since ABI 3). */
#define YSB_F_LAYOUT_AUTO 0x200u /* (the default since ABI 2; the bit is accepted and
                                   ignored) layout read from the data: every submit picks
                                   the scan instantiation from 64 stratified lines of the
                                   launch (since ABI 3; ABI 2: the first line) -- host
                                   batches from the pinned slot, device batches from
                                   <= 288-byte samples taken on the device in stream order
                                   (ysb_submit_device) -- the generator's layout, compact
                                   JSON, a learned key order (the sampled order and
                                   spacing, checked in place on every line), when 46 of
                                   the 64 agree; else (several producers) the per-tile
                                   dispatch (layout 4) when the sample's adjacent lines
                                   are mostly alike (producers writing in runs), the
                                   flat-object tier (2) when they are not.  Counts
                                   are identical whichever runs.  The explicit hints above
                                   take precedence.  Every join-table layout: since ABI 3
                                   the HBM-resident table's serial-probe and record-mode
                                   kernels (configs[2]) have the layout instantiations
                                   too. */
#define YSB_F_LAYOUT_FIXED 0x800u /* no layout sampling: the generator's layout first (or
                                   the explicit hint); device batches are then never read
                                   by the host before their launch */
#define YSB_F_H2D_SDMA 0x1000u   /* the slots' host-to-device copies by the DMA engine
                                   (hipMemcpyAsync) instead of a copy kernel reading the
                                   pinned slot (the default since ABI 4): on this pool DMA
                                   copies run at half rate in episodes after the GPU idled
                                   ("H2D") */
#define YSB_F_STRICT 0x400u      /* ysb_sync (and the calls built on it) return YSB_ERR_DATA
                                   once a record the reference would have thrown on was seen
                                   (parse_errors / time_errors: JSONObject / getString /
                                   Long.parseLong exceptions fail the Flink task,
                                   AdvertisingTopologyNative.java:263-272,
                                   CampaignProcessorCommon.java:58) or a view whose ad_id
                                   belongs to another rank's shard (foreign_shard: input
                                   routed by another hash than the join table's).  Sticky
                                   until ysb_reset; the counts of the other records stay
                                   exact and readable through ysb_stats_get. */
#define YSB_F_SPARSE_FAST_JOIN 0x8u /* test hook: leave every other 36-byte key out of
                                   the fast-path cuckoo table, as a failed cuckoo
                                   placement would; its misses then take the
                                   general path (results unchanged)              */

typedef struct ysb_ctx ysb_ctx;

typedef struct ysb_config {
    int64_t  time_divisor_ms;    /* 10000: CampaignProcessorCommon.java:28.  Any value
                                    >= 1: bucket = Long.parseLong(event_time) / divisor,
                                    Java long division (truncating toward zero, so bucket 0
                                    is the one window 2 * divisor - 1 ms wide), for negative
                                    times too.  Every bucket must lie in
                                    (INT64_MIN + W, INT64_MAX - W): the ring's bounds
                                    (ring base + W, first bucket - W / 8) are computed in
                                    int64_t.  Only a divisor of 1 with |event_time| >
                                    2^63 - W can leave that range; with a divisor of 1 the
                                    bucket INT64_MAX also has no half-open [lo, hi) range
                                    that ysb_drain could name.                           */
    uint32_t n_campaigns;        /* campaign index space [0, n_campaigns)            */
    uint32_t window_ring;        /* W: live (campaign, bucket) slots per campaign,
                                    power of two >= 16 (the reference keeps <= 9 live
                                    buckets: LRUHashMap(10), CampaignProcessorCommon.java:37) */
    uint64_t max_ads;            /* capacity of the device ad -> campaign table      */
    uint64_t max_batch_events;   /* per ysb_submit                                   */
    uint64_t max_batch_bytes;    /* per ysb_submit, <= 4 GiB (u32 line offsets)      */
    int64_t  ring_base_bucket;   /* first bucket of the ring; INT64_MIN = take it from
                                    the first event of the first batch (the smallest bucket
                                    among the joined views of its first 256 lines, minus
                                    W / 8).  May be negative or zero: the ring
                                    [base, base + W) may straddle bucket 0 or lie below it.
                                    base + W must not overflow: base in
                                    (INT64_MIN + W, INT64_MAX - W), as every bucket        */
    uint64_t overflow_capacity;  /* (campaign, bucket) deltas outside the ring that
                                    are kept exactly in a side list                  */
    uint32_t flags;              /* YSB_F_*                                          */
    uint32_t reserved;
} ysb_config;

/* Running totals since ysb_open / ysb_reset. */
typedef struct ysb_stats {
    uint64_t events;       /* lines scanned                                          */
    uint64_t views;        /* parsed lines with event_type == "view"
                              (EventFilterBolt, AdvertisingTopologyNative.java:434)   */
    uint64_t joined;       /* views whose ad_id is in the map (RedisJoinBolt :464)   */
    uint64_t join_misses;  /* views dropped on a map miss (:465-467)                 */
    uint64_t parse_errors; /* lines org.json's JSONObject/getString would throw on
                              (:263-272)                                             */
    uint64_t time_errors;  /* joined views whose event_time Long.parseLong rejects
                              (CampaignProcessorCommon.java:58)                       */
    uint64_t out_of_ring;  /* joined views counted through the overflow side list    */
    uint64_t overflow_dropped; /* side-list entries lost for lack of capacity (must be 0) */
    uint64_t batches;      /* submits                                                */
    uint64_t deferred;     /* lines the fast path handed to the general tokenizer    */
    uint64_t foreign_shard; /* views dropped on a map miss whose ad_id belongs to another
                              rank's shard (ysb_load_ad_map_shard): mis-routed input, not a
                              miss of the reference's map; join_misses excludes them      */
} ysb_stats;

/* One (campaign, window) delta: the unit the Redis writer HINCRBYs into
 * <windowUUID>.seen_count (AdvertisingSpark.scala:184-208,
 * CampaignProcessorCommon.java:70-88 (commented in the fork)). */
typedef struct ysb_count {
    uint32_t campaign;     /* campaign index                                         */
    uint32_t reserved;
    int64_t  window_ms;    /* bucket * time_divisor_ms = Redis window timestamp
                              (CampaignProcessorCommon.java:103)                      */
    uint64_t count;
} ysb_count;

/* ---- lifecycle ---------------------------------------------------------------- */

int         ysb_abi_version(void);
void        ysb_config_default(ysb_config* cfg);
/* The HIP devices this process sees (hipGetDeviceCount; 0 when there is none or the runtime
 * fails).  A launcher maps rank -> device with it (one context per GPU, the reference's one
 * subtask per slot) without a framework's device query. */
int         ysb_device_count(void);
/* hipDeviceSynchronize on `device` through the library's own HIP runtime (ABI 5): a host
 * (bench.py, a JVM) that must wait for the whole GPU without loading a framework's HIP
 * runtime.  A process may hold only one working HIP/HSA runtime: if another one (e.g. the
 * libamdhip64 a framework bundles) opens the GPU first, this library's runtime may see no
 * device, and ysb_open / ysb_device_sync fail with a message that says so (INTEGRATION.md
 * section 1.4a: load order). */
int         ysb_device_sync(int device);
/* The NUMA node of `device`'s PCI function (sysfs numa_node of hipDeviceGetPCIBusId's address;
 * -1 when unknown), ABI 5: where a caller's registered batches and feeder threads for this GPU
 * belong (each Flink source instance NUMA-local to the GPU its chain runs on). */
int         ysb_device_numa_node(int device);

/* Replaces CampaignProcessorCommon(String)/prepare() (CampaignProcessorCommon.java:30-55)
 * and RedisJoinBolt.open() (AdvertisingTopologyNative.java:451-458). */
int         ysb_open(ysb_ctx** out, int device, const ysb_config* cfg);
int         ysb_close(ysb_ctx* ctx);
/* ctx may be NULL: then the last error of a failed ysb_open on this thread. */
const char* ysb_last_error(const ysb_ctx* ctx);

/* Replaces getAdCampaignMap + RedisJoinBolt(Map) (AdvertisingTopologyNative.java:47-56,
 * 443-448) and RedisAdCampaignCache (RedisAdCampaignCache.java:23-35): builds the
 * GPU-resident open-addressing ad_id -> campaign table.  ad_ids[i] points at
 * ad_id_lens[i] bytes (NULL lens = 36 each, the UUID length); a later duplicate
 * wins, as HashMap.put does.  Keys are matched as exact byte strings (<= 56 B). */
int         ysb_load_ad_map(ysb_ctx* ctx, const char* const* ad_ids,
                            const uint32_t* ad_id_lens, const uint32_t* campaign_idx,
                            uint64_t n);
/* Same for n keys of key_len bytes packed back to back (a JNI byte[] of UUIDs; config 3
 * loads 10M ads this way). */
int         ysb_load_ad_map_packed(ysb_ctx* ctx, const char* keys, uint32_t key_len,
                                   const uint32_t* campaign_idx, uint64_t n);
/* The join table sharded 1/nranks per GPU: of the n entries only
 * those with ysb_ad_shard(ad_id, nranks) == rank are loaded, and the context remembers its
 * shard.  A view whose ad_id misses the table is then classified on the miss path only:
 * an ad of another shard counts as foreign_shard (input routed by another hash -- with
 * YSB_F_STRICT ysb_sync fails with YSB_ERR_DATA), any other as a join miss that the
 * reference's RedisJoinBolt would drop too (AdvertisingTopologyNative.java:443-448,
 * 465-467).  nranks = 1 is ysb_load_ad_map. */
int         ysb_load_ad_map_shard(ysb_ctx* ctx, const char* const* ad_ids,
                                  const uint32_t* ad_id_lens, const uint32_t* campaign_idx,
                                  uint64_t n, uint32_t rank, uint32_t nranks);
int         ysb_load_ad_map_packed_shard(ysb_ctx* ctx, const char* keys, uint32_t key_len,
                                         const uint32_t* campaign_idx, uint64_t n,
                                         uint32_t rank, uint32_t nranks);

/* ---- the live map: HashMap.put while the stream runs ------------------------------
 * RedisAdCampaignCache.execute puts an ad into its HashMap the first time it is seen
 * (RedisAdCampaignCache.java:23-35), and getAdCampaignMap's put lets a later entry win
 * (AdvertisingTopologyNative.java:47-56).  ysb_ad_map_upsert is that put on the context's
 * device tables: new ad ids are added, known ones get the campaign given, by kernels on the
 * compute stream between two launches -- no host rebuild, no upload of the tables.  (Additive
 * within ABI 6, as the columnar calls.) */
typedef struct ysb_upsert_info {
    uint64_t entries;        /* n as given = foreign + duplicates + updated + inserted            */
    uint64_t foreign;        /* skipped: ysb_ad_shard(key, shard_n) != shard_rank (as load_*_shard) */
    uint64_t duplicates;     /* earlier entries of a key given more than once (the last one wins)  */
    uint64_t updated;        /* keys already in the map: campaign rewritten                        */
    uint64_t inserted;       /* new keys                                                           */
    uint64_t cuckoo_first, cuckoo_second;  /* new 36-byte keys placed in their first / second slot or bucket */
    uint64_t cuckoo_moved;   /* ... placed by the eviction chain                                   */
    uint64_t cuckoo_left_out;/* ... in the general table only: the table is now partial            */
    uint32_t rebuilt;        /* 1: the tables were rebuilt at new sizes (see below)                */
    uint32_t partial;        /* some 36-byte key is in the general table only, after the call      */
    double   device_ms;      /* HIP events around the call's kernels (0 when rebuilt)              */
} ysb_upsert_info;
/* HashMap.put of entry 0, 1, ..., n - 1 in this order (ids as ysb_load_ad_map takes them:
 * exact byte strings of at most 56 bytes, length 0 allowed, NULL lens = 36 each): after the
 * call the map equals a fresh ysb_load_ad_map of the old entries followed by these.
 * Stream order: batches submitted before the call join against the old map, batches
 * submitted after it against the new one (a raw batch still awaiting its launch is launched
 * first).  The call returns when the change is applied and its counters are read back: it
 * waits for the compute stream, as a load does.
 * Every entry is checked before any device work: YSB_ERR_FORMAT for a campaign index >=
 * n_campaigns or an id above 56 bytes, YSB_ERR_ARG for a NULL id of nonzero length,
 * YSB_ERR_STATE before the first load (a load of n = 0 is a valid empty map); a rejected call
 * changes nothing.  n = 0 changes nothing and fills info.  An id given more than once counts
 * with its last campaign; on a sharded context (ysb_load_ad_map_shard) the ids of other
 * shards are skipped (foreign).
 * The call works in place exactly while the sizing rules of a load still hold for the grown
 * map: distinct keys <= table_slots / 2, and 36-byte keys in the cuckoo table <= ctable_slots
 * / 4 (slot layout) or <= ctable_slots / 2 (bucket layout; ysb_ad_map_info) -- an upserted
 * table is never denser than a fresh load's could be.  Otherwise it rebuilds (rebuilt = 1):
 * the general table is read back, merged with the call's entries, and built, uploaded and
 * committed as by ysb_load_ad_map, with that call's failure guarantees for the tables (the
 * campaigns of the call's known keys may already be rewritten when a rebuild fails); the
 * layout may change between slots and buckets.  In place a new 36-byte key that finds both
 * its slots or buckets full goes through the loader's eviction chain; the key in hand when
 * the kicks run out stays in the general table only (cuckoo_left_out, partial = 1 until the
 * next load or rebuild: the scan then defers cuckoo misses to the general table, so the join
 * stays exact).  YSB_F_SPARSE_FAST_JOIN (test hook) leaves every other new 36-byte key of a
 * call out of the cuckoo table.  At most 2^31 - 1 entries per call (YSB_ERR_CAPACITY).
 * info may be NULL. */
int         ysb_ad_map_upsert(ysb_ctx* ctx, const char* const* ad_ids, const uint32_t* ad_id_lens,
                              const uint32_t* campaign_idx, uint64_t n, ysb_upsert_info* info);
/* Same for n keys of key_len bytes packed back to back. */
int         ysb_ad_map_upsert_packed(ysb_ctx* ctx, const char* keys, uint32_t key_len,
                                     const uint32_t* campaign_idx, uint64_t n, ysb_upsert_info* info);
uint64_t    ysb_upsert_info_size(void);

/* out_campaign[i] = the campaign of key i or 0xFFFFFFFF; out_where[i] = 0 absent, 1 / 2 in
 * the cuckoo table, in the key's first / second slot or bucket, 3 in the general table only
 * (a key of another length than 36, or a 36-byte key the cuckoo table left out).  Either
 * array may be NULL.  A device kernel over the live tables, on the compute stream behind
 * everything submitted; waits for it.  YSB_ERR_STATE before the first load, YSB_ERR_FORMAT
 * for an id above 56 bytes, YSB_ERR_ARG for a NULL id of nonzero length. */
int         ysb_ad_map_lookup(ysb_ctx* ctx, const char* const* ad_ids, const uint32_t* ad_id_lens,
                              uint64_t n, uint32_t* out_campaign, uint32_t* out_where);

/* The map as the context holds it: keys distinct ad ids, keys36 of them in the cuckoo table
 * (ctable_slots slots, or with buckets = 1 that many 3-entry buckets), table_slots slots of the
 * general table, partial as in ysb_upsert_info, the shard of the last load.  No device work.
 * YSB_ERR_STATE before the first load. */
typedef struct ysb_admap_desc {
    uint64_t keys, keys36, table_slots, ctable_slots;
    uint32_t buckets, partial, shard_rank, shard_n;
} ysb_admap_desc;
int         ysb_ad_map_info(ysb_ctx* ctx, ysb_admap_desc* out);
uint64_t    ysb_admap_desc_size(void);

/* ---- parked views: jedis.get for an ad the map does not hold ------------------------
 * RedisAdCampaignCache.execute asks Redis for an ad its HashMap misses, puts what it finds and
 * drops only a view whose ad Redis does not know either (RedisAdCampaignCache.java:23-35);
 * prepare() starts that HashMap empty.  With parking enabled a view whose ad is in no device
 * table is not counted as a join miss: it is parked on the device as a self-contained record
 * (its decoded ad_id, whether Long.parseLong(event_time) succeeded, the parsed value) until the
 * caller has looked the ad up.  The caller's loop after a batch (or several):
 *     ysb_parked_keys    -> the distinct ad ids parked (one lookup per ad, not per view)
 *     its own lookup        (Redis GET, a database, ...)
 *     ysb_ad_map_upsert  -> the ads found, into the live tables
 *     ysb_parked_resolve -> every parked view counted as if its ad had been known from the
 *                           start; the views of the ads still unknown become join misses
 * Then the counts, and events, views, joined, join_misses, time_errors and out_of_ring of
 * ysb_stats, are those of a run whose map was complete from the start -- the reference's, as
 * long as Redis does not change during the run.  While records are parked
 *     views == joined + join_misses + foreign_shard + parked (ysb_parked_info).
 * A view parks where the join reaches its final verdict: in the deferred-line kernel (with
 * parking enabled every scan launch sends its fast-tier misses there, the route a partial or
 * sharded table already takes) and at the columnar count's miss.  An ad_id above 56 bytes
 * cannot be a map key and stays a join miss; on a sharded context only a key of this rank's
 * shard parks, a foreign one stays foreign_shard.  (Additive within ABI 6.)
 * Limits: one GPU (ysb_group_init refuses a context with parking enabled, and the reverse), and
 * a caller that flushes windows before it resolves sees the parked counts as later deltas. */
typedef struct ysb_parked_desc {
    uint64_t capacity;            /* records the log holds (0: parking is off)                      */
    uint64_t parked;              /* records parked now                                             */
    uint64_t parked_total;        /* records parked since ysb_open / ysb_reset (dropped not among them) */
    uint64_t dropped;             /* views that found the log full: counted as join misses (sticky) */
    uint64_t resolved_joined;     /* the last ysb_parked_resolve: records whose ad was found ...    */
    uint64_t resolved_missed;     /* ... and was not (join misses)                                  */
    uint64_t resolved_time_errors;/* ... found, but Long.parseLong had rejected the event_time      */
    uint64_t distinct_keys;       /* the last ysb_parked_keys: distinct ad ids                      */
    double   distinct_ms;         /* HIP events around the last distinct / resolve kernels          */
    double   resolve_ms;
} ysb_parked_desc;
/* Allocates the log and the distinct-key table for `capacity` records (72 + ~72 bytes of HBM
 * each) and enables parking for every later launch; 0 disables it and frees them.  Waits for
 * everything submitted.  YSB_ERR_STATE before the first map load, after ysb_group_init, or while
 * records are parked (resolve first); YSB_ERR_CAPACITY for a capacity of 2^30 or more. */
int         ysb_parked_enable(ysb_ctx* ctx, uint64_t capacity);
/* Waits for everything submitted, then: *n = the distinct ad ids among the parked records, and
 * with keys != NULL key i's bytes at keys + 56 * i (zero-padded) and its length in lens[i], in
 * no particular order.  keys == NULL: only the count.  YSB_ERR_CAPACITY, *n set, if cap (in
 * keys) is short.  YSB_ERR_STATE with parking off.  Changes nothing. */
int         ysb_parked_keys(ysb_ctx* ctx, char* keys, uint32_t* lens, uint64_t cap, uint64_t* n);
/* Walks the log against the join tables as they are now, on the compute stream behind
 * everything submitted (a raw batch awaiting its launch is launched first), and waits.  A
 * record whose ad is found counts joined += 1 and then, like a view the scan joined,
 * time_errors += 1 for a bad event_time or else one view in its (campaign, window) cell (the
 * ring, or the out-of-ring map and out_of_ring); any other record counts join_misses += 1.  The
 * log is then empty.  If no batch has fixed the ring's base yet it is the smallest bucket
 * counted here minus window_ring / 8; counts do not depend on the base.  info may be NULL.
 * YSB_ERR_STATE with parking off. */
int         ysb_parked_resolve(ysb_ctx* ctx, ysb_parked_desc* info);
/* The log's state after everything submitted (waits).  Valid, all zero, with parking off. */
int         ysb_parked_info(ysb_ctx* ctx, ysb_parked_desc* info);
uint64_t    ysb_parked_info_size(void);   /* sizeof(ysb_parked_desc) */
/* A full log: the view is a join miss as without parking and dropped += 1; ysb_sync and the
 * calls built on it then return YSB_ERR_CAPACITY until ysb_reset -- the counts are no longer
 * the reference's, as after overflow_dropped (ysb_parked_keys, _resolve and _info still work).
 * ysb_reset empties the log and zeroes these counters; parking stays enabled. */

/* ---- batches --------------------------------------------------------------------
 * A batch is n_events JSON lines packed back to back in `bytes`; line i spans
 * [line_off[i], line_off[i+1]) (the last one ends at nbytes).  This replaces the
 * per-record FlatMapFunction.flatMap calls of the chain
 * (AdvertisingTopologyNative.java:111-119 / 122-138). */

/* Library-owned pinned staging buffers for double-buffered slots 0 and 1, each
 * max_batch_bytes / max_batch_events large.  Fill, then ysb_submit the slot. */
int         ysb_slot_buffers(ysb_ctx* ctx, int slot, uint8_t** bytes, uint32_t** line_off);
/* Asynchronous: H2D copy on the copy stream, kernel on the compute stream.
 * bytes/line_off may be the slot's own buffers (zero-copy staging) or any host
 * memory (copied into the slot first).  The caller must not touch the slot's
 * buffers until ysb_wait(ctx, slot). */
int         ysb_submit(ysb_ctx* ctx, int slot, const uint8_t* bytes, uint64_t nbytes,
                       const uint32_t* line_off, uint64_t n_events);
int         ysb_wait(ysb_ctx* ctx, int slot);
/* The capacity the context was opened with (ysb_config.max_batch_bytes / max_batch_events):
 * the size of each slot's pinned buffers from ysb_slot_buffers, for a caller (e.g. a JNI
 * NewDirectByteBuffer over them) that must not write past them. */
int         ysb_slot_capacity(ysb_ctx* ctx, uint64_t* max_bytes, uint64_t* max_events);
/* A raw batch: whole lines as bytes, no offsets.  The line starts are found on the GPU
 * (ysb_split.hip) where BufferedReader.readLine ends a line -- '\n', "\r\n" or a lone '\r';
 * a last line without a terminator is a line, a terminator that ends the batch starts none --
 * so the caller (FileBasedDataSource.run, AdvertisingTopologyNative.java:144-165) only reads
 * the file into the pinned slot (max_batch_bytes bytes, at most max(max_batch_events,
 * max_batch_bytes / 32) lines: the device keeps 4 B per line start, not per byte).
 * Asynchronous and double-buffered like ysb_submit: H2D on the copy stream, the split right
 * behind it on the same stream (with YSB_F_H2D_SDMA: on a stream of its own); the batch's scan
 * is launched once its line count is back, at the next call on the context (the next submit,
 * ysb_sync, ...), so a caller that fills the other slot in between keeps the copies going;
 * ysb_wait(ctx, slot) before the slot's pinned buffer is rewritten.  A batch that cannot
 * launch (more lines than the slot holds: YSB_ERR_CAPACITY, or a HIP failure) is dropped, and
 * its error is returned by the call that performs the launch and by every later call that
 * orders work after it, until ysb_reset. */
int         ysb_submit_raw(ysb_ctx* ctx, int slot, const uint8_t* bytes, uint64_t nbytes);
/* Zero-copy raw batches (ABI 5).  ysb_host_register pins and maps caller host memory (a JNI
 * DirectByteBuffer, a replay file read into memory) for this context's device, so that
 * ysb_submit_raw_mapped reads a batch in place over PCIe -- no copy into the pinned slot, no
 * host pass over the bytes (the streaming replay's ingest: FileBasedDataSource.run,
 * AdvertisingTopologyNative.java:144-165, with the source's buffer itself pinned).  Ranges
 * must not overlap; ysb_close unregisters what is left. */
int         ysb_host_register(ysb_ctx* ctx, void* host, uint64_t bytes);
int         ysb_host_unregister(ysb_ctx* ctx, void* host);
/* The replay's event-time rebasing on the device (the data/ generator's batch replay output,
 * core.clj:166-174 played past its first cycle).  A replay cycle's line i holds its 13-digit
 * event_time at byte time_at[i] & 0xFFFF of the line, and its leading nine digits (the
 * 10-second bucket) equal lead_base + (time_at[i] >> 16).  The table (4 B per line) is copied
 * into HBM; n_lines = 0 drops it. */
int         ysb_rebase_table(ysb_ctx* ctx, const uint32_t* time_at, uint64_t n_lines, int64_t lead_base);
typedef struct ysb_rebase {
    uint64_t first_line;   /* the batch's first line is the table's line first_line         */
    int64_t  lead_shift;   /* added to every line's leading nine digits (cycle k of a cycle of
                              c ms: k * c / 10000); the result must lie in [0, 10^9)         */
} ysb_rebase;
/* ysb_submit_raw of a batch that lies in a registered range: at any byte address (a file
 * mapping's batch starts where the previous one's last line ended), the range holding the batch
 * widened to 16-byte boundaries on both sides (the copy reads whole 16-byte vectors).  The copy
 * kernel (or, YSB_F_H2D_SDMA, the DMA
 * engine) reads it in place into the slot's device buffer, the GPU splits the lines, and with
 * rebase != NULL every line's leading event_time digits are rewritten from the rebase table
 * before the scan (YSB_ERR_ARG at the launch if the batch has more lines than the table holds
 * from first_line).  Asynchronous like ysb_submit_raw; the caller must not rewrite the bytes
 * until ysb_wait(ctx, slot).  The slot's pinned host buffer is not used. */
int         ysb_submit_raw_mapped(ysb_ctx* ctx, int slot, const uint8_t* bytes, uint64_t nbytes,
                                  const ysb_rebase* rebase);
/* The same for a batch whose record boundaries the source already knows (a Kafka source's
 * messages; a replay cycle's line offsets, computed once and kept in HBM for every cycle):
 * d_line_off holds n_events u32 offsets into `bytes` in device memory.  No line split: the copy
 * kernel reads the bytes in place, the scan (after the rebase, with rebase != NULL: lines
 * [first_line, first_line + n_events) of the table) is enqueued behind it on the compute stream
 * at once.  The call first waits for the slot's previous copy (at most two in flight); the
 * caller must not rewrite the bytes until ysb_wait(ctx, slot). */
int         ysb_submit_mapped(ysb_ctx* ctx, int slot, const uint8_t* bytes, uint64_t nbytes,
                              const uint32_t* d_line_off, uint64_t n_events, const ysb_rebase* rebase);
/* The same split of a device-resident batch (16-byte aligned, < 4 GiB): d_off[0..*n) <- its
 * line starts (YSB_ERR_CAPACITY, *n = the lines, if more than cap).  Synchronous. */
int         ysb_split_lines_device(ysb_ctx* ctx, const uint8_t* d_bytes, uint64_t nbytes, uint32_t* d_off,
                                   uint64_t cap, uint64_t* n);
/* ---- LZ4-compressed raw batches (additive within ABI 6) ---------------------------------
 * A source whose bytes arrive compressed -- FileBasedDataSource.run
 * (AdvertisingTopologyNative.java:144-165) reading a compressed replay file, or a Kafka
 * consumer's message codec (the reference's Kafka 0.8.2.1 offers LZ4, stream-bench.sh) --
 * decodes them on a CPU before the first operator sees a line.  Here it hands them over as they
 * are: fewer bytes cross PCIe, and the GPU decodes them in front of the line split.
 * A batch is n_blocks independent LZ4 *blocks* (the block format: no frame headers, no
 * dictionary, a match never reaches before its own block) back to back, and this directory;
 * the decoded blocks, back to back in directory order, are the raw batch.  A block decodes to
 * 1..65536 bytes.  Bit 31 of comp_bytes marks a stored block: raw_bytes bytes as they are. */
typedef struct ysb_lz4_block {
    uint32_t comp_bytes;   /* the block's bytes in the batch (| YSB_LZ4_STORED)   */
    uint32_t raw_bytes;    /* what it decodes to: 1..65536                        */
} ysb_lz4_block;
#define YSB_LZ4_STORED  0x80000000u
#define YSB_LZ4_MAX_RAW 65536u
/* ysb_submit_raw for a compressed batch -- replaces the source's decompress-then-readLine loop:
 * the compressed bytes (and nothing else) go through the slot's pinned buffer over PCIe, the
 * blocks are decoded into the slot's device buffer on the stream the split uses, behind the
 * slot's copy, then split and scanned as a raw batch; double-buffering, ysb_wait, ordering and
 * the sticky-error rule are ysb_submit_raw's.  comp_bytes and the sum of raw_bytes must each be
 * <= max_batch_bytes (YSB_ERR_CAPACITY); YSB_ERR_ARG for a raw_bytes of 0 or above 65536 and for
 * a directory whose sizes do not sum to comp_bytes; n_blocks = 0 is an empty batch.  A batch
 * with any block that breaks the format's rules is dropped whole -- none of its lines is
 * counted -- and YSB_ERR_FORMAT, its message naming the first bad block, is returned by the call
 * that would have launched it and by every later one that orders work after it, until
 * ysb_reset.  (The layout sample is taken from block 0 decoded on the host; counts never depend
 * on it.) */
int         ysb_submit_raw_lz4(ysb_ctx* ctx, int slot, const uint8_t* bytes, uint64_t comp_bytes,
                               const ysb_lz4_block* dir, uint32_t n_blocks);
/* The same for a compressed batch that lies in a registered range (ysb_host_register) -- the
 * compressed form of ysb_submit_raw_mapped and ysb_submit_mapped (additive within ABI 6).
 * bytes[0, comp_bytes) are the blocks back to back, at any byte address; the span widened to
 * 16-byte boundaries on both sides must lie inside one registered range.  dir is host memory.
 * The copy kernel (or, YSB_F_H2D_SDMA, the DMA engine) reads the compressed bytes in place into
 * the slot's device staging; the slot's pinned byte buffer is not used and the host makes no
 * pass over the bytes (block 0 apart, which the host model decodes as the layout sample; counts
 * never depend on it); the block descriptors go through the slot's pinned descriptor buffer.
 * The decode runs on the split's stream behind the slot's copy.  Then
 *   d_line_off == NULL (n_events must be 0): the GPU line split;
 *   otherwise: no split, d_line_off[0, n_events) are device offsets into the DECODED batch;
 * then, with rebase != NULL, the rebase on the decoded bytes (from the split: YSB_ERR_ARG at the
 * launch if the batch has more lines than the table holds from first_line; with offsets: at the
 * call).  With offsets too the scan is launched by the next call that orders work, not at once
 * as ysb_submit_mapped's: the verdict on the blocks must be known before a line is counted.
 * The rules are the union of ysb_submit_raw_lz4's (directory, capacity, a bad block drops the
 * batch whole with a sticky YSB_ERR_FORMAT, n_blocks = 0 is an empty batch) and the mapped
 * calls' (registration, rebase arguments, at most two copies in flight: the call first waits
 * for the slot's previous copy; the caller must not rewrite the bytes until
 * ysb_wait(ctx, slot)).  ysb_lz4_info and ysb_copy_time account these batches like the others. */
int         ysb_submit_lz4_mapped(ysb_ctx* ctx, int slot, const uint8_t* bytes, uint64_t comp_bytes,
                                  const ysb_lz4_block* dir, uint32_t n_blocks,
                                  const uint32_t* d_line_off, uint64_t n_events, const ysb_rebase* rebase);
/* The decode alone, as ysb_split_lines_device is the split alone (the codec call of a Kafka
 * consumer or a compressed-file reader, on bytes already in HBM): d_comp (device, any
 * alignment) holds the blocks, dir is host memory, d_out (device, out_cap bytes) receives
 * *raw_bytes bytes.  Synchronous.  *first_bad: the first bad block, or 0xFFFFFFFF; a bad
 * block's output range is left as it was, the other blocks are decoded, and the call returns
 * YSB_ERR_FORMAT.  Argument and capacity errors as above (the capacity is out_cap). */
int         ysb_lz4_decode_device(ysb_ctx* ctx, const uint8_t* d_comp, uint64_t comp_bytes,
                                  const ysb_lz4_block* dir, uint32_t n_blocks, uint8_t* d_out,
                                  uint64_t out_cap, uint64_t* raw_bytes, uint32_t* first_bad);
/* The last compressed batch whose decode has been read back (ysb_submit_raw_lz4: at its launch;
 * ysb_lz4_decode_device: at once).  Read-only measurement and test support; replaces nothing
 * in the reference.  Waits for everything submitted. */
typedef struct ysb_lz4_desc {
    uint64_t batches;        /* compressed batches since ysb_open / ysb_reset      */
    uint64_t blocks;         /* the last batch: its blocks ...                     */
    uint64_t stored_blocks;  /* ... those stored                                   */
    uint64_t comp_bytes;
    uint64_t raw_bytes;
    uint64_t bad_blocks;
    uint64_t first_bad;      /* 0xFFFFFFFF: none                                   */
    double   decode_ms;      /* YSB_F_TIMING: HIP events around its decode kernel  */
} ysb_lz4_desc;
int         ysb_lz4_info(ysb_ctx* ctx, ysb_lz4_desc* info);
uint64_t    ysb_lz4_desc_size(void);   /* sizeof(ysb_lz4_desc) */
/* The host model of the format (csrc/ysb_lz4.h), for callers and tests: what a source without
 * a compressor of its own (or a test) uses in place of the codec library of a Kafka producer.
 * compress_block: src[0, raw_bytes) (1..65536) into dst (cap >= ysb_lz4_compress_bound(raw_bytes),
 * else YSB_ERR_CAPACITY), *entry its directory entry -- stored when allow_stored and the block did
 * not shrink.  decompress_block: YSB_ERR_FORMAT for a block that breaks the rules,
 * YSB_ERR_CAPACITY if cap < entry->raw_bytes.
 * ysb_lz4_pack: a whole buffer cut into blocks of block_bytes (1..65536; with line_aligned
 * every block but the last ends behind a line terminator where its range holds one), *dst_bytes
 * and *n_blocks out; dst_cap >= nbytes + nbytes / 255 + 16 * blocks and dir_cap >= the blocks
 * (ceil(nbytes / block_bytes) without line_aligned), else YSB_ERR_CAPACITY with both counts set
 * to what is needed.  threads > 1 compresses blocks in parallel (at most 16). */
uint32_t    ysb_lz4_compress_bound(uint32_t raw_bytes);
int         ysb_lz4_compress_block(const uint8_t* src, uint32_t raw_bytes, uint8_t* dst, uint32_t cap,
                                   int allow_stored, ysb_lz4_block* entry);
int         ysb_lz4_decompress_block(const uint8_t* src, const ysb_lz4_block* entry, uint8_t* dst,
                                     uint32_t cap);
int         ysb_lz4_pack(const uint8_t* src, uint64_t nbytes, uint32_t block_bytes, int line_aligned,
                         int allow_stored, int threads, uint8_t* dst, uint64_t dst_cap, uint64_t* dst_bytes,
                         ysb_lz4_block* dir, uint64_t dir_cap, uint64_t* n_blocks);
/* A compressed replay file (ysb_gen --lz4 writes it, ysb_topology --lz4 reads it): this header,
 * n_blocks directory entries, then the blocks back to back; all fields little-endian.  With
 * YSB_LZ4_FILE_LINE_ALIGNED every block ends behind a line terminator (or at the file's end),
 * so any run of whole blocks is a raw batch of whole lines.  ysb_lz4_write_file compresses
 * src[0, nbytes) with ysb_lz4_pack's parameters into `path` (YSB_ERR_ARG if it cannot be
 * written). */
typedef struct ysb_lz4_file_header {
    char     magic[8];     /* YSB_LZ4_FILE_MAGIC                          */
    uint32_t version;      /* 1                                           */
    uint32_t flags;        /* YSB_LZ4_FILE_LINE_ALIGNED                   */
    uint64_t n_blocks;
    uint64_t raw_bytes;    /* the sum of the directory's raw_bytes        */
} ysb_lz4_file_header;
#define YSB_LZ4_FILE_MAGIC        "YSBLZ4B\n"   /* 8 bytes, no terminator */
#define YSB_LZ4_FILE_LINE_ALIGNED 1u
int         ysb_lz4_write_file(const char* path, const uint8_t* src, uint64_t nbytes, uint32_t block_bytes,
                               int line_aligned, int allow_stored, int threads);
/* ---- standard LZ4 frames (additive within ABI 6) -----------------------------------------
 * What `lz4 -B4`, liblz4's LZ4F_*, Python's lz4.frame and a Kafka LZ4 codec write: a frame
 * records only each block's COMPRESSED size, so the directory above cannot be filled without a
 * pass over the tokens.  Here the host reads one size word per block (ysb_lz4_frame_index) and
 * the GPU finds the raw sizes (the measure pass) in front of the decode.
 * ysb_lz4_frame_index walks bytes[0, nbytes), one or more concatenated frames and skippable
 * frames (magic 0x184D2A50..5F), and fills one entry per data block: `offset` is the block's
 * first data byte (behind its 4-byte size word), comp_bytes its size | YSB_LZ4_STORED.  Accepted:
 * magic 04 22 4D 18, version 01, independent blocks, a block maximum of 64 KiB (BD id 4), an
 * optional content size, block checksums and a content checksum (skipped and reported, never
 * verified); the header checksum byte is verified.  YSB_ERR_FORMAT, the message naming the byte
 * offset and the rule, for: another or the legacy magic, another version, reserved bits, a
 * header checksum mismatch, linked blocks, a dictionary id, a block maximum above 64 KiB, a
 * block size word above the maximum, a stored block of no bytes, and any truncation (no byte
 * at or past nbytes is read).  YSB_ERR_CAPACITY with *n_blocks set when cap is short (blocks
 * may be NULL with cap 0 to count).  info may be NULL.  No context: the message is the
 * thread's (ysb_last_error(NULL)). */
typedef struct ysb_lz4_frame_block {
    uint64_t offset;       /* of the block's first data byte in the indexed buffer */
    uint32_t comp_bytes;   /* its bytes there (| YSB_LZ4_STORED)                   */
    uint32_t reserved;     /* 0                                                    */
} ysb_lz4_frame_block;
typedef struct ysb_lz4_frame_summary {
    uint64_t frames;            /* LZ4 frames (skippable ones not counted)       */
    uint64_t skippable_frames;
    uint64_t blocks;            /* data blocks of all frames                     */
    uint64_t stored_blocks;
    uint64_t comp_bytes;        /* the sum of the blocks' sizes                  */
    uint64_t content_bytes;     /* the sum of the content sizes that were stated */
    uint32_t block_checksums;   /* frames with block checksums ...               */
    uint32_t content_checksums; /* ... with a content checksum ...               */
    uint32_t content_sizes;     /* ... with a content size                       */
    uint32_t reserved;
} ysb_lz4_frame_summary;
int         ysb_lz4_frame_index(const uint8_t* bytes, uint64_t nbytes, ysb_lz4_frame_block* blocks, uint64_t cap,
                                uint64_t* n_blocks, ysb_lz4_frame_summary* info);
/* src[0, nbytes) as ONE standard frame any LZ4 tool reads: independent blocks, 64 KiB block
 * maximum, no checksums, the content size set; blocks of block_bytes (1..65536; below 65536:
 * short blocks, valid in a 64 KiB frame) from the library's greedy compressor, a block that did
 * not shrink stored.  ysb_lz4_frame_pack writes into dst (dst_cap >= ysb_lz4_frame_bound(nbytes,
 * block_bytes), else YSB_ERR_CAPACITY with *dst_bytes the bound); ysb_lz4_frame_write into a
 * file.  threads > 1 compresses blocks in parallel (at most 16). */
uint64_t    ysb_lz4_frame_bound(uint64_t nbytes, uint32_t block_bytes);
int         ysb_lz4_frame_pack(const uint8_t* src, uint64_t nbytes, uint32_t block_bytes, int threads, uint8_t* dst,
                               uint64_t dst_cap, uint64_t* dst_bytes);
int         ysb_lz4_frame_write(const char* path, const uint8_t* src, uint64_t nbytes, uint32_t block_bytes,
                                int threads);
/* The host model of the measure pass: the raw size (1..65536) of one frame block src[0, comp)
 * (comp_field: its index entry's comp_bytes, with the stored bit), found by a walk of its tokens
 * alone.  YSB_ERR_FORMAT for a block that no raw size makes valid. */
int         ysb_lz4_measure_block(const uint8_t* src, uint32_t comp_field, uint32_t* raw_bytes);
/* The carry rule of a stream of frame batches, for a source that feeds decoded batches itself
 * and for tests: of data[0, n) -- a batch's decoded bytes behind what the batch before left
 * over -- how many bytes are whole lines; the rest is carried in front of the next batch.  The
 * cut is behind the last '\n', or behind the last '\r' that is not the buffer's last byte (a
 * '\r' there may be half of a "\r\n" whose '\n' opens the next batch: the whole last line is
 * carried).  more == 0 (the stream's last batch): n, the tail is a line as in ysb_submit_raw. */
uint64_t    ysb_lz4_frame_carry_cut(const uint8_t* data, uint64_t n, int more);
/* The measure pass alone and measure + decode, device to device (synchronous; test support and
 * the codec call of another GPU operator).  d_base (device, any alignment) is the buffer the
 * index entries' offsets refer to; blocks is host memory.
 * ysb_lz4_measure_device: raw_out[i] (host) <- block i's raw size, 0 for a bad block;
 * *first_bad the first such block or 0xFFFFFFFF (then YSB_ERR_FORMAT is returned).
 * ysb_lz4_decode_blocks_device: the blocks' bytes back to back into d_out; *raw_bytes the
 * measured total (YSB_ERR_CAPACITY, nothing decoded, if above out_cap); a bad block's range --
 * it has none: its measured size is 0 -- is skipped, the other blocks are decoded, and the call
 * returns YSB_ERR_FORMAT with *first_bad set. */
int         ysb_lz4_measure_device(ysb_ctx* ctx, const uint8_t* d_base, const ysb_lz4_frame_block* blocks,
                                   uint32_t n_blocks, uint32_t* raw_out, uint32_t* first_bad);
int         ysb_lz4_decode_blocks_device(ysb_ctx* ctx, const uint8_t* d_base, const ysb_lz4_frame_block* blocks,
                                         uint32_t n_blocks, uint8_t* d_out, uint64_t out_cap, uint64_t* raw_bytes,
                                         uint32_t* first_bad);
/* A frame batch through a slot -- ysb_submit_raw_lz4 for a standard frame: blocks[0, n_blocks) is
 * a run of consecutive entries of ysb_lz4_frame_index over `base` (host memory).  The span from
 * the first block's data to the last block's end (size and checksum words between them included)
 * goes through the slot's pinned buffer, or (_mapped) is read in place from a registered range
 * (ysb_host_register; the span widened to 16-byte boundaries must lie inside one).  On the
 * split's stream behind the slot's copy: the measure pass, the descriptors, the decode, the
 * carry, the line split (its byte count read from device memory); the scan launches at the
 * next call that orders work, as for every raw batch.  Frame blocks end mid-line: with
 * YSB_LZ4F_MORE in flags the bytes behind the batch's last certain line terminator
 * (ysb_lz4_frame_carry_cut's rule) are no line but are kept on the device (at most 64 KiB) and
 * put in front of the next frame batch; without it the tail is a line, as in ysb_submit_raw.
 * YSB_ERR_CAPACITY unless the span and (n_blocks + 1) x 65536 are both <= max_batch_bytes;
 * YSB_ERR_ARG for entries that are not consecutive or not 1..65536 bytes, unknown flags, a span
 * outside a registered range.  A batch with a bad block is dropped whole (sticky
 * YSB_ERR_FORMAT naming the block), as is one that leaves more than 64 KiB behind its last
 * terminator (sticky YSB_ERR_CAPACITY); the carry is emptied then and by ysb_reset.  While a
 * carry is pending (the last frame batch queued had YSB_LZ4F_MORE) every other submit -- lines,
 * compressed batches, device batches, column batches -- returns YSB_ERR_STATE.  The layout sample is block 0 decoded by the host model; counts never depend
 * on it.  ysb_lz4_frame_info reports the last frame batch settled. */
#define YSB_LZ4F_MORE 1u
int         ysb_submit_lz4_blocks(ysb_ctx* ctx, int slot, const uint8_t* base, const ysb_lz4_frame_block* blocks,
                                  uint32_t n_blocks, uint32_t flags);
int         ysb_submit_lz4_blocks_mapped(ysb_ctx* ctx, int slot, const uint8_t* base,
                                         const ysb_lz4_frame_block* blocks, uint32_t n_blocks, uint32_t flags);
/* Which decode kernel the context's LZ4 calls launch: 0 by the batch's largest block (the
 * default: one wave per block up to 16 KiB of raw bytes, the several-wave kernel above),
 * 1 always the one-wave kernel, 2 always the several-wave kernel.  Results never depend on it;
 * tests and tools/bench_lz4.py run both on every shape. */
#define YSB_LZ4_DECODER_AUTO   0
#define YSB_LZ4_DECODER_NARROW 1
#define YSB_LZ4_DECODER_WIDE   2
int         ysb_lz4_set_decoder(ysb_ctx* ctx, int decoder);
/* The last synchronous call above, or the last frame batch settled (read-only measurement and
 * test support).  Waits for everything submitted. */
typedef struct ysb_lz4_frame_desc {
    uint64_t blocks;
    uint64_t stored_blocks;
    uint64_t comp_bytes;
    uint64_t raw_bytes;      /* the measured total                                  */
    uint64_t bad_blocks;
    uint64_t first_bad;      /* 0xFFFFFFFF: none                                    */
    uint64_t decoder;        /* YSB_LZ4_DECODER_NARROW / _WIDE: which ran (0: none) */
    uint64_t batches;        /* frame batches settled since ysb_open / ysb_reset    */
    uint64_t carry_in;       /* a frame batch: bytes carried in front of it ...     */
    uint64_t carry_out;      /* ... and behind its last certain line terminator     */
    double   measure_ms;     /* YSB_F_TIMING: HIP events around the measure and
                                descriptor kernels ...                              */
    double   decode_ms;      /* ... and around the decode kernel                    */
} ysb_lz4_frame_desc;
int         ysb_lz4_frame_info(ysb_ctx* ctx, ysb_lz4_frame_desc* info);
uint64_t    ysb_lz4_frame_desc_size(void);   /* sizeof(ysb_lz4_frame_desc) */
/* ---- Kafka record batches (additive within ABI 6) ----------------------------------------
 * What a Kafka consumer holds -- the reference's ingest: the ad-events topic, KafkaSpout
 * (AdvertisingTopology.java), the fork's FlinkKafkaConsumer -- is a fetch response: a run of
 * record batches (message format v2, Kafka >= 0.11; a partition's .log segment is the same bytes).
 * The event values lie between varint-framed record headers, so they are neither newline-
 * separated nor back to back.  Here the framed bytes cross PCIe as they are: the host reads one
 * 61-byte header per batch (ysb_kafka_index), the GPU walks the records, finds the values and
 * gathers them back to back with their offsets in front of the unchanged scan.
 * ysb_kafka_index walks bytes[0, nbytes) and fills one entry per data batch.  A last batch that
 * is not whole is normal in a fetch response and no error: info->consumed stops in front of it,
 * so the caller keeps the tail.  Control batches are skipped and counted.  YSB_ERR_FORMAT, the
 * message naming the byte offset, the field, its value and the rule, for: a magic other than 2
 * (message formats v0 / v1), a codec other than 0 (compressed batches), batchLength < 49, a
 * negative recordsCount and, with YSB_KAFKA_CHECK_CRC, a CRC-32C mismatch (verified on the host,
 * in software: a pass over the bytes, so off by default; YSB_KAFKA_CHECK_CRC_CONTROL verifies only
 * the control batches the index skips -- with ysb_kafka_set_crc's device check of the indexed
 * batches, every byte a check.crcs=true consumer verifies).  YSB_ERR_CAPACITY with info complete
 * when cap is short (batches may be NULL with cap 0 to count).  No context: the message is the
 * thread's (ysb_last_error(NULL)). */
typedef struct ysb_kafka_batch {
    uint64_t records_off;     /* of the batch's first record byte in the indexed buffer      */
    uint32_t records_bytes;   /* its records' bytes: batchLength - 49                        */
    uint32_t n_records;       /* recordsCount                                                */
    uint64_t first_record;    /* the records of the entries before it: the running sum       */
    int64_t  base_offset;     /* baseOffset                                                  */
    uint32_t control_before;  /* control batches skipped between the entry before and this   */
    uint32_t reserved;        /* 0                                                           */
} ysb_kafka_batch;
typedef struct ysb_kafka_summary {
    uint64_t n_batches;       /* data batches                                   */
    uint64_t n_records;
    uint64_t consumed;        /* bytes of whole batches: the rest is the tail   */
    uint64_t control_batches; /* skipped                                        */
    uint64_t crc_checked;     /* batches whose CRC-32C was verified             */
} ysb_kafka_summary;
#define YSB_KAFKA_CHECK_CRC 1u
#define YSB_KAFKA_CHECK_CRC_CONTROL 2u
int         ysb_kafka_index(const uint8_t* bytes, uint64_t nbytes, uint32_t flags, ysb_kafka_batch* batches,
                            uint64_t cap, ysb_kafka_summary* info);
uint32_t    ysb_kafka_crc32c(const uint8_t* bytes, uint64_t nbytes);   /* "123456789" -> 0xE3069283 */
/* Why a batch is bad: a record of it breaks a rule.  rule: 1 a varint runs past its limit (5
 * bytes; timestampDelta 10) or its extent, 2 length < 6, 3 the record runs past the batch, 4 the
 * key runs past the record (or its length is below -1), 5 the same for the value, 6 the headers
 * do not end exactly at the record's end (or a negative count / header key length), 7 the walk
 * does not yield exactly recordsCount records ending exactly at the batch's end (record: where
 * it stopped), 8 (compressed batches only, below) a block of the batch's LZ4 frame does not
 * decode (record: the block), 9 (only where the CRC is checked: ysb_kafka_set_crc,
 * ysb_kafka_verdict_crc_host) the batch's CRC-32C differs from the stored one (record 0; it comes
 * first: no record of such a batch is looked at).  The verdict names the smallest bad batch and
 * its smallest bad record. */
typedef struct ysb_kafka_verdict {
    uint32_t bad_batches;
    uint32_t first_bad;       /* index entry; 0xFFFFFFFF: none */
    uint32_t record;          /* within that batch             */
    uint32_t rule;
} ysb_kafka_verdict;
typedef struct ysb_kafka_counters {
    uint64_t records;
    uint64_t null_values;     /* valueLength -1 (an empty value is not counted)  */
    uint64_t keyed;           /* records with a key (an empty one included)      */
    uint64_t headers;         /* record headers in all                           */
    uint64_t value_bytes;
} ysb_kafka_counters;
/* The host model of the GPU's unframing (csrc/ysb_kafka.h): the values of every record of the
 * indexed batches back to back into out, line_off[0 .. n] their offsets (line_off[n]: the
 * total; off_cap >= n + 1), the counters.  A null value and an empty value are both a line of no
 * bytes.  out / line_off NULL: sizes and counters only.  YSB_ERR_FORMAT with *verdict set for a
 * bad batch (nothing of a bad batch is written); YSB_ERR_ARG for an index entry outside the
 * buffer or with a wrong running sum; YSB_ERR_CAPACITY when out or line_off is short or the
 * values pass 4 GiB (u32 offsets). */
int         ysb_kafka_unframe_host(const uint8_t* bytes, uint64_t nbytes, const ysb_kafka_batch* batches,
                                   uint64_t n_batches, uint8_t* out, uint64_t out_cap, uint32_t* line_off,
                                   uint64_t off_cap, uint64_t* n_lines, uint64_t* out_bytes,
                                   ysb_kafka_counters* counters, ysb_kafka_verdict* verdict);
/* The packer (a test's, a tool's or a source's stand-in for a producer): lines
 * [line_off[i], line_off[i + 1]) of src (the last one ends at nbytes) as record batches.  A batch
 * is closed before the record that would take it past batch_bytes bytes (header included; a
 * batch holds one record at least) or past batch_records records (0: no such limit).  Record i
 * gets offset base_offset + i; keys are null (key_off NULL) or key i is keys[key_off[i],
 * key_off[i + 1]); ts_delta NULL: 0; the n_headers headers (a value length of -1: null) go on
 * every record.  baseOffset, offsetDelta, lastOffsetDelta, maxTimestamp and the CRC-32C are
 * what a consumer checks.  dst_cap >= ysb_kafka_bound(...), else YSB_ERR_CAPACITY with
 * *dst_bytes the bound. */
typedef struct ysb_kafka_pack_opts {
    uint32_t        batch_bytes;
    uint32_t        batch_records;
    int64_t         base_offset;
    int64_t         base_timestamp;
    const uint32_t* key_off;         /* n_lines + 1 offsets into keys, or NULL */
    const uint8_t*  keys;
    const int64_t*  ts_delta;        /* n_lines, or NULL                       */
    uint32_t        n_headers;
    uint32_t        codec;           /* 0: uncompressed; YSB_KAFKA_CODEC_LZ4: each batch's records as one
                                        standard LZ4 frame (64 KiB independent blocks, a block that does not
                                        shrink stored), attributes = 3, the CRC over the wire bytes;
                                        YSB_KAFKA_CODEC_SNAPPY: as snappy (snappy_framing below), attributes
                                        = 2; any other value: YSB_ERR_ARG                                   */
    const char* const*    header_keys;      /* NUL-terminated                  */
    const uint8_t* const* header_vals;
    const int32_t*        header_val_len;   /* -1: a null value                */
    uint32_t        snappy_framing;  /* codec YSB_KAFKA_CODEC_SNAPPY: YSB_KAFKA_SNAPPY_XERIAL (0, the Java client's
                                        stream of chunks) or _RAW (one raw block per batch, as librdkafka writes:
                                        YSB_ERR_ARG where a batch's records pass 64 KiB)                     */
    uint32_t        snappy_chunk;    /* raw bytes per xerial chunk: 0 takes the client's 32 KiB, at most 65536 */
} ysb_kafka_pack_opts;
uint64_t    ysb_kafka_bound(uint64_t nbytes, uint64_t n_lines, const ysb_kafka_pack_opts* opts);
int         ysb_kafka_pack(const uint8_t* src, uint64_t nbytes, const uint32_t* line_off, uint64_t n_lines,
                           const ysb_kafka_pack_opts* opts, uint8_t* dst, uint64_t dst_cap, uint64_t* dst_bytes,
                           uint64_t* n_batches);
int         ysb_kafka_write_file(const char* path, const uint8_t* src, uint64_t nbytes, const uint32_t* line_off,
                                 uint64_t n_lines, const ysb_kafka_pack_opts* opts);
/* The unframing alone, device to device (synchronous, like ysb_lz4_decode_device): d_bytes
 * (device, any alignment; the 16-byte vectors that hold its first and last byte are read whole)
 * holds the framed bytes that `batches` (host memory) indexes; d_out (out_cap bytes) receives the
 * values back to back, d_line_off (off_cap >= records + 1 entries) their offsets and the total.
 * Three launches: a walk (one wave per Kafka batch), a scan of the batches' totals, a gather.
 * Returns as ysb_kafka_unframe_host does; with a bad batch nothing is written to d_out or
 * d_line_off. */
int         ysb_kafka_unframe_device(ysb_ctx* ctx, const uint8_t* d_bytes, uint64_t nbytes,
                                     const ysb_kafka_batch* batches, uint64_t n_batches, uint8_t* d_out,
                                     uint64_t out_cap, uint32_t* d_line_off, uint64_t off_cap, uint64_t* n_lines,
                                     uint64_t* out_bytes);
/* A run of whole Kafka batches through a slot -- what replaces the consumer's per-record
 * deserialisation loop in front of the first operator: bytes[0, nbytes) is (part of) the buffer
 * that `batches` indexes (records_off relative to `bytes`; first_record running from 0).  The
 * framed bytes and the index are what crosses PCIe, into a device staging buffer that is not
 * the slot's device buffer: through the slot's pinned buffer, or (_mapped) read in place from a
 * registered range (ysb_host_register) at any byte address, the span widened to 16-byte
 * boundaries inside one range.  On the split's stream behind the slot's copy the three kernels
 * leave the values, their offsets and the count in the slot's device buffers; no line split
 * runs; the scan launches at the next call that orders work, as for every raw batch.
 * YSB_ERR_CAPACITY at the call for nbytes above max_batch_bytes or more records than the
 * slot's line capacity (ysb_submit_raw's).  A bad Kafka batch drops the whole slot batch: a
 * sticky YSB_ERR_FORMAT naming the Kafka batch, its baseOffset, the record and the rule, from
 * the call that would have launched it and every later one that orders work, until ysb_reset.
 * The layout sample is the first batch's first values as the host model unframes them; counts
 * never depend on it.  No rebase; YSB_ERR_STATE while a frame batch's carry is pending. */
int         ysb_submit_kafka(ysb_ctx* ctx, int slot, const uint8_t* bytes, uint64_t nbytes,
                             const ysb_kafka_batch* batches, uint64_t n_batches);
int         ysb_submit_kafka_mapped(ysb_ctx* ctx, int slot, const uint8_t* bytes, uint64_t nbytes,
                                    const ysb_kafka_batch* batches, uint64_t n_batches);
/* The last Kafka call settled (a slot batch: at its launch; ysb_kafka_unframe_device: at once).
 * Read-only measurement and test support.  Waits for everything submitted. */
typedef struct ysb_kafka_desc {
    uint64_t calls;            /* Kafka submits and unframe calls since ysb_open / ysb_reset */
    uint64_t batches;          /* the last call: its Kafka batches ...                       */
    uint64_t records;
    uint64_t null_values;
    uint64_t keyed;
    uint64_t headers;
    uint64_t control_skipped;  /* control batches the index skipped among them               */
    uint64_t framed_bytes;
    uint64_t value_bytes;
    uint64_t window_bytes;     /* the walk kernel's window                                   */
    ysb_kafka_verdict verdict;
    double   walk_ms;          /* YSB_F_TIMING: HIP events around each kernel                */
    double   base_ms;
    double   gather_ms;
} ysb_kafka_desc;
int         ysb_kafka_info(ysb_ctx* ctx, ysb_kafka_desc* info);
uint64_t    ysb_kafka_batch_size(void);      /* sizeof(ysb_kafka_batch)     */
uint64_t    ysb_kafka_summary_size(void);
uint64_t    ysb_kafka_verdict_size(void);
uint64_t    ysb_kafka_counters_size(void);
uint64_t    ysb_kafka_pack_opts_size(void);
uint64_t    ysb_kafka_desc_size(void);
/* ---- Kafka record batches: CRC-32C on the GPU (additive within ABI 6) -----------------------
 * What a consumer with check.crcs=true does before it reads a record, on the device, where the
 * bytes already are: one launch behind the walk (and the codec verdict) and in front of the scan
 * of the batches' totals verifies every indexed batch -- the range [records_off - 40, records_off
 * + records_bytes) against the big-endian word at records_off - 44; on the compressed path the
 * wire bytes.  A batch whose CRC differs is bad by rule 9, whatever the walk or the decoder made
 * of its bytes.  Only the 16-byte vectors that hold [records_off - 44, records_off +
 * records_bytes) are loaded.
 * ysb_kafka_set_crc: YSB_KAFKA_CRC_OFF (the default: no launch, no memory) or _DEVICE (anything
 * else: YSB_ERR_ARG).  A context setting, kept across ysb_reset; a slot batch is verified by the
 * mode in force when it was submitted.  With the mode on, ysb_submit_kafka, _mapped, _lz4,
 * _lz4_mapped, ysb_kafka_unframe_device and _lz4_device verify, and YSB_ERR_ARG for an index
 * entry with records_off < 44.  The sticky YSB_ERR_FORMAT of a dropped slot batch names the
 * Kafka batch, its baseOffset and the stored and the computed value. */
#define YSB_KAFKA_CRC_OFF 0
#define YSB_KAFKA_CRC_DEVICE 1
int         ysb_kafka_set_crc(ysb_ctx* ctx, int mode);
/* The kernel alone, synchronously, whatever the mode: computed[k] / stored[k] (host arrays of
 * n_batches; stored may be NULL) for the batches of an index over d_bytes (device, any
 * alignment).  No verdict: a difference is the caller's to see. */
int         ysb_kafka_crc_device(ysb_ctx* ctx, const uint8_t* d_bytes, uint64_t nbytes, const ysb_kafka_batch* batches,
                                 uint64_t n_batches, uint32_t* computed, uint32_t* stored);
/* The last call that verified (a slot batch: at its launch).  Waits for everything submitted. */
typedef struct ysb_kafka_crc_desc {
    uint64_t calls;           /* calls that ran the kernel since ysb_open / ysb_reset         */
    uint64_t mode;            /* the context's setting                                        */
    uint64_t batches;         /* the last such call: batches verified ...                     */
    uint64_t bytes;           /* ... and the bytes their CRCs cover                           */
    uint64_t bad_batches;     /* batches whose CRC differs                                    */
    uint64_t first_bad;       /* 0xFFFFFFFF: none                                             */
    uint32_t stored;          /* of first_bad                                                 */
    uint32_t computed;
    uint64_t grid_waves;      /* the waves of the kernel's largest grid, one batch each at a
                                 time: a call with more batches turns the kernel's loop       */
    double   crc_ms;          /* YSB_F_TIMING: HIP events around the kernel                   */
} ysb_kafka_crc_desc;
int         ysb_kafka_crc_info(ysb_ctx* ctx, ysb_kafka_crc_desc* info);
uint64_t    ysb_kafka_crc_desc_size(void);
/* The host models with the same rule: the verdict ysb_kafka_unframe_host / _lz4_host give when
 * every batch's CRC is checked first (rule 9).  YSB_OK or YSB_ERR_FORMAT (the message naming the
 * batch and, for rule 9, both values) with *verdict set; YSB_ERR_ARG as those, and for an entry
 * with records_off < 44. */
int         ysb_kafka_verdict_crc_host(const uint8_t* bytes, uint64_t nbytes, const ysb_kafka_batch* batches,
                                       uint64_t n_batches, ysb_kafka_verdict* verdict);
/* ---- LZ4-compressed Kafka record batches (additive within ABI 6) ---------------------------
 * A topic whose producers set compression.type=lz4: in message format v2 the 61-byte batch header
 * stays as it is and the records section is ONE standard LZ4 frame (attributes codec 3).  The
 * Java client writes FLG 0x60 / BD 0x40 and an EndMark, librdkafka LZ4F_blockIndependent with the
 * default block size: independent blocks of at most 64 KiB, which is what ysb_lz4_frame_index
 * accepts.  Everything here is opt-in: ysb_kafka_index and the submits above keep refusing any
 * codec.  The wire bytes and three index arrays cross PCIe; the GPU measures the blocks, plans
 * the inflated layout (the walk's index is made on the device: the host never learns a batch's
 * raw size), decodes, then walks, scans and gathers as above.
 * ysb_kafka_index_lz4 is ysb_kafka_index for codec 0 and codec 3: batches[k] as above
 * (records_off / records_bytes: the wire bytes, for codec 3 the frame; n_records, first_record
 * and base_offset from the header), frames[k] the blocks of entry k, blocks[] every block's
 * place in the indexed buffer.  A codec-0 batch's records become stored blocks of at most 64 KiB,
 * so a mixed fetch response takes one path.  YSB_ERR_FORMAT naming the Kafka batch, its byte, and
 * the frame's byte and rule (with the way out where ysb_lz4_frame_index gives one: linked blocks,
 * a block maximum above 64 KiB) for every frame refusal, truncation inside the records and bytes
 * behind the last frame included; codecs 1, 2 and 4 are refused by name (gzip, snappy, zstd:
 * have the producer write lz4 or none; snappy is read with YSB_KAFKA_ACCEPT_SNAPPY, below).  cap counts batches and frames, block_cap blocks;
 * YSB_ERR_CAPACITY with info complete when either is short (NULL arrays with 0 caps count). */
#define YSB_KAFKA_CODEC_LZ4 3u
typedef struct ysb_kafka_frame {
    uint64_t first_block;     /* the blocks of the entries before it: the running sum */
    uint32_t n_blocks;        /* at most 32767                                        */
    uint32_t codec;           /* 0 (stored blocks over the records) or 3              */
} ysb_kafka_frame;
typedef struct ysb_kafka_lz4_summary {
    uint64_t n_batches;       /* as ysb_kafka_summary ...                        */
    uint64_t n_records;
    uint64_t consumed;
    uint64_t control_batches;
    uint64_t crc_checked;
    uint64_t compressed_batches; /* ... and: data batches with codec 3           */
    uint64_t blocks;          /* entries of blocks[]                             */
    uint64_t stored_blocks;   /* a frame's stored blocks and the codec-0 batches' */
    uint64_t comp_bytes;      /* the sum of the blocks' sizes on the wire        */
} ysb_kafka_lz4_summary;
int         ysb_kafka_index_lz4(const uint8_t* bytes, uint64_t nbytes, uint32_t flags, ysb_kafka_batch* batches,
                                ysb_kafka_frame* frames, uint64_t cap, ysb_lz4_frame_block* blocks, uint64_t block_cap,
                                ysb_kafka_lz4_summary* info);
/* The host model (csrc/ysb_kafka_lz4.h): each batch's blocks decoded by the host block decoder,
 * then ysb_kafka_unframe_host's walk over the result.  verdict->rule 8: a block of the batch's
 * frame does not decode (the measure walk or the decoder refuses it); `record` is then the
 * smallest such block within the batch.  The verdict is the smallest bad batch, whichever kind
 * of fault it has; bad_batches counts both kinds.  *inflated (may be NULL): the good batches'
 * decoded bytes.  YSB_ERR_ARG for entries that break their rules (a frame entry's running block
 * sum, a block outside its batch's wire bytes or not 1..65536 bytes). */
int         ysb_kafka_unframe_lz4_host(const uint8_t* bytes, uint64_t nbytes, const ysb_kafka_batch* batches,
                                       const ysb_kafka_frame* frames, uint64_t n_batches,
                                       const ysb_lz4_frame_block* blocks, uint64_t n_blocks, uint8_t* out,
                                       uint64_t out_cap, uint32_t* line_off, uint64_t off_cap, uint64_t* n_lines,
                                       uint64_t* out_bytes, uint64_t* inflated, ysb_kafka_counters* counters,
                                       ysb_kafka_verdict* verdict);
/* The inflate and the unframing alone, device to device (synchronous): as
 * ysb_kafka_unframe_device, with the chain measure, plan, decode, walk, codec verdict, base,
 * gather on one stream.  The inflated bytes go to a buffer of the context's own (n_blocks x 64
 * KiB, grown on demand).  Same outputs and returns; rule 8 in ysb_kafka_info's verdict. */
int         ysb_kafka_unframe_lz4_device(ysb_ctx* ctx, const uint8_t* d_bytes, uint64_t nbytes,
                                         const ysb_kafka_batch* batches, const ysb_kafka_frame* frames,
                                         uint64_t n_batches, const ysb_lz4_frame_block* blocks, uint64_t n_blocks,
                                         uint8_t* d_out, uint64_t out_cap, uint32_t* d_line_off, uint64_t off_cap,
                                         uint64_t* n_lines, uint64_t* out_bytes);
/* ysb_submit_kafka / _mapped for batches indexed by ysb_kafka_index_lz4 (offsets relative to
 * `bytes`).  The host cannot know raw sizes, so the capacity rule is the guaranteed bound:
 * YSB_ERR_CAPACITY at the call unless nbytes <= max_batch_bytes and n_blocks x 65536 <=
 * max_batch_bytes (and the record-count rule above).  The inflated buffer, max_batch_bytes + 64
 * per slot, is allocated at a slot's first compressed submit: a context that never calls these
 * pays nothing.  A batch with a bad block or a bad record drops the whole slot batch (sticky
 * YSB_ERR_FORMAT until ysb_reset, the message naming the batch and the block or record).
 * YSB_ERR_STATE while a frame batch's carry is pending. */
int         ysb_submit_kafka_lz4(ysb_ctx* ctx, int slot, const uint8_t* bytes, uint64_t nbytes,
                                 const ysb_kafka_batch* batches, const ysb_kafka_frame* frames, uint64_t n_batches,
                                 const ysb_lz4_frame_block* blocks, uint64_t n_blocks);
int         ysb_submit_kafka_lz4_mapped(ysb_ctx* ctx, int slot, const uint8_t* bytes, uint64_t nbytes,
                                        const ysb_kafka_batch* batches, const ysb_kafka_frame* frames,
                                        uint64_t n_batches, const ysb_lz4_frame_block* blocks, uint64_t n_blocks);
/* The inflate half of the last compressed Kafka call settled (ysb_kafka_info keeps reporting its
 * walk, base and gather).  Waits for everything submitted. */
typedef struct ysb_kafka_lz4_desc {
    uint64_t calls;              /* compressed Kafka calls since ysb_open / ysb_reset      */
    uint64_t blocks;
    uint64_t stored_blocks;
    uint64_t compressed_batches;
    uint64_t wire_bytes;
    uint64_t inflated_bytes;     /* the measured total                                     */
    uint64_t bad_blocks;         /* refused by the measure pass or by the decoder          */
    uint64_t decoder;            /* YSB_LZ4_DECODER_NARROW / _WIDE: which ran (0: none); 3:
                                    both, each on its size class (blocks of up to 16 KiB of
                                    raw bytes the one-wave kernel: _AUTO, where only the
                                    device knows the sizes)                                */
    uint64_t inflated_buffer_bytes; /* the context's inflated buffers in all (0: none yet) */
    uint64_t inflated_total;     /* inflated_bytes of every call since ysb_open / ysb_reset */
    double   measure_ms;         /* YSB_F_TIMING: HIP events around each kernel            */
    double   plan_ms;
    double   decode_ms;
    uint64_t snappy_blocks;      /* of `blocks`: those tagged YSB_SNAPPY_BLOCK             */
    double   preamble_ms;        /* YSB_F_TIMING: the snappy preamble kernel               */
} ysb_kafka_lz4_desc;
int         ysb_kafka_lz4_info(ysb_ctx* ctx, ysb_kafka_lz4_desc* info);
int         ysb_kafka_verdict_crc_lz4_host(const uint8_t* bytes, uint64_t nbytes, const ysb_kafka_batch* batches,
                                           const ysb_kafka_frame* frames, uint64_t n_batches,
                                           const ysb_lz4_frame_block* blocks, uint64_t n_blocks,
                                           ysb_kafka_verdict* verdict);   /* ysb_kafka_verdict_crc_host, compressed */
uint64_t    ysb_kafka_frame_size(void);
uint64_t    ysb_kafka_lz4_summary_size(void);
uint64_t    ysb_kafka_lz4_desc_size(void);
/* ---- snappy-compressed Kafka record batches (additive within ABI 6) -------------------------
 * A topic whose producers set compression.type=snappy (attributes codec 2).  The 61-byte batch
 * header stays as it is, the CRC-32C covers the wire bytes, and the records section is either the
 * Java client's xerial stream -- a 16-byte header (magic 82 'SNAPPY' 00, version, compatible
 * version 1) and chunks of a big-endian int32 length and one raw snappy block, 32 KiB of raw
 * bytes by default -- or, without that magic, one raw block (librdkafka, sarama, kafka-python).
 * A raw block opens with its raw size as a varint, so no measure pass runs over it: a thread per
 * block reads the preamble (snappy_preamble_kernel), the plan and the rest of the compressed
 * chain stay as they are, and snappy_decode_kernel decodes a block per wave beside the LZ4
 * kernels, each skipping the other's blocks: a fetch response of codecs 0, 2 and 3 takes one call.
 * Opt-in twice.  At the index: ysb_kafka_index_lz4 with YSB_KAFKA_ACCEPT_SNAPPY accepts codec 2
 * (without the flag it stays refused by name): frames[k].codec = 2 and one block entry per chunk,
 * or one for a raw block, offset at the preamble, comp_bytes the chunk's length |
 * YSB_SNAPPY_BLOCK.  Refused, naming the Kafka batch, its byte, the chunk's byte and the rule: a
 * compatible version other than 1, a chunk length <= 0 or past the records section, trailing
 * bytes shorter than a length word, a preamble of more than 5 bytes or >= 2^32, and a block of 0
 * or more than 65536 raw bytes -- larger raw blocks are chains of 64 KiB fragments whose
 * compressed boundaries nothing records; the way out is the Java client's framing or a producer
 * batch.size of at most 64 KiB.  At the context: ysb_kafka_set_codecs with YSB_KAFKA_CODECS_SNAPPY
 * in the mask (the default, YSB_KAFKA_CODECS_DEFAULT, is none and lz4; the only other mask taken
 * adds snappy; kept across ysb_reset) lets ysb_submit_kafka_lz4, _mapped and
 * ysb_kafka_unframe_lz4_device take such an index; without it YSB_ERR_ARG, as before.  The host
 * models (ysb_kafka_unframe_lz4_host, ysb_kafka_verdict_crc_lz4_host) have no context and take
 * what the index wrote.  Capacity: a slot batch's snappy blocks count their preambles' raw
 * sizes, every other block 65536, the sum at most max_batch_bytes; the plan kernel also makes
 * a block bad whose extent would pass the inflated buffer (mapped memory may change under the
 * host's read).  A block that breaks the format's rules is rule 8, as for LZ4. */
#define YSB_KAFKA_CODEC_SNAPPY 2u
#define YSB_KAFKA_ACCEPT_SNAPPY 0x100u     /* ysb_kafka_index_lz4's flags */
#define YSB_SNAPPY_BLOCK 0x40000000u       /* ysb_lz4_frame_block.comp_bytes bit 30 */
#define YSB_KAFKA_SNAPPY_XERIAL 0u
#define YSB_KAFKA_SNAPPY_RAW 1u
#define YSB_KAFKA_CODECS_DEFAULT 0x9u      /* codec 0 and codec 3 */
#define YSB_KAFKA_CODECS_SNAPPY 0x4u
int         ysb_kafka_set_codecs(ysb_ctx* ctx, uint32_t mask);
/* Test support: the plan kernel refuses (rule 8) a batch whose inflated extent would end past the
 * inflated buffer -- reachable otherwise only when registered memory changes under the host's
 * capacity check.  A non-zero `bytes` below the buffer's size takes its place in the kernel's test
 * for the compressed calls that follow; 0 (the default) and ysb_reset restore it.  Nothing else
 * changes. */
int         ysb_kafka_test_inflated_cap(ysb_ctx* ctx, uint64_t bytes);
/* The capacity rule per Kafka batch, for a caller that cuts an index into slot batches: bounds[k]
 * <- what batch k's blocks count -- a snappy block its preamble's raw size, every other block
 * 65536.  A run of batches fits a slot when their sum is at most max_batch_bytes.  Host only; the
 * entries are checked as ysb_kafka_unframe_lz4_host checks them (YSB_ERR_ARG). */
int         ysb_kafka_inflate_bounds(const uint8_t* bytes, uint64_t nbytes, const ysb_kafka_batch* batches,
                                     const ysb_kafka_frame* frames, uint64_t n_batches,
                                     const ysb_lz4_frame_block* blocks, uint64_t n_blocks, uint64_t* bounds);
/* One snappy block by the host compressor and the host decoder (csrc/ysb_snappy.h; test inputs
 * and the model of the kernel, no context).  compress: raw_bytes in 1..65536 into dst, cap at
 * least 32 + raw_bytes + raw_bytes / 6; *comp_bytes the block's size, preamble included.
 * decompress: src[0, comp_bytes) into dst (cap at least the preamble's size, 65536 always
 * suffices); *raw_bytes the decoded size; YSB_ERR_FORMAT for a block that breaks the format's
 * rules or says 0 or more than 65536 raw bytes. */
int         ysb_snappy_compress_block(const uint8_t* src, uint32_t raw_bytes, uint8_t* dst, uint32_t cap, uint32_t* comp_bytes);
int         ysb_snappy_decompress_block(const uint8_t* src, uint32_t comp_bytes, uint8_t* dst, uint32_t cap, uint32_t* raw_bytes);
/* Device-resident batch (HBM pointers, e.g. from ysb_device_alloc). Asynchronous.  The batch
 * must be complete when submitted, or its producer ordered before the compute stream
 * (hipStreamWaitEvent(ysb_stream(ctx), ...), or produced on that stream).  Unless
 * YSB_F_LAYOUT_FIXED, 64 stratified lines of the launch (ABI 2: each segment's first line) are
 * copied into pinned memory by a small kernel on the compute stream (so after that producer)
 * to pick the scan's instantiation (46 of 64 must agree, else the per-tile dispatch or the flat
 * tier): the launch's own sample when the compute stream is idle at the submit (the host waits
 * for that copy, microseconds); else the previous launch's sample if the one before it decided
 * the same (the host waits for that copy, which is queued behind the launch before the
 * previous one -- never for the launch just queued), and the per-tile dispatch when the two
 * disagree (producers alternating by batch: every producer's tiles still take its own path) or
 * no earlier sample exists.  A producer that changes its layout on a busy stream therefore
 * runs one launch through the old instantiation, then the dispatch until two samples agree;
 * counts never depend on the choice (ysb_launch_info tells which ran). */
int         ysb_submit_device(ysb_ctx* ctx, const uint8_t* d_bytes, uint64_t nbytes,
                              const uint32_t* d_line_off, uint64_t n_events);
/* Several device-resident batches in ONE kernel launch.  Each segment is a batch as
 * for ysb_submit_device (its own u32 line offsets, so each stays under 4 GiB); every
 * scan workgroup walks its run of tiles in segment 0, then segment 1, ..., so a step
 * over many batches pays one launch tail instead of one per batch.  Results are the
 * same as n_segs ysb_submit_device calls in order.  At most 16 segments and 2^31-1
 * events per call.  Replaces the same flatMap chain as ysb_submit (:111-119), for a
 * replay file larger than 4 GiB (FileBasedDataSource.run, :144-165). */
typedef struct ysb_segment {
    const uint8_t*  d_bytes;       /* HBM, 16-byte aligned */
    uint64_t        nbytes;        /* < 4 GiB */
    const uint32_t* d_line_off;    /* HBM, n_events offsets into d_bytes */
    uint64_t        n_events;
} ysb_segment;
int         ysb_submit_device_segments(ysb_ctx* ctx, const ysb_segment* segs, uint32_t n_segs);
/* Wait for every submitted batch.  YSB_ERR_CAPACITY if joined views were lost because
 * the out-of-ring map and its fallback list (overflow_capacity) both filled (stats.
 * overflow_dropped > 0): counts are then not exact, and every ysb_sync / ysb_drain reports
 * it until ysb_reset.  The map is emptied into the exact host-side list once it is a
 * quarter full: here, and at every submit from its fill level after the launch before
 * the previous one (read without waiting).  So a chain of submits without ysb_sync loses
 * counts only if ONE or two launches fill the map from below a quarter to full
 * (overflow_capacity distinct out-of-ring cells).  With YSB_F_STRICT, YSB_ERR_DATA once a
 * record the reference would have thrown on (or a foreign-shard view) was seen. */
int         ysb_sync(ysb_ctx* ctx);

/* ---- results ------------------------------------------------------------------------
 * Replaces CampaignProcessorCommon.flushWindows/writeWindow
 * (CampaignProcessorCommon.java:41-54, 69-98): returns the nonzero
 * (campaign, window) deltas with bucket in [bucket_lo, bucket_hi) (ring + side
 * list), sorted by (campaign, window).  clear != 0 zeroes what was returned (a
 * flush: the next drain reports only new deltas).  out == NULL: *n_out = rows
 * needed.  After ysb_group_reduce_scatter the ring part covers only this rank's
 * campaign block (every rank still reports its own side-list deltas; deltas are
 * additive, exactly like the HINCRBY they feed). */
int         ysb_drain(ysb_ctx* ctx, int64_t bucket_lo, int64_t bucket_hi, int clear,
                      ysb_count* out, uint64_t cap, uint64_t* n_out);
/* Asynchronous flush for streaming callers: CampaignProcessorCommon's flusher thread
 * (CampaignProcessorCommon.java:35-55, 91-98) writes every second while records keep flowing.
 * ysb_flush_begin enqueues, behind every batch submitted so far (a pending raw batch is launched
 * first), the compaction of the ring's nonzero (campaign, bucket) cells of [bucket_lo,
 * bucket_hi) straight into pinned host rows, clearing them on the device, and returns without
 * waiting: the stream keeps running.  Up to 4 flushes may be outstanding.  ysb_flush_end
 * returns the oldest one's rows sorted by (campaign, window): with wait = 0 it returns
 * YSB_PENDING if the device has not reached it yet; out = NULL: *n_out = rows needed (the rows
 * stay until they are taken).  A flush holds at most min(n_campaigns * window_ring, 2^20) rows:
 * cells beyond that keep their counts for the next flush (*more = 1).  Counts outside the ring
 * (the out-of-ring map and the side list) are not part of an asynchronous flush -- ysb_drain
 * reports them; deltas are additive, so a caller that sums flushes and drains has every count
 * exactly once.  Not after ysb_group_init (YSB_ERR_STATE). */
int         ysb_flush_begin(ysb_ctx* ctx, int64_t bucket_lo, int64_t bucket_hi);
int         ysb_flush_end(ysb_ctx* ctx, int wait, ysb_count* out, uint64_t cap, uint64_t* n_out, int* more);
int         ysb_stats_get(ysb_ctx* ctx, ysb_stats* out);
/* Zero counts, side list and stats; the ad table is kept. */
int         ysb_reset(ysb_ctx* ctx);
/* Bucket range currently held by the ring: [*lo, *lo + window_ring). */
int         ysb_ring_range(ysb_ctx* ctx, int64_t* lo, uint32_t* width);
/* Moves the ring to [new_lo, new_lo + window_ring) (streaming: follow the watermark).
 * Counts of buckets leaving the ring move to the exact host-side list and are reported
 * by later drains; events of buckets outside the new range keep going to the side list.
 * Replaces the LRU eviction of old buckets (LRUHashMap(10), CampaignProcessorCommon.java:37,
 * LRUHashMap.java:18-19) without its loss of counts.  After ysb_group_init this is a
 * collective: every rank calls it with the same new_lo (YSB_ERR_ARG on every rank if they
 * differ). */
int         ysb_ring_advance(ysb_ctx* ctx, int64_t new_lo);

/* ---- columnar decode -------------------------------------------------------------------
 * The fork's second use of the parsed events: WindowedArrowFormatBolter
 * (AdvertisingTopologyNative.java:278-356, wired commented at :106-109) turns a count window
 * of tuples into a fixed-stride, page-aligned columnar batch in a shared mapping, its hand-off
 * format for an accelerator.  These calls give DeserializeBolt's Tuple7 (:263-272) /
 * split("\\|")'s items (:197-226) in that layout, in HBM, for other GPU operators.  Additive:
 * nothing of the counting path is touched (the ABI version stays 5). */

/* The layout of a batch of batch_rows rows (host function, no context): seven columns
 * user_id, page_id, ad_id, ad_type, event_type, event_time, stamp of width[] =
 * {36,36,36,4,4,8,8} bytes per row (:284).  As the reference's constructor does (:291-302),
 * column j starts at the running offset start[j], which then grows by width[j] * batch_rows
 * rounded up to 4096-byte pages; the offset after column 6 is the reference's buffer_size =
 * image_bytes, so the first image_bytes bytes are the reference's file image.  One more buffer
 * follows at start[7] = image_bytes, an Arrow-style validity bitmap: row i is bit i % 64 of the
 * little-endian 64-bit word i / 64, ceil(batch_rows / 64) words rounded up to a page;
 * start[8] is the whole size.  YSB_ERR_ARG for batch_rows 0 or above 2^31 - 1. */
typedef struct ysb_columns_layout {
    uint64_t rows;          /* batch_rows the layout was computed for                */
    uint64_t start[9];      /* byte offset of column j; [7] validity, [8] = total    */
    uint32_t width[7];      /* 36,36,36,4,4,8,8 (AdvertisingTopologyNative.java:284) */
    uint32_t reserved;
    uint64_t image_bytes;   /* the reference's buffer_size = start[7]                */
} ysb_columns_layout;
int         ysb_columns_layout_of(uint64_t batch_rows, ysb_columns_layout* out);

#define YSB_COL_JAVA_ORDER 0x1u  /* columns 5 and 6 big-endian, as MappedByteBuffer.putLong writes them */
typedef struct ysb_decode_info {
    uint64_t rows;          /* n_events                                              */
    uint64_t valid;         /* rows the reference would not have thrown on           */
    uint64_t fast_rows;     /* rows the kernel's fast tier took                      */
    double   kernel_ms;     /* device time of the decode kernel (a HIP event pair)   */
} ysb_decode_info;
/* Replaces WindowedArrowFormatBolter.flatMap's per-tuple puts (:323-334) for one device batch
 * (as for ysb_submit_device: d_bytes 16-byte aligned, < 4 GiB, n_events u32 line offsets).
 * d_out is a 16-byte aligned HBM buffer of ysb_columns_layout_of(batch_rows).start[8] bytes;
 * n_events > batch_rows is YSB_ERR_CAPACITY.  Row i is line i.  The input format is the
 * context's: JSON lines with org.json's semantics, or .tbl rows under YSB_F_FORMAT_TBL;
 * YSB_F_REQUIRE_IP also requires a string ip_address (which gets no column).
 *   A row is valid iff the reference would not throw on it: the line parses (new JSONObject +
 * getString of the six keys, :263-272; .tbl: at least 6 items, :197-226), each of the five
 * String values has at least its column's width in UTF-8 bytes (put(bytes, 0, entry_len[j])
 * throws on a shorter array, :325-331), and Long.parseLong(event_time) succeeds.  A valid row
 * holds the first width[j] bytes of each String value (longer ones are cut, as the reference
 * cuts them: "banner" -> "bann"; a multi-byte character may be cut), the parsed long in column
 * 5 and `stamp` in column 6 (the reference writes 10L, :333) -- little-endian, or with
 * YSB_COL_JAVA_ORDER the file image's big-endian.  An invalid row holds zero bytes in every
 * column and a zero validity bit.
 *   Only rows [0, n_events) of each column and validity words [0, ceil(n_events / 64)) are
 * written (the bits of rows >= n_events in the last word zero); page padding and rows
 * [n_events, batch_rows) keep whatever d_out held.
 *   Runs on the compute stream behind everything submitted, then waits.  It reads no join
 * table (no ad map needs to be loaded) and changes neither the ring, the side list, the stats
 * nor the layout sampling's state.  info may be NULL. */
int         ysb_decode_columns_device(ysb_ctx* ctx, const uint8_t* d_bytes, uint64_t nbytes,
                                      const uint32_t* d_line_off, uint64_t n_events,
                                      uint8_t* d_out, uint64_t batch_rows, int64_t stamp,
                                      uint32_t flags, ysb_decode_info* info);

/* ---- columnar count ---------------------------------------------------------------------
 * The consumer half of the hand-off format: the filter -> join -> window-count chain
 * (EventFilterBolt, RedisJoinBolt, CampaignProcessor, AdvertisingTopologyNative.java:115-119)
 * on a column batch instead of on text -- what the accelerator behind
 * WindowedArrowFormatBolter (:278-356) does with a window of tuples.  Additive (the ABI
 * version stays 6); works in a context of either input format: columns have none.
 *
 * A batch is a buffer in the layout ysb_columns_layout_of(batch_rows); rows [0, n_rows)
 * count, n_rows <= batch_rows.  Without YSB_COL_VALIDITY the buffer is the reference's file
 * image (image_bytes) and every row is taken; with it the buffer extends to start[8] and a
 * row whose validity bit is zero is the row the reference would have thrown on: it adds 1 to
 * parse_errors and nothing else (YSB_ERR_DATA at ysb_sync under YSB_F_STRICT).  Per row, in
 * order: events += 1; the row is a view iff the four bytes of column 4 equal "view"
 * (event_type.equals("view"), :434, on the value as the layout cut it: the layout keeps four
 * bytes of event_type, so a value such as "viewer" is a view here and not on the JSON path
 * -- a property of the fork's layout); the key is the 36 bytes of column 2, joined as
 * ad_campaign.get(ad_id) (:464) through the 36-byte-key table and, where that table is
 * partial, the general one (a miss: join_misses, or foreign_shard for a key of another shard
 * of a sharded table); event_time is column 5 as an int64, little-endian or with
 * YSB_COL_JAVA_ORDER big-endian; bucket = event_time / time_divisor_ms in Java long division
 * for any divisor and negative times (CampaignProcessorCommon.java:58), counted as the scan
 * counts a joined view (LDS window counters, ring atomics, out-of-ring map).  time_errors and
 * deferred never change.  Each submit adds 1 to batches; n_rows = 0 is a batch that counts
 * nothing.  An unknown ring base is taken from the batch's first 256 rows by ring_base_bucket's
 * rule.  The calls read only rows < n_rows of columns 2, 4 and 5 and, with YSB_COL_VALIDITY,
 * validity words < ceil(n_rows / 64): never page padding, rows >= n_rows or the other four
 * columns.  They leave the layout sampling's state alone and never run in record mode (they
 * count into the u64 ring).  With YSB_F_TIMING they are part of ysb_kernel_time and
 * ysb_path_time; ysb_launch_info keeps describing scan launches only. */
#define YSB_COL_VALIDITY 0x2u    /* the buffer carries the validity bitmap at start[7] */

/* The byte ranges of a batch that a columnar count reads (host function, no context): n = 3,
 * or 4 with YSB_COL_VALIDITY, ranges [offset[i], offset[i] + bytes[i]) in ascending order --
 * rows [0, n_rows) of columns 2, 4 and 5, then the validity words.  What a JNI caller must
 * make visible to the device (of the MappedByteBuffer the bolter fills, :309-311), and what
 * ysb_submit_columns copies.  n_rows = 0: every range is empty.  YSB_ERR_ARG for unknown
 * flags or batch_rows outside [1, 2^31 - 1], YSB_ERR_CAPACITY for n_rows > batch_rows. */
int         ysb_columns_read_ranges(uint64_t batch_rows, uint64_t n_rows, uint32_t flags,
                                    uint64_t offset[4], uint64_t bytes[4], uint32_t* n);
/* Replaces the chain's flatMap calls (:115-119) for one device-resident column batch (HBM, 16-
 * byte aligned; e.g. ysb_decode_columns_device's output, with YSB_COL_VALIDITY).  Asynchronous
 * on the compute stream, behind everything submitted, like ysb_submit_device.  YSB_ERR_STATE
 * without an ad map; YSB_ERR_ARG for unknown flags, a NULL or misaligned buffer or batch_rows
 * outside [1, 2^31 - 1]; YSB_ERR_CAPACITY for n_rows > batch_rows. */
int         ysb_submit_columns_device(ysb_ctx* ctx, const uint8_t* d_cols, uint64_t batch_rows,
                                      uint64_t n_rows, uint32_t flags);
/* The host form, double-buffered like ysb_submit: `image` is the slot's own pinned buffer
 * (ysb_slot_buffers) or any host memory, e.g. the bolter's mapped file <shared_file>_<k>
 * (:303-311) read with YSB_COL_JAVA_ORDER.  Only ysb_columns_read_ranges' bytes are copied
 * (whole 16-byte vectors): into the slot's pinned buffer if the image is elsewhere, then to
 * the slot's device buffer at the same offsets by the context's H2D path (the copy kernel, or
 * the DMA engine under YSB_F_H2D_SDMA); the count launches behind the copy on the compute
 * stream.  ysb_wait(ctx, slot) before the slot's buffer is rewritten.  YSB_ERR_CAPACITY if the
 * buffer (image_bytes, or start[8] with YSB_COL_VALIDITY) exceeds max_batch_bytes; the other
 * errors as ysb_submit_columns_device. */
int         ysb_submit_columns(ysb_ctx* ctx, int slot, const uint8_t* image, uint64_t batch_rows,
                               uint64_t n_rows, uint32_t flags);
/* The last columnar launch (n_rows > 0): its rows, whether it counted through the LDS window
 * counters, whether it probed the HBM-resident bucket table, and its two flags -- each 0 or 1
 * but rows.  YSB_ERR_STATE before the first one. */
typedef struct ysb_colcount_desc {
    uint64_t rows;
    uint32_t lds_counters;
    uint32_t hbm_table;
    uint32_t java_order;
    uint32_t validity;
} ysb_colcount_desc;
int         ysb_columns_launch_info(ysb_ctx* ctx, ysb_colcount_desc* out);
/* sizeof(ysb_colcount_desc) as this library writes it. */
uint64_t    ysb_colcount_desc_size(void);

/* ---- joined views ------------------------------------------------------------------------
 * The third boundary inside the chain DeserializeBolt -> EventFilterBolt -> project ->
 * RedisJoinBolt -> keyBy -> CampaignProcessor (AdvertisingTopologyNative.java:111-119): after
 * the join.  RedisJoinBolt.flatMap (:460-474) emits a Tuple3(campaign_id, ad_id, event_time) for
 * every view whose ad is in the map; ysb_join_device gives that stream for one device batch, in
 * HBM and in stream order, as columns -- what a caller's own keyed operator consumes (another
 * window size, a session window, a per-ad count, a sink of joined tuples).  Additive: nothing of
 * the counting path is touched and the ABI version stays 6.
 *
 * Row i of the batch yields an output row iff the reference would not throw on it before the
 * join (the counting path's rule: the line parses and getString of the required keys succeeds,
 * YSB_F_REQUIRE_IP honoured; .tbl rows: the row split's rule), its event_type is exactly "view"
 * after unescaping, and its decoded ad_id is in the context's device tables as they are at the
 * call -- earlier ysb_ad_map_upsert calls apply; every table layout is covered (cache-resident
 * cuckoo slots, the HBM bucket table, the general table for ids that are not 36 bytes, sharded
 * loads).  Output rows are in ascending source row; nothing else is emitted.  A joined view
 * whose event_time Long.parseLong rejects is still emitted, as the reference parses the time only
 * after the join (CampaignProcessorCommon.java:58): time_ok = 0, event_time = 0, one time_error.
 *
 * The columns of a buffer for cap_rows rows (host function, no context), each starting on a
 * 4096-byte page like the columnar decode's: 0 campaign (u32, the campaign index), 1 row (u32,
 * the line's index in the batch), 2 event_time (int64, little-endian), 3 time_ok (u8) and, with
 * YSB_JOIN_KEYS, 4 key (56-byte stride: the decoded ad_id in the join tables' own key form,
 * zero-padded, as ysb_parked_keys returns it) and 5 key_len (u8).  start[j] is column j's byte
 * offset, start[6] the whole size; a column the flags leave out has width 0 and starts where
 * the next one does.  cap_rows = 0 is legal (an empty buffer).  YSB_ERR_ARG for unknown flags
 * or cap_rows above 2^32 - 1. */
#define YSB_JOIN_KEYS 0x1u       /* also the key and key_len columns */
typedef struct ysb_joined_layout {
    uint64_t cap_rows;
    uint64_t start[7];
    uint32_t width[6];      /* 4,4,8,1,56,1 (0 for a column the flags leave out)     */
    uint32_t flags;
    uint32_t n_cols;        /* 4, or 6 with YSB_JOIN_KEYS                            */
} ysb_joined_layout;
int         ysb_joined_layout_of(uint64_t cap_rows, uint32_t flags, ysb_joined_layout* out);

/* By definition events .. foreign_shard equal the change in ysb_stats that ysb_submit_device of
 * the same batch would have made (on a context that does not park). */
typedef struct ysb_join_info {
    uint64_t events, views, joined, join_misses, parse_errors, time_errors, foreign_shard;
    uint64_t rows_written;  /* min(joined, cap_rows)                                 */
    uint64_t fast_rows;     /* lines the kernel's fast tier took                     */
    uint64_t tiles;         /* 64-line tiles of the batch                            */
    uint32_t grid;          /* workgroups of the join kernel in this call ...        */
    uint32_t max_grid;      /* ... and the most it launches on this device: each
                               workgroup takes tiles grid apart                      */
    double   join_ms, prefix_ms, pack_ms;   /* the three kernels (HIP event pairs)   */
} ysb_join_info;
/* One device batch (as for ysb_submit_device: d_bytes 16-byte aligned, < 4 GiB, n_events u32
 * line offsets; the context's YSB_F_FORMAT_TBL decides the format) through filter and join into
 * d_out, a 16-byte aligned HBM buffer of ysb_joined_layout_of(cap_rows, flags).start[6] bytes.
 * Only rows < joined of each column are written; the rest of d_out keeps what it held.  If
 * joined > cap_rows the first cap_rows rows are written, info is complete and the call returns
 * YSB_ERR_CAPACITY; cap_rows = n_events always suffices.  n_events = 0 is legal and writes
 * nothing.
 *   Runs on the compute stream behind everything submitted, then waits.  It leaves the ring, the
 * side list, ysb_stats, the parked log and the layout sampling's state alone, and it never
 * parks: a miss is a miss, or foreign_shard on a sharded context.
 *   Three kernels, none waiting for another's workgroups: the join writes each 64-line tile's
 * joined rows to a context-owned scratch area, a prefix over the tiles' counts places them, a
 * pack moves them into the columns.  The scratch area is allocated on first use, reused and
 * freed with the context: at most 16 bytes per line of the batch (rounded up to whole tiles)
 * without YSB_JOIN_KEYS, at most 80 with it.
 *   YSB_ERR_ARG for unknown flags, NULL buffers, a misaligned d_bytes or d_out; YSB_ERR_CAPACITY
 * for a batch above 4 GiB or n_events above max_batch_events; YSB_ERR_STATE without an ad map
 * and after ysb_group_init.  info may be NULL. */
int         ysb_join_device(ysb_ctx* ctx, const uint8_t* d_bytes, uint64_t nbytes,
                            const uint32_t* d_line_off, uint64_t n_events,
                            uint8_t* d_out, uint64_t cap_rows, uint32_t flags,
                            ysb_join_info* info);
/* sizeof(ysb_join_info) as this library writes it. */
size_t      ysb_join_info_size(void);

/* ---- Arrow record batches -----------------------------------------------------------------
 * The same chain on an Apache Arrow record batch: three columns named ad_id, event_type and
 * event_time among a struct's children, as the Arrow C data interface hands them over
 * (pyarrow's _export_to_c / __arrow_c_array__, Arrow Java's Data.exportVectorSchemaRoot).
 * Additive (the ABI version stays 6).  The two structs below are the specification's own,
 * under its own guard: a caller that includes Arrow's header first compiles.
 *
 * Accepted formats: ad_id `u` / `z`; event_type `u` / `z`, or dictionary-encoded with `i`
 * (int32) indices and a `u` / `z` dictionary; event_time `u` / `z` (a decimal string, as the
 * JSON carries it), `l` or `tsm:*` (int64).  Everything else is YSB_ERR_FORMAT, the message
 * naming the field, its format and the way out.  Every array may be a slice (a nonzero
 * offset): row i of the batch is element batch.offset + child.offset + i of the child.  A
 * validity bitmap may be absent (all valid); bit k is bit k % 8 of byte k / 8, at the element
 * index.  The row rule -- stated once in csrc/ysb_arrow.h, which also holds its host model --
 * per row, in order: events += 1; a row with a zero validity bit at struct level or in any of
 * the three columns, a dictionary index outside [0, dict_len), a null dictionary value, or
 * offsets that break data_first <= off[k] <= off[k+1] <= data_bytes adds 1 to parse_errors and
 * nothing else (YSB_ERR_DATA at ysb_sync under YSB_F_STRICT); the row is a view iff its
 * event_type value is exactly the four bytes `view`; the key is the ad_id value's bytes (above
 * 56 bytes: a join miss; 36 bytes: the cuckoo table, then the general table where that is
 * partial; other lengths: the general table; a miss is join_misses, foreign_shard on a sharded
 * context, or with parking the view is parked); joined += 1; an int64 time is taken as it is, a
 * string time is Long.parseLong's ([+-]?[0-9]+ within int64, at any length), a rejected one
 * adds 1 to time_errors and counts nothing; bucket = time / time_divisor_ms in Java long
 * division, counted as the columnar count counts a joined view.  deferred never changes; each
 * submit adds 1 to batches; n_rows = 0 counts nothing.  The calls never run in record mode,
 * leave the layout sampling's state alone, and are part of ysb_kernel_time / ysb_path_time
 * under YSB_F_TIMING.  No byte outside the stated buffers is read, except that an access is
 * made in whole aligned 32-bit words: the up to three bytes that share a word with a buffer's
 * first or last byte may be loaded (never used). */
#ifndef ARROW_C_DATA_INTERFACE
#define ARROW_C_DATA_INTERFACE
#define ARROW_FLAG_DICTIONARY_ORDERED 1
#define ARROW_FLAG_NULLABLE 2
#define ARROW_FLAG_MAP_KEYS_SORTED 4
struct ArrowSchema {
    const char* format;
    const char* name;
    const char* metadata;
    int64_t flags;
    int64_t n_children;
    struct ArrowSchema** children;
    struct ArrowSchema* dictionary;
    void (*release)(struct ArrowSchema*);
    void* private_data;
};
struct ArrowArray {
    int64_t length;
    int64_t null_count;
    int64_t offset;
    int64_t n_buffers;
    int64_t n_children;
    const void** buffers;
    struct ArrowArray** children;
    struct ArrowArray* dictionary;
    void (*release)(struct ArrowArray*);
    void* private_data;
};
#endif

#define YSB_ARROW_STRING 1u   /* `u` / `z`: int32 offsets and bytes             */
#define YSB_ARROW_INT64  2u   /* `l` / `tsm:*`: int64 values (event_time)       */
#define YSB_ARROW_DICT   3u   /* int32 indices into a string dictionary (event_type) */

/* Where the three columns are in a struct schema, and how each is stored. */
typedef struct ysb_arrow_binding {
    int64_t  n_children;     /* of the schema bound                              */
    int64_t  child[3];       /* ad_id, event_type, event_time                    */
    uint32_t kind[3];        /* YSB_ARROW_*                                      */
    uint32_t reserved;
} ysb_arrow_binding;
/* Host, no context (messages: ysb_last_error(NULL), the thread's).  Finds the three fields by
 * name among the children of a struct schema (`+s`), checks their formats, records the child
 * indices and kinds.  Never calls release.  YSB_ERR_FORMAT as above, YSB_ERR_ARG for NULL. */
int         ysb_arrow_bind(const struct ArrowSchema* schema, ysb_arrow_binding* out);
uint64_t    ysb_arrow_binding_size(void);

/* One column as the count reads it.  Strings: int32 `offsets` (element k's bytes are
 * [off[k], off[k+1])) and `data`, which holds the bytes from offset data_first on (so byte x is
 * data[x - data_first]; 0 for a whole buffer) up to data_bytes, the buffer's stated end:
 * offsets outside [data_first, data_bytes] make their row invalid and are never followed.
 * YSB_ARROW_INT64 / _DICT: `data` holds the int64 values / int32 indices, data_bytes their
 * stated size (at least (offset + n_rows) elements).  validity: the bitmap or NULL.  offset:
 * the element of row 0 in offsets / values, validity_offset: its bit in the bitmap (for an
 * Arrow child both are batch.offset + child.offset; the host form's packed copy keeps only
 * the rows' elements and the bitmap bytes that cover them, so there they differ). */
typedef struct ysb_arrow_col {
    uint32_t kind;           /* YSB_ARROW_*                                      */
    uint32_t data_first;
    const uint8_t* validity;
    const uint8_t* offsets;
    const uint8_t* data;
    uint64_t data_bytes;
    uint64_t offset;
    uint64_t validity_offset;
} ysb_arrow_col;
typedef struct ysb_arrow_cols {
    uint64_t n_rows;
    const uint8_t* validity; /* struct level, or NULL                            */
    uint64_t offset;         /* ... its element of row 0 (batch.offset)          */
    ysb_arrow_col col[3];    /* ad_id, event_type, event_time                    */
    ysb_arrow_col dict;      /* event_type's dictionary (kind[1] == YSB_ARROW_DICT): a string
                                column whose element `offset + index` is the value */
    uint64_t dict_len;
} ysb_arrow_cols;
uint64_t    ysb_arrow_cols_size(void);

/* The host form, double-buffered like ysb_submit_columns.  Only what the rows need is copied
 * into the slot's pinned buffer, each range at a 16-byte boundary: offsets [o, o + n] of each
 * string column, the data bytes between the first and last of those offsets, the bitmap bytes
 * that cover the rows, the int64 times or the indices of the rows, the dictionary's offsets and
 * bytes (the plan: csrc/ysb_arrow.h arrow_plan).  The Arrow C data interface states no data
 * size, so a string column's bounds are its first and last offset.  The bytes go to the device
 * by the context's H2D path and the count launches behind the copy on the compute stream.
 * Never calls release; the caller keeps the batch alive until ysb_wait(ctx, slot).
 * YSB_ERR_CAPACITY if the planned bytes exceed max_batch_bytes; YSB_ERR_ARG for a NULL offsets
 * or data buffer on a non-empty column, n_children not matching the binding, a negative length
 * or offset, length > 2^31 - 1, a child shorter than the batch, a last offset below the first;
 * YSB_ERR_STATE without an ad map or while a frame carry is pending. */
int         ysb_submit_arrow(ysb_ctx* ctx, int slot, const ysb_arrow_binding* binding,
                             const struct ArrowArray* batch);
/* The device form: every pointer is device memory at any alignment.  Asynchronous on the
 * compute stream, behind everything submitted, like ysb_submit_columns_device.  YSB_ERR_ARG
 * for unknown kinds, a NULL buffer on a non-empty column, n_rows > 2^31 - 1, data_first >
 * data_bytes, string data above 2^31 bytes, fixed-width data shorter than its rows;
 * YSB_ERR_CAPACITY for a dictionary above 2^30 - 2 values; YSB_ERR_STATE as above. */
int         ysb_submit_arrow_device(ysb_ctx* ctx, const ysb_arrow_cols* cols);
/* The host form's copy plan (host, no context; csrc/ysb_arrow.h arrow_plan): the only bytes of
 * a batch that ysb_submit_arrow touches, as ranges {src, bytes, dst} -- dst the range's place in
 * the packed image, a multiple of 16 --, col 0..2 the column, 3 the dictionary, 4 the struct's
 * bitmap, what 0 a bitmap, 1 offsets, 2 data / values.  *n <- their number, *total <- the packed
 * image's bytes; YSB_ERR_CAPACITY if cap (in ranges) is short.  ysb_arrow_pack makes the packed
 * image in host memory (cap bytes; YSB_ERR_CAPACITY with too few) and *packed the batch as it
 * lies there; ysb_arrow_view is the whole batch in place (nothing copied; a string column's
 * data ends at its array's last offset).  Errors as ysb_submit_arrow's argument errors. */
typedef struct ysb_arrow_range {
    const uint8_t* src;
    uint64_t bytes;
    uint64_t dst;
    uint32_t col;
    uint32_t what;
} ysb_arrow_range;
int         ysb_arrow_plan(const ysb_arrow_binding* binding, const struct ArrowArray* batch,
                           ysb_arrow_range* ranges, uint64_t cap, uint64_t* n, uint64_t* total);
int         ysb_arrow_pack(const ysb_arrow_binding* binding, const struct ArrowArray* batch,
                           uint8_t* image, uint64_t cap, ysb_arrow_cols* packed);
int         ysb_arrow_view(const ysb_arrow_binding* binding, const struct ArrowArray* batch,
                           ysb_arrow_cols* out);
/* The host model of the row rule over host buffers (csrc/ysb_arrow.h arrow_count_rows): no
 * context, no GPU.  The map: n_keys keys, key i the bytes keys[key_off[i], key_off[i + 1]) with
 * campaign[i] (later entries win).  stats[8] <- events, views, joined, join_misses,
 * parse_errors, time_errors, foreign_shard, 0; invalid[3] <- invalid rows by cause (null,
 * offsets, dictionary index); cells <- up to cap triples {campaign, bucket, count}, *n_cells
 * their number (YSB_ERR_CAPACITY if cap is short). */
int         ysb_arrow_count_host(const ysb_arrow_cols* cols, const uint8_t* keys, const uint32_t* key_off,
                                 const uint32_t* campaign, uint64_t n_keys, int64_t divisor,
                                 uint32_t shard_rank, uint32_t shard_n, uint64_t stats[8],
                                 uint64_t invalid[3], int64_t* cells, uint64_t cap, uint64_t* n_cells);
/* The last Arrow launch (n_rows > 0); waits for it.  resident_grid: the largest grid a launch
 * takes (a batch of more than 64 * resident_grid rows makes workgroups take several tiles);
 * per_lane_tiles: tiles that did not go through the staged path. */
typedef struct ysb_arrow_desc {
    uint64_t rows, tiles;
    uint32_t grid, resident_grid;
    uint64_t per_lane_tiles;
    uint64_t invalid_null, invalid_offsets, invalid_dict;
    uint32_t kind[3];
    uint32_t lds_counters;
    uint32_t hbm_table;
    uint32_t reserved;
} ysb_arrow_desc;
int         ysb_arrow_launch_info(ysb_ctx* ctx, ysb_arrow_desc* out);
uint64_t    ysb_arrow_desc_size(void);

/* ---- measurement -------------------------------------------------------------------- */
/* With YSB_F_TIMING: total device time of the scan kernel launches (HIP events on
 * the compute stream) and the number of launches since the last call (resets). */
int         ysb_kernel_time(ysb_ctx* ctx, double* total_ms, uint64_t* launches);
/* With YSB_F_TIMING: device time of the host-to-device copies of ysb_submit / ysb_submit_raw
 * (HIP events on the copy stream), their number and bytes since the last call (resets). */
int         ysb_copy_time(ysb_ctx* ctx, double* total_ms, uint64_t* copies, uint64_t* bytes);
/* The same launches' whole device sequence -- scan, general-path and (record mode)
 * partition + count kernels -- as measured by the last ysb_kernel_time call (which
 * collects both), and the launches so far that used record mode. */
int         ysb_path_time(ysb_ctx* ctx, double* total_ms, uint64_t* launches, uint64_t* record_launches);
/* The scan instantiation the last launch ran: the JSON layout tried first (0 the
 * generator's, 1 compact JSON, 2 the flat-object tier, 3 a learned key order, 4 the per-tile
 * dispatch for several producers in one batch; what layout sampling or a hint chose), record-mode counting, the HBM-resident join table (bucket layout, serial
 * probes), the .tbl format -- each 0 or 1. */
typedef struct ysb_launch_desc {
    uint32_t layout;
    uint32_t record_mode;
    uint32_t hbm_table;
    uint32_t tbl;
} ysb_launch_desc;
int         ysb_launch_info(ysb_ctx* ctx, ysb_launch_desc* out);
/* A read-only view of the last record-mode launch (ABI 6; the tests' evidence of which device
 * paths ran): its plan -- level-2 blocks of 1 << blk_shift campaigns, level-1 bins of
 * 1 << sub_log2 blocks, `cap` records per (scan workgroup, bin) sub-buffer, `area` u32 words per
 * (bin, slice) partition output, `part` words in all -- the launch's scan workgroups (grid) and
 * partition slices per bin (slices), whether anything was added to the u64 ring past the u8
 * delta ring (dirty: a delta cell passed 255, a full sub-buffer's views or a general-path view
 * went to the atomics; sticky until ysb_reset or an exchange) and the events counted into the
 * delta ring since it was last folded (delta_bound).  rec_n (may be NULL) receives the records
 * stored per sub-buffer as [grid][bins], runs (may be NULL) each block's run per slice as
 * [n_blocks][slices][2] = {offset, length} in words of the partition output; a capacity
 * (in elements) too small for either fails with YSB_ERR_CAPACITY, the descriptor filled in.
 * Waits for every queued launch; changes nothing (no fold).  YSB_ERR_STATE before the first
 * record-mode launch. */
typedef struct ysb_record_desc {
    uint32_t w_log2;
    uint32_t blk_shift;
    uint32_t n_blocks;
    uint32_t sub_log2;
    uint32_t bins;
    uint32_t cap;
    uint32_t grid;
    uint32_t slices;
    uint64_t area;
    uint64_t part;
    uint64_t delta_bound;
    uint32_t dirty;
    uint32_t reserved;
} ysb_record_desc;
int         ysb_record_info(ysb_ctx* ctx, ysb_record_desc* out, uint32_t* rec_n, uint64_t rec_n_cap,
                            uint32_t* runs, uint64_t runs_cap);
/* sizeof(ysb_record_desc) as this library writes it (ABI 6). */
uint64_t    ysb_record_desc_size(void);
/* The layout sampling's decision for one line (host function; what every submit applies
 * to its batch's first line): 0 the generator's layout (core.clj:90-96), 1 its keys in its
 * order as compact JSON, 3 another order or subset of DeserializeBolt's keys with one
 * consistent spacing -- order[0..*n) then receives the key indices (0 user_id, 1 page_id,
 * 2 ad_id, 3 ad_type, 4 event_type, 5 event_time, 6 ip_address) and *compact the spacing
 * -- or 2 anything else (the flat-object tier first).  require_ip: YSB_F_REQUIRE_IP's
 * rule (ip_address must be among the keys). */
int         ysb_layout_of_line(const uint8_t* line, uint64_t len, int require_ip, uint32_t order[8],
                               uint32_t* n, uint32_t* compact);
/* The compute stream (hipStream_t) for callers that want to order work with it (a pending
 * raw batch is launched first); NULL if that launch failed (ysb_last_error). */
void*       ysb_stream(ysb_ctx* ctx);

/* ---- device memory helpers (so host code needs no framework for HBM buffers) ----------- */
int         ysb_device_alloc(ysb_ctx* ctx, uint64_t bytes, void** d_ptr);
int         ysb_device_free(ysb_ctx* ctx, void* d_ptr);
int         ysb_memcpy_h2d(ysb_ctx* ctx, void* d_dst, const void* h_src, uint64_t bytes);
int         ysb_memcpy_d2h(ysb_ctx* ctx, void* h_dst, const void* d_src, uint64_t bytes);

/* ---- multi-GPU: replaces the keyBy(0) shuffle (AdvertisingTopologyNative.java:118) ----
 * Events are sharded by ad_id hash across ranks; the per-rank (campaign, window)
 * tables are summed with one RCCL reduce-scatter over xGMI, leaving rank r the
 * owner of campaigns [r*Cp/N, (r+1)*Cp/N), Cp = n_campaigns padded to N. */
#define YSB_UNIQUE_ID_BYTES 128
int         ysb_group_unique_id(uint8_t uid[YSB_UNIQUE_ID_BYTES]);
/* Collective.  Also agrees on the ring base (every rank's ring must start at the same
 * bucket: the tables are summed cell by cell): the smallest base any rank holds wins; a
 * rank whose ring starts later moves the buckets the common range does not hold to its
 * exact side list.  If no rank has a base yet, the first ysb_group_reduce_scatter agrees.
 * After ysb_group_init, ysb_ring_advance is collective too (same new_lo on every rank). */
int         ysb_group_init(ysb_ctx* ctx, int rank, int nranks,
                           const uint8_t uid[YSB_UNIQUE_ID_BYTES]);
/* The same group over the caller's own collectives instead of RCCL (a job whose ranks
 * already share a transport; the test rehearsal of N ranks on one GPU, where RCCL refuses
 * two ranks per device).  Both callbacks run on the calling thread, on host memory, and
 * must be collective over the nranks ranks; nonzero = failure:
 *   allreduce_max_u64: buf[0..n) <- elementwise max over the ranks, in place;
 *   reduce_scatter_sum: recv[0..count) <- sum over the ranks of their send blocks
 *     [rank * count, (rank + 1) * count), cells of `width` bytes (1, 4 or 8), unsigned. */
typedef struct ysb_collectives {
    int (*allreduce_max_u64)(void* user, uint64_t* buf, uint64_t n);
    int (*reduce_scatter_sum)(void* user, const void* send, void* recv, uint64_t count, uint32_t width);
    void* user;
} ysb_collectives;
int         ysb_group_init_host(ysb_ctx* ctx, int rank, int nranks, const ysb_collectives* ops);
/* Collective: sums the ranks' pending counts (everything counted since the previous call)
 * into the owner ranks' tables and zeroes them.  Range-limited, like the reference's keyed
 * shuffle, which carries only the touched (campaign, window) pairs: per ring bucket the
 * largest pending count on any rank is agreed by one W-element all-reduce(max) (the call's
 * only wait for the device), and only the buckets holding a count travel, as a dense
 * [C_pad][buckets] array of the narrowest cell width that cannot wrap in the sum (1 byte
 * while nranks * max <= 255, else 4, else 8) through one ncclReduceScatter.  The rest is
 * asynchronous on the compute stream.  Record mode's u8 delta ring is read directly (no
 * fold): configs[2]'s 1M campaigns x 100 live buckets move 100 MB per rank and exchange
 * instead of the whole 1 GB u64 ring. */
int         ysb_group_reduce_scatter(ysb_ctx* ctx);
/* Collective, the streaming form of ysb_group_reduce_scatter: no wait for the device.  This
 * call's per-bucket maxima are only enqueued (all-reduced and read back asynchronously);
 * the buckets and width that travel are the PREVIOUS call's plan, read back while the
 * step's scan ran.  Counts in buckets outside that plan, or larger than its width sums over
 * the ranks, stay pending for a later exchange (nothing is lost or double counted; the
 * owners' tables lag by at most one call).  The first call after ysb_group_init, ysb_reset
 * or ysb_ring_advance is a complete ysb_group_reduce_scatter; a complete call settles
 * everything (do one before reading the owned tables).  Every rank must use the same
 * sequence of the two calls. */
int         ysb_group_exchange_pipelined(ysb_ctx* ctx);
/* Exchange accounting: exchanges run, reduce-scatter input bytes this rank contributed
 * (campaign rows x the planned buckets, each run widened to aligned groups of 4 ring slots,
 * x the cell width), device
 * time of the exchanges (HIP events: plan, all-reduce(max), read-back, pack, reduce-scatter,
 * unpack), of their part on the compute stream (critical_ms: plan to pack, plus the unpack --
 * what the launches queue behind; the reduce-scatter runs on a stream of its own beside the
 * next launch, and the unpack is enqueued on the compute stream at the next exchange or read),
 * the last exchange's bucket count and cell width (0: nothing was pending), what one
 * whole-ring u64 exchange would move, the reduce-scatters' own time (rs_ms: pack done to
 * reduce-scatter done, on the exchange stream, waiting for the peers included) and the part of
 * it the compute stream stood waiting for at the unpack (exposed_ms; rs_ms - exposed_ms ran
 * hidden beside the launches queued since -- a complete exchange exposes all of it).  reset != 0
 * zeroes the totals after reading them.  (ABI 4 appended rs_ms and exposed_ms.) */
typedef struct ysb_exchange_info {
    uint64_t exchanges;
    uint64_t bytes;
    double   ms;
    uint32_t last_buckets;
    uint32_t last_width;
    uint64_t full_ring_bytes;
    double   critical_ms;
    double   rs_ms;
    double   exposed_ms;
} ysb_exchange_info;
int         ysb_group_exchange_info(ysb_ctx* ctx, ysb_exchange_info* out, int reset);
/* sizeof(ysb_exchange_info) as this library writes it (ABI 5): a caller built against an older
 * header (ABI 3: 48 bytes) must not pass its smaller struct to ysb_group_exchange_info. */
uint64_t    ysb_exchange_info_size(void);
/* The plan every rank derives from the all-reduced per-bucket maxima (host function):
 * slots[0..*n_slots) = the ring slots with slot_max > 0, ascending; *width = the cell width
 * above.  YSB_ERR_CAPACITY if nranks * max does not fit 64 bits. */
int         ysb_exchange_plan(const uint64_t* slot_max, uint32_t W, uint32_t nranks, uint32_t* slots,
                              uint32_t* n_slots, uint32_t* width);
/* Linear checksums for a multi-rank check that moves no tables (sum over cells of count x
 * an odd 64-bit weight of (campaign, bucket), mod 2^64, so checksums add like the tables):
 *   YSB_SUM_TRUTH_BLOCKS   out[r], r < nranks: the generator truth's cells of owner block r
 *   YSB_SUM_PENDING_BLOCKS out[r], r < nranks: this rank's pending (not yet exchanged) cells
 *   YSB_SUM_OWNED          out[0]: this rank's owned table (its block, after exchanges)
 * After ysb_group_reduce_scatter on every rank: OWNED of rank r + SUM over ranks of
 * PENDING[r] == SUM over ranks of TRUTH[r]. */
#define YSB_SUM_TRUTH_BLOCKS   0
#define YSB_SUM_PENDING_BLOCKS 1
#define YSB_SUM_OWNED          2
int         ysb_group_checksum(ysb_ctx* ctx, int what, uint32_t nranks, uint64_t* out);
int         ysb_group_owned(ysb_ctx* ctx, uint32_t* campaign_lo, uint32_t* campaign_hi);
/* The communicator as RCCL sees it (ncclCommUserRank / ncclCommCount): a check that the
 * exchange really spans the ranks the launcher started. */
int         ysb_group_info(ysb_ctx* ctx, int* rank, int* nranks);
/* Shard of an ad_id under the partitioning above (host function). */
uint32_t    ysb_ad_shard(const char* ad_id, uint32_t len, uint32_t nranks);
/* Campaign block [*lo, *hi) that rank `rank` of `nranks` owns after
 * ysb_group_reduce_scatter (host function, no context needed; ysb_group_owned of an
 * initialised context reports the same block).  Replaces the key -> subtask mapping of
 * Flink's keyBy(0) hash partitioner (AdvertisingTopologyNative.java:118-119). */
int         ysb_group_block(uint32_t n_campaigns, int rank, int nranks, uint32_t* lo, uint32_t* hi);
/* Host router for batches that are not pre-sharded: out_shard[i] = ysb_ad_shard of line
 * i's top-level "ad_id" string, its escapes decoded to UTF-8 as org.json and the device
 * decode them (an escaped key name is found too; generator lines: bytes 113..148; other
 * layouts: a key scan); lines without one go to shard 0.  shard_counts (nranks
 * entries, may be NULL) receives the lines per shard.  Routing must match the join table:
 * with a sharded table (ysb_load_ad_map_shard) only this hash is exact -- a view routed
 * elsewhere misses and is counted as foreign_shard (an error under YSB_F_STRICT); with the
 * whole map on every rank (ysb_load_ad_map) any deterministic routing is exact. */
int         ysb_route_lines(const uint8_t* bytes, uint64_t nbytes, const uint32_t* line_off,
                            uint64_t n, uint32_t nranks, uint32_t* out_shard,
                            uint64_t* shard_counts);

/* ---- synthetic input: the data/ generator's event format (core.clj:61-98, 163-181)
 * restated as a seeded, counter-based generator with a file-dump mode.  Host and
 * device produce byte-identical lines for the same parameters. */
typedef struct ysb_gen_params {
    uint64_t seed;
    uint32_t n_campaigns;       /* 100 (core.clj:15)                                  */
    uint32_t ads_per_campaign;  /* 10 ((partition 10 ads), core.clj:52)               */
    int64_t  t0_ms;             /* event_time of event 0                              */
    uint64_t events_per_sec;    /* event time advances 1000/rate ms per event;
                                   100 reproduces catch-up mode (10 ms, core.clj:95)   */
    uint32_t with_skew;         /* 1: +-50 ms skew, 1e-5 late by <60 s (core.clj:166-174);
                                   2: the skew only (out of order, never late)         */
    uint32_t n_users;           /* 0: a fresh user/page UUID per event (core.clj:79-80);
                                   k: draw from a pool of k (core.clj:187-188)         */
    const uint32_t* ad_subset;  /* optional: draw ads only from these indices (shards) */
    uint32_t n_ad_subset;
    uint32_t event_stream;      /* 0: the single-stream generator; k > 0: an independent
                                   event stream over the SAME campaign/ad ids (one per
                                   rank of a sharded run); ids depend on seed only     */
    uint32_t format;            /* YSB_GEN_JSON (core.clj:90-97 lines) or YSB_GEN_TBL (the
                                   fork's .tbl rows of the same events, :197-226)       */
    uint32_t variant;           /* 0: the generator's own lines; YSB_GEN_RANDOM_IP /
                                   YSB_GEN_MORE_AD_TYPES / YSB_GEN_COMPACT / YSB_GEN_REORDER:
                                   the same events as other producers would write them (a
                                   random dotted-quad ip_address, 8 ad_types, no space after
                                   ':' and ',', the keys in another fixed order) --
                                   lines the vocabulary fast path does not take; the views,
                                   ads and times (and so the truth) are unchanged except that
                                   YSB_GEN_MORE_AD_TYPES draws the ad_type from 8           */
} ysb_gen_params;
#define YSB_GEN_JSON 0u
#define YSB_GEN_TBL  1u
#define YSB_GEN_RANDOM_IP     1u
#define YSB_GEN_MORE_AD_TYPES 2u
#define YSB_GEN_COMPACT       4u
#define YSB_GEN_REORDER       8u
#define YSB_GEN_MIXED        16u  /* four producers interleaved line by line: each event's layout drawn
                                     from {the generator's, compact, reordered keys, random ip with 8
                                     ad_types}; the same events and truth */
#define YSB_GEN_MIXED_BLOCKS 32u  /* the same four producers in runs of 256 events (drawn per run) */

void        ysb_gen_default(ysb_gen_params* p);
/* Campaign and ad UUIDs, 36 bytes each, no separators (ad a -> campaign a / ads_per_campaign). */
int         ysb_gen_ids(const ysb_gen_params* p, char* campaign_ids, char* ad_ids);
/* Events [first, first+n) into out (cap bytes); line offsets relative to out. */
int         ysb_gen_events_host(const ysb_gen_params* p, uint64_t first, uint64_t n,
                                uint8_t* out, uint64_t cap, uint32_t* line_off,
                                uint64_t* nbytes);
/* The same with `threads` host threads (lengths, their prefix, then the lines in place): a
 * real-time producer fast enough to load the streaming path (configs[4] under load). */
int         ysb_gen_events_host_mt(const ysb_gen_params* p, uint64_t first, uint64_t n, uint8_t* out,
                                   uint64_t cap, uint32_t* line_off, uint64_t* nbytes, uint32_t threads);
/* Same on the device (d_out / d_line_off are HBM); synchronous. */
int         ysb_gen_events_device(ysb_ctx* ctx, const ysb_gen_params* p, uint64_t first,
                                  uint64_t n, uint8_t* d_out, uint64_t cap,
                                  uint32_t* d_line_off, uint64_t* nbytes);
/* Upper bound of one generated line in bytes. */
uint64_t    ysb_gen_max_line_bytes(const ysb_gen_params* p);
/* Generator truth, independent of any parsing: adds the (campaign, bucket) view
 * counts of events [first, first+n) to a second device table ("truth") laid out
 * like the ring; ysb_truth_compare counts ring/truth cells that differ. */
int         ysb_truth_accumulate(ysb_ctx* ctx, const ysb_gen_params* p, uint64_t first,
                                 uint64_t n);
int         ysb_truth_compare(ysb_ctx* ctx, uint64_t* mismatched_cells,
                              uint64_t* truth_total, uint64_t* ring_total);
/* The truth table itself: n_campaigns x window_ring u64, campaign-major, cell (c, b mod W)
 * holding bucket b of [*ring_lo, *ring_lo + W) (cells >= n_campaigns * window_ring).  Lets
 * a multi-rank check sum the ranks' truths and compare them with the owners' drains. */
int         ysb_truth_read(ysb_ctx* ctx, uint64_t* out, uint64_t cells, int64_t* ring_lo);
/* Writes the generator's files into dir: campaign-ids.txt, ad-ids.txt (core.clj:24-34),
 * ad-to-campaign-ids.txt ({ "AD": "CAMPAIGN"} lines, core.clj:58), ad-to-campaign.csv
 * (ad,campaign lines, AdvertisingTopologyNative.java:52) and kafka-json.txt with
 * n_events events (core.clj:76-97). */
int         ysb_gen_dump(const ysb_gen_params* p, uint64_t n_events, const char* dir);
/* The fork's events.tbl rows from generator-format JSON lines (the external tool that
 * wrote conf/benchmarkConf.yaml:6's events.tbl is not in the reference):
 * user_id|page_id|ad_id|ad_type|event_type|event_time\n per line, values copied raw.
 * YSB_ERR_FORMAT for a line that is not 7 unescaped "key": "value" pairs in the
 * generator's key order (core.clj:90-96); YSB_ERR_CAPACITY if out (cap bytes) is short. */
int         ysb_json_to_tbl(const uint8_t* bytes, uint64_t nbytes, const uint32_t* line_off,
                            uint64_t n, uint8_t* out, uint64_t cap, uint32_t* out_off,
                            uint64_t* out_nbytes);
/* Sharded file-dump mode (config 4's pre-sharded replay files): the id and map files
 * as ysb_gen_dump, and events [0, n_events) split by ysb_route_lines into
 * kafka-json.<r>.txt for r in [0, nranks). */
int         ysb_gen_dump_shards(const ysb_gen_params* p, uint64_t n_events, const char* dir,
                                uint32_t nranks);

#ifdef __cplusplus
}
#endif
#endif /* YSB_HIP_H */
