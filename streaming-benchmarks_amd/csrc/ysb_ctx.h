// ysb_ctx.h -- the library context behind the C ABI (include/ysb_hip.h), shared by the
// library's host translation units:
//   ysb_capi.cpp    context lifecycle, the ad -> campaign tables, sync / drain / ring / stats
//   ysb_submit.cpp  segments into launches: slots, device batches, the layout samples, the scan launch
//   ysb_raw.cpp     batches that cross PCIe into a slot and launch a call later (raw, mapped, LZ4, Kafka)
//   ysb_columns.cpp the columnar decode and the columnar count's submits
//   ysb_join_api.cpp the join's output as ordered columns (its layout, scratch format and plan:
//                   ysb_join.h, no HIP: tests/native/join_logic.cpp)
//   ysb_layout.h    the layout sampling's rules (no HIP: tests/native/layout_logic.cpp)
//   ysb_admap.h     the join tables as host data and the live map's rules (no HIP:
//                   tests/native/admap_logic.cpp, upsert_logic.cpp)
//   ysb_recplan.h   record mode's plan of a launch (no HIP: tests/native/recplan_logic.cpp)
//   ysb_parked_api.cpp  parked views: the log of the views of unknown ads, its keys, its resolve
//   ysb_parked.h    their record format, rules and host model (no HIP: tests/native/parked_logic.cpp)
//   ysb_lz4_api.cpp LZ4 batches: the directory's checks, the decode's staging, the host codec entries
//   ysb_lz4.h       their format, its one sequence reader and the host model (no HIP:
//                   tests/native/lz4_logic.cpp)
//   ysb_lz4_frame.h standard LZ4 frames: the index, XXH32, the writer, the measure model and the carry
//                   rule (no HIP: tests/native/lz4_frame_logic.cpp)
//   ysb_kafka_api.cpp Kafka record batches: the index's checks, a slot batch's staging, the three launches
//   ysb_kafka.h     their format, the one record reader, the host model and the packer (no HIP:
//                   tests/native/kafka_logic.cpp)
//   ysb_group.cpp   multi-GPU: the RCCL / host-collective group and the keyBy exchange
//   ysb_gen_api.cpp the synthetic generator (host and device) and its truth tables
// Internal: nothing here is part of the ABI (the shared helpers have hidden visibility).
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <array>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <optional>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/ysb_hip.h"
#include "ysb_admap.h"
#include "ysb_kernels.h"
#include "ysb_layout.h"

using namespace ysb;   // (an internal header of the library's own units)


namespace ysb {
int scan_lds_bytes();
}

constexpr size_t XEV_KEEP = 64;   // exchange timing pairs pending before they are folded into x_ms
// YSB_F_TIMING: launch / copy event records pending before the older half is folded into
// running totals (a streaming caller may never call ysb_kernel_time / ysb_copy_time)
constexpr size_t TIMING_KEEP = 256;

// One owner per GPU resource: move-only, released when the owner goes (the context's members
// in ysb_close, with its device current) or takes another, and converting to the raw handle
// that the kernels' parameter structs and the launch functions take.
template <class H, hipError_t (*Free)(H)>
struct Owned {
    H h = nullptr;
    Owned() = default;
    Owned(Owned&& o) noexcept : h(o.h) { o.h = nullptr; }
    Owned& operator=(Owned&& o) noexcept {
        if (this != &o) { reset(); h = o.h; o.h = nullptr; }
        return *this;
    }
    ~Owned() { reset(); }
    void reset() { if (h) Free(h); h = nullptr; }
};
struct DevMem : Owned<void*, hipFree> {   // device memory (alloc releases what it held first)
    u64 n = 0;
    hipError_t alloc(u64 bytes) { reset(); n = bytes; return hipMalloc(&h, bytes); }
    u64 bytes() const { return h ? n : 0; }
};
template <class T>
struct DevBuf : DevMem {
    T* get() const { return static_cast<T*>(h); }
    operator T*() const { return get(); }
};
template <class T>
struct PinBuf : Owned<void*, hipHostFree> {   // pinned host memory
    hipError_t alloc(u64 bytes) { reset(); return hipHostMalloc(&h, bytes); }
    T* get() const { return static_cast<T*>(h); }
    operator T*() const { return get(); }
};
struct Event : Owned<hipEvent_t, hipEventDestroy> {
    hipError_t create(unsigned flags = hipEventDisableTiming) { reset(); return hipEventCreateWithFlags(&h, flags); }
    hipEvent_t get() const { return h; }
    operator hipEvent_t() const { return h; }
};

// YSB_F_TIMING's event log: N events per entry (a launch, a slot copy), kept until a getter
// collects them.  total[k] sums elapsed(ev[0], ev[k]) over the entries taken in so far, k =
// 1..N-1.  A caller that never collects (a streaming job) would grow the log without bound:
// once TIMING_KEEP entries are pending, acquire folds the older half into the totals (those
// are TIMING_KEEP / 2 entries old -- normally long done; else this waits for them) and their
// events are reused.
template <int N>
struct EventLog {
    std::vector<std::array<Event, N>> ev;
    size_t used = 0;
    u64 folded = 0;
    double total[N] = {};

    // the oldest n entries into the totals (wait: for each entry's last event first)
    hipError_t fold(size_t n, bool wait) {
        for (size_t i = 0; i < n; ++i) {
            hipError_t e = wait ? hipEventSynchronize(ev[i][N - 1]) : hipSuccess;
            float ms[N] = {};
            for (int k = 1; k < N && e == hipSuccess; ++k) e = hipEventElapsedTime(&ms[k], ev[i][0], ev[i][k]);
            if (e != hipSuccess) return e;
            for (int k = 1; k < N; ++k) total[k] += ms[k];
            ++folded;
        }
        std::rotate(ev.begin(), ev.begin() + (ptrdiff_t)n, ev.begin() + (ptrdiff_t)used);
        used -= n;
        return hipSuccess;
    }
    // the next entry's events (created on demand)
    hipError_t acquire(Event** out) {
        hipError_t e = used == TIMING_KEEP ? fold(TIMING_KEEP / 2, true) : hipSuccess;
        if (e == hipSuccess && used == ev.size()) {
            std::array<Event, N> a;
            for (int k = 0; k < N && e == hipSuccess; ++k) e = a[k].create(hipEventDefault);
            if (e == hipSuccess) ev.push_back(std::move(a));
        }
        if (e == hipSuccess) *out = ev[used++].data();
        return e;
    }
    // every entry so far (all complete: the caller has synchronised): totals[1..N-1] and the
    // entry count; the log starts over
    hipError_t collect(double* totals, u64* n) {
        const hipError_t e = fold(used, false);
        if (e != hipSuccess) return e;
        for (int k = 1; k < N; ++k) { totals[k] = total[k]; total[k] = 0; }
        *n = folded;
        folded = 0;
        return hipSuccess;
    }
};

// The scan instantiation a submit chose for its batch: layout -1 is the flags'; learn the key
// order of layouts 3 and 4.
struct Layout {
    int layout = -1;
    LearnDesc learn{};
};

// A compressed batch as lz4_stage / lz4f_stage leaves it: its figures until its launch settles
// them into lz4_last / lz4f_last, and its largest block (the decode's LDS window).
struct Lz4Staged {
    ysb_lz4_desc info{};
    u32 max_raw = 0;
    u32 decoder = 0;                     // a frame batch: the decode kernel chosen when it was staged
    bool frame = false;                  // a frame batch (ysb_submit_lz4_blocks): sizes measured on the device
    bool more = false;                   // ... with YSB_LZ4F_MORE: its tail is carried
};

// A Kafka batch as kafka_stage / kafka_lz4_stage leaves it: what its settling reports (the index stays in the
// slot's pinned buffer until the slot is claimed again, which launches this batch first).
struct KafkaStaged {
    u64 n_batches = 0, n_records = 0, framed_bytes = 0, control_skipped = 0;
    // a compressed batch (ysb_submit_kafka_lz4): the inflate chain runs in front of the walk
    bool lz4 = false;
    u64 n_blocks = 0, stored_blocks = 0, compressed_batches = 0;
    u32 decoder = 0;                     // the decode kernel chosen when it was staged
    u64 snappy_blocks = 0;               // of n_blocks: those tagged SNAPPY_BLOCK, and the largest raw size their
    u32 snappy_max_raw = 0;              //   preambles gave the host (0: none; sizes the decode's LDS)
    u32 crc = 0;                         // ysb_kafka_set_crc's mode when it was staged; with it on, where in the
    u64 crc_back = 0;                    //   slot's pinned buffer the batches' {computed, stored} come back
};

// A slot's batch between its submit and its launch one call later (ysb_raw.cpp).  Every submit
// assigns the whole record and launch_pending_raw resets it whole.
struct RawBatch {
    u64 nbytes = 0;                      // decoded bytes in d_bytes[slot]; a bound where only the device knows them
                                         //   (a frame or Kafka batch: its settle step reports the count)
    Layout lay;                          // its first lines' layout (sampled on the host)
    const u32* off = nullptr;            // the caller's n_off device line offsets; NULL: the GPU
    u64 n_off = 0;                       //   split's, in d_roff[slot]
    std::optional<ysb_rebase> rebase;    // its lines' event times rebased before the scan
    std::optional<Lz4Staged> lz4;        // a decode precedes the split
    std::optional<KafkaStaged> kafka;    // the Kafka kernels produce the bytes and `off` (the slot's d_roff); no split
};

struct ysb_ctx {
    int device = 0;
    ysb_config cfg{};
    std::string err;
    int cus = 256;
    hipStream_t s_comp = nullptr, s_copy = nullptr;
    // ad table
    DevBuf<u32> d_table;
    u64 table_slots = 0;
    DevBuf<u32> d_ctable;      // 36-byte-key cuckoo table
    u64 ctable_slots = 0;      // slots, or buckets when ctable_buckets
    bool ctable_buckets = false; // HBM-resident table: 3-entry 128-B buckets (CB_*), serial probes
    ysb_launch_desc last_launch{};   // the instantiation of the last launch
    // device batches' first-line samples: written by sample_kernel on the compute stream (so
    // after whatever produced the batch there) into pinned memory, two buffers alternating
    // by launch; ev_sample[k] marks buffer k complete, sample_nseg[k] its segments (0: none)
    PinBuf<u8> h_sample;
    Event ev_sample[2];
    u32 sample_nseg[2] = {0, 0};
    int sample_cur = 0;
    // the layout decided from buffer k's sample (-1: not decided yet) and its key order
    int sample_dec[2] = {-1, -1};
    LearnDesc sample_learn[2]{};
    PinBuf<u32> h_used;          // pinned: the out-of-ring map's fill level after a launch ...
    Event ev_used;                // ... readable once this has completed
    bool used_pending = false;
    // raw batches (ysb_submit_raw): the line starts are found on the GPU (ysb_split.hip) on
    // s_split after the slot's H2D, into d_roff[slot]; the scan is launched once the line
    // count is back (launch_pending_raw, at the next call), so the next H2D queues first
    hipStream_t s_split = nullptr;
    DevBuf<u32> d_roff[2];                      // raw_lines_cap starts per slot
    u64 raw_lines_cap = 0;                      // lines a raw batch may hold (raw_line_cap)
    DevBuf<u32> d_split_chunk;                  // per-chunk counts, then bases
    PinBuf<unsigned long long> h_rawn;          // pinned: [2] lines of the slot's raw batch
    Event ev_raw[2];                            // split done and its count read back
    int raw_pend = -1;                          // the slot whose raw batch awaits its launch
    int raw_fail = 0;                           // a raw batch that could not launch: sticky until ysb_reset
    std::string raw_fail_msg;
    RawBatch raw[2];                            // the slot's batch while it awaits its launch
    // H2D timing (YSB_F_TIMING): {start, end} of each slot copy since the last ysb_copy_time
    EventLog<2> cev;
    u64 copy_bytes = 0;
    // caller host ranges registered for zero-copy raw batches (ysb_host_register): base ->
    // {bytes, device address}
    struct HostRange {
        u64 bytes;
        u8* dptr;
    };
    std::map<uintptr_t, HostRange> host_ranges;
    // the replay's rebase table (ysb_rebase_table)
    DevBuf<u32> d_rebase;
    u64 rebase_n = 0;
    i64 rebase_base = 0;
    u32 rebase_kmax = 0;                        // the largest bucket index in it
    CuckooSeed cseed{};
    bool ctable_partial = false;
    bool table_loaded = false;
    u32 shard_rank = 0, shard_n = 1;      // the join table's shard (ysb_load_ad_map_shard)
    // the live map (ysb_ad_map_upsert): the distinct keys and the 36-byte keys in the cuckoo
    // table, from the build and from each upsert (what upsert_fits decides by); the call's
    // records, new-key and homeless lists and counters on the device, the counters' pinned
    // mirror, the event pair around its kernels
    u64 map_keys = 0, map_keys36 = 0;
    DevBuf<u32> d_up_rec, d_up_fresh, d_up_homeless, d_up_ctr, d_up_out;
    PinBuf<u32> h_up_ctr;
    Event ev_up[2];
    // parked views (ysb_parked_api.cpp; ysb_parked.h): park_cap records of PARK_WORDS words (0:
    // parking is off), the device counters and their pinned mirror, the distinct kernel's slot
    // table (park_slots of them) and compacted output, the resolve's campaign per record, the
    // event pair around the log's kernels; what earlier resolves took out of the log, and the
    // last distinct / resolve call's figures
    u64 park_cap = 0, park_slots = 0;
    DevBuf<u32> d_park_log, d_park_ctr, d_park_slots, d_park_lens, d_park_camp;
    DevBuf<u8> d_park_keys;
    PinBuf<u32> h_park_ctr;
    Event ev_park[2];
    u64 park_resolved_total = 0;
    ysb_parked_desc park_last{};
    // The wire buffer: per slot a batch's bytes as they crossed PCIe, compressed (LZ4 batches) or
    // framed (Kafka batches) -- through the slot's pinned buffer, or read in place from a
    // registered range (stage_wire).  A slot holds one batch, of any kind, from its copy until
    // its kernels on the split's stream are done; they leave the lines in d_bytes[slot].
    // max_batch_bytes + 64, allocated at the slot's first such batch (ensure_wire).
    DevBuf<u8> d_wire[2];
    // LZ4 batches (ysb_lz4_api.cpp; ysb_lz4.h): per slot the block descriptors -- pinned and
    // device, LZ4_DESC_HEAD bytes of {first bad, bad blocks} in front, initialised by the same
    // copy --; the pair read back to pinned memory behind the decode (h_lz4bad[2 * slot]); the
    // last settled batch's figures; YSB_F_TIMING's marks per slot: around the decode kernel, a
    // frame batch's in front of its measure pass, between it and the decode, behind the decode
    PinBuf<u8> h_lz4desc[2];
    u8* hd_lz4desc[2] = {nullptr, nullptr};
    DevBuf<u8> d_lz4desc[2];
    u64 lz4desc_cap[2] = {0, 0};
    PinBuf<u32> h_lz4bad;
    ysb_lz4_desc lz4_last{};
    Event ev_lz4[2][3];
    DevBuf<u8> d_lz4desc_sync;                  // ysb_lz4_decode_device's descriptors
    // standard frames (ysb_lz4_frame.h): the synchronous calls' device scratch -- {first bad, bad
    // blocks, raw total (u64)}, the index entries, the measured sizes, the descriptors --, the
    // last call's figures, and which decode kernel the context's LZ4 calls launch
    DevBuf<u8> d_lz4f_sync;
    ysb_lz4_frame_desc lz4f_last{};
    u32 lz4_decoder = 0;                        // YSB_LZ4_DECODER_*
    // frame batches through the slots (ysb_submit_lz4_blocks): per slot the descriptors and
    // measured sizes (the index entries and the batch's Lz4FrameHead travel in d_lz4desc[slot]),
    // the head read back to pinned memory behind the split (h_lz4f[slot]), the carry between
    // batches (Lz4 CARRY_HEAD bytes of length, then the bytes) and whether one is pending
    DevBuf<u8> d_lz4f[2];
    PinBuf<Lz4FrameHead> h_lz4f;
    DevBuf<u8> d_carry;
    bool lz4f_more = false;
    // Kafka record batches (ysb_kafka_api.cpp; ysb_kafka.h): per slot one pinned / device buffer
    // pair, {KafkaHead, the index entries} -- one copy --, and behind them on the device the
    // kernels' scratch (kafka_layout; a compressed batch's: kafka_lz4_layout, its three index
    // arrays in the one copy); the head read back to pinned memory behind the gather
    // (h_kafka_head[slot]); the synchronous call's buffer; the last call settled;
    // YSB_F_TIMING's marks around the three kernels
    PinBuf<u8> h_kafka[2];
    u8* hd_kafka[2] = {nullptr, nullptr};
    DevBuf<u8> d_kafka[2];
    u64 kafka_cap[2] = {0, 0}, kafka_hcap[2] = {0, 0};   // device bytes; pinned bytes (what the one copy carries)
    PinBuf<KafkaHead> h_kafka_head;
    DevBuf<u8> d_kafka_sync;
    ysb_kafka_desc kafka_last{};
    Event ev_kafka[2][4];
    // LZ4-compressed Kafka batches (ysb_kafka_lz4.h): per slot the inflated records (max_batch_bytes
    // + 64, allocated at the slot's first compressed submit: a context that never sees one pays
    // nothing) -- the decode's output and the walk's input --; the synchronous call's inflated
    // buffer and scratch; the plan's head read back beside the verdict; the last call settled;
    // YSB_F_TIMING's marks around measure, plan and decode
    DevBuf<u8> d_kafka_infl[2];
    DevBuf<u8> d_kafka_infl_sync, d_kafka_lz4_sync;
    PinBuf<KafkaPlanHead> h_kafka_plan;
    ysb_kafka_lz4_desc kafka_lz4_last{};
    Event ev_kafka_lz4[2][6];                   // (4, 5: around the snappy preamble kernel)
    u32 kafka_codecs = YSB_KAFKA_CODECS_DEFAULT;   // ysb_kafka_set_codecs's mask, kept across ysb_reset
    u64 kafka_infl_cap_test = 0;                   // ysb_kafka_test_inflated_cap: 0 (and after ysb_reset), or a smaller limit for the plan kernel
    // CRC-32C of Kafka batches on the device (ysb_kafka_crc.h; ysb_kafka_set_crc): the mode, kept
    // across ysb_reset; the kernel's tables and constants, built on the host and copied at the
    // first call that verifies; ysb_kafka_crc_device's scratch; the last call that verified.
    u32 kafka_crc_mode = 0;
    DevBuf<u32> d_kafka_crc_tab;
    DevBuf<u8> d_kafka_crc_sync;
    ysb_kafka_crc_desc kafka_crc_last{};
    Event ev_kafka_crc[2][2];
    // counts
    u32 c_pad = 0;                        // campaigns padded to the group size
    DevBuf<unsigned long long> d_counts;      // [c_pad][W]
    DevBuf<unsigned long long> d_owned;       // [c_pad / nranks][W] after reduce-scatter
    DevBuf<u8> d_owned8;                      // ... its saturating u8 accumulator (xunpack), folded before reads
    bool owned8_dirty = false;
    bool ring_agreed = false;                 // ranks' ring bases checked equal
    DevBuf<TableRow> d_rows;                  // drain compaction output
    DevBuf<u32> d_rows_n;
    DevBuf<i64> d_ring;                   // [lo, set]
    PinBuf<i64> h_ring;                   // pinned mirror
    Event ev_ring;
    bool ring_query_pending = false;
    bool ring_known = false;
    i64 ring_lo = 0;
    DevBuf<OvfEntry> d_ovf;
    DevBuf<u32> d_ovf_count;
    DevBuf<SideSlot> d_side;                  // out-of-ring cells (device hash map)
    u64 side_slots = 0;
    u32 side_cbits = 1;
    u32* d_side_used = nullptr;               // = (u32*)(d_stats + ST_COUNT_)
    DevBuf<unsigned long long> d_stats;       // ST_COUNT_ u64, then the map's slot count
    u64 batches = 0;
    std::map<std::pair<u32, i64>, u64> side;   // drained side-list deltas
    DivMagic div{};
    u32 lds_wl = 0, lds_wl_log2 = 0;
    // slots
    PinBuf<u8> h_bytes[2];
    PinBuf<u32> h_off[2];
    u8* hd_bytes[2] = {nullptr, nullptr};      // the pinned slots' device-visible addresses (the CU copy)
    u32* hd_off[2] = {nullptr, nullptr};
    DevBuf<u8> d_bytes[2];
    DevBuf<u32> d_off[2];
    Event ev_h2d[2], ev_kdone[2];
    // timing: per launch {before scan, after scan, after the last kernel of the launch}
    // (total[1]: the scan kernels' time, total[2]: the launch's whole path)
    EventLog<3> tev;
    double path_ms_acc = 0;                // ysb_path_time's share, collected by ysb_kernel_time
    u64 path_launches_acc = 0;
    // record mode (ysb_count.hip)
    DevBuf<u32> d_rec, d_rec_n, d_part, d_runs;
    u64 rec_launches = 0;
    RecPlan rec_last{};                    // the last record launch's plan and grid (ysb_record_info)
    u32 rec_last_grid = 0;
    // record mode counts into a saturating u8 delta ring with the u64 ring's layout (a cell
    // passing 255 goes to the u64 ring, ysb_count.hip add16); fold_delta adds it to the u64
    // ring before anything reads that.  delta_bound: events counted into it since the last
    // fold; YSB_DELTA_FOLD_EVENTS (test hook) folds before a launch once it would pass that
    DevBuf<u8> d_delta;
    u64 delta_cells = 0;
    u64 delta_bound = 0;
    u64 delta_limit = ~0ull;
    // pending counts since the last exchange: the u64 ring holds some once a launch without
    // record mode ran or a fold moved the delta there (pend_u64), or a record-mode path
    // wrote it (*d_dirty, set on the device)
    bool pend_u64 = true;
    DevBuf<u32> d_dirty;
    // group: an RCCL communicator, or the caller's host collectives (ysb_group_init_host)
    ncclComm_t comm = nullptr;
    bool host_coll = false;
    ysb_collectives hops{};
    int rank = 0, nranks = 1;
    // the range-limited exchange: per-slot maxima (all-reduced), the plan's slots, the packed
    // send / receive buffers, and its accounting (HIP event pairs, collected on request)
    // Two plan buffers (device maxima; pinned host maxima + slots): a pipelined exchange
    // packs with the previous call's plan (buffer xb, ready at xplan_ev[xb]) while its own
    // plan is reduced into the other one.
    DevBuf<unsigned long long> d_xmax;      // [2][W]
    PinBuf<unsigned long long> h_xmax;      // [2][W] maxima, then [2][W] u32 slots
    Event xplan_ev[2];
    int xb = 0;
    bool x_have_plan = false;
    // plan -> pack run on the compute stream (in order with the scans that add to the rings);
    // the reduce-scatter on s_x, beside the next launch (at N ranks: the xGMI transfer); the
    // unpack into the owned table on the compute stream again, at the next exchange (or before
    // anything reads the owned table) -- beside a running scan it starved it (round 4 A/B).
    // Two buffer sets (slots, send, receive) alternate; a pack into set k waits for the
    // reduce-scatter that last used it (ev_xdone[k]), the exchange stream for the pack
    // (ev_xpacked[k]).
    hipStream_t s_x = nullptr;
    DevBuf<u32> d_xslots;                   // [2][W]
    DevBuf<void> d_xsend[2], d_xrecv[2];
    Event ev_xpacked[2], ev_xdone[2];
    bool xset_used[2] = {false, false};
    int xk = 0;
    // the pipelined exchange whose unpack is still to run: its set, slots, width, timing entry
    int unpack_set = -1;
    u32 unpack_R = 0, unpack_width = 0;
    size_t unpack_entry = 0;
    u64 x_count = 0, x_bytes = 0;
    u32 x_last_slots = 0, x_last_width = 0;
    double x_ms = 0, x_crit_ms = 0, x_rs_ms = 0, x_exposed_ms = 0;
    // per exchange {start, packed (compute stream), reduce-scatter done (exchange stream),
    // unpack start, unpack end (compute stream)}
    std::vector<std::array<Event, 6>> xev;
    size_t xev_used = 0;
    // asynchronous flushes (ysb_flush_begin / ysb_flush_end): a ring of FLUSH_SLOTS pinned row
    // buffers the compaction kernel writes straight into, each with its device-side count
    // copied back and an event; fl_head the oldest outstanding, fl_n how many
    struct FlushSlot {
        PinBuf<TableRow> h_rows;      // pinned (device-visible: written by the kernel)
        TableRow* hd_rows = nullptr;  // ... its device address
        PinBuf<u32> h_n;              // pinned: the rows the kernel wrote
        u64 cap = 0;
        Event ev;
    };
    static constexpr int FLUSH_SLOTS = 4;
    FlushSlot fl[FLUSH_SLOTS];
    int fl_head = 0, fl_n = 0;
    DevBuf<u32> d_fl_n;                    // [FLUSH_SLOTS] device counters
    // truth
    DevBuf<unsigned long long> d_truth, d_truth_out, d_cmp;
    DevBuf<u32> d_subset;
    u32 d_subset_n = 0;
    DevBuf<u32> d_defer;                   // deferred (general-path) line indices
    DevBuf<u32> d_defer_ctr;               // [count, done, pad, pad, dynamic-claim counters[MAX_SEGS]]
    u32 dyn_pct = 0;                       // % of a large segment's tiles claimed dynamically (YSB_DYN_PCT; measured neutral, off)
    u32 dyn_chunk = 16;                    // tiles per claim (YSB_DYN_CHUNK)
    DevBuf<unsigned long long> d_dbg;      // YSB_STAMPS diagnostic build
    u64 dbg_words = 0;
    // columnar decode (ysb_columns.cpp): {valid rows, fast-tier rows} of a call, its event pair
    DevBuf<unsigned long long> d_colinfo;
    Event ev_col[2];
    // joined views (ysb_join_api.cpp; ysb_join.h): the scratch area between the three launches --
    // the tiles' blocks, their counts, the prefix; grown on first use --, a call's tallies (the
    // scan's ST_COUNT_ u64, then the fast tier's rows) and the events around its kernels
    DevBuf<u8> d_join_scratch;
    DevBuf<unsigned long long> d_join_info;
    Event ev_join[4];
    // columnar count (ysb_columns.cpp): the last columnar launch (ysb_columns_launch_info)
    ysb_colcount_desc last_col{};
    bool col_launched = false;
    // Arrow count (ysb_arrow_api.cpp): the last Arrow launch (ysb_arrow_launch_info) and its device
    // counters {per-lane tiles, rows invalid by null / offsets / dictionary index}
    ysb_arrow_desc last_arrow{};
    bool arrow_launched = false;
    DevBuf<unsigned long long> d_arrow_info;
};

// One host -> device copy of a slot: the source's device address (the copy kernel) and its
// host address (YSB_F_H2D_SDMA); 0 bytes: none.
struct SlotCopy {
    void* dst;
    const void* dsrc;
    const void* hsrc;
    u64 bytes;
};

#define YSB_INTERNAL __attribute__((visibility("hidden")))

// an error message for ysb_last_error (the context's, or the thread's when c is NULL)
YSB_INTERNAL int fail(ysb_ctx* c, int code, const char* fmt, ...);
// Grows the device buffer to at least max(bytes, floor_bytes); contents are not kept.  Before
// the old buffer is freed every stream of the context is synchronised (without launching
// pending work, unlike sync_streams): growth is outside steady state.
YSB_INTERNAL int grow_device(ysb_ctx* c, DevMem& buf, u64 bytes, u64 floor_bytes);
// A small device buffer that is allocated (bytes, not cleared) at its first use.
YSB_INTERNAL int first_use(ysb_ctx* c, DevMem& buf, u64 bytes);
// A campaign-major u64 table (the ring's layout) regrown from old_cells to cells: the first
// old_cells kept, the rest zero.  The new table is allocated before the old one goes, so a
// failed call leaves the old table in place and the context usable.
YSB_INTERNAL int regrow_table(ysb_ctx* c, DevBuf<unsigned long long>& t, u64 old_cells, u64 cells);
extern thread_local std::string g_open_err;

#define HIPCHK(ctx, expr)                                                                         \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail(ctx, YSB_ERR_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, \
                        __LINE__);                                                                \
    } while (0)

inline bool is_pow2(u64 x) { return x && !(x & (x - 1)); }   // (log2u: ysb_recplan.h)
inline int slot_arg(ysb_ctx* c, int slot) { return slot < 0 || slot > 1 ? fail(c, YSB_ERR_ARG, "slot must be 0 or 1") : YSB_OK; }

// The synchronous calls copy to and from the caller's pageable memory and their own stack: no
// return, an error's included, leaves such a copy pending.
struct SyncOnExit {
    hipStream_t s;
    ~SyncOnExit() { (void)hipStreamSynchronize(s); }
};

// YSB_F_TIMING's marks around a call's kernels.  Mark k of ev recorded on s, the event created on
// demand; ev NULL (the call is not timed): nothing.
inline hipError_t mark(Event* ev, int k, hipStream_t s) {
    if (!ev) return hipSuccess;
    if (!ev[k]) {
        const hipError_t e = ev[k].create(hipEventDefault);
        if (e != hipSuccess) return e;
    }
    return hipEventRecord(ev[k], s);
}
// The milliseconds between marks a and b added to *figure, if both are readable (complete: the
// caller has waited for what follows them); ev NULL: nothing.
inline void add_span(const Event* ev, int a, int b, double* figure) {
    float ms = 0;
    if (ev && hipEventElapsedTime(&ms, ev[a], ev[b]) == hipSuccess) *figure += ms;
}

// The slot's wire buffer (d_wire), allocated at its first use.
inline int ensure_wire(ysb_ctx* c, int slot) {
    if (!c->d_wire[slot]) HIPCHK(c, c->d_wire[slot].alloc(c->cfg.max_batch_bytes + 64));
    return YSB_OK;
}
// The slot's copy of a batch's wire bytes.  dsrc NULL: through the slot's pinned buffer, into
// which they are copied now (the caller has waited for the slot's previous copy); else they
// stay where they lie, in a registered range whose device alias of `bytes` dsrc is.
inline SlotCopy stage_wire(ysb_ctx* c, int slot, const u8* bytes, u64 nbytes, const u8* dsrc) {
    if (dsrc) return {c->d_wire[slot], dsrc, bytes, nbytes};
    if (nbytes && bytes != c->h_bytes[slot]) std::memcpy(c->h_bytes[slot], bytes, nbytes);
    return {c->d_wire[slot], c->hd_bytes[slot], c->h_bytes[slot].get(), nbytes};
}

extern "C" {
// ysb_capi.cpp
YSB_INTERNAL int sync_streams(ysb_ctx* c);       // every queued launch / copy / exchange done
YSB_INTERNAL int pull_side_list(ysb_ctx* c);     // the out-of-ring map into the host side list
YSB_INTERNAL void poll_ring(ysb_ctx* c);         // the auto-based ring's base, if known by now
YSB_INTERNAL int read_ring(ysb_ctx* c);          // ... read with a wait
YSB_INTERNAL int move_ring(ysb_ctx* c, i64 new_lo);
YSB_INTERNAL int fold_delta(ysb_ctx* c);         // record mode's u8 delta ring into the u64 ring
// ysb_submit.cpp
YSB_INTERNAL int ensure_slots(ysb_ctx* c);       // the pinned slots and their device buffers
// the launch of 1..MAX_SEGS device-resident segments (empty ones skipped) on the compute stream
YSB_INTERNAL int enqueue_scan(ysb_ctx* c, const ysb_segment* segs, u32 nseg, const Layout& lay);
// the hinted layout of a raw batch from these host bytes of it (the flags' if batches are not sampled)
YSB_INTERNAL void sampled_layout(const ysb_ctx* c, const u8* bytes, u64 nbytes, Layout* out);
// n copies of a slot on the copy stream once its previous kernel has run; ev_h2d[slot] marks them done
YSB_INTERNAL int copy_slot_ranges(ysb_ctx* c, int slot, const SlotCopy* v, int n);
// the out-of-ring map emptied into the host list if an earlier launch left it a quarter full
YSB_INTERNAL int drain_side_if_due(ysb_ctx* c);
// the context's join tables, ring, out-of-ring map and stats as a launch's parameters (no batch)
YSB_INTERNAL void context_params(ysb_ctx* c, ScanParams* out);
// The bracket of one counting launch on the compute stream, whatever its front end (enqueue_scan,
// the columnar count, the Arrow count), in this order:
//   launch_begin      the out-of-ring map emptied if it is due; L->used_out for the parameters'
//                     used_out; whether the ring still needs its base (L->base_ring)
//   launch_ring_based if so, behind the caller's auto-base kernel: the base on its way to the host
//   launch_mark 0     YSB_F_TIMING's {before the main kernel, after it, after the launch's last kernel}
//   the caller's main kernel, launch_mark 1, its level / deferred-line / record kernels
//   launch_end        mark 2, the fill level's event, the launch accounted
struct Launch {
    u32* used_out = nullptr;   // where the launch's last kernel stores the map's fill level; NULL: an earlier one is unread
    bool base_ring = false;
    Event* te = nullptr;
};
YSB_INTERNAL int launch_begin(ysb_ctx* c, Launch* L);
YSB_INTERNAL int launch_ring_based(ysb_ctx* c);
YSB_INTERNAL int launch_mark(ysb_ctx* c, Launch* L, int k);
// u64_ring: the launch counts into the u64 ring; batches: the batches it carried
YSB_INTERNAL int launch_end(ysb_ctx* c, Launch* L, bool u64_ring, u64 batches);
// A slot submit's two shared pieces.  slot_begin: the pending batch launches first (batches launch
// in submission order), the slots exist, the device is current, and the slot's previous H2D is
// done -- its pinned buffers may be rewritten.  slot_launch: the slot's copies, the compute stream
// behind them, the caller's enqueue, and the event that frees the slot's device buffers.
YSB_INTERNAL int slot_begin(ysb_ctx* c, int slot);
extern "C++" template <class Enqueue>
int slot_launch(ysb_ctx* c, int slot, const SlotCopy* v, int n, Enqueue enqueue) {
    int rc = copy_slot_ranges(c, slot, v, n);
    if (rc) return rc;
    HIPCHK(c, hipStreamWaitEvent(c->s_comp, c->ev_h2d[slot], 0));
    if ((rc = enqueue())) return rc;
    HIPCHK(c, hipEventRecord(c->ev_kdone[slot], c->s_comp));
    return YSB_OK;
}
// ysb_raw.cpp
YSB_INTERNAL int launch_pending_raw(ysb_ctx* c); // the raw batch awaiting its launch
// ysb_parked_api.cpp
// the context's log as a launch's park sites take it; false: parking is off
YSB_INTERNAL bool park_params(const ysb_ctx* c, ParkParams* out);
// the log's device counters into h_park_ctr (a small read on the compute stream; waits for it)
YSB_INTERNAL int park_counters(ysb_ctx* c);
YSB_INTERNAL int park_reset(ysb_ctx* c);         // ysb_reset's part: the log emptied, the counters zero
// ysb_lz4_api.cpp
// A compressed batch's directory checked and its descriptors placed in the slot's pinned memory,
// with its bytes (stage_wire), for the slot's copies v[2] (the caller has waited for the slot's
// previous copy): batch->lz4 the staged batch, batch->nbytes its raw size, *sample its block 0
// decoded on the host (the layout sample; empty if there is none or it is bad).
YSB_INTERNAL int lz4_stage(ysb_ctx* c, int slot, const uint8_t* bytes, uint64_t comp_bytes, const ysb_lz4_block* dir,
                           uint32_t n_blocks, const uint8_t* dsrc, RawBatch* batch, SlotCopy v[2], std::vector<u8>* sample);
// a frame batch staged (ysb_submit_lz4_blocks): the span from the first block's data to the last
// block's end as the wire bytes, the rebased index entries and the batch's head into the pinned
// descriptor buffer; batch->nbytes the bound (n_blocks + 1) x 65536; *sample block 0 decoded by
// the host model, from behind its first terminator when a carry is pending
YSB_INTERNAL int lz4f_stage(ysb_ctx* c, int slot, const uint8_t* base, const ysb_lz4_frame_block* blocks, uint32_t n_blocks,
                            uint32_t flags, const uint8_t* dsrc, RawBatch* batch, SlotCopy v[2], std::vector<u8>* sample);
// the staged batch decoded into d_bytes[slot] on s, and its {first bad, bad blocks} read back;
// *d_nbytes: where on the device the split reads a frame batch's measured byte count (else untouched)
YSB_INTERNAL int lz4_enqueue_decode(ysb_ctx* c, int slot, const Lz4Staged& b, hipStream_t s, const u64** d_nbytes);
// a frame batch's head read back to pinned memory behind the split
YSB_INTERNAL int lz4f_readback(ysb_ctx* c, int slot, hipStream_t s);
// at the batch's launch (its decode is complete): lz4_last / lz4f_last <- its figures, *nbytes
// its decoded bytes; YSB_ERR_FORMAT, the message naming the first bad block, if it had one
YSB_INTERNAL int lz4_settle(ysb_ctx* c, int slot, const Lz4Staged& b, u64* nbytes);
// ysb_kafka_api.cpp
// A Kafka batch's index checked against the slot's capacities and placed, with the bytes
// (stage_wire), for the slot's copies v[2]; batch->kafka the staged batch, *sample its first
// values as the host model unframes them, a line each (the layout sample).  The caller has
// waited for the slot's previous copy.
YSB_INTERNAL int kafka_stage(ysb_ctx* c, int slot, const uint8_t* bytes, uint64_t nbytes, const ysb_kafka_batch* batches,
                             uint64_t n_batches, const uint8_t* dsrc, RawBatch* batch, SlotCopy v[2], std::vector<u8>* sample);
// ... of a compressed one (index, frames and blocks in the slot's pinned buffer, one copy)
YSB_INTERNAL int kafka_lz4_stage(ysb_ctx* c, int slot, const uint8_t* bytes, uint64_t nbytes, const ysb_kafka_batch* batches,
                                 const ysb_kafka_frame* frames, uint64_t nb, const ysb_lz4_frame_block* blocks,
                                 uint64_t n_blocks, const uint8_t* dsrc, RawBatch* batch, SlotCopy v[2], std::vector<u8>* sample);
// the three kernels on s behind the slot's copies: d_bytes[slot], d_roff[slot]; the head's read-back
// (a compressed batch: measure, plan, decode in front of them, the codec verdict behind the walk)
YSB_INTERNAL int kafka_enqueue(ysb_ctx* c, int slot, const KafkaStaged& b, hipStream_t s);
// at the batch's launch: kafka_last <- its figures, *nbytes the value bytes the kernels left in
// d_bytes[slot]; YSB_ERR_FORMAT naming the bad Kafka batch
YSB_INTERNAL int kafka_settle(ysb_ctx* c, int slot, const KafkaStaged& b, u64* nbytes);
// any submit that is not a frame batch while a carry is pending
inline int carry_guard(ysb_ctx* c) {
    return c->lz4f_more ? fail(c, YSB_ERR_STATE, "a frame batch left a carry (YSB_LZ4F_MORE): only ysb_submit_lz4_blocks "
                                                 "may follow, until one without the flag or ysb_reset") : YSB_OK;
}
// ysb_group.cpp
YSB_INTERNAL bool grouped(const ysb_ctx* c);
YSB_INTERNAL int agree_ring(ysb_ctx* c);
YSB_INTERNAL int allreduce_max(ysb_ctx* c, i64* h, int n);
YSB_INTERNAL int finish_unpack(ysb_ctx* c);      // a pipelined exchange's owner-block unpack
YSB_INTERNAL int fold_owned(ysb_ctx* c);         // the owned table's u8 accumulator into it
}
