// ysb_kernels.h -- launch interface between the C-ABI layer (ysb_capi.cpp) and the
// gfx950 kernels (ysb_scan.hip, ysb_gen.hip).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/ysb_hip.h"   // ysb_kafka_batch: the index entry the Kafka kernels read
#include "ysb_common.h"
#include "ysb_parked.h"   // the parked views' record format and counters
#include "ysb_recplan.h"   // TILE_LINES, MAX_TILES_PER_BLOCK and record mode's REC_* constants

namespace ysb {

// Geometry of the fused scan kernel (see DESIGN.md "Kernel 1").
// One wave per workgroup: no intra-workgroup barrier ever waits for a slower wave,
// and the two waves of a SIMD drift into different phases (one classifying while the
// other parses), which hides each other's LDS latency.
constexpr int SCAN_TPB = 64;                  // threads per scan workgroup (one wave)
// (TILE_LINES, the lines per tile: ysb_recplan.h)
static_assert(TILE_LINES >= 1 && TILE_LINES <= SCAN_TPB, "one line per lane at most");
#ifndef YSB_WG_PER_CU
#define YSB_WG_PER_CU 8
#endif
constexpr int SCAN_WG_PER_CU = YSB_WG_PER_CU; // resident scan workgroups per CU (LDS-bound)
#ifndef YSB_TILE_LINE_BYTES
#define YSB_TILE_LINE_BYTES 272
#endif
constexpr int TILE_CAP = TILE_LINES * YSB_TILE_LINE_BYTES;   // LDS bytes of one tile (per-line average cap)
constexpr int TILE_CHUNKS = TILE_CAP / 16;    // 16-byte chunks per tile
constexpr int CHUNKS_PER_THREAD = (TILE_CHUNKS + SCAN_TPB - 1) / SCAN_TPB;  // 17
constexpr int LCNT_CAP = 256;                 // u32 per-workgroup (campaign, window) counters
// .tbl rows are ~140 B (JSON lines ~254 B): smaller tiles, so more workgroups fit a CU's
// LDS and the bytes in flight per CU stay comparable.
#ifndef YSB_TBL_LINE_BYTES
#define YSB_TBL_LINE_BYTES 160
#endif
#ifndef YSB_TBL_WG_PER_CU
#define YSB_TBL_WG_PER_CU 12
#endif

// Per-input-format geometry of the scan kernel: tile capacity, prefetch registers and
// the LDS carve (tile | slack | window counters | misc | tile bounds).
// Record mode (REC): the window-counter area holds the record staging lines instead --
// REC_BINS_MAX level-1 bins (ysb_recplan.h) x a 64-record ring each (2 KiB).
constexpr int REC_RING = 64;         // staged records per bin (two 128-B lines)
template <bool TBL, bool REC = false>
struct Geom {
    static constexpr int WG_PER_CU = TBL ? YSB_TBL_WG_PER_CU : SCAN_WG_PER_CU;
    // (.tbl record mode: 8 B less per row, so its record staging lines fit 12 workgroups per
    // CU in whole LDS granules; the generator's rows average 140 B, at most 151)
    static constexpr int CAP = TILE_LINES * (TBL ? YSB_TBL_LINE_BYTES - (REC ? 8 : 0) : YSB_TILE_LINE_BYTES);
    static constexpr int CHUNKS = CAP / 16;
    static constexpr int CPT = (CHUNKS + SCAN_TPB - 1) / SCAN_TPB;   // 16-byte chunks per thread
    static constexpr int OFF_TILE = 0;
    static constexpr int OFF_LCNT = OFF_TILE + CAP + 64;             // 64 B slack for reads past a tile
    static constexpr int LCNT_BYTES = REC ? REC_BINS_MAX * REC_RING * 4 : LCNT_CAP * 4;
    static constexpr int OFF_MISC = OFF_LCNT + LCNT_BYTES;
    static constexpr int OFF_TB = OFF_MISC + 64;
    static constexpr int LDS = OFF_TB + (MAX_TILES_PER_BLOCK + 4) * 4;
    static_assert(OFF_LCNT % 16 == 0 && OFF_MISC % 16 == 0 && OFF_TB % 16 == 0 && LDS % 16 == 0,
                  "LDS carve must stay 16-byte aligned");
    // LDS is allocated per workgroup in 1280-byte granules (measured round 3: a .tbl geometry
    // of 13,232 B ran 12 per CU at 2/3 speed, 12,656 B at full; 163,840 / 128 = 1280)
    static constexpr int LDS_ALLOC = (LDS + 1279) / 1280 * 1280;
    static_assert(LDS_ALLOC * WG_PER_CU <= 163840, "WG_PER_CU workgroups must fit one CU's 160 KiB of LDS");
};
constexpr int AUX_TPB = 256;                  // threads per workgroup of the other kernels

// One batch of a multi-batch launch (ysb_submit_device_segments): each keeps its own
// u32 line offsets (so each stays under 4 GiB), and one launch scans them all -- every
// workgroup walks its run of tiles in segment 0, then in segment 1, ..., without a
// grid-wide drain between batches (one launch tail per step instead of one per batch).
constexpr int MAX_SEGS = 16;
struct ScanSeg {
    const u8* bytes;            // 16-byte aligned
    const u32* off;
    u64 n;
    u64 nbytes;
    u64 line_base;              // index of the segment's first line among all segments
    u64 n_tiles;
    u64 n_static;               // tiles [0, n_static) split over the grid, the rest claimed in chunks
    u32 tiles_per_block;        // static tiles per workgroup (q) ...
    u32 static_rem;             // ... plus one for workgroups b < static_rem
};

struct ScanParams {
    // the batch being scanned: segment 0 on the host side; scan_kernel sets them to each
    // segment in turn, defer_kernel to the segment of each deferred line
    const u8* bytes;            // batch bytes (16-byte aligned)
    u64 nbytes;
    const u32* off;             // n line offsets
    u64 n;
    u64 line_base;              // segment's first line among all segments (defer list indices)
    const u32* table;           // ad table, SLOT_WORDS u32 per slot (every key)
    u32 table_mask;             // slots - 1
    const u32* ctable;          // 36-byte-key cuckoo table, CSLOT_WORDS u32 per slot
    u32 ctable_mask;
    u32 ctable_partial;         // 1: some 36-byte key missed the cuckoo build (misses defer)
    u32 probe_serial;           // 1: probe the second cuckoo slot only after a first-slot miss
    u32 tbl;                    // 1: the fork's .tbl rows (YSB_F_FORMAT_TBL) instead of JSON lines
    CuckooSeed cseed;
    u32 n_campaigns;
    unsigned long long* counts; // [c_pad][W] u64, campaign-major
    u32 ring_w;                 // W (power of two)
    u32 lds_wl;                 // per-WG window slots in LDS (power of two), 0 = off
    u32 lds_wl_log2;
    u32 require_mask;           // required-key bit mask
    const i64* ring;            // ring[0] = first bucket, ring[1] = 1 when set
    DivMagic div;
    SideSlot* side;             // out-of-ring cells (hash map)
    u32* side_used;             // slots taken
    u32 side_mask;              // slots - 1
    u32 side_cbits;             // campaign bits of a key
    OvfEntry* ovf;              // fallback list: buckets a key cannot express, or a full map
    u32* ovf_count;
    u32 ovf_cap;
    u32 tiles_per_block;
    u64 n_tiles;
    u32 grid;                   // scan workgroups: max over segments of ceil(n_tiles / tiles_per_block)
    u32 n_segs;                 // >= 1
    u32 dyn_chunk;              // tiles per dynamic claim (0: all static)
    u32* dyn_ctr;               // [MAX_SEGS] claim counters, zero at launch
    ScanSeg seg[MAX_SEGS];
    unsigned long long* stats;  // ST_COUNT_ u64
    unsigned long long* dbg;    // diagnostic build only (YSB_STAMPS): per-wave phase cycles
    u32* defer;                 // line indices for the general path (defer_kernel)
    u32* defer_count;           // [0] entries, reset by defer_kernel
    u32* defer_done;            // workgroup ticket of defer_kernel
    u32 defer_cap;
    // Record mode (large count tables, no LDS window counters: configs[2]): a joined
    // in-ring view is not an HBM atomic but a u32 record (its ring cell index) appended
    // to the sub-buffer of (workgroup, campaign range); partition_kernel and
    // count_kernel then sum the records per campaign block in LDS and add each touched
    // ring cell once (RecParams).  A full sub-buffer falls back to the atomic.
    u32 rec_on;
    u32 rec_bins;               // level-1 bins (campaign >> rec_shift), <= REC_BINS_MAX
    u32 rec_shift;
    u32 rec_cap;                // records per (workgroup, bin) sub-buffer
    u32* rec;                   // [grid][rec_bins][rec_cap]
    u32* rec_n;                 // [grid][rec_bins] records written
    u32 layout;                 // JSON layout tried first: 0 generator, 1 YSB_F_COMPACT_FIRST, 2 YSB_F_FLAT_FIRST
    // the join table's shard (ysb_load_ad_map_shard): a miss of a key whose shard is not
    // shard_rank counts as ST_FOREIGN (shard_n 1: unsharded).  Sharded contexts defer the
    // scan's misses (ctable_partial) so that only the deferred-line kernel classifies them.
    u32 shard_rank;
    u32 shard_n;
    // record mode: set when a view went to the u64 ring instead of a record (the exchange
    // then reads that ring too; ysb_capi.cpp exchange)
    u32* pend_dirty;
    // pinned host word (or null): defer_kernel stores the out-of-ring map's fill level there
    // (the host checks it at the next submit without waiting)
    u32* used_out;
    // layout 3 (a learned key order): the batch's key order as key indices (0 user_id,
    // 1 page_id, 2 ad_id, 3 ad_type, 4 event_type, 5 event_time, 6 ip_address), 3 bits per
    // key (key k in bits 3k..3k+2: no array, so no indexed private memory), read off its
    // first line by the host (ysb_capi.cpp learn_layout); learn_cp: compact separators
    u32 learn_code;
    u32 learn_n;
    u32 learn_cp;
};

// Record-mode pipeline after the scan (ysb_count.hip).  Level-2 bins ("blocks") are
// L2C = 32768 / W campaigns, so a block's L2C x W cells fit one workgroup's LDS as u32.
// Every stage writes whole 128-B lines from LDS staging: a partial-line store costs a
// memory write of its own (the XCD L2s are write-through for stores), which made scattered
// 4-B record stores as slow as the atomics they replace (tools/mb_scatter.hip).
// REC_BLOCK_CELLS, REC_QUARTERS, REC_SUB_MAX and the launch's geometry: ysb_recplan.h.
struct RecParams {
    const u32* rec;             // the scan's sub-buffers
    const u32* rec_n;
    u32 grid;                   // scan workgroups
    u32 bins;                   // level-1 bins
    u32 cap;                    // records per sub-buffer
    u32 sub_log2;               // level-2 blocks per level-1 bin = 1 << sub_log2
    u32 blk_shift;              // block = campaign >> blk_shift (L2C = 1 << blk_shift)
    u32 n_blocks;               // ceil(c_pad / L2C)
    u32 ring_w;
    u32 w_log2;
    u32 c_pad;
    u64 area;                   // u32 words of one (bin, quarter) output area
    u32* part;                  // partitioned records: [bins * QUARTERS][area], runs 32-record aligned
    u32* runs;                  // [n_blocks][QUARTERS] {offset, count} into part
    u8* delta;                  // the u8 delta ring [c_pad][W] (saturating: a cell that would pass
                                // 255 adds its whole value to the u64 ring instead and restarts at 0)
    unsigned long long* counts; // the u64 ring
    u32* dirty;                 // set when the count kernel added to the u64 ring
};
void launch_rec_partition(const RecParams& r, hipStream_t s);
void launch_rec_count(const RecParams& r, hipStream_t s);
// counts[i] += delta[i], delta[i] = 0 (cells: a multiple of 16)
void launch_fold(unsigned long long* counts, u8* delta, u64 cells, hipStream_t s);

// Range-limited exchange (ysb_group_reduce_scatter).  A rank's pending counts are its u64
// ring (read when force_u64 or *dirty) plus, in record mode, its u8 delta ring.
// xplan: slot_max[s] = max over campaigns of the pending count in ring slot s (atomicMax:
// zero slot_max first).  xpack: the pending cells of slots[0..R) as a dense [rows][R] array
// of `width`-byte cells (1, 4 or 8), the sources zeroed.  xunpack: owned[c][slots[k]] +=
// in[c][k] for the owner block's rows (through the saturating u8 accumulator owned8).
void launch_xplan(const unsigned long long* counts, const u8* delta, u32 W, u64 cells, int force_u64,
                  const u32* dirty, unsigned long long* slot_max, hipStream_t s);
void launch_xpack(unsigned long long* counts, u8* delta, u32 W, u32 rows, const u32* slots, u32 R, int force_u64,
                  const u32* dirty, void* out, u32 width, unsigned long long cap, hipStream_t s);
void launch_xunpack(unsigned long long* owned, u8* owned8, u32 W, u32 rows, const u32* slots, u32 R, const void* in,
                    u32 width, hipStream_t s);
// Linear checksum of a campaign-major [rows][W] u64 table (row i = campaign c_off + i) over
// the campaigns [c_lo, c_hi): *out += SUM count * cell_weight(campaign, bucket) (mod 2^64).
void launch_checksum(const unsigned long long* table, u32 rows, u32 W, i64 ring_lo, u32 c_off, u32 c_lo, u32 c_hi,
                     unsigned long long* out, hipStream_t s);

// BufferedReader.readLine's line split of raw bytes (ysb_split.hip): off[0..min(n, cap)) <-
// the line starts of b[0, nbytes) (b 16-byte aligned, nbytes < 4 GiB), *d_n <- n.  chunk:
// split_chunks(nbytes) u32 of scratch.  Asynchronous on s.
u64 split_chunks(u64 nbytes);
// the slots' host -> device copy by a kernel (ysb_split.hip): src a device-visible pinned host pointer
void launch_h2d_copy(void* dst, const void* src, u64 bytes, int wgs, hipStream_t s);
// the same from a device-visible host address at any byte alignment (reads up to 31 bytes
// past src + bytes, from the 16-byte boundary below src)
void launch_h2d_copy_unaligned(void* dst, const void* src, u64 bytes, int wgs, hipStream_t s);
// (d_nbytes: the byte count in device memory -- nbytes is then the bound the grid is sized
// for --, or NULL: nbytes itself, the path of every batch whose size the host knows)
hipError_t launch_split_lines(const u8* b, u64 nbytes, u32* chunk, u32* off, u64 cap, unsigned long long* d_n,
                              hipStream_t s, const u64* d_nbytes = nullptr);
// The replay's event-time rebasing (ysb_split.hip, ysb_submit_raw_mapped): for the first
// min(*d_n, tab_n, cap) lines of a split raw batch (starts off[0..cap)), the nine digits at line
// start + (tab[i] & 0xFFFF) <- lead + (tab[i] >> 16), zero-padded; writes stay inside [0, nbytes).
void launch_rebase(u8* b, u64 nbytes, const u32* off, u64 cap, const unsigned long long* d_n, u64 n_val,
                   const u32* tab, u64 tab_n, i64 lead, int cus, hipStream_t s);   // d_n NULL: n_val lines
// Layout sampling of device launches: sampled lines (spread over the launch's segments),
// copied on the device (in stream order after the batch's producer) into pinned host memory,
// SAMPLE_STRIDE bytes per line: u32 {line start, sampled length, valid, 0}, then
// <= SAMPLE_BYTES line bytes (the constants: ysb_common.h).
struct SampleSegs {                  // per sampled line: its batch and its index there
    const u8* bytes[SAMPLE_MAX];
    const u32* off[SAMPLE_MAX];
    u64 nbytes[SAMPLE_MAX];
    u64 n[SAMPLE_MAX];   // >= 1
    u64 line[SAMPLE_MAX];
};
void launch_sample(const SampleSegs& s, u32 nseg, u8* out, hipStream_t st);

constexpr int N_STAMPS = 8;     // phases timed by the YSB_STAMPS diagnostic build

// Parked views (ysb_parked.h): the context's log as the park sites (defer_kernel, the columnar
// count) and the log's own kernels (ysb_parked.hip) take it.
struct ParkParams {
    u32* log;                   // [cap][PARK_WORDS]
    u32 cap;                    // records the log holds
    u32* ctr;                   // [PK_COUNT_] (ysb_parked.h)
};

void launch_scan(const ScanParams& p, hipStream_t s);
// The general-path lines the scan deferred (same stream, right after launch_scan).  park: the
// log that takes the views whose ad is in no table (null: they are join misses).
void launch_defer(const ScanParams& p, int blocks, hipStream_t s, const ParkParams* park = nullptr);
// Sets ring[0..1] from the first lines of a batch (JSON, or .tbl rows with p.tbl) if ring[1] == 0.
void launch_ring_autobase(const ScanParams& p, hipStream_t s);

// Columnar decode (ysb_scan_columns.h, ysb_decode_columns_device): lines [0, n) of one device
// batch into rows [0, n) of the seven columns and the validity words [0, ceil(n / 64)) of out;
// nothing else of out is written.  info[0] += valid rows, info[1] += rows the fast tier took.
struct ColParams {
    const u8* bytes;            // batch bytes (16-byte aligned)
    u64 nbytes;
    const u32* off;             // n line offsets
    u64 n;
    u64 n_tiles;                // ceil(n / TILE_LINES)
    u8* out;                    // 16-byte aligned
    u64 start[8];               // byte offsets of the columns, [7] the validity bitmap (page multiples)
    i64 stamp;                  // column 6 of every valid row
    u32 java_order;             // 1: columns 5 and 6 big-endian (YSB_COL_JAVA_ORDER)
    u32 tbl;                    // 1: the fork's .tbl rows instead of JSON lines
    u32 require_mask;           // required-key bit mask (JSON)
    unsigned long long* info;   // [2]
};
void launch_columns(const ColParams& p, int cus, hipStream_t s);

// Columnar count (ysb_count_columns.h, ysb_submit_columns*): rows [0, n_rows) of a batch in the
// seven-column layout through filter, join and window count.  Reads rows < n_rows of columns 2
// (ad_id), 4 (event_type) and 5 (event_time) and, with validity, the bitmap words
// [0, ceil(n_rows / 64)) -- nothing else of cols.  sp: the context's join tables, ring,
// out-of-ring map and stats as a scan launch gets them (its batch, segment, deferred-line and
// record fields are not used; used_out as for defer_kernel).  Two instantiations: parallel
// probes of the cache-resident slots, serial probes of the HBM bucket table (sp.probe_serial).
struct ColCountParams {
    ScanParams sp;
    const u8* cols;             // 16-byte aligned
    u64 start[8];               // byte offsets of the columns, [7] the validity bitmap (page multiples)
    u64 n_rows;
    u64 n_tiles;                // ceil(n_rows / TILE_LINES)
    u32 java_order;             // 1: column 5 big-endian (YSB_COL_JAVA_ORDER)
    u32 validity;               // 1: rows with a zero validity bit are parse errors (YSB_COL_VALIDITY)
};
void launch_colcount(const ColCountParams& p, int cus, hipStream_t s, const ParkParams* park = nullptr);   // park: as launch_defer's
// Right behind it or launch_arrowcount: *sp.used_out <- the out-of-ring map's fill level (nothing
// if used_out is null).
void launch_used_level(const ScanParams& sp, hipStream_t s);
// Sets ring[0..1] from the batch's first 256 rows if ring[1] == 0 (launch_ring_autobase's rule).
void launch_colcount_autobase(const ColCountParams& p, hipStream_t s);

// Joined views as ordered columns (ysb_scan_join.h, ysb_join_device; the layout, the scratch
// format and the plan: ysb_join.h).  b: the batch as a columnar decode gets it, out the joined
// layout's buffer, start[0..5] its columns; sp: the context's join tables, with stats pointing
// at the call's own tallies (ST_COUNT_ u64 as the scan fills them, then the fast tier's rows).
// Three launches on s: the tiles' joined rows into scratch, the prefix over their counts, the
// rows into out.  Only rows < min(joined, cap_rows) of each column are written.
struct JoinParams {
    ScanParams sp;
    ColParams b;
    u8* scratch;                // join_scratch_bytes(b.n, flags) bytes, 16-byte aligned
    u32* tile_count;            // [b.n_tiles] inside scratch
    u32* prefix;                // [b.n_tiles] behind them
    u64 cap_rows;
    u32 keys;                   // 1: YSB_JOIN_KEYS
};
void launch_join(const JoinParams& p, int cus, hipStream_t s);
void launch_join_prefix(const JoinParams& p, hipStream_t s);
void launch_join_pack(const JoinParams& p, int cus, hipStream_t s);
// join_kernel's workgroups for a batch of n_tiles tiles, and the most it launches on a device of
// `cus` compute units (each workgroup walks tiles blockIdx.x + k * grid)
u32 join_grid(u64 n_tiles, int cus, bool tbl);
u32 join_max_grid(int cus, bool tbl);

// Arrow count (ysb_count_arrow.h, ysb_submit_arrow*; the row rule: ysb_arrow.h): rows
// [0, n_rows) of a batch of three Arrow columns through filter, join and window count.  Column
// c is 0 ad_id, 1 event_type, 2 event_time, 3 event_type's dictionary; every pointer is device
// memory at any alignment.  sp as for ColCountParams.  info[4] (zero before the launch) +=
// tiles on the per-lane path, rows invalid by null / offsets / dictionary index.
struct ArrowCountParams {
    ScanParams sp;
    u64 n_rows;
    u64 n_tiles;                // ceil(n_rows / TILE_LINES)
    const u8* sval;             // the struct's bitmap (or null) ...
    u64 sval_off;               // ... and row 0's bit in it
    const u8* val[4];           // the column's bitmap (or null) ...
    u64 val_off[4];             // ... and row 0's (dictionary: value 0's) bit in it
    const u8* offs[4];          // a string column's int32 offsets ...
    u64 elem[4];                // ... and row 0's (value 0's) element in them / in the values
    const u8* data[4];          // a string column's bytes from offset first[c] on; the int64 times; the int32 indices
    u32 first[4], end[4];       // string data: the offsets a value may have, [first, end]
    u32 type_dict;              // 1: event_type is dictionary-encoded
    u32 time_i64;               // 1: event_time is int64
    u32 dict_len;
    unsigned long long* info;
};
void launch_arrowcount(const ArrowCountParams& p, int cus, hipStream_t s, const ParkParams* park = nullptr);
// Sets ring[0..1] from the batch's first 256 rows if ring[1] == 0 (launch_ring_autobase's rule).
void launch_arrowcount_autobase(const ArrowCountParams& p, hipStream_t s);
// the largest grid launch_arrowcount takes on a device of `cus` compute units
u32 arrowcount_resident_grid(int cus);

// Generator kernels (ysb_gen.hip).
hipError_t gen_events_device(const GenSpec& spec, u64 first, u64 n, u8* d_out, u64 cap,
                             u32* d_off, u64* nbytes, hipStream_t s);
void launch_truth(const GenSpec& spec, u64 first, u64 n, const DivMagic& div,
                  unsigned long long* truth, u32 ring_w, const i64* ring,
                  unsigned long long* truth_outside, hipStream_t s);
// out[0] += #cells differing, out[1] += sum(truth), out[2] += sum(counts)
void launch_compare(const unsigned long long* a, const unsigned long long* b, u64 cells,
                    unsigned long long* out, hipStream_t s);
void launch_add_u64(unsigned long long* dst, const unsigned long long* src, u64 n, hipStream_t s);

// Table maintenance (ysb_table.hip): the non-zero cells of buckets [blo, blo + nb) of a
// campaign-major [rows][W] table as rows (campaign + c_off), optionally cleared.  With
// count_only only *out_n is incremented (by the number of such cells).
struct TableRow {
    u32 campaign;
    u32 pad;
    i64 bucket;
    unsigned long long count;
};
void launch_compact(unsigned long long* table, u32 rows, u32 W, i64 blo, u32 nb, u32 c_off, bool count_only,
                    bool clear, TableRow* out, u32* out_n, u32 cap, hipStream_t s);
// Empties the out-of-ring map (keys SIDE_EMPTY, counts 0).
void launch_side_clear(SideSlot* t, u64 slots, hipStream_t s);
// Every occupied slot of the out-of-ring map as rows (count_only: just the number).
void launch_side_compact(const SideSlot* t, u64 slots, u32 cbits, bool count_only, TableRow* out, u32* out_n,
                         u32 cap, hipStream_t s);

// Join-table kernels (ysb_upsert.hip): ysb_ad_map_upsert's three passes over n records of
// distinct keys in the general table's slot format {len, campaign, 14 key words} (the rules:
// ysb_admap.h), and ysb_ad_map_lookup's probe of the live tables.
enum : u32 {
    UP_NEW = 0, UP_NEW36, UP_UPDATED,          // classify: new keys, new 36-byte keys, known keys
    UP_FIRST, UP_SECOND, UP_HOMELESS,          // insert: first-fit placements, keys with both full
    UP_MOVED, UP_LEFT_OUT,                     // evict (and insert: the sparse hook's keys)
    UP_COUNT_ = 16
};
constexpr u32 UP_LEAVE_OUT = 0x80000000u;      // fresh[]: the sparse hook keeps this key out of the cuckoo table
struct UpsertParams {
    u32* table;                 // the general table
    u32 table_mask;
    u32* ctable;                // the 36-byte-key cuckoo table
    u32 ctable_mask;
    u32 buckets;                // 1: bucket layout
    u32 sparse;                 // YSB_F_SPARSE_FAST_JOIN
    CuckooSeed cseed;
    const u32* rec;             // [n][SLOT_WORDS]
    u32 n;
    u32* fresh;                 // [n] the new keys' record indices (| UP_LEAVE_OUT), classify's output
    u32* homeless;              // [n] records whose slots / buckets were both full, insert's output
    u32* ctr;                   // [UP_COUNT_], zero before classify
    u64 rng;                    // the eviction draws' first state (upsert_rng)
};
void launch_upsert_classify(const UpsertParams& p, hipStream_t s);
void launch_upsert_insert(const UpsertParams& p, u32 n_new, hipStream_t s);
void launch_upsert_evict(const UpsertParams& p, hipStream_t s);   // over ctr[UP_HOMELESS] keys, one thread
// out_campaign[i], out_where[i] of record i's key (ysb_ad_map_lookup)
void launch_admap_lookup(const UpsertParams& p, u32* out_campaign, u32* out_where, hipStream_t s);


// The log's own kernels (ysb_parked.hip).  distinct: one representative per distinct key of
// records [0, n) -- slots[0, mask] all EMPTY_SLOT before, ctr[PK_DISTINCT] zero -- compacted
// into out_keys (PARK_KEY_STRIDE bytes each) and out_lens, ctr[PK_DISTINCT] of them.
void launch_parked_distinct(const ParkParams& k, u32 n, u32* slots, u32 mask, u8* out_keys, u32* out_lens,
                            hipStream_t s);
// resolve: records [0, n) against the general table as it is now (sp: context_params).  Three
// launches: probe (camp[i] <- campaign or EMPTY_SLOT; the smallest bucket to be counted into
// ctr[PK_MINB], INT64_MAX before), base (the ring base from it if none is set), count (stats,
// ctr[PK_JOINED / PK_MISSED / PK_TIME_ERR], the ring through global_add, *sp.pend_dirty).
void launch_parked_resolve(const ScanParams& sp, const ParkParams& k, u32 n, u32* camp, hipStream_t s);

// LZ4 batches (ysb_lz4.hip; the format's rules: ysb_lz4.h).  One descriptor per block, made
// by the host from the directory: where its compressed bytes start in `in`, where its output
// starts in `out`, and the directory entry itself (comp with the stored bit).
struct Lz4Desc {
    u64 in_off, out_off;
    u32 comp, raw;
};
struct Lz4Params {
    const u8* in;               // the batch's compressed bytes, any alignment
    const Lz4Desc* desc;        // [n_blocks]
    u32 n_blocks;
    u32 max_raw;                // the largest raw of the batch (sizes the LDS window)
    u8* out;                    // block i's bytes go to out[desc[i].out_off, + raw)
    u32* bad;                   // [2]: {first bad block (LZ4_NO_BAD before), bad blocks (0 before)}
    u32 decoder;                // YSB_LZ4_DECODER_*: 0 picks the kernel by max_raw (lz4_pick_decoder)
    u32* block_bad;             // NULL, or [n_blocks] (0 before): 1 for every block recorded in bad[]
    // 0, or a launch that takes one size class of the blocks and leaves the others alone (neither
    // decoded nor bad): the one-wave kernel skips blocks of more than skip_above raw bytes, the
    // several-wave kernel blocks of skip_upto or fewer.  A compressed Kafka call, whose sizes only
    // the device knows, launches both (ysb_kafka_api.cpp).
    u32 skip_above, skip_upto;
    // 0, or bits of desc[i].comp that mark a block as another codec's (YSB_SNAPPY_BLOCK in a
    // compressed Kafka call): the LZ4 kernels leave it alone, snappy_decode_kernel takes only those
    u32 skip_tag;
};
// Every block decoded (a bad block writes nothing and is recorded in bad[]).  Asynchronous on s.
// One wave per block (lz4_decode_kernel) or four (lz4_decode_wide_kernel), by p.decoder.
hipError_t launch_lz4_decode(const Lz4Params& p, hipStream_t s);

// Standard frames (ysb_lz4_frame.h): the blocks' raw sizes are found on the GPU.  An index
// entry as the kernels read it (ysb_lz4_frame_block's layout).
struct Lz4FrameBlock {
    u64 offset;
    u32 comp, reserved;
};
// raw[i] <- block i's raw size by a walk of its tokens alone (no copies), 0 for a bad block.
// One wave per block, four blocks per workgroup.  Asynchronous on s.
// (skip_tag: bits of blocks[i].comp that mark another codec's block, whose raw[i] is left alone)
hipError_t launch_lz4_measure(const u8* base, const Lz4FrameBlock* blocks, u32 n_blocks, u32* raw, hipStream_t s,
                              u32 skip_tag = 0);

// snappy blocks (ysb_snappy.hip; the format's rules: ysb_snappy.h), for the blocks tagged
// YSB_SNAPPY_BLOCK alone.  raw[i] <- block i's preamble when it is in 1..65536, else 0: a thread
// per block.  Asynchronous on s.
hipError_t launch_snappy_preamble(const u8* base, const Lz4FrameBlock* blocks, u32 n_blocks, u32* raw, hipStream_t s);
// Every tagged block of p.desc decoded (comp: the tag and the length; raw: the planned size, which
// the kernel asks the preamble to repeat); a bad block writes nothing and is recorded in bad[] and
// block_bad[].  One wave per block, LDS sized by p.max_raw.  Asynchronous on s.
hipError_t launch_snappy_decode(const Lz4Params& p, hipStream_t s);
// desc[i] <- {blocks[i].offset, carry + the raw sizes before it, blocks[i].comp, raw[i]};
// *total <- the sum of the raw sizes.  One workgroup.  Asynchronous on s.
// (d_carry: the carry length in device memory, or NULL: `carry`)
hipError_t launch_lz4_frame_descs(const Lz4FrameBlock* blocks, const u32* raw, u32 n_blocks, u64 carry, Lz4Desc* desc,
                                  u64* total, hipStream_t s, const u64* d_carry = nullptr);

// A frame batch's device state (ysb_submit_lz4_blocks): what its kernels leave for the host,
// read back in one copy behind the split.
struct Lz4FrameHead {
    u32 bad[2];        // first bad block (LZ4_NO_BAD), bad blocks
    u64 raw_total;     // the measured sizes' sum
    u64 nbytes;        // whole lines in the slot's buffer: carry in + raw_total - carry out (0: dropped)
    u32 carry_in, carry_out;
    u32 overflow;      // the bytes behind the last certain terminator exceed LZ4_CARRY_MAX
    u32 pad;
};
constexpr u32 LZ4_CARRY_MAX = 65536;
// The context's carry: a u64 length and 8 spare bytes in front of LZ4_CARRY_MAX bytes.
constexpr u32 LZ4_CARRY_HEAD = 16;
// Behind the decode of a frame batch into out (block 0 at the carry's length): the carry of the
// batch before copied in front; with `more` the bytes behind the last certain line terminator
// (ysb_lz4_frame.h lz4f_carry_cut's rule) moved to the carry, else the carry emptied; head's
// nbytes / carry_in / carry_out / overflow written.  A batch with a bad block or an overflow is
// dropped: nbytes 0, the carry emptied.  One workgroup.  Asynchronous on s.
hipError_t launch_lz4_frame_carry(u8* out, u8* carry, Lz4FrameHead* head, u32 more, hipStream_t s);

// Kafka record batches (ysb_kafka.hip; the format's rules: ysb_kafka.h).  Three launches between
// the framed bytes and the scan's input.  What the walk leaves per Kafka batch:
struct KafkaBatchOut {
    u64 total;                  // its values' bytes
    u32 bad_rec, rule;          // its smallest bad record and that record's rule (rule 0: a good batch)
    u32 nulls, keyed, headers, pad;
};
// ... and the call's result, which the base kernel writes and the host reads back.
struct KafkaHead {
    u64 out_bytes, n_lines;
    u32 bad_batches, first_bad, bad_rec, rule;   // first_bad KAFKA_NONE: none
    u64 nulls, keyed, headers;
    u32 overflow, pad;          // the values exceed out_cap or 4 GiB: nothing is gathered
};
struct KafkaParams {
    const u8* bytes;            // the framed bytes, any alignment
    const ysb_kafka_batch* batches;
    u32 n_batches;
    u64 n_records;              // the batches' records in all
    uint4* meta;                // [n_records] {value position in its batch, output offset in its batch, length, batch}
    KafkaBatchOut* bout;        // [n_batches]
    u64* base;                  // [n_batches] where a batch's values start in out
    KafkaHead* head;
    u8* out;
    u64 out_cap;
    u32* line_off;              // [n_records + 1]
};
// One wave per Kafka batch: the serial chain of record lengths, 64 record bodies parsed at a
// time, meta and bout written.  Nothing outside the 16-byte vectors that hold
// [records_off, records_off + records_bytes) is read.  Asynchronous on s; n_batches >= 1.
hipError_t launch_kafka_walk(const KafkaParams& p, hipStream_t s);
// One workgroup: base <- the exclusive scan of the good batches' totals, *head <- the result.
hipError_t launch_kafka_base(const KafkaParams& p, hipStream_t s);
// Each value copied to out + base[batch] + its offset, line_off written (line_off[n_records]:
// the total); nothing at all when head says a batch is bad or the values do not fit.
hipError_t launch_kafka_gather(const KafkaParams& p, hipStream_t s);

// CRC-32C of the indexed batches (ysb_kafka_crc.h), between the walk and the base kernel: one
// wave per batch at a time, a bounded grid looping over the batches so that the copy of the 16
// KiB of tables into LDS amortises.
struct KafkaCrcParams {
    const u8* bytes;            // the wire bytes, any alignment
    const ysb_kafka_batch* batches;   // [n_batches] the host's index: records_off >= 44, the host checked
    u32 n_batches;
    const u32* tables;          // CRC_TABLE_WORDS (distance CRC_WIN), then CRC_CONST_WORDS
    uint2* crc;                 // [n_batches] out: {computed, stored}
    KafkaBatchOut* bout;        // [n_batches] a batch whose CRC differs becomes rule 9; NULL: the values only
};
constexpr u32 KAFKA_CRC_TPB = 256;           // four waves: four batches at a time
constexpr u32 KAFKA_CRC_WGS_PER_CU = 4;      // the grid's bound
// Only the 16-byte vectors that hold [records_off - 44, records_off + records_bytes) of a batch
// are read.  Asynchronous on s; n_batches >= 1.
hipError_t launch_kafka_crc(const KafkaCrcParams& p, u32 cus, hipStream_t s);
inline u32 kafka_crc_grid_waves(u32 cus) { return cus * KAFKA_CRC_WGS_PER_CU * (KAFKA_CRC_TPB / 64); }


// LZ4-compressed Kafka batches (ysb_kafka_lz4.h): between the measure pass and the decode, one
// launch turns the measured sizes into the decode's descriptors AND the walk's index.
struct KafkaPlanHead {
    u32 bad[2];                 // the decode's Lz4Params::bad (the plan sets LZ4_NO_BAD, 0)
    u32 zero_blocks;            // blocks the measure pass refused
    u32 decoder_bad;            // blocks only the decoder refused (kafka_codec_kernel)
    u64 inflated;               // the measured sizes' sum
};
struct KafkaPlanParams {
    const Lz4FrameBlock* blocks;     // [n_blocks] offsets into the wire bytes
    const u32* raw;                  // [n_blocks] the measured sizes, 0: a bad block
    u32 n_blocks;
    const ysb_kafka_frame* frames;   // [n_batches]: first_block + n_blocks <= n_blocks, the host checked
    const ysb_kafka_batch* batches;  // [n_batches] the host's index (never written)
    u32 n_batches;
    Lz4Desc* desc;                   // [n_blocks] out: out_off the inflated offset; raw 0 for every block of a bad batch
    u32* zeros;                      // [n_blocks + 1] out: the bad blocks in front of block i
    u32* block_bad;                  // [n_blocks] out: zeroed (the decode's per-block flags)
    ysb_kafka_batch* planned;        // [n_batches] out: records_off / records_bytes in the inflated buffer, the rest copied
    u32* codec_bad;                  // [n_batches] out: the smallest block measured 0, or KAFKA_NONE
    KafkaPlanHead* head;
    u64 infl_cap;                    // the inflated buffer's bytes: a batch whose extent would pass them is bad
};
// One workgroup: a pass over the blocks with two running prefixes (raw bytes, blocks measured
// 0), KAFKA_PLAN_STEP blocks per step, then one thread per Kafka batch.  Asynchronous on s.
constexpr u32 KAFKA_PLAN_STEP = 256;
hipError_t launch_kafka_plan(const KafkaPlanParams& p, hipStream_t s);
// Behind the walk, in front of the base kernel: bout[k] <- {rule 8, the smallest bad block} for
// every batch with a block the plan (codec_bad) or the decoder (block_bad) refused.
hipError_t launch_kafka_codec(const KafkaPlanParams& p, KafkaBatchOut* bout, hipStream_t s);

}  // namespace ysb
