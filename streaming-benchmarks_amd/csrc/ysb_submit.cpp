// ysb_submit.cpp -- segments into launches: the pinned double-buffered slots (ysb_submit) and
// their copies, device batches (ysb_submit_device*), the layout samples that pick the scan
// instantiation (their rules: ysb_layout.h), record-mode planning and the launch sequence
// itself (scan, deferred lines, record partition + count).  The batches that launch a call
// after their submit (raw lines, mapped, compressed) are ysb_raw.cpp's.
#include "ysb_ctx.h"

using namespace ysb;

extern "C" {

// ---- batches ---------------------------------------------------------------------------

static u32 require_mask(const ysb_ctx* c) { return (c->cfg.flags & YSB_F_REQUIRE_IP) ? 0x7Fu : 0x3Fu; }
static bool flat_first(const ysb_ctx* c) { return (c->cfg.flags & YSB_F_FLAT_FIRST) != 0; }

// segs: 1..MAX_SEGS batches, none empty
static ScanParams make_params(ysb_ctx* c, const ysb_segment* segs, u32 nseg, const Layout& lay) {
    ScanParams p{};
    p.tbl = (c->cfg.flags & YSB_F_FORMAT_TBL) ? 1u : 0u;
    p.bytes = segs[0].d_bytes;
    p.nbytes = segs[0].nbytes;
    p.off = segs[0].d_line_off;
    p.n = segs[0].n_events;
    p.line_base = 0;
    p.table = c->d_table;
    p.table_mask = (u32)(c->table_slots - 1);
    p.ctable = c->d_ctable;
    p.ctable_mask = (u32)(c->ctable_slots - 1);
    p.cseed = c->cseed;
    // a sharded table's misses go to the deferred-line kernel, which tells a foreign-shard
    // key from a real miss (the scan kernels themselves carry no shard logic)
    // -- and so do a context's with parking enabled (ysb_parked_enable): that kernel and the
    // columnar count hold the park sites
    p.ctable_partial = (c->ctable_partial || c->shard_n > 1 || c->park_cap) ? 1u : 0u;
    p.shard_rank = c->shard_rank;
    p.shard_n = c->shard_n;
    p.pend_dirty = c->d_dirty;
    // HBM-resident table: buckets, the second one read only after a miss in a full first
    p.probe_serial = c->ctable_buckets ? 1u : 0u;
    p.layout = (c->cfg.flags & YSB_F_FLAT_FIRST) ? 2u : (c->cfg.flags & YSB_F_COMPACT_FIRST) ? 1u : 0u;
    if (lay.layout >= 0) p.layout = (u32)lay.layout;
    if (p.layout == 3 || p.layout == 4) {   // (4: learn_n 0 when the sample named no learned order)
        p.learn_code = 0;
        for (u32 i = 0; i < lay.learn.n; ++i) p.learn_code |= lay.learn.order[i] << (3 * i);
        p.learn_n = lay.learn.n;
        p.learn_cp = lay.learn.cp;
    }
    p.n_campaigns = c->cfg.n_campaigns;
    p.counts = c->d_counts;
    p.ring_w = c->cfg.window_ring;
    p.lds_wl = c->lds_wl;
    p.lds_wl_log2 = c->lds_wl_log2;
    p.require_mask = require_mask(c);
    p.ring = c->d_ring;
    p.div = c->div;
    p.side = c->d_side;
    p.side_used = c->d_side_used;
    p.side_mask = (u32)(c->side_slots - 1);
    p.side_cbits = c->side_cbits;
    p.ovf = c->d_ovf;
    p.ovf_count = c->d_ovf_count;
    p.ovf_cap = (u32)c->cfg.overflow_capacity;
    p.stats = c->d_stats;
    // Each segment's tiles: a static share split evenly over the grid, and for large
    // segments (>= 8 tiles per resident workgroup) a dynamic share of dyn_pct % claimed in
    // chunks by the workgroups that finish first.  The grid is whole rounds of resident
    // workgroups (a partial last round would idle most CUs), enough that no static run
    // exceeds MAX_TILES_PER_BLOCK tiles (the LDS copy of a run's tile bounds).
    const u64 resident = (u64)c->cus * (p.tbl ? Geom<true>::WG_PER_CU : Geom<false>::WG_PER_CU);
    const u32 chunk = std::min<u32>(c->dyn_chunk, MAX_TILES_PER_BLOCK);
    u64 line_base = 0, max_static = 0;
    bool any_dyn = false;
    p.n_segs = nseg;
    for (u32 i = 0; i < nseg; ++i) {
        ScanSeg& sg = p.seg[i];
        sg.bytes = segs[i].d_bytes;
        sg.off = segs[i].d_line_off;
        sg.n = segs[i].n_events;
        sg.nbytes = segs[i].nbytes;
        sg.line_base = line_base;
        line_base += sg.n;
        sg.n_tiles = (sg.n + TILE_LINES - 1) / TILE_LINES;
        const bool dyn = chunk && c->dyn_pct && sg.n_tiles >= 8 * resident;
        sg.n_static = dyn ? sg.n_tiles - sg.n_tiles * std::min<u32>(c->dyn_pct, 100) / 100 : sg.n_tiles;
        any_dyn |= sg.n_static < sg.n_tiles;
        max_static = std::max(max_static, sg.n_static);
    }
    const u64 rounds = std::max<u64>(1, (max_static + resident * MAX_TILES_PER_BLOCK - 1) / (resident * MAX_TILES_PER_BLOCK));
    const u64 grid = std::max<u64>(1, std::min<u64>(max_static, rounds * resident));
    for (u32 i = 0; i < nseg; ++i) {
        ScanSeg& sg = p.seg[i];
        sg.tiles_per_block = (u32)(sg.n_static / grid);
        sg.static_rem = (u32)(sg.n_static % grid);
    }
    p.dyn_chunk = any_dyn ? chunk : 0u;
    p.n_tiles = p.seg[0].n_tiles;
    p.tiles_per_block = p.seg[0].tiles_per_block;
    p.grid = (u32)grid;
    return p;
}

// s waits for e -- unless e has completed already: the slot copies' wait for the slot's last
// scan is normally long satisfied, and a cross-queue barrier packet costs the copy queue time
// between copies even when it has nothing to wait for.
static hipError_t wait_unless_done(hipStream_t s, hipEvent_t e) {
    if (hipEventQuery(e) == hipSuccess) return hipSuccess;
    return hipStreamWaitEvent(s, e, 0);
}

// Record mode (ysb_count.hip) for this launch: large count tables without LDS window
// counters (configs[2]), where one global atomic per joined view is the bottleneck.
// Auto: ring >= 1M cells and launch >= 1M events; YSB_F_RECORD_COUNT forces it on
// wherever it is possible, YSB_F_NO_RECORD_COUNT off.
static int plan_records(ysb_ctx* c, ScanParams& p, u64 n_events, RecParams& r) {
    p.rec_on = 0;
    const u32 W = c->cfg.window_ring;
    const u64 cells = (u64)c->c_pad * W;
    const bool force = (c->cfg.flags & YSB_F_RECORD_COUNT) != 0;
    // (the record-mode kernels are the HBM-table instantiations: bucket-layout join table)
    if ((c->cfg.flags & YSB_F_NO_RECORD_COUNT) || c->lds_wl || p.dyn_chunk || !c->ctable_buckets) return YSB_OK;
    if (!force && (cells < (1ull << 20) || n_events < (1ull << 20))) return YSB_OK;
    // tiles one workgroup scans at most in this launch, then the geometry (ysb_recplan.h)
    u64 tiles = 0;
    for (u32 i = 0; i < p.n_segs; ++i) tiles += p.seg[i].tiles_per_block + (p.seg[i].static_rem ? 1 : 0);
    RecPlan pl;
    if (!rec_plan(c->c_pad, W, p.grid, tiles, &pl)) return YSB_OK;
    r.ring_w = W;
    r.w_log2 = pl.w_log2;
    r.blk_shift = pl.blk_shift;
    r.c_pad = c->c_pad;
    r.n_blocks = pl.n_blocks;
    r.sub_log2 = pl.sub_log2;
    r.bins = pl.bins;
    r.grid = p.grid;
    r.cap = pl.cap;
    r.area = pl.area;
    int rc;
    if ((rc = grow_device(c, c->d_rec, (u64)r.grid * r.bins * pl.cap * 4, 0))) return rc;
    if ((rc = grow_device(c, c->d_rec_n, (u64)r.grid * r.bins * 4, 0))) return rc;
    if ((rc = grow_device(c, c->d_part, pl.part * 4, 0))) return rc;
    if ((rc = grow_device(c, c->d_runs, (u64)r.n_blocks * REC_QUARTERS * 2 * 4, 0))) return rc;
    if (c->delta_cells != cells) {   // the delta ring: the u64 ring's layout, one byte a cell, zeroed
        if ((rc = fold_delta(c))) return rc;
        c->delta_cells = 0;   // (c_pad only grows, and ysb_group_init drops the ring it outgrows)
        if ((rc = grow_device(c, c->d_delta, cells, 0))) return rc;
        HIPCHK(c, hipMemset(c->d_delta, 0, cells));
        c->delta_cells = cells;
    }
    // the delta saturates instead of wrapping, so it needs no fold between launches; the
    // test hook YSB_DELTA_FOLD_EVENTS folds anyway once the events since the last fold
    // would reach its bound
    if (c->delta_bound + n_events >= c->delta_limit && (rc = fold_delta(c))) return rc;
    c->delta_bound += n_events;
    r.delta = c->d_delta;
    r.counts = c->d_counts;
    r.dirty = c->d_dirty;
    r.rec = c->d_rec;
    r.rec_n = c->d_rec_n;
    r.part = c->d_part;
    r.runs = c->d_runs;
    p.rec_on = 1;
    p.rec_bins = r.bins;
    p.rec_shift = r.blk_shift + r.sub_log2;
    p.rec_cap = r.cap;
    p.rec = c->d_rec;
    p.rec_n = c->d_rec_n;
    c->rec_last = pl;   // (ysb_record_info)
    c->rec_last_grid = p.grid;
    return YSB_OK;
}

// The out-of-ring map's fill level after an earlier launch (read without waiting): a quarter
// full empties it into the exact host list before the next launch adds to it.
int drain_side_if_due(ysb_ctx* c) {
    if (c->used_pending && hipEventQuery(c->ev_used) == hipSuccess) {
        c->used_pending = false;
        if ((u64)*c->h_used * 4 > c->side_slots) {
            int rc = sync_streams(c);
            if (!rc) rc = pull_side_list(c);
            if (rc) return rc;
        }
    }
    return YSB_OK;
}

void context_params(ysb_ctx* c, ScanParams* out) {
    const ysb_segment none{nullptr, 0, nullptr, 1};
    *out = make_params(c, &none, 1, Layout{});
}

// ---- the bracket of a counting launch (ysb_ctx.h) ----------------------------------------------

int launch_begin(ysb_ctx* c, Launch* L) {
    const int rc = drain_side_if_due(c);
    if (rc) return rc;
    L->used_out = c->used_pending ? nullptr : c->h_used.get();
    poll_ring(c);
    L->base_ring = !c->ring_known;
    return YSB_OK;
}

int launch_ring_based(ysb_ctx* c) {
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->h_ring, c->d_ring, 16, hipMemcpyDeviceToHost, c->s_comp));
    HIPCHK(c, hipEventRecord(c->ev_ring, c->s_comp));
    c->ring_query_pending = true;
    return YSB_OK;
}

int launch_mark(ysb_ctx* c, Launch* L, int k) {
    if (!(c->cfg.flags & YSB_F_TIMING)) return YSB_OK;
    if (k == 0) HIPCHK(c, c->tev.acquire(&L->te));
    HIPCHK(c, hipEventRecord(L->te[k], c->s_comp));
    return YSB_OK;
}

int launch_end(ysb_ctx* c, Launch* L, bool u64_ring, u64 batches) {
    if (const int rc = launch_mark(c, L, 2)) return rc;
    if (u64_ring) c->pend_u64 = true;
    if (L->used_out) {   // the launch's last kernel wrote the map's fill level into h_used
        HIPCHK(c, hipEventRecord(c->ev_used, c->s_comp));
        c->used_pending = true;
    }
    c->batches += batches;
    return YSB_OK;
}

int enqueue_scan(ysb_ctx* c, const ysb_segment* in, u32 nin, const Layout& lay) {
    if (!c->table_loaded) return fail(c, YSB_ERR_STATE, "ysb_load_ad_map has not been called");
    ysb_segment segs[MAX_SEGS];
    u32 nseg = 0;
    u64 n = 0;
    for (u32 i = 0; i < nin; ++i)
        if (in[i].n_events) { segs[nseg++] = in[i]; n += in[i].n_events; }
    if (n == 0) { c->batches += nin; return YSB_OK; }
    if (n >= (1ull << 31)) return fail(c, YSB_ERR_CAPACITY, "at most 2^31-1 events per launch");
    // the deferred-line list can hold every line of a batch
    int rc = grow_device(c, c->d_defer, n * 4, 4u << 16);
    if (rc) return rc;
    if (!c->d_defer_ctr) {
        HIPCHK(c, c->d_defer_ctr.alloc(16 + 4 * MAX_SEGS));
        HIPCHK(c, hipMemset(c->d_defer_ctr, 0, 16 + 4 * MAX_SEGS));
    }
    Launch L;
    if ((rc = launch_begin(c, &L))) return rc;
    ScanParams p = make_params(c, segs, nseg, lay);
    p.used_out = L.used_out;
    p.defer = c->d_defer;
    p.defer_count = c->d_defer_ctr;
    p.defer_done = c->d_defer_ctr + 1;
    p.dyn_ctr = c->d_defer_ctr + 4;
    p.defer_cap = (u32)(c->d_defer.bytes() / 4);
#if defined(YSB_STAMPS) || defined(YSB_WGTIME)
    const u64 words = (u64)c->cus * std::max(Geom<true>::WG_PER_CU, Geom<false>::WG_PER_CU) * (SCAN_TPB / 64) * N_STAMPS;
    if (!c->d_dbg) {
        HIPCHK(c, c->d_dbg.alloc(words * 8));
        HIPCHK(c, hipMemset(c->d_dbg, 0, words * 8));
        c->dbg_words = words;
    }
    p.dbg = c->d_dbg;
#endif
    if (L.base_ring) {
        launch_ring_autobase(p, c->s_comp);
        if ((rc = launch_ring_based(c))) return rc;
    }
    // dynamic claims (off by default) count from zero in every launch
    if (p.dyn_chunk) HIPCHK(c, hipMemsetAsync(p.dyn_ctr, 0, 4 * MAX_SEGS, c->s_comp));
    RecParams rp{};
    if ((rc = plan_records(c, p, n, rp))) return rc;
    if ((rc = launch_mark(c, &L, 0))) return rc;
    launch_scan(p, c->s_comp);
    HIPCHK(c, hipGetLastError());
    // (launch_scan: the layout instantiations exist for every JSON table layout)
    c->last_launch.layout = p.tbl ? 0u : p.layout;
    c->last_launch.record_mode = p.rec_on ? 1u : 0u;
    c->last_launch.hbm_table = p.probe_serial ? 1u : 0u;
    c->last_launch.tbl = p.tbl ? 1u : 0u;
    if ((rc = launch_mark(c, &L, 1))) return rc;
    ParkParams park;
    launch_defer(p, c->cus, c->s_comp, park_params(c, &park) ? &park : nullptr);
    HIPCHK(c, hipGetLastError());
    if (p.rec_on) {
        launch_rec_partition(rp, c->s_comp);
        HIPCHK(c, hipGetLastError());
        launch_rec_count(rp, c->s_comp);
        HIPCHK(c, hipGetLastError());
        c->rec_launches++;
    }
    // (record mode counts into the delta ring; each segment counts as the batch it is)
    return launch_end(c, &L, !p.rec_on, nin);
}

// Whether batches pick the scan instantiation from their first line (the default): not
// with YSB_F_COMPACT_FIRST or YSB_F_LAYOUT_FIXED, and only where the layout instantiations
// exist (JSON: the cache-resident table's and, since round 4, the HBM-resident table's
// serial-probe and record-mode kernels).  Under YSB_F_FLAT_FIRST the sample only tells
// whether the batch has one learnable key order (hinted_layout).
static bool layout_sampling(const ysb_ctx* c) {
    const u32 f = c->cfg.flags;
    return !(f & (YSB_F_LAYOUT_FIXED | YSB_F_COMPACT_FIRST | YSB_F_FORMAT_TBL));
}

void sampled_layout(const ysb_ctx* c, const u8* bytes, u64 nbytes, Layout* out) {
    *out = Layout{};
    if (layout_sampling(c)) out->layout = hinted_layout(flat_first(c), sniff_raw(require_mask(c), bytes, nbytes, &out->learn));
}

// Device batches: SAMPLE_LINES lines spread over the launch's segments (as sniff_layout
// spreads them over a host batch), copied by sample_kernel on the compute stream -- in
// stream order, so after whatever produced the batch there (the caller's contract: a device
// batch is complete when submitted, or its producer is ordered before ysb_stream(ctx)) --
// into one of two pinned buffers, alternating by launch.  Which layout runs:
//  * compute stream idle at the submit: this launch's own sample (the copy takes microseconds);
//  * busy: the previous launch's sample (queued behind the launch before it, so the host waits
//    for that one, never for the launch it is queueing behind) -- if it and the sample before
//    it decided the same layout (or there is no decided sample before it), that one; if they
//    disagree (producers alternating by batch,
//    or a producer that just changed its layout), the per-tile dispatch (4), which takes every
//    producer's tiles at that producer's speed, until two samples agree again;
//  * busy with no earlier sample (the first launch queued behind other work): the per-tile
//    dispatch, without a wait.
// So a producer that changes its layout costs one launch of the wrong instantiation and then
// dispatch launches until it settles; counts never depend on the choice.
static int decide_sample(ysb_ctx* c, int k) {
    if (c->sample_dec[k] >= 0) return YSB_OK;
    HIPCHK(c, hipEventSynchronize(c->ev_sample[k]));
    const u8* h = c->h_sample + (u64)k * SAMPLE_LINES * SAMPLE_STRIDE;
    std::vector<std::pair<const u8*, u64>> lines;
    LearnDesc d{};
    int lay = -1;
    for (u32 i = 0; i < c->sample_nseg[k]; ++i) {
        const u8* sp = h + (u64)i * SAMPLE_STRIDE;
        u32 hd[3];
        std::memcpy(hd, sp, 12);
        if (!hd[2]) { lay = 0; break; }   // bad offsets: the scan defers them anyway
        lines.push_back({sp + 16, hd[1]});
    }
    if (lay < 0) lay = decide_layout(require_mask(c), lines, &d);
    c->sample_dec[k] = lay;
    c->sample_learn[k] = lay == 3 || lay == 4 ? d : LearnDesc{};
    return YSB_OK;
}

static int sample_device_layout(ysb_ctx* c, const ysb_segment* segs, u32 nseg, Layout* out) {
    const u64 buf = (u64)SAMPLE_LINES * SAMPLE_STRIDE;
    if (!c->h_sample) {
        HIPCHK(c, c->h_sample.alloc(2 * buf));
        for (Event& e : c->ev_sample) HIPCHK(c, e.create());
    }
    const bool idle = hipStreamQuery(c->s_comp) == hipSuccess;
    const int k = c->sample_cur;
    c->sample_cur ^= 1;
    // buffer k still holds the sample of the launch before the previous one: its decision (if
    // the copy is done -- it is whenever the previous launch waited for a sample) is the
    // older of the two the busy rule compares
    if (c->sample_nseg[k] && c->sample_dec[k] < 0 && hipEventQuery(c->ev_sample[k]) == hipSuccess) {
        int rc = decide_sample(c, k);
        if (rc) return rc;
    }
    const int older = c->sample_nseg[k] ? c->sample_dec[k] : -1;
    const LearnDesc older_learn = c->sample_learn[k];
    u64 total = 0;
    for (u32 i = 0; i < nseg; ++i) total += segs[i].n_events;
    SampleSegs ss{};
    u32 n = 0;
    for (u32 j = 0; j < SAMPLE_LINES && j < total; ++j) {
        u64 g = sample_index(total, j), i = 0;   // global line -> (segment, line)
        while (g >= segs[i].n_events) g -= segs[i++].n_events;
        ss.bytes[n] = segs[i].d_bytes;
        ss.off[n] = segs[i].d_line_off;
        ss.nbytes[n] = segs[i].nbytes;
        ss.n[n] = segs[i].n_events;
        ss.line[n] = g;
        ++n;
    }
    launch_sample(ss, n, c->h_sample + (u64)k * buf, c->s_comp);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev_sample[k], c->s_comp));
    c->sample_nseg[k] = n;
    c->sample_dec[k] = -1;
    int rc;
    if (idle) {   // this launch's own sample
        if ((rc = decide_sample(c, k))) return rc;
        *out = {c->sample_dec[k], c->sample_learn[k]};
        return YSB_OK;
    }
    const int p = k ^ 1;   // the previous launch's sample
    if (!c->sample_nseg[p]) {   // none: no wait, the dispatch
        *out = {4, LearnDesc{}};
        return YSB_OK;
    }
    if ((rc = decide_sample(c, p))) return rc;
    out->layout = settled_layout(older, older_learn, c->sample_dec[p], c->sample_learn[p], &out->learn);
    return YSB_OK;
}

int ensure_slots(ysb_ctx* c) {
    if (c->h_bytes[0]) return YSB_OK;
    HIPCHK(c, hipSetDevice(c->device));
    for (int s = 0; s < 2; ++s) {
        HIPCHK(c, c->h_bytes[s].alloc(c->cfg.max_batch_bytes + 64));
        HIPCHK(c, c->h_off[s].alloc(c->cfg.max_batch_events * 4 + 64));
        HIPCHK(c, c->d_bytes[s].alloc(c->cfg.max_batch_bytes + 64));
        HIPCHK(c, c->d_off[s].alloc(c->cfg.max_batch_events * 4 + 64));
        HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&c->hd_bytes[s]), c->h_bytes[s], 0));
        HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&c->hd_off[s]), c->h_off[s], 0));
    }
    return YSB_OK;
}

// A slot's host -> device copy on the copy stream: by the CUs from the pinned slot's device
// address (launch_h2d_copy, the default: ysb_split.hip says why; a mapped batch that does not
// start on a 16-byte boundary by launch_h2d_copy_unaligned), or by the DMA engine with
// YSB_F_H2D_SDMA.  H2D_WGS: the copy kernels' grid (clamped to the vectors there are by their
// launch functions; why 32: ysb_raw.cpp enqueue_deferred).
constexpr int H2D_WGS = 32;
static hipError_t h2d(ysb_ctx* c, void* dst, const void* dsrc, const void* hsrc, u64 bytes) {
    if (c->cfg.flags & YSB_F_H2D_SDMA) return hipMemcpyAsync(dst, hsrc, bytes, hipMemcpyHostToDevice, c->s_copy);
    if (reinterpret_cast<uintptr_t>(dsrc) & 15) launch_h2d_copy_unaligned(dst, dsrc, bytes, H2D_WGS, c->s_copy);
    else launch_h2d_copy(dst, dsrc, bytes, H2D_WGS, c->s_copy);
    return hipGetLastError();
}

// A slot's copies (0 bytes: none) on the copy stream once the slot's previous kernel has run
// -- its device buffers are free then -- with YSB_F_TIMING inside an event pair
// (ysb_copy_time); ev_h2d[slot] marks them done.  (SlotCopy: ysb_ctx.h)
int copy_slot_ranges(ysb_ctx* c, int slot, const SlotCopy* v, int n) {
    HIPCHK(c, wait_unless_done(c->s_copy, c->ev_kdone[slot]));
    Event* ce = nullptr;
    if (c->cfg.flags & YSB_F_TIMING) {
        HIPCHK(c, c->cev.acquire(&ce));
        for (int i = 0; i < n; ++i) c->copy_bytes += v[i].bytes;
        HIPCHK(c, hipEventRecord(ce[0], c->s_copy));
    }
    for (int i = 0; i < n; ++i)
        if (v[i].bytes) HIPCHK(c, h2d(c, v[i].dst, v[i].dsrc, v[i].hsrc, v[i].bytes));
    if (ce) HIPCHK(c, hipEventRecord(ce[1], c->s_copy));
    HIPCHK(c, hipEventRecord(c->ev_h2d[slot], c->s_copy));
    return YSB_OK;
}

int slot_begin(ysb_ctx* c, int slot) {
    int rc = launch_pending_raw(c);
    if (!rc) rc = ensure_slots(c);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipEventSynchronize(c->ev_h2d[slot]));
    return YSB_OK;
}

int ysb_slot_buffers(ysb_ctx* c, int slot, uint8_t** bytes, uint32_t** line_off) {
    if (!c) return YSB_ERR_ARG;
    int rc = slot_arg(c, slot);
    if (!rc) rc = ensure_slots(c);
    if (rc) return rc;
    if (bytes) *bytes = c->h_bytes[slot];
    if (line_off) *line_off = c->h_off[slot];
    return YSB_OK;
}

int ysb_submit(ysb_ctx* c, int slot, const uint8_t* bytes, uint64_t nbytes, const uint32_t* line_off,
               uint64_t n) {
    if (!c) return YSB_ERR_ARG;
    if (int rc = slot_arg(c, slot)) return rc;
    if (nbytes > c->cfg.max_batch_bytes || n > c->cfg.max_batch_events)
        return fail(c, YSB_ERR_CAPACITY, "batch (%llu B, %llu events) exceeds max_batch_bytes/max_batch_events",
                    (unsigned long long)nbytes, (unsigned long long)n);
    if ((nbytes && !bytes) || (n && !line_off)) return fail(c, YSB_ERR_ARG, "NULL batch buffers");
    if (int g = carry_guard(c)) return g;
    if (int rc = slot_begin(c, slot)) return rc;
    if (bytes != c->h_bytes[slot] && nbytes) std::memcpy(c->h_bytes[slot], bytes, nbytes);
    if (line_off != c->h_off[slot] && n) std::memcpy(c->h_off[slot], line_off, n * 4);
    const SlotCopy v[2] = {{c->d_bytes[slot], c->hd_bytes[slot], c->h_bytes[slot], nbytes},
                           {c->d_off[slot], c->hd_off[slot], c->h_off[slot], n * 4}};
    const ysb_segment sg{c->d_bytes[slot], nbytes, c->d_off[slot], n};
    // the scan instantiation named by the batch's first line, which the host holds in the
    // pinned slot (counts are the same whichever runs)
    Layout lay;
    if (layout_sampling(c) && n)
        lay.layout = hinted_layout(flat_first(c), sniff_layout(require_mask(c), c->h_bytes[slot], nbytes,
                                                               c->h_off[slot], n, &lay.learn));
    return slot_launch(c, slot, v, 2, [&] { return enqueue_scan(c, &sg, 1, lay); });
}

int ysb_wait(ysb_ctx* c, int slot) {
    if (!c) return YSB_ERR_ARG;
    if (const int rc = slot_arg(c, slot)) return rc;
    if (!c->h_bytes[0]) return YSB_OK;
    HIPCHK(c, hipEventSynchronize(c->ev_h2d[slot]));
    return YSB_OK;
}

int ysb_slot_capacity(ysb_ctx* c, uint64_t* max_bytes, uint64_t* max_events) {
    if (!c) return YSB_ERR_ARG;
    if (max_bytes) *max_bytes = c->cfg.max_batch_bytes;
    if (max_events) *max_events = c->cfg.max_batch_events;
    return YSB_OK;
}

// Device batches: the layout sampled from their lines (unless fixed), then the launch.
static int enqueue_device(ysb_ctx* c, const ysb_segment* segs, u32 nseg) {
    int prc = launch_pending_raw(c);   // batches launch in submission order
    if (prc) return prc;
    Layout lay;
    if (c->table_loaded && layout_sampling(c)) {
        const int rc = sample_device_layout(c, segs, nseg, &lay);
        if (rc) return rc;
        lay.layout = hinted_layout(flat_first(c), lay.layout);
    }
    return enqueue_scan(c, segs, nseg, lay);
}

int ysb_submit_device(ysb_ctx* c, const uint8_t* d_bytes, uint64_t nbytes, const uint32_t* d_off, uint64_t n) {
    if (!c) return YSB_ERR_ARG;
    if (nbytes > (4ull << 30) - 64) return fail(c, YSB_ERR_CAPACITY, "device batch larger than 4 GiB (u32 offsets)");
    if ((nbytes && !d_bytes) || (n && !d_off)) return fail(c, YSB_ERR_ARG, "NULL batch buffers");
    if (reinterpret_cast<uintptr_t>(d_bytes) & 15) return fail(c, YSB_ERR_ARG, "d_bytes must be 16-byte aligned");
    if (int g = carry_guard(c)) return g;
    HIPCHK(c, hipSetDevice(c->device));
    const ysb_segment sg{d_bytes, nbytes, d_off, n};
    return enqueue_device(c, &sg, 1);
}

int ysb_submit_device_segments(ysb_ctx* c, const ysb_segment* segs, uint32_t n_segs) {
    if (!c) return YSB_ERR_ARG;
    if (n_segs > (u32)MAX_SEGS) return fail(c, YSB_ERR_CAPACITY, "at most %d segments per launch", MAX_SEGS);
    if (n_segs && !segs) return fail(c, YSB_ERR_ARG, "NULL segment list");
    for (u32 i = 0; i < n_segs; ++i) {
        const ysb_segment& s = segs[i];
        if (s.nbytes > (4ull << 30) - 64)
            return fail(c, YSB_ERR_CAPACITY, "segment %u larger than 4 GiB (u32 offsets)", i);
        if ((s.nbytes && !s.d_bytes) || (s.n_events && !s.d_line_off))
            return fail(c, YSB_ERR_ARG, "NULL buffers in segment %u", i);
        if (reinterpret_cast<uintptr_t>(s.d_bytes) & 15)
            return fail(c, YSB_ERR_ARG, "segment %u: d_bytes must be 16-byte aligned", i);
    }
    if (int g = carry_guard(c)) return g;
    HIPCHK(c, hipSetDevice(c->device));
    return enqueue_device(c, segs, n_segs);
}

int ysb_layout_of_line(const uint8_t* line, uint64_t len, int require_ip, uint32_t order[8], uint32_t* n,
                       uint32_t* compact) {
    if (!line && len) return YSB_ERR_ARG;
    LearnDesc d{};
    const int l = learn_layout(line, len, require_ip ? 0x7Fu : 0x3Fu, &d);
    if (order) for (int i = 0; i < 8; ++i) order[i] = d.order[i];
    if (n) *n = l == 3 ? d.n : 0;
    if (compact) *compact = l == 3 ? d.cp : (l == 1 ? 1u : 0u);
    return l;
}

}  // extern "C"
