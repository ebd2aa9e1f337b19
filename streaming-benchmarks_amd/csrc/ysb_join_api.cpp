// ysb_join_api.cpp -- the joined-views calls of the C ABI (include/ysb_hip.h, "joined views"):
// the output layout and the three launches of Kernel 7 (ysb_scan_join.h; the layout, the scratch
// format and the plan: ysb_join.h) for one device batch.
#include "ysb_ctx.h"
#include "ysb_join.h"

static_assert(YSB_JOIN_KEYS == JOIN_KEYS, "the flag as the kernels read it");

extern "C" {

int ysb_joined_layout_of(uint64_t cap_rows, uint32_t flags, ysb_joined_layout* out) {
    u64 start[JC_COUNT_ + 1];
    if (!out || !join_layout(cap_rows, flags, start)) return YSB_ERR_ARG;
    out->cap_rows = cap_rows;
    for (u32 j = 0; j <= (u32)JC_COUNT_; ++j) out->start[j] = start[j];
    for (u32 j = 0; j < (u32)JC_COUNT_; ++j) out->width[j] = j < join_cols(flags) ? join_col_width(j) : 0u;
    out->flags = flags;
    out->n_cols = join_cols(flags);
    return YSB_OK;
}

size_t ysb_join_info_size(void) { return sizeof(ysb_join_info); }

int ysb_join_device(ysb_ctx* c, const uint8_t* d_bytes, uint64_t nbytes, const uint32_t* d_line_off, uint64_t n_events,
                    uint8_t* d_out, uint64_t cap_rows, uint32_t flags, ysb_join_info* info) {
    if (!c) return YSB_ERR_ARG;
    ysb_joined_layout lay;
    if (flags & ~YSB_JOIN_KEYS) return fail(c, YSB_ERR_ARG, "unknown join flags 0x%x", flags);
    if (ysb_joined_layout_of(cap_rows, flags, &lay)) return fail(c, YSB_ERR_ARG, "cap_rows must be at most 2^32 - 1");
    if ((nbytes && !d_bytes) || (n_events && !d_line_off)) return fail(c, YSB_ERR_ARG, "NULL batch buffers");
    if (reinterpret_cast<uintptr_t>(d_bytes) & 15) return fail(c, YSB_ERR_ARG, "d_bytes must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_out) & 15) return fail(c, YSB_ERR_ARG, "d_out must be 16-byte aligned");
    if (cap_rows && !d_out) return fail(c, YSB_ERR_ARG, "NULL d_out for cap_rows > 0");
    if (nbytes > (4ull << 30) - 64) return fail(c, YSB_ERR_CAPACITY, "device batch larger than 4 GiB (u32 offsets)");
    if (n_events > c->cfg.max_batch_events)
        return fail(c, YSB_ERR_CAPACITY, "n_events %llu exceeds max_batch_events %llu", (unsigned long long)n_events,
                    (unsigned long long)c->cfg.max_batch_events);
    if (grouped(c)) return fail(c, YSB_ERR_STATE, "ysb_join_device after ysb_group_init");
    if (!c->table_loaded) return fail(c, YSB_ERR_STATE, "ysb_load_ad_map has not been called");
    HIPCHK(c, hipSetDevice(c->device));
    const int prc = launch_pending_raw(c);   // behind everything submitted
    if (prc) return prc;
    const bool tbl = (c->cfg.flags & YSB_F_FORMAT_TBL) != 0;
    ysb_join_info res{};
    res.events = n_events;
    res.tiles = join_tiles(n_events);
    res.grid = join_grid(res.tiles, c->cus, tbl);
    res.max_grid = join_max_grid(c->cus, tbl);
    if (n_events == 0) {   // legal: nothing is written
        if (info) *info = res;
        return YSB_OK;
    }
    constexpr u64 INFO_BYTES = (ST_COUNT_ + 1) * sizeof(unsigned long long);   // the scan's tallies, then fast rows
    if (!c->d_join_info) {
        for (Event& e : c->ev_join) HIPCHK(c, e.create(hipEventDefault));
        HIPCHK(c, c->d_join_info.alloc(INFO_BYTES));   // (last: it marks the events present)
    }
    int rc = grow_device(c, c->d_join_scratch, join_scratch_bytes(n_events, flags), 1u << 20);
    if (rc) return rc;
    JoinParams p{};
    context_params(c, &p.sp);
    p.sp.stats = c->d_join_info;   // the call's own tallies: ysb_stats is left alone
    p.sp.used_out = nullptr;
    p.b.bytes = d_bytes;
    p.b.nbytes = nbytes;
    p.b.off = d_line_off;
    p.b.n = n_events;
    p.b.n_tiles = res.tiles;
    p.b.out = d_out;
    for (u32 j = 0; j < (u32)JC_COUNT_; ++j) p.b.start[j] = lay.start[j];
    p.b.tbl = tbl ? 1u : 0u;
    p.b.require_mask = p.sp.require_mask;
    p.scratch = c->d_join_scratch;
    p.tile_count = reinterpret_cast<u32*>(c->d_join_scratch.get() + join_scratch_counts(n_events, flags));
    p.prefix = p.tile_count + res.tiles;
    p.cap_rows = cap_rows;
    p.keys = (flags & YSB_JOIN_KEYS) ? 1u : 0u;
    HIPCHK(c, hipMemsetAsync(c->d_join_info, 0, INFO_BYTES, c->s_comp));
    HIPCHK(c, hipEventRecord(c->ev_join[0], c->s_comp));
    launch_join(p, c->cus, c->s_comp);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev_join[1], c->s_comp));
    launch_join_prefix(p, c->s_comp);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev_join[2], c->s_comp));
    launch_join_pack(p, c->cus, c->s_comp);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev_join[3], c->s_comp));
    unsigned long long got[ST_COUNT_ + 1] = {};
    HIPCHK(c, hipMemcpyAsync(got, c->d_join_info, INFO_BYTES, hipMemcpyDeviceToHost, c->s_comp));
    HIPCHK(c, hipStreamSynchronize(c->s_comp));
    float ms[3] = {0, 0, 0};
    for (int k = 0; k < 3; ++k) HIPCHK(c, hipEventElapsedTime(&ms[k], c->ev_join[k], c->ev_join[k + 1]));
    res.events = got[ST_EVENTS];
    res.views = got[ST_VIEWS];
    res.joined = got[ST_JOINED];
    res.join_misses = got[ST_MISSES];
    res.parse_errors = got[ST_PARSE_ERR];
    res.time_errors = got[ST_TIME_ERR];
    res.foreign_shard = got[ST_FOREIGN];
    res.rows_written = std::min<u64>(res.joined, cap_rows);
    res.fast_rows = got[ST_COUNT_];
    res.join_ms = ms[0];
    res.prefix_ms = ms[1];
    res.pack_ms = ms[2];
    if (info) *info = res;
    if (res.joined > cap_rows)
        return fail(c, YSB_ERR_CAPACITY, "%llu joined views do not fit cap_rows %llu: the first %llu were written",
                    (unsigned long long)res.joined, (unsigned long long)cap_rows, (unsigned long long)cap_rows);
    return YSB_OK;
}

}  // extern "C"
