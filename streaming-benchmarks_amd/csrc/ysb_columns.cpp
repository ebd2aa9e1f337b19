// ysb_columns.cpp -- the columnar calls of the C ABI (include/ysb_hip.h, "columnar decode" and
// "columnar count"): the fork's WindowedArrowFormatBolter layout (AdvertisingTopologyNative.java:
// 278-356), the launch of columns_kernel (ysb_scan_columns.h) for one device batch, and the
// submits that count a batch in that layout (colcount_kernel, ysb_count_columns.h) from HBM or
// through the pinned slots.
#include "ysb_ctx.h"

namespace {

constexpr u64 COL_PAGE_BYTES = 4096;                       // page_align (:291-302)
constexpr u32 COL_WIDTH[7] = {36, 36, 36, 4, 4, 8, 8};     // entry_len (:284)

u64 page_align(u64 b) { return (b + COL_PAGE_BYTES - 1) / COL_PAGE_BYTES * COL_PAGE_BYTES; }

}  // namespace

extern "C" {

int ysb_columns_layout_of(uint64_t batch_rows, ysb_columns_layout* out) {
    if (!out || batch_rows == 0 || batch_rows > 0x7FFFFFFFull) return YSB_ERR_ARG;
    out->rows = batch_rows;
    u64 at = 0;
    for (int j = 0; j < 7; ++j) {
        out->width[j] = COL_WIDTH[j];
        out->start[j] = at;
        at += page_align((u64)COL_WIDTH[j] * batch_rows);
    }
    out->reserved = 0;
    out->image_bytes = at;
    out->start[7] = at;
    out->start[8] = at + page_align((batch_rows + 63) / 64 * 8);
    return YSB_OK;
}

int ysb_decode_columns_device(ysb_ctx* c, const uint8_t* d_bytes, uint64_t nbytes, const uint32_t* d_line_off,
                              uint64_t n_events, uint8_t* d_out, uint64_t batch_rows, int64_t stamp, uint32_t flags,
                              ysb_decode_info* info) {
    if (!c) return YSB_ERR_ARG;
    ysb_columns_layout lay;
    if (ysb_columns_layout_of(batch_rows, &lay)) return fail(c, YSB_ERR_ARG, "batch_rows must be in [1, 2^31 - 1]");
    if (flags & ~YSB_COL_JAVA_ORDER) return fail(c, YSB_ERR_ARG, "unknown decode flags 0x%x", flags);
    if (!d_out) return fail(c, YSB_ERR_ARG, "NULL output buffer");
    if ((nbytes && !d_bytes) || (n_events && !d_line_off)) return fail(c, YSB_ERR_ARG, "NULL batch buffers");
    if ((reinterpret_cast<uintptr_t>(d_bytes) & 15) || (reinterpret_cast<uintptr_t>(d_out) & 15))
        return fail(c, YSB_ERR_ARG, "d_bytes and d_out must be 16-byte aligned");
    if (nbytes > (4ull << 30) - 64) return fail(c, YSB_ERR_CAPACITY, "device batch larger than 4 GiB (u32 offsets)");
    if (n_events > batch_rows)
        return fail(c, YSB_ERR_CAPACITY, "%llu events do not fit %llu rows", (unsigned long long)n_events,
                    (unsigned long long)batch_rows);
    HIPCHK(c, hipSetDevice(c->device));
    const int prc = launch_pending_raw(c);   // behind everything submitted
    if (prc) return prc;
    if (!c->d_colinfo) {
        for (Event& e : c->ev_col) HIPCHK(c, e.create(hipEventDefault));
        HIPCHK(c, c->d_colinfo.alloc(2 * sizeof(unsigned long long)));   // (last: it marks the events present)
    }
    ColParams p{};
    p.bytes = d_bytes;
    p.nbytes = nbytes;
    p.off = d_line_off;
    p.n = n_events;
    p.n_tiles = (n_events + TILE_LINES - 1) / TILE_LINES;
    p.out = d_out;
    for (int j = 0; j < 8; ++j) p.start[j] = lay.start[j];
    p.stamp = stamp;
    p.java_order = (flags & YSB_COL_JAVA_ORDER) ? 1u : 0u;
    p.tbl = (c->cfg.flags & YSB_F_FORMAT_TBL) ? 1u : 0u;
    p.require_mask = (c->cfg.flags & YSB_F_REQUIRE_IP) ? 0x7Fu : 0x3Fu;
    p.info = c->d_colinfo;
    HIPCHK(c, hipMemsetAsync(c->d_colinfo, 0, 2 * sizeof(unsigned long long), c->s_comp));
    HIPCHK(c, hipEventRecord(c->ev_col[0], c->s_comp));
    launch_columns(p, c->cus, c->s_comp);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev_col[1], c->s_comp));
    unsigned long long got[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(got, c->d_colinfo, sizeof(got), hipMemcpyDeviceToHost, c->s_comp));
    HIPCHK(c, hipStreamSynchronize(c->s_comp));
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev_col[0], c->ev_col[1]));
    if (info) {
        info->rows = n_events;
        info->valid = got[0];
        info->fast_rows = got[1];
        info->kernel_ms = ms;
    }
    return YSB_OK;
}

// ---- columnar count (Kernel 5, ysb_count_columns.h) ------------------------------------------

int ysb_columns_read_ranges(uint64_t batch_rows, uint64_t n_rows, uint32_t flags, uint64_t offset[4],
                            uint64_t bytes[4], uint32_t* n) {
    ysb_columns_layout lay;
    if (!offset || !bytes || !n || (flags & ~(YSB_COL_JAVA_ORDER | YSB_COL_VALIDITY)) ||
        ysb_columns_layout_of(batch_rows, &lay))
        return YSB_ERR_ARG;
    if (n_rows > batch_rows) return YSB_ERR_CAPACITY;
    const int col[3] = {2, 4, 5};   // ad_id, event_type, event_time
    for (int i = 0; i < 3; ++i) {
        offset[i] = lay.start[col[i]];
        bytes[i] = n_rows * COL_WIDTH[col[i]];
    }
    *n = 3;
    if (flags & YSB_COL_VALIDITY) {
        offset[3] = lay.start[7];
        bytes[3] = (n_rows + 63) / 64 * 8;
        *n = 4;
    }
    return YSB_OK;
}

// The arguments every columnar submit checks; *total <- the buffer's size.
static int colcount_args(ysb_ctx* c, const uint8_t* cols, u64 batch_rows, u64 n_rows, u32 flags,
                         ysb_columns_layout* lay, u64* total) {
    if (ysb_columns_layout_of(batch_rows, lay)) return fail(c, YSB_ERR_ARG, "batch_rows must be in [1, 2^31 - 1]");
    if (flags & ~(YSB_COL_JAVA_ORDER | YSB_COL_VALIDITY)) return fail(c, YSB_ERR_ARG, "unknown columnar flags 0x%x", flags);
    if (!cols) return fail(c, YSB_ERR_ARG, "NULL column batch");
    if (n_rows > batch_rows)
        return fail(c, YSB_ERR_CAPACITY, "%llu rows do not fit a batch of %llu rows", (unsigned long long)n_rows,
                    (unsigned long long)batch_rows);
    if (!c->table_loaded) return fail(c, YSB_ERR_STATE, "ysb_load_ad_map has not been called");
    *total = (flags & YSB_COL_VALIDITY) ? lay->start[8] : lay->image_bytes;
    return YSB_OK;
}

// One columnar launch on the compute stream: the ring's auto-base if it is not known yet, the
// count kernel, the out-of-ring map's fill level for the host.
static int enqueue_colcount(ysb_ctx* c, const u8* d_cols, const ysb_columns_layout& lay, u64 n_rows, u32 flags) {
    if (n_rows == 0) { c->batches++; return YSB_OK; }
    Launch L;
    int rc = launch_begin(c, &L);
    if (rc) return rc;
    ColCountParams p{};
    context_params(c, &p.sp);
    p.sp.used_out = L.used_out;
    p.cols = d_cols;
    for (int j = 0; j < 8; ++j) p.start[j] = lay.start[j];
    p.n_rows = n_rows;
    p.n_tiles = (n_rows + TILE_LINES - 1) / TILE_LINES;
    p.java_order = (flags & YSB_COL_JAVA_ORDER) ? 1u : 0u;
    p.validity = (flags & YSB_COL_VALIDITY) ? 1u : 0u;
    if (L.base_ring) {
        launch_colcount_autobase(p, c->s_comp);
        if ((rc = launch_ring_based(c))) return rc;
    }
    if ((rc = launch_mark(c, &L, 0))) return rc;
    ParkParams park;
    launch_colcount(p, c->cus, c->s_comp, park_params(c, &park) ? &park : nullptr);
    HIPCHK(c, hipGetLastError());
    if ((rc = launch_mark(c, &L, 1))) return rc;
    launch_used_level(p.sp, c->s_comp);   // the map's fill level into h_used (sp.used_out)
    HIPCHK(c, hipGetLastError());
    c->last_col.rows = n_rows;
    c->last_col.lds_counters = p.sp.lds_wl ? 1u : 0u;
    c->last_col.hbm_table = p.sp.probe_serial ? 1u : 0u;
    c->last_col.java_order = p.java_order;
    c->last_col.validity = p.validity;
    c->col_launched = true;
    return launch_end(c, &L, true, 1);
}

int ysb_submit_columns_device(ysb_ctx* c, const uint8_t* d_cols, uint64_t batch_rows, uint64_t n_rows, uint32_t flags) {
    if (!c) return YSB_ERR_ARG;
    if (int g = carry_guard(c)) return g;
    ysb_columns_layout lay;
    u64 total = 0;
    if (reinterpret_cast<uintptr_t>(d_cols) & 15) return fail(c, YSB_ERR_ARG, "d_cols must be 16-byte aligned");
    int rc = colcount_args(c, d_cols, batch_rows, n_rows, flags, &lay, &total);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = launch_pending_raw(c))) return rc;   // batches launch in submission order
    return enqueue_colcount(c, d_cols, lay, n_rows, flags);
}

int ysb_submit_columns(ysb_ctx* c, int slot, const uint8_t* image, uint64_t batch_rows, uint64_t n_rows,
                       uint32_t flags) {
    if (!c) return YSB_ERR_ARG;
    if (int rc = slot_arg(c, slot)) return rc;
    if (int g = carry_guard(c)) return g;
    ysb_columns_layout lay;
    u64 total = 0;
    int rc = colcount_args(c, image, batch_rows, n_rows, flags, &lay, &total);
    if (rc) return rc;
    if (total > c->cfg.max_batch_bytes)
        return fail(c, YSB_ERR_CAPACITY, "column batch of %llu B exceeds max_batch_bytes", (unsigned long long)total);
    if ((rc = slot_begin(c, slot))) return rc;
    u64 off[4], len[4];
    u32 nr = 0;
    if ((rc = ysb_columns_read_ranges(batch_rows, n_rows, flags, off, len, &nr))) return fail(c, rc, "bad column ranges");
    SlotCopy v[4];
    for (u32 i = 0; i < nr; ++i) {
        if (image != c->h_bytes[slot] && len[i]) std::memcpy(c->h_bytes[slot] + off[i], image + off[i], len[i]);
        v[i] = {c->d_bytes[slot] + off[i], c->hd_bytes[slot] + off[i], c->h_bytes[slot] + off[i], len[i]};
    }
    return slot_launch(c, slot, v, (int)nr, [&] { return enqueue_colcount(c, c->d_bytes[slot], lay, n_rows, flags); });
}

int ysb_columns_launch_info(ysb_ctx* c, ysb_colcount_desc* out) {
    if (!c || !out) return c ? fail(c, YSB_ERR_ARG, "NULL output") : YSB_ERR_ARG;
    if (!c->col_launched) return fail(c, YSB_ERR_STATE, "no columnar launch yet");
    *out = c->last_col;
    return YSB_OK;
}

uint64_t ysb_colcount_desc_size(void) { return sizeof(ysb_colcount_desc); }

}  // extern "C"
