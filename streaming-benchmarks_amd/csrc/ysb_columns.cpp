// ysb_columns.cpp -- the columnar decode of the C ABI (include/ysb_hip.h, "columnar decode"):
// the fork's WindowedArrowFormatBolter layout (AdvertisingTopologyNative.java:278-356) and
// the launch of columns_kernel (ysb_scan_columns.h) for one device batch.
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

}  // extern "C"
