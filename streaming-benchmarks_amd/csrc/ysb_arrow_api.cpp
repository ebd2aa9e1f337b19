// ysb_arrow_api.cpp -- the Arrow calls of the C ABI (include/ysb_hip.h, "Arrow record
// batches"): the schema binding and the host model (ysb_arrow.h, no context), and the submits
// that count a record batch (arrowcount_kernel, ysb_count_arrow.h) from HBM or through the
// pinned slots.
#include "ysb_ctx.h"
#include "ysb_arrow.h"

namespace {

// The arguments of a batch as the kernel takes them, checked.
int arrow_params(ysb_ctx* c, const ysb_arrow_cols& A, ArrowCountParams* p) {
    if (A.n_rows > AR_MAX_ROWS) return fail(c, YSB_ERR_ARG, "more than 2^31 - 1 rows");
    const ysb_arrow_col* col[4] = {&A.col[0], &A.col[1], &A.col[2], &A.dict};
    static const char* const NAME[4] = {"ad_id", "event_type", "event_time", "event_type's dictionary"};
    const u32 k0 = A.col[0].kind, k1 = A.col[1].kind, k2 = A.col[2].kind;
    if (k0 != YSB_ARROW_STRING || (k1 != YSB_ARROW_STRING && k1 != YSB_ARROW_DICT) ||
        (k2 != YSB_ARROW_STRING && k2 != YSB_ARROW_INT64))
        return fail(c, YSB_ERR_ARG, "column kinds %u, %u, %u: ad_id is a string, event_type a string or a dictionary, "
                                    "event_time a string or int64", k0, k1, k2);
    p->n_rows = A.n_rows;
    p->n_tiles = (A.n_rows + TILE_LINES - 1) / TILE_LINES;
    p->sval = A.validity;
    p->sval_off = A.offset;
    p->type_dict = k1 == YSB_ARROW_DICT;
    p->time_i64 = k2 == YSB_ARROW_INT64;
    p->dict_len = 0;
    if (p->type_dict) {
        if (A.dict_len > AR_MAX_DICT) return fail(c, YSB_ERR_CAPACITY, "a dictionary of %llu values (at most 2^30 - 2)", (unsigned long long)A.dict_len);
        if (A.dict.kind != YSB_ARROW_STRING) return fail(c, YSB_ERR_ARG, "the dictionary's values must be strings");
        p->dict_len = (u32)A.dict_len;
    }
    for (int k = 0; k < 4; ++k) {
        const ysb_arrow_col& s = *col[k];
        const bool used = k < 3 || p->type_dict;
        const u64 n = !used ? 0 : k < 3 ? A.n_rows : A.dict_len;
        p->val[k] = used ? s.validity : nullptr;
        p->val_off[k] = s.validity_offset;
        p->offs[k] = nullptr;
        p->data[k] = nullptr;
        p->elem[k] = s.offset;
        p->first[k] = p->end[k] = 0;
        if (!n) continue;
        if (s.offset + n > AR_MAX_ROWS + 1 || s.validity_offset + n > (1ull << 40))
            return fail(c, YSB_ERR_ARG, "%s: element offset too large", NAME[k]);
        if (s.kind == YSB_ARROW_STRING) {
            if (!s.offsets) return fail(c, YSB_ERR_ARG, "%s: NULL offsets buffer", NAME[k]);
            if (s.data_first > s.data_bytes || s.data_bytes > AR_MAX_ROWS || s.data_bytes - s.data_first > AR_MAX_DATA)
                return fail(c, YSB_ERR_ARG, "%s: data_first %u, data_bytes %llu (at most 2^31 - 65 bytes)", NAME[k],
                            s.data_first, (unsigned long long)s.data_bytes);
            if (!s.data && s.data_bytes > s.data_first) return fail(c, YSB_ERR_ARG, "%s: NULL data buffer", NAME[k]);
            p->offs[k] = s.offsets;
            p->data[k] = s.data;
            p->first[k] = s.data_first;
            p->end[k] = (u32)s.data_bytes;
        } else {
            const u64 w = s.kind == YSB_ARROW_INT64 ? 8 : 4;
            if (!s.data) return fail(c, YSB_ERR_ARG, "%s: NULL values buffer", NAME[k]);
            if (s.data_bytes < (s.offset + n) * w)
                return fail(c, YSB_ERR_ARG, "%s: %llu bytes of values do not hold elements up to %llu", NAME[k],
                            (unsigned long long)s.data_bytes, (unsigned long long)(s.offset + n));
            p->data[k] = s.data;
        }
    }
    return YSB_OK;
}

// One Arrow launch on the compute stream: the ring's auto-base if it is not known yet, the count
// kernel, the out-of-ring map's fill level for the host.
int enqueue_arrowcount(ysb_ctx* c, ArrowCountParams& p) {
    if (p.n_rows == 0) { c->batches++; return YSB_OK; }
    // the batch's device counters, zero (in front of everything the bracket queues)
    int rc = first_use(c, c->d_arrow_info, 4 * sizeof(unsigned long long));
    if (rc) return rc;
    p.info = c->d_arrow_info;
    HIPCHK(c, hipMemsetAsync(c->d_arrow_info, 0, 4 * sizeof(unsigned long long), c->s_comp));
    Launch L;
    if ((rc = launch_begin(c, &L))) return rc;
    context_params(c, &p.sp);
    p.sp.used_out = L.used_out;
    if (L.base_ring) {
        launch_arrowcount_autobase(p, c->s_comp);
        if ((rc = launch_ring_based(c))) return rc;
    }
    if ((rc = launch_mark(c, &L, 0))) return rc;
    ParkParams park;
    launch_arrowcount(p, c->cus, c->s_comp, park_params(c, &park) ? &park : nullptr);
    HIPCHK(c, hipGetLastError());
    if ((rc = launch_mark(c, &L, 1))) return rc;
    launch_used_level(p.sp, c->s_comp);   // the map's fill level into h_used (sp.used_out)
    HIPCHK(c, hipGetLastError());
    ysb_arrow_desc& d = c->last_arrow;
    d = ysb_arrow_desc{};
    d.rows = p.n_rows;
    d.tiles = p.n_tiles;
    d.resident_grid = arrowcount_resident_grid(c->cus);
    d.grid = (u32)std::min<u64>(p.n_tiles, d.resident_grid);
    d.kind[0] = YSB_ARROW_STRING;
    d.kind[1] = p.type_dict ? YSB_ARROW_DICT : YSB_ARROW_STRING;
    d.kind[2] = p.time_i64 ? YSB_ARROW_INT64 : YSB_ARROW_STRING;
    d.lds_counters = p.sp.lds_wl ? 1u : 0u;
    d.hbm_table = p.sp.probe_serial ? 1u : 0u;
    c->arrow_launched = true;
    return launch_end(c, &L, true, 1);
}

}  // namespace

extern "C" {

int ysb_arrow_bind(const struct ArrowSchema* schema, ysb_arrow_binding* out) {
    std::string err;
    const int rc = arrow_bind(schema, out, &err);
    return rc ? fail(nullptr, rc, "%s", err.c_str()) : YSB_OK;
}

uint64_t ysb_arrow_binding_size(void) { return sizeof(ysb_arrow_binding); }
uint64_t ysb_arrow_cols_size(void) { return sizeof(ysb_arrow_cols); }
uint64_t ysb_arrow_desc_size(void) { return sizeof(ysb_arrow_desc); }

int ysb_arrow_count_host(const ysb_arrow_cols* cols, const uint8_t* keys, const uint32_t* key_off, const uint32_t* campaign,
                         uint64_t n_keys, int64_t divisor, uint32_t shard_rank, uint32_t shard_n, uint64_t stats[8],
                         uint64_t invalid[3], int64_t* cells, uint64_t cap, uint64_t* n_cells) {
    if (!cols || !stats || !invalid || !n_cells || divisor < 1 || (n_keys && (!keys || !key_off || !campaign)))
        return fail(nullptr, YSB_ERR_ARG, "NULL argument or a divisor below 1");
    std::map<std::string, u32> map;
    for (u64 i = 0; i < n_keys; ++i)
        map[std::string(reinterpret_cast<const char*>(keys) + key_off[i], key_off[i + 1] - key_off[i])] = campaign[i];
    ArrowCounts r;
    arrow_count_rows(*cols, divisor, shard_rank, shard_n ? shard_n : 1u, [&](const u8* k, u32 n) {
        const auto it = map.find(std::string(reinterpret_cast<const char*>(k), n));
        return it == map.end() ? (u32)EMPTY_SLOT : it->second;
    }, &r);
    const u64 st[8] = {r.events, r.views, r.joined, r.misses, r.parse_errors, r.time_errors, r.foreign, 0};
    std::copy(st, st + 8, stats);
    invalid[0] = r.invalid[AR_NULL];
    invalid[1] = r.invalid[AR_OFFSETS];
    invalid[2] = r.invalid[AR_DICT];
    *n_cells = r.cells.size();
    if (r.cells.size() > cap || (r.cells.size() && !cells)) return fail(nullptr, YSB_ERR_CAPACITY, "%llu cells", (unsigned long long)r.cells.size());
    u64 k = 0;
    for (const auto& kv : r.cells) {
        cells[3 * k] = (int64_t)kv.first.first;
        cells[3 * k + 1] = kv.first.second;
        cells[3 * k + 2] = (int64_t)kv.second;
        ++k;
    }
    return YSB_OK;
}

int ysb_arrow_view(const ysb_arrow_binding* binding, const struct ArrowArray* batch, ysb_arrow_cols* out) {
    if (!binding || !out) return fail(nullptr, YSB_ERR_ARG, "NULL binding or output");
    std::string err;
    const int rc = arrow_view(*binding, batch, out, &err);
    return rc ? fail(nullptr, rc, "%s", err.c_str()) : YSB_OK;
}

int ysb_arrow_plan(const ysb_arrow_binding* binding, const struct ArrowArray* batch, ysb_arrow_range* ranges, uint64_t cap,
                   uint64_t* n, uint64_t* total) {
    if (!binding || !n || !total) return fail(nullptr, YSB_ERR_ARG, "NULL binding or output");
    ArrowPlan plan;
    std::string err;
    const int rc = arrow_plan(*binding, batch, &plan, &err);
    if (rc) return fail(nullptr, rc, "%s", err.c_str());
    *n = plan.r.size();
    *total = plan.total;
    if (plan.r.size() > cap || (plan.r.size() && !ranges)) return fail(nullptr, YSB_ERR_CAPACITY, "%llu ranges", (unsigned long long)plan.r.size());
    for (size_t i = 0; i < plan.r.size(); ++i) ranges[i] = {plan.r[i].src, plan.r[i].bytes, plan.r[i].dst, plan.r[i].col, plan.r[i].what};
    return YSB_OK;
}

int ysb_arrow_pack(const ysb_arrow_binding* binding, const struct ArrowArray* batch, uint8_t* image, uint64_t cap,
                   ysb_arrow_cols* packed) {
    if (!binding || !packed || (cap && !image)) return fail(nullptr, YSB_ERR_ARG, "NULL binding, image or output");
    ArrowPlan plan;
    std::string err;
    const int rc = arrow_plan(*binding, batch, &plan, &err);
    if (rc) return fail(nullptr, rc, "%s", err.c_str());
    if (plan.total > cap) return fail(nullptr, YSB_ERR_CAPACITY, "the packed batch takes %llu B", (unsigned long long)plan.total);
    for (const ArrowRange& q : plan.r) std::memcpy(image + q.dst, q.src, q.bytes);
    *packed = arrow_plan_cols(plan, image);
    return YSB_OK;
}

int ysb_submit_arrow_device(ysb_ctx* c, const ysb_arrow_cols* cols) {
    if (!c) return YSB_ERR_ARG;
    if (int g = carry_guard(c)) return g;
    if (!cols) return fail(c, YSB_ERR_ARG, "NULL columns");
    if (!c->table_loaded) return fail(c, YSB_ERR_STATE, "ysb_load_ad_map has not been called");
    ArrowCountParams p{};
    int rc = arrow_params(c, *cols, &p);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = launch_pending_raw(c))) return rc;   // batches launch in submission order
    return enqueue_arrowcount(c, p);
}

int ysb_submit_arrow(ysb_ctx* c, int slot, const ysb_arrow_binding* binding, const struct ArrowArray* batch) {
    if (!c) return YSB_ERR_ARG;
    if (int rc = slot_arg(c, slot)) return rc;
    if (int g = carry_guard(c)) return g;
    if (!binding) return fail(c, YSB_ERR_ARG, "NULL binding");
    if (!c->table_loaded) return fail(c, YSB_ERR_STATE, "ysb_load_ad_map has not been called");
    ArrowPlan plan;
    std::string err;
    int rc = arrow_plan(*binding, batch, &plan, &err);
    if (rc) return fail(c, rc, "%s", err.c_str());
    if (plan.total > c->cfg.max_batch_bytes)
        return fail(c, YSB_ERR_CAPACITY, "Arrow batch of %llu B (the rows' bytes) exceeds max_batch_bytes", (unsigned long long)plan.total);
    if ((rc = slot_begin(c, slot))) return rc;
    ArrowCountParams p{};   // (checked before anything is copied)
    if ((rc = arrow_params(c, arrow_plan_cols(plan, c->h_bytes[slot]), &p))) return rc;
    for (const ArrowRange& q : plan.r) std::memcpy(c->h_bytes[slot] + q.dst, q.src, q.bytes);
    // one copy: the ranges are packed back to back (16-byte boundaries)
    SlotCopy v{c->d_bytes[slot], c->hd_bytes[slot], c->h_bytes[slot], plan.total};
    return slot_launch(c, slot, &v, 1, [&] {
        p = ArrowCountParams{};
        const int re = arrow_params(c, arrow_plan_cols(plan, c->d_bytes[slot]), &p);
        return re ? re : enqueue_arrowcount(c, p);
    });
}

int ysb_arrow_launch_info(ysb_ctx* c, ysb_arrow_desc* out) {
    if (!c || !out) return c ? fail(c, YSB_ERR_ARG, "NULL output") : YSB_ERR_ARG;
    if (!c->table_loaded) return fail(c, YSB_ERR_STATE, "ysb_load_ad_map has not been called");
    if (!c->arrow_launched) return fail(c, YSB_ERR_STATE, "no Arrow launch yet");
    HIPCHK(c, hipSetDevice(c->device));
    unsigned long long info[4] = {0, 0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(info, c->d_arrow_info, sizeof(info), hipMemcpyDeviceToHost, c->s_comp));
    HIPCHK(c, hipStreamSynchronize(c->s_comp));
    c->last_arrow.per_lane_tiles = info[0];
    c->last_arrow.invalid_null = info[1];
    c->last_arrow.invalid_offsets = info[2];
    c->last_arrow.invalid_dict = info[3];
    *out = c->last_arrow;
    return YSB_OK;
}

}  // extern "C"
