// ysb_parked_api.cpp -- parked views over the C ABI: ysb_parked_enable / _keys / _resolve /
// _info (include/ysb_hip.h).  The record format and rules are ysb_parked.h's, the kernels
// ysb_parked.hip's; the park sites run inside the launches (ysb_submit.cpp, ysb_columns.cpp),
// which ask park_params for the log.
#include "ysb_ctx.h"

using namespace ysb;

extern "C" {

bool park_params(const ysb_ctx* c, ParkParams* out) {
    if (!c->park_cap) return false;
    *out = ParkParams{c->d_park_log, (u32)c->park_cap, c->d_park_ctr};
    return true;
}

int park_counters(ysb_ctx* c) {
    HIPCHK(c, hipMemcpyAsync(c->h_park_ctr, c->d_park_ctr, PK_COUNT_ * 4, hipMemcpyDeviceToHost, c->s_comp));
    HIPCHK(c, hipStreamSynchronize(c->s_comp));
    return YSB_OK;
}

static u64 ctr64(const u32* k, u32 at) { return ((u64)k[at + 1] << 32) | k[at]; }
static u64 parked_now(const ysb_ctx* c) { return std::min<u64>(c->h_park_ctr[PK_CLAIMED], c->park_cap); }

// The counters as no record parked and nothing resolved; dropped is kept unless `all`.
static int park_clear(ysb_ctx* c, bool all) {
    u32 k[PK_COUNT_] = {};
    const i64 none = INT64_MAX;
    std::memcpy(&k[PK_MINB], &none, 8);
    HIPCHK(c, hipMemcpyAsync(c->d_park_ctr, k, (all ? (u32)PK_COUNT_ : (u32)PK_DROPPED) * 4, hipMemcpyHostToDevice, c->s_comp));
    HIPCHK(c, hipStreamSynchronize(c->s_comp));   // (k is on this stack)
    return YSB_OK;
}

int park_reset(ysb_ctx* c) {
    c->park_resolved_total = 0;
    const u64 cap = c->park_cap;
    c->park_last = ysb_parked_desc{};
    c->park_last.capacity = cap;
    return cap ? park_clear(c, true) : YSB_OK;
}

static void fill_info(const ysb_ctx* c, ysb_parked_desc* out) {
    *out = c->park_last;
    out->capacity = c->park_cap;
    if (!c->park_cap) return;
    out->parked = parked_now(c);
    out->parked_total = c->park_resolved_total + out->parked;
    out->dropped = ctr64(c->h_park_ctr, PK_DROPPED);
}

int ysb_parked_enable(ysb_ctx* c, uint64_t capacity) {
    if (!c) return YSB_ERR_ARG;
    if (!c->table_loaded) return fail(c, YSB_ERR_STATE, "ysb_load_ad_map has not been called");
    if (grouped(c)) return fail(c, YSB_ERR_STATE, "parked views are not available after ysb_group_init");
    if (capacity >= (1ull << 30)) return fail(c, YSB_ERR_CAPACITY, "at most 2^30-1 parked records");
    int rc = sync_streams(c);   // (launches a raw batch awaiting its launch: it runs under the old setting)
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->park_cap) {
        if ((rc = park_counters(c))) return rc;
        if (parked_now(c)) return fail(c, YSB_ERR_STATE, "%llu views are parked: ysb_parked_resolve first", (unsigned long long)parked_now(c));
    }
    if (capacity == c->park_cap) return YSB_OK;
    c->park_cap = 0;
    for (DevMem* m : {static_cast<DevMem*>(&c->d_park_log), static_cast<DevMem*>(&c->d_park_slots),
                      static_cast<DevMem*>(&c->d_park_lens), static_cast<DevMem*>(&c->d_park_camp),
                      static_cast<DevMem*>(&c->d_park_keys)})
        m->reset();
    c->park_last = ysb_parked_desc{};
    c->park_resolved_total = 0;
    if (!capacity) return YSB_OK;
    const u64 slots = park_distinct_slots(capacity);
    HIPCHK(c, c->d_park_log.alloc(capacity * PARK_WORDS * 4));
    HIPCHK(c, c->d_park_slots.alloc(slots * 4));
    HIPCHK(c, c->d_park_lens.alloc(capacity * 4));
    HIPCHK(c, c->d_park_camp.alloc(capacity * 4));
    HIPCHK(c, c->d_park_keys.alloc(capacity * PARK_KEY_STRIDE));
    if (!c->d_park_ctr) HIPCHK(c, c->d_park_ctr.alloc(PK_COUNT_ * 4));
    if (!c->h_park_ctr) HIPCHK(c, c->h_park_ctr.alloc(PK_COUNT_ * 4));
    for (Event& e : c->ev_park)
        if (!e.h) HIPCHK(c, e.create(hipEventDefault));
    c->park_slots = slots;
    c->park_cap = capacity;
    if ((rc = park_clear(c, true)) || (rc = park_counters(c))) {
        c->park_cap = 0;
        return rc;
    }
    return YSB_OK;
}

// Everything submitted done, the counters read: what every call on the log starts with.
static int park_begin(ysb_ctx* c) {
    if (!c->park_cap) return fail(c, YSB_ERR_STATE, "parking is not enabled (ysb_parked_enable)");
    int rc = sync_streams(c);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    return park_counters(c);
}

int ysb_parked_keys(ysb_ctx* c, char* keys, uint32_t* lens, uint64_t cap, uint64_t* n_out) {
    if (!c || !n_out) return c ? fail(c, YSB_ERR_ARG, "NULL count") : YSB_ERR_ARG;
    if (keys && !lens) return fail(c, YSB_ERR_ARG, "NULL lens");
    int rc = park_begin(c);
    if (rc) return rc;
    const u32 n = (u32)parked_now(c);
    u64 distinct = 0;
    float ms = 0;
    if (n) {
        ParkParams k;
        park_params(c, &k);
        HIPCHK(c, hipMemsetAsync(c->d_park_slots, 0xFF, c->park_slots * 4, c->s_comp));
        HIPCHK(c, hipMemsetAsync(c->d_park_ctr + PK_DISTINCT, 0, 4, c->s_comp));
        HIPCHK(c, hipEventRecord(c->ev_park[0], c->s_comp));
        launch_parked_distinct(k, n, c->d_park_slots, (u32)(c->park_slots - 1), c->d_park_keys, c->d_park_lens, c->s_comp);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(c->ev_park[1], c->s_comp));
        if ((rc = park_counters(c))) return rc;
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev_park[0], c->ev_park[1]));
        distinct = c->h_park_ctr[PK_DISTINCT];
    }
    c->park_last.distinct_keys = distinct;
    c->park_last.distinct_ms = ms;
    *n_out = distinct;
    if (!keys) return YSB_OK;
    if (cap < distinct)
        return fail(c, YSB_ERR_CAPACITY, "%llu distinct parked keys, room for %llu", (unsigned long long)distinct,
                    (unsigned long long)cap);
    if (distinct) {
        HIPCHK(c, hipMemcpy(keys, c->d_park_keys, distinct * PARK_KEY_STRIDE, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(lens, c->d_park_lens, distinct * 4, hipMemcpyDeviceToHost));
    }
    return YSB_OK;
}

int ysb_parked_resolve(ysb_ctx* c, ysb_parked_desc* info) {
    if (!c) return YSB_ERR_ARG;
    int rc = park_begin(c);
    if (rc) return rc;
    const u32 n = (u32)parked_now(c);
    float ms = 0;
    c->park_last.resolved_joined = c->park_last.resolved_missed = c->park_last.resolved_time_errors = 0;
    if (n) {
        if ((rc = drain_side_if_due(c))) return rc;
        if ((rc = park_clear(c, false))) return rc;   // the log is taken: nothing parked, this resolve's tallies zero
        ParkParams k;
        park_params(c, &k);
        ScanParams sp;
        context_params(c, &sp);
        HIPCHK(c, hipEventRecord(c->ev_park[0], c->s_comp));
        launch_parked_resolve(sp, k, n, c->d_park_camp, c->s_comp);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(c->ev_park[1], c->s_comp));
        c->pend_u64 = true;   // the resolve counts into the u64 ring
        if ((rc = park_counters(c))) return rc;
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev_park[0], c->ev_park[1]));
        const u32* h = c->h_park_ctr;
        c->park_last.resolved_joined = h[PK_JOINED];
        c->park_last.resolved_missed = h[PK_MISSED];
        c->park_last.resolved_time_errors = h[PK_TIME_ERR];
        c->park_resolved_total += n;
        if (!c->ring_known && (rc = read_ring(c))) return rc;   // this resolve may have based the ring
    }
    c->park_last.resolve_ms = ms;
    if (info) fill_info(c, info);
    return YSB_OK;
}

int ysb_parked_info(ysb_ctx* c, ysb_parked_desc* info) {
    if (!c || !info) return c ? fail(c, YSB_ERR_ARG, "NULL info") : YSB_ERR_ARG;
    if (c->park_cap) {
        const int rc = park_begin(c);
        if (rc) return rc;
    }
    fill_info(c, info);
    return YSB_OK;
}

uint64_t ysb_parked_info_size(void) { return sizeof(ysb_parked_desc); }

}  // extern "C"
