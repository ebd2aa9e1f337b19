// ysb_capi.cpp -- the C ABI of include/ysb_hip.h: context lifecycle, the device ad ->
// campaign tables, sync / drain / ring / stats, measurement getters and device memory helpers.
// Batches are in ysb_submit.cpp, the multi-GPU group in ysb_group.cpp, the generator in
// ysb_gen_api.cpp (all over the context of ysb_ctx.h).
#include "ysb_ctx.h"

#include <unistd.h>

#include <cctype>

using namespace ysb;

thread_local std::string g_open_err;

int fail(ysb_ctx* c, int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    else g_open_err = buf;
    return code;
}

int grow_device(ysb_ctx* c, DevMem& buf, u64 bytes, u64 floor_bytes) {
    if (buf.bytes() >= bytes) return YSB_OK;
    for (hipStream_t s : {c->s_comp, c->s_copy, c->s_split, c->s_x})   // nothing queued may still use the old one
        if (s) HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, buf.alloc(std::max(bytes, floor_bytes)));
    return YSB_OK;
}

int first_use(ysb_ctx* c, DevMem& buf, u64 bytes) {
    if (!buf.h) HIPCHK(c, buf.alloc(bytes));
    return YSB_OK;
}

int regrow_table(ysb_ctx* c, DevBuf<unsigned long long>& t, u64 old_cells, u64 cells) {
    DevBuf<unsigned long long> grown;
    HIPCHK(c, grown.alloc(cells * 8));
    HIPCHK(c, hipMemset(grown, 0, cells * 8));
    if (old_cells) HIPCHK(c, hipMemcpy(grown, t, old_cells * 8, hipMemcpyDeviceToDevice));
    t = std::move(grown);
    return YSB_OK;
}

extern "C" {

int ysb_abi_version(void) { return YSB_ABI_VERSION; }

int ysb_device_count(void) {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

// Why this process's HIP runtime sees no device: the likely cause named (Weak 6 of the round-5
// review: torch 2.10 bundles its own libamdhip64 / libhsa-runtime64, and whichever runtime
// opens the GPU first in a process is the one that sees it).
static int no_device(hipError_t e) {
    const bool kfd = access("/dev/kfd", F_OK) == 0;
    const char* vis = getenv("HIP_VISIBLE_DEVICES");
    if (!vis) vis = getenv("ROCR_VISIBLE_DEVICES");
    if (kfd && !(vis && *vis == '\0'))
        return fail(nullptr, YSB_ERR_HIP,
                    "no HIP device available to this library's HIP runtime (hipGetDeviceCount: %s) although "
                    "/dev/kfd exists: another HIP/HSA runtime in this process (e.g. the libamdhip64 a framework "
                    "such as torch bundles) probably opened the GPU first -- load libysb_hip and call "
                    "ysb_device_count / ysb_open before any other GPU runtime initialises (INTEGRATION.md 1.4a)%s%s",
                    hipGetErrorString(e), vis ? "; *_VISIBLE_DEVICES=" : "", vis ? vis : "");
    return fail(nullptr, YSB_ERR_HIP, "no HIP device available (hipGetDeviceCount: %s%s)", hipGetErrorString(e),
                kfd ? "" : "; no /dev/kfd: no AMD GPU driver in this environment");
}

int ysb_device_numa_node(int device) {
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, sizeof bus, device) != hipSuccess) return -1;
    for (char* p = bus; *p; ++p) *p = (char)std::tolower((unsigned char)*p);
    char path[160];
    std::snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bus);
    FILE* f = std::fopen(path, "r");
    if (!f) return -1;
    int node = -1;
    if (std::fscanf(f, "%d", &node) != 1) node = -1;
    std::fclose(f);
    return node;
}

int ysb_device_sync(int device) {
    int ndev = 0;
    const hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) return no_device(e);
    if (device < 0 || device >= ndev) return fail(nullptr, YSB_ERR_ARG, "device %d out of range (%d)", device, ndev);
    hipError_t r = hipSetDevice(device);
    if (r == hipSuccess) r = hipDeviceSynchronize();
    if (r != hipSuccess) return fail(nullptr, YSB_ERR_HIP, "hipDeviceSynchronize(%d): %s", device, hipGetErrorString(r));
    return YSB_OK;
}

void ysb_config_default(ysb_config* c) {
    std::memset(c, 0, sizeof *c);
    c->time_divisor_ms = 10000;
    c->n_campaigns = 100;
    c->window_ring = 1024;
    c->max_ads = 1000;
    c->max_batch_events = 1u << 20;
    c->max_batch_bytes = 256ull << 20;
    c->ring_base_bucket = INT64_MIN;
    c->overflow_capacity = 1u << 20;
    c->flags = 0;
}

const char* ysb_last_error(const ysb_ctx* c) { return c ? c->err.c_str() : g_open_err.c_str(); }

static void destroy(ysb_ctx* c) {
    if (!c) return;
    hipSetDevice(c->device);
    for (hipStream_t s : {c->s_comp, c->s_copy, c->s_split, c->s_x})
        if (s) hipStreamSynchronize(s);
    if (c->comm) ncclCommDestroy(c->comm);
    for (auto& r : c->host_ranges) hipHostUnregister(reinterpret_cast<void*>(r.first));
    if (c->s_x) hipStreamDestroy(c->s_x);
    if (c->s_split) hipStreamDestroy(c->s_split);
    if (c->s_comp) hipStreamDestroy(c->s_comp);
    if (c->s_copy) hipStreamDestroy(c->s_copy);
    delete c;   // the members release themselves, the device still current
}

// A new context's streams, events and tables on its device; the error code (its text in c->err).
static int init(ysb_ctx* c) {
    const ysb_config& cfg = c->cfg;
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, YSB_ERR_HIP, "hipSetDevice(%d) failed", c->device);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c->device) == hipSuccess && prop.multiProcessorCount > 0) c->cus = prop.multiProcessorCount;
    // scan schedule overrides (timing experiments): YSB_DYN_PCT=0 -> all static
    if (const char* e = getenv("YSB_DYN_PCT")) c->dyn_pct = (u32)strtoul(e, nullptr, 10);
    if (const char* e = getenv("YSB_DELTA_FOLD_EVENTS")) {
        const u64 v = strtoull(e, nullptr, 10);
        if (v > 0 && v < c->delta_limit) c->delta_limit = v;
    }
    if (const char* e = getenv("YSB_DYN_CHUNK")) c->dyn_chunk = (u32)strtoul(e, nullptr, 10);
    if (hipStreamCreateWithFlags(&c->s_comp, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&c->s_copy, hipStreamNonBlocking) != hipSuccess)
        return fail(c, YSB_ERR_HIP, "stream creation failed");
    for (Event* e : {&c->ev_h2d[0], &c->ev_kdone[0], &c->ev_h2d[1], &c->ev_kdone[1], &c->ev_ring, &c->ev_used})
        if (e->create() != hipSuccess) return fail(c, YSB_ERR_HIP, "event creation failed");
    if (c->h_used.alloc(16) != hipSuccess) return fail(c, YSB_ERR_HIP, "event creation failed");   // (the text this pinned word has always failed with)
    const int rc = regrow_table(c, c->d_counts, 0, (u64)c->c_pad * cfg.window_ring);
    if (rc) return rc;
    // out-of-ring map: load <= 1/2 at overflow_capacity distinct cells
    c->side_slots = 64;
    while (c->side_slots < 2 * cfg.overflow_capacity) c->side_slots <<= 1;
    c->side_cbits = 1;
    while (c->side_cbits < 32 && (1ull << c->side_cbits) <= cfg.n_campaigns) ++c->side_cbits;   // bit_width
    // stats and the map's slot count share one allocation: ysb_sync reads both in one copy
    if (c->d_side.alloc(c->side_slots * sizeof(SideSlot)) != hipSuccess ||
        c->d_stats.alloc((ST_COUNT_ + 1) * 8) != hipSuccess ||
        hipMemset(c->d_stats, 0, (ST_COUNT_ + 1) * 8) != hipSuccess ||
        c->d_dirty.alloc(16) != hipSuccess || hipMemset(c->d_dirty, 0, 16) != hipSuccess)
        return fail(c, YSB_ERR_NOMEM, "device allocation failed");
    c->d_side_used = reinterpret_cast<u32*>(c->d_stats + ST_COUNT_);
    launch_side_clear(c->d_side, c->side_slots, c->s_comp);
    if (hipStreamSynchronize(c->s_comp) != hipSuccess) return fail(c, YSB_ERR_HIP, "side map initialisation failed");
    if (c->d_ring.alloc(16) != hipSuccess || c->h_ring.alloc(16) != hipSuccess ||
        c->d_ovf.alloc(cfg.overflow_capacity * sizeof(OvfEntry)) != hipSuccess || c->d_ovf_count.alloc(16) != hipSuccess)
        return fail(c, YSB_ERR_NOMEM, "device allocation failed");
    i64 ring[2] = {0, 0};
    if (cfg.ring_base_bucket != INT64_MIN) {
        ring[0] = cfg.ring_base_bucket;
        ring[1] = 1;
        c->ring_known = true;
        c->ring_lo = cfg.ring_base_bucket;
    }
    if (hipMemcpy(c->d_ring, ring, 16, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(c->d_ovf_count, 0, 16) != hipSuccess)
        return fail(c, YSB_ERR_HIP, "initialisation copy failed");
    // LDS window counters: WL = largest power of two with n_campaigns * WL <= LCNT_CAP
    if (!(cfg.flags & YSB_F_NO_LDS_COUNT)) {
        u32 wl = 0;
        for (u32 w = 2; (u64)w * cfg.n_campaigns <= (u64)LCNT_CAP && w <= cfg.window_ring; w <<= 1) wl = w;
        c->lds_wl = wl;
        c->lds_wl_log2 = wl ? log2u(wl) : 0;
    }
    return YSB_OK;
}

int ysb_open(ysb_ctx** out, int device, const ysb_config* cfg_in) {
    if (!out) return fail(nullptr, YSB_ERR_ARG, "out is NULL");
    *out = nullptr;
    ysb_config cfg;
    if (cfg_in) cfg = *cfg_in;
    else ysb_config_default(&cfg);
    if (cfg.time_divisor_ms < 1) return fail(nullptr, YSB_ERR_ARG, "time_divisor_ms must be >= 1");
    if (cfg.n_campaigns == 0) return fail(nullptr, YSB_ERR_ARG, "n_campaigns must be > 0");
    if (!is_pow2(cfg.window_ring) || cfg.window_ring < 16)
        return fail(nullptr, YSB_ERR_ARG, "window_ring must be a power of two >= 16");
    if (cfg.max_batch_bytes == 0 || cfg.max_batch_bytes > (4ull << 30) - 64)
        return fail(nullptr, YSB_ERR_ARG, "max_batch_bytes must be in (0, 4 GiB)");
    if (cfg.overflow_capacity == 0 || cfg.overflow_capacity > 0xFFFFFFFFull)
        return fail(nullptr, YSB_ERR_ARG, "overflow_capacity must be in [1, 2^32)");
    int ndev = 0;
    const hipError_t de = hipGetDeviceCount(&ndev);
    if (de != hipSuccess || ndev == 0) return no_device(de);
    if (device < 0 || device >= ndev) return fail(nullptr, YSB_ERR_ARG, "device %d out of range (%d)", device, ndev);

    ysb_ctx* c = new ysb_ctx();
    c->device = device;
    c->cfg = cfg;
    c->c_pad = cfg.n_campaigns;
    c->div = div_magic(cfg.time_divisor_ms);
    const int rc = init(c);
    if (rc) {
        g_open_err = c->err;
        destroy(c);
        return rc;
    }
    *out = c;
    return YSB_OK;
}

int ysb_close(ysb_ctx* c) {
    destroy(c);
    return YSB_OK;
}

// ---- ad table -------------------------------------------------------------------------

static int load_map(ysb_ctx* c, const char* const* ad_ids, const uint32_t* lens, const uint32_t* campaign_idx,
                    uint64_t n);

int ysb_load_ad_map_packed(ysb_ctx* c, const char* keys, uint32_t key_len, const uint32_t* campaign_idx,
                           uint64_t n) {
    return ysb_load_ad_map_packed_shard(c, keys, key_len, campaign_idx, n, 0, 1);
}

int ysb_load_ad_map_packed_shard(ysb_ctx* c, const char* keys, uint32_t key_len, const uint32_t* campaign_idx,
                                 uint64_t n, uint32_t rank, uint32_t nranks) {
    if (!c) return YSB_ERR_ARG;
    if (n && (!keys || !campaign_idx)) return fail(c, YSB_ERR_ARG, "NULL ad map arrays");
    std::vector<const char*> ptr(n);
    std::vector<u32> len(n, key_len);
    for (u64 i = 0; i < n; ++i) ptr[i] = keys + i * key_len;
    return ysb_load_ad_map_shard(c, ptr.data(), len.data(), campaign_idx, n, rank, nranks);
}

int ysb_load_ad_map(ysb_ctx* c, const char* const* ad_ids, const uint32_t* lens, const uint32_t* campaign_idx,
                    uint64_t n) {
    return ysb_load_ad_map_shard(c, ad_ids, lens, campaign_idx, n, 0, 1);
}

// The entries of this rank's shard only (the host-side hash the router and the generator's
// shard files use, ysb_ad_shard), then the tables; the context keeps its shard so that the
// deferred-line kernel can tell a foreign key's miss from a real one.
int ysb_load_ad_map_shard(ysb_ctx* c, const char* const* ad_ids, const uint32_t* lens, const uint32_t* campaign_idx,
                          uint64_t n, uint32_t rank, uint32_t nranks) {
    if (!c) return YSB_ERR_ARG;
    if (nranks == 0 || rank >= nranks) return fail(c, YSB_ERR_ARG, "bad shard %u / %u", rank, nranks);
    if (n && (!ad_ids || !campaign_idx)) return fail(c, YSB_ERR_ARG, "NULL ad map arrays");
    int rc = launch_pending_raw(c);   // a batch submitted before the new map joins against the old one
    if (rc) return rc;
    if (nranks == 1) {
        rc = load_map(c, ad_ids, lens, campaign_idx, n);
    } else {
        std::vector<const char*> p;
        std::vector<u32> l, cm;
        for (u64 i = 0; i < n; ++i) {
            const u32 len = lens ? lens[i] : 36u;
            if (ad_ids[i] && ad_shard(ad_ids[i], len, nranks) != rank) continue;
            p.push_back(ad_ids[i]);
            l.push_back(len);
            cm.push_back(campaign_idx[i]);
        }
        rc = load_map(c, p.data(), l.data(), cm.data(), p.size());
    }
    if (rc) return rc;
    c->shard_rank = rank;
    c->shard_n = nranks;
    return YSB_OK;
}

// Build (ysb_admap.h: host data only), upload, commit.  A table whose size changes gets its
// new buffer before the old one is released (peak device memory during such a reload: the old
// tables plus the new ones), and the context takes nothing before both copies are done: a
// failed allocation leaves the old map whole and in use.  Only a failed copy into a buffer
// that is reused (same size) has damaged the map in use: submits then fail as before a load.
static int commit_tables(ysb_ctx* c, const JoinTables& jt);

static int load_map(ysb_ctx* c, const char* const* ad_ids, const uint32_t* lens, const uint32_t* campaign_idx,
                    uint64_t n) {
    // the tables live on this context's GPU, whichever device the calling thread last set
    // (one process may drive several contexts, e.g. one per GPU of a node)
    HIPCHK(c, hipSetDevice(c->device));
    JoinTables jt;
    std::string err;
    const int rc = build_join_tables(ad_ids, lens, campaign_idx, n, c->cfg.n_campaigns,
                                     (c->cfg.flags & YSB_F_SPARSE_FAST_JOIN) != 0, &jt, &err);
    if (rc) return fail(c, rc, "%s", err.c_str());
    return commit_tables(c, jt);
}

static int commit_tables(ysb_ctx* c, const JoinTables& jt) {
    HIPCHK(c, hipStreamSynchronize(c->s_comp));
    const u64 tbytes = jt.table.size() * 4, cbytes = jt.ctable.size() * 4;
    DevBuf<u32> table, ctable;   // the new buffers of the tables that change size
    if (tbytes != c->d_table.bytes()) HIPCHK(c, table.alloc(tbytes));
    if (cbytes != c->d_ctable.bytes()) HIPCHK(c, ctable.alloc(cbytes));
    hipError_t e = hipMemcpy(table.h ? table : c->d_table, jt.table.data(), tbytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(ctable.h ? ctable : c->d_ctable, jt.ctable.data(), cbytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (!table.h || !ctable.h) c->table_loaded = false;   // a buffer of the map in use may be half written
        return fail(c, YSB_ERR_HIP, "ad map upload: %s", hipGetErrorString(e));
    }
    if (table.h) c->d_table = std::move(table);
    if (ctable.h) c->d_ctable = std::move(ctable);
    c->table_slots = jt.slots;
    c->ctable_slots = jt.cslots;
    c->cseed = jt.cseed;
    c->ctable_buckets = jt.buckets;
    c->ctable_partial = jt.partial;
    c->map_keys = jt.keys;
    c->map_keys36 = jt.keys36;
    c->table_loaded = true;
    return YSB_OK;
}

// ---- the live map (ysb_ad_map_upsert, ysb_ad_map_lookup, ysb_ad_map_info) -----------------

// The call's records on the device and the tables as the table kernels take them.
static int upsert_params(ysb_ctx* c, const std::vector<u32>& rec, UpsertParams* p) {
    const u64 n = rec.size() / SLOT_WORDS;
    int rc = grow_device(c, c->d_up_rec, rec.size() * 4, 64u << 10);
    if (!rc) rc = first_use(c, c->d_up_ctr, UP_COUNT_ * 4);
    if (rc) return rc;
    if (!c->h_up_ctr) HIPCHK(c, c->h_up_ctr.alloc(UP_COUNT_ * 4));
    HIPCHK(c, hipMemcpyAsync(c->d_up_rec, rec.data(), rec.size() * 4, hipMemcpyHostToDevice, c->s_comp));
    *p = UpsertParams{};
    p->table = c->d_table;
    p->table_mask = (u32)(c->table_slots - 1);
    p->ctable = c->d_ctable;
    p->ctable_mask = (u32)(c->ctable_slots - 1);
    p->buckets = c->ctable_buckets ? 1u : 0u;
    p->sparse = (c->cfg.flags & YSB_F_SPARSE_FAST_JOIN) ? 1u : 0u;
    p->cseed = c->cseed;
    p->rec = c->d_up_rec;
    p->n = (u32)n;
    p->ctr = c->d_up_ctr;
    p->rng = upsert_rng(c->cseed, c->map_keys);
    return YSB_OK;
}

// The counters after the kernels queued so far (one small pinned read; waits).
static int upsert_counters(ysb_ctx* c) {
    HIPCHK(c, hipMemcpyAsync(c->h_up_ctr, c->d_up_ctr, UP_COUNT_ * 4, hipMemcpyDeviceToHost, c->s_comp));
    HIPCHK(c, hipStreamSynchronize(c->s_comp));
    return YSB_OK;
}

// The rebuild: the general table read back, the call's records merged in, the tables of the
// grown map built and committed as a load's.
static int upsert_rebuild(ysb_ctx* c, const std::vector<u32>& rec) {
    std::vector<u32> table(c->table_slots * SLOT_WORDS), merged;
    HIPCHK(c, hipMemcpy(table.data(), c->d_table, table.size() * 4, hipMemcpyDeviceToHost));
    upsert_merge(table.data(), c->table_slots, rec.data(), rec.size() / SLOT_WORDS, &merged);
    std::vector<u32>().swap(table);
    JoinTables jt;
    std::string err;
    const int rc = build_join_tables_rec(merged, c->cfg.n_campaigns, (c->cfg.flags & YSB_F_SPARSE_FAST_JOIN) != 0, &jt, &err);
    if (rc) return fail(c, rc, "%s", err.c_str());
    return commit_tables(c, jt);
}

int ysb_ad_map_upsert(ysb_ctx* c, const char* const* ad_ids, const uint32_t* lens, const uint32_t* campaign_idx,
                      uint64_t n, ysb_upsert_info* info) {
    if (!c) return YSB_ERR_ARG;
    if (n && (!ad_ids || !campaign_idx)) return fail(c, YSB_ERR_ARG, "NULL ad map arrays");
    if (!c->table_loaded) return fail(c, YSB_ERR_STATE, "ysb_load_ad_map has not been called");
    if (n >= (1ull << 31)) return fail(c, YSB_ERR_CAPACITY, "at most 2^31-1 entries per upsert");
    ysb_upsert_info out{};
    std::vector<u32> rec;
    std::string err;
    int rc = upsert_records(ad_ids, lens, campaign_idx, n, c->cfg.n_campaigns, c->shard_rank, c->shard_n, &rec,
                            &out.foreign, &out.duplicates, &err);
    if (rc) return fail(c, rc, "%s", err.c_str());
    out.entries = n;
    out.partial = c->ctable_partial ? 1u : 0u;
    const u64 nrec = rec.size() / SLOT_WORDS;
    if (nrec) {
        if ((rc = launch_pending_raw(c))) return rc;   // a batch submitted before the call joins against the old map
        HIPCHK(c, hipSetDevice(c->device));
        UpsertParams p;
        if ((rc = upsert_params(c, rec, &p))) return rc;
        if ((rc = grow_device(c, c->d_up_fresh, nrec * 4, 16u << 10))) return rc;
        if ((rc = grow_device(c, c->d_up_homeless, nrec * 4, 16u << 10))) return rc;
        p.fresh = c->d_up_fresh;
        p.homeless = c->d_up_homeless;
        for (Event& e : c->ev_up)
            if (!e.h) HIPCHK(c, e.create(hipEventDefault));
        HIPCHK(c, hipMemsetAsync(c->d_up_ctr, 0, UP_COUNT_ * 4, c->s_comp));
        HIPCHK(c, hipEventRecord(c->ev_up[0], c->s_comp));
        launch_upsert_classify(p, c->s_comp);
        HIPCHK(c, hipGetLastError());
        if ((rc = upsert_counters(c))) return rc;
        const u32* k = c->h_up_ctr;
        out.updated = k[UP_UPDATED];
        out.inserted = k[UP_NEW];
        const u64 n_new = k[UP_NEW], n_new36 = k[UP_NEW36];
        if (!upsert_fits(c->map_keys + n_new, c->map_keys36 + n_new36, c->table_slots, c->ctable_slots, c->ctable_buckets)) {
            if ((rc = upsert_rebuild(c, rec))) return rc;
            out.rebuilt = 1;
        } else {
            if (n_new) {
                launch_upsert_insert(p, (u32)n_new, c->s_comp);
                if (n_new36) launch_upsert_evict(p, c->s_comp);
                HIPCHK(c, hipGetLastError());
            }
            HIPCHK(c, hipEventRecord(c->ev_up[1], c->s_comp));
            if ((rc = upsert_counters(c))) return rc;
            float ms = 0;
            HIPCHK(c, hipEventElapsedTime(&ms, c->ev_up[0], c->ev_up[1]));
            out.device_ms = ms;
            out.cuckoo_first = k[UP_FIRST];
            out.cuckoo_second = k[UP_SECOND];
            out.cuckoo_moved = k[UP_MOVED];
            out.cuckoo_left_out = k[UP_LEFT_OUT];
            if (out.cuckoo_left_out) c->ctable_partial = true;   // until the next load or rebuild
            c->map_keys += n_new;
            c->map_keys36 += out.cuckoo_first + out.cuckoo_second + out.cuckoo_moved;
        }
        out.partial = c->ctable_partial ? 1u : 0u;
    }
    if (info) *info = out;
    return YSB_OK;
}

int ysb_ad_map_upsert_packed(ysb_ctx* c, const char* keys, uint32_t key_len, const uint32_t* campaign_idx,
                             uint64_t n, ysb_upsert_info* info) {
    if (!c) return YSB_ERR_ARG;
    if (n && (!keys || !campaign_idx)) return fail(c, YSB_ERR_ARG, "NULL ad map arrays");
    std::vector<const char*> ptr(n);
    std::vector<u32> len(n, key_len);
    for (u64 i = 0; i < n; ++i) ptr[i] = keys + i * key_len;
    return ysb_ad_map_upsert(c, ptr.data(), len.data(), campaign_idx, n, info);
}

uint64_t ysb_upsert_info_size(void) { return sizeof(ysb_upsert_info); }

int ysb_ad_map_lookup(ysb_ctx* c, const char* const* ad_ids, const uint32_t* lens, uint64_t n, uint32_t* out_campaign,
                      uint32_t* out_where) {
    if (!c) return YSB_ERR_ARG;
    if (n && !ad_ids) return fail(c, YSB_ERR_ARG, "NULL ad ids");
    if (!c->table_loaded) return fail(c, YSB_ERR_STATE, "ysb_load_ad_map has not been called");
    if (n >= (1ull << 31)) return fail(c, YSB_ERR_CAPACITY, "at most 2^31-1 ids per lookup");
    std::vector<u32> rec(n * SLOT_WORDS, 0);
    for (u64 i = 0; i < n; ++i) {
        const u32 len = lens ? lens[i] : 36u;
        if (len > MAX_KEY_BYTES) return fail(c, YSB_ERR_FORMAT, "ad id %llu longer than %u bytes", (unsigned long long)i, MAX_KEY_BYTES);
        if (!ad_ids[i] && len) return fail(c, YSB_ERR_ARG, "ad id %llu is NULL", (unsigned long long)i);
        rec[i * SLOT_WORDS] = len;
        if (len) std::memcpy(&rec[i * SLOT_WORDS + 2], ad_ids[i], len);
    }
    if (!n) return YSB_OK;
    int rc = launch_pending_raw(c);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    UpsertParams p;
    if ((rc = upsert_params(c, rec, &p))) return rc;
    if ((rc = grow_device(c, c->d_up_out, 2 * n * 4, 32u << 10))) return rc;
    u32* d_where = c->d_up_out + n;
    launch_admap_lookup(p, c->d_up_out, d_where, c->s_comp);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->s_comp));
    if (out_campaign) HIPCHK(c, hipMemcpy(out_campaign, c->d_up_out, n * 4, hipMemcpyDeviceToHost));
    if (out_where) HIPCHK(c, hipMemcpy(out_where, d_where, n * 4, hipMemcpyDeviceToHost));
    return YSB_OK;
}

int ysb_ad_map_info(ysb_ctx* c, ysb_admap_desc* out) {
    if (!c || !out) return YSB_ERR_ARG;
    if (!c->table_loaded) return fail(c, YSB_ERR_STATE, "ysb_load_ad_map has not been called");
    *out = ysb_admap_desc{c->map_keys, c->map_keys36, c->table_slots, c->ctable_slots, c->ctable_buckets ? 1u : 0u,
                          c->ctable_partial ? 1u : 0u, c->shard_rank, c->shard_n};
    return YSB_OK;
}

uint64_t ysb_admap_desc_size(void) { return sizeof(ysb_admap_desc); }

void poll_ring(ysb_ctx* c) {
    if (c->ring_known || !c->ring_query_pending) return;
    if (hipEventQuery(c->ev_ring) == hipSuccess) {
        c->ring_query_pending = false;
        if (c->h_ring[1]) { c->ring_known = true; c->ring_lo = c->h_ring[0]; }
    }
}

// The delta ring into the u64 ring (queued on the compute stream), delta cleared.
int fold_delta(ysb_ctx* c) {
    if (!c->d_delta || c->delta_bound == 0) return YSB_OK;
    launch_fold(c->d_counts, c->d_delta, c->delta_cells, c->s_comp);
    HIPCHK(c, hipGetLastError());
    c->delta_bound = 0;
    c->pend_u64 = true;   // pending counts now sit in the u64 ring
    return YSB_OK;
}

int sync_streams(ysb_ctx* c) {
    int rc = launch_pending_raw(c);
    if (!rc) rc = finish_unpack(c);   // a pipelined exchange's owner block
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->s_copy));
    HIPCHK(c, hipStreamSynchronize(c->s_comp));
    if (c->s_x) HIPCHK(c, hipStreamSynchronize(c->s_x));
    poll_ring(c);
    return YSB_OK;
}


// After the streams are idle: the out-of-ring map is emptied into the exact host-side
// list once it is a quarter full (so it never fills across launches: the side list
// grows on demand), and counts the device could not place anywhere (the map full
// within one launch AND the fallback list full) fail the call -- results would no
// longer be exact.  The loss is sticky until ysb_reset.
static int check_capacity(ysb_ctx* c) {
    unsigned long long v[ST_COUNT_ + 1];
    HIPCHK(c, hipMemcpy(v, c->d_stats, sizeof v, hipMemcpyDeviceToHost));
    const u32 used = (u32)v[ST_COUNT_];
    if ((u64)used * 4 > c->side_slots) {
        int rc = pull_side_list(c);
        if (rc) return rc;
    }
    if (v[ST_OVF_DROPPED])
        return fail(c, YSB_ERR_CAPACITY,
                    "%llu joined views outside the window ring were lost: the out-of-ring map and its "
                    "fallback list (overflow_capacity %llu) filled; counts are not exact "
                    "until ysb_reset (raise overflow_capacity or window_ring, or submit smaller batches)",
                    (unsigned long long)v[ST_OVF_DROPPED], (unsigned long long)c->cfg.overflow_capacity);
    if (c->park_cap) {   // a full log of parked views (ysb_parked_enable): those views were join misses
        const int rc = park_counters(c);
        if (rc) return rc;
        const u64 dropped = ((u64)c->h_park_ctr[PK_DROPPED + 1] << 32) | c->h_park_ctr[PK_DROPPED];
        if (dropped)
            return fail(c, YSB_ERR_CAPACITY,
                        "%llu views of unknown ads found the log of parked views full (capacity %llu) and "
                        "were counted as join misses; counts are not the reference's until ysb_reset "
                        "(raise the capacity or resolve more often)",
                        (unsigned long long)dropped, (unsigned long long)c->park_cap);
    }
    if ((c->cfg.flags & YSB_F_STRICT) && (v[ST_PARSE_ERR] || v[ST_TIME_ERR] || v[ST_FOREIGN]))
        return fail(c, YSB_ERR_DATA,
                    "strict mode: %llu lines JSONObject/getString would throw on, %llu event_times "
                    "Long.parseLong rejects, %llu views of another rank's ad shard (routing does not match "
                    "the sharded join table); sticky until ysb_reset",
                    (unsigned long long)v[ST_PARSE_ERR], (unsigned long long)v[ST_TIME_ERR],
                    (unsigned long long)v[ST_FOREIGN]);
    return YSB_OK;
}

int ysb_sync(ysb_ctx* c) {
    if (!c) return YSB_ERR_ARG;
    int rc = sync_streams(c);
    if (rc) return rc;
    return check_capacity(c);
}

// ---- results --------------------------------------------------------------------------------

int read_ring(ysb_ctx* c) {
    i64 r[2];
    HIPCHK(c, hipMemcpy(r, c->d_ring, 16, hipMemcpyDeviceToHost));
    if (r[1]) { c->ring_known = true; c->ring_lo = r[0]; }
    c->ring_query_pending = false;
    return YSB_OK;
}

int pull_side_list(ysb_ctx* c) {
    u32 cnt = 0;
    HIPCHK(c, hipMemcpy(&cnt, c->d_ovf_count, 4, hipMemcpyDeviceToHost));
    const u32 m = (u32)std::min<u64>(cnt, c->cfg.overflow_capacity);
    if (m) {
        std::vector<OvfEntry> v(m);
        HIPCHK(c, hipMemcpy(v.data(), c->d_ovf, (u64)m * sizeof(OvfEntry), hipMemcpyDeviceToHost));
        for (const auto& e : v) c->side[{e.campaign, e.bucket}] += e.count;
    }
    if (cnt) HIPCHK(c, hipMemset(c->d_ovf_count, 0, 4));
    // the out-of-ring map: every occupied slot to the host map, then the map is emptied
    u32 used = 0;
    HIPCHK(c, hipMemcpy(&used, c->d_side_used, 4, hipMemcpyDeviceToHost));
    if (used) {
        int rc = first_use(c, c->d_rows_n, 8);
        if (rc) return rc;
        u32 k = 0;
        HIPCHK(c, hipMemsetAsync(c->d_rows_n, 0, 4, c->s_comp));
        launch_side_compact(c->d_side, c->side_slots, c->side_cbits, true, nullptr, c->d_rows_n, 0, c->s_comp);
        HIPCHK(c, hipMemcpyAsync(&k, c->d_rows_n, 4, hipMemcpyDeviceToHost, c->s_comp));
        HIPCHK(c, hipStreamSynchronize(c->s_comp));
        if ((rc = grow_device(c, c->d_rows, k * sizeof(TableRow), 4096 * sizeof(TableRow)))) return rc;
        if (k) {
            std::vector<TableRow> h(k);
            HIPCHK(c, hipMemsetAsync(c->d_rows_n, 0, 4, c->s_comp));
            launch_side_compact(c->d_side, c->side_slots, c->side_cbits, false, c->d_rows, c->d_rows_n, k, c->s_comp);
            HIPCHK(c, hipMemcpyAsync(h.data(), c->d_rows, (u64)k * sizeof(TableRow), hipMemcpyDeviceToHost, c->s_comp));
            HIPCHK(c, hipStreamSynchronize(c->s_comp));
            for (const TableRow& r : h) c->side[{r.campaign, r.bucket}] += r.count;
        }
        launch_side_clear(c->d_side, c->side_slots, c->s_comp);
        HIPCHK(c, hipMemsetAsync(c->d_side_used, 0, 4, c->s_comp));
        HIPCHK(c, hipStreamSynchronize(c->s_comp));
    }
    return YSB_OK;
}

// Non-zero ring cells of buckets [blo, bhi) (rank-local table + owned block), compacted
// on the device (two passes: count, then rows), added to `into`; clear zeroes them.
static int ring_rows(ysb_ctx* c, i64 blo, i64 bhi, bool clear, std::map<std::pair<u32, i64>, u64>& into) {
    HIPCHK(c, hipSetDevice(c->device));
    int frc = fold_delta(c);
    if (frc) return frc;
    if (!c->ring_known) return YSB_OK;
    const u32 W = c->cfg.window_ring;
    const i64 lo = c->ring_lo;
    const i64 a = std::max<i64>(blo, lo), b = std::min<i64>(bhi, lo + (i64)W);
    if (a >= b) return YSB_OK;
    const u32 nb = (u32)(b - a);
    if ((frc = fold_owned(c))) return frc;
    struct Tab { unsigned long long* t; u32 rows, off; };
    std::vector<Tab> tabs{{c->d_counts, c->cfg.n_campaigns, 0u}};
    if (c->d_owned) {
        u32 olo = 0, ohi = 0;
        ysb_group_block(c->cfg.n_campaigns, c->rank, c->nranks, &olo, &ohi);
        if (ohi > olo) tabs.push_back({c->d_owned, ohi - olo, olo});
    }
    if ((frc = first_use(c, c->d_rows_n, 8))) return frc;
    for (const Tab& t : tabs) {
        u32 n = 0;
        HIPCHK(c, hipMemsetAsync(c->d_rows_n, 0, 4, c->s_comp));
        launch_compact(t.t, t.rows, W, a, nb, t.off, true, false, nullptr, c->d_rows_n, 0, c->s_comp);
        HIPCHK(c, hipMemcpyAsync(&n, c->d_rows_n, 4, hipMemcpyDeviceToHost, c->s_comp));
        HIPCHK(c, hipStreamSynchronize(c->s_comp));
        if (!n) continue;
        if ((frc = grow_device(c, c->d_rows, n * sizeof(TableRow), 4096 * sizeof(TableRow)))) return frc;
        std::vector<TableRow> h(n);
        u32 m = 0;
        HIPCHK(c, hipMemsetAsync(c->d_rows_n, 0, 4, c->s_comp));
        launch_compact(t.t, t.rows, W, a, nb, t.off, false, clear, c->d_rows, c->d_rows_n, n, c->s_comp);
        HIPCHK(c, hipMemcpyAsync(&m, c->d_rows_n, 4, hipMemcpyDeviceToHost, c->s_comp));
        HIPCHK(c, hipMemcpyAsync(h.data(), c->d_rows, (u64)n * sizeof(TableRow), hipMemcpyDeviceToHost, c->s_comp));
        HIPCHK(c, hipStreamSynchronize(c->s_comp));
        if (m != n) return fail(c, YSB_ERR_STATE, "table changed during drain (%u vs %u cells)", m, n);
        for (const TableRow& r : h) into[{r.campaign, r.bucket}] += r.count;
    }
    return YSB_OK;
}

// ---- asynchronous flush (CampaignProcessorCommon's flusher thread, :35-55, 91-98) --------------

constexpr u64 FLUSH_MAX_ROWS = 1u << 20;

int ysb_flush_begin(ysb_ctx* c, int64_t blo, int64_t bhi) {
    if (!c) return YSB_ERR_ARG;
    if (grouped(c)) return fail(c, YSB_ERR_STATE, "ysb_flush_begin after ysb_group_init: use ysb_drain");
    if (c->fl_n == ysb_ctx::FLUSH_SLOTS)
        return fail(c, YSB_ERR_STATE, "%d flushes outstanding: ysb_flush_end first", ysb_ctx::FLUSH_SLOTS);
    int rc = launch_pending_raw(c);   // every batch submitted so far is counted before the compaction
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const u32 W = c->cfg.window_ring;
    const int k = (c->fl_head + c->fl_n) % ysb_ctx::FLUSH_SLOTS;
    auto& f = c->fl[k];
    if (!c->d_fl_n) {
        HIPCHK(c, c->d_fl_n.alloc(4 * ysb_ctx::FLUSH_SLOTS));
        HIPCHK(c, hipMemset(c->d_fl_n, 0, 4 * ysb_ctx::FLUSH_SLOTS));
    }
    if (!f.h_rows) {   // every nonzero cell of the ring fits (up to FLUSH_MAX_ROWS)
        f.cap = std::min<u64>((u64)c->cfg.n_campaigns * W, FLUSH_MAX_ROWS);
        HIPCHK(c, f.h_rows.alloc(f.cap * sizeof(TableRow)));
        HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&f.hd_rows), f.h_rows, 0));
        HIPCHK(c, f.h_n.alloc(16));
        HIPCHK(c, f.ev.create());
    }
    // the ring's base: known once the first launch's auto-base is back (a copy of 16 bytes)
    poll_ring(c);
    if (!c->ring_known && c->ring_query_pending) {
        HIPCHK(c, hipEventSynchronize(c->ev_ring));
        poll_ring(c);
    }
    if ((rc = fold_delta(c))) return rc;   // record mode's pending bytes into the u64 ring (stream order)
    HIPCHK(c, hipMemsetAsync(c->d_fl_n + k, 0, 4, c->s_comp));
    if (c->ring_known) {
        const i64 a = std::max<i64>(blo, c->ring_lo), b = std::min<i64>(bhi, c->ring_lo + (i64)W);
        if (a < b)   // straight into the pinned rows; a cell past cap keeps its count (next flush)
            launch_compact(c->d_counts, c->cfg.n_campaigns, W, a, (u32)(b - a), 0, false, true, f.hd_rows,
                           c->d_fl_n + k, (u32)f.cap, c->s_comp);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipMemcpyAsync(f.h_n, c->d_fl_n + k, 4, hipMemcpyDeviceToHost, c->s_comp));
    HIPCHK(c, hipEventRecord(f.ev, c->s_comp));
    c->fl_n++;
    return YSB_OK;
}

int ysb_flush_end(ysb_ctx* c, int wait, ysb_count* out, uint64_t cap, uint64_t* n_out, int* more) {
    if (!c || !n_out) return c ? fail(c, YSB_ERR_ARG, "n_out is NULL") : YSB_ERR_ARG;
    if (!c->fl_n) return fail(c, YSB_ERR_STATE, "no flush begun");
    HIPCHK(c, hipSetDevice(c->device));
    auto& f = c->fl[c->fl_head];
    if (!wait) {
        const hipError_t q = hipEventQuery(f.ev);
        if (q == hipErrorNotReady) return YSB_PENDING;
        if (q != hipSuccess) return fail(c, YSB_ERR_HIP, "hipEventQuery: %s", hipGetErrorString(q));
    }
    HIPCHK(c, hipEventSynchronize(f.ev));
    const u64 written = *f.h_n;
    const u64 n = std::min<u64>(written, f.cap);
    *n_out = n;
    if (more) *more = written > f.cap ? 1 : 0;
    if (!out) return YSB_OK;   // (the rows stay: call again with a buffer)
    if (cap < n) return fail(c, YSB_ERR_CAPACITY, "flush needs %llu rows, cap %llu", (unsigned long long)n,
                             (unsigned long long)cap);
    std::vector<TableRow> rows(f.h_rows.get(), f.h_rows.get() + n);
    std::sort(rows.begin(), rows.end(), [](const TableRow& x, const TableRow& y) {
        return x.campaign != y.campaign ? x.campaign < y.campaign : x.bucket < y.bucket;
    });
    for (u64 i = 0; i < n; ++i) {
        out[i].campaign = rows[i].campaign;
        out[i].reserved = 0;
        out[i].window_ms = rows[i].bucket * c->cfg.time_divisor_ms;
        out[i].count = rows[i].count;
    }
    c->fl_head = (c->fl_head + 1) % ysb_ctx::FLUSH_SLOTS;
    c->fl_n--;
    return YSB_OK;
}

int ysb_drain(ysb_ctx* c, int64_t blo, int64_t bhi, int clear, ysb_count* out, uint64_t cap, uint64_t* n_out) {
    if (!c || !n_out) return c ? fail(c, YSB_ERR_ARG, "n_out is NULL") : YSB_ERR_ARG;
    int rc = ysb_sync(c);
    if (rc) return rc;
    if ((rc = read_ring(c))) return rc;
    if ((rc = pull_side_list(c))) return rc;
    std::map<std::pair<u32, i64>, u64> rows;
    if (clear && out) {
        // move the ring range into the host map first: nothing is lost if `cap` is short
        if ((rc = ring_rows(c, blo, bhi, true, c->side))) return rc;
    } else if ((rc = ring_rows(c, blo, bhi, false, rows))) {
        return rc;
    }
    for (auto it = c->side.begin(); it != c->side.end(); ++it)
        if (it->first.second >= blo && it->first.second < bhi && it->second) rows[it->first] += it->second;
    *n_out = rows.size();
    if (!out) return YSB_OK;
    if (cap < rows.size()) return fail(c, YSB_ERR_CAPACITY, "drain needs %llu rows, cap %llu", (unsigned long long)rows.size(), (unsigned long long)cap);
    u64 k = 0;
    for (const auto& r : rows) {
        out[k].campaign = r.first.first;
        out[k].reserved = 0;
        out[k].window_ms = r.first.second * c->cfg.time_divisor_ms;
        out[k].count = r.second;
        ++k;
    }
    if (clear) {
        for (auto it = c->side.begin(); it != c->side.end();) {
            if (it->first.second >= blo && it->first.second < bhi) it = c->side.erase(it);
            else ++it;
        }
    }
    return YSB_OK;
}

// Moves the ring to [new_lo, new_lo + W): buckets of the old range that the new range
// does not hold go to the exact host-side list (both the rank-local table and, after an
// exchange, the owned block); cells are indexed by bucket mod W, so the rest stays put.
int move_ring(ysb_ctx* c, i64 new_lo) {
    int rc;
    if (c->ring_known && new_lo != c->ring_lo) {
        const i64 lo = c->ring_lo, W = (i64)c->cfg.window_ring;
        const i64 a = new_lo > lo ? lo : std::max<i64>(new_lo + W, lo);
        const i64 b = new_lo > lo ? std::min<i64>(new_lo, lo + W) : lo + W;
        if (a < b && (rc = ring_rows(c, a, b, true, c->side))) return rc;
    }
    i64 r[2] = {new_lo, 1};
    HIPCHK(c, hipMemcpy(c->d_ring, r, 16, hipMemcpyHostToDevice));
    c->ring_known = true;
    c->ring_lo = new_lo;
    c->ring_query_pending = false;
    return YSB_OK;
}

int ysb_ring_advance(ysb_ctx* c, int64_t new_lo) {
    if (!c) return YSB_ERR_ARG;
    // (no capacity check here: after ysb_group_init this is a collective, and a rank must
    // not leave before the others' all-reduce; ysb_sync / ysb_drain report a loss)
    int rc = sync_streams(c);
    if (rc) return rc;
    if ((rc = read_ring(c))) return rc;
    if (grouped(c)) {
        // collective after ysb_group_init: every rank's ring moves together (all ranks call
        // it with the same new_lo; a disagreement fails on every rank alike)
        if (!c->ring_agreed && (rc = agree_ring(c))) return rc;
        i64 h[2] = {new_lo, -new_lo};
        if ((rc = allreduce_max(c, h, 2))) return rc;
        if (h[0] != -h[1]) return fail(c, YSB_ERR_ARG, "ysb_ring_advance: ranks asked for different ring bases");
        c->x_have_plan = false;   // the plan's slots held other buckets
    }
    if (new_lo <= INT64_MIN / 2 || new_lo >= INT64_MAX / 2) return fail(c, YSB_ERR_ARG, "ring base out of range");
    return move_ring(c, new_lo);
}

int ysb_stats_get(ysb_ctx* c, ysb_stats* s) {
    if (!c || !s) return c ? fail(c, YSB_ERR_ARG, "NULL stats") : YSB_ERR_ARG;
    int rc = sync_streams(c);   // readable after a capacity loss (overflow_dropped tells it)
    if (rc) return rc;
    unsigned long long v[ST_COUNT_];
    HIPCHK(c, hipMemcpy(v, c->d_stats, sizeof v, hipMemcpyDeviceToHost));
    s->events = v[ST_EVENTS];
    s->views = v[ST_VIEWS];
    s->joined = v[ST_JOINED];
    s->join_misses = v[ST_MISSES];
    s->parse_errors = v[ST_PARSE_ERR];
    s->time_errors = v[ST_TIME_ERR];
    s->out_of_ring = v[ST_OUT_OF_RING];
    s->overflow_dropped = v[ST_OVF_DROPPED];
    s->batches = c->batches;
    s->deferred = v[ST_DEFERRED];
    s->foreign_shard = v[ST_FOREIGN];
    return YSB_OK;
}

int ysb_reset(ysb_ctx* c) {
    if (!c) return YSB_ERR_ARG;
    c->raw_fail = 0;   // a raw batch that could not launch was dropped: counting starts over
    int rc = sync_streams(c);
    if (rc) return rc;
    c->fl_head = c->fl_n = 0;   // outstanding asynchronous flushes are dropped
    const u64 cells = (u64)c->c_pad * c->cfg.window_ring;
    HIPCHK(c, hipMemset(c->d_counts, 0, cells * 8));
    if (c->d_delta) HIPCHK(c, hipMemset(c->d_delta, 0, c->delta_cells));
    c->delta_bound = 0;
    HIPCHK(c, hipMemset(c->d_dirty, 0, 4));
    c->pend_u64 = false;
    c->x_have_plan = false;
    if (c->d_owned) HIPCHK(c, hipMemset(c->d_owned, 0, cells / c->nranks * 8));
    if (c->d_owned8) HIPCHK(c, hipMemset(c->d_owned8, 0, cells / c->nranks));
    c->owned8_dirty = false;
    if (c->d_truth) HIPCHK(c, hipMemset(c->d_truth, 0, cells * 8));
    if (c->d_truth_out) HIPCHK(c, hipMemset(c->d_truth_out, 0, 8));
    HIPCHK(c, hipMemset(c->d_ovf_count, 0, 16));
    launch_side_clear(c->d_side, c->side_slots, c->s_comp);
    HIPCHK(c, hipStreamSynchronize(c->s_comp));
    HIPCHK(c, hipMemset(c->d_side_used, 0, 4));
    HIPCHK(c, hipMemset(c->d_stats, 0, ST_COUNT_ * 8));
    if ((rc = park_reset(c))) return rc;   // the log of parked views emptied; parking stays enabled
    c->side.clear();
    c->batches = 0;
    c->lz4_last = ysb_lz4_desc{};
    c->lz4f_last = ysb_lz4_frame_desc{};
    c->lz4f_more = false;
    c->kafka_last = ysb_kafka_desc{};
    c->kafka_lz4_last = ysb_kafka_lz4_desc{};
    c->kafka_infl_cap_test = 0;   // (test support does not outlive a reset)
    c->kafka_crc_last = ysb_kafka_crc_desc{};   // (the mode stays: a context setting)
    if (c->d_carry) HIPCHK(c, hipMemset(c->d_carry, 0, LZ4_CARRY_HEAD));   // the carry is cleared
    return YSB_OK;
}

int ysb_ring_range(ysb_ctx* c, int64_t* lo, uint32_t* width) {
    if (!c) return YSB_ERR_ARG;
    int rc = ysb_sync(c);
    if (rc) return rc;
    if ((rc = read_ring(c))) return rc;
    if (!c->ring_known) return fail(c, YSB_ERR_STATE, "ring base not set yet");
    if (lo) *lo = c->ring_lo;
    if (width) *width = c->cfg.window_ring;
    return YSB_OK;
}

int ysb_kernel_time(ysb_ctx* c, double* total_ms, uint64_t* launches) {
    if (!c) return YSB_ERR_ARG;
    int rc = sync_streams(c);
    if (rc) return rc;
    double t[3] = {0, 0, 0};   // (-, the scans, the launches' whole path)
    u64 n = 0;
    HIPCHK(c, c->tev.collect(t, &n));
    if (total_ms) *total_ms = t[1];
    if (launches) *launches = n;
    c->path_ms_acc = t[2];
    c->path_launches_acc = n;
    return YSB_OK;
}

int ysb_path_time(ysb_ctx* c, double* total_ms, uint64_t* launches, uint64_t* record_launches) {
    if (!c) return YSB_ERR_ARG;
    if (total_ms) *total_ms = c->path_ms_acc;
    if (launches) *launches = c->path_launches_acc;
    if (record_launches) *record_launches = c->rec_launches;
    return YSB_OK;
}

int ysb_launch_info(ysb_ctx* c, ysb_launch_desc* out) {
    if (!c || !out) return c ? fail(c, YSB_ERR_ARG, "NULL output") : YSB_ERR_ARG;
    int rc = launch_pending_raw(c);
    if (rc) return rc;
    *out = c->last_launch;
    return YSB_OK;
}

uint64_t ysb_record_desc_size(void) { return sizeof(ysb_record_desc); }

int ysb_record_info(ysb_ctx* c, ysb_record_desc* out, uint32_t* rec_n, uint64_t rec_n_cap, uint32_t* runs,
                    uint64_t runs_cap) {
    if (!c || !out) return c ? fail(c, YSB_ERR_ARG, "NULL output") : YSB_ERR_ARG;
    int rc = sync_streams(c);
    if (rc) return rc;
    if (!c->rec_launches) return fail(c, YSB_ERR_STATE, "no record-mode launch has run");
    const RecPlan& pl = c->rec_last;
    *out = ysb_record_desc{};
    out->w_log2 = pl.w_log2;
    out->blk_shift = pl.blk_shift;
    out->n_blocks = pl.n_blocks;
    out->sub_log2 = pl.sub_log2;
    out->bins = pl.bins;
    out->cap = pl.cap;
    out->grid = c->rec_last_grid;
    out->slices = REC_QUARTERS;
    out->area = pl.area;
    out->part = pl.part;
    out->delta_bound = c->delta_bound;
    HIPCHK(c, hipMemcpy(&out->dirty, c->d_dirty, 4, hipMemcpyDeviceToHost));
    const u64 n_rec = (u64)c->rec_last_grid * pl.bins, n_runs = (u64)pl.n_blocks * REC_QUARTERS * 2;
    if ((rec_n && rec_n_cap < n_rec) || (runs && runs_cap < n_runs))
        return fail(c, YSB_ERR_CAPACITY, "ysb_record_info: rec_n holds %llu of %llu, runs %llu of %llu",
                    (unsigned long long)rec_n_cap, (unsigned long long)n_rec, (unsigned long long)runs_cap,
                    (unsigned long long)n_runs);
    if (rec_n) HIPCHK(c, hipMemcpy(rec_n, c->d_rec_n, n_rec * 4, hipMemcpyDeviceToHost));
    if (runs) HIPCHK(c, hipMemcpy(runs, c->d_runs, n_runs * 4, hipMemcpyDeviceToHost));
    return YSB_OK;
}

void* ysb_stream(ysb_ctx* c) {
    if (!c) return nullptr;
    // work the caller orders after it follows every submitted batch; NULL if one could not
    // launch (ysb_last_error says why)
    if (launch_pending_raw(c)) return nullptr;
    return (void*)c->s_comp;
}

// ---- device memory ----------------------------------------------------------------------------

int ysb_device_alloc(ysb_ctx* c, uint64_t bytes, void** p) {
    if (!c || !p) return YSB_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMalloc(p, bytes ? bytes : 16));
    return YSB_OK;
}
int ysb_device_free(ysb_ctx* c, void* p) {
    if (!c) return YSB_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipFree(p));
    return YSB_OK;
}
int ysb_memcpy_h2d(ysb_ctx* c, void* d, const void* h, uint64_t bytes) {
    if (!c) return YSB_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(d, h, bytes, hipMemcpyHostToDevice));
    return YSB_OK;
}
int ysb_memcpy_d2h(ysb_ctx* c, void* h, const void* d, uint64_t bytes) {
    if (!c) return YSB_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost));
    return YSB_OK;
}

#if defined(YSB_STAMPS) || defined(YSB_WGTIME)
// Diagnostic build only: the deferred-line list of the last batch.
int ysb_debug_defer_list(ysb_ctx* c, uint32_t* out, uint64_t cap) {
    if (!c) return YSB_ERR_ARG;
    int rc = ysb_sync(c);
    if (rc) return rc;
    if (!c->d_defer) return YSB_OK;
    HIPCHK(c, hipMemcpy(out, c->d_defer, std::min<u64>(cap * 4, c->d_defer.bytes()), hipMemcpyDeviceToHost));
    return YSB_OK;
}

// Diagnostic build only: per-wave phase cycles of the scan kernel since the last call.
int ysb_debug_stamps(ysb_ctx* c, uint64_t* out, uint64_t cap, uint64_t* n) {
    if (!c || !n) return YSB_ERR_ARG;
    int rc = ysb_sync(c);
    if (rc) return rc;
    *n = c->dbg_words;
    if (!out || !c->d_dbg) return YSB_OK;
    HIPCHK(c, hipMemcpy(out, c->d_dbg, std::min<u64>(cap, c->dbg_words) * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemset(c->d_dbg, 0, c->dbg_words * 8));
    return YSB_OK;
}
#endif

}  // extern "C"
