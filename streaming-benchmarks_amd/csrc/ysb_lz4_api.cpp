// ysb_lz4_api.cpp -- LZ4 batches above the kernel (ysb_lz4.hip; the rules: ysb_lz4.h): the
// directory's checks, a slot's staging (compressed bytes in pinned memory or left in place in a
// registered range, block descriptors in pinned memory, one copy each), the decode's one launch
// and read-back (launch_decode), the synchronous decode alone, the last batch's figures, and the
// host codec entries.  ysb_submit_raw_lz4 and ysb_submit_lz4_mapped sit beside ysb_submit_raw in
// ysb_raw.cpp.
#include "ysb_ctx.h"
#include "ysb_lz4.h"

using namespace ysb;

constexpr u64 LZ4_DESC_HEAD = 16;   // {first bad, bad blocks, 0, 0} in front of the descriptors

// the directory as argument errors (the same for both entry points)
static int dir_args(ysb_ctx* c, const uint8_t* bytes, u64 comp_bytes, const ysb_lz4_block* dir, u32 n, u64* raw_total) {
    if ((comp_bytes && !bytes) || (n && !dir)) return fail(c, YSB_ERR_ARG, "NULL batch buffers");
    u32 at = 0;
    *raw_total = 0;
    switch (lz4_check_dir(dir, n, comp_bytes, raw_total, &at)) {
    case LZ4_DIR_RAW:
        return fail(c, YSB_ERR_ARG, "LZ4 block %u: raw_bytes %u, not in 1..%u", at, dir[at].raw_bytes, LZ4_MAX_RAW);
    case LZ4_DIR_SUM:
        return fail(c, YSB_ERR_ARG, "the directory's %u blocks do not sum to comp_bytes (%llu)", n,
                    (unsigned long long)comp_bytes);
    }
    return YSB_OK;
}

// header and descriptors of a batch into `out`; the batch's figures into *info
static void fill_descs(const ysb_lz4_block* dir, u32 n, u8* out, ysb_lz4_desc* info, u32* max_raw) {
    const u32 head[4] = {LZ4_NO_BAD, 0, 0, 0};
    std::memcpy(out, head, LZ4_DESC_HEAD);
    Lz4Desc d{0, 0, 0, 0};
    u64 stored = 0;
    u32 mx = 0;
    for (u32 i = 0; i < n; ++i) {
        d.comp = dir[i].comp_bytes;
        d.raw = dir[i].raw_bytes;
        std::memcpy(out + LZ4_DESC_HEAD + (u64)i * sizeof(Lz4Desc), &d, sizeof d);
        d.in_off += lz4_entry_comp(dir[i]);
        d.out_off += d.raw;
        stored += (d.comp & LZ4_STORED) ? 1 : 0;
        mx = std::max(mx, d.raw);
    }
    *info = ysb_lz4_desc{};
    info->blocks = n;
    info->stored_blocks = stored;
    info->comp_bytes = d.in_off;
    info->raw_bytes = d.out_off;
    info->first_bad = LZ4_NO_BAD;
    *max_raw = mx;
}

extern "C" {

// One decode launch on s: the n_blocks blocks of d_comp, by the descriptors behind the
// LZ4_DESC_HEAD bytes of {first bad, bad blocks} in d_descs, into d_out; that pair's read-back
// to h_bad queued behind it.  ev: YSB_F_TIMING's event pair around the kernel (created on
// demand), or NULL.
static int launch_decode(ysb_ctx* c, const u8* d_comp, u8* d_descs, u32 n_blocks, u32 max_raw, u8* d_out, hipStream_t s,
                         Event* ev, u32* h_bad) {
    if (ev) {
        for (int k = 0; k < 2; ++k)
            if (!ev[k]) HIPCHK(c, ev[k].create(hipEventDefault));
        HIPCHK(c, hipEventRecord(ev[0], s));
    }
    u32* bad = reinterpret_cast<u32*>(d_descs);
    const Lz4Params lp{d_comp, reinterpret_cast<const Lz4Desc*>(d_descs + LZ4_DESC_HEAD), n_blocks, max_raw, d_out, bad};
    HIPCHK(c, launch_lz4_decode(lp, s));
    if (ev) HIPCHK(c, hipEventRecord(ev[1], s));
    HIPCHK(c, hipMemcpyAsync(h_bad, bad, 8, hipMemcpyDeviceToHost, s));
    return YSB_OK;
}

int lz4_stage(ysb_ctx* c, int slot, const uint8_t* bytes, uint64_t comp_bytes, const ysb_lz4_block* dir,
              uint32_t n_blocks, const uint8_t* dsrc, RawBatch* batch, std::vector<u8>* sample) {
    u64 raw_total = 0;
    int rc = dir_args(c, bytes, comp_bytes, dir, n_blocks, &raw_total);
    if (rc) return rc;
    if (comp_bytes > c->cfg.max_batch_bytes || raw_total > c->cfg.max_batch_bytes)
        return fail(c, YSB_ERR_CAPACITY, "LZ4 batch of %llu B (%llu B decoded) exceeds max_batch_bytes",
                    (unsigned long long)comp_bytes, (unsigned long long)raw_total);
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->d_lz4[slot]) HIPCHK(c, c->d_lz4[slot].alloc(c->cfg.max_batch_bytes + 64));
    if (!c->h_lz4bad) {
        HIPCHK(c, c->h_lz4bad.alloc(16));
        std::memset(c->h_lz4bad, 0, 16);
    }
    const u64 need = LZ4_DESC_HEAD + (u64)n_blocks * sizeof(Lz4Desc);
    if (need > c->lz4desc_cap[slot]) {   // (outside steady state: a batch with more blocks than any before)
        const u64 cap = std::max<u64>(need + need / 2, 64u << 10);
        if ((rc = grow_device(c, c->d_lz4desc[slot], cap + 64, 0))) return rc;
        HIPCHK(c, c->h_lz4desc[slot].alloc(cap + 64));
        HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&c->hd_lz4desc[slot]), c->h_lz4desc[slot], 0));
        c->lz4desc_cap[slot] = cap;
    }
    // the bytes: into the slot's pinned buffer, or read where they lie (a registered range)
    if (!dsrc && bytes != c->h_bytes[slot] && comp_bytes) std::memcpy(c->h_bytes[slot], bytes, comp_bytes);
    batch->nbytes = raw_total;
    Lz4Staged* out = &batch->lz4.emplace();
    out->hsrc = dsrc ? bytes : c->h_bytes[slot].get();
    out->dsrc = dsrc ? dsrc : c->hd_bytes[slot];
    fill_descs(dir, n_blocks, c->h_lz4desc[slot], &out->info, &out->max_raw);
    // the layout sample: block 0 as the host model decodes it (nothing if it is bad -- the
    // device decides that for the batch)
    sample->clear();
    if (n_blocks) {
        sample->resize(dir[0].raw_bytes);
        if (!lz4_decode_block(out->hsrc, dir[0], sample->data())) sample->clear();
    }
    return YSB_OK;
}

void lz4_copies(ysb_ctx* c, int slot, const Lz4Staged& b, SlotCopy v[2]) {
    v[0] = {c->d_lz4[slot], b.dsrc, b.hsrc, b.info.comp_bytes};
    v[1] = {c->d_lz4desc[slot], c->hd_lz4desc[slot], c->h_lz4desc[slot],
            b.info.blocks ? LZ4_DESC_HEAD + b.info.blocks * sizeof(Lz4Desc) : 0};
}

int lz4_enqueue_decode(ysb_ctx* c, int slot, const Lz4Staged& b, hipStream_t s) {
    c->h_lz4bad[2 * slot] = LZ4_NO_BAD;
    c->h_lz4bad[2 * slot + 1] = 0;
    if (!b.info.blocks) return YSB_OK;
    // the bad-block pair comes back through pinned memory with the line count: no host wait here
    return launch_decode(c, c->d_lz4[slot], c->d_lz4desc[slot], (u32)b.info.blocks, b.max_raw, c->d_bytes[slot], s,
                         (c->cfg.flags & YSB_F_TIMING) ? c->ev_lz4[slot] : nullptr, c->h_lz4bad + 2 * slot);
}

int lz4_settle(ysb_ctx* c, int slot, const Lz4Staged& b) {
    ysb_lz4_desc d = b.info;
    d.batches = c->lz4_last.batches + 1;
    d.first_bad = c->h_lz4bad[2 * slot];
    d.bad_blocks = c->h_lz4bad[2 * slot + 1];
    if (d.blocks && (c->cfg.flags & YSB_F_TIMING)) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, c->ev_lz4[slot][0], c->ev_lz4[slot][1]) == hipSuccess) d.decode_ms = ms;
    }
    c->lz4_last = d;
    if (d.bad_blocks)
        return fail(c, YSB_ERR_FORMAT, "LZ4 batch (slot %d): block %llu of %llu breaks the block format (%llu bad in all); "
                    "the batch was dropped", slot, (unsigned long long)d.first_bad, (unsigned long long)d.blocks,
                    (unsigned long long)d.bad_blocks);
    return YSB_OK;
}

int ysb_lz4_decode_device(ysb_ctx* c, const uint8_t* d_comp, uint64_t comp_bytes, const ysb_lz4_block* dir,
                          uint32_t n_blocks, uint8_t* d_out, uint64_t out_cap, uint64_t* raw_bytes,
                          uint32_t* first_bad) {
    if (!c) return YSB_ERR_ARG;
    u64 raw_total = 0;
    int rc = dir_args(c, d_comp, comp_bytes, dir, n_blocks, &raw_total);
    if (rc) return rc;
    if (raw_bytes) *raw_bytes = raw_total;
    if (first_bad) *first_bad = LZ4_NO_BAD;
    if (raw_total > out_cap)
        return fail(c, YSB_ERR_CAPACITY, "%llu B decoded, cap %llu", (unsigned long long)raw_total, (unsigned long long)out_cap);
    if (raw_total && !d_out) return fail(c, YSB_ERR_ARG, "NULL output buffer");
    if ((rc = launch_pending_raw(c))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    ysb_lz4_desc info{};
    u32 max_raw = 0;
    std::vector<u8> descs(LZ4_DESC_HEAD + (u64)n_blocks * sizeof(Lz4Desc));
    fill_descs(dir, n_blocks, descs.data(), &info, &max_raw);
    info.batches = c->lz4_last.batches + 1;
    u32 bad[2] = {LZ4_NO_BAD, 0};
    if (n_blocks) {
        if ((rc = grow_device(c, c->d_lz4desc_sync, descs.size(), 64u << 10))) return rc;
        HIPCHK(c, hipMemcpyAsync(c->d_lz4desc_sync, descs.data(), descs.size(), hipMemcpyHostToDevice, c->s_comp));
        const bool timed = (c->cfg.flags & YSB_F_TIMING) != 0u;
        Event ev[2];
        if ((rc = launch_decode(c, d_comp, c->d_lz4desc_sync, n_blocks, max_raw, d_out, c->s_comp, timed ? ev : nullptr, bad)))
            return rc;
        HIPCHK(c, hipStreamSynchronize(c->s_comp));
        float ms = 0;
        if (timed && hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) info.decode_ms = ms;
    }
    info.first_bad = bad[0];
    info.bad_blocks = bad[1];
    c->lz4_last = info;
    if (first_bad) *first_bad = bad[0];
    if (bad[1])
        return fail(c, YSB_ERR_FORMAT, "LZ4 block %u of %u breaks the block format (%u bad in all)", bad[0], n_blocks, bad[1]);
    return YSB_OK;
}

int ysb_lz4_info(ysb_ctx* c, ysb_lz4_desc* info) {
    if (!c || !info) return c ? fail(c, YSB_ERR_ARG, "info is NULL") : YSB_ERR_ARG;
    const int rc = sync_streams(c);   // (a compressed batch awaiting its launch settles here)
    *info = c->lz4_last;
    return rc;
}

uint64_t ysb_lz4_desc_size(void) { return sizeof(ysb_lz4_desc); }

uint32_t ysb_lz4_compress_bound(uint32_t raw_bytes) { return lz4_compress_bound(raw_bytes); }

int ysb_lz4_compress_block(const uint8_t* src, uint32_t raw_bytes, uint8_t* dst, uint32_t cap, int allow_stored,
                           ysb_lz4_block* entry) {
    if (!src || !dst || !entry || raw_bytes < 1 || raw_bytes > LZ4_MAX_RAW)
        return fail(nullptr, YSB_ERR_ARG, "ysb_lz4_compress_block: NULL buffers or raw_bytes not in 1..65536");
    if (cap < lz4_compress_bound(raw_bytes)) return fail(nullptr, YSB_ERR_CAPACITY, "cap below ysb_lz4_compress_bound");
    *entry = lz4_pack_block(src, raw_bytes, dst, allow_stored != 0);
    return YSB_OK;
}

int ysb_lz4_decompress_block(const uint8_t* src, const ysb_lz4_block* entry, uint8_t* dst, uint32_t cap) {
    if (!src || !dst || !entry) return fail(nullptr, YSB_ERR_ARG, "ysb_lz4_decompress_block: NULL argument");
    if (!lz4_entry_ok(*entry)) return fail(nullptr, YSB_ERR_FORMAT, "raw_bytes %u, not in 1..65536", entry->raw_bytes);
    if (cap < entry->raw_bytes) return fail(nullptr, YSB_ERR_CAPACITY, "cap below raw_bytes");
    if (!lz4_decode_block(src, *entry, dst)) return fail(nullptr, YSB_ERR_FORMAT, "the block breaks the LZ4 block format");
    return YSB_OK;
}

int ysb_lz4_pack(const uint8_t* src, uint64_t nbytes, uint32_t block_bytes, int line_aligned, int allow_stored,
                 int threads, uint8_t* dst, uint64_t dst_cap, uint64_t* dst_bytes, ysb_lz4_block* dir, uint64_t dir_cap,
                 uint64_t* n_blocks) {
    if ((nbytes && !src) || !dst_bytes || !n_blocks || block_bytes < 1 || block_bytes > LZ4_MAX_RAW)
        return fail(nullptr, YSB_ERR_ARG, "ysb_lz4_pack: NULL argument or block_bytes not in 1..65536");
    // the blocks' ranges first (line alignment makes them data-dependent) ...
    std::vector<u64> cut{0};
    while (cut.back() < nbytes) cut.push_back(lz4_block_end(src, nbytes, cut.back(), block_bytes, line_aligned != 0));
    const u64 n = cut.size() - 1;
    // ... each block at its worst-case place, compressed in parallel, then closed up in order
    const u64 need = nbytes + nbytes / 255 + 16 * n;
    *n_blocks = n;
    *dst_bytes = need;
    if (need > dst_cap || n > dir_cap || (n && (!dst || !dir)))
        return fail(nullptr, YSB_ERR_CAPACITY, "ysb_lz4_pack: needs %llu bytes and %llu directory entries",
                    (unsigned long long)need, (unsigned long long)n);
    auto place = [&](u64 i) { return cut[i] + cut[i] / 255 + 16 * i; };   // (>= the sum of the bounds before it)
    const int nt = (int)std::max<u64>(1, std::min<u64>({(u64)std::max(threads, 1), 16, n}));
    auto work = [&](int t) {
        for (u64 i = (u64)t; i < n; i += (u64)nt)
            dir[i] = lz4_pack_block(src + cut[i], (u32)(cut[i + 1] - cut[i]), dst + place(i), allow_stored != 0);
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < nt; ++t) pool.emplace_back(work, t);
    work(0);
    for (auto& th : pool) th.join();
    u64 o = 0;
    for (u64 i = 0; i < n; ++i) {
        const u32 cb = lz4_entry_comp(dir[i]);
        std::memmove(dst + o, dst + place(i), cb);
        o += cb;
    }
    *dst_bytes = o;
    return YSB_OK;
}

int ysb_lz4_write_file(const char* path, const uint8_t* src, uint64_t nbytes, uint32_t block_bytes, int line_aligned,
                       int allow_stored, int threads) {
    if (!path) return fail(nullptr, YSB_ERR_ARG, "ysb_lz4_write_file: NULL path");
    u64 need = 0, n = 0;
    int rc = ysb_lz4_pack(src, nbytes, block_bytes, line_aligned, allow_stored, threads, nullptr, 0, &need, nullptr, 0, &n);
    if (rc && rc != YSB_ERR_CAPACITY) return rc;
    std::vector<u8> blob(need);
    std::vector<ysb_lz4_block> dir(n);
    if ((rc = ysb_lz4_pack(src, nbytes, block_bytes, line_aligned, allow_stored, threads, blob.data(), blob.size(), &need,
                           dir.data(), dir.size(), &n)))
        return rc;
    ysb_lz4_file_header h{};
    std::memcpy(h.magic, YSB_LZ4_FILE_MAGIC, 8);
    h.version = 1;
    h.flags = line_aligned ? YSB_LZ4_FILE_LINE_ALIGNED : 0u;
    h.n_blocks = n;
    h.raw_bytes = nbytes;
    FILE* f = std::fopen(path, "wb");
    if (!f) return fail(nullptr, YSB_ERR_ARG, "cannot write %s", path);
    bool ok = std::fwrite(&h, sizeof h, 1, f) == 1;
    ok = ok && (!n || std::fwrite(dir.data(), sizeof(ysb_lz4_block), n, f) == n);
    ok = ok && (!need || std::fwrite(blob.data(), 1, need, f) == need);
    ok = (std::fclose(f) == 0) && ok;
    return ok ? YSB_OK : fail(nullptr, YSB_ERR_ARG, "short write to %s", path);
}

}  // extern "C"
