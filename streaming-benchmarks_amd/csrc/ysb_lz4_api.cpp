// ysb_lz4_api.cpp -- LZ4 batches above the kernel (ysb_lz4.hip; the rules: ysb_lz4.h): the
// directory's checks, a slot's staging (compressed bytes in pinned memory or left in place in a
// registered range, block descriptors in pinned memory, one copy each), the decode's one launch
// and read-back (launch_decode), the synchronous decode alone, the last batch's figures, and the
// host codec entries.  ysb_submit_raw_lz4 and ysb_submit_lz4_mapped sit beside ysb_submit_raw in
// ysb_raw.cpp.  Standard frames (ysb_lz4_frame.h): the index, the writer and the host models as C
// entries, and the synchronous measure and measure + decode.
#include "ysb_ctx.h"
#include "ysb_lz4.h"
#include "ysb_lz4_frame.h"

using namespace ysb;

constexpr u64 LZ4F_HEAD = sizeof(Lz4FrameHead);   // a frame batch's head in front of its index entries
static_assert(LZ4F_HEAD % 8 == 0, "the index entries behind the head hold 64-bit offsets");
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
// to h_bad queued behind it.  ev: YSB_F_TIMING's marks around the kernel, or NULL.
static int launch_decode(ysb_ctx* c, const u8* d_comp, u8* d_descs, u32 n_blocks, u32 max_raw, u8* d_out, hipStream_t s,
                         Event* ev, u32* h_bad) {
    HIPCHK(c, mark(ev, 0, s));
    u32* bad = reinterpret_cast<u32*>(d_descs);
    const Lz4Params lp{d_comp, reinterpret_cast<const Lz4Desc*>(d_descs + LZ4_DESC_HEAD), n_blocks, max_raw, d_out, bad, c->lz4_decoder};
    HIPCHK(c, launch_lz4_decode(lp, s));
    HIPCHK(c, mark(ev, 1, s));
    HIPCHK(c, hipMemcpyAsync(h_bad, bad, 8, hipMemcpyDeviceToHost, s));
    return YSB_OK;
}

// The descriptors' pinned / device buffers of a slot grown to `need` bytes (outside steady
// state: a batch with more blocks than any before).
static int grow_descs(ysb_ctx* c, int slot, u64 need) {
    if (need <= c->lz4desc_cap[slot]) return YSB_OK;
    const u64 cap = std::max<u64>(need + need / 2, 64u << 10);
    if (int rc = grow_device(c, c->d_lz4desc[slot], cap + 64, 0)) return rc;
    HIPCHK(c, c->h_lz4desc[slot].alloc(cap + 64));
    HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&c->hd_lz4desc[slot]), c->h_lz4desc[slot], 0));
    c->lz4desc_cap[slot] = cap;
    return YSB_OK;
}

int lz4_stage(ysb_ctx* c, int slot, const uint8_t* bytes, uint64_t comp_bytes, const ysb_lz4_block* dir,
              uint32_t n_blocks, const uint8_t* dsrc, RawBatch* batch, SlotCopy v[2], std::vector<u8>* sample) {
    u64 raw_total = 0;
    int rc = dir_args(c, bytes, comp_bytes, dir, n_blocks, &raw_total);
    if (rc) return rc;
    if (comp_bytes > c->cfg.max_batch_bytes || raw_total > c->cfg.max_batch_bytes)
        return fail(c, YSB_ERR_CAPACITY, "LZ4 batch of %llu B (%llu B decoded) exceeds max_batch_bytes",
                    (unsigned long long)comp_bytes, (unsigned long long)raw_total);
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = ensure_wire(c, slot))) return rc;
    if (!c->h_lz4bad) {
        HIPCHK(c, c->h_lz4bad.alloc(16));
        std::memset(c->h_lz4bad, 0, 16);
    }
    const u64 desc_bytes = LZ4_DESC_HEAD + (u64)n_blocks * sizeof(Lz4Desc);
    if ((rc = grow_descs(c, slot, desc_bytes))) return rc;
    batch->nbytes = raw_total;
    Lz4Staged* out = &batch->lz4.emplace();
    fill_descs(dir, n_blocks, c->h_lz4desc[slot], &out->info, &out->max_raw);
    v[0] = stage_wire(c, slot, bytes, comp_bytes, dsrc);
    v[1] = {c->d_lz4desc[slot], c->hd_lz4desc[slot], c->h_lz4desc[slot], n_blocks ? desc_bytes : 0};
    // the layout sample: block 0 as the host model decodes it (nothing if it is bad -- the
    // device decides that for the batch)
    sample->clear();
    if (n_blocks) {
        sample->resize(dir[0].raw_bytes);
        if (!lz4_decode_block(static_cast<const u8*>(v[0].hsrc), dir[0], sample->data())) sample->clear();
    }
    return YSB_OK;
}

// ---- frame batches through the slots (ysb_submit_lz4_blocks) ----------------------------------
// d_lz4desc[slot]: the batch's Lz4FrameHead, then its index entries (offsets from the span's
// start); d_lz4f[slot]: the descriptors, then the measured sizes.

// The index entries of a call as argument errors: every block's size rule and, for a slot batch
// (in_order: a run of consecutive index entries), that each lies behind the one before; how
// many are stored and their compressed bytes into *stored and *comp_bytes.
static int frame_blocks(ysb_ctx* c, const ysb_lz4_frame_block* blocks, u32 n, bool in_order, u64* stored, u64* comp_bytes) {
    *stored = *comp_bytes = 0;
    for (u32 i = 0; i < n; ++i) {
        const u32 comp = blocks[i].comp_bytes & ~LZ4_STORED;
        if (comp < 1 || comp > LZ4F_BLOCK_MAX)
            return fail(c, YSB_ERR_ARG, "frame block %u: %u bytes, not in 1..%u", i, comp, LZ4F_BLOCK_MAX);
        if (in_order && i && blocks[i].offset < blocks[i - 1].offset + (blocks[i - 1].comp_bytes & ~LZ4_STORED) + 4)
            return fail(c, YSB_ERR_ARG, "frame block %u does not lie behind block %u: a batch is a run of consecutive index entries", i, i - 1);
        *stored += (blocks[i].comp_bytes & LZ4_STORED) ? 1 : 0;
        *comp_bytes += comp;
    }
    return YSB_OK;
}

int lz4f_stage(ysb_ctx* c, int slot, const uint8_t* base, const ysb_lz4_frame_block* blocks, uint32_t n, uint32_t flags,
               const uint8_t* dsrc, RawBatch* batch, SlotCopy v[2], std::vector<u8>* sample) {
    if (n && (!base || !blocks)) return fail(c, YSB_ERR_ARG, "NULL frame buffers");
    if (flags & ~YSB_LZ4F_MORE) return fail(c, YSB_ERR_ARG, "unknown flags %#x", flags);
    ysb_lz4_desc info{};
    info.blocks = n;
    info.first_bad = LZ4_NO_BAD;
    int rc = frame_blocks(c, blocks, n, true, &info.stored_blocks, &info.comp_bytes);
    if (rc) return rc;
    const u64 first = n ? blocks[0].offset : 0;
    const u64 span = n ? blocks[n - 1].offset + (blocks[n - 1].comp_bytes & ~LZ4_STORED) - first : 0;
    const u64 bound = ((u64)n + 1) * LZ4_MAX_RAW;
    if (span > c->cfg.max_batch_bytes || bound > c->cfg.max_batch_bytes)
        return fail(c, YSB_ERR_CAPACITY, "frame batch of %u blocks (%llu B; up to %llu B decoded with the carry) exceeds max_batch_bytes",
                    n, (unsigned long long)span, (unsigned long long)bound);
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = ensure_wire(c, slot))) return rc;
    if (!c->h_lz4f) {
        HIPCHK(c, c->h_lz4f.alloc(2 * LZ4F_HEAD));
        std::memset(c->h_lz4f.get(), 0, 2 * LZ4F_HEAD);
    }
    if (!c->d_carry) {
        HIPCHK(c, c->d_carry.alloc(LZ4_CARRY_HEAD + LZ4_CARRY_MAX));
        HIPCHK(c, hipMemset(c->d_carry, 0, LZ4_CARRY_HEAD));
    }
    const u64 index_bytes = LZ4F_HEAD + (u64)n * sizeof(Lz4FrameBlock);
    rc = grow_descs(c, slot, index_bytes);
    if (!rc) rc = grow_device(c, c->d_lz4f[slot], (u64)n * (sizeof(Lz4Desc) + 4) + 64, 64u << 10);
    if (rc) return rc;
    v[0] = stage_wire(c, slot, n ? base + first : nullptr, span, dsrc);
    v[1] = {c->d_lz4desc[slot], c->hd_lz4desc[slot], c->h_lz4desc[slot], index_bytes};
    const u8* hsrc = static_cast<const u8*>(v[0].hsrc);
    Lz4FrameHead head{};
    head.bad[0] = LZ4_NO_BAD;
    std::memcpy(c->h_lz4desc[slot], &head, LZ4F_HEAD);
    for (u32 i = 0; i < n; ++i) {
        const Lz4FrameBlock e{blocks[i].offset - first, blocks[i].comp_bytes, 0};
        std::memcpy(c->h_lz4desc[slot] + LZ4F_HEAD + (u64)i * sizeof e, &e, sizeof e);
    }
    batch->nbytes = bound;
    Lz4Staged* out = &batch->lz4.emplace();
    out->info = info;
    out->max_raw = LZ4_MAX_RAW;
    out->frame = true;
    out->decoder = lz4_pick_decoder(LZ4_MAX_RAW, c->lz4_decoder);
    out->more = (flags & YSB_LZ4F_MORE) != 0;
    // the layout sample: block 0 as the host model measures and decodes it, from behind its
    // first terminator when the batch before left a carry (its head is the tail of a line)
    sample->clear();
    if (n) {
        const u32 raw = lz4_measure_block(hsrc, blocks[0].comp_bytes);
        sample->resize(raw);
        if (raw && !lz4_decode_block(hsrc, ysb_lz4_block{blocks[0].comp_bytes, raw}, sample->data())) sample->clear();
        if (c->lz4f_more && !sample->empty()) {
            size_t k = 0;
            while (k < sample->size() && (*sample)[k] != '\n' && (*sample)[k] != '\r') ++k;
            sample->erase(sample->begin(), sample->begin() + std::min(sample->size(), k + 1));
        }
    }
    return YSB_OK;
}

int lz4f_readback(ysb_ctx* c, int slot, hipStream_t s) {
    HIPCHK(c, hipMemcpyAsync(c->h_lz4f + slot, c->d_lz4desc[slot], LZ4F_HEAD, hipMemcpyDeviceToHost, s));
    return YSB_OK;
}

// YSB_F_TIMING's marks of the slot's LZ4 batch (ev_lz4[slot]; NULL: not timed): a directory batch's
// decode lies between marks 0 and 1, a frame batch's measure + descriptors there and its decode
// between marks 1 and 2
static Event* lz4_marks(ysb_ctx* c, int slot) { return (c->cfg.flags & YSB_F_TIMING) ? c->ev_lz4[slot] : nullptr; }

// measure, descriptors, decode behind the carry's length, carry in and out: on s behind the slot's
// copies; *d_nbytes: the batch's byte count in its head on the device
static int lz4f_enqueue(ysb_ctx* c, int slot, const Lz4Staged& b, hipStream_t s, const u64** d_nbytes) {
    const u32 n = (u32)b.info.blocks;
    Lz4FrameHead* head = reinterpret_cast<Lz4FrameHead*>(c->d_lz4desc[slot].get());
    const Lz4FrameBlock* blocks = reinterpret_cast<const Lz4FrameBlock*>(c->d_lz4desc[slot] + LZ4F_HEAD);
    Lz4Desc* desc = reinterpret_cast<Lz4Desc*>(c->d_lz4f[slot].get());
    u32* raw = reinterpret_cast<u32*>(c->d_lz4f[slot] + (u64)n * sizeof(Lz4Desc));
    Event* ev = lz4_marks(c, slot);
    HIPCHK(c, mark(ev, 0, s));
    HIPCHK(c, launch_lz4_measure(c->d_wire[slot], blocks, n, raw, s));
    HIPCHK(c, launch_lz4_frame_descs(blocks, raw, n, 0, desc, &head->raw_total, s, reinterpret_cast<const u64*>(c->d_carry.get())));
    HIPCHK(c, mark(ev, 1, s));
    const Lz4Params lp{c->d_wire[slot], desc, n, LZ4_MAX_RAW, c->d_bytes[slot], head->bad, b.decoder};
    HIPCHK(c, launch_lz4_decode(lp, s));
    HIPCHK(c, mark(ev, 2, s));
    HIPCHK(c, launch_lz4_frame_carry(c->d_bytes[slot], c->d_carry, head, b.more ? 1u : 0u, s));
    *d_nbytes = &head->nbytes;
    return YSB_OK;
}

// at a frame batch's launch: lz4f_last <- its figures; a bad block or a carry above 64 KiB drops it
static int lz4f_settle(ysb_ctx* c, int slot, const Lz4Staged& b, u64* nbytes) {
    const Lz4FrameHead h = c->h_lz4f[slot];
    *nbytes = h.nbytes;
    ysb_lz4_frame_desc d{};
    d.blocks = b.info.blocks;
    d.stored_blocks = b.info.stored_blocks;
    d.comp_bytes = b.info.comp_bytes;
    d.raw_bytes = h.raw_total;
    d.bad_blocks = h.bad[1];
    d.first_bad = h.bad[0];
    d.decoder = d.blocks ? b.decoder : 0;
    d.carry_in = h.carry_in;
    d.carry_out = h.carry_out;
    d.batches = c->lz4f_last.batches + 1;
    add_span(lz4_marks(c, slot), 0, 1, &d.measure_ms);
    add_span(lz4_marks(c, slot), 1, 2, &d.decode_ms);
    c->lz4f_last = d;
    if (h.bad[1])
        return fail(c, YSB_ERR_FORMAT, "frame batch (slot %d): block %u of %llu breaks the block format (%u bad in all); "
                    "the batch was dropped", slot, h.bad[0], (unsigned long long)d.blocks, h.bad[1]);
    if (h.overflow)
        return fail(c, YSB_ERR_CAPACITY, "frame batch (slot %d): more than %u bytes behind its last line terminator; "
                    "the batch was dropped", slot, LZ4_CARRY_MAX);
    return YSB_OK;
}

int lz4_enqueue_decode(ysb_ctx* c, int slot, const Lz4Staged& b, hipStream_t s, const u64** d_nbytes) {
    if (b.frame) return lz4f_enqueue(c, slot, b, s, d_nbytes);
    c->h_lz4bad[2 * slot] = LZ4_NO_BAD;
    c->h_lz4bad[2 * slot + 1] = 0;
    if (!b.info.blocks) return YSB_OK;
    // the bad-block pair comes back through pinned memory with the line count: no host wait here
    return launch_decode(c, c->d_wire[slot], c->d_lz4desc[slot], (u32)b.info.blocks, b.max_raw, c->d_bytes[slot], s,
                         lz4_marks(c, slot), c->h_lz4bad + 2 * slot);
}

int lz4_settle(ysb_ctx* c, int slot, const Lz4Staged& b, u64* nbytes) {
    if (b.frame) return lz4f_settle(c, slot, b, nbytes);
    ysb_lz4_desc d = b.info;
    *nbytes = d.raw_bytes;
    d.batches = c->lz4_last.batches + 1;
    d.first_bad = c->h_lz4bad[2 * slot];
    d.bad_blocks = c->h_lz4bad[2 * slot + 1];
    if (d.blocks) add_span(lz4_marks(c, slot), 0, 1, &d.decode_ms);   // (no blocks: no decode ran, the marks are an earlier batch's)
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
        Event marks[2];
        Event* ev = (c->cfg.flags & YSB_F_TIMING) ? marks : nullptr;
        if ((rc = launch_decode(c, d_comp, c->d_lz4desc_sync, n_blocks, max_raw, d_out, c->s_comp, ev, bad))) return rc;
        HIPCHK(c, hipStreamSynchronize(c->s_comp));
        add_span(ev, 0, 1, &info.decode_ms);
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

// ---- standard frames ------------------------------------------------------------------------

static_assert(sizeof(Lz4FrameBlock) == sizeof(ysb_lz4_frame_block) && offsetof(Lz4FrameBlock, comp) == offsetof(ysb_lz4_frame_block, comp_bytes),
              "the kernels read the public index entry");

int ysb_lz4_frame_index(const uint8_t* bytes, uint64_t nbytes, ysb_lz4_frame_block* blocks, uint64_t cap,
                        uint64_t* n_blocks, ysb_lz4_frame_summary* info) {
    if (nbytes && !bytes) return fail(nullptr, YSB_ERR_ARG, "ysb_lz4_frame_index: NULL buffer");
    Lz4fError err;
    const int rc = lz4f_index(bytes, nbytes, blocks, blocks ? cap : 0, n_blocks, info, &err);
    return rc ? fail(nullptr, rc, "%s", err.msg) : YSB_OK;
}

uint64_t ysb_lz4_frame_bound(uint64_t nbytes, uint32_t block_bytes) { return lz4f_bound(nbytes, block_bytes); }

int ysb_lz4_frame_pack(const uint8_t* src, uint64_t nbytes, uint32_t block_bytes, int threads, uint8_t* dst,
                       uint64_t dst_cap, uint64_t* dst_bytes) {
    if ((nbytes && !src) || !dst_bytes || block_bytes < 1 || block_bytes > LZ4_MAX_RAW)
        return fail(nullptr, YSB_ERR_ARG, "ysb_lz4_frame_pack: NULL argument or block_bytes not in 1..65536");
    *dst_bytes = lz4f_bound(nbytes, block_bytes);
    if (*dst_bytes > dst_cap || !dst)
        return fail(nullptr, YSB_ERR_CAPACITY, "ysb_lz4_frame_pack: needs %llu bytes", (unsigned long long)*dst_bytes);
    *dst_bytes = lz4f_pack(src, nbytes, block_bytes, threads, dst);
    return YSB_OK;
}

int ysb_lz4_frame_write(const char* path, const uint8_t* src, uint64_t nbytes, uint32_t block_bytes, int threads) {
    if (!path) return fail(nullptr, YSB_ERR_ARG, "ysb_lz4_frame_write: NULL path");
    if ((nbytes && !src) || block_bytes < 1 || block_bytes > LZ4_MAX_RAW)
        return fail(nullptr, YSB_ERR_ARG, "ysb_lz4_frame_write: NULL source or block_bytes not in 1..65536");
    std::vector<u8> blob(lz4f_bound(nbytes, block_bytes));
    const u64 n = lz4f_pack(src, nbytes, block_bytes, threads, blob.data());
    FILE* f = std::fopen(path, "wb");
    if (!f) return fail(nullptr, YSB_ERR_ARG, "cannot write %s", path);
    bool ok = std::fwrite(blob.data(), 1, n, f) == n;
    ok = (std::fclose(f) == 0) && ok;
    return ok ? YSB_OK : fail(nullptr, YSB_ERR_ARG, "short write to %s", path);
}

int ysb_lz4_measure_block(const uint8_t* src, uint32_t comp_field, uint32_t* raw_bytes) {
    if (!src || !raw_bytes) return fail(nullptr, YSB_ERR_ARG, "ysb_lz4_measure_block: NULL argument");
    *raw_bytes = lz4_measure_block(src, comp_field);
    return *raw_bytes ? YSB_OK : fail(nullptr, YSB_ERR_FORMAT, "the block breaks the LZ4 block format");
}

uint64_t ysb_lz4_frame_carry_cut(const uint8_t* data, uint64_t n, int more) { return data ? lz4f_carry_cut(data, n, more != 0) : 0; }

int ysb_lz4_set_decoder(ysb_ctx* c, int decoder) {
    if (!c) return YSB_ERR_ARG;
    if (decoder < YSB_LZ4_DECODER_AUTO || decoder > YSB_LZ4_DECODER_WIDE)
        return fail(c, YSB_ERR_ARG, "decoder must be 0 (auto), 1 (one wave per block) or 2 (several waves)");
    c->lz4_decoder = (u32)decoder;
    return YSB_OK;
}

// The synchronous calls' device scratch (d_lz4f_sync): a 16-byte head {first bad, bad blocks,
// raw total (u64)}, then the index entries, the descriptors and the measured sizes.
struct FrameScratch {
    u32* bad;
    u64* total;
    Lz4FrameBlock* blocks;
    Lz4Desc* desc;
    u32* raw;
};

static int frame_scratch(ysb_ctx* c, const ysb_lz4_frame_block* blocks, u32 n, FrameScratch* fs) {
    const u64 need = 16 + (u64)n * (sizeof(Lz4FrameBlock) + sizeof(Lz4Desc) + 4);
    int rc = grow_device(c, c->d_lz4f_sync, need, 64u << 10);
    if (rc) return rc;
    u8* p = c->d_lz4f_sync;
    fs->bad = reinterpret_cast<u32*>(p);
    fs->total = reinterpret_cast<u64*>(p + 8);
    fs->blocks = reinterpret_cast<Lz4FrameBlock*>(p + 16);
    fs->desc = reinterpret_cast<Lz4Desc*>(p + 16 + (u64)n * sizeof(Lz4FrameBlock));
    fs->raw = reinterpret_cast<u32*>(p + 16 + (u64)n * (sizeof(Lz4FrameBlock) + sizeof(Lz4Desc)));
    static const u32 head[4] = {LZ4_NO_BAD, 0, 0, 0};   // (static: the copy is asynchronous)
    HIPCHK(c, hipMemcpyAsync(p, head, 16, hipMemcpyHostToDevice, c->s_comp));
    HIPCHK(c, hipMemcpyAsync(fs->blocks, blocks, (u64)n * sizeof(Lz4FrameBlock), hipMemcpyHostToDevice, c->s_comp));
    return YSB_OK;
}

static int frame_args(ysb_ctx* c, const uint8_t* d_base, const ysb_lz4_frame_block* blocks, u32 n, ysb_lz4_frame_desc* info) {
    if (n && (!d_base || !blocks)) return fail(c, YSB_ERR_ARG, "NULL frame buffers");
    *info = ysb_lz4_frame_desc{};
    info->blocks = n;
    info->first_bad = LZ4_NO_BAD;
    return frame_blocks(c, blocks, n, false, &info->stored_blocks, &info->comp_bytes);
}

// measure + descriptors on s_comp between marks 0 and 1 of ev (YSB_F_TIMING; NULL: not timed)
static int frame_measure(ysb_ctx* c, const uint8_t* d_base, u32 n, const FrameScratch& fs, Event* ev) {
    HIPCHK(c, mark(ev, 0, c->s_comp));
    HIPCHK(c, launch_lz4_measure(d_base, fs.blocks, n, fs.raw, c->s_comp));
    HIPCHK(c, launch_lz4_frame_descs(fs.blocks, fs.raw, n, 0, fs.desc, fs.total, c->s_comp));
    HIPCHK(c, mark(ev, 1, c->s_comp));
    return YSB_OK;
}

int ysb_lz4_measure_device(ysb_ctx* c, const uint8_t* d_base, const ysb_lz4_frame_block* blocks, uint32_t n_blocks,
                           uint32_t* raw_out, uint32_t* first_bad) {
    if (!c) return YSB_ERR_ARG;
    ysb_lz4_frame_desc info;
    int rc = frame_args(c, d_base, blocks, n_blocks, &info);
    if (rc) return rc;
    if (n_blocks && !raw_out) return fail(c, YSB_ERR_ARG, "raw_out is NULL");
    if (first_bad) *first_bad = LZ4_NO_BAD;
    if ((rc = launch_pending_raw(c))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (n_blocks) {
        FrameScratch fs;
        const SyncOnExit settled{c->s_comp};
        if ((rc = frame_scratch(c, blocks, n_blocks, &fs))) return rc;
        Event marks[2];
        Event* ev = (c->cfg.flags & YSB_F_TIMING) ? marks : nullptr;
        if ((rc = frame_measure(c, d_base, n_blocks, fs, ev))) return rc;
        HIPCHK(c, hipMemcpyAsync(raw_out, fs.raw, (u64)n_blocks * 4, hipMemcpyDeviceToHost, c->s_comp));
        HIPCHK(c, hipMemcpyAsync(&info.raw_bytes, fs.total, 8, hipMemcpyDeviceToHost, c->s_comp));
        HIPCHK(c, hipStreamSynchronize(c->s_comp));
        add_span(ev, 0, 1, &info.measure_ms);
        for (u32 i = 0; i < n_blocks; ++i)
            if (!raw_out[i]) {
                if (!info.bad_blocks) info.first_bad = i;
                ++info.bad_blocks;
            }
    }
    c->lz4f_last = info;
    if (first_bad) *first_bad = (u32)info.first_bad;
    if (info.bad_blocks)
        return fail(c, YSB_ERR_FORMAT, "frame block %llu of %u breaks the block format (%llu bad in all)",
                    (unsigned long long)info.first_bad, n_blocks, (unsigned long long)info.bad_blocks);
    return YSB_OK;
}

int ysb_lz4_decode_blocks_device(ysb_ctx* c, const uint8_t* d_base, const ysb_lz4_frame_block* blocks, uint32_t n_blocks,
                                 uint8_t* d_out, uint64_t out_cap, uint64_t* raw_bytes, uint32_t* first_bad) {
    if (!c) return YSB_ERR_ARG;
    ysb_lz4_frame_desc info;
    int rc = frame_args(c, d_base, blocks, n_blocks, &info);
    if (rc) return rc;
    if (raw_bytes) *raw_bytes = 0;
    if (first_bad) *first_bad = LZ4_NO_BAD;
    if ((rc = launch_pending_raw(c))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (n_blocks) {
        FrameScratch fs;
        const SyncOnExit settled{c->s_comp};
        if ((rc = frame_scratch(c, blocks, n_blocks, &fs))) return rc;
        Event marks[4];   // the measure pass between marks 0 and 1, the decode (behind a host wait) between 2 and 3
        Event* ev = (c->cfg.flags & YSB_F_TIMING) ? marks : nullptr;
        if ((rc = frame_measure(c, d_base, n_blocks, fs, ev))) return rc;
        // the measured total decides the capacity before a byte is decoded (this call is synchronous)
        HIPCHK(c, hipMemcpyAsync(&info.raw_bytes, fs.total, 8, hipMemcpyDeviceToHost, c->s_comp));
        HIPCHK(c, hipStreamSynchronize(c->s_comp));
        if (raw_bytes) *raw_bytes = info.raw_bytes;
        if (info.raw_bytes > out_cap)
            return fail(c, YSB_ERR_CAPACITY, "%llu B decoded, cap %llu", (unsigned long long)info.raw_bytes,
                        (unsigned long long)out_cap);
        if (info.raw_bytes && !d_out) return fail(c, YSB_ERR_ARG, "NULL output buffer");
        HIPCHK(c, mark(ev, 2, c->s_comp));
        // (a block measured bad has raw 0: the decode kernel records it in the bad pair)
        const Lz4Params lp{d_base, fs.desc, n_blocks, LZ4_MAX_RAW, d_out, fs.bad, c->lz4_decoder};
        HIPCHK(c, launch_lz4_decode(lp, c->s_comp));
        HIPCHK(c, mark(ev, 3, c->s_comp));
        u32 bad[2] = {LZ4_NO_BAD, 0};
        HIPCHK(c, hipMemcpyAsync(bad, fs.bad, 8, hipMemcpyDeviceToHost, c->s_comp));
        HIPCHK(c, hipStreamSynchronize(c->s_comp));
        add_span(ev, 0, 1, &info.measure_ms);
        add_span(ev, 2, 3, &info.decode_ms);
        info.first_bad = bad[0];
        info.bad_blocks = bad[1];
        info.decoder = lz4_pick_decoder(LZ4_MAX_RAW, c->lz4_decoder);
    }
    c->lz4f_last = info;
    if (first_bad) *first_bad = (u32)info.first_bad;
    if (info.bad_blocks)
        return fail(c, YSB_ERR_FORMAT, "frame block %llu of %u breaks the block format (%llu bad in all)",
                    (unsigned long long)info.first_bad, n_blocks, (unsigned long long)info.bad_blocks);
    return YSB_OK;
}

int ysb_lz4_frame_info(ysb_ctx* c, ysb_lz4_frame_desc* info) {
    if (!c || !info) return c ? fail(c, YSB_ERR_ARG, "info is NULL") : YSB_ERR_ARG;
    const int rc = sync_streams(c);   // (a frame batch awaiting its launch settles here)
    *info = c->lz4f_last;
    return rc;
}

uint64_t ysb_lz4_frame_desc_size(void) { return sizeof(ysb_lz4_frame_desc); }

}  // extern "C"
