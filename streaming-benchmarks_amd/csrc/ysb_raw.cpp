// ysb_raw.cpp -- every batch that crosses PCIe into a slot and may launch a call later: raw
// lines split on the GPU (ysb_submit_raw), read in place from registered caller memory
// (ysb_submit_raw_mapped, ysb_submit_mapped; host registration, the rebase table), LZ4 batches
// decoded in front of the split (ysb_submit_raw_lz4, ysb_submit_lz4_mapped), Kafka record batches
// unframed in its place (ysb_submit_kafka, ysb_submit_kafka_mapped).  A deferred batch is
// one RawBatch per slot (ysb_ctx.h): enqueue_deferred states its order once, launch_pending_raw
// launches it at the next call.  The launch (enqueue_scan) and the slot copies: ysb_submit.cpp.
#include "ysb_ctx.h"

using namespace ysb;

extern "C" {

// ---- the slot's pending batch ------------------------------------------------------------------

// Lines a raw batch may hold: max_batch_events, or one per 32 bytes of the slot if that is
// more (an event line is > 60 bytes; the device's line-start array is 4 B per line, not per
// byte); at most one per byte.  A batch with more lines fails its launch (YSB_ERR_CAPACITY).
static u64 raw_line_cap(const ysb_config& cfg) {
    return std::min<u64>(cfg.max_batch_bytes + 1, std::max<u64>(cfg.max_batch_events, cfg.max_batch_bytes / 32) + 1);
}

static int ensure_raw(ysb_ctx* c) {
    if (c->h_rawn) return YSB_OK;
    HIPCHK(c, hipSetDevice(c->device));
    c->raw_lines_cap = raw_line_cap(c->cfg);
    for (int s = 0; s < 2; ++s) {   // (a failed earlier attempt may have left some of these)
        HIPCHK(c, c->d_roff[s].alloc(c->raw_lines_cap * 4));
        if (!c->ev_raw[s]) HIPCHK(c, c->ev_raw[s].create());
    }
    if (!c->s_split) HIPCHK(c, hipStreamCreateWithFlags(&c->s_split, hipStreamNonBlocking));
    const u64 chunk_bytes = (split_chunks(c->cfg.max_batch_bytes) + 1) * 4;
    const int rc = grow_device(c, c->d_split_chunk, chunk_bytes, 0);
    if (rc) return rc;
    HIPCHK(c, c->h_rawn.alloc(16));
    return YSB_OK;
}

// The raw batch waiting for its launch (if any): its line count is back from the device
// (ev_raw), so its scan is enqueued now -- the order of submission is kept.  A batch that
// cannot launch (more lines than raw_lines_cap, a failed enqueue) is dropped and its error
// is sticky: every later call on the context that would order work after it returns it,
// until ysb_reset -- counts after a lost batch are not the stream's.
int launch_pending_raw(ysb_ctx* c) {
    if (c->raw_fail) return fail(c, c->raw_fail, "%s", c->raw_fail_msg.c_str());
    if (c->raw_pend < 0) return YSB_OK;
    // the batch is taken before anything is done with it: nothing called below finds it pending
    // again (enqueue_scan empties a due out-of-ring map through sync_streams, which comes here)
    const int slot = c->raw_pend;
    const RawBatch b = std::move(c->raw[slot]);
    c->raw_pend = -1;
    c->raw[slot] = RawBatch{};
    // the decoded bytes: a plain batch's as submitted; counted on the device for a frame or a
    // Kafka batch, whose settle step reads them from the pinned head that came back with the split's count
    u64 nbytes = b.nbytes;
    int rc = YSB_OK;
    if (hipSetDevice(c->device) != hipSuccess || hipEventSynchronize(c->ev_raw[slot]) != hipSuccess ||
        hipStreamWaitEvent(c->s_comp, c->ev_raw[slot], 0) != hipSuccess) {
        rc = fail(c, YSB_ERR_HIP, "raw batch (slot %d): waiting for its line split failed", slot);
    } else if (b.lz4 && (rc = lz4_settle(c, slot, *b.lz4, &nbytes))) {
        // a compressed batch with a bad block: dropped whole (YSB_ERR_FORMAT, the message lz4_settle's)
    } else if (b.kafka && (rc = kafka_settle(c, slot, *b.kafka, &nbytes))) {
        // a Kafka batch with a bad record: dropped whole (YSB_ERR_FORMAT, the message kafka_settle's)
    } else if (b.rebase && c->h_rawn[slot] > c->rebase_n - b.rebase->first_line) {
        rc = fail(c, YSB_ERR_ARG, "raw batch (slot %d): %llu lines, more than the rebase table holds from line %llu",
                  slot, (unsigned long long)c->h_rawn[slot], (unsigned long long)b.rebase->first_line);
    } else if (!b.off && c->h_rawn[slot] > c->raw_lines_cap) {   // (the caller's offsets: no d_roff to fit)
        rc = fail(c, YSB_ERR_CAPACITY, "raw batch (slot %d): %llu lines, more than the %llu its slot holds "
                  "(max(max_batch_events, max_batch_bytes / 32))", slot, (unsigned long long)c->h_rawn[slot],
                  (unsigned long long)c->raw_lines_cap);
    } else {
        const ysb_segment sg{c->d_bytes[slot], nbytes, b.off ? b.off : c->d_roff[slot].get(), c->h_rawn[slot]};
        rc = enqueue_scan(c, &sg, 1, b.lay);
    }
    // the slot's device buffers are free again once this launch (or nothing) has run
    if (hipEventRecord(c->ev_kdone[slot], c->s_comp) != hipSuccess && !rc)
        rc = fail(c, YSB_ERR_HIP, "hipEventRecord failed");
    if (rc) {
        c->raw_fail = rc;
        c->raw_fail_msg = c->err;
    }
    return rc;
}

static int raw_args(ysb_ctx* c, int slot, const uint8_t* bytes, uint64_t nbytes) {
    if (int rc = slot_arg(c, slot)) return rc;
    if (nbytes > c->cfg.max_batch_bytes)
        return fail(c, YSB_ERR_CAPACITY, "raw batch of %llu B exceeds max_batch_bytes", (unsigned long long)nbytes);
    if (nbytes && !bytes) return fail(c, YSB_ERR_ARG, "NULL batch buffer");
    if (!c->table_loaded) return fail(c, YSB_ERR_STATE, "ysb_load_ad_map has not been called");
    return carry_guard(c);
}

// The slot made the caller's to refill, once the entry's arguments are checked: its own earlier
// batch launches first if it is the pending one (its device buffers are about to be reused),
// its buffers and the split's exist, the context's device is current.
static int claim_slot(ysb_ctx* c, int slot) {
    int rc = c->raw_pend == slot ? launch_pending_raw(c) : YSB_OK;
    if (!rc) rc = ensure_slots(c);
    if (!rc) rc = ensure_raw(c);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    return YSB_OK;
}

// The rebase of a batch's lines in d_bytes[slot] on s from rb.first_line of the context's
// table: the caller's n device offsets, or (off NULL) the split's in d_roff[slot], as many as
// its count says.
static int rebase_lines(ysb_ctx* c, int slot, u64 nbytes, const u32* off, u64 n, const ysb_rebase& rb, hipStream_t s) {
    launch_rebase(c->d_bytes[slot], nbytes, off ? off : c->d_roff[slot].get(), off ? n : c->raw_lines_cap,
                  off ? nullptr : c->h_rawn + slot, off ? n : 0, c->d_rebase + rb.first_line, c->rebase_n - rb.first_line,
                  c->rebase_base + rb.lead_shift, c->cus, s);
    HIPCHK(c, hipGetLastError());
    return YSB_OK;
}

// The ONE statement of a deferred batch's order.  b says what the slot's nv copies carry
// (sample: its first lines on the host, 0 bytes: none).  The copies once the slot's previous
// kernel has run.  Everything behind them on a stream of the split's own, so the next slot's
// copy queues right behind this one: the decode of a compressed batch into the slot's device
// buffer, then the split as for any raw batch or, with b.off, the caller's device offsets into
// the (decoded) batch and no split, then the rebase on the (decoded) bytes.  Its scan launches at
// the next call, with offsets too: the verdict on a compressed batch's blocks must be known
// before its lines are counted.  The caller has claimed the slot.
// Round 5 kept the split on the copy stream: beside a copy kernel of one workgroup per CU the
// split was starved (its 32 us count took 2.7 ms, and the slot's scan waited behind it).  The
// copy kernel's grid is now 32 workgroups (H2D_WGS): still far more bytes in flight than PCIe's
// bandwidth x latency, and the HBM work beside it (split, scan) no longer queues behind its slow
// requests.  Same-box A/B (profiles/AB_LOG.md, round 6): raw host-staged 210 -> 214-218 M events/s, the
// raw streaming replay 197 -> 206-209 (copy queue busy 0.958 -> 0.986).
static int enqueue_deferred(ysb_ctx* c, int slot, RawBatch b, const SlotCopy* v, int nv, const u8* sample, u64 sample_bytes) {
    int rc;
    if (sample_bytes) sampled_layout(c, sample, sample_bytes, &b.lay);
    if ((rc = copy_slot_ranges(c, slot, v, nv))) return rc;
    hipStream_t s = c->s_split;
    HIPCHK(c, hipStreamWaitEvent(s, c->ev_h2d[slot], 0));
    const u64* d_nbytes = nullptr;   // a frame batch: its byte count is measured on the device, where the split reads it
    if (b.lz4 && (rc = lz4_enqueue_decode(c, slot, *b.lz4, s, &d_nbytes))) return rc;
    // a Kafka batch's kernels leave the values in the slot's device buffer and their offsets in
    // d_roff[slot], which is b.off: no split
    if (b.kafka && (rc = kafka_enqueue(c, slot, *b.kafka, s))) return rc;
    // the line count goes straight to pinned memory (read at the launch): the caller's (0: an
    // empty batch) or the split's
    if (b.off || !b.nbytes) c->h_rawn[slot] = b.n_off;
    else HIPCHK(c, launch_split_lines(c->d_bytes[slot], b.nbytes, c->d_split_chunk, c->d_roff[slot], c->raw_lines_cap,
                                      c->h_rawn + slot, s, d_nbytes));
    if (d_nbytes && (rc = lz4f_readback(c, slot, s))) return rc;
    if (b.rebase && (b.off || b.nbytes) && (rc = rebase_lines(c, slot, b.nbytes, b.off, b.n_off, *b.rebase, s))) return rc;
    HIPCHK(c, hipEventRecord(c->ev_raw[slot], s));
    c->raw[slot] = b;
    // the other slot's batch, submitted before this one, launches now; this one at the next call
    rc = launch_pending_raw(c);
    c->raw_pend = slot;
    return rc;
}

// ---- raw batches (ysb_submit_raw): the line split on the GPU ----------------------------------

// A raw batch from hsrc (host address: the layout sample, the DMA engine) / dsrc (its device
// address: the copy kernel) into the slot's device buffer, split, optionally rebased.
static int enqueue_plain(ysb_ctx* c, int slot, const u8* hsrc, const u8* dsrc, u64 nbytes, const ysb_rebase* rb) {
    RawBatch b;
    b.nbytes = nbytes;
    if (rb) b.rebase = *rb;
    const SlotCopy v{c->d_bytes[slot], dsrc, hsrc, nbytes};
    return enqueue_deferred(c, slot, b, &v, 1, hsrc, nbytes);
}

int ysb_submit_raw(ysb_ctx* c, int slot, const uint8_t* bytes, uint64_t nbytes) {
    if (!c) return YSB_ERR_ARG;
    int rc = raw_args(c, slot, bytes, nbytes);
    if (!rc) rc = claim_slot(c, slot);
    if (rc) return rc;
    // the slot's previous H2D must be done before its pinned buffer is rewritten
    HIPCHK(c, hipEventSynchronize(c->ev_h2d[slot]));
    if (bytes != c->h_bytes[slot] && nbytes) std::memcpy(c->h_bytes[slot], bytes, nbytes);
    return enqueue_plain(c, slot, c->h_bytes[slot], c->hd_bytes[slot], nbytes, nullptr);
}

// ---- batches staged in front of the split: LZ4, standard frames, Kafka ------------------------

// What every such submit does once its own arguments are checked: the slot claimed, the batch
// staged by the entry's own step -- stage(batch, v, sample) fills the RawBatch, the slot's two
// copies (the wire bytes, from the slot's pinned buffer or in place from a registered range,
// and the descriptors or index: what crosses PCIe) and the layout sample --, enqueued.
extern "C++" template <class Stage>
static int submit_staged(ysb_ctx* c, int slot, Stage stage) {
    int rc = claim_slot(c, slot);
    if (rc) return rc;
    // the slot's previous H2D must be done before its pinned buffers are rewritten (a batch read
    // in place: the descriptors' or the index's; so at most two copies are in flight)
    HIPCHK(c, hipEventSynchronize(c->ev_h2d[slot]));
    RawBatch b;
    SlotCopy v[2];
    std::vector<u8> sample;
    if ((rc = stage(&b, v, &sample))) return rc;
    return enqueue_deferred(c, slot, b, v, 2, sample.data(), sample.size());
}

// ---- LZ4-compressed raw batches (ysb_lz4_api.cpp lz4_stage; ysb_lz4.hip) ----------------------

// both compressed submits once their own arguments are checked (dsrc: lz4_stage)
static int submit_lz4(ysb_ctx* c, int slot, const uint8_t* bytes, u64 comp_bytes, const ysb_lz4_block* dir, u32 n_blocks,
                      const u8* dsrc, const u32* d_line_off, u64 n, const ysb_rebase* rb) {
    return submit_staged(c, slot, [&](RawBatch* b, SlotCopy* v, std::vector<u8>* sample) -> int {
        if (int rc = lz4_stage(c, slot, bytes, comp_bytes, dir, n_blocks, dsrc, b, v, sample)) return rc;
        b->off = d_line_off;
        b->n_off = n;
        if (rb) b->rebase = *rb;
        return YSB_OK;
    });
}

int ysb_submit_raw_lz4(ysb_ctx* c, int slot, const uint8_t* bytes, uint64_t comp_bytes, const ysb_lz4_block* dir,
                       uint32_t n_blocks) {
    if (!c) return YSB_ERR_ARG;
    if (int rc = slot_arg(c, slot)) return rc;
    if (!c->table_loaded) return fail(c, YSB_ERR_STATE, "ysb_load_ad_map has not been called");
    if (int rc = carry_guard(c)) return rc;
    return submit_lz4(c, slot, bytes, comp_bytes, dir, n_blocks, nullptr, nullptr, 0, nullptr);
}

// ---- standard-frame batches (ysb_lz4_api.cpp lz4f_stage; ysb_lz4_frame.h) ---------------------

static int mapped_src(ysb_ctx* c, const uint8_t* bytes, u64 nbytes, const u8** dsrc);

// Both frame submits: the slot claimed, the batch staged, enqueued like every deferred batch;
// whether a carry is pending afterwards is the flag's.
static int submit_frame(ysb_ctx* c, int slot, const uint8_t* base, const ysb_lz4_frame_block* blocks, u32 n_blocks,
                        u32 flags, bool mapped) {
    if (!c) return YSB_ERR_ARG;
    if (int rc = slot_arg(c, slot)) return rc;
    if (!c->table_loaded) return fail(c, YSB_ERR_STATE, "ysb_load_ad_map has not been called");
    const u8* dsrc = nullptr;
    if (mapped && n_blocks && base && blocks) {
        const u64 first = blocks[0].offset, last = blocks[n_blocks - 1].offset + (blocks[n_blocks - 1].comp_bytes & 0x7FFFFFFFu);
        if (last < first) return fail(c, YSB_ERR_ARG, "the frame blocks are not in order");
        if (int rc = mapped_src(c, base + first, last - first, &dsrc)) return rc;
    }
    bool staged = false;
    const int rc = submit_staged(c, slot, [&](RawBatch* b, SlotCopy* v, std::vector<u8>* sample) {
        const int rs = lz4f_stage(c, slot, base, blocks, n_blocks, flags, dsrc, b, v, sample);
        staged = !rs;
        return rs;
    });
    // only once the batch is on the device's queue (the slot was claimed, so it is this batch
    // that is pending there)
    if (staged && c->raw_pend == slot) c->lz4f_more = (flags & YSB_LZ4F_MORE) != 0;
    return rc;
}

int ysb_submit_lz4_blocks(ysb_ctx* c, int slot, const uint8_t* base, const ysb_lz4_frame_block* blocks, uint32_t n_blocks,
                          uint32_t flags) {
    return submit_frame(c, slot, base, blocks, n_blocks, flags, false);
}

int ysb_submit_lz4_blocks_mapped(ysb_ctx* c, int slot, const uint8_t* base, const ysb_lz4_frame_block* blocks,
                                 uint32_t n_blocks, uint32_t flags) {
    return submit_frame(c, slot, base, blocks, n_blocks, flags, true);
}

// ---- Kafka record batches (ysb_kafka_api.cpp kafka_stage; ysb_kafka.h) ------------------------

// What the four Kafka submits check in front: a raw batch's arguments, then (mapped) that the
// bytes lie in a registered range -- *dsrc their device alias there, else NULL.
static int kafka_args(ysb_ctx* c, int slot, const uint8_t* bytes, u64 nbytes, bool mapped, const u8** dsrc) {
    *dsrc = nullptr;
    const int rc = raw_args(c, slot, bytes, nbytes);
    return !rc && mapped ? mapped_src(c, bytes, nbytes, dsrc) : rc;
}

// Both Kafka submits: the framed bytes and the index are what crosses PCIe.
static int submit_kafka(ysb_ctx* c, int slot, const uint8_t* bytes, u64 nbytes, const ysb_kafka_batch* batches, u64 n_batches,
                        bool mapped) {
    if (!c) return YSB_ERR_ARG;
    const u8* dsrc = nullptr;
    if (int rc = kafka_args(c, slot, bytes, nbytes, mapped, &dsrc)) return rc;
    return submit_staged(c, slot, [&](RawBatch* b, SlotCopy* v, std::vector<u8>* sample) {
        return kafka_stage(c, slot, bytes, nbytes, batches, n_batches, dsrc, b, v, sample);
    });
}

int ysb_submit_kafka(ysb_ctx* c, int slot, const uint8_t* bytes, uint64_t nbytes, const ysb_kafka_batch* batches,
                     uint64_t n_batches) {
    return submit_kafka(c, slot, bytes, nbytes, batches, n_batches, false);
}

int ysb_submit_kafka_mapped(ysb_ctx* c, int slot, const uint8_t* bytes, uint64_t nbytes, const ysb_kafka_batch* batches,
                            uint64_t n_batches) {
    return submit_kafka(c, slot, bytes, nbytes, batches, n_batches, true);
}

// Both compressed Kafka submits (ysb_kafka_api.cpp kafka_lz4_stage; ysb_kafka_lz4.h): as
// submit_kafka, with the frames and the blocks beside the index; the inflate chain runs in
// enqueue_deferred's Kafka step (kafka_enqueue).
static int submit_kafka_lz4(ysb_ctx* c, int slot, const uint8_t* bytes, u64 nbytes, const ysb_kafka_batch* batches,
                            const ysb_kafka_frame* frames, u64 n_batches, const ysb_lz4_frame_block* blocks, u64 n_blocks,
                            bool mapped) {
    if (!c) return YSB_ERR_ARG;
    const u8* dsrc = nullptr;
    if (int rc = kafka_args(c, slot, bytes, nbytes, mapped, &dsrc)) return rc;
    return submit_staged(c, slot, [&](RawBatch* b, SlotCopy* v, std::vector<u8>* sample) {
        return kafka_lz4_stage(c, slot, bytes, nbytes, batches, frames, n_batches, blocks, n_blocks, dsrc, b, v, sample);
    });
}

int ysb_submit_kafka_lz4(ysb_ctx* c, int slot, const uint8_t* bytes, uint64_t nbytes, const ysb_kafka_batch* batches,
                         const ysb_kafka_frame* frames, uint64_t n_batches, const ysb_lz4_frame_block* blocks,
                         uint64_t n_blocks) {
    return submit_kafka_lz4(c, slot, bytes, nbytes, batches, frames, n_batches, blocks, n_blocks, false);
}

int ysb_submit_kafka_lz4_mapped(ysb_ctx* c, int slot, const uint8_t* bytes, uint64_t nbytes, const ysb_kafka_batch* batches,
                                const ysb_kafka_frame* frames, uint64_t n_batches, const ysb_lz4_frame_block* blocks,
                                uint64_t n_blocks) {
    return submit_kafka_lz4(c, slot, bytes, nbytes, batches, frames, n_batches, blocks, n_blocks, true);
}

// ---- zero-copy raw batches from registered caller memory (ABI 5) ----------------------------

int ysb_host_register(ysb_ctx* c, void* host, uint64_t bytes) {
    if (!c) return YSB_ERR_ARG;
    if (!host || !bytes) return fail(c, YSB_ERR_ARG, "empty host range");
    const uintptr_t a = reinterpret_cast<uintptr_t>(host);
    for (const auto& r : c->host_ranges)
        if (a < r.first + r.second.bytes && r.first < a + bytes) return fail(c, YSB_ERR_ARG, "host range overlaps a registered one");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipHostRegister(host, bytes, hipHostRegisterMapped));
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, host, 0) != hipSuccess) {
        hipHostUnregister(host);
        return fail(c, YSB_ERR_HIP, "hipHostGetDevicePointer of a registered range failed");
    }
    if ((reinterpret_cast<uintptr_t>(d) ^ a) & 15) {   // the copy's 16-byte widening assumes it
        hipHostUnregister(host);
        return fail(c, YSB_ERR_HIP, "the device alias of a registered range is not 16-byte congruent to it");
    }
    c->host_ranges[a] = {bytes, static_cast<u8*>(d)};
    return YSB_OK;
}

int ysb_host_unregister(ysb_ctx* c, void* host) {
    if (!c) return YSB_ERR_ARG;
    auto it = c->host_ranges.find(reinterpret_cast<uintptr_t>(host));
    if (it == c->host_ranges.end()) return fail(c, YSB_ERR_ARG, "not a registered range");
    // nothing queued may still read it
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->s_copy));
    HIPCHK(c, hipHostUnregister(host));
    c->host_ranges.erase(it);
    return YSB_OK;
}

int ysb_rebase_table(ysb_ctx* c, const uint32_t* time_at, uint64_t n_lines, int64_t lead_base) {
    if (!c) return YSB_ERR_ARG;
    if (n_lines && !time_at) return fail(c, YSB_ERR_ARG, "NULL table");
    HIPCHK(c, hipSetDevice(c->device));
    // batches queued with the old table must be done with it
    HIPCHK(c, hipStreamSynchronize(c->s_copy));
    if (c->s_split) HIPCHK(c, hipStreamSynchronize(c->s_split));
    c->d_rebase.reset();
    c->rebase_n = 0;
    if (!n_lines) return YSB_OK;
    u32 kmax = 0;
    for (u64 i = 0; i < n_lines; ++i) kmax = std::max(kmax, time_at[i] >> 16);
    if (lead_base < 0 || lead_base + kmax >= 1000000000LL) return fail(c, YSB_ERR_ARG, "leading digits out of [0, 10^9)");
    HIPCHK(c, c->d_rebase.alloc(n_lines * 4));
    HIPCHK(c, hipMemcpy(c->d_rebase, time_at, n_lines * 4, hipMemcpyHostToDevice));
    c->rebase_n = n_lines;
    c->rebase_base = lead_base;
    c->rebase_kmax = kmax;
    return YSB_OK;
}

// *dsrc <- the device alias of a mapped batch, or NULL when the batch widened to 16-byte
// boundaries on both sides (what the copy reads: launch_h2d_copy / launch_h2d_copy_unaligned) is
// not inside one registered range: the error for a batch with bytes, which must have one.
static int mapped_src(ysb_ctx* c, const uint8_t* bytes, u64 nbytes, const u8** dsrc) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(bytes);
    const uintptr_t lo = a & ~uintptr_t(15), hi = (a + nbytes + 15) & ~uintptr_t(15);
    auto it = c->host_ranges.upper_bound(a);
    const bool in = it != c->host_ranges.begin() && lo >= (--it)->first && hi <= it->first + it->second.bytes;
    *dsrc = in ? it->second.dptr + (a - it->first) : nullptr;
    if (nbytes && !in)
        return fail(c, YSB_ERR_ARG, "the batch (widened to 16-byte boundaries) is not inside a registered range");
    return YSB_OK;
}

// A mapped batch's rebase argument (NULL: none) against the context's table.  A raw batch
// (n_lines NULL: its line count is not known yet, launch_pending_raw checks it) must start
// inside the table; a batch with offsets must fit its *n_lines lines.
static int rebase_args(ysb_ctx* c, const ysb_rebase* rb, const u64* n_lines) {
    if (!rb) return YSB_OK;
    if (!c->d_rebase) return fail(c, YSB_ERR_STATE, "no rebase table (ysb_rebase_table)");
    if (!n_lines && rb->first_line >= c->rebase_n) return fail(c, YSB_ERR_ARG, "first_line beyond the rebase table");
    if (n_lines && (rb->first_line > c->rebase_n || *n_lines > c->rebase_n - rb->first_line))
        return fail(c, YSB_ERR_ARG, "the batch's lines run past the rebase table");
    const i64 lo = c->rebase_base + rb->lead_shift;
    if (lo < 0 || lo + (i64)c->rebase_kmax >= 1000000000LL)
        return fail(c, YSB_ERR_ARG, "rebased leading digits out of [0, 10^9)");
    return YSB_OK;
}

// (no host wait for the slot's previous copy: the bytes are the caller's, and the streaming
// replay's feeder thread runs through this call)
int ysb_submit_raw_mapped(ysb_ctx* c, int slot, const uint8_t* bytes, uint64_t nbytes, const ysb_rebase* rb) {
    if (!c) return YSB_ERR_ARG;
    int rc = raw_args(c, slot, bytes, nbytes);
    const u8* dsrc = nullptr;
    if (!rc) rc = mapped_src(c, bytes, nbytes, &dsrc);
    if (!rc) rc = rebase_args(c, rb, nullptr);
    if (!rc) rc = claim_slot(c, slot);
    if (rc) return rc;
    return enqueue_plain(c, slot, bytes, dsrc, nbytes, rb);
}

// A compressed batch read in place from a registered range: the union of
// ysb_submit_raw_lz4's rules and the mapped calls'.  The copy kernel (the DMA engine with
// YSB_F_H2D_SDMA) reads the blocks where they lie into d_wire[slot]; the slot's pinned byte
// buffer is not used and the host makes no pass over the bytes (block 0 apart: the layout
// sample).  d_line_off NULL: the GPU line split; otherwise n device offsets into the decoded batch.
int ysb_submit_lz4_mapped(ysb_ctx* c, int slot, const uint8_t* bytes, uint64_t comp_bytes, const ysb_lz4_block* dir,
                          uint32_t n_blocks, const uint32_t* d_line_off, uint64_t n, const ysb_rebase* rb) {
    if (!c) return YSB_ERR_ARG;
    if (int rc = slot_arg(c, slot)) return rc;
    if (!c->table_loaded) return fail(c, YSB_ERR_STATE, "ysb_load_ad_map has not been called");
    if (int g = carry_guard(c)) return g;
    if (comp_bytes && !bytes) return fail(c, YSB_ERR_ARG, "NULL batch buffer");
    if (!d_line_off && n) return fail(c, YSB_ERR_ARG, "n_events without line offsets (NULL d_line_off: the GPU split, n_events 0)");
    if (d_line_off && !n) return fail(c, YSB_ERR_ARG, "line offsets without n_events");
    if (n > 0x7FFFFFFFull) return fail(c, YSB_ERR_CAPACITY, "at most 2^31-1 events per batch");
    const u8* dsrc = nullptr;
    int rc = mapped_src(c, bytes, comp_bytes, &dsrc);
    if (!rc) rc = rebase_args(c, rb, d_line_off ? &n : nullptr);
    if (rc) return rc;
    return submit_lz4(c, slot, bytes, comp_bytes, dir, n_blocks, dsrc, d_line_off, n, rb);
}

// A mapped batch whose line offsets are already in HBM: nothing waits for a line count, so the
// copy queue holds copies only (a raw batch's split and rebase between copies cost the copy
// queue ~4 % of its time: DESIGN.md section 11) and the scan is enqueued at once behind the
// copy on the compute stream.
int ysb_submit_mapped(ysb_ctx* c, int slot, const uint8_t* bytes, uint64_t nbytes, const uint32_t* d_line_off,
                      uint64_t n, const ysb_rebase* rb) {
    if (!c) return YSB_ERR_ARG;
    int rc = raw_args(c, slot, bytes, nbytes);
    if (rc) return rc;
    if (n > 0x7FFFFFFFull) return fail(c, YSB_ERR_CAPACITY, "at most 2^31-1 events per batch");
    if (n && !d_line_off) return fail(c, YSB_ERR_ARG, "NULL line offsets");
    const u8* dsrc = nullptr;
    if ((rc = mapped_src(c, bytes, nbytes, &dsrc)) || (rc = rebase_args(c, rb, &n))) return rc;
    if (!n) return YSB_OK;
    // at most two copies in flight: the slot's previous one must be done (its device buffer is
    // then only still read by its scan, which the copy waits for on the device)
    if ((rc = slot_begin(c, slot))) return rc;
    Layout lay;
    sampled_layout(c, bytes, nbytes, &lay);
    const SlotCopy v{c->d_bytes[slot], dsrc, bytes, nbytes};
    return slot_launch(c, slot, &v, 1, [&] {
        if (rb)
            if (const int rr = rebase_lines(c, slot, nbytes, d_line_off, n, *rb, c->s_comp)) return rr;
        const ysb_segment sg{c->d_bytes[slot], nbytes, d_line_off, n};
        return enqueue_scan(c, &sg, 1, lay);
    });
}

int ysb_split_lines_device(ysb_ctx* c, const uint8_t* d_bytes, uint64_t nbytes, uint32_t* d_off, uint64_t cap,
                           uint64_t* n) {
    if (!c || !n) return c ? fail(c, YSB_ERR_ARG, "n is NULL") : YSB_ERR_ARG;
    if (nbytes > (4ull << 30) - 64) return fail(c, YSB_ERR_CAPACITY, "batch larger than 4 GiB (u32 offsets)");
    if ((nbytes && !d_bytes) || (cap && !d_off)) return fail(c, YSB_ERR_ARG, "NULL buffers");
    if (reinterpret_cast<uintptr_t>(d_bytes) & 15) return fail(c, YSB_ERR_ARG, "d_bytes must be 16-byte aligned");
    int rc = launch_pending_raw(c);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = grow_device(c, c->d_split_chunk, (split_chunks(nbytes) + 1) * 4, 0))) return rc;
    if ((rc = first_use(c, c->d_cmp, 32))) return rc;
    unsigned long long* d_n = c->d_cmp + 3;
    HIPCHK(c, launch_split_lines(d_bytes, nbytes, c->d_split_chunk, d_off, cap, d_n, c->s_comp));
    unsigned long long got = 0;
    HIPCHK(c, hipMemcpyAsync(&got, d_n, 8, hipMemcpyDeviceToHost, c->s_comp));
    HIPCHK(c, hipStreamSynchronize(c->s_comp));
    *n = got;
    if (got > cap) return fail(c, YSB_ERR_CAPACITY, "%llu lines, cap %llu", (unsigned long long)got, (unsigned long long)cap);
    return YSB_OK;
}

int ysb_copy_time(ysb_ctx* c, double* total_ms, uint64_t* copies, uint64_t* bytes) {
    if (!c) return YSB_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->s_copy));
    double t[2] = {0, 0};
    u64 n = 0;
    HIPCHK(c, c->cev.collect(t, &n));
    if (total_ms) *total_ms = t[1];
    if (copies) *copies = n;
    if (bytes) *bytes = c->copy_bytes;
    c->copy_bytes = 0;
    return YSB_OK;
}

}  // extern "C"
