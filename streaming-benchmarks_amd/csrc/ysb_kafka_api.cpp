// ysb_kafka_api.cpp -- Kafka record batches above the kernels (ysb_kafka.hip; the rules:
// ysb_kafka.h): the index, the host model and the packer as C entries, a slot batch's staging
// (the framed bytes in the slot's pinned buffer or left in place in a registered range, the
// index in pinned memory, one copy each), the three launches and the verdict's read-back, the
// synchronous unframing alone and the last call's figures.  ysb_submit_kafka and
// ysb_submit_kafka_mapped sit beside ysb_submit_raw in ysb_raw.cpp.
#include "ysb_ctx.h"
#include "ysb_kafka.h"
#include "ysb_kafka_lz4.h"

using namespace ysb;

static_assert(sizeof(KafkaHead) == 64 && sizeof(KafkaBatchOut) == 32 && sizeof(ysb_kafka_batch) == 40,
              "the device layout below counts on these sizes");

// A call's device buffer: the head and the index entries (what one copy carries), then the
// kernels' scratch.
struct KafkaLayout {
    u64 batches, meta, bout, base, crc, total;
};
// crc: the call verifies the batches' CRCs -- {computed, stored} per batch behind the rest (a
// call that does not pays nothing for them)
static KafkaLayout kafka_layout(u64 nb, u64 nrec, bool crc = false) {
    KafkaLayout l;
    l.batches = sizeof(KafkaHead);
    l.meta = (l.batches + nb * sizeof(ysb_kafka_batch) + 15) & ~15ull;
    l.bout = l.meta + nrec * 16;
    l.base = l.bout + nb * sizeof(KafkaBatchOut);
    l.crc = l.base + nb * 8;
    l.total = l.crc + (crc ? nb * sizeof(uint2) : 0);
    return l;
}
static KafkaParams kafka_params(u8* d, const KafkaLayout& l, const u8* d_bytes, u64 nb, u64 nrec, u8* out, u64 out_cap,
                                u32* line_off) {
    KafkaParams p{};
    p.bytes = d_bytes;
    p.batches = reinterpret_cast<const ysb_kafka_batch*>(d + l.batches);
    p.n_batches = (u32)nb;
    p.n_records = nrec;
    p.meta = reinterpret_cast<uint4*>(d + l.meta);
    p.bout = reinterpret_cast<KafkaBatchOut*>(d + l.bout);
    p.base = reinterpret_cast<u64*>(d + l.base);
    p.head = reinterpret_cast<KafkaHead*>(d);
    p.out = out;
    p.out_cap = out_cap;
    p.line_off = line_off;
    return p;
}

// the index as argument errors (the same for every entry that takes one): *n_records its records
static int crc_args(ysb_ctx* c, const ysb_kafka_batch* batches, u64 nb) {
    const u64 k = kafka_crc_entries_ok(batches, nb);
    if (k != nb)
        return fail(c, YSB_ERR_ARG, "Kafka index entry %llu: records_off %llu, fewer than 44 bytes in front of its records, where "
                    "the stored CRC-32C lies (the CRC check is on: ysb_kafka_set_crc)", (unsigned long long)k,
                    (unsigned long long)batches[k].records_off);
    return YSB_OK;
}

// The CRC kernel's tables and constants on the device, at the first call that verifies.
static int ensure_crc_tables(ysb_ctx* c) {
    if (c->d_kafka_crc_tab) return YSB_OK;
    const CrcTables& T = crc_tables();
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->d_kafka_crc_tab.alloc((CRC_TABLE_WORDS + CRC_CONST_WORDS) * sizeof(u32)));
    hipError_t e = hipMemcpy(c->d_kafka_crc_tab.get(), T.win, sizeof T.win, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(c->d_kafka_crc_tab.get() + CRC_TABLE_WORDS, T.consts, sizeof T.consts, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        c->d_kafka_crc_tab.reset();
        return fail(c, YSB_ERR_HIP, "copying the CRC tables: %s", hipGetErrorString(e));
    }
    return YSB_OK;
}

static int index_args(ysb_ctx* c, const uint8_t* bytes, u64 nbytes, const ysb_kafka_batch* batches, u64 nb, u64* n_records,
                      u64* control) {
    if ((nbytes && !bytes) || (nb && !batches)) return fail(c, YSB_ERR_ARG, "NULL Kafka buffers");
    if (nb > 0x7FFFFFFFull) return fail(c, YSB_ERR_CAPACITY, "at most 2^31-1 Kafka batches per call");
    u64 first = 0, ctl = 0;
    for (u64 k = 0; k < nb; ++k) {
        if (!kafka_entry_ok(batches[k], nbytes, first))
            return fail(c, YSB_ERR_ARG, "Kafka index entry %llu does not lie in the %llu bytes given or breaks the running "
                        "record count (first_record %llu, expected %llu)", (unsigned long long)k, (unsigned long long)nbytes,
                        (unsigned long long)batches[k].first_record, (unsigned long long)first);
        first += batches[k].n_records;
        ctl += batches[k].control_before;
    }
    *n_records = first;
    if (control) *control = ctl;
    return YSB_OK;
}

// walk, base, gather on s (ev: YSB_F_TIMING's four events, created on demand, or NULL; codec: a
// compressed call's plan, whose bad batches become rule 8 behind the walk, or NULL)
// crc: the call verifies -- one launch behind the walk and the codec verdict, in front of the base
// kernel, so a batch whose CRC differs is bad by rule 9 whatever they made of its bytes (cev:
// YSB_F_TIMING's two marks around it, or NULL)
static int launch_unframe(ysb_ctx* c, const KafkaParams& p, hipStream_t s, Event* ev, const KafkaPlanParams* codec = nullptr,
                          const KafkaCrcParams* crc = nullptr, Event* cev = nullptr) {
    if (ev)
        for (int k = 0; k < 4; ++k)
            if (!ev[k]) HIPCHK(c, ev[k].create(hipEventDefault));
    if (ev) HIPCHK(c, hipEventRecord(ev[0], s));
    if (p.n_batches) HIPCHK(c, launch_kafka_walk(p, s));
    if (codec) HIPCHK(c, launch_kafka_codec(*codec, p.bout, s));
    if (ev) HIPCHK(c, hipEventRecord(ev[1], s));
    if (crc && crc->n_batches) {
        HIPCHK(c, mark(cev, 0, s));
        HIPCHK(c, launch_kafka_crc(*crc, (u32)c->cus, s));
        HIPCHK(c, mark(cev, 1, s));
    }
    HIPCHK(c, launch_kafka_base(p, s));
    if (ev) HIPCHK(c, hipEventRecord(ev[2], s));
    HIPCHK(c, launch_kafka_gather(p, s));
    if (ev) HIPCHK(c, hipEventRecord(ev[3], s));
    return YSB_OK;
}

// kafka_last <- a call's figures; the error its verdict asks for
// kafka_crc_last <- what a call's CRC kernel found: crcs[k] = {computed, stored}
static void settle_crc(ysb_ctx* c, const uint2* crcs, const ysb_kafka_batch* batches, u64 nb, Event* cev) {
    ysb_kafka_crc_desc d{};
    d.calls = c->kafka_crc_last.calls + 1;
    d.batches = nb;
    d.first_bad = KAFKA_NONE;
    for (u64 k = 0; k < nb; ++k) {
        d.bytes += (u64)batches[k].records_bytes + KAFKA_CRC_COVERED;
        if (crcs[k].x == crcs[k].y) continue;
        if (!d.bad_batches++) {
            d.first_bad = k;
            d.computed = crcs[k].x;
            d.stored = crcs[k].y;
        }
    }
    if (nb) add_span(cev, 0, 1, &d.crc_ms);
    c->kafka_crc_last = d;
}

// crcs: the call verified (settle_crc), else NULL
static int settle(ysb_ctx* c, const KafkaHead& h, u64 nb, u64 framed, u64 control, const ysb_kafka_batch* batches,
                  Event* ev, const char* what, const uint2* crcs = nullptr, Event* cev = nullptr) {
    if (crcs) settle_crc(c, crcs, batches, nb, cev);
    ysb_kafka_desc d{};
    d.calls = c->kafka_last.calls + 1;
    d.batches = nb;
    d.records = h.n_lines;
    d.null_values = h.nulls;
    d.keyed = h.keyed;
    d.headers = h.headers;
    d.control_skipped = control;
    d.framed_bytes = framed;
    d.value_bytes = h.out_bytes;
    d.window_bytes = KAFKA_WIN;
    d.verdict = ysb_kafka_verdict{h.bad_batches, h.bad_batches ? h.first_bad : KAFKA_NONE, h.bad_rec, h.rule};
    if (ev) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) d.walk_ms = ms;
        if (hipEventElapsedTime(&ms, ev[1], ev[2]) == hipSuccess) d.base_ms = ms;
        if (hipEventElapsedTime(&ms, ev[2], ev[3]) == hipSuccess) d.gather_ms = ms;
        if (crcs) d.base_ms = std::max(0.0, d.base_ms - c->kafka_crc_last.crc_ms);   // (the CRC launch lies between those marks)
    }
    c->kafka_last = d;
    if (h.bad_batches) {
        char msg[512], pre[64];
        std::snprintf(pre, sizeof pre, "%s: ", what);
        const bool named = crcs && h.first_bad < nb;
        kafka_bad_batch_message(msg, sizeof msg, pre, h.first_bad, h.first_bad < nb ? (long long)batches[h.first_bad].base_offset : -1LL,
                                h.rule, h.bad_rec, named ? crcs[h.first_bad].y : 0u, named ? crcs[h.first_bad].x : 0u, h.bad_batches,
                                "; nothing of the call was counted");
        return fail(c, YSB_ERR_FORMAT, "%s", msg);
    }
    if (h.overflow)
        return fail(c, YSB_ERR_CAPACITY, "%s: %llu value bytes do not fit the output", what, (unsigned long long)h.out_bytes);
    return YSB_OK;
}


// ---- LZ4-compressed batches (ysb_kafka_lz4.h) ---------------------------------------------------
static_assert(sizeof(ysb_kafka_frame) == 16 && sizeof(ysb_lz4_frame_block) == sizeof(Lz4FrameBlock) && sizeof(Lz4Desc) == 24 &&
              sizeof(KafkaPlanHead) == 24, "the device layout below counts on these sizes");

// A compressed call's device buffer: the head and the three index arrays (what one copy
// carries), the plan's outputs and the measured sizes, then the Kafka kernels' scratch as
// kafka_layout has it (its own index area stays unused: the walk reads the planned one).
struct KafkaLz4Layout {
    u64 batches, frames, blocks, copied;
    u64 planned, desc, phead, raw, zeros, bbad, cbad, kafka, total;
    KafkaLayout kl;
};
static KafkaLz4Layout kafka_lz4_layout(u64 nb, u64 nblk, u64 nrec, bool crc = false) {
    KafkaLz4Layout l;
    l.batches = sizeof(KafkaHead);
    l.frames = l.batches + nb * sizeof(ysb_kafka_batch);
    l.blocks = l.frames + nb * sizeof(ysb_kafka_frame);
    l.copied = l.blocks + nblk * sizeof(ysb_lz4_frame_block);
    l.planned = (l.copied + 15) & ~15ull;
    l.desc = l.planned + nb * sizeof(ysb_kafka_batch);
    l.phead = l.desc + nblk * sizeof(Lz4Desc);
    l.raw = l.phead + sizeof(KafkaPlanHead);
    l.zeros = l.raw + nblk * 4;
    l.bbad = l.zeros + (nblk + 1) * 4;
    l.cbad = l.bbad + nblk * 4;
    l.kafka = (l.cbad + nb * 4 + 15) & ~15ull;
    l.kl = kafka_layout(nb, nrec, crc);
    l.total = l.kafka + l.kl.total;
    return l;
}
static KafkaPlanParams kafka_plan_params(u8* d, const KafkaLz4Layout& l, u64 nb, u64 nblk, u64 infl_cap) {
    KafkaPlanParams p{};
    p.blocks = reinterpret_cast<const Lz4FrameBlock*>(d + l.blocks);
    p.raw = reinterpret_cast<const u32*>(d + l.raw);
    p.n_blocks = (u32)nblk;
    p.frames = reinterpret_cast<const ysb_kafka_frame*>(d + l.frames);
    p.batches = reinterpret_cast<const ysb_kafka_batch*>(d + l.batches);
    p.n_batches = (u32)nb;
    p.desc = reinterpret_cast<Lz4Desc*>(d + l.desc);
    p.zeros = reinterpret_cast<u32*>(d + l.zeros);
    p.block_bad = reinterpret_cast<u32*>(d + l.bbad);
    p.planned = reinterpret_cast<ysb_kafka_batch*>(d + l.planned);
    p.codec_bad = reinterpret_cast<u32*>(d + l.cbad);
    p.head = reinterpret_cast<KafkaPlanHead*>(d + l.phead);
    p.infl_cap = infl_cap;
    return p;
}

// The inflate chain on s: measure, plan, decode of the wire bytes into d_infl by pp's arrays (ev:
// YSB_F_TIMING's marks, or NULL).  snappy_max_raw set: the call holds blocks tagged SNAPPY_BLOCK --
// their preambles are read in front of the chain (marks 4 and 5) and their decode follows the LZ4
// kernels', each kernel skipping the other codec's blocks; its LDS is sized by that many raw bytes.
static int launch_inflate(ysb_ctx* c, const KafkaPlanParams& pp, const u8* d_wire, u8* d_infl, u32 decoder, hipStream_t s,
                          Event* ev, u32 snappy_max_raw) {
    const u32 tag = snappy_max_raw ? SNAPPY_BLOCK : 0u;
    if (tag) {
        HIPCHK(c, mark(ev, 4, s));
        HIPCHK(c, launch_snappy_preamble(d_wire, pp.blocks, pp.n_blocks, const_cast<u32*>(pp.raw), s));
        HIPCHK(c, mark(ev, 5, s));
    }
    HIPCHK(c, mark(ev, 0, s));
    HIPCHK(c, launch_lz4_measure(d_wire, pp.blocks, pp.n_blocks, const_cast<u32*>(pp.raw), s, tag));
    HIPCHK(c, mark(ev, 1, s));
    HIPCHK(c, launch_kafka_plan(pp, s));
    HIPCHK(c, mark(ev, 2, s));
    if (decoder == YSB_LZ4_DECODER_AUTO) {
        // only the device knows the sizes: each kernel takes its size class (lz4_pick_decoder's
        // threshold), the one-wave kernel with the small window that keeps many waves per CU
        const Lz4Params small{d_wire, pp.desc, pp.n_blocks, LZ4_WIDE_ABOVE, d_infl, pp.head->bad, YSB_LZ4_DECODER_NARROW,
                              pp.block_bad, LZ4_WIDE_ABOVE, 0, tag};
        const Lz4Params large{d_wire, pp.desc, pp.n_blocks, LZ4_MAX_RAW, d_infl, pp.head->bad, YSB_LZ4_DECODER_WIDE,
                              pp.block_bad, 0, LZ4_WIDE_ABOVE, tag};
        HIPCHK(c, launch_lz4_decode(small, s));
        HIPCHK(c, launch_lz4_decode(large, s));
    } else {
        const Lz4Params lp{d_wire, pp.desc, pp.n_blocks, LZ4_MAX_RAW, d_infl, pp.head->bad, decoder, pp.block_bad, 0, 0, tag};
        HIPCHK(c, launch_lz4_decode(lp, s));
    }
    if (tag) {
        const Lz4Params sp{d_wire, pp.desc, pp.n_blocks, snappy_max_raw, d_infl, pp.head->bad, 0, pp.block_bad, 0, 0, tag};
        HIPCHK(c, launch_snappy_decode(sp, s));
    }
    HIPCHK(c, mark(ev, 3, s));
    return YSB_OK;
}

// A call's kernels on s behind the copy of its index into d, the wire bytes in d_wire: walk, base,
// gather into out and line_off.  d_infl set: a compressed call (index, frames and blocks in d as
// kafka_lz4_layout has them) -- the inflate chain in front, the walk over the inflated bytes by
// the planned index, the codec verdict behind it.  *head / *plan: where the two heads lie on the
// device (*plan NULL: not compressed).  zev / kev: YSB_F_TIMING's marks around the inflate chain's
// and the unframing's kernels, or NULL.  crc: the call verifies its batches' CRCs over the wire
// bytes by the host's index (*d_crc: where the values lie on the device; cev: its two marks).
static int launch_call(ysb_ctx* c, u8* d, const u8* d_wire, u8* d_infl, u64 nb, u64 nblk, u64 nrec, u32 decoder, u8* out,
                       u64 out_cap, u32* line_off, hipStream_t s, Event* zev, Event* kev, const KafkaHead** head,
                       const KafkaPlanHead** plan, bool crc = false, const uint2** d_crc = nullptr, Event* cev = nullptr,
                       u64 infl_cap = 0, u32 snappy_max_raw = 0) {
    KafkaParams p;
    KafkaPlanParams pp{};
    KafkaCrcParams cp{};
    if (crc) {
        if (int rc = ensure_crc_tables(c)) return rc;
        cp.bytes = d_wire;
        cp.n_batches = (u32)nb;
        cp.tables = c->d_kafka_crc_tab;
    }
    if (d_infl) {
        if (c->kafka_infl_cap_test && c->kafka_infl_cap_test < infl_cap) infl_cap = c->kafka_infl_cap_test;
        const KafkaLz4Layout l = kafka_lz4_layout(nb, nblk, nrec, crc);
        cp.batches = reinterpret_cast<const ysb_kafka_batch*>(d + l.batches);
        cp.crc = reinterpret_cast<uint2*>(d + l.kafka + l.kl.crc);
        pp = kafka_plan_params(d, l, nb, nblk, infl_cap);
        p = kafka_params(d + l.kafka, l.kl, d_infl, nb, nrec, out, out_cap, line_off);
        p.batches = pp.planned;
        if (int rc = launch_inflate(c, pp, d_wire, d_infl, decoder, s, zev, snappy_max_raw)) return rc;
    } else {
        const KafkaLayout l = kafka_layout(nb, nrec, crc);
        p = kafka_params(d, l, d_wire, nb, nrec, out, out_cap, line_off);
        cp.batches = p.batches;
        cp.crc = reinterpret_cast<uint2*>(d + l.crc);
    }
    cp.bout = p.bout;
    *head = p.head;
    *plan = d_infl ? pp.head : nullptr;
    if (d_crc) *d_crc = cp.crc;
    return launch_unframe(c, p, s, kev, d_infl ? &pp : nullptr, crc ? &cp : nullptr, cev);
}

// kafka_lz4_last <- the inflate half of a call's figures
static void settle_lz4(ysb_ctx* c, const KafkaPlanHead& h, u64 nblk, u64 stored, u64 compressed, u64 wire, u32 decoder,
                       Event* ev, u64 snappy = 0) {
    ysb_kafka_lz4_desc d{};
    d.calls = c->kafka_lz4_last.calls + 1;
    d.blocks = nblk;
    d.stored_blocks = stored;
    d.compressed_batches = compressed;
    d.wire_bytes = wire;
    d.inflated_bytes = h.inflated;
    d.inflated_total = c->kafka_lz4_last.inflated_total + h.inflated;
    d.bad_blocks = (u64)h.zero_blocks + h.decoder_bad;
    d.decoder = nblk == snappy ? 0 : decoder == YSB_LZ4_DECODER_AUTO ? 3 : decoder;
    d.snappy_blocks = snappy;
    if (snappy) add_span(ev, 4, 5, &d.preamble_ms);
    add_span(ev, 0, 1, &d.measure_ms);
    add_span(ev, 1, 2, &d.plan_ms);
    add_span(ev, 2, 3, &d.decode_ms);
    c->kafka_lz4_last = d;
}

extern "C" {

// ---- a Kafka batch through a slot (ysb_raw.cpp submit_kafka) ----------------------------------

// the slot's line capacity as a Kafka batch's (the gather writes one offset more than the records)
static int lines_fit(ysb_ctx* c, u64 nrec) {
    if (nrec + 1 > c->raw_lines_cap)
        return fail(c, YSB_ERR_CAPACITY, "Kafka batch of %llu records, more than the %llu lines its slot holds "
                    "(max(max_batch_events, max_batch_bytes / 32))", (unsigned long long)nrec,
                    (unsigned long long)(c->raw_lines_cap - 1));
    return YSB_OK;
}

// What both stage functions do once the batch's arguments and capacity rules are checked.  The
// slot's buffers: the wire buffer and the pinned heads at their first use, d_kafka[slot] grown
// to dev_total bytes and h_kafka[slot] to `pinned` (outside steady state: more batches, blocks
// or records than any call before).  Then the batch placed: a fresh head and the index at the
// front of the pinned buffer (both layouts'), the wire bytes and the pinned buffer's first
// `copied` bytes as the slot's copies, the RawBatch's fields.
static int place(ysb_ctx* c, int slot, const u8* bytes, u64 nbytes, const u8* dsrc, const ysb_kafka_batch* batches, u64 nb,
                 u64 nrec, u64 control, u64 dev_total, u64 pinned_index, u64 copied, RawBatch* batch, SlotCopy v[2]) {
    HIPCHK(c, hipSetDevice(c->device));
    // with the CRC check on the batches' {computed, stored} come back behind the index
    const u64 pinned = c->kafka_crc_mode ? ((pinned_index + 7) & ~7ull) + nb * sizeof(uint2) : pinned_index;
    if (int rc = ensure_wire(c, slot)) return rc;
    if (!c->h_kafka_head) {
        HIPCHK(c, c->h_kafka_head.alloc(2 * sizeof(KafkaHead)));
        std::memset(c->h_kafka_head.get(), 0, 2 * sizeof(KafkaHead));
    }
    if (dev_total > c->kafka_cap[slot]) {
        const u64 cap = std::max<u64>(dev_total + dev_total / 2, 256u << 10);
        if (int rc = grow_device(c, c->d_kafka[slot], cap + 64, 0)) return rc;
        c->kafka_cap[slot] = cap;
    }
    if (pinned > c->kafka_hcap[slot]) {
        const u64 cap = std::max<u64>(pinned + pinned / 2, 64u << 10);
        c->kafka_hcap[slot] = 0;
        HIPCHK(c, c->h_kafka[slot].alloc(cap + 64));
        HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&c->hd_kafka[slot]), c->h_kafka[slot], 0));
        c->kafka_hcap[slot] = cap;
    }
    KafkaHead head{};
    head.first_bad = KAFKA_NONE;
    std::memcpy(c->h_kafka[slot], &head, sizeof head);
    if (nb) std::memcpy(c->h_kafka[slot] + sizeof head, batches, nb * sizeof(ysb_kafka_batch));
    v[0] = stage_wire(c, slot, bytes, nbytes, dsrc);
    v[1] = {c->d_kafka[slot], c->hd_kafka[slot], c->h_kafka[slot], copied};
    batch->nbytes = nbytes;
    batch->off = c->d_roff[slot];
    batch->n_off = nrec;
    batch->kafka = KafkaStaged{nb, nrec, nbytes, control};
    batch->kafka->crc = c->kafka_crc_mode;
    batch->kafka->crc_back = (pinned_index + 7) & ~7ull;
    return YSB_OK;
}

// The layout sample: the first SAMPLE_LINES values of a run of n records (`limit` bytes at p) as
// the host model's reader finds them, a line each (nothing from a record the reader refuses --
// the device decides that for the batch).
static void sample_values(const u8* p, u64 limit, u32 n, std::vector<u8>* sample) {
    KafkaHostIn in{p};
    u32 pos = 0;
    for (u32 i = 0; i < n && i < SAMPLE_LINES && pos < limit; ++i) {
        u32 body = 0, end = 0;
        KafkaRec r{};
        if (kafka_read_len(in, pos, (u32)limit, &body, &end) || kafka_read_body(in, body, end, &r)) break;
        sample->insert(sample->end(), in.p + r.val_pos, in.p + r.val_pos + r.val_len);
        if (sample->empty() || sample->back() != '\n') sample->push_back('\n');
        pos = end;
    }
}

int kafka_stage(ysb_ctx* c, int slot, const uint8_t* bytes, uint64_t nbytes, const ysb_kafka_batch* batches,
                uint64_t nb, const uint8_t* dsrc, RawBatch* batch, SlotCopy v[2], std::vector<u8>* sample) {
    u64 nrec = 0, control = 0;
    int rc = index_args(c, bytes, nbytes, batches, nb, &nrec, &control);
    if (!rc) rc = lines_fit(c, nrec);
    if (!rc && c->kafka_crc_mode) rc = crc_args(c, batches, nb);
    if (rc) return rc;
    const KafkaLayout l = kafka_layout(nb, nrec, c->kafka_crc_mode != 0);
    if ((rc = place(c, slot, bytes, nbytes, dsrc, batches, nb, nrec, control, l.total, l.meta,
                    l.batches + nb * sizeof(ysb_kafka_batch), batch, v)))
        return rc;
    sample->clear();
    if (nb) sample_values(bytes + batches[0].records_off, batches[0].records_bytes, batches[0].n_records, sample);
    return YSB_OK;
}

// ---- a compressed Kafka batch through a slot (ysb_raw.cpp submit_kafka_lz4) ---------------------

int kafka_lz4_stage(ysb_ctx* c, int slot, const uint8_t* bytes, uint64_t nbytes, const ysb_kafka_batch* batches,
                    const ysb_kafka_frame* frames, uint64_t nb, const ysb_lz4_frame_block* blocks, uint64_t nblk,
                    const uint8_t* dsrc, RawBatch* batch, SlotCopy v[2], std::vector<u8>* sample) {
    if ((nbytes && !bytes) || (nb && (!batches || !frames)) || (nblk && !blocks)) return fail(c, YSB_ERR_ARG, "NULL Kafka buffers");
    if (nb > 0x7FFFFFFFull || nblk > 0x7FFFFFFFull) return fail(c, YSB_ERR_CAPACITY, "at most 2^31-1 Kafka batches and blocks per call");
    u64 nrec = 0, control = 0, compressed = 0, stored = 0, snappy = 0;
    KafkaError err;
    int rc = kafka_lz4_entries(batches, frames, nb, blocks, nblk, nbytes, &nrec, &control, &compressed, &stored, &err,
                               c->kafka_codecs, &snappy);
    if (rc) return fail(c, rc, "%s", err.msg);
    if ((rc = lines_fit(c, nrec))) return rc;
    if (c->kafka_crc_mode && (rc = crc_args(c, batches, nb))) return rc;
    // the host cannot know an LZ4 block's raw size: the guaranteed bound, 64 KiB per block; a
    // snappy block says its own (a preamble the index would refuse counts nothing: the device
    // makes that block bad)
    u64 bound = 0;
    u32 snappy_max = 0;
    if (snappy)
        for (u64 k = 0; k < nb; ++k) bound += kafka_inflate_bound(bytes, frames[k], blocks, &snappy_max);
    const u64 snappy_raw = snappy ? bound - (nblk - snappy) * (u64)LZ4_MAX_RAW : 0;
    if (snappy && bound > c->cfg.max_batch_bytes)
        return fail(c, YSB_ERR_CAPACITY, "compressed Kafka batch: %llu snappy blocks of %llu raw bytes by their preambles and "
                    "%llu other blocks x 65536 B may not fit max_batch_bytes (%llu); submit fewer Kafka batches per call",
                    (unsigned long long)snappy, (unsigned long long)snappy_raw, (unsigned long long)(nblk - snappy),
                    (unsigned long long)c->cfg.max_batch_bytes);
    if (!snappy && nblk * (u64)LZ4_MAX_RAW > c->cfg.max_batch_bytes)
        return fail(c, YSB_ERR_CAPACITY, "compressed Kafka batch of %llu blocks: %llu x 65536 B may not fit max_batch_bytes "
                    "(%llu); submit fewer Kafka batches per call", (unsigned long long)nblk, (unsigned long long)nblk,
                    (unsigned long long)c->cfg.max_batch_bytes);
    const KafkaLz4Layout l = kafka_lz4_layout(nb, nblk, nrec, c->kafka_crc_mode != 0);
    if ((rc = place(c, slot, bytes, nbytes, dsrc, batches, nb, nrec, control, l.total, l.copied, l.copied, batch, v))) return rc;
    // a compressed batch's own: the inflated records and the plan's pinned head at their first
    // use, the frames and the blocks behind the index, what its settling reports
    if (!c->d_kafka_infl[slot]) HIPCHK(c, c->d_kafka_infl[slot].alloc(c->cfg.max_batch_bytes + 64));
    if (!c->h_kafka_plan) {
        HIPCHK(c, c->h_kafka_plan.alloc(2 * sizeof(KafkaPlanHead)));
        std::memset(c->h_kafka_plan.get(), 0, 2 * sizeof(KafkaPlanHead));
    }
    if (nb) std::memcpy(c->h_kafka[slot] + l.frames, frames, nb * sizeof(ysb_kafka_frame));
    if (nblk) std::memcpy(c->h_kafka[slot] + l.blocks, blocks, nblk * sizeof(ysb_lz4_frame_block));
    KafkaStaged& st = *batch->kafka;
    st.lz4 = true;
    st.n_blocks = nblk;
    st.stored_blocks = stored;
    st.compressed_batches = compressed;
    st.decoder = c->lz4_decoder;
    st.snappy_blocks = snappy;
    st.snappy_max_raw = snappy ? std::max(snappy_max, 1u) : 0u;
    // the layout sample: the first batch inflated and read by the host model
    sample->clear();
    if (nb) {
        std::vector<u8> infl((u64)frames[0].n_blocks * LZ4_MAX_RAW + 1);
        u64 total = 0;
        if (kafka_inflate_batch(bytes, frames[0], blocks, infl.data(), &total) == KAFKA_NONE)
            sample_values(infl.data(), total, batches[0].n_records, sample);
    }
    return YSB_OK;
}

int kafka_enqueue(ysb_ctx* c, int slot, const KafkaStaged& b, hipStream_t s) {
    const bool timed = (c->cfg.flags & YSB_F_TIMING) != 0u;
    const KafkaHead* head = nullptr;
    const KafkaPlanHead* plan = nullptr;
    const uint2* d_crc = nullptr;
    if (int rc = launch_call(c, c->d_kafka[slot], c->d_wire[slot], b.lz4 ? c->d_kafka_infl[slot].get() : nullptr, b.n_batches,
                             b.n_blocks, b.n_records, b.decoder, c->d_bytes[slot], c->cfg.max_batch_bytes, c->d_roff[slot], s,
                             timed ? c->ev_kafka_lz4[slot] : nullptr, timed ? c->ev_kafka[slot] : nullptr, &head, &plan,
                             b.crc != 0, &d_crc, timed ? c->ev_kafka_crc[slot] : nullptr, c->cfg.max_batch_bytes, b.snappy_max_raw))
        return rc;
    if (b.crc && b.n_batches)
        HIPCHK(c, hipMemcpyAsync(c->h_kafka[slot] + b.crc_back, d_crc, b.n_batches * sizeof(uint2), hipMemcpyDeviceToHost, s));
    // the verdict comes back through pinned memory with the line count: no host wait here
    HIPCHK(c, hipMemcpyAsync(c->h_kafka_head + slot, head, sizeof(KafkaHead), hipMemcpyDeviceToHost, s));
    if (plan) HIPCHK(c, hipMemcpyAsync(c->h_kafka_plan + slot, plan, sizeof(KafkaPlanHead), hipMemcpyDeviceToHost, s));
    return YSB_OK;
}

int kafka_settle(ysb_ctx* c, int slot, const KafkaStaged& b, u64* nbytes) {
    const bool timed = (c->cfg.flags & YSB_F_TIMING) != 0u;
    if (b.lz4)
        settle_lz4(c, c->h_kafka_plan[slot], b.n_blocks, b.stored_blocks, b.compressed_batches, b.framed_bytes, b.decoder,
                   timed ? c->ev_kafka_lz4[slot] : nullptr, b.snappy_blocks);
    *nbytes = c->h_kafka_head[slot].out_bytes;
    char what[48];
    std::snprintf(what, sizeof what, "Kafka batch (slot %d)", slot);
    return settle(c, c->h_kafka_head[slot], b.n_batches, b.framed_bytes, b.control_skipped,
                  reinterpret_cast<const ysb_kafka_batch*>(c->h_kafka[slot] + sizeof(KafkaHead)),
                  timed ? c->ev_kafka[slot] : nullptr, what,
                  b.crc ? reinterpret_cast<const uint2*>(c->h_kafka[slot] + b.crc_back) : nullptr,
                  timed ? c->ev_kafka_crc[slot] : nullptr);
}

// ---- the unframing alone ----------------------------------------------------------------------

int ysb_kafka_unframe_device(ysb_ctx* c, const uint8_t* d_bytes, uint64_t nbytes, const ysb_kafka_batch* batches,
                             uint64_t nb, uint8_t* d_out, uint64_t out_cap, uint32_t* d_line_off, uint64_t off_cap,
                             uint64_t* n_lines, uint64_t* out_bytes) {
    if (!c) return YSB_ERR_ARG;
    u64 nrec = 0, control = 0;
    int rc = index_args(c, d_bytes, nbytes, batches, nb, &nrec, &control);
    const bool crc = c->kafka_crc_mode != 0;
    if (!rc && crc) rc = crc_args(c, batches, nb);
    if (rc) return rc;
    if (n_lines) *n_lines = nrec;
    if (out_bytes) *out_bytes = 0;
    if (!d_line_off || nrec + 1 > off_cap)
        return fail(c, YSB_ERR_CAPACITY, "%llu records, room for %llu offsets (one more than the records is needed)",
                    (unsigned long long)nrec, (unsigned long long)(d_line_off ? off_cap : 0));
    if (out_cap && !d_out) return fail(c, YSB_ERR_ARG, "NULL output buffer");
    if ((rc = launch_pending_raw(c))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const KafkaLayout l = kafka_layout(nb, nrec, crc);
    if ((rc = grow_device(c, c->d_kafka_sync, l.total + 64, 256u << 10))) return rc;
    if (crc && (rc = ensure_crc_tables(c))) return rc;
    const KafkaParams p = kafka_params(c->d_kafka_sync, l, d_bytes, nb, nrec, d_out, d_out ? out_cap : 0, d_line_off);
    const KafkaCrcParams cp{d_bytes, p.batches, (u32)nb, c->d_kafka_crc_tab, reinterpret_cast<uint2*>(c->d_kafka_sync + l.crc), p.bout};
    std::vector<uint2> crcs(crc ? nb : 0);
    // (the index is the caller's pageable memory, the head this frame's: nothing is left pending)
    const SyncOnExit settled{c->s_comp};
    if (nb) HIPCHK(c, hipMemcpyAsync(c->d_kafka_sync + l.batches, batches, nb * sizeof(ysb_kafka_batch), hipMemcpyHostToDevice, c->s_comp));
    const bool timed = (c->cfg.flags & YSB_F_TIMING) != 0u;
    Event ev[4], cev[2];
    if ((rc = launch_unframe(c, p, c->s_comp, timed ? ev : nullptr, nullptr, crc ? &cp : nullptr, timed ? cev : nullptr))) return rc;
    KafkaHead h{};
    HIPCHK(c, hipMemcpyAsync(&h, p.head, sizeof h, hipMemcpyDeviceToHost, c->s_comp));
    if (crc && nb) HIPCHK(c, hipMemcpyAsync(crcs.data(), cp.crc, nb * sizeof(uint2), hipMemcpyDeviceToHost, c->s_comp));
    HIPCHK(c, hipStreamSynchronize(c->s_comp));
    if (out_bytes) *out_bytes = h.out_bytes;
    return settle(c, h, nb, nbytes, control, batches, timed ? ev : nullptr, "ysb_kafka_unframe_device", crc ? crcs.data() : nullptr,
                  timed ? cev : nullptr);
}

// ---- the inflate and the unframing alone ---------------------------------------------------------

int ysb_kafka_unframe_lz4_device(ysb_ctx* c, const uint8_t* d_bytes, uint64_t nbytes, const ysb_kafka_batch* batches,
                                 const ysb_kafka_frame* frames, uint64_t nb, const ysb_lz4_frame_block* blocks, uint64_t nblk,
                                 uint8_t* d_out, uint64_t out_cap, uint32_t* d_line_off, uint64_t off_cap, uint64_t* n_lines,
                                 uint64_t* out_bytes) {
    if (!c) return YSB_ERR_ARG;
    if ((nbytes && !d_bytes) || (nb && (!batches || !frames)) || (nblk && !blocks)) return fail(c, YSB_ERR_ARG, "NULL Kafka buffers");
    if (nb > 0x7FFFFFFFull || nblk > 0x7FFFFFFFull) return fail(c, YSB_ERR_CAPACITY, "at most 2^31-1 Kafka batches and blocks per call");
    u64 nrec = 0, control = 0, compressed = 0, stored = 0, snappy = 0;
    KafkaError err;
    int rc = kafka_lz4_entries(batches, frames, nb, blocks, nblk, nbytes, &nrec, &control, &compressed, &stored, &err,
                               c->kafka_codecs, &snappy);
    if (rc) return fail(c, rc, "%s", err.msg);
    const bool crc = c->kafka_crc_mode != 0;
    if (crc && (rc = crc_args(c, batches, nb))) return rc;
    if (n_lines) *n_lines = nrec;
    if (out_bytes) *out_bytes = 0;
    if (!d_line_off || nrec + 1 > off_cap)
        return fail(c, YSB_ERR_CAPACITY, "%llu records, room for %llu offsets (one more than the records is needed)",
                    (unsigned long long)nrec, (unsigned long long)(d_line_off ? off_cap : 0));
    if (out_cap && !d_out) return fail(c, YSB_ERR_ARG, "NULL output buffer");
    if ((rc = launch_pending_raw(c))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const KafkaLz4Layout l = kafka_lz4_layout(nb, nblk, nrec, crc);
    std::vector<uint2> crcs(crc ? nb : 0);
    const uint2* d_crc = nullptr;
    if ((rc = grow_device(c, c->d_kafka_lz4_sync, l.total + 64, 256u << 10))) return rc;
    if ((rc = grow_device(c, c->d_kafka_infl_sync, nblk * (u64)LZ4_MAX_RAW + 64, 1u << 20))) return rc;
    u8* d = c->d_kafka_lz4_sync;
    hipStream_t s = c->s_comp;
    const SyncOnExit settled{s};
    if (nb) HIPCHK(c, hipMemcpyAsync(d + l.batches, batches, nb * sizeof(ysb_kafka_batch), hipMemcpyHostToDevice, s));
    if (nb) HIPCHK(c, hipMemcpyAsync(d + l.frames, frames, nb * sizeof(ysb_kafka_frame), hipMemcpyHostToDevice, s));
    if (nblk) HIPCHK(c, hipMemcpyAsync(d + l.blocks, blocks, nblk * sizeof(ysb_lz4_frame_block), hipMemcpyHostToDevice, s));
    const bool timed = (c->cfg.flags & YSB_F_TIMING) != 0u;
    Event ev[6], kev[4], cev[2];
    const KafkaHead* dh = nullptr;
    const KafkaPlanHead* dp = nullptr;
    if ((rc = launch_call(c, d, d_bytes, c->d_kafka_infl_sync, nb, nblk, nrec, c->lz4_decoder, d_out, d_out ? out_cap : 0,
                          d_line_off, s, timed ? ev : nullptr, timed ? kev : nullptr, &dh, &dp, crc, &d_crc, timed ? cev : nullptr,
                          nblk * (u64)LZ4_MAX_RAW, snappy ? SNAPPY_MAX_RAW : 0u)))
        return rc;
    if (crc && nb) HIPCHK(c, hipMemcpyAsync(crcs.data(), d_crc, nb * sizeof(uint2), hipMemcpyDeviceToHost, s));
    KafkaHead h{};
    KafkaPlanHead ph{};
    HIPCHK(c, hipMemcpyAsync(&h, dh, sizeof h, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(&ph, dp, sizeof ph, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (out_bytes) *out_bytes = h.out_bytes;
    settle_lz4(c, ph, nblk, stored, compressed, nbytes, c->lz4_decoder, timed ? ev : nullptr, snappy);
    return settle(c, h, nb, nbytes, control, batches, timed ? kev : nullptr, "ysb_kafka_unframe_lz4_device",
                  crc ? crcs.data() : nullptr, timed ? cev : nullptr);
}

// ---- CRC-32C on the device: the setting, the kernel alone, the last call's figures ---------------

int ysb_kafka_set_crc(ysb_ctx* c, int mode) {
    if (!c) return YSB_ERR_ARG;
    if (mode != YSB_KAFKA_CRC_OFF && mode != YSB_KAFKA_CRC_DEVICE)
        return fail(c, YSB_ERR_ARG, "ysb_kafka_set_crc: mode %d (0: off, 1: on the device)", mode);
    c->kafka_crc_mode = (u32)mode;
    return YSB_OK;
}

int ysb_kafka_set_codecs(ysb_ctx* c, uint32_t mask) {
    if (!c) return YSB_ERR_ARG;
    if (mask != YSB_KAFKA_CODECS_DEFAULT && mask != (YSB_KAFKA_CODECS_DEFAULT | YSB_KAFKA_CODECS_SNAPPY))
        return fail(c, YSB_ERR_ARG, "ysb_kafka_set_codecs: mask %#x (0x9: none and lz4; 0xd: snappy too)", mask);
    c->kafka_codecs = mask;
    return YSB_OK;
}

int ysb_kafka_test_inflated_cap(ysb_ctx* c, uint64_t bytes) {
    if (!c) return YSB_ERR_ARG;
    c->kafka_infl_cap_test = bytes;
    return YSB_OK;
}

int ysb_kafka_crc_device(ysb_ctx* c, const uint8_t* d_bytes, uint64_t nbytes, const ysb_kafka_batch* batches, uint64_t nb,
                         uint32_t* computed, uint32_t* stored) {
    if (!c) return YSB_ERR_ARG;
    if (nb && !computed) return fail(c, YSB_ERR_ARG, "ysb_kafka_crc_device: computed is NULL");
    u64 nrec = 0;
    int rc = index_args(c, d_bytes, nbytes, batches, nb, &nrec, nullptr);
    if (!rc) rc = crc_args(c, batches, nb);
    if (!rc) rc = launch_pending_raw(c);
    if (!rc) rc = ensure_crc_tables(c);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const u64 idx_bytes = (nb * sizeof(ysb_kafka_batch) + 15) & ~15ull;
    if ((rc = grow_device(c, c->d_kafka_crc_sync, idx_bytes + nb * sizeof(uint2) + 64, 64u << 10))) return rc;
    u8* d = c->d_kafka_crc_sync;
    const KafkaCrcParams cp{d_bytes, reinterpret_cast<const ysb_kafka_batch*>(d), (u32)nb, c->d_kafka_crc_tab,
                            reinterpret_cast<uint2*>(d + idx_bytes), nullptr};
    std::vector<uint2> crcs(nb);
    hipStream_t s = c->s_comp;
    const SyncOnExit settled{s};
    const bool timed = (c->cfg.flags & YSB_F_TIMING) != 0u;
    Event cev[2];
    if (nb) {
        HIPCHK(c, hipMemcpyAsync(d, batches, nb * sizeof(ysb_kafka_batch), hipMemcpyHostToDevice, s));
        HIPCHK(c, mark(timed ? cev : nullptr, 0, s));
        HIPCHK(c, launch_kafka_crc(cp, (u32)c->cus, s));
        HIPCHK(c, mark(timed ? cev : nullptr, 1, s));
        HIPCHK(c, hipMemcpyAsync(crcs.data(), cp.crc, nb * sizeof(uint2), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(c, hipStreamSynchronize(s));
    for (u64 k = 0; k < nb; ++k) {
        computed[k] = crcs[k].x;
        if (stored) stored[k] = crcs[k].y;
    }
    settle_crc(c, crcs.data(), batches, nb, timed ? cev : nullptr);
    return YSB_OK;
}

int ysb_kafka_crc_info(ysb_ctx* c, ysb_kafka_crc_desc* info) {
    if (!c || !info) return c ? fail(c, YSB_ERR_ARG, "info is NULL") : YSB_ERR_ARG;
    const int rc = sync_streams(c);   // (a Kafka batch awaiting its launch settles here)
    *info = c->kafka_crc_last;
    info->mode = c->kafka_crc_mode;
    info->grid_waves = kafka_crc_grid_waves((u32)c->cus);
    if (!info->calls) info->first_bad = KAFKA_NONE;
    return rc;
}

int ysb_kafka_verdict_crc_host(const uint8_t* bytes, uint64_t nbytes, const ysb_kafka_batch* batches, uint64_t n_batches,
                               ysb_kafka_verdict* verdict) {
    if ((nbytes && !bytes) || (n_batches && !batches)) return fail(nullptr, YSB_ERR_ARG, "ysb_kafka_verdict_crc_host: NULL buffers");
    KafkaError err;
    const int rc = kafka_unframe(bytes, nbytes, batches, n_batches, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, verdict,
                                 &err, true);
    return rc ? fail(nullptr, rc, "%s", err.msg) : YSB_OK;
}

int ysb_kafka_verdict_crc_lz4_host(const uint8_t* bytes, uint64_t nbytes, const ysb_kafka_batch* batches,
                                   const ysb_kafka_frame* frames, uint64_t n_batches, const ysb_lz4_frame_block* blocks,
                                   uint64_t n_blocks, ysb_kafka_verdict* verdict) {
    if ((nbytes && !bytes) || (n_batches && (!batches || !frames)) || (n_blocks && !blocks))
        return fail(nullptr, YSB_ERR_ARG, "ysb_kafka_verdict_crc_lz4_host: NULL buffers");
    KafkaError err;
    const int rc = kafka_unframe_lz4(bytes, nbytes, batches, frames, n_batches, blocks, n_blocks, nullptr, 0, nullptr, 0, nullptr,
                                     nullptr, nullptr, nullptr, verdict, &err, true, KAFKA_CODECS_ALL);
    return rc ? fail(nullptr, rc, "%s", err.msg) : YSB_OK;
}

uint64_t ysb_kafka_crc_desc_size(void) { return sizeof(ysb_kafka_crc_desc); }

int ysb_kafka_lz4_info(ysb_ctx* c, ysb_kafka_lz4_desc* info) {
    if (!c || !info) return c ? fail(c, YSB_ERR_ARG, "info is NULL") : YSB_ERR_ARG;
    const int rc = sync_streams(c);   // (a Kafka batch awaiting its launch settles here)
    *info = c->kafka_lz4_last;
    info->inflated_buffer_bytes = c->d_kafka_infl[0].bytes() + c->d_kafka_infl[1].bytes() + c->d_kafka_infl_sync.bytes();
    return rc;
}

int ysb_kafka_info(ysb_ctx* c, ysb_kafka_desc* info) {
    if (!c || !info) return c ? fail(c, YSB_ERR_ARG, "info is NULL") : YSB_ERR_ARG;
    const int rc = sync_streams(c);   // (a Kafka batch awaiting its launch settles here)
    *info = c->kafka_last;
    info->window_bytes = KAFKA_WIN;
    return rc;
}

// ---- the host entries: index, model, packer ---------------------------------------------------

int ysb_kafka_index(const uint8_t* bytes, uint64_t nbytes, uint32_t flags, ysb_kafka_batch* batches, uint64_t cap,
                    ysb_kafka_summary* info) {
    if (nbytes && !bytes) return fail(nullptr, YSB_ERR_ARG, "ysb_kafka_index: NULL buffer");
    if (flags & ~(YSB_KAFKA_CHECK_CRC | YSB_KAFKA_CHECK_CRC_CONTROL)) return fail(nullptr, YSB_ERR_ARG, "ysb_kafka_index: unknown flags %#x", flags);
    KafkaError err;
    const int rc = kafka_index(bytes, nbytes, flags, batches, batches ? cap : 0, info, &err);
    return rc ? fail(nullptr, rc, "%s", err.msg) : YSB_OK;
}

uint32_t ysb_kafka_crc32c(const uint8_t* bytes, uint64_t nbytes) { return bytes || !nbytes ? kafka_crc32c(bytes, nbytes) : 0; }

int ysb_kafka_unframe_host(const uint8_t* bytes, uint64_t nbytes, const ysb_kafka_batch* batches, uint64_t n_batches,
                           uint8_t* out, uint64_t out_cap, uint32_t* line_off, uint64_t off_cap, uint64_t* n_lines,
                           uint64_t* out_bytes, ysb_kafka_counters* counters, ysb_kafka_verdict* verdict) {
    if ((nbytes && !bytes) || (n_batches && !batches)) return fail(nullptr, YSB_ERR_ARG, "ysb_kafka_unframe_host: NULL buffers");
    KafkaError err;
    const int rc = kafka_unframe(bytes, nbytes, batches, n_batches, out, out_cap, line_off, off_cap, n_lines, out_bytes,
                                 counters, verdict, &err);
    return rc ? fail(nullptr, rc, "%s", err.msg) : YSB_OK;
}

int ysb_kafka_index_lz4(const uint8_t* bytes, uint64_t nbytes, uint32_t flags, ysb_kafka_batch* batches, ysb_kafka_frame* frames,
                        uint64_t cap, ysb_lz4_frame_block* blocks, uint64_t block_cap, ysb_kafka_lz4_summary* info) {
    if (nbytes && !bytes) return fail(nullptr, YSB_ERR_ARG, "ysb_kafka_index_lz4: NULL buffer");
    if (flags & ~(YSB_KAFKA_CHECK_CRC | YSB_KAFKA_CHECK_CRC_CONTROL | YSB_KAFKA_ACCEPT_SNAPPY))
        return fail(nullptr, YSB_ERR_ARG, "ysb_kafka_index_lz4: unknown flags %#x", flags);
    if (!batches != !frames) return fail(nullptr, YSB_ERR_ARG, "ysb_kafka_index_lz4: batches and frames go together");
    KafkaError err;
    const int rc = kafka_index_lz4(bytes, nbytes, flags, batches, frames, batches ? cap : 0, blocks, blocks ? block_cap : 0, info, &err);
    return rc ? fail(nullptr, rc, "%s", err.msg) : YSB_OK;
}

int ysb_kafka_unframe_lz4_host(const uint8_t* bytes, uint64_t nbytes, const ysb_kafka_batch* batches, const ysb_kafka_frame* frames,
                               uint64_t n_batches, const ysb_lz4_frame_block* blocks, uint64_t n_blocks, uint8_t* out,
                               uint64_t out_cap, uint32_t* line_off, uint64_t off_cap, uint64_t* n_lines, uint64_t* out_bytes,
                               uint64_t* inflated, ysb_kafka_counters* counters, ysb_kafka_verdict* verdict) {
    if ((nbytes && !bytes) || (n_batches && (!batches || !frames)) || (n_blocks && !blocks))
        return fail(nullptr, YSB_ERR_ARG, "ysb_kafka_unframe_lz4_host: NULL buffers");
    KafkaError err;
    const int rc = kafka_unframe_lz4(bytes, nbytes, batches, frames, n_batches, blocks, n_blocks, out, out_cap, line_off, off_cap,
                                     n_lines, out_bytes, inflated, counters, verdict, &err, false, KAFKA_CODECS_ALL);
    return rc ? fail(nullptr, rc, "%s", err.msg) : YSB_OK;
}

static const ysb_kafka_pack_opts KAFKA_DEFAULT_OPTS{};

uint64_t ysb_kafka_bound(uint64_t nbytes, uint64_t n_lines, const ysb_kafka_pack_opts* opts) {
    return kafka_bound(nbytes, n_lines, opts ? *opts : KAFKA_DEFAULT_OPTS);
}

static int pack_args(const uint8_t* src, uint64_t nbytes, const uint32_t* line_off, uint64_t n_lines, const ysb_kafka_pack_opts& o) {
    if ((nbytes && !src) || (n_lines && !line_off)) return fail(nullptr, YSB_ERR_ARG, "ysb_kafka_pack: NULL buffers");
    for (u64 i = 0; i < n_lines; ++i)
        if (line_off[i] > nbytes || (i && line_off[i] < line_off[i - 1]))
            return fail(nullptr, YSB_ERR_ARG, "ysb_kafka_pack: line offset %llu is out of order or past the bytes", (unsigned long long)i);
    if (o.key_off && !o.keys && o.key_off[n_lines]) return fail(nullptr, YSB_ERR_ARG, "ysb_kafka_pack: key offsets without keys");
    if (o.n_headers && (!o.header_keys || !o.header_vals || !o.header_val_len))
        return fail(nullptr, YSB_ERR_ARG, "ysb_kafka_pack: headers without their arrays");
    if (o.codec != 0 && o.codec != YSB_KAFKA_CODEC_LZ4 && o.codec != YSB_KAFKA_CODEC_SNAPPY)
        return fail(nullptr, YSB_ERR_ARG, "ysb_kafka_pack: codec %u: 0 (none), 2 (snappy) and 3 (lz4) are written", o.codec);
    if (o.codec == YSB_KAFKA_CODEC_SNAPPY && (o.snappy_framing > YSB_KAFKA_SNAPPY_RAW || o.snappy_chunk > SNAPPY_MAX_RAW))
        return fail(nullptr, YSB_ERR_ARG, "ysb_kafka_pack: snappy_framing %u (0: xerial, 1: raw), snappy_chunk %u (at most 65536)",
                    o.snappy_framing, o.snappy_chunk);
    return YSB_OK;
}

static int raw_over(uint64_t* dst_bytes) {
    if (dst_bytes) *dst_bytes = 0;
    return fail(nullptr, YSB_ERR_ARG, "ysb_kafka_pack: snappy_framing raw: a batch's records are not 1..65536 bytes, which one raw "
                "block holds (a batch_bytes of at most 65536, or the xerial framing)");
}

int ysb_kafka_pack(const uint8_t* src, uint64_t nbytes, const uint32_t* line_off, uint64_t n_lines,
                   const ysb_kafka_pack_opts* opts, uint8_t* dst, uint64_t dst_cap, uint64_t* dst_bytes, uint64_t* n_batches) {
    const ysb_kafka_pack_opts& o = opts ? *opts : KAFKA_DEFAULT_OPTS;
    if (!dst_bytes) return fail(nullptr, YSB_ERR_ARG, "ysb_kafka_pack: dst_bytes is NULL");
    if (int rc = pack_args(src, nbytes, line_off, n_lines, o)) return rc;
    *dst_bytes = kafka_bound(nbytes, n_lines, o);
    if (*dst_bytes > dst_cap || (!dst && *dst_bytes))
        return fail(nullptr, YSB_ERR_CAPACITY, "ysb_kafka_pack: needs %llu bytes", (unsigned long long)*dst_bytes);
    u64 nb = 0;
    *dst_bytes = o.codec ? kafka_pack_lz4(src, nbytes, line_off, n_lines, o, dst, &nb)
                         : kafka_pack(src, nbytes, line_off, n_lines, o, dst, &nb);
    if (n_batches) *n_batches = nb;
    if (*dst_bytes == KAFKA_PACK_RAW_OVER) return raw_over(dst_bytes);
    return YSB_OK;
}

int ysb_kafka_write_file(const char* path, const uint8_t* src, uint64_t nbytes, const uint32_t* line_off, uint64_t n_lines,
                         const ysb_kafka_pack_opts* opts) {
    if (!path) return fail(nullptr, YSB_ERR_ARG, "ysb_kafka_write_file: NULL path");
    const ysb_kafka_pack_opts& o = opts ? *opts : KAFKA_DEFAULT_OPTS;
    if (int rc = pack_args(src, nbytes, line_off, n_lines, o)) return rc;
    std::vector<u8> blob(kafka_bound(nbytes, n_lines, o) + 1);
    u64 nb = 0;
    const u64 n = o.codec ? kafka_pack_lz4(src, nbytes, line_off, n_lines, o, blob.data(), &nb)
                          : kafka_pack(src, nbytes, line_off, n_lines, o, blob.data(), &nb);
    if (n == KAFKA_PACK_RAW_OVER) return raw_over(nullptr);
    FILE* f = std::fopen(path, "wb");
    if (!f) return fail(nullptr, YSB_ERR_ARG, "cannot write %s", path);
    bool ok = !n || std::fwrite(blob.data(), 1, n, f) == n;
    ok = (std::fclose(f) == 0) && ok;
    return ok ? YSB_OK : fail(nullptr, YSB_ERR_ARG, "short write to %s", path);
}

int ysb_kafka_inflate_bounds(const uint8_t* bytes, uint64_t nbytes, const ysb_kafka_batch* batches, const ysb_kafka_frame* frames,
                             uint64_t n_batches, const ysb_lz4_frame_block* blocks, uint64_t n_blocks, uint64_t* bounds) {
    if ((nbytes && !bytes) || (n_batches && (!batches || !frames || !bounds)) || (n_blocks && !blocks))
        return fail(nullptr, YSB_ERR_ARG, "ysb_kafka_inflate_bounds: NULL buffers");
    KafkaError err;
    if (int rc = kafka_lz4_entries(batches, frames, n_batches, blocks, n_blocks, nbytes, nullptr, nullptr, nullptr, nullptr, &err,
                                   KAFKA_CODECS_ALL))
        return fail(nullptr, rc, "%s", err.msg);
    for (u64 k = 0; k < n_batches; ++k) bounds[k] = kafka_inflate_bound(bytes, frames[k], blocks);
    return YSB_OK;
}

int ysb_snappy_compress_block(const uint8_t* src, uint32_t raw_bytes, uint8_t* dst, uint32_t cap, uint32_t* comp_bytes) {
    if (!src || !dst || !comp_bytes || raw_bytes < 1 || raw_bytes > SNAPPY_MAX_RAW)
        return fail(nullptr, YSB_ERR_ARG, "ysb_snappy_compress_block: NULL buffers or raw_bytes not in 1..65536");
    if (cap < snappy_bound(raw_bytes)) return fail(nullptr, YSB_ERR_CAPACITY, "ysb_snappy_compress_block: needs %u bytes", snappy_bound(raw_bytes));
    *comp_bytes = snappy_compress_block(src, raw_bytes, dst);
    return YSB_OK;
}

int ysb_snappy_decompress_block(const uint8_t* src, uint32_t comp_bytes, uint8_t* dst, uint32_t cap, uint32_t* raw_bytes) {
    if (!src || !dst || !raw_bytes) return fail(nullptr, YSB_ERR_ARG, "ysb_snappy_decompress_block: NULL argument");
    const u32 raw = snappy_raw_of(src, comp_bytes);
    if (raw > cap) return fail(nullptr, YSB_ERR_CAPACITY, "ysb_snappy_decompress_block: the preamble says %u bytes, room for %u", raw, cap);
    *raw_bytes = raw ? snappy_decode_block(src, comp_bytes, dst) : 0;
    if (!*raw_bytes)
        return fail(nullptr, YSB_ERR_FORMAT, "ysb_snappy_decompress_block: a block of %u bytes that breaks the format's rules, or "
                    "whose preamble is not 1..65536", comp_bytes);
    return YSB_OK;
}

uint64_t ysb_kafka_batch_size(void) { return sizeof(ysb_kafka_batch); }
uint64_t ysb_kafka_summary_size(void) { return sizeof(ysb_kafka_summary); }
uint64_t ysb_kafka_verdict_size(void) { return sizeof(ysb_kafka_verdict); }
uint64_t ysb_kafka_counters_size(void) { return sizeof(ysb_kafka_counters); }
uint64_t ysb_kafka_pack_opts_size(void) { return sizeof(ysb_kafka_pack_opts); }
uint64_t ysb_kafka_desc_size(void) { return sizeof(ysb_kafka_desc); }
uint64_t ysb_kafka_frame_size(void) { return sizeof(ysb_kafka_frame); }
uint64_t ysb_kafka_lz4_summary_size(void) { return sizeof(ysb_kafka_lz4_summary); }
uint64_t ysb_kafka_lz4_desc_size(void) { return sizeof(ysb_kafka_lz4_desc); }

}  // extern "C"
