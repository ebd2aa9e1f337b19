// ysb_kafka_lz4.h -- LZ4-compressed Kafka record batches (attributes codec 3; ysb_kafka_index_lz4,
// ysb_submit_kafka_lz4, include/ysb_hip.h): what a consumer of a topic whose producers set
// compression.type=lz4 holds.  In message format v2 the 61-byte batch header stays uncompressed
// and the records section is ONE standard LZ4 frame (the Java client's KafkaLZ4BlockOutputStream:
// FLG 0x60, BD 0x40, an EndMark; librdkafka: LZ4F_blockIndependent, the default 64 KiB blocks) --
// what ysb_lz4_frame.h indexes and ysb_lz4.hip measures and decodes.  The records of a batch are
// found behind the inflate, so the walk's index (records_off, records_bytes) is made on the
// device (kafka_inflate_plan_kernel, ysb_kafka.hip); the host keeps what the header says:
// recordsCount, the running record sum, baseOffset.
//
// No HIP here: the index that accepts codec 0 and 3 (every refusal), the entries' own rules, the
// host model (blocks decoded by ysb_lz4.h's host decoder, then ysb_kafka.h's record walk) and the
// packer for codec 3.  tests/native/kafka_lz4_logic.cpp runs all of it on the CPU.
#pragma once
#include <vector>

#include "ysb_kafka.h"
#include "ysb_lz4_frame.h"
#include "ysb_snappy.h"

namespace ysb {

// a batch's blocks: the bound that keeps its inflated bytes below 2^31 (records_bytes is u32)
constexpr u32 KAFKA_LZ4_MAX_BLOCKS = 32767;
// every codec the compressed path reads (the host models, which have no context's mask)
constexpr u32 KAFKA_CODECS_ALL = YSB_KAFKA_CODECS_DEFAULT | YSB_KAFKA_CODECS_SNAPPY;

#if !defined(__HIP_DEVICE_COMPILE__)

inline const char* kafka_codec_name(u32 codec) {
    return codec == 1 ? "gzip" : codec == 2 ? "snappy" : codec == 3 ? "lz4" : codec == 4 ? "zstd" : codec ? "unknown" : "none";
}

// ---- the index that accepts codec 0 and codec 3 ----------------------------------------------
// kafka_index's walk and rules (magic, batchLength, recordsCount, the partial tail, control
// batches, the CRC over the wire bytes, the counts complete when a cap is short) with three
// arrays: out[] as kafka_index fills it (records_off / records_bytes: the wire bytes, for codec
// 3 the frame), frames[k] the blocks of entry k, blocks[] every block's place in the buffer.  A
// codec-3 batch's records go through lz4f_index and any refusal of it becomes a refusal of the
// Kafka batch; a codec-0 batch's records become stored blocks of at most 64 KiB, so a mixed
// fetch response takes one path on the device.  Codecs 1, 2 and 4 are refused by name -- unless
// flags holds YSB_KAFKA_ACCEPT_SNAPPY: then a codec-2 batch's records go through snappy_index
// (ysb_snappy.h: one block entry per xerial chunk, or one for a raw block, each tagged
// SNAPPY_BLOCK), and any refusal of it becomes a refusal of the Kafka batch.
inline int kafka_index_lz4(const u8* bytes, u64 nbytes, u32 flags, ysb_kafka_batch* out, ysb_kafka_frame* frames, u64 cap,
                           ysb_lz4_frame_block* blocks, u64 block_cap, ysb_kafka_lz4_summary* info, KafkaError* err) {
    ysb_kafka_lz4_summary s{};
    u64 pos = 0;
    u32 control_before = 0;
    auto refuse = [&](const char* field, long long value, const char* rule) {
        std::snprintf(err->msg, sizeof err->msg, "Kafka batch %llu at byte %llu: %s = %lld: %s",
                      (unsigned long long)(s.n_batches + s.control_batches), (unsigned long long)pos, field, value, rule);
        if (info) *info = s;
        return YSB_ERR_FORMAT;
    };
    while (nbytes - pos >= KAFKA_HEADER) {
        const u8* h = bytes + pos;
        const int32_t batch_len = (int32_t)kafka_be(h + 8, 4);
        const int magic = (int8_t)h[16];
        if (magic != 2) return refuse("magic", magic, "only message format v2 (magic 2) is read");
        if (batch_len < (int32_t)(KAFKA_HEADER - KAFKA_LEN_BASE))
            return refuse("batchLength", batch_len, "below 49, the header's own bytes behind the field");
        const u32 attributes = (u32)kafka_be(h + 21, 2), codec = attributes & 7u;
        const bool snappy = codec == YSB_KAFKA_CODEC_SNAPPY && (flags & YSB_KAFKA_ACCEPT_SNAPPY);
        if (codec != 0 && codec != YSB_KAFKA_CODEC_LZ4 && !snappy) {
            char rule[96];
            std::snprintf(rule, sizeof rule, "%s-compressed record batches are not read (codec 0, none, and 3, lz4, only)",
                          kafka_codec_name(codec));
            return refuse("attributes.codec", codec, rule);
        }
        const int32_t count = (int32_t)kafka_be(h + 57, 4);
        if (count < 0) return refuse("recordsCount", count, "negative");
        const u64 span = (u64)KAFKA_LEN_BASE + (u64)batch_len;
        if (nbytes - pos < span) break;   // the tail of a fetch response
        if (kafka_index_checks_crc(flags, attributes)) {
            const u32 want = (u32)kafka_be(h + 17, 4), got = kafka_crc32c(h + KAFKA_CRC_FROM, span - KAFKA_CRC_FROM);
            if (want != got) return refuse("crc", (long long)want, "the batch's CRC-32C differs");
            ++s.crc_checked;
        }
        if (attributes & 0x20u) {
            ++s.control_batches;
            ++control_before;
        } else {
            const u64 roff = pos + KAFKA_HEADER, rbytes = span - KAFKA_HEADER;
            const u64 first_block = s.blocks;
            u64 nblk = 0;
            if (codec == YSB_KAFKA_CODEC_LZ4) {
                const bool room = blocks && first_block < block_cap;
                ysb_lz4_frame_summary fs{};
                Lz4fError fe;
                const int rc = lz4f_index(bytes + roff, rbytes, room ? blocks + first_block : nullptr,
                                          room ? block_cap - first_block : 0, &nblk, &fs, &fe);
                if (rc == YSB_ERR_FORMAT) {
                    char rule[400];
                    std::snprintf(rule, sizeof rule, "its records, %llu bytes at byte %llu, are not a frame that is read: %s",
                                  (unsigned long long)rbytes, (unsigned long long)roff, fe.msg);
                    return refuse("attributes.codec", codec, rule);
                }
                if (nblk > KAFKA_LZ4_MAX_BLOCKS) return refuse("blocks", (long long)nblk, "more than 32767 blocks in one batch");
                if (room)
                    for (u64 j = 0; j < nblk && first_block + j < block_cap; ++j) blocks[first_block + j].offset += roff;
                s.stored_blocks += fs.stored_blocks;
                s.comp_bytes += fs.comp_bytes;
                ++s.compressed_batches;
            } else if (snappy) {
                const bool room = blocks && first_block < block_cap;
                SnappyError se;
                const int rc = snappy_index(bytes + roff, rbytes, room ? blocks + first_block : nullptr,
                                            room ? block_cap - first_block : 0, &nblk, &se);
                if (rc == YSB_ERR_FORMAT) {
                    char rule[400];
                    std::snprintf(rule, sizeof rule, "its records, %llu bytes at byte %llu, are not snappy that is read: %s",
                                  (unsigned long long)rbytes, (unsigned long long)roff, se.msg);
                    return refuse("attributes.codec", codec, rule);
                }
                if (nblk > KAFKA_LZ4_MAX_BLOCKS) return refuse("blocks", (long long)nblk, "more than 32767 blocks in one batch");
                if (room)
                    for (u64 j = 0; j < nblk && first_block + j < block_cap; ++j) blocks[first_block + j].offset += roff;
                s.comp_bytes += snappy_is_xerial(bytes + roff, rbytes) ? rbytes - XERIAL_HEADER - 4 * nblk : rbytes;
                ++s.compressed_batches;
            } else {
                nblk = (rbytes + LZ4F_BLOCK_MAX - 1) / LZ4F_BLOCK_MAX;
                for (u64 j = 0; j < nblk; ++j) {
                    const u32 len = (u32)std::min<u64>(LZ4F_BLOCK_MAX, rbytes - j * LZ4F_BLOCK_MAX);
                    if (blocks && first_block + j < block_cap)
                        blocks[first_block + j] = ysb_lz4_frame_block{roff + j * LZ4F_BLOCK_MAX, len | LZ4_STORED, 0};
                }
                s.stored_blocks += nblk;
                s.comp_bytes += rbytes;
            }
            if (out && frames && s.n_batches < cap) {
                ysb_kafka_batch& b = out[s.n_batches];
                b.records_off = roff;
                b.records_bytes = (u32)rbytes;
                b.n_records = (u32)count;
                b.first_record = s.n_records;
                b.base_offset = (i64)kafka_be(h, 8);
                b.control_before = control_before;
                b.reserved = 0;
                frames[s.n_batches] = ysb_kafka_frame{first_block, (u32)nblk, codec};
            }
            control_before = 0;
            s.blocks += nblk;
            ++s.n_batches;
            s.n_records += (u32)count;
        }
        pos += span;
    }
    s.consumed = pos;
    if (info) *info = s;
    if (s.n_batches > cap || s.blocks > block_cap) {
        std::snprintf(err->msg, sizeof err->msg, "%llu Kafka batches, cap %llu; %llu blocks, cap %llu",
                      (unsigned long long)s.n_batches, (unsigned long long)cap, (unsigned long long)s.blocks,
                      (unsigned long long)block_cap);
        return YSB_ERR_CAPACITY;
    }
    return YSB_OK;
}

// ---- the entries' own rules (the caller supplies all three arrays) ---------------------------
// A batch entry as kafka_entry_ok has it; a frame entry's first_block the running sum, its codec
// 0 or 3, at most KAFKA_LZ4_MAX_BLOCKS blocks; each block of 1..65536 bytes inside its batch's
// wire bytes; the frames' blocks n_blocks in all.  0, or the message in err.
// codecs (ysb_kafka_set_codecs's mask) with YSB_KAFKA_CODECS_SNAPPY: a frame entry of codec 2 is
// taken too, each of its blocks tagged SNAPPY_BLOCK and of 1..SNAPPY_MAX_COMP bytes; a tagged
// block anywhere else is refused.  *snappy (may be NULL): the tagged blocks.
inline int kafka_lz4_entries(const ysb_kafka_batch* batches, const ysb_kafka_frame* frames, u64 nb,
                             const ysb_lz4_frame_block* blocks, u64 n_blocks, u64 nbytes, u64* n_records, u64* control,
                             u64* compressed, u64* stored, KafkaError* err, u32 codecs = YSB_KAFKA_CODECS_DEFAULT,
                             u64* snappy = nullptr) {
    u64 first = 0, blk = 0, ctl = 0, comp = 0, st = 0, sn = 0;
    for (u64 k = 0; k < nb; ++k) {
        const ysb_kafka_batch& b = batches[k];
        const ysb_kafka_frame& f = frames[k];
        if (!kafka_entry_ok(b, nbytes, first)) {
            std::snprintf(err->msg, sizeof err->msg, "Kafka index entry %llu does not lie in the %llu bytes given or breaks the "
                          "running record count (first_record %llu, expected %llu)", (unsigned long long)k,
                          (unsigned long long)nbytes, (unsigned long long)b.first_record, (unsigned long long)first);
            return YSB_ERR_ARG;
        }
        if (f.first_block != blk || f.n_blocks > KAFKA_LZ4_MAX_BLOCKS || f.n_blocks > n_blocks - blk ||
            (f.codec != 0 && f.codec != YSB_KAFKA_CODEC_LZ4 &&
             !(f.codec == YSB_KAFKA_CODEC_SNAPPY && (codecs & YSB_KAFKA_CODECS_SNAPPY)))) {
            std::snprintf(err->msg, sizeof err->msg, "Kafka frame entry %llu: first_block %llu (expected %llu), %u blocks of "
                          "%llu, codec %u", (unsigned long long)k, (unsigned long long)f.first_block, (unsigned long long)blk,
                          f.n_blocks, (unsigned long long)n_blocks, f.codec);
            return YSB_ERR_ARG;
        }
        for (u64 j = 0; j < f.n_blocks; ++j) {
            const ysb_lz4_frame_block& e = blocks[blk + j];
            const bool tagged = f.codec == YSB_KAFKA_CODEC_SNAPPY;
            const u32 len = tagged ? e.comp_bytes & SNAPPY_LEN_MASK : e.comp_bytes & ~LZ4_STORED;
            const bool kind_ok = tagged ? (e.comp_bytes & ~SNAPPY_LEN_MASK) == SNAPPY_BLOCK : !(e.comp_bytes & SNAPPY_BLOCK);
            if (!kind_ok || len < 1 || len > (tagged ? SNAPPY_MAX_COMP : LZ4F_BLOCK_MAX) || e.offset < b.records_off || e.offset - b.records_off > b.records_bytes ||
                len > b.records_bytes - (e.offset - b.records_off)) {
                std::snprintf(err->msg, sizeof err->msg, "block %llu of Kafka batch %llu is not 1..%u bytes inside the "
                              "batch's records%s", (unsigned long long)j, (unsigned long long)k, tagged ? SNAPPY_MAX_COMP : 65536u,
                              tagged ? ", tagged as a snappy block" : "");
                return YSB_ERR_ARG;
            }
            st += (!tagged && (e.comp_bytes & LZ4_STORED)) ? 1 : 0;
            sn += tagged ? 1 : 0;
        }
        comp += f.codec ? 1 : 0;
        blk += f.n_blocks;
        first += b.n_records;
        ctl += b.control_before;
    }
    if (blk != n_blocks) {
        std::snprintf(err->msg, sizeof err->msg, "the frame entries hold %llu blocks, %llu given", (unsigned long long)blk,
                      (unsigned long long)n_blocks);
        return YSB_ERR_ARG;
    }
    if (n_records) *n_records = first;
    if (control) *control = ctl;
    if (compressed) *compressed = comp;
    if (stored) *stored = st;
    if (snappy) *snappy = sn;
    return YSB_OK;
}

// ---- the capacity rule ------------------------------------------------------------------------
// What a batch's blocks may inflate to, as the slot submits count it: a snappy block what its
// preamble says (0 for a preamble the index would refuse: the device makes that block bad), every
// other block LZ4_MAX_RAW, the host having no way to know.  *snappy_max (may be NULL) is raised to
// the largest preamble seen.  The entries have passed kafka_lz4_entries.
inline u64 kafka_inflate_bound(const u8* bytes, const ysb_kafka_frame& f, const ysb_lz4_frame_block* blocks, u32* snappy_max = nullptr) {
    u64 sum = 0;
    for (u32 j = 0; j < f.n_blocks; ++j) {
        const ysb_lz4_frame_block& e = blocks[f.first_block + j];
        u32 raw = LZ4_MAX_RAW;
        if (e.comp_bytes & SNAPPY_BLOCK) {
            raw = snappy_raw_of(bytes + e.offset, e.comp_bytes & SNAPPY_LEN_MASK);
            if (snappy_max && raw > *snappy_max) *snappy_max = raw;
        }
        sum += raw;
    }
    return sum;
}

// ---- the host model ---------------------------------------------------------------------------
// One batch's blocks into scratch (n_blocks x 65536 bytes at least), back to back.  Returns the
// smallest block that the measure walk or the decoder refuses, or KAFKA_NONE; *total the bytes.
inline u32 kafka_inflate_batch(const u8* bytes, const ysb_kafka_frame& f, const ysb_lz4_frame_block* blocks, u8* scratch,
                               u64* total) {
    u64 at = 0;
    for (u32 j = 0; j < f.n_blocks; ++j) {
        const ysb_lz4_frame_block& e = blocks[f.first_block + j];
        u32 raw = 0;
        if (e.comp_bytes & SNAPPY_BLOCK) {
            raw = snappy_decode_block(bytes + e.offset, e.comp_bytes & SNAPPY_LEN_MASK, scratch + at);
            if (!raw) return j;
        } else {
            raw = lz4_measure_block(bytes + e.offset, e.comp_bytes);
            if (!raw || !lz4_decode_block(bytes + e.offset, ysb_lz4_block{e.comp_bytes, raw}, scratch + at)) return j;
        }
        at += raw;
    }
    *total = at;
    return KAFKA_NONE;
}

// kafka_unframe over compressed batches: each batch in order inflated into a scratch area, then
// the same record walk over the result.  A batch with a bad block is KAFKA_R_CODEC, `record` the
// block; the verdict is the smallest bad batch, whichever kind of fault it has; bad_batches
// counts both kinds; nothing of a call with a bad batch is written.
inline int kafka_unframe_lz4(const u8* bytes, u64 nbytes, const ysb_kafka_batch* batches, const ysb_kafka_frame* frames,
                             u64 n_batches, const ysb_lz4_frame_block* blocks, u64 n_blocks, u8* out, u64 out_cap,
                             u32* line_off, u64 off_cap, u64* n_lines, u64* out_bytes, u64* inflated,
                             ysb_kafka_counters* counters, ysb_kafka_verdict* verdict, KafkaError* err,
                             bool check_crc = false, u32 codecs = YSB_KAFKA_CODECS_DEFAULT) {
    ysb_kafka_counters ct{};
    ysb_kafka_verdict vd{0, KAFKA_NONE, 0, 0};
    u64 first = 0;
    u32 bad_want = 0, bad_got = 0;
    if (check_crc && kafka_crc_entries_ok(batches, n_batches) != n_batches) {
        std::snprintf(err->msg, sizeof err->msg, "index entry %llu: fewer than 44 bytes in front of its records, where the stored "
                      "CRC lies", (unsigned long long)kafka_crc_entries_ok(batches, n_batches));
        return YSB_ERR_ARG;
    }
    if (int rc = kafka_lz4_entries(batches, frames, n_batches, blocks, n_blocks, nbytes, &first, nullptr, nullptr, nullptr, err,
                                   codecs))
        return rc;
    if (n_lines) *n_lines = first;
    if (line_off && first + 1 > off_cap) {
        std::snprintf(err->msg, sizeof err->msg, "%llu records, room for %llu offsets (one more than the records is needed)",
                      (unsigned long long)first, (unsigned long long)off_cap);
        return YSB_ERR_CAPACITY;
    }
    std::vector<u8> scratch;
    u64 at = 0, infl = 0;
    for (u64 k = 0; k < n_batches; ++k) {
        u32 bad_rec = 0;
        ysb_kafka_counters bc{};
        const u64 at0 = at;
        u64 total = 0;
        if (scratch.size() < (u64)frames[k].n_blocks * LZ4_MAX_RAW) scratch.resize((u64)frames[k].n_blocks * LZ4_MAX_RAW);
        u32 rule = KAFKA_OK, want = 0, got = 0;
        // the CRC is over the wire bytes and comes first: a batch that fails it is not inflated
        const bool crc_bad = check_crc && kafka_crc_differs(bytes, batches[k], &want, &got);
        const u32 bad_block = crc_bad ? KAFKA_NONE : kafka_inflate_batch(bytes, frames[k], blocks, scratch.data(), &total);
        if (crc_bad) {
            rule = KAFKA_R_CRC;
        } else if (bad_block != KAFKA_NONE) {
            rule = KAFKA_R_CODEC;
            bad_rec = bad_block;
        } else {
            ysb_kafka_batch b = batches[k];
            b.records_off = 0;
            b.records_bytes = (u32)total;
            infl += total;
            rule = kafka_unframe_batch(scratch.data(), b, vd.bad_batches ? nullptr : out, out_cap,
                                       vd.bad_batches ? nullptr : line_off, &at, &bc, &bad_rec);
        }
        if (rule) {
            if (!vd.bad_batches) {
                bad_want = want;
                bad_got = got;
                vd.first_bad = (u32)k;
                vd.record = bad_rec;
                vd.rule = rule;
            }
            ++vd.bad_batches;
            at = at0;
            continue;
        }
        ct.records += bc.records;
        ct.null_values += bc.null_values;
        ct.keyed += bc.keyed;
        ct.headers += bc.headers;
    }
    ct.value_bytes = at;
    if (counters) *counters = ct;
    if (verdict) *verdict = vd;
    if (out_bytes) *out_bytes = at;
    if (inflated) *inflated = infl;
    if (vd.bad_batches) {
        kafka_bad_batch_message(err->msg, sizeof err->msg, "", vd.first_bad, (long long)batches[vd.first_bad].base_offset, vd.rule,
                                vd.record, bad_want, bad_got, vd.bad_batches, "");
        return YSB_ERR_FORMAT;
    }
    if (at > 0xFFFFFFFFull || (out && at > out_cap)) {
        std::snprintf(err->msg, sizeof err->msg, "%llu value bytes, cap %llu", (unsigned long long)at,
                      (unsigned long long)std::min<u64>(out_cap, 0xFFFFFFFFull));
        return YSB_ERR_CAPACITY;
    }
    if (line_off) line_off[first] = (u32)at;
    return YSB_OK;
}

// ---- the packer for codec 3 -------------------------------------------------------------------
// kafka_pack's batches (closed by their uncompressed size, as a producer's batch.size closes
// them), each one's records rewritten as one standard frame: 64 KiB blocks from the library's
// greedy compressor, a block that does not shrink stored; attributes = 3, batchLength and the
// CRC over what is on the wire.  dst holds kafka_bound bytes (o.codec == 3).
// o.codec == 2: the records as snappy instead (ysb_snappy.h snappy_pack: a xerial stream of chunks
// of o.snappy_chunk raw bytes, or with o.snappy_framing RAW one raw block -- KAFKA_PACK_RAW_OVER
// is returned where a batch's records are not 1..65536 bytes, which one block cannot hold).
constexpr u64 KAFKA_PACK_RAW_OVER = ~0ull;
inline u64 kafka_pack_lz4(const u8* src, u64 nbytes, const u32* line_off, u64 n_lines, const ysb_kafka_pack_opts& o, u8* dst,
                          u64* n_batches) {
    ysb_kafka_pack_opts plain = o;
    plain.codec = 0;
    std::vector<u8> tmp(kafka_bound(nbytes, n_lines, plain) + 1);
    u64 nb = 0;
    const u64 n = kafka_pack(src, nbytes, line_off, n_lines, plain, tmp.data(), &nb);
    u64 at = 0, pos = 0;
    while (pos < n) {
        const u8* h = tmp.data() + pos;
        const u64 span = KAFKA_LEN_BASE + kafka_be(h + 8, 4);
        u8* d = dst + at;
        std::memcpy(d, h, KAFKA_HEADER);
        const u64 rb = span - KAFKA_HEADER;
        const bool snappy = o.codec == YSB_KAFKA_CODEC_SNAPPY, xerial = o.snappy_framing != YSB_KAFKA_SNAPPY_RAW;
        if (snappy && !xerial && (rb < 1 || rb > SNAPPY_MAX_RAW)) return KAFKA_PACK_RAW_OVER;
        const u64 fb = snappy ? snappy_pack(h + KAFKA_HEADER, rb, o.snappy_chunk, xerial, d + KAFKA_HEADER)
                              : lz4f_pack(h + KAFKA_HEADER, rb, LZ4F_BLOCK_MAX, 1, d + KAFKA_HEADER);
        const u64 p = KAFKA_HEADER + fb;
        kafka_put_be(d + 8, 4, p - KAFKA_LEN_BASE);
        kafka_put_be(d + 21, 2, o.codec);
        kafka_put_be(d + 17, 4, kafka_crc32c(d + KAFKA_CRC_FROM, p - KAFKA_CRC_FROM));
        at += p;
        pos += span;
    }
    *n_batches = nb;
    return at;
}

#endif  // !__HIP_DEVICE_COMPILE__

}  // namespace ysb
