// ysb_kafka.h -- Kafka record batches (message format v2, Kafka >= 0.11): what a consumer's
// fetch response holds and what a partition's .log segment is, byte for byte.  The reference's
// ingest is Kafka (the ad-events topic, KafkaSpout, the fork's FlinkKafkaConsumer); here the
// framed bytes cross PCIe as they are and the GPU finds the event values and gathers them back
// to back in front of the unchanged scan (ysb_kafka.hip; ysb_submit_kafka, include/ysb_hip.h).
//
// No HIP here: the varint reader, the batch header's rules (kafka_index), the record's rules in
// ONE reader -- kafka_read_len + kafka_read_body, which the host model below and the kernel
// both call with their own byte source, so "is this record valid" is written once --, the host
// unframer (the model), CRC-32C and a packer.  tests/native/kafka_logic.cpp runs all of it on
// the CPU.
//
// Format (everything big-endian).  A batch: baseOffset i64, batchLength i32 (the bytes behind
// that field: the batch spans 12 + batchLength), partitionLeaderEpoch i32, magic i8 = 2, crc u32
// (CRC-32C from `attributes` to the batch's end), attributes i16 (bits 0-2 the codec, bit 5 a
// control batch), lastOffsetDelta i32, baseTimestamp i64, maxTimestamp i64, producerId i64,
// producerEpoch i16, baseSequence i32, recordsCount i32: 61 bytes, then the records.  A record:
// length (varint: the bytes behind it), attributes i8, timestampDelta (varlong), offsetDelta
// (varint), keyLength (varint, -1 null), key, valueLength (varint, -1 null), value, headersCount
// (varint), per header keyLength (varint), key, valueLength (varint, -1 null), value.  Varints
// are base-128 little-endian groups, zigzag-coded; at most 5 bytes (varlong: 10); longer ones
// are illegal, non-minimal ones legal.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "../../include/ysb_hip.h"
#include "ysb_common.h"
#include "ysb_kafka_crc.h"

namespace ysb {

constexpr u32 KAFKA_HEADER = 61;         // a batch's header
constexpr u32 KAFKA_LEN_BASE = 12;       // baseOffset and batchLength: what batchLength does not count
constexpr u32 KAFKA_CRC_FROM = 21;       // `attributes`: where the CRC's range begins
constexpr u32 KAFKA_MIN_RECORD = 6;      // attributes, two deltas, two lengths, a count: one byte each
constexpr u32 KAFKA_NONE = 0xFFFFFFFFu;  // first_bad of a call whose batches are all good
// The walk kernel's window: 64 lanes x one 16-byte vector.  A record header or a value may
// lie anywhere across its edges (tests/test_gpu_kafka.py places them there: ysb_kafka_info
// reports the size).
constexpr u32 KAFKA_WIN = 1024;
constexpr u32 KAFKA_GROUP = 64;          // record bodies parsed at once: one per lane

// Why a batch is bad (ysb_kafka_verdict.rule); the smallest bad record of a batch and ITS rule
// are the verdict, so the serial host walk and the kernel's 64-at-a-time walk agree.
enum : u32 {
    KAFKA_OK = 0,
    KAFKA_R_VARINT = 1,    // a varint longer than its limit, or running past the record (`length`: the batch)
    KAFKA_R_LENGTH = 2,    // length < 6
    KAFKA_R_BATCH = 3,     // the record runs past the batch
    KAFKA_R_KEY = 4,       // a key length below -1, or the key runs past the record
    KAFKA_R_VALUE = 5,     // the same for the value
    KAFKA_R_HEADERS = 6,   // a negative count or header key length, a header past the record, or the
                           //   headers not ending exactly at the record's end
    KAFKA_R_COUNT = 7,     // the batch ends in front of record recordsCount, or bytes are left behind it
    KAFKA_R_CODEC = 8,     // a block of the batch's LZ4 frame does not decode (`record`: the smallest such block
                           //   of the batch; ysb_kafka_lz4.h)
    KAFKA_R_CRC = 9        // the batch's CRC-32C differs from the stored one (`record` 0; only where the check
                           //   is asked for: ysb_kafka_set_crc, ysb_kafka_verdict_crc_host).  It comes first: a
                           //   consumer never reads a record of such a batch
};
YSB_HD const char* kafka_rule_name(u32 r) {
    return r == KAFKA_R_VARINT ? "a varint runs past its limit or its extent"
         : r == KAFKA_R_LENGTH ? "length < 6"
         : r == KAFKA_R_BATCH ? "the record runs past the batch"
         : r == KAFKA_R_KEY ? "the key runs past the record"
         : r == KAFKA_R_VALUE ? "the value runs past the record"
         : r == KAFKA_R_HEADERS ? "the headers do not end at the record's end"
         : r == KAFKA_R_COUNT ? "the records do not end at the batch's end"
         : r == KAFKA_R_CODEC ? "a block of the batch's LZ4 frame does not decode"
         : r == KAFKA_R_CRC ? "the batch's CRC-32C differs" : "none";
}

YSB_HD int32_t kafka_unzigzag32(u32 v) { return (int32_t)(v >> 1) ^ -(int32_t)(v & 1); }
YSB_HD i64 kafka_unzigzag64(u64 v) { return (i64)(v >> 1) ^ -(i64)(v & 1); }
YSB_HD u32 kafka_zigzag32(int32_t v) { return ((u32)v << 1) ^ (u32)(v >> 31); }
YSB_HD u64 kafka_zigzag64(i64 v) { return ((u64)v << 1) ^ (u64)(v >> 63); }

// The base-128 groups at pos, at most max_bytes of them; no byte at or past `end` is read.
// false: the groups do not end within max_bytes or within [pos, end).  Bits above 64 are dropped.
template <class In>
YSB_HD bool kafka_read_uvar(In& in, u32& pos, u32 end, u32 max_bytes, u64* v) {
    u64 r = 0;
    for (u32 k = 0; k < max_bytes; ++k) {
        if (pos >= end) return false;
        const u32 b = in.byte(pos++);
        r |= (u64)(b & 127u) << (7 * k);
        if (!(b & 128u)) {
            *v = r;
            return true;
        }
    }
    return false;
}
// A varint (at most 5 bytes; bits above 32 dropped, as Kafka's own int arithmetic drops them).
template <class In>
YSB_HD bool kafka_read_vint(In& in, u32& pos, u32 end, int32_t* v) {
    u64 r;
    if (!kafka_read_uvar(in, pos, end, 5, &r)) return false;
    *v = kafka_unzigzag32((u32)r);
    return true;
}

// One record as the reader found it (positions relative to the batch's first record byte).
struct KafkaRec {
    u32 val_pos, val_len;       // a null value: length 0
    u32 null_value, keyed, headers;
};

// THE reader, first half: the record whose `length` is at pos < n of a batch of n record
// bytes.  *body: its first byte behind `length`, *end: its end.  This is all the serial walk
// decodes; every call that returns KAFKA_OK moves on by at least 7 bytes, so a walk ends.
template <class In>
YSB_HD u32 kafka_read_len(In& in, u32 pos, u32 n, u32* body, u32* end) {
    int32_t len;
    if (!kafka_read_vint(in, pos, n, &len)) return KAFKA_R_VARINT;
    if (len < (int32_t)KAFKA_MIN_RECORD) return KAFKA_R_LENGTH;
    if ((u32)len > n - pos) return KAFKA_R_BATCH;
    *body = pos;
    *end = pos + (u32)len;
    return KAFKA_OK;
}

// ... second half: the body [body, end) that kafka_read_len returned (end - body >= 6).
// In::byte(pos) is called with body <= pos < end only.  The headers' loop ends: a header takes
// two bytes at least.
template <class In>
YSB_HD u32 kafka_read_body(In& in, u32 body, u32 end, KafkaRec* r) {
    u32 pos = body + 1;   // attributes
    u64 t;
    int32_t v;
    if (!kafka_read_uvar(in, pos, end, 10, &t)) return KAFKA_R_VARINT;   // timestampDelta
    if (!kafka_read_vint(in, pos, end, &v)) return KAFKA_R_VARINT;       // offsetDelta
    if (!kafka_read_vint(in, pos, end, &v)) return KAFKA_R_VARINT;       // keyLength
    if (v < -1 || (v > 0 && (u32)v > end - pos)) return KAFKA_R_KEY;
    r->keyed = v >= 0;
    if (v > 0) pos += (u32)v;
    if (!kafka_read_vint(in, pos, end, &v)) return KAFKA_R_VARINT;       // valueLength
    if (v < -1 || (v > 0 && (u32)v > end - pos)) return KAFKA_R_VALUE;
    r->null_value = v < 0;
    r->val_pos = pos;
    r->val_len = v > 0 ? (u32)v : 0;
    pos += r->val_len;
    if (!kafka_read_vint(in, pos, end, &v)) return KAFKA_R_VARINT;       // headersCount
    if (v < 0) return KAFKA_R_HEADERS;
    r->headers = (u32)v;
    for (u32 h = 0; h < r->headers; ++h) {
        if (!kafka_read_vint(in, pos, end, &v)) return KAFKA_R_VARINT;
        if (v < 0 || (u32)v > end - pos) return KAFKA_R_HEADERS;
        pos += (u32)v;
        if (!kafka_read_vint(in, pos, end, &v)) return KAFKA_R_VARINT;
        if (v < -1 || (v > 0 && (u32)v > end - pos)) return KAFKA_R_HEADERS;
        if (v > 0) pos += (u32)v;
    }
    return pos == end ? KAFKA_OK : KAFKA_R_HEADERS;
}

// An index entry's own rules (the caller supplies the index: ysb_kafka_unframe_*, the submits):
// the records lie inside the buffer and first_record is the running sum.
YSB_HD bool kafka_entry_ok(const ysb_kafka_batch& b, u64 nbytes, u64 first_record) {
    return b.records_off <= nbytes && b.records_bytes <= nbytes - b.records_off && b.records_bytes < 0x80000000u &&
           b.n_records < 0x80000000u && b.first_record == first_record;
}

#if !defined(__HIP_DEVICE_COMPILE__)

// ---- CRC-32C: kafka_crc32c, sliced sixteen bytes a round (ysb_kafka_crc.h) --------------------

// ---- big-endian fields ----------------------------------------------------------------------

inline u64 kafka_be(const u8* p, int n) {
    u64 v = 0;
    for (int i = 0; i < n; ++i) v = (v << 8) | p[i];
    return v;
}
inline void kafka_put_be(u8* p, int n, u64 v) {
    for (int i = n - 1; i >= 0; --i, v >>= 8) p[i] = (u8)v;
}

struct KafkaError {
    char msg[512];
};

// Which batches the index verifies on the host: all of them (YSB_KAFKA_CHECK_CRC), or only the
// control batches it skips (YSB_KAFKA_CHECK_CRC_CONTROL) -- what the device, which verifies the
// indexed batches (ysb_kafka_set_crc), never sees.
inline bool kafka_index_checks_crc(u32 flags, u32 attributes) {
    return (flags & YSB_KAFKA_CHECK_CRC) || ((flags & YSB_KAFKA_CHECK_CRC_CONTROL) && (attributes & 0x20u));
}

// An indexed batch's stored CRC and the one its bytes give: the range is [records_off - 40,
// records_off + records_bytes), the stored value the big-endian word in front of it.  The
// entry's records_off is at least KAFKA_CRC_STORED (kafka_crc_entries_ok).
inline bool kafka_crc_differs(const u8* bytes, const ysb_kafka_batch& b, u32* want, u32* got) {
    *want = (u32)kafka_be(bytes + b.records_off - KAFKA_CRC_STORED, 4);
    *got = kafka_crc32c(bytes + b.records_off - KAFKA_CRC_COVERED, (u64)b.records_bytes + KAFKA_CRC_COVERED);
    return *want != *got;
}
// the first entry whose header does not lie in the buffer in front of its records, or n
inline u64 kafka_crc_entries_ok(const ysb_kafka_batch* batches, u64 n) {
    for (u64 k = 0; k < n; ++k)
        if (batches[k].records_off < KAFKA_CRC_STORED) return k;
    return n;
}
// a bad batch as a message (the model's, the device calls'): a CRC names the two values
inline void kafka_bad_batch_message(char* msg, size_t cap, const char* what, u32 k, long long base_offset, u32 rule, u32 rec,
                                    u32 want, u32 got, u32 bad_batches, const char* tail) {
    if (rule == KAFKA_R_CRC)
        std::snprintf(msg, cap, "%sKafka batch %u (baseOffset %lld): %s: stored %08x, computed %08x: the batch's bytes changed "
                      "between the producer and here (%u bad batches in all)%s", what, k, base_offset, kafka_rule_name(rule),
                      want, got, bad_batches, tail);
    else
        std::snprintf(msg, cap, "%sKafka batch %u (baseOffset %lld), %s %u: %s (%u bad batches in all)%s", what, k, base_offset,
                      rule == KAFKA_R_CODEC ? "block" : "record", rec, kafka_rule_name(rule), bad_batches, tail);
}

// ---- the index: the headers alone -------------------------------------------------------------
// One 61-byte read per batch.  A last batch that is not whole (fewer than 61 bytes, or fewer than
// 12 + batchLength) is a fetch response's normal tail: *consumed stops in front of it.  Control
// batches are skipped and counted.  YSB_ERR_FORMAT naming the byte offset, the field, its value
// and the rule; YSB_ERR_CAPACITY (the counts complete) when cap is short.
inline int kafka_index(const u8* bytes, u64 nbytes, u32 flags, ysb_kafka_batch* out, u64 cap, ysb_kafka_summary* info,
                       KafkaError* err) {
    ysb_kafka_summary s{};
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
        const u32 attributes = (u32)kafka_be(h + 21, 2);
        if (attributes & 7u) return refuse("attributes.codec", attributes & 7u, "compressed record batches are not read (codec 0 only)");
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
            if (out && s.n_batches < cap) {
                ysb_kafka_batch& b = out[s.n_batches];
                b.records_off = pos + KAFKA_HEADER;
                b.records_bytes = (u32)(span - KAFKA_HEADER);
                b.n_records = (u32)count;
                b.first_record = s.n_records;
                b.base_offset = (i64)kafka_be(h, 8);
                b.control_before = control_before;
                b.reserved = 0;
            }
            control_before = 0;
            ++s.n_batches;
            s.n_records += (u32)count;
        }
        pos += span;
    }
    s.consumed = pos;
    if (info) *info = s;
    if (s.n_batches > cap) {
        std::snprintf(err->msg, sizeof err->msg, "%llu Kafka batches, cap %llu", (unsigned long long)s.n_batches,
                      (unsigned long long)cap);
        return YSB_ERR_CAPACITY;
    }
    return YSB_OK;
}

// ---- the host unframer: the model -------------------------------------------------------------

struct KafkaHostIn {
    const u8* p;
    u32 byte(u32 pos) const { return p[pos]; }
};

// One batch walked record by record: each value appended at out + *at (NULL out: sizes only),
// line_off[first_record + i] its offset.  Returns the rule that makes the batch bad (*bad_rec
// the record) or KAFKA_OK.
inline u32 kafka_unframe_batch(const u8* bytes, const ysb_kafka_batch& b, u8* out, u64 out_cap, u32* line_off, u64* at,
                               ysb_kafka_counters* ct, u32* bad_rec) {
    KafkaHostIn in{bytes + b.records_off};
    const u32 n = b.records_bytes;
    u32 pos = 0;
    for (u32 i = 0; i < b.n_records; ++i) {
        *bad_rec = i;
        if (pos >= n) return KAFKA_R_COUNT;
        u32 body = 0, end = 0;
        KafkaRec r{};
        u32 rule = kafka_read_len(in, pos, n, &body, &end);
        if (!rule) rule = kafka_read_body(in, body, end, &r);
        if (rule) return rule;
        if (line_off) line_off[b.first_record + i] = (u32)*at;
        if (out && r.val_len && *at + r.val_len <= out_cap) std::memcpy(out + *at, in.p + r.val_pos, r.val_len);
        *at += r.val_len;
        ct->records += 1;
        ct->null_values += r.null_value;
        ct->keyed += r.keyed;
        ct->headers += r.headers;
        pos = end;
    }
    *bad_rec = b.n_records;
    return pos == n ? KAFKA_OK : KAFKA_R_COUNT;
}

// The whole buffer: values back to back, line_off[0 .. n] (the last: the total), the counters.
// The first bad (batch, record, rule) ends the walk (verdict->bad_batches counts every bad
// batch all the same: the kernel's verdict says the same).  out / line_off NULL: sizes only.
inline int kafka_unframe(const u8* bytes, u64 nbytes, const ysb_kafka_batch* batches, u64 n_batches, u8* out, u64 out_cap,
                         u32* line_off, u64 off_cap, u64* n_lines, u64* out_bytes, ysb_kafka_counters* counters,
                         ysb_kafka_verdict* verdict, KafkaError* err, bool check_crc = false) {
    ysb_kafka_counters ct{};
    ysb_kafka_verdict vd{0, KAFKA_NONE, 0, 0};
    u64 first = 0;
    u32 bad_want = 0, bad_got = 0;
    if (check_crc && kafka_crc_entries_ok(batches, n_batches) != n_batches) {
        std::snprintf(err->msg, sizeof err->msg, "index entry %llu: fewer than 44 bytes in front of its records, where the stored "
                      "CRC lies", (unsigned long long)kafka_crc_entries_ok(batches, n_batches));
        return YSB_ERR_ARG;
    }
    for (u64 k = 0; k < n_batches; ++k) {
        if (!kafka_entry_ok(batches[k], nbytes, first)) {
            std::snprintf(err->msg, sizeof err->msg, "index entry %llu does not lie in the buffer or breaks the running record count",
                          (unsigned long long)k);
            return YSB_ERR_ARG;
        }
        first += batches[k].n_records;
    }
    if (n_lines) *n_lines = first;
    if (line_off && first + 1 > off_cap) {
        std::snprintf(err->msg, sizeof err->msg, "%llu records, room for %llu offsets (one more than the records is needed)",
                      (unsigned long long)first, (unsigned long long)off_cap);
        return YSB_ERR_CAPACITY;
    }
    u64 at = 0;
    for (u64 k = 0; k < n_batches; ++k) {
        u32 bad_rec = 0;
        ysb_kafka_counters bc{};
        const u64 at0 = at;
        u32 want = 0, got = 0;
        const u32 rule = check_crc && kafka_crc_differs(bytes, batches[k], &want, &got)
                             ? KAFKA_R_CRC
                             : kafka_unframe_batch(bytes, batches[k], vd.bad_batches ? nullptr : out, out_cap,
                                                   vd.bad_batches ? nullptr : line_off, &at, &bc, &bad_rec);
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

// ---- the packer ---------------------------------------------------------------------------

inline u32 kafka_put_uvar(u8* p, u64 v) {
    u32 n = 0;
    while (v >= 128) {
        p[n++] = (u8)(v | 128);
        v >>= 7;
    }
    p[n++] = (u8)v;
    return n;
}
inline u32 kafka_put_vint(u8* p, int32_t v) { return kafka_put_uvar(p, kafka_zigzag32(v)); }
inline u32 kafka_put_vlong(u8* p, i64 v) { return kafka_put_uvar(p, kafka_zigzag64(v)); }

inline u64 kafka_headers_bytes(const ysb_kafka_pack_opts& o) {
    u64 n = 0;
    for (u32 h = 0; h < o.n_headers; ++h)
        n += 10 + std::strlen(o.header_keys[h]) + (o.header_val_len[h] > 0 ? (u64)o.header_val_len[h] : 0);
    return n;
}

// What kafka_pack may write for n_lines lines of nbytes bytes (each record in a batch of its own).
// With o.codec 3 (kafka_pack_lz4, ysb_kafka_lz4.h) a batch's records are a frame: 19 bytes of
// header and EndMark per batch and a size word per 64 KiB block (a block is never above its raw size).
inline u64 kafka_bound(u64 nbytes, u64 n_lines, const ysb_kafka_pack_opts& o) {
    const u64 keys = o.key_off ? o.key_off[n_lines] : 0;
    const u64 plain = nbytes + keys + n_lines * (KAFKA_HEADER + 40 + kafka_headers_bytes(o));
    if (o.codec == YSB_KAFKA_CODEC_SNAPPY) {   // (ysb_snappy.h snappy_pack_bound, a batch per line at the worst)
        const u64 chunk = o.snappy_chunk ? o.snappy_chunk : 32768u;
        return plain + plain / 6 + (plain / chunk + n_lines + 1) * 36 + n_lines * 48;
    }
    return o.codec ? plain + n_lines * 23 + 4 * (plain / 65536 + 1) : plain;
}

// Lines [line_off[i], line_off[i + 1]) (the last one ends at nbytes) as record batches: a batch
// is closed before the record that would take it past o.batch_bytes (its header included; a
// batch holds one record at least) or past o.batch_records records.  Offsets are consecutive
// from o.base_offset; offsetDelta, lastOffsetDelta, maxTimestamp and the CRC are what a broker
// checks.  dst holds kafka_bound bytes.
inline u64 kafka_pack(const u8* src, u64 nbytes, const u32* line_off, u64 n_lines, const ysb_kafka_pack_opts& o, u8* dst,
                      u64* n_batches) {
    u64 at = 0, nb = 0, i = 0;
    while (i < n_lines) {
        u8* h = dst + at;
        u64 p = KAFKA_HEADER;
        u32 cnt = 0;
        i64 max_ts = 0;
        while (i < n_lines) {
            const u64 v0 = line_off[i], v1 = i + 1 < n_lines ? line_off[i + 1] : nbytes;
            const u32 vlen = (u32)(v1 - v0);
            const int32_t klen = o.key_off ? (int32_t)(o.key_off[i + 1] - o.key_off[i]) : -1;
            const i64 ts = o.ts_delta ? o.ts_delta[i] : 0;
            u8 head[40];
            u32 hn = 0;
            head[hn++] = 0;   // attributes
            hn += kafka_put_vlong(head + hn, ts);
            hn += kafka_put_vint(head + hn, (int32_t)cnt);
            hn += kafka_put_vint(head + hn, klen);
            u8 vl[8], hc[8];
            const u32 vln = kafka_put_vint(vl, (int32_t)vlen), hcn = kafka_put_vint(hc, (int32_t)o.n_headers);
            u64 body = hn + (klen > 0 ? klen : 0) + vln + vlen + hcn;
            for (u32 k = 0; k < o.n_headers; ++k) {
                u8 t[8];
                const u32 kl = (u32)std::strlen(o.header_keys[k]);
                body += kafka_put_vint(t, (int32_t)kl) + kl + kafka_put_vint(t, o.header_val_len[k]) +
                        (o.header_val_len[k] > 0 ? (u32)o.header_val_len[k] : 0);
            }
            u8 ln[8];
            const u32 lnn = kafka_put_vint(ln, (int32_t)body);
            if (cnt && ((o.batch_bytes && p + lnn + body > o.batch_bytes) || (o.batch_records && cnt >= o.batch_records))) break;
            std::memcpy(h + p, ln, lnn);
            p += lnn;
            std::memcpy(h + p, head, hn);
            p += hn;
            if (klen > 0) {
                std::memcpy(h + p, o.keys + o.key_off[i], (u32)klen);
                p += (u32)klen;
            }
            std::memcpy(h + p, vl, vln);
            p += vln;
            if (vlen) std::memcpy(h + p, src + v0, vlen);
            p += vlen;
            std::memcpy(h + p, hc, hcn);
            p += hcn;
            for (u32 k = 0; k < o.n_headers; ++k) {
                const u32 kl = (u32)std::strlen(o.header_keys[k]);
                p += kafka_put_vint(h + p, (int32_t)kl);
                std::memcpy(h + p, o.header_keys[k], kl);
                p += kl;
                p += kafka_put_vint(h + p, o.header_val_len[k]);
                if (o.header_val_len[k] > 0) {
                    std::memcpy(h + p, o.header_vals[k], (u32)o.header_val_len[k]);
                    p += (u32)o.header_val_len[k];
                }
            }
            if (!cnt || ts > max_ts) max_ts = ts;
            ++cnt;
            ++i;
        }
        kafka_put_be(h, 8, (u64)(o.base_offset + (i64)(i - cnt)));
        kafka_put_be(h + 8, 4, p - KAFKA_LEN_BASE);
        kafka_put_be(h + 12, 4, 0);                          // partitionLeaderEpoch
        h[16] = 2;                                           // magic
        kafka_put_be(h + 21, 2, 0);                          // attributes: no codec, create time
        kafka_put_be(h + 23, 4, cnt - 1);                    // lastOffsetDelta
        kafka_put_be(h + 27, 8, (u64)o.base_timestamp);
        kafka_put_be(h + 35, 8, (u64)(o.base_timestamp + max_ts));
        kafka_put_be(h + 43, 8, ~0ull);                      // producerId -1: not idempotent
        kafka_put_be(h + 51, 2, 0xFFFF);                     // producerEpoch -1
        kafka_put_be(h + 53, 4, 0xFFFFFFFFu);                // baseSequence -1
        kafka_put_be(h + 57, 4, cnt);
        kafka_put_be(h + 17, 4, kafka_crc32c(h + KAFKA_CRC_FROM, p - KAFKA_CRC_FROM));
        at += p;
        ++nb;
    }
    *n_batches = nb;
    return at;
}

#endif  // !__HIP_DEVICE_COMPILE__

}  // namespace ysb
