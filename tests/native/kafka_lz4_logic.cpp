// kafka_lz4_logic.cpp -- the rules of LZ4-compressed Kafka record batches (csrc/ysb_kafka_lz4.h, no
// HIP) on the CPU, built with g++ alone (tests/test_kafka_lz4_logic.py builds it plain and with
// -fsanitize=address,undefined): the index over hand-built compressed batches, every refusal
// with its byte, every buffer cut at every byte (in exact-size heap buffers), the host model
// over the malformed record corpus of kafka_logic.cpp carried inside good frames, bad blocks
// (rule 8) beside bad records in both orders, and the packer's round trip.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "ysb_kafka_lz4.h"

using namespace ysb;
using Bytes = std::vector<u8>;

static int fails = 0;
#define CHECK(...) do { if (!(__VA_ARGS__)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #__VA_ARGS__); ++fails; } } while (0)

static std::unique_ptr<u8[]> exact(const Bytes& b, u64 n) {   // n bytes in a heap block of exactly n
    std::unique_ptr<u8[]> p(new u8[n ? n : 1]);
    if (n) std::memcpy(p.get(), b.data(), n);
    return p;
}
static void put(Bytes& b, const Bytes& x) { b.insert(b.end(), x.begin(), x.end()); }
static Bytes vint(int32_t v) {
    u8 t[8];
    return Bytes(t, t + kafka_put_vint(t, v));
}
static Bytes vlong(i64 v) {
    u8 t[12];
    return Bytes(t, t + kafka_put_vlong(t, v));
}
static Bytes str(const char* s) { return Bytes(s, s + std::strlen(s)); }
static void le32(Bytes& b, u32 v) { for (int k = 0; k < 4; ++k) b.push_back((u8)(v >> (8 * k))); }

// ---- builders -----------------------------------------------------------------------------------

static Bytes record(const Bytes& value, int32_t offset_delta) {
    Bytes body = {0};
    put(body, vlong(0));
    put(body, vint(offset_delta));
    put(body, vint(-1));
    put(body, vint((int32_t)value.size()));
    put(body, value);
    put(body, vint(0));
    Bytes r = vint((int32_t)body.size());
    put(r, body);
    return r;
}
static Bytes records(u32 n, u32 vlen, u32 seed) {
    Bytes all;
    for (u32 i = 0; i < n; ++i) {
        Bytes v(vlen);
        for (u32 j = 0; j < vlen; ++j) v[j] = (u8)('a' + (seed + i + j / 7) % 13);
        put(all, record(v, (int32_t)i));
    }
    return all;
}
static Bytes batch(const Bytes& recs, u32 count, u32 attributes, i64 base_offset) {
    Bytes b(KAFKA_HEADER);
    put(b, recs);
    u8* h = b.data();
    kafka_put_be(h, 8, (u64)base_offset);
    kafka_put_be(h + 8, 4, b.size() - KAFKA_LEN_BASE);
    kafka_put_be(h + 12, 4, 0);
    h[16] = 2;
    kafka_put_be(h + 21, 2, attributes);
    kafka_put_be(h + 23, 4, count ? count - 1 : 0);
    kafka_put_be(h + 27, 8, 0);
    kafka_put_be(h + 35, 8, 0);
    kafka_put_be(h + 43, 8, ~0ull);
    kafka_put_be(h + 51, 2, 0xFFFF);
    kafka_put_be(h + 53, 4, 0xFFFFFFFFu);
    kafka_put_be(h + 57, 4, count);
    kafka_put_be(h + 17, 4, kafka_crc32c(h + KAFKA_CRC_FROM, b.size() - KAFKA_CRC_FROM));
    return b;
}
struct Blk { Bytes data; bool stored; };
// a frame around blocks as they go on the wire; flg: the flag bits beside version 01 (0x20 B.Indep, 0x10 B.Checksum,
// 0x08 C.Size, 0x04 C.Checksum, 0x01 DictID); hc_xor breaks the header checksum
static Bytes frame_of(const std::vector<Blk>& blocks, u32 flg = 0x20, u32 bd = 0x40, u64 content = 0, u8 hc_xor = 0, bool end_mark = true) {
    Bytes f;
    le32(f, LZ4F_MAGIC);
    const size_t d0 = f.size();
    f.push_back((u8)(0x40 | flg));
    f.push_back((u8)bd);
    if (flg & 0x08) for (int k = 0; k < 8; ++k) f.push_back((u8)(content >> (8 * k)));
    if (flg & 0x01) le32(f, 7);
    f.push_back((u8)((xxh32(f.data() + d0, f.size() - d0, 0) >> 8) ^ hc_xor));
    for (const Blk& b : blocks) {
        le32(f, (u32)b.data.size() | (b.stored ? LZ4_STORED : 0));
        put(f, b.data);
        if (flg & 0x10) le32(f, xxh32(b.data.data(), b.data.size(), 0));
    }
    if (end_mark) le32(f, 0);
    if (end_mark && (flg & 0x04)) le32(f, 0x12345678u);   // (never verified)
    return f;
}
static Blk compressed(const Bytes& raw) {
    Bytes c(lz4_compress_bound((u32)raw.size()));
    c.resize(lz4_compress_block(raw.data(), (u32)raw.size(), c.data()));
    return {c, false};
}
// raw as a frame of blocks of block_bytes raw bytes, every `stored_every`-th one stored
static Bytes frame(const Bytes& raw, u32 block_bytes = 65536, u32 flg = 0x20, u32 stored_every = 0) {
    std::vector<Blk> blocks;
    for (u64 a = 0, i = 0; a < raw.size(); a += block_bytes, ++i) {
        const Bytes part(raw.begin() + (ptrdiff_t)a, raw.begin() + (ptrdiff_t)std::min<u64>(raw.size(), a + block_bytes));
        blocks.push_back(stored_every && i % stored_every == stored_every - 1 ? Blk{part, true} : compressed(part));
    }
    return frame_of(blocks, flg, 0x40, raw.size());
}

struct Indexed {
    int rc;
    std::vector<ysb_kafka_batch> b;
    std::vector<ysb_kafka_frame> f;
    std::vector<ysb_lz4_frame_block> k;
    ysb_kafka_lz4_summary s{};
    KafkaError err{};
};
static Indexed index_of(const u8* p, u64 n, u32 flags = YSB_KAFKA_CHECK_CRC) {
    Indexed x;
    x.rc = kafka_index_lz4(p, n, flags, nullptr, nullptr, 0, nullptr, 0, &x.s, &x.err);
    if (x.rc != YSB_OK && x.rc != YSB_ERR_CAPACITY) return x;
    x.b.resize(x.s.n_batches);
    x.f.resize(x.s.n_batches);
    x.k.resize(x.s.blocks);
    ysb_kafka_lz4_summary s2{};
    x.rc = kafka_index_lz4(p, n, flags, x.b.data(), x.f.data(), x.b.size(), x.k.data(), x.k.size(), &s2, &x.err);
    CHECK(std::memcmp(&s2, &x.s, sizeof s2) == 0);
    return x;
}
struct Unframed {
    int rc;
    Bytes out;
    std::vector<u32> off;
    u64 n = 0, bytes = 0, inflated = 0;
    ysb_kafka_counters ct{};
    ysb_kafka_verdict vd{};
};
static Unframed unframe_of(const u8* p, u64 n, const Indexed& x) {
    Unframed u;
    KafkaError err;
    u.rc = kafka_unframe_lz4(p, n, x.b.data(), x.f.data(), x.b.size(), x.k.data(), x.k.size(), nullptr, 0, nullptr, 0, &u.n, &u.bytes,
                             &u.inflated, &u.ct, &u.vd, &err);
    if (u.rc) return u;
    u.out.assign(u.bytes + 1, 0xEE);
    u.off.assign(u.n + 1, 0xEEEEEEEEu);
    u.rc = kafka_unframe_lz4(p, n, x.b.data(), x.f.data(), x.b.size(), x.k.data(), x.k.size(), u.out.data(), u.bytes, u.off.data(),
                             u.off.size(), &u.n, &u.bytes, &u.inflated, &u.ct, &u.vd, &err);
    u.out.resize(u.bytes);
    return u;
}

// ---- the index over hand-built batches ------------------------------------------------------------

static Bytes mixed_buffer() {
    Bytes blob;
    put(blob, batch(frame(records(5, 40, 1)), 5, 3, 0));                            // one block
    put(blob, batch(frame(records(40, 100, 2), 1000), 40, 3, 5));                   // several blocks
    put(blob, batch(frame(records(30, 100, 3), 900, 0x20, 2), 30, 3, 45));          // stored blocks inside a frame
    put(blob, batch(frame(records(9, 60, 4), 300, 0x20 | 0x10 | 0x08 | 0x04), 9, 3, 75));   // every optional flag
    put(blob, batch(frame_of({}), 0, 3, 84));                                        // an empty frame, recordsCount 0
    put(blob, batch(records(7, 30, 5), 7, 0, 84));                                   // uncompressed
    put(blob, batch(records(1, 4, 6), 1, 0x20, 91));                                 // a control batch
    put(blob, batch(frame(records(3, 20, 7)), 3, 3, 92));
    return blob;
}

static void index_and_model() {
    const Bytes blob = mixed_buffer();
    auto p = exact(blob, blob.size());
    Indexed x = index_of(p.get(), blob.size());
    CHECK(x.rc == YSB_OK && x.s.n_batches == 7 && x.s.control_batches == 1 && x.s.compressed_batches == 6);
    CHECK(x.s.n_records == 94 && x.s.consumed == blob.size() && x.s.crc_checked == 8);
    CHECK(x.f[0].n_blocks == 1 && x.f[0].codec == 3 && x.f[1].n_blocks > 3 && x.f[4].n_blocks == 0 && x.f[5].codec == 0 && x.f[5].n_blocks == 1);
    CHECK(x.b[6].control_before == 1 && x.b[5].control_before == 0 && x.b[6].first_record == 91);
    u64 blk = 0, stored = 0;
    for (u64 k = 0; k < x.b.size(); ++k) {
        CHECK(x.f[k].first_block == blk);
        for (u32 j = 0; j < x.f[k].n_blocks; ++j) {
            const ysb_lz4_frame_block& e = x.k[blk + j];
            CHECK(e.offset >= x.b[k].records_off && e.offset + (e.comp_bytes & ~LZ4_STORED) <= x.b[k].records_off + x.b[k].records_bytes);
            stored += (e.comp_bytes & LZ4_STORED) ? 1 : 0;
        }
        blk += x.f[k].n_blocks;
    }
    CHECK(blk == x.s.blocks && stored == x.s.stored_blocks && stored >= 2);
    Unframed u = unframe_of(p.get(), blob.size(), x);
    CHECK(u.rc == YSB_OK && u.n == 94 && u.ct.records == 94 && u.vd.bad_batches == 0 && u.vd.first_bad == KAFKA_NONE);
    // the same records packed uncompressed give the same values, offsets and counters
    Bytes plain;
    put(plain, batch(records(5, 40, 1), 5, 0, 0));
    put(plain, batch(records(40, 100, 2), 40, 0, 5));
    put(plain, batch(records(30, 100, 3), 30, 0, 45));
    put(plain, batch(records(9, 60, 4), 9, 0, 75));
    put(plain, batch(Bytes(), 0, 0, 84));
    put(plain, batch(records(7, 30, 5), 7, 0, 84));
    put(plain, batch(records(3, 20, 7), 3, 0, 92));
    std::vector<ysb_kafka_batch> pi(7);
    ysb_kafka_summary ps{};
    KafkaError err;
    CHECK(kafka_index(plain.data(), plain.size(), 0, pi.data(), 7, &ps, &err) == YSB_OK);
    Bytes pout(u.bytes + 1);
    std::vector<u32> poff(95);
    u64 pn = 0, pb = 0;
    ysb_kafka_counters pct{};
    ysb_kafka_verdict pvd{};
    CHECK(kafka_unframe(plain.data(), plain.size(), pi.data(), 7, pout.data(), pout.size(), poff.data(), poff.size(), &pn, &pb, &pct, &pvd, &err) == YSB_OK);
    pout.resize(pb);
    CHECK(pb == u.bytes && pout == u.out && poff == u.off && std::memcmp(&pct, &u.ct, sizeof pct) == 0);
    CHECK(u.inflated == plain.size() - 7 * KAFKA_HEADER);
    // short caps: the counts are complete
    Indexed y;
    y.b.resize(3);
    y.f.resize(3);
    y.k.resize(2);
    CHECK(kafka_index_lz4(p.get(), blob.size(), 0, y.b.data(), y.f.data(), 3, y.k.data(), 2, &y.s, &y.err) == YSB_ERR_CAPACITY);
    CHECK(y.s.n_batches == 7 && y.s.blocks == x.s.blocks && y.k[1].offset == x.k[1].offset);
    // a wrong CRC over the wire bytes
    Bytes q = blob;
    q[43] ^= 1;   // (producerId: under the CRC, read by nobody)
    CHECK(index_of(q.data(), q.size()).rc == YSB_ERR_FORMAT);
    CHECK(index_of(q.data(), q.size(), 0).rc == YSB_OK);
}

// every buffer cut at every byte: whole batches only, the tail left alone, nothing past the cut read
static void cut_everywhere() {
    const Bytes blob = mixed_buffer();
    std::vector<u64> ends;
    {
        Indexed x = index_of(blob.data(), blob.size());
        for (u64 pos = 0; pos < blob.size();) {
            pos += KAFKA_LEN_BASE + kafka_be(blob.data() + pos + 8, 4);
            ends.push_back(pos);
        }
        CHECK(ends.size() == 8);
    }
    for (u64 n = 0; n <= blob.size(); ++n) {
        auto p = exact(blob, n);
        Indexed x = index_of(p.get(), n);
        u64 whole = 0;
        for (u64 e : ends) if (e <= n) whole = e;
        CHECK(x.rc == YSB_OK && x.s.consumed == whole);
        if (x.rc == YSB_OK && n % 97 == 0) CHECK(unframe_of(p.get(), n, x).rc == YSB_OK);
    }
}

// ---- every refusal, with its byte ------------------------------------------------------------------

static void refusals() {
    const Bytes good = batch(frame(records(4, 30, 1)), 4, 3, 0);
    const Bytes recs = records(4, 30, 2);
    const Blk blk = compressed(recs);
    struct R { const char* name; Bytes records_section; const char* frame_byte; const char* rule; };
    Bytes trailing = frame(recs);
    put(trailing, str("junk!"));
    Bytes cut_in_block = frame(recs);
    cut_in_block.resize(cut_in_block.size() - 9);
    const std::vector<R> cases = {
        {"linked blocks", frame_of({blk}, 0x00), "byte 4:", "LZ4F_blockIndependent"},
        {"a block maximum above 64 KiB", frame_of({blk}, 0x20, 0x50), "byte 5:", "LZ4F_max64KB"},
        {"a dictionary id", frame_of({blk}, 0x21), "byte 4:", "dictionar"},
        {"a bad header checksum", frame_of({blk}, 0x20, 0x40, 0, 0x55), "byte 6:", "header checksum"},
        {"no EndMark inside the records", frame_of({blk}, 0x20, 0x40, 0, 0, false), nullptr, "EndMark"},
        {"the records end inside a block", cut_in_block, nullptr, "ends inside a block"},
        {"bytes behind the last frame", trailing, nullptr, "not an LZ4 frame magic"},
        {"the legacy magic", Bytes{0x02, 0x21, 0x4C, 0x18, 1, 2, 3, 4}, "byte 0:", "legacy"},
        {"a block size word above the maximum", [&] { Bytes f = frame_of({}); f.resize(f.size() - 4); le32(f, 65537); return f; }(), "byte 7:", "block maximum"},
    };
    for (const R& r : cases) {
        Bytes blob = good;
        const u64 at = blob.size();
        put(blob, batch(r.records_section, 4, 3, 4));
        put(blob, good);
        auto p = exact(blob, blob.size());
        Indexed x = index_of(p.get(), blob.size());
        char where[64], recs_at[64];
        std::snprintf(where, sizeof where, "Kafka batch 1 at byte %llu:", (unsigned long long)at);
        std::snprintf(recs_at, sizeof recs_at, "at byte %llu,", (unsigned long long)(at + KAFKA_HEADER));
        CHECK(x.rc == YSB_ERR_FORMAT);
        CHECK(std::strstr(x.err.msg, where) && std::strstr(x.err.msg, recs_at) && std::strstr(x.err.msg, "attributes.codec = 3"));
        CHECK(std::strstr(x.err.msg, r.rule) && (!r.frame_byte || std::strstr(x.err.msg, r.frame_byte)));
        if (!std::strstr(x.err.msg, r.rule)) std::printf("  %s: %s\n", r.name, x.err.msg);
        CHECK(x.s.n_batches == 1);   // the batches in front of it are counted
    }
    const struct { u32 codec; const char* name; } others[] = {{1, "gzip"}, {2, "snappy"}, {4, "zstd"}, {5, "unknown"}, {7, "unknown"}};
    for (const auto& o : others) {
        Bytes blob = good;
        put(blob, batch(recs, 4, o.codec, 4));
        Indexed x = index_of(blob.data(), blob.size());
        char where[64], field[64];
        std::snprintf(where, sizeof where, "Kafka batch 1 at byte %llu:", (unsigned long long)good.size());
        std::snprintf(field, sizeof field, "attributes.codec = %u", o.codec);
        CHECK(x.rc == YSB_ERR_FORMAT && std::strstr(x.err.msg, where) && std::strstr(x.err.msg, field) && std::strstr(x.err.msg, o.name));
    }
    // kafka_index's own rules still hold here
    Bytes bad = good;
    bad[16] = 1;
    CHECK(index_of(bad.data(), bad.size(), 0).rc == YSB_ERR_FORMAT);
    bad = good;
    kafka_put_be(bad.data() + 57, 4, 0xFFFFFFFFu);
    Indexed x = index_of(bad.data(), bad.size(), 0);
    CHECK(x.rc == YSB_ERR_FORMAT && std::strstr(x.err.msg, "recordsCount"));
    // the plain index keeps refusing any codec
    ysb_kafka_summary s{};
    KafkaError err;
    CHECK(kafka_index(good.data(), good.size(), 0, nullptr, 0, &s, &err) == YSB_ERR_FORMAT && std::strstr(err.msg, "codec 0 only"));
}

// ---- the malformed record corpus (kafka_logic.cpp's, byte for byte) inside good frames -------------

struct Mal { const char* name; u32 rule; u32 count; Bytes rec; };

static std::vector<Mal> corpus() {
    Bytes good;
    put(good, {0});
    put(good, vlong(-3));
    put(good, vint(0));
    put(good, vint(1));
    put(good, str("k"));
    put(good, vint(7));
    put(good, str("{\"a\":1}"));
    put(good, vint(1));
    put(good, vint(1));
    put(good, str("h"));
    put(good, vint(-1));
    Bytes g = vint((int32_t)good.size());
    put(g, good);
    auto with = [&](const Bytes& body, int32_t len) {
        Bytes r = g;
        put(r, vint(len));
        put(r, body);
        return r;
    };
    Bytes head = {0};
    put(head, vlong(0));
    put(head, vint(1));
    std::vector<Mal> c;
    Bytes b;
    b = g; put(b, {0x80, 0x80, 0x80, 0x80, 0x80, 0x01}); put(b, good);
    c.push_back({"length varint of six bytes", KAFKA_R_VARINT, 2, b});
    b = g; put(b, {0x80, 0x80});
    c.push_back({"length varint cut by the batch", KAFKA_R_VARINT, 2, b});
    c.push_back({"length 5", KAFKA_R_LENGTH, 2, with(Bytes(good.begin(), good.begin() + 5), 5)});
    c.push_back({"negative length", KAFKA_R_LENGTH, 2, with(good, -3)});
    c.push_back({"record past the batch", KAFKA_R_BATCH, 2, with(good, (int32_t)good.size() + 1)});
    b = {0}; put(b, Bytes(10, 0x80)); put(b, {0x01, 0, 0, 0, 0, 0});
    c.push_back({"timestamp delta of eleven bytes", KAFKA_R_VARINT, 2, with(b, (int32_t)b.size())});
    b = head; put(b, vint(100)); put(b, str("abcdef"));
    c.push_back({"key past the record", KAFKA_R_KEY, 2, with(b, (int32_t)b.size())});
    b = head; put(b, vint(-2)); put(b, str("abcdef"));
    c.push_back({"key length -2", KAFKA_R_KEY, 2, with(b, (int32_t)b.size())});
    b = head; put(b, vint(-1)); put(b, vint(50)); put(b, str("abcdef"));
    c.push_back({"value past the record", KAFKA_R_VALUE, 2, with(b, (int32_t)b.size())});
    b = good; put(b, str("x"));
    c.push_back({"bytes behind the headers", KAFKA_R_HEADERS, 2, with(b, (int32_t)b.size())});
    b = head; put(b, vint(-1)); put(b, vint(2)); put(b, str("ab")); put(b, vint(3)); put(b, vint(1)); put(b, str("h")); put(b, vint(1)); put(b, str("v"));
    c.push_back({"three headers stated, one present", KAFKA_R_VARINT, 2, with(b, (int32_t)b.size())});
    b = head; put(b, vint(-1)); put(b, vint(2)); put(b, str("ab")); put(b, vint(1)); put(b, vint(1)); put(b, str("h")); put(b, vint(9)); put(b, str("v"));
    c.push_back({"header value past the record", KAFKA_R_HEADERS, 2, with(b, (int32_t)b.size())});
    b = head; put(b, vint(-1)); put(b, vint(2)); put(b, str("ab")); put(b, vint(-1));
    c.push_back({"negative headers count", KAFKA_R_HEADERS, 2, with(b, (int32_t)b.size())});
    c.push_back({"a record short", KAFKA_R_COUNT, 3, with(good, (int32_t)good.size())});
    c.push_back({"a record over", KAFKA_R_COUNT, 1, with(good, (int32_t)good.size())});
    return c;
}

static ysb_kafka_verdict plain_verdict(const Bytes& blob) {
    std::vector<ysb_kafka_batch> idx(16);
    ysb_kafka_summary s{};
    KafkaError err;
    CHECK(kafka_index(blob.data(), blob.size(), 0, idx.data(), idx.size(), &s, &err) == YSB_OK);
    u64 n = 0, b = 0;
    ysb_kafka_counters ct{};
    ysb_kafka_verdict vd{};
    kafka_unframe(blob.data(), blob.size(), idx.data(), s.n_batches, nullptr, 0, nullptr, 0, &n, &b, &ct, &vd, &err);
    return vd;
}
static bool same(const ysb_kafka_verdict& a, const ysb_kafka_verdict& b) {
    return a.bad_batches == b.bad_batches && a.first_bad == b.first_bad && a.record == b.record && a.rule == b.rule;
}

static void malformed_records_in_good_frames() {
    const Bytes ok = records(2, 10, 1);
    for (const Mal& m : corpus()) {
        Bytes plain, comp;
        put(plain, batch(ok, 2, 0, 0));
        put(plain, batch(m.rec, m.count, 0, 2));
        put(plain, batch(ok, 2, 0, 9));
        put(comp, batch(frame(ok), 2, 3, 0));
        put(comp, batch(frame(m.rec, 16), m.count, 3, 2));    // blocks of 16 raw bytes: the records straddle them
        put(comp, batch(frame(ok), 2, 3, 9));
        const ysb_kafka_verdict want = plain_verdict(plain);
        CHECK(want.bad_batches == 1 && want.first_bad == 1 && want.rule == m.rule);
        auto p = exact(comp, comp.size());
        Indexed x = index_of(p.get(), comp.size());
        CHECK(x.rc == YSB_OK);
        Unframed u = unframe_of(p.get(), comp.size(), x);
        CHECK(u.rc == YSB_ERR_FORMAT && same(u.vd, want));
        if (!same(u.vd, want)) std::printf("  %s\n", m.name);
    }
}

// ---- bad blocks: rule 8 ---------------------------------------------------------------------------------

static void bad_blocks() {
    const Bytes ok = records(2, 10, 1);
    const Blk good_blk = compressed(records(1, 30, 2));
    const Bytes a4 = {1, 2, 3, 4};
    auto seq = [&](std::initializer_list<u8> tail) { Bytes b = {0x40}; put(b, a4); put(b, Bytes(tail)); return Blk{b, false}; };
    const std::vector<std::pair<const char*, Blk>> bad = {
        {"offset 0", seq({0, 0, 0x00})},
        {"offset before the block's start", seq({5, 0, 0x00})},
        {"input exhausted inside the offset", seq({4})},
        {"the block ends with a match", seq({4, 0})},
        {"input exhausted inside the literals", Blk{{0x80, 1, 2, 3}, false}},
        {"a literal length past 64 KiB", Blk{[] { Bytes b = {0xF0}; b.insert(b.end(), 300, 255); return b; }(), false}},
    };
    for (const auto& c : bad) {
        CHECK(lz4_measure_block(c.second.data.data(), (u32)c.second.data.size()) == 0);
        for (u32 j = 0; j < 3; ++j) {
            std::vector<Blk> blocks(3, good_blk);
            blocks[j] = c.second;
            Bytes blob;
            put(blob, batch(frame(ok), 2, 3, 0));
            put(blob, batch(frame_of(blocks), 3, 3, 2));
            put(blob, batch(ok, 2, 0, 5));
            auto p = exact(blob, blob.size());
            Indexed x = index_of(p.get(), blob.size());
            Unframed u = unframe_of(p.get(), blob.size(), x);
            CHECK(x.rc == YSB_OK && u.rc == YSB_ERR_FORMAT && u.vd.bad_batches == 1 && u.vd.first_bad == 1 && u.vd.record == j &&
                  u.vd.rule == KAFKA_R_CODEC);
            if (u.vd.rule != KAFKA_R_CODEC) std::printf("  %s\n", c.first);
        }
    }
    CHECK(!std::strcmp(kafka_rule_name(KAFKA_R_CODEC), "a block of the batch's LZ4 frame does not decode"));
    // a bad record in batch 2 and a bad block in batch 5, and the reverse: the smallest bad batch,
    // whichever kind of fault it has; bad_batches counts both
    const Mal m = corpus()[8];
    const Bytes bad_rec = batch(frame(m.rec), m.count, 3, 100);
    const Bytes bad_blk = batch(frame_of({good_blk, bad[0].second}), 1, 3, 200);
    for (int order = 0; order < 2; ++order) {
        Bytes blob;
        for (int k = 0; k < 7; ++k) {
            if (k == 2) put(blob, order ? bad_blk : bad_rec);
            else if (k == 5) put(blob, order ? bad_rec : bad_blk);
            else put(blob, batch(frame(ok), 2, 3, k));
        }
        auto p = exact(blob, blob.size());
        Indexed x = index_of(p.get(), blob.size());
        Unframed u = unframe_of(p.get(), blob.size(), x);
        CHECK(u.rc == YSB_ERR_FORMAT && u.vd.bad_batches == 2 && u.vd.first_bad == 2);
        CHECK(order ? (u.vd.rule == KAFKA_R_CODEC && u.vd.record == 1) : (u.vd.rule == m.rule && u.vd.record == 1));
    }
    // recordsCount > 0 over an empty frame: rule 7
    Bytes blob = batch(frame_of({}), 2, 3, 0);
    Indexed x = index_of(blob.data(), blob.size());
    Unframed u = unframe_of(blob.data(), blob.size(), x);
    CHECK(u.rc == YSB_ERR_FORMAT && u.vd.rule == KAFKA_R_COUNT && u.vd.record == 0);
    // entries that break their own rules are argument errors
    blob = batch(frame(ok), 2, 3, 0);
    x = index_of(blob.data(), blob.size());
    Indexed y = x;
    y.f[0].first_block = 1;
    CHECK(unframe_of(blob.data(), blob.size(), y).rc == YSB_ERR_ARG);
    y = x;
    y.k[0].offset = blob.size() - 2;
    CHECK(unframe_of(blob.data(), blob.size(), y).rc == YSB_ERR_ARG);
    y = x;
    y.k[0].comp_bytes = 0;
    CHECK(unframe_of(blob.data(), blob.size(), y).rc == YSB_ERR_ARG);
    y = x;
    y.f[0].codec = 2;
    CHECK(unframe_of(blob.data(), blob.size(), y).rc == YSB_ERR_ARG);
}

// ---- the packer -------------------------------------------------------------------------------------------

static void packer() {
    Bytes data;
    std::vector<u32> off;
    for (u32 i = 0; i < 3000; ++i) {
        off.push_back((u32)data.size());
        char line[96];
        const int n = std::snprintf(line, sizeof line, "{\"user_id\":\"%08x\",\"event_type\":\"%s\",\"t\":%u}", i * 2654435761u,
                                    i % 3 ? "view" : "click", 1000 + i);
        data.insert(data.end(), line, line + n);
    }
    for (u32 limit : {1u, 4096u, 16384u, 200000u, 0u}) {
        ysb_kafka_pack_opts o{};
        o.batch_bytes = limit;
        o.codec = YSB_KAFKA_CODEC_LZ4;
        o.base_offset = 500;
        Bytes dst(kafka_bound(data.size(), off.size(), o));
        u64 nb = 0;
        const u64 n = kafka_pack_lz4(data.data(), data.size(), off.data(), off.size(), o, dst.data(), &nb);
        CHECK(n <= dst.size());
        auto p = exact(dst, n);
        Indexed x = index_of(p.get(), n);
        CHECK(x.rc == YSB_OK && x.s.n_batches == nb && x.s.compressed_batches == nb && x.s.consumed == n && x.s.n_records == off.size());
        if (limit == 200000u) CHECK(x.f[0].n_blocks >= 2);
        if (limit == 1u) CHECK(nb == off.size());
        Unframed u = unframe_of(p.get(), n, x);
        CHECK(u.rc == YSB_OK && u.out == data && std::equal(off.begin(), off.end(), u.off.begin()) && u.off[u.n] == data.size());
        for (u64 k = 0; k < nb; ++k) CHECK(x.b[k].base_offset == 500 + (i64)x.b[k].first_record);
        if (limit >= 4096u) CHECK(n < data.size() * 3 / 4);   // the lines compress
    }
}

int main() {
    index_and_model();
    cut_everywhere();
    refusals();
    malformed_records_in_good_frames();
    bad_blocks();
    packer();
    std::printf(fails ? "%d FAILED\n" : "OK\n", fails);
    return fails ? 1 : 0;
}
