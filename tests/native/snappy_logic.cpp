// snappy_logic.cpp -- the rules of snappy blocks and snappy-compressed Kafka record batches
// (csrc/ysb_snappy.h and the codec-2 parts of csrc/ysb_kafka_lz4.h, no HIP) on the CPU, built with
// g++ alone (tests/test_snappy_logic.py builds it plain and with -fsanitize=address,undefined):
// the preamble and element readers over hand-built blocks, the host decoder over every malformed
// block and over every block cut at every byte (in exact-size heap buffers), the compressor's
// round trip and its bound (all three copy forms and overlapping copies come out), the xerial
// index with every refusal and its byte, the opt-in at the Kafka index and at the entries'
// rules, the host model and the packer's round trip in both framings.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
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
static Bytes cat(std::initializer_list<Bytes> parts) {
    Bytes b;
    for (const Bytes& p : parts) put(b, p);
    return b;
}
static Bytes str(const char* s) { return Bytes(s, s + std::strlen(s)); }

// ---- element builders ------------------------------------------------------------------------------
static Bytes pre(u32 n, u32 pad = 0) {
    u8 t[8];
    u32 o = snappy_put_preamble(t, n);
    for (u32 i = 0; i < pad; ++i) {
        t[o - 1] |= 128;
        t[o++] = 0;
    }
    return Bytes(t, t + o);
}
static Bytes lit(const Bytes& d, int length_bytes = -1) {
    const u32 m = (u32)d.size() - 1;
    if (length_bytes < 0) length_bytes = m < 60 ? 0 : m < 256 ? 1 : m < 65536 ? 2 : 3;
    Bytes b;
    if (!length_bytes) {
        b.push_back((u8)(m << 2));
    } else {
        b.push_back((u8)((59 + length_bytes) << 2));
        for (int i = 0; i < length_bytes; ++i) b.push_back((u8)(m >> (8 * i)));
    }
    put(b, d);
    return b;
}
static Bytes copy1(u32 len, u32 off) { return {(u8)(1 | (len - 4) << 2 | (off >> 8) << 5), (u8)off}; }
static Bytes copy2(u32 len, u32 off) { return {(u8)(2 | (len - 1) << 2), (u8)off, (u8)(off >> 8)}; }
static Bytes copy4(u32 len, u32 off) {
    return {(u8)(3 | (len - 1) << 2), (u8)off, (u8)(off >> 8), (u8)(off >> 16), (u8)(off >> 24)};
}
static Bytes pattern(u32 n, u32 seed) {
    Bytes b(n);
    for (u32 i = 0; i < n; ++i) b[i] = (u8)('a' + (seed + i * 7 + i / 13) % 23);
    return b;
}

// the decoder over an exact-size copy: the raw bytes, or empty for a refused block
static Bytes decode(const Bytes& block) {
    const auto p = exact(block, block.size());
    Bytes out(SNAPPY_MAX_RAW);
    const u32 raw = snappy_decode_block(p.get(), (u32)block.size(), out.data());
    out.resize(raw);
    return out;
}

static void test_reader_and_decoder() {
    // preambles: minimal, non-minimal (85 00), the largest, and the refused ones
    u32 raw = 0, next = 0;
    const Bytes p51 = pre(5, 1);
    SnappyHostIn in51{p51.data()};
    CHECK(p51 == Bytes({0x85, 0x00}) && snappy_read_preamble(in51, 2, &raw, &next) && raw == 5 && next == 2);
    const Bytes big = {0xFF, 0xFF, 0xFF, 0xFF, 0x0F};
    SnappyHostIn inbig{big.data()};
    CHECK(snappy_read_preamble(inbig, 5, &raw, &next) && raw == 0xFFFFFFFFu && next == 5);
    CHECK(snappy_block_raw(inbig, 5, nullptr) == 0);   // above 65536: not read
    const Bytes six = {0x88, 0x80, 0x80, 0x80, 0x80, 0x00}, over = {0x80, 0x80, 0x80, 0x80, 0x10};
    SnappyHostIn in6{six.data()}, ino{over.data()};
    CHECK(!snappy_read_preamble(in6, 6, &raw, &next) && !snappy_read_preamble(ino, 5, &raw, &next));
    CHECK(!snappy_read_preamble(in6, 3, &raw, &next));   // cut
    CHECK(snappy_raw_of(pre(65536).data(), 3) == 65536 && snappy_raw_of(pre(65537).data(), 3) == 0 && snappy_raw_of(pre(0).data(), 1) == 0);

    // every literal form and every copy form decodes to what the rules say
    const Bytes d8 = str("abcdefgh");
    CHECK(decode(cat({pre(8), lit(d8)})) == d8);
    CHECK(decode(cat({pre(8, 2), lit(d8, 4)})) == d8);                       // non-minimal preamble and length
    for (u32 n : {1u, 60u, 61u, 257u, 65536u}) CHECK(decode(cat({pre(n), lit(pattern(n, n))})) == pattern(n, n));
    CHECK(decode(cat({pre(12), lit(d8), copy1(4, 8)})) == str("abcdefghabcd"));
    CHECK(decode(cat({pre(12), lit(d8), copy2(4, 3)})) == str("abcdefghfghf"));   // overlapping: replicates
    CHECK(decode(cat({pre(12), lit(d8), copy4(4, 1)})) == str("abcdefghhhhh"));   // a small offset in the 4-byte form
    CHECK(decode(cat({pre(9), lit(d8), copy2(1, 8)})) == str("abcdefgha"));       // offset equal to the output position
    {
        Bytes run = cat({pre(1 + 64 + 11), lit(str("z")), copy2(64, 1), copy1(11, 1)});   // fe 01 00: a run
        CHECK(run[3] == 0xFE && run[4] == 1 && run[5] == 0 && decode(run) == Bytes(76, 'z'));
        const Bytes far = pattern(2047, 3);
        CHECK(decode(cat({pre(2047 + 11), lit(far), copy1(11, 2047)})) == cat({far, Bytes(far.begin(), far.begin() + 11)}));
        const Bytes full = pattern(65535, 5);
        CHECK(decode(cat({pre(65536), lit(full), copy2(1, 65535)})) == cat({full, Bytes(1, full[0])}));
    }
    // each malformed block is refused, as a whole and cut at every byte
    const struct { const char* name; Bytes b; } bad[] = {
        {"offset 0", cat({pre(12), lit(d8), copy2(4, 0)})},
        {"copy at output position 0", cat({pre(4), copy2(4, 1)})},
        {"offset one past the output", cat({pre(12), lit(d8), copy2(4, 9)})},
        {"cut copy-1", cat({pre(12), lit(d8), {copy1(4, 1)[0]}})},
        {"cut copy-4", cat({pre(12), lit(d8), {copy4(4, 1)[0], 1, 0, 0}})},
        {"cut length bytes", cat({pre(300), {(u8)(61 << 2), 0x2B}})},
        {"literal over the size", cat({pre(7), lit(d8)})},
        {"copy over the size", cat({pre(11), lit(d8), copy2(4, 8)})},
        {"input left at the size", cat({pre(8), lit(d8), lit(str("x"))})},
        {"output under the size", cat({pre(13), lit(d8), copy2(4, 8)})},
        {"only a preamble", pre(5)},
        {"a preamble of 0", pre(0)},
        {"a preamble of 65537", cat({pre(65537), lit(str("x"))})},
        {"a 6-byte preamble", cat({six, lit(d8)})},
        {"a 4-byte literal length of 2^32 - 1", cat({pre(8), {(u8)(63 << 2), 255, 255, 255, 255}, d8})},
    };
    for (const auto& c : bad) {
        if (!decode(c.b).empty()) { std::printf("FAIL accepted: %s\n", c.name); ++fails; }
    }
    const Bytes good = cat({pre(8 + 4 + 11 + 64 + 300), lit(d8), copy1(4, 8), copy2(11, 3), copy4(64, 20), lit(pattern(300, 1))});
    CHECK(decode(good).size() == 387);
    for (u64 n = 0; n < good.size(); ++n) {
        const Bytes cutb(good.begin(), good.begin() + (ptrdiff_t)n);
        CHECK(decode(cutb).empty());
    }
}

static void test_compressor() {
    u32 forms[4] = {0, 0, 0, 0}, overlaps = 0;
    std::vector<Bytes> inputs = {Bytes(1, 'x'), str("abc"), Bytes(5000, 'r'), pattern(65536, 9), pattern(40000, 2)};
    Bytes mixed = pattern(70, 1);            // a far repeat (copy-4), near repeats (copy-1), runs (offset 1)
    put(mixed, Bytes(40000, 0));
    for (u32 i = 0; i < 40000; ++i) mixed[70 + i] = (u8)((i * 2654435761u) >> 13);
    put(mixed, pattern(70, 1));
    put(mixed, Bytes(300, 'q'));
    put(mixed, str("0123456789"));
    put(mixed, str("0123456789"));
    inputs.push_back(mixed);
    Bytes noise(65536);
    u32 x = 12345;
    for (u8& b : noise) b = (u8)((x = x * 1664525u + 1013904223u) >> 24);
    inputs.push_back(noise);
    for (const Bytes& raw : inputs) {
        Bytes z(snappy_bound((u32)raw.size()));
        const u32 n = snappy_compress_block(raw.data(), (u32)raw.size(), z.data());
        CHECK(n <= snappy_bound((u32)raw.size()));
        z.resize(n);
        CHECK(decode(z) == raw);
        SnappyHostIn src{z.data()};
        u32 ip = 0, op = 0;
        const u32 rawn = snappy_block_raw(src, n, &ip);
        CHECK(rawn == raw.size());
        while (ip < n) {
            SnappyEl e;
            if (snappy_read_el(src, ip, n, op, rawn, &e) != SNAPPY_EL_OK) { CHECK(false); break; }
            ++forms[z[ip] & 3];
            overlaps += e.offset && e.offset < e.len;
            op += e.len;
            ip = e.next;
        }
    }
    CHECK(forms[0] && forms[1] && forms[2] && forms[3] && overlaps);
    CHECK(snappy_bound(65536) == SNAPPY_MAX_COMP && SNAPPY_MAX_COMP == 76490);
}

static Bytes be32(int32_t v) { return {(u8)(v >> 24), (u8)(v >> 16), (u8)(v >> 8), (u8)v}; }
static Bytes xerial_of(const std::vector<Bytes>& chunks, int32_t version = 1, int32_t compat = 1) {
    Bytes b(XERIAL_MAGIC, XERIAL_MAGIC + 8);
    put(b, be32(version));
    put(b, be32(compat));
    for (const Bytes& c : chunks) {
        put(b, be32((int32_t)c.size()));
        put(b, c);
    }
    return b;
}
static Bytes zblock(const Bytes& raw) {
    Bytes z(snappy_bound((u32)raw.size()));
    z.resize(snappy_compress_block(raw.data(), (u32)raw.size(), z.data()));
    return z;
}

static void test_section_index() {
    const Bytes a = zblock(pattern(500, 1)), b = zblock(pattern(70, 2));
    const Bytes x = xerial_of({a, b});
    ysb_lz4_frame_block blk[4];
    u64 n = 0;
    SnappyError err;
    CHECK(snappy_index(x.data(), x.size(), blk, 4, &n, &err) == YSB_OK && n == 2);
    CHECK(blk[0].offset == 20 && blk[0].comp_bytes == (a.size() | SNAPPY_BLOCK) && blk[1].offset == 24 + a.size() &&
          blk[1].comp_bytes == (b.size() | SNAPPY_BLOCK));
    CHECK(snappy_index(x.data(), x.size(), nullptr, 0, &n, &err) == YSB_OK && n == 2);   // counting alone
    CHECK(snappy_index(a.data(), a.size(), blk, 4, &n, &err) == YSB_OK && n == 1 && blk[0].offset == 0 &&
          blk[0].comp_bytes == (a.size() | SNAPPY_BLOCK));
    const Bytes none = xerial_of({});
    CHECK(snappy_index(none.data(), none.size(), blk, 4, &n, &err) == YSB_OK && n == 0);
    // every refusal names the byte and the rule
    Bytes neg = xerial_of({a});
    std::memcpy(neg.data() + 16, be32(-3).data(), 4);
    Bytes zero = xerial_of({a});
    std::memcpy(zero.data() + 16, be32(0).data(), 4);
    Bytes past = xerial_of({a});
    std::memcpy(past.data() + 16, be32((int32_t)a.size() + 1).data(), 4);
    Bytes trail = xerial_of({a});
    put(trail, {0, 0, 1});
    const Bytes hdr_cut(x.begin(), x.begin() + 12);
    const Bytes big_raw = cat({pre(65537), lit(str("x"))}), zero_raw = pre(0), six = {0x88, 0x80, 0x80, 0x80, 0x80, 0x00, 0x01};
    const struct { const char* name; Bytes s; u64 at; const char* word; } cases[] = {
        {"compatible version", xerial_of({a}, 1, 2), 12, "compatible version 2"},
        {"negative chunk", neg, 16, "chunk length -3"},
        {"zero chunk", zero, 16, "chunk length 0"},
        {"chunk past the section", past, 16, "runs past the records section"},
        {"trailing bytes", trail, 20 + a.size(), "3 trailing bytes"},
        {"header cut", hdr_cut, 8, "header is cut"},
        {"a raw block above 64 KiB", big_raw, 0, "a raw block of 65537 bytes"},
        {"the same inside a chunk", xerial_of({a, big_raw}), 24 + a.size(), "batch.size of at most 64 KiB"},
        {"a raw size of 0", zero_raw, 0, "a raw block of 0 bytes"},
        {"a 6-byte preamble", six, 0, "preamble is not a varint"},
        {"an empty section", Bytes(), 0, "empty records section"},
    };
    for (const auto& c : cases) {
        const auto p = exact(c.s, c.s.size());
        SnappyError e;
        const int rc = snappy_index(p.get(), c.s.size(), blk, 4, &n, &e);
        char at[32];
        std::snprintf(at, sizeof at, "byte %llu:", (unsigned long long)c.at);
        if (rc != YSB_ERR_FORMAT || e.at != c.at || !std::strstr(e.msg, c.word) || !std::strstr(e.msg, at)) {
            std::printf("FAIL refusal %s: rc %d at %llu: %s\n", c.name, rc, (unsigned long long)e.at, e.msg);
            ++fails;
        }
    }
    // a stream cut at every byte is indexed or refused, never read past its end
    for (u64 k = 0; k < x.size(); ++k) {
        const auto p = exact(x, k);
        SnappyError e;
        const int rc = snappy_index(p.get(), k, blk, 4, &n, &e);
        CHECK(rc == YSB_OK || rc == YSB_ERR_FORMAT);
        // (2..7 bytes of the magic are no magic: a raw block whose preamble, 82 53, says 10626 -- the index reads no further)
        CHECK(rc != YSB_OK || (k >= 2 && k < 8) || k == 16 || k == 20 + a.size());
    }
}

// ---- Kafka batches ------------------------------------------------------------------------------------
static Bytes vint(int32_t v) {
    u8 t[8];
    return Bytes(t, t + kafka_put_vint(t, v));
}
static Bytes record(const Bytes& value, int32_t offset_delta) {
    Bytes body = {0};
    put(body, {0});   // timestampDelta 0
    put(body, vint(offset_delta));
    put(body, vint(-1));
    put(body, vint((int32_t)value.size()));
    put(body, value);
    put(body, vint(0));
    Bytes r = vint((int32_t)body.size());
    put(r, body);
    return r;
}
static Bytes records(u32 n, u32 vlen, u32 seed, Bytes* values) {
    Bytes all;
    for (u32 i = 0; i < n; ++i) {
        const Bytes v = pattern(vlen, seed + i);
        put(all, record(v, (int32_t)i));
        put(*values, v);
    }
    return all;
}
static Bytes batch(const Bytes& recs, u32 count, u32 attributes, i64 base_offset) {
    Bytes b(KAFKA_HEADER);
    put(b, recs);
    u8* h = b.data();
    kafka_put_be(h, 8, (u64)base_offset);
    kafka_put_be(h + 8, 4, b.size() - KAFKA_LEN_BASE);
    h[16] = 2;
    kafka_put_be(h + 21, 2, attributes);
    kafka_put_be(h + 23, 4, count ? count - 1 : 0);
    kafka_put_be(h + 43, 8, ~0ull);
    kafka_put_be(h + 51, 2, 0xFFFF);
    kafka_put_be(h + 53, 4, 0xFFFFFFFFu);
    kafka_put_be(h + 57, 4, count);
    kafka_put_be(h + 17, 4, kafka_crc32c(h + KAFKA_CRC_FROM, b.size() - KAFKA_CRC_FROM));
    return b;
}
static Bytes xerial_chunks(const Bytes& raw, u32 chunk) {
    std::vector<Bytes> c;
    for (u64 a = 0; a < raw.size(); a += chunk)
        c.push_back(zblock(Bytes(raw.begin() + (ptrdiff_t)a, raw.begin() + (ptrdiff_t)std::min<u64>(raw.size(), a + chunk))));
    return xerial_of(c);
}

struct Indexed {
    int rc;
    std::vector<ysb_kafka_batch> b;
    std::vector<ysb_kafka_frame> f;
    std::vector<ysb_lz4_frame_block> k;
    ysb_kafka_lz4_summary s{};
    KafkaError err{};
};
static Indexed index_of(const u8* p, u64 n, u32 flags) {
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

static void test_kafka_layer() {
    Bytes values;
    const Bytes r0 = records(3, 40, 1, &values), r1 = records(40, 90, 2, &values), r2 = records(5, 30, 3, &values),
                r3 = records(4, 50, 4, &values);
    Bytes lz(lz4f_bound(r3.size(), 65536));
    lz.resize(lz4f_pack(r3.data(), r3.size(), 65536, 1, lz.data()));
    Bytes blob = batch(r0, 3, 0, 0);
    const u64 at1 = blob.size();
    put(blob, batch(xerial_chunks(r1, 100), 40, 2, 3));      // records straddle the chunks
    const u64 at2 = blob.size();
    put(blob, batch(zblock(r2), 5, 2, 43));                  // one raw block
    put(blob, batch(lz, 4, 3, 48));
    const u32 F = YSB_KAFKA_CHECK_CRC | YSB_KAFKA_ACCEPT_SNAPPY;

    // the opt-in: without the flag a codec-2 batch is refused by name, as before
    Indexed no = index_of(blob.data(), blob.size(), YSB_KAFKA_CHECK_CRC);
    char want[96];
    std::snprintf(want, sizeof want, "Kafka batch 1 at byte %llu: attributes.codec = 2: snappy-compressed", (unsigned long long)at1);
    CHECK(no.rc == YSB_ERR_FORMAT && std::strstr(no.err.msg, want) && std::strstr(no.err.msg, "codec 0, none, and 3, lz4, only"));

    Indexed x = index_of(blob.data(), blob.size(), F);
    CHECK(x.rc == YSB_OK && x.s.n_batches == 4 && x.s.n_records == 52 && x.s.compressed_batches == 3 && x.s.consumed == blob.size());
    const u32 nchunks = (u32)((r1.size() + 99) / 100);
    CHECK(x.f[0].codec == 0 && x.f[1].codec == 2 && x.f[1].n_blocks == nchunks && x.f[2].codec == 2 && x.f[2].n_blocks == 1 &&
          x.f[3].codec == 3 && x.s.blocks == 1 + nchunks + 1 + x.f[3].n_blocks);
    CHECK(x.k[1].offset == at1 + KAFKA_HEADER + 20 && (x.k[1].comp_bytes & SNAPPY_BLOCK) && !(x.k[0].comp_bytes & SNAPPY_BLOCK));
    CHECK(x.k[1 + nchunks].offset == at2 + KAFKA_HEADER && x.k[1 + nchunks].comp_bytes == ((x.b[2].records_bytes) | SNAPPY_BLOCK));
    u64 wire = 0;   // the summary's wire bytes are the entries'
    for (const ysb_lz4_frame_block& e : x.k) wire += e.comp_bytes & SNAPPY_LEN_MASK;
    CHECK(x.s.comp_bytes == wire && wire > r0.size() + x.b[2].records_bytes);

    // the entries' rules: codec 2 only with the mask; a tag outside a codec-2 frame and an untagged block inside one
    u64 nrec = 0, snappy = 0;
    KafkaError err;
    CHECK(kafka_lz4_entries(x.b.data(), x.f.data(), 4, x.k.data(), x.k.size(), blob.size(), &nrec, nullptr, nullptr, nullptr, &err) == YSB_ERR_ARG);
    CHECK(std::strstr(err.msg, "codec 2"));
    CHECK(kafka_lz4_entries(x.b.data(), x.f.data(), 4, x.k.data(), x.k.size(), blob.size(), &nrec, nullptr, nullptr, nullptr, &err,
                            KAFKA_CODECS_ALL, &snappy) == YSB_OK && nrec == 52 && snappy == nchunks + 1);
    {
        std::vector<ysb_lz4_frame_block> k = x.k;
        k[0].comp_bytes |= SNAPPY_BLOCK;
        CHECK(kafka_lz4_entries(x.b.data(), x.f.data(), 4, k.data(), k.size(), blob.size(), &nrec, nullptr, nullptr, nullptr, &err, KAFKA_CODECS_ALL) == YSB_ERR_ARG);
        k = x.k;
        k[2].comp_bytes &= SNAPPY_LEN_MASK;
        CHECK(kafka_lz4_entries(x.b.data(), x.f.data(), 4, k.data(), k.size(), blob.size(), &nrec, nullptr, nullptr, nullptr, &err, KAFKA_CODECS_ALL) == YSB_ERR_ARG);
        k = x.k;
        k[2].comp_bytes |= LZ4_STORED;
        CHECK(kafka_lz4_entries(x.b.data(), x.f.data(), 4, k.data(), k.size(), blob.size(), &nrec, nullptr, nullptr, nullptr, &err, KAFKA_CODECS_ALL) == YSB_ERR_ARG);
        k = x.k;
        k[2].comp_bytes = (x.b[1].records_bytes + 1) | SNAPPY_BLOCK;   // past its batch's records
        CHECK(kafka_lz4_entries(x.b.data(), x.f.data(), 4, k.data(), k.size(), blob.size(), &nrec, nullptr, nullptr, nullptr, &err, KAFKA_CODECS_ALL) == YSB_ERR_ARG);
    }

    // the host model: the values of all four batches, in an exact-size buffer
    {
        const auto p = exact(blob, blob.size());
        Bytes out(values.size());
        std::vector<u32> off(53);
        u64 nl = 0, nb = 0, infl = 0;
        ysb_kafka_verdict vd{};
        CHECK(kafka_unframe_lz4(p.get(), blob.size(), x.b.data(), x.f.data(), 4, x.k.data(), x.k.size(), out.data(), out.size(),
                                off.data(), off.size(), &nl, &nb, &infl, nullptr, &vd, &err, true, KAFKA_CODECS_ALL) == YSB_OK);
        CHECK(nl == 52 && nb == values.size() && out == values && infl == r0.size() + r1.size() + r2.size() + r3.size());
        CHECK(kafka_unframe_lz4(p.get(), blob.size(), x.b.data(), x.f.data(), 4, x.k.data(), x.k.size(), nullptr, 0, nullptr, 0, &nl,
                                &nb, nullptr, nullptr, &vd, &err) == YSB_ERR_ARG);   // the default mask
    }
    // a bad chunk in the middle batch is rule 8 with its block; a flipped wire byte with the CRC checked is rule 9
    {
        Bytes bad = blob;
        const u64 j = 1 + nchunks / 2;
        bad[x.k[j].offset] ^= 0x7F;   // the chunk's preamble: another raw size
        ysb_kafka_verdict vd{};
        u64 nl = 0, nb = 0;
        CHECK(kafka_unframe_lz4(bad.data(), bad.size(), x.b.data(), x.f.data(), 4, x.k.data(), x.k.size(), nullptr, 0, nullptr, 0, &nl,
                                &nb, nullptr, nullptr, &vd, &err, false, KAFKA_CODECS_ALL) == YSB_ERR_FORMAT);
        CHECK(vd.bad_batches == 1 && vd.first_bad == 1 && vd.rule == KAFKA_R_CODEC && vd.record == nchunks / 2);
        CHECK(std::strstr(err.msg, "batch 1") && std::strstr(err.msg, "baseOffset 3") && std::strstr(err.msg, "block"));
        CHECK(kafka_unframe_lz4(bad.data(), bad.size(), x.b.data(), x.f.data(), 4, x.k.data(), x.k.size(), nullptr, 0, nullptr, 0, &nl,
                                &nb, nullptr, nullptr, &vd, &err, true, KAFKA_CODECS_ALL) == YSB_ERR_FORMAT);
        CHECK(vd.first_bad == 1 && vd.rule == KAFKA_R_CRC);
    }
    // a section refusal becomes the Kafka batch's, naming both bytes
    {
        Bytes sect = xerial_chunks(r1, 100);
        sect.push_back(9);
        Bytes b2 = batch(r0, 3, 0, 0);
        put(b2, batch(sect, 40, 2, 3));
        Indexed r = index_of(b2.data(), b2.size(), F);
        char where[64], chunk[48];
        std::snprintf(where, sizeof where, "%llu bytes at byte %llu,", (unsigned long long)sect.size(), (unsigned long long)(at1 + KAFKA_HEADER));
        std::snprintf(chunk, sizeof chunk, "snappy: byte %llu: 1 trailing bytes", (unsigned long long)(sect.size() - 1));
        CHECK(r.rc == YSB_ERR_FORMAT && std::strstr(r.err.msg, "Kafka batch 1 at byte") &&
              std::strstr(r.err.msg, "attributes.codec = 2") && std::strstr(r.err.msg, where) && std::strstr(r.err.msg, chunk));
    }
    // the blob cut at every byte: indexed up to the last whole batch or refused, never read past its end
    for (u64 n = 0; n < blob.size(); n += 1 + n / 64) {
        const auto p = exact(blob, n);
        Indexed c = index_of(p.get(), n, F);
        CHECK(c.rc == YSB_OK && c.s.consumed <= n);
    }
}

static void test_packer() {
    Bytes lines;
    std::vector<u32> off;
    for (u32 i = 0; i < 900; ++i) {
        off.push_back((u32)lines.size());
        put(lines, pattern(60 + i % 50, i % 17));
    }
    for (u32 framing : {YSB_KAFKA_SNAPPY_XERIAL, YSB_KAFKA_SNAPPY_RAW})
        for (u32 chunk : {0u, 1u, 77u, 65536u}) {
            ysb_kafka_pack_opts o{};
            o.codec = YSB_KAFKA_CODEC_SNAPPY;
            o.batch_bytes = framing == YSB_KAFKA_SNAPPY_RAW ? 30000 : chunk == 1 ? 4000 : 100000;
            o.base_offset = 7;
            o.snappy_framing = framing;
            o.snappy_chunk = chunk;
            Bytes dst(kafka_bound(lines.size(), off.size(), o));
            u64 nb = 0;
            const u64 n = kafka_pack_lz4(lines.data(), lines.size(), off.data(), off.size(), o, dst.data(), &nb);
            CHECK(n != KAFKA_PACK_RAW_OVER && n <= dst.size());
            const auto p = exact(dst, n);
            Indexed x = index_of(p.get(), n, YSB_KAFKA_CHECK_CRC | YSB_KAFKA_ACCEPT_SNAPPY);
            CHECK(x.rc == YSB_OK && x.s.n_batches == nb && x.s.n_records == 900 && x.s.consumed == n && x.s.compressed_batches == nb);
            if (framing == YSB_KAFKA_SNAPPY_RAW) CHECK(x.s.blocks == nb);
            else if (chunk == 1) CHECK(x.s.blocks > 50000);
            Bytes out(lines.size());
            std::vector<u32> lo(901);
            u64 nl = 0, ob = 0;
            KafkaError err;
            CHECK(kafka_unframe_lz4(p.get(), n, x.b.data(), x.f.data(), x.b.size(), x.k.data(), x.k.size(), out.data(), out.size(), lo.data(),
                                    lo.size(), &nl, &ob, nullptr, nullptr, nullptr, &err, false, KAFKA_CODECS_ALL) == YSB_OK);
            CHECK(nl == 900 && out == lines && std::memcmp(lo.data(), off.data(), 900 * 4) == 0 && x.b[0].base_offset == 7);
        }
    // one raw block cannot hold a batch of more than 64 KiB of records
    ysb_kafka_pack_opts o{};
    o.codec = YSB_KAFKA_CODEC_SNAPPY;
    o.batch_bytes = 100000;
    o.snappy_framing = YSB_KAFKA_SNAPPY_RAW;
    Bytes dst(kafka_bound(lines.size(), off.size(), o));
    u64 nb = 0;
    CHECK(kafka_pack_lz4(lines.data(), lines.size(), off.data(), off.size(), o, dst.data(), &nb) == KAFKA_PACK_RAW_OVER);
}

int main() {
    test_reader_and_decoder();
    test_compressor();
    test_section_index();
    test_kafka_layer();
    test_packer();
    std::printf(fails ? "%d FAILED\n" : "snappy_logic OK\n", fails);
    return fails ? 1 : 0;
}
