// Host-side checks of the Kafka record batch rules (csrc/ysb_kafka.h): the varint reader, the
// index, the record reader the kernels of csrc/ysb_kafka.hip share, the host unframer (the
// model), CRC-32C and the packer.  Every input lives in a heap buffer of its exact size, so the
// same program built with -fsanitize=address,undefined (tests/test_kafka_logic.py) shows any read
// one byte out of range.  Built and run by tests/test_kafka_logic.py with g++ (no GPU, no HIP
// header).
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>
#include "ysb_kafka.h"
#include "kafka_walk.h"

using namespace ysb;
typedef std::vector<u8> Bytes;

static int fails = 0;
#define CHECK(...) do { if (!(__VA_ARGS__)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #__VA_ARGS__); ++fails; } } while (0)

static std::string golden(const char* name) {
    std::string p = __FILE__;   // .../tests/native/kafka_logic.cpp
    p = p.substr(0, p.rfind('/'));
    return p.substr(0, p.rfind('/')) + "/golden/" + name;
}
static Bytes slurp(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    return Bytes(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}
// an exact-size heap copy (a read past the end is the sanitizer's to find)
static std::unique_ptr<u8[]> exact(const Bytes& b) {
    std::unique_ptr<u8[]> p(new u8[b.size() ? b.size() : 1]);
    if (!b.empty()) std::memcpy(p.get(), b.data(), b.size());
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

// (the kernel's walk on the host, walk_like_kernel: kafka_walk.h)

// records `rec` with recordsCount `count` through the model and the kernel's order, in an exact-size buffer
static u32 verdict_of(const Bytes& rec, u32 count, u32* bad_rec) {
    auto p = exact(rec);
    ysb_kafka_batch b{0, (u32)rec.size(), count, 0, 0, 0, 0};
    ysb_kafka_counters ct{};
    u64 at = 0, total = 0;
    u32 r1 = 0, r2 = 0;
    Bytes out(rec.size() + 1);
    std::vector<u32> off(count + 1);
    const u32 rule = kafka_unframe_batch(p.get(), b, out.data(), out.size(), off.data(), &at, &ct, &r1);
    const u32 rule2 = walk_like_kernel(p.get(), (u32)rec.size(), count, &r2, &total);
    CHECK(rule == rule2 && r1 == r2);
    if (!rule) CHECK(total == at);
    *bad_rec = r1;
    return rule;
}

static void vectors() {
    CHECK(kafka_crc32c(reinterpret_cast<const u8*>("123456789"), 9) == 0xE3069283u);
    CHECK(kafka_crc32c(nullptr, 0) == 0);
    CHECK(kafka_zigzag32(0) == 0 && kafka_zigzag32(-1) == 1 && kafka_zigzag32(1) == 2 && kafka_zigzag32(-2) == 3);
    CHECK(kafka_unzigzag32(0xFFFFFFFFu) == INT32_MIN && kafka_unzigzag32(0xFFFFFFFEu) == INT32_MAX);
    CHECK(kafka_unzigzag64(kafka_zigzag64(INT64_MIN)) == INT64_MIN && kafka_unzigzag64(kafka_zigzag64(-7)) == -7);
    u8 t[12];
    CHECK(kafka_put_uvar(t, 300) == 2 && t[0] == 0xAC && t[1] == 0x02);
    CHECK(vint(INT32_MAX).size() == 5 && vint(INT32_MIN).size() == 5 && vlong(INT64_MIN).size() == 10);
    struct Case { Bytes b; u32 max; bool ok; u64 v; };
    const Case cases[] = {
        {{0xAC, 0x02}, 5, true, 300},
        {{0x80, 0x00}, 5, true, 0},                                         // non-minimal: legal
        {{0x81, 0x80, 0x80, 0x80, 0x00}, 5, true, 1},                       // five bytes: the limit
        {{0x80, 0x80, 0x80, 0x80, 0x80, 0x00}, 5, false, 0},                // six: illegal
        {{0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0x01}, 10, true, ~0ull},
        {{0x80, 0x80, 0x80, 0x80, 0x80, 0x80, 0x80, 0x80, 0x80, 0x80, 0x00}, 10, false, 0},
        {{0x80, 0x80}, 5, false, 0},                                        // cut
        {{}, 5, false, 0},
    };
    for (const Case& c : cases) {
        auto p = exact(c.b);
        KafkaHostIn in{p.get()};
        u32 pos = 0;
        u64 v = 0;
        const bool ok = kafka_read_uvar(in, pos, (u32)c.b.size(), c.max, &v);
        CHECK(ok == c.ok);
        if (ok) CHECK(v == c.v && pos == c.b.size());
    }
}

static void round_trip(const char* name, u32 per_batch) {
    const Bytes data = slurp(golden(name));
    CHECK(!data.empty());
    std::vector<u32> off;
    for (u64 i = 0; i < data.size(); ++i)
        if (i == 0 || data[i - 1] == '\n') off.push_back((u32)i);
    std::vector<u32> koff(off.size() + 1);
    Bytes keys;
    std::vector<i64> ts(off.size());
    for (size_t i = 0; i < off.size(); ++i) {
        koff[i] = (u32)keys.size();
        for (size_t k = 0; k < i % 40; ++k) keys.push_back((u8)('a' + k % 26));
        ts[i] = (i64)i * 1000003 - 5000;
    }
    koff[off.size()] = (u32)keys.size();
    keys.push_back(0);
    const char* hk[2] = {"trace", "n"};
    const u8* hv[2] = {reinterpret_cast<const u8*>("abc"), nullptr};
    const int32_t hl[2] = {3, -1};
    ysb_kafka_pack_opts o{};
    o.batch_records = per_batch;
    o.base_offset = 1000;
    o.base_timestamp = 1700000000000ll;
    o.key_off = koff.data();
    o.keys = keys.data();
    o.ts_delta = ts.data();
    o.n_headers = 2;
    o.header_keys = hk;
    o.header_vals = hv;
    o.header_val_len = hl;
    Bytes dst(kafka_bound(data.size(), off.size(), o));
    u64 nb = 0;
    const u64 n = kafka_pack(data.data(), data.size(), off.data(), off.size(), o, dst.data(), &nb);
    CHECK(n <= dst.size() && nb == (off.size() + per_batch - 1) / per_batch);
    dst.resize(n);
    auto p = exact(dst);
    std::vector<ysb_kafka_batch> idx(nb);
    ysb_kafka_summary s{};
    KafkaError err;
    CHECK(kafka_index(p.get(), n, YSB_KAFKA_CHECK_CRC, idx.data(), nb, &s, &err) == YSB_OK);
    CHECK(s.n_batches == nb && s.n_records == off.size() && s.consumed == n && s.crc_checked == nb);
    for (u64 k = 0; k < nb; ++k) CHECK(idx[k].base_offset == 1000 + (i64)idx[k].first_record);
    Bytes out(data.size());
    std::vector<u32> lo(off.size() + 1);
    u64 nl = 0, ob = 0;
    ysb_kafka_counters ct{};
    ysb_kafka_verdict vd{};
    CHECK(kafka_unframe(p.get(), n, idx.data(), nb, out.data(), out.size(), lo.data(), lo.size(), &nl, &ob, &ct, &vd, &err) == YSB_OK);
    CHECK(nl == off.size() && ob == data.size() && out == data && lo[nl] == data.size());
    CHECK(std::equal(off.begin(), off.end(), lo.begin()));
    CHECK(ct.records == nl && ct.null_values == 0 && ct.keyed == nl && ct.headers == 2 * nl && ct.value_bytes == ob);
    CHECK(vd.bad_batches == 0 && vd.first_bad == KAFKA_NONE);
    // every batch through the kernel's order too
    for (u64 k = 0; k < nb; ++k) {
        Bytes rec(dst.begin() + idx[k].records_off, dst.begin() + idx[k].records_off + idx[k].records_bytes);
        u32 br = 0;
        CHECK(verdict_of(rec, idx[k].n_records, &br) == KAFKA_OK);
    }
    // a flipped bit breaks the CRC and nothing else
    dst[n - 1] ^= 1;
    auto q = exact(dst);
    CHECK(kafka_index(q.get(), n, YSB_KAFKA_CHECK_CRC, idx.data(), nb, &s, &err) == YSB_ERR_FORMAT && std::strstr(err.msg, "crc"));
    CHECK(kafka_index(q.get(), n, 0, idx.data(), nb, &s, &err) == YSB_OK);
}

struct Mal { const char* name; u32 rule; u32 count; Bytes rec; u32 first = 0; };   // first: the good first record's bytes

static std::vector<Mal> corpus() {
    Bytes good;   // attributes, deltas, key "k", value, one header
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
    Bytes head = {0};   // a second record's head up to its key length
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
    for (Mal& m : c) m.first = (u32)g.size();
    return c;
}

static void malformed() {
    u32 cuts = 0;
    for (const Mal& m : corpus()) {
        u32 br = 0;
        const u32 rule = verdict_of(m.rec, m.count, &br);
        if (rule != m.rule) {
            std::printf("FAIL %s: rule %u, expected %u (record %u)\n", m.name, rule, m.rule, br);
            ++fails;
        }
        // each cut at every byte: valid only where exactly recordsCount whole records are left,
        // never a read out of range
        for (size_t n = 0; n < m.rec.size(); ++n) {
            const Bytes cut(m.rec.begin(), m.rec.begin() + n);
            CHECK((verdict_of(cut, m.count, &br) == KAFKA_OK) == (m.count == 1 && n == m.first));
            ++cuts;
        }
    }
    CHECK(cuts > 400);
    // 130 records (three groups of the kernel's walk) with the break in each group
    for (u32 at : {0u, 63u, 64u, 65u, 129u}) {
        Bytes rec;
        for (u32 i = 0; i < 130; ++i) {
            Bytes body = {0};
            put(body, vlong(i));
            put(body, vint((int32_t)i));
            put(body, vint(-1));
            put(body, vint(i == at ? 77 : 3));
            put(body, str("abc"));
            put(body, vint(0));
            put(rec, vint((int32_t)body.size()));
            put(rec, body);
        }
        u32 br = 0;
        CHECK(verdict_of(rec, 130, &br) == KAFKA_R_VALUE && br == at);
    }
}

static void index_rules() {
    const Bytes data = slurp(golden("gen_s7.jsonl"));
    std::vector<u32> off;
    for (u64 i = 0; i < data.size() && off.size() < 40; ++i)
        if (i == 0 || data[i - 1] == '\n') off.push_back((u32)i);
    const u64 nbytes = off.back();
    off.pop_back();
    ysb_kafka_pack_opts o{};
    o.batch_records = 13;
    Bytes blob(kafka_bound(nbytes, off.size(), o));
    u64 nb = 0;
    blob.resize(kafka_pack(data.data(), nbytes, off.data(), off.size(), o, blob.data(), &nb));
    CHECK(nb == 3);
    std::vector<ysb_kafka_batch> idx(8);
    ysb_kafka_summary s{};
    KafkaError err;
    CHECK(kafka_index(nullptr, 0, 0, idx.data(), 8, &s, &err) == YSB_OK && s.n_batches == 0 && s.consumed == 0);
    CHECK(kafka_index(blob.data(), blob.size(), 0, idx.data(), 8, &s, &err) == YSB_OK && s.n_batches == 3);
    const u64 last = idx[2].records_off - KAFKA_HEADER;
    // partial tails: every cut of the last batch stops in front of it
    for (u64 n = last; n < blob.size(); ++n) {
        const Bytes cut(blob.begin(), blob.begin() + n);
        auto p = exact(cut);
        CHECK(kafka_index(p.get(), n, YSB_KAFKA_CHECK_CRC, idx.data(), 8, &s, &err) == YSB_OK);
        CHECK(s.n_batches == 2 && s.consumed == last && s.n_records == 26);
    }
    // capacity: the counts are complete
    CHECK(kafka_index(blob.data(), blob.size(), 0, idx.data(), 2, &s, &err) == YSB_ERR_CAPACITY && s.n_batches == 3);
    CHECK(kafka_index(blob.data(), blob.size(), 0, nullptr, 0, &s, &err) == YSB_ERR_CAPACITY && s.n_records == 39);
    // the refusals, in the second batch
    const u64 at = idx[1].records_off - KAFKA_HEADER;
    struct R { u32 pos; u8 val; const char* field; };
    for (const R& r : {R{16, 1, "magic"}, R{16, 0, "magic"}, R{22, 3, "codec"}, R{57, 0x80, "recordsCount"}}) {
        Bytes bad = blob;
        bad[at + r.pos] = r.val;
        CHECK(kafka_index(bad.data(), bad.size(), 0, idx.data(), 8, &s, &err) == YSB_ERR_FORMAT);
        char where[32];
        std::snprintf(where, sizeof where, "at byte %llu", (unsigned long long)at);
        CHECK(std::strstr(err.msg, r.field) && std::strstr(err.msg, where));
    }
    Bytes bad = blob;
    kafka_put_be(bad.data() + at + 8, 4, 48);
    CHECK(kafka_index(bad.data(), bad.size(), 0, idx.data(), 8, &s, &err) == YSB_ERR_FORMAT && std::strstr(err.msg, "batchLength = 48"));
    // a control batch in the middle: skipped, counted, the running sum unbroken
    Bytes ctl = blob;
    ctl[at + 22] = 0x20;
    CHECK(kafka_index(ctl.data(), ctl.size(), 0, idx.data(), 8, &s, &err) == YSB_OK);
    CHECK(s.n_batches == 2 && s.control_batches == 1 && s.n_records == 26 && s.consumed == blob.size());
    CHECK(idx[1].first_record == 13 && idx[1].control_before == 1 && idx[0].control_before == 0);
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "--corpus")) {   // the malformed corpus, for the tests that reuse it
        for (const Mal& m : corpus()) {
            std::printf("%s|%u|%u|", m.name, m.rule, m.count);
            for (u8 b : m.rec) std::printf("%02x", b);
            std::printf("\n");
        }
        return 0;
    }
    vectors();
    for (const char* f : {"gen_s7.jsonl", "edge.jsonl", "edge_orgjson.jsonl", "edge_long.jsonl"})
        for (u32 per : {1u, 63u, 64u, 65u, 1000u}) round_trip(f, per);
    malformed();
    index_rules();
    std::printf(fails ? "%d checks failed\n" : "kafka_logic: OK\n", fails);
    return fails ? 1 : 0;
}
