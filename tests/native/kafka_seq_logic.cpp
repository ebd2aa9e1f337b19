// The generated Kafka corpus (tests/kafka_seqgen.py) through the host side of csrc/ysb_kafka.h:
// the record reader the kernels share, in the serial model's order (kafka_unframe_batch) and in
// the walk kernel's (walk_like_kernel, kafka_walk.h).  argv[1] is the corpus file that
// tests/test_kafka_seq_logic.py writes: u32 count, then per batch u32 name length, the name, u32
// recordsCount, bad record, rule (0: valid), u64 value bytes, u32 null values, keyed, headers, u32
// record bytes, the record bytes.  For every batch: the two orders agree, they give the stated
// verdict, and a valid batch returns its stated totals; every batch of at most SMALL bytes is
// also cut at every byte, where the two orders must agree.  Every input lives in a heap buffer of
// its exact size, so the same program built with -fsanitize=address,undefined shows any read one
// byte out of range -- the gate for sending the malformed batches to a GPU.
// Built and run by tests/test_kafka_seq_logic.py with g++ (no GPU, no HIP header).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>
#include "ysb_kafka.h"
#include "kafka_walk.h"

using namespace ysb;

static int fails = 0;
#define CHECK(name, ...) do { if (!(__VA_ARGS__)) { std::printf("FAIL %s: %s\n", (name).c_str(), #__VA_ARGS__); ++fails; } } while (0)

constexpr u32 SMALL = 256;

struct Result {
    u32 rule, rec;
    u64 bytes;
    ysb_kafka_counters ct;
};

// `n` record bytes with recordsCount `count` in an exact-size heap buffer, in both orders
static bool both(const std::string& name, const u8* bytes, u32 n, u32 count, Result* r) {
    std::unique_ptr<u8[]> p(new u8[n ? n : 1]);
    if (n) std::memcpy(p.get(), bytes, n);
    const ysb_kafka_batch b{0, n, count, 0, 0, 0, 0};
    std::unique_ptr<u8[]> out(new u8[n ? n : 1]);
    std::vector<u32> off((size_t)std::min<u32>(count, n) + 1);   // (a record takes a byte at least: no more are written)
    Result a{}, w{};
    u64 at = 0;
    a.rule = kafka_unframe_batch(p.get(), b, out.get(), n, off.data(), &at, &a.ct, &a.rec);
    a.bytes = at;
    w.rule = walk_like_kernel(p.get(), n, count, &w.rec, &w.bytes, &w.ct);
    const bool same = a.rule == w.rule && a.rec == w.rec &&
                      (a.rule || (a.bytes == w.bytes && a.ct.records == w.ct.records && a.ct.null_values == w.ct.null_values &&
                                  a.ct.keyed == w.ct.keyed && a.ct.headers == w.ct.headers));
    CHECK(name, same);
    *r = a;
    return same;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::printf("usage: kafka_seq_logic CORPUS\n"); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    const std::vector<u8> file((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    size_t at = 0;
    auto need = [&](size_t n) {
        if (file.size() - at < n) { std::printf("FAIL: the corpus file ends early\n"); std::exit(1); }
    };
    auto word = [&]() -> u32 {
        need(4);
        u32 v;
        std::memcpy(&v, file.data() + at, 4);
        at += 4;
        return v;
    };
    const u32 total = word();
    u32 n_valid = 0, n_bad = 0, n_cuts = 0;
    for (u32 i = 0; i < total; ++i) {
        const u32 name_len = word();
        need(name_len);
        const std::string name(reinterpret_cast<const char*>(file.data() + at), name_len);
        at += name_len;
        const u32 count = word(), rec = word(), rule = word();
        need(8);
        u64 value_bytes;
        std::memcpy(&value_bytes, file.data() + at, 8);
        at += 8;
        const u32 nulls = word(), keyed = word(), headers = word(), n = word();
        need(n);
        const u8* bytes = file.data() + at;
        at += n;
        Result r{};
        both(name, bytes, n, count, &r);
        CHECK(name, r.rule == rule && r.rec == rec);
        if (!rule) {
            ++n_valid;
            CHECK(name, r.bytes == value_bytes && r.ct.records == count && r.ct.null_values == nulls && r.ct.keyed == keyed &&
                            r.ct.headers == headers);
        } else {
            ++n_bad;
        }
        if (n <= SMALL)
            for (u32 c = 0; c < n; ++c, ++n_cuts) both(name + " (cut)", bytes, c, count, &r);
    }
    if (at != file.size()) { std::printf("FAIL: %zu bytes behind the last batch\n", file.size() - at); ++fails; }
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("%u valid and %u bad batches, %u cuts: kafka seq logic OK\n", n_valid, n_bad, n_cuts);
    return 0;
}
