// Host-side checks of the LZ4 batch rules (csrc/ysb_lz4.h): the sequence reader the kernel of
// csrc/ysb_lz4.hip shares, the host decoder (the model), the compressor, the directory's checks,
// line-aligned cuts and the kernel's in-place window geometry.  Every input and output lives in
// a heap buffer of its exact size, so the same program built with -fsanitize=address,undefined
// (tests/test_lz4_logic.py) shows any read or write one byte out of range.
// Built and run by tests/test_lz4_logic.py with g++ (no GPU, no HIP header).
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>
#include "ysb_lz4.h"

using namespace ysb;
typedef std::vector<u8> Bytes;

static int fails = 0;
#define CHECK(...) do { if (!(__VA_ARGS__)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #__VA_ARGS__); ++fails; } } while (0)

static std::string golden(const char* name) {
    std::string p = __FILE__;   // .../tests/native/lz4_logic.cpp
    p = p.substr(0, p.rfind('/'));
    return p.substr(0, p.rfind('/')) + "/golden/" + name;
}
static Bytes slurp(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    return Bytes(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

// exact-size heap copies in and out: decode `comp` as an entry, compare with `want` (NULL: must be bad)
static bool decodes_to(const Bytes& comp, u32 field_flags, u32 raw, const Bytes* want, bool* in_place = nullptr) {
    std::unique_ptr<u8[]> in(new u8[comp.size() ? comp.size() : 1]);
    if (!comp.empty()) std::memcpy(in.get(), comp.data(), comp.size());
    std::unique_ptr<u8[]> out(new u8[raw ? raw : 1]);
    const ysb_lz4_block e{(u32)comp.size() | field_flags, raw};
    bool ip_ok = true;
    const bool ok = lz4_decode_block(in.get(), e, out.get(), &ip_ok);
    if (in_place) *in_place = ip_ok;
    if (!want) return !ok;
    return ok && want->size() == raw && std::memcmp(out.get(), want->data(), raw) == 0;
}

// data -> blocks -> the host decoder -> data; every compressed block within its bound and
// decodable in place in the kernel's window
static void round_trip(const Bytes& data, u32 block, bool aligned, bool allow_stored, u64* comp_total = nullptr,
                       u64* stored = nullptr) {
    u64 at = 0, total = 0, st = 0;
    while (at < data.size()) {
        const u64 end = lz4_block_end(data.data(), data.size(), at, block, aligned);
        const u32 n = (u32)(end - at);
        CHECK(n >= 1 && n <= block);
        if (aligned && end < data.size() && n < block) CHECK(data[end - 1] == '\n' || data[end - 1] == '\r');
        Bytes src(data.begin() + at, data.begin() + end), dst(lz4_compress_bound(n));
        const ysb_lz4_block e = lz4_pack_block(src.data(), n, dst.data(), allow_stored);
        const u32 cb = lz4_entry_comp(e);
        CHECK(cb <= lz4_compress_bound(n) && e.raw_bytes == n);
        if (!allow_stored) CHECK(!(e.comp_bytes & LZ4_STORED));
        dst.resize(cb);
        bool in_place = false;
        if (!decodes_to(dst, e.comp_bytes & LZ4_STORED, n, &src, &in_place) || !in_place) {
            std::printf("FAIL round trip: block at %llu of %u bytes (block size %u)\n", (unsigned long long)at, n, block);
            ++fails;
            return;
        }
        st += (e.comp_bytes & LZ4_STORED) ? 1 : 0;
        total += cb;
        at = end;
    }
    if (comp_total) *comp_total = total;
    if (stored) *stored = st;
}

static Bytes lits(u32 n, u32 seed) {
    Bytes b(n);
    for (u32 i = 0; i < n; ++i) b[i] = (u8)(seed * 37 + i * 11);
    return b;
}
static Bytes cat(std::initializer_list<Bytes> parts) {
    Bytes o;
    for (const Bytes& p : parts) o.insert(o.end(), p.begin(), p.end());
    return o;
}

static void test_round_trips() {
    for (const char* name : {"gen_s7.jsonl", "gen_s7.tbl"}) {
        const Bytes data = slurp(golden(name));
        CHECK(data.size() > 65536);
        for (u32 block : {1u, 13u, 64u, 4096u, 65536u}) {
            // (1-byte blocks over the first 8 KiB only: 700,000 blocks say nothing more)
            const Bytes part = block == 1 ? Bytes(data.begin(), data.begin() + 8192) : data;
            round_trip(part, block, false, true);
            round_trip(part, block, true, true);
        }
        u64 c16 = 0;
        round_trip(data, 16384, true, true, &c16);
        CHECK(c16 * 10 < data.size() * 9);   // it does compress
    }
    // 65536 equal bytes: offset 1, a match length with 250-odd extension bytes
    {
        const Bytes same(65536, 0x61);
        Bytes dst(lz4_compress_bound(65536));
        const u32 cb = lz4_compress_block(same.data(), 65536, dst.data());
        CHECK(cb < 300);
        u32 n255 = 0;
        for (u32 i = 0; i < cb; ++i) n255 += dst[i] == 255;
        CHECK(n255 >= 250);
        CHECK(dst[2] == 1 && dst[3] == 0);   // token, one literal, offset 1
        round_trip(same, 65536, false, true);
    }
    // periods on either side of 4-, 16- and 64-byte copy widths
    for (u32 period : {2u, 3u, 7u, 15u, 16u, 17u, 63u, 64u, 65u}) {
        Bytes p(65536);
        for (u32 i = 0; i < p.size(); ++i) p[i] = (u8)((i % period) * 29);
        u64 c = 0;
        round_trip(p, 65536, false, true, &c);
        CHECK(c < 600);
        round_trip(p, 4099, false, true);
    }
    // 65536 random bytes: stored; one literal-only block when storing is off
    {
        Bytes r(65536);
        u64 x = 12345;
        for (u8& b : r) { x = x * 6364136223846793005ull + 1442695040888963407ull; b = (u8)(x >> 56); }
        u64 c = 0, st = 0;
        round_trip(r, 65536, false, true, &c, &st);
        CHECK(st == 1 && c == 65536);
        round_trip(r, 65536, false, false, &c, &st);
        CHECK(st == 0 && c == 65536 + 1 + 1 + (65536 - 15) / 255);   // token, extensions, literals
    }
    round_trip(Bytes(), 4096, true, true);   // empty input: no block
    u64 rt = 1;
    CHECK(lz4_check_dir(nullptr, 0, 0, &rt, nullptr) == LZ4_DIR_OK && rt == 0);
}

struct Hand {
    const char* name;
    Bytes comp, raw;
};
static std::vector<Hand> hand_blocks() {
    std::vector<Hand> h;
    const Bytes a15 = lits(15, 1), a270 = lits(270, 2), a8 = lits(8, 3), a5 = lits(5, 5), a4 = lits(4, 6);
    h.push_back({"literal length exactly 15, extension byte 0", cat({{0xF0, 0}, a15}), a15});
    h.push_back({"literal length 15 + 255, a terminating 0", cat({{0xF0, 255, 0}, a270}), a270});
    Bytes m19;
    for (u32 i = 0; i < 19; ++i) m19.push_back(a8[i % 8]);
    h.push_back({"match length exactly 19", cat({{0x8F}, a8, {8, 0, 0, 0x10, 0x77}}), cat({a8, m19, {0x77}})});
    // the largest offset a valid block can use: 65532 bytes out, a match of 4 ends the 65536
    const Bytes big = lits(65532, 4);
    Bytes hdr{0xF0};
    hdr.insert(hdr.end(), (65532 - 15) / 255, 255);
    hdr.push_back((65532 - 15) % 255);
    h.push_back({"offset 65532 = the bytes produced so far", cat({hdr, big, {0xFC, 0xFF, 0x00}}),
                 cat({big, Bytes(big.begin(), big.begin() + 4)})});
    h.push_back({"offset equal to the bytes produced so far", cat({{0x51}, a5, {5, 0, 0x10, 0x42}}), cat({a5, a5, {0x42}})});
    h.push_back({"a block of one literal", {0x10, 0x5A}, {0x5A}});
    h.push_back({"an empty last sequence after a match", cat({{0x40}, a4, {4, 0, 0x00}}), cat({a4, a4})});
    return h;
}

struct Mal {
    const char* name;
    Bytes comp;
    u32 raw;
};
static std::vector<Mal> malformed_bases() {
    const Bytes a4 = lits(4, 7), big = lits(65535, 8), ff(300, 255);
    Bytes hdr{0xF0};
    hdr.insert(hdr.end(), (65535 - 15) / 255, 255);
    hdr.push_back((65535 - 15) % 255);
    return {
        {"no input at all", {}, 1},
        {"input exhausted inside a literal extension", {0xF0, 255, 255}, 600},
        {"input exhausted inside the literals", cat({{0x80}, a4}), 8},
        {"input exhausted inside the offset", cat({{0x40}, a4, {4}}), 12},
        {"input exhausted inside a match extension", cat({{0x4F}, a4, {4, 0, 255}}), 600},
        {"offset 0", cat({{0x40}, a4, {0, 0, 0x00}}), 12},
        {"offset before the block's start", cat({{0x40}, a4, {5, 0, 0x00}}), 12},
        {"literals past raw_bytes", cat({{0x40}, a4}), 3},
        {"match past raw_bytes", cat({{0x40}, a4, {4, 0, 0x00}}), 7},
        {"fewer bytes than raw_bytes", cat({{0x40}, a4}), 5},
        {"more: input left after raw_bytes are out", cat({{0x40}, a4, {4, 0, 0x10, 0x33}}), 8},
        {"the block ends with a match", cat({{0x40}, a4, {4, 0}}), 8},
        {"offset 65535 in a 65536-byte block", cat({hdr, big, {0xFF, 0xFF, 0x00}}), 65536},
        {"a literal length of 64 KiB of 255s", cat({{0xF0}, ff}), 65536},
        {"a match length far past raw_bytes", cat({{0x4F}, a4, {1, 0}, ff, {0, 0}}), 65536},
    };
}

static void test_hand_and_malformed() {
    for (const Hand& h : hand_blocks()) {
        bool in_place = false;
        if (!decodes_to(h.comp, 0, (u32)h.raw.size(), &h.raw, &in_place) || !in_place) {
            std::printf("FAIL hand block: %s\n", h.name);
            ++fails;
        }
        // ... and with any other raw size it is bad
        CHECK(decodes_to(h.comp, 0, (u32)h.raw.size() + 1, nullptr));
        if (h.raw.size() > 1) CHECK(decodes_to(h.comp, 0, (u32)h.raw.size() - 1, nullptr));
        for (size_t cut = 0; cut < h.comp.size() && h.comp.size() <= 400; ++cut)
            CHECK(decodes_to(Bytes(h.comp.begin(), h.comp.begin() + cut), 0, (u32)h.raw.size(), nullptr));
    }
    for (const Mal& m : malformed_bases()) {
        if (!decodes_to(m.comp, 0, m.raw, nullptr)) {
            std::printf("FAIL malformed block accepted: %s\n", m.name);
            ++fails;
        }
        for (size_t cut = 0; cut < m.comp.size() && m.comp.size() <= 400; ++cut)
            CHECK(decodes_to(Bytes(m.comp.begin(), m.comp.begin() + cut), 0, m.raw, nullptr));
    }
    // stored blocks: exactly raw_bytes bytes; the directory's own rules
    CHECK(decodes_to({1, 2, 3}, LZ4_STORED, 3, nullptr) == false);
    const Bytes s3{1, 2, 3};
    CHECK(decodes_to(s3, LZ4_STORED, 3, &s3));
    CHECK(decodes_to(s3, LZ4_STORED, 4, nullptr) && decodes_to(s3, LZ4_STORED, 2, nullptr));
    CHECK(decodes_to({0x10, 0x5A}, 0, 0, nullptr) && decodes_to({0x10, 0x5A}, 0, 65537, nullptr));
    const ysb_lz4_block dir[3] = {{2, 1}, {3 | LZ4_STORED, 3}, {2, 1}};
    u64 raw = 0;
    u32 at = 9;
    CHECK(lz4_check_dir(dir, 3, 7, &raw, &at) == LZ4_DIR_OK && raw == 5);
    CHECK(lz4_check_dir(dir, 3, 8, &raw, &at) == LZ4_DIR_SUM);
    const ysb_lz4_block dir0[2] = {{2, 1}, {2, 0}}, dirbig[1] = {{2, 65537}};
    CHECK(lz4_check_dir(dir0, 2, 4, &raw, &at) == LZ4_DIR_RAW && at == 1);
    CHECK(lz4_check_dir(dirbig, 1, 2, &raw, &at) == LZ4_DIR_RAW && at == 0);
    // a batch: good, bad, good -> the first bad block is 1, its neighbours decode
    const Bytes blob{0x10, 0x41, 0x40, 1, 2, 3, 4, 0, 0, 0x00, 0x10, 0x42};
    const ysb_lz4_block bd[3] = {{2, 1}, {8, 8}, {2, 1}};
    Bytes out(10, 0xEE);
    CHECK(lz4_decode_batch(blob.data(), bd, 3, out.data()) == 1 && out[0] == 0x41 && out[9] == 0x42);
    // the kernel's window: the launch's LDS holds any block's window and its two alignment pads
    CHECK(lz4_lds_bytes(LZ4_MAX_RAW) == 66096 && lz4_lds_bytes(16384) <= 16600);
    for (u32 r : {1u, 13u, 4096u, 65536u}) CHECK(r + r / 255 + 2 <= lz4_window(r) && 31 + lz4_window(r) <= lz4_lds_bytes(r));
}

int main() {
    test_round_trips();
    test_hand_and_malformed();
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("lz4 logic OK\n");
    return 0;
}
