// Host-side checks of the standard-frame rules (csrc/ysb_lz4_frame.h): XXH32, the index over
// hand-built frames and the liblz4-made fixtures (tests/golden/lz4frame), one case per refusal,
// a frame cut at every byte, the writer, the measure model against the host decoder, and the
// carry rule over whole streams of one-block batches.  Every buffer handed to the code under
// test is a heap buffer of its exact size, so the same program built with
// -fsanitize=address,undefined (tests/test_lz4_frame_logic.py) shows any access out of range.
// Built and run by tests/test_lz4_frame_logic.py with g++ (no GPU, no HIP header).
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>
#include "ysb_lz4_frame.h"

using namespace ysb;
typedef std::vector<u8> Bytes;

static int fails = 0;
#define CHECK(...) do { if (!(__VA_ARGS__)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #__VA_ARGS__); ++fails; } } while (0)

static std::string golden(const char* name) {
    std::string p = __FILE__;   // .../tests/native/lz4_frame_logic.cpp
    p = p.substr(0, p.rfind('/'));
    return p.substr(0, p.rfind('/')) + "/golden/" + name;
}
static Bytes slurp(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    return Bytes(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}
static void put32(Bytes& b, u32 v) { for (int k = 0; k < 4; ++k) b.push_back((u8)(v >> (8 * k))); }
static void append(Bytes& b, const Bytes& x) { b.insert(b.end(), x.begin(), x.end()); }

// the index on an exact-size heap copy
struct Indexed {
    int rc;
    std::vector<ysb_lz4_frame_block> blocks;
    ysb_lz4_frame_summary info;
    std::string msg;
};
static Indexed index_of(const Bytes& frame, u64 cap = 1000) {
    std::unique_ptr<u8[]> heap(new u8[frame.size() ? frame.size() : 1]);
    if (!frame.empty()) std::memcpy(heap.get(), frame.data(), frame.size());
    Indexed r{};
    r.blocks.resize(cap);
    u64 n = 0;
    Lz4fError err;
    r.rc = lz4f_index(heap.get(), frame.size(), r.blocks.data(), cap, &n, &r.info, &err);
    r.blocks.resize(n < cap ? n : cap);
    r.msg = err.msg;
    if (r.rc == YSB_ERR_CAPACITY) r.info.blocks = n;
    return r;
}

// a frame built by hand: the fields are written here, not by the code under test (the header
// checksum apart, which the liblz4-made fixtures check independently)
struct Opt {
    bool content_size = false, block_sum = false, content_sum = false, dict = false, indep = true;
    u32 version = 1, bid = 4, flg_extra = 0, bd_extra = 0;
    int hc_delta = 0;
};
struct Blk {
    Bytes data;
    bool stored;
};
static Bytes build(const std::vector<Blk>& blocks, const Opt& o = Opt(), u64 content = 0) {
    Bytes f;
    put32(f, LZ4F_MAGIC);
    const size_t d = f.size();
    f.push_back((u8)(o.version << 6 | (o.indep ? 0x20 : 0) | (o.block_sum ? 0x10 : 0) | (o.content_size ? 0x08 : 0) |
                     (o.content_sum ? 0x04 : 0) | (o.dict ? 0x01 : 0) | o.flg_extra));
    f.push_back((u8)(o.bid << 4 | o.bd_extra));
    if (o.content_size) for (int k = 0; k < 8; ++k) f.push_back((u8)(content >> (8 * k)));
    if (o.dict) put32(f, 0x11223344);
    f.push_back((u8)((xxh32(f.data() + d, f.size() - d, 0) >> 8) + o.hc_delta));
    for (const Blk& b : blocks) {
        put32(f, (u32)b.data.size() | (b.stored ? LZ4_STORED : 0));
        append(f, b.data);
        if (o.block_sum) put32(f, 0xDEADBEEF);   // (never verified)
    }
    put32(f, 0);
    if (o.content_sum) put32(f, 0xFEEDFACE);
    return f;
}

static Bytes text(u32 n, u32 seed) {
    Bytes b(n);
    for (u32 i = 0; i < n; ++i) b[i] = (u8)('a' + (i * 7 + seed + i / 13) % 23);
    return b;
}
static Blk packed(const Bytes& raw, bool allow_stored = true) {
    Bytes dst(lz4_compress_bound((u32)raw.size()));
    const ysb_lz4_block e = lz4_pack_block(raw.data(), (u32)raw.size(), dst.data(), allow_stored);
    dst.resize(lz4_entry_comp(e));
    return {dst, (e.comp_bytes & LZ4_STORED) != 0};
}

// every indexed block measured and decoded by the host model, back to back
static bool decode_all(const Bytes& frame, const Indexed& ix, Bytes* out) {
    out->clear();
    for (const ysb_lz4_frame_block& b : ix.blocks) {
        const u32 comp = b.comp_bytes & ~LZ4_STORED;
        if (b.offset + comp > frame.size()) return false;
        std::unique_ptr<u8[]> in(new u8[comp]);
        std::memcpy(in.get(), frame.data() + b.offset, comp);
        const u32 raw = lz4_measure_block(in.get(), b.comp_bytes);
        if (!raw) return false;
        std::unique_ptr<u8[]> dst(new u8[raw]);
        if (!lz4_decode_block(in.get(), ysb_lz4_block{b.comp_bytes, raw}, dst.get())) return false;
        out->insert(out->end(), dst.get(), dst.get() + raw);
    }
    return true;
}

static void test_xxh32() {
    CHECK(xxh32(nullptr, 0, 0) == 0x02CC5D05u);
    const char* s = "Nobody inspects the spammish repetition";   // (39 bytes: the 16-byte lanes, a 4-byte and 1-byte tail)
    CHECK(xxh32(reinterpret_cast<const u8*>(s), std::strlen(s), 0) == 0xE2293B2Fu);
}

static void test_index_valid() {
    const Bytes a = text(3000, 1), b = text(500, 2), c{0x42};
    // with and without each optional field
    for (int m = 0; m < 8; ++m) {
        Opt o;
        o.content_size = m & 1;
        o.block_sum = m & 2;
        o.content_sum = m & 4;
        const Bytes f = build({packed(a), packed(b), packed(c)}, o, 3501);
        const Indexed ix = index_of(f);
        CHECK(ix.rc == YSB_OK && ix.blocks.size() == 3 && ix.info.frames == 1 && ix.info.blocks == 3);
        CHECK(ix.info.content_sizes == (o.content_size ? 1u : 0u) && ix.info.content_bytes == (o.content_size ? 3501u : 0u));
        CHECK(ix.info.block_checksums == (o.block_sum ? 1u : 0u) && ix.info.content_checksums == (o.content_sum ? 1u : 0u));
        CHECK(ix.blocks[0].offset == (u64)(4 + 3 + (o.content_size ? 8 : 0) + 4) && ix.blocks[0].reserved == 0);
        CHECK(ix.info.stored_blocks == 1 && (ix.blocks[2].comp_bytes & LZ4_STORED));   // one byte does not shrink
        Bytes out, want = a;
        append(want, b);
        append(want, c);
        CHECK(decode_all(f, ix, &out) && out == want);
    }
    // an empty frame, an empty buffer, two frames, a skippable frame between them
    {
        const Indexed e = index_of(build({}));
        CHECK(e.rc == YSB_OK && e.blocks.empty() && e.info.frames == 1);
        const Indexed none = index_of(Bytes());
        CHECK(none.rc == YSB_OK && none.info.frames == 0);
        Bytes two = build({packed(a)});
        const size_t first = two.size();
        put32(two, 0x184D2A5Fu);
        put32(two, 5);
        append(two, Bytes{1, 2, 3, 4, 5});
        append(two, build({}));
        Opt o;
        o.content_sum = true;
        append(two, build({packed(b)}, o));
        const Indexed ix = index_of(two);
        CHECK(ix.rc == YSB_OK && ix.info.frames == 3 && ix.info.skippable_frames == 1 && ix.blocks.size() == 2);
        CHECK(ix.blocks.size() == 2 && ix.blocks[1].offset > first + 13);
        Bytes out, want = a;
        append(want, b);
        CHECK(decode_all(two, ix, &out) && out == want);
        // a short cap: the count comes back, the entries that fit are filled
        const Indexed shortcap = index_of(two, 1);
        CHECK(shortcap.rc == YSB_ERR_CAPACITY && shortcap.info.blocks == 2 && shortcap.blocks[0].offset == ix.blocks[0].offset);
    }
    // a full 64 KiB stored block is within the block maximum
    {
        Bytes r(65536);
        u64 x = 99;
        for (u8& v : r) { x = x * 6364136223846793005ull + 1442695040888963407ull; v = (u8)(x >> 56); }
        const Blk s = packed(r);
        CHECK(s.stored && s.data.size() == 65536);
        const Bytes f = build({s});
        const Indexed ix = index_of(f);
        Bytes out;
        CHECK(ix.rc == YSB_OK && decode_all(f, ix, &out) && out == r);
    }
}

static void test_fixtures() {
    const Bytes lines = slurp(golden("gen_s7.jsonl"));
    {
        const Bytes f = slurp(golden("lz4frame/gen_s7_150k.lz4"));
        const Indexed ix = index_of(f);
        CHECK(ix.rc == YSB_OK && ix.blocks.size() == 3 && ix.info.frames == 1);
        Bytes out;
        CHECK(decode_all(f, ix, &out) && out.size() > 2 * 65536 && out.size() <= 150000 && out.back() == '\n');
        CHECK(out.size() <= lines.size() && std::memcmp(out.data(), lines.data(), out.size()) == 0);
        CHECK(out[65535] != '\n' && out[131071] != '\n');   // lines straddle both block edges
    }
    {
        const Bytes f = slurp(golden("lz4frame/small_checksums.lz4"));
        const Indexed ix = index_of(f);
        CHECK(ix.rc == YSB_OK && ix.info.block_checksums == 1 && ix.info.content_checksums == 1 && ix.info.content_sizes == 1);
        Bytes out;
        CHECK(decode_all(f, ix, &out) && out.size() == ix.info.content_bytes && std::memcmp(out.data(), lines.data(), out.size()) == 0);
    }
    {
        const Bytes f = slurp(golden("lz4frame/small_skip_two.lz4"));
        const Indexed ix = index_of(f);
        CHECK(ix.rc == YSB_OK && ix.info.frames == 2 && ix.info.skippable_frames == 1 && ix.blocks.size() == 2);
        Bytes out;
        CHECK(decode_all(f, ix, &out) && out.size() > 2000 && std::memcmp(out.data(), lines.data(), out.size()) == 0);
    }
    const Indexed linked = index_of(slurp(golden("lz4frame/small_linked.lz4")));
    CHECK(linked.rc == YSB_ERR_FORMAT && linked.msg.find("lz4 -BI") != std::string::npos &&
          linked.msg.find("LZ4F_blockIndependent") != std::string::npos && linked.msg.find("block_linked=False") != std::string::npos);
    const Indexed b5 = index_of(slurp(golden("lz4frame/small_b5.lz4")));
    CHECK(b5.rc == YSB_ERR_FORMAT && b5.msg.find("-B4") != std::string::npos && b5.msg.find("byte 5") != std::string::npos);
}

static void refused(const char* what, const Bytes& f, const char* in_msg) {
    const Indexed ix = index_of(f);
    if (ix.rc != YSB_ERR_FORMAT || ix.msg.find(in_msg) == std::string::npos || ix.msg.find("byte ") == std::string::npos) {
        std::printf("FAIL refusal: %s -> rc %d, \"%s\"\n", what, ix.rc, ix.msg.c_str());
        ++fails;
    }
}

static void test_refusals() {
    const std::vector<Blk> one{packed(text(200, 3))};
    Bytes f = build(one);
    f[0] = 0x05;
    refused("another magic", f, "magic");
    f = build(one);
    f[0] = 0x02; f[1] = 0x21; f[2] = 0x4C;
    refused("the legacy magic", f, "legacy");
    Opt o;
    o.version = 2;
    refused("version 10", build(one, o), "version");
    o = Opt();
    o.version = 0;
    refused("version 00", build(one, o), "version");
    o = Opt();
    o.flg_extra = 0x02;
    refused("FLG reserved bit", build(one, o), "reserved");
    o = Opt();
    o.bd_extra = 0x01;
    refused("BD low reserved bits", build(one, o), "reserved");
    o.bd_extra = 0x80;
    refused("BD high reserved bit", build(one, o), "reserved");
    o = Opt();
    o.hc_delta = 1;
    refused("HC mismatch", build(one, o), "header checksum");
    o = Opt();
    o.indep = false;
    refused("linked blocks", build(one, o), "lz4 -BI");
    o = Opt();
    o.dict = true;
    refused("a dictionary id", build(one, o), "dictionar");
    for (u32 bid : {5u, 6u, 7u}) {
        o = Opt();
        o.bid = bid;
        refused("a block maximum above 64 KiB", build(one, o), "-B4");
    }
    o = Opt();
    o.bid = 3;
    refused("an undefined block maximum id", build(one, o), "below 4");
    // a size word above the maximum: compressed and stored
    for (u32 flag : {0u, LZ4_STORED}) {
        f = build({});
        f.resize(f.size() - 4);
        put32(f, 65537 | flag);
        f.resize(f.size() + 65537);
        put32(f, 0);
        refused("a block size word above the maximum", f, "above the frame's block maximum");
    }
    f = build({});
    f.resize(f.size() - 4);
    put32(f, LZ4_STORED);
    put32(f, 0);
    refused("a stored block of no bytes", f, "no bytes");
}

static void test_truncation() {
    Opt o;
    o.content_size = o.block_sum = o.content_sum = true;
    Bytes f;
    put32(f, 0x184D2A50u);   // a skippable frame in front: its header and body are cut too
    put32(f, 3);
    append(f, Bytes{7, 8, 9});
    const size_t skip = f.size();
    append(f, build({packed(text(90, 4)), packed(Bytes{0x31})}, o, 91));
    CHECK(index_of(f).rc == YSB_OK);
    for (size_t cut = 1; cut < f.size(); ++cut) {
        if (cut == skip) continue;   // (the skippable frame alone is a whole buffer)
        const Indexed ix = index_of(Bytes(f.begin(), f.begin() + cut));
        if (ix.rc != YSB_ERR_FORMAT || ix.msg.find("ends") == std::string::npos) {
            std::printf("FAIL truncation at %zu: rc %d \"%s\"\n", cut, ix.rc, ix.msg.c_str());
            ++fails;
        }
    }
    CHECK(index_of(Bytes(f.begin(), f.begin() + skip)).rc == YSB_OK);
}

static void test_writer_and_measure() {
    const Bytes data = slurp(golden("gen_s7.jsonl"));
    CHECK(data.size() > 3 * 65536);
    for (u32 block : {1u, 13u, 64u, 251u, 4096u, 65536u}) {
        const Bytes part(data.begin(), data.begin() + (block == 1 ? 2000 : block < 64 ? 20000 : block < 4096 ? 60000 : 200000));
        Bytes f(lz4f_bound(part.size(), block));
        f.resize(lz4f_pack(part.data(), part.size(), block, 3, f.data()));
        const Indexed ix = index_of(f, 100000);
        CHECK(ix.rc == YSB_OK && ix.info.frames == 1 && ix.info.content_sizes == 1 && ix.info.content_bytes == part.size());
        CHECK(ix.blocks.size() == (part.size() + block - 1) / block && !ix.info.block_checksums && !ix.info.content_checksums);
        Bytes out;
        CHECK(decode_all(f, ix, &out) && out == part);
    }
    Bytes e(lz4f_bound(0, 65536));
    e.resize(lz4f_pack(nullptr, 0, 65536, 1, e.data()));
    const Indexed ie = index_of(e);
    CHECK(ie.rc == YSB_OK && ie.blocks.empty() && ie.info.frames == 1 && ie.info.content_sizes == 1);
    // measure: a compressed block cut at every byte either has no raw size, or decodes with
    // exactly the size measured and with no other
    const Bytes src(data.begin(), data.begin() + 700);
    const Blk b = packed(src, false);
    for (size_t cut = 0; cut <= b.data.size(); ++cut) {
        std::unique_ptr<u8[]> in(new u8[cut ? cut : 1]);
        std::memcpy(in.get(), b.data.data(), cut);
        const u32 raw = lz4_measure_block(in.get(), (u32)cut);
        CHECK(raw <= 700 && (cut < b.data.size() || raw == 700));
        for (u32 r : {raw, raw + 1, raw ? raw - 1 : 700u, 700u}) {
            if (!r) continue;
            std::unique_ptr<u8[]> out(new u8[r]);
            const bool ok = lz4_decode_block(in.get(), ysb_lz4_block{(u32)cut, r}, out.get());
            CHECK(ok == (r == raw));
        }
    }
    // a block that decodes to more than 65536 bytes has no raw size: 65536 literals and a match
    Bytes big{0xF0};
    big.insert(big.end(), (65536 - 15) / 255, 255);
    big.push_back((65536 - 15) % 255);
    big.resize(big.size() + 65536, 0x55);
    CHECK(lz4_measure_block(big.data(), (u32)big.size()) == 65536);
    append(big, Bytes{1, 0, 0x00});
    CHECK(lz4_measure_block(big.data(), (u32)big.size()) == 0);
    const Bytes zero{0x00};   // an empty last sequence alone: raw size 0
    CHECK(lz4_measure_block(zero.data(), 1) == 0);
    CHECK(lz4_measure_block(zero.data(), 1 | LZ4_STORED) == 1);
}

// ---- the carry rule over whole streams --------------------------------------------------------

// the lines of a buffer by the split's rule: '\n', '\r' and "\r\n" end a line; an unterminated
// tail is a line
static std::vector<std::string> lines_of(const Bytes& b) {
    std::vector<std::string> out;
    size_t at = 0;
    for (size_t i = 0; i < b.size(); ++i) {
        if (b[i] != '\n' && b[i] != '\r') continue;
        out.emplace_back(b.begin() + at, b.begin() + i);
        if (b[i] == '\r' && i + 1 < b.size() && b[i + 1] == '\n') ++i;
        at = i + 1;
    }
    if (at < b.size()) out.emplace_back(b.begin() + at, b.end());
    return out;
}

static void carry_stream(const Bytes& stream, u32 block) {
    Bytes f(lz4f_bound(stream.size(), block));
    f.resize(lz4f_pack(stream.data(), stream.size(), block, 2, f.data()));
    const Indexed ix = index_of(f, 100000);
    CHECK(ix.rc == YSB_OK && ix.blocks.size() == (stream.size() + block - 1) / block);
    std::vector<std::string> got;
    Bytes buf;   // the carry, then the batch's bytes behind it
    size_t max_carry = 0, cr_carried = 0;
    for (size_t i = 0; i < ix.blocks.size(); ++i) {
        Indexed one{};
        one.blocks.assign(1, ix.blocks[i]);
        Bytes dec;
        CHECK(decode_all(f, one, &dec));
        append(buf, dec);
        std::unique_ptr<u8[]> heap(new u8[buf.size()]);
        std::memcpy(heap.get(), buf.data(), buf.size());
        const bool more = i + 1 < ix.blocks.size();
        const u64 cut = lz4f_carry_cut(heap.get(), buf.size(), more);
        CHECK(cut <= buf.size());
        if (more && buf.back() == '\r') { CHECK(cut < buf.size()); ++cr_carried; }
        for (std::string& l : lines_of(Bytes(buf.begin(), buf.begin() + cut))) got.push_back(std::move(l));
        buf.erase(buf.begin(), buf.begin() + cut);
        max_carry = std::max(max_carry, buf.size());
    }
    CHECK(buf.empty());
    const std::vector<std::string> want = lines_of(stream);
    if (got != want) {
        std::printf("FAIL carry: %zu lines out, %zu in (block %u)\n", got.size(), want.size(), block);
        ++fails;
    }
    CHECK(max_carry > 3 * (size_t)block);   // a line longer than three blocks was carried
    CHECK(cr_carried >= 1);                 // a batch ended in '\r'
}

static void test_carry() {
    const char* d0 = "ab\ncd\r";
    const u8* d = reinterpret_cast<const u8*>(d0);
    CHECK(lz4f_carry_cut(d, 6, true) == 3 && lz4f_carry_cut(d, 6, false) == 6 && lz4f_carry_cut(d, 5, true) == 3);
    CHECK(lz4f_carry_cut(reinterpret_cast<const u8*>("ab\rcd"), 5, true) == 3);
    CHECK(lz4f_carry_cut(reinterpret_cast<const u8*>("ab\r\ncd"), 6, true) == 4);
    CHECK(lz4f_carry_cut(reinterpret_cast<const u8*>("abc"), 3, true) == 0 && lz4f_carry_cut(d, 0, true) == 0);
    CHECK(lz4f_carry_cut(reinterpret_cast<const u8*>("\r"), 1, true) == 0);
    // 40 golden lines, their terminators '\n', "\r\n" and '\r' in turn, one line made longer
    // than three of the largest blocks, the stream ending in a lone '\r'
    const Bytes data = slurp(golden("gen_s7.jsonl"));
    std::vector<std::string> src = lines_of(Bytes(data.begin(), data.begin() + 12000));
    CHECK(src.size() >= 41);
    for (u32 block : {13u, 64u, 251u}) {
        Bytes stream;
        size_t crlf_at = 0;
        for (int k = 0; k < 40; ++k) {
            std::string l = src[k];
            if (k == 7) l = l + src[8] + src[9] + src[10];   // ~950 bytes, no terminator inside
            if (k == 3) {
                // pad this line so that its "\r\n" straddles two blocks: the '\r' a block's last byte
                const size_t end = stream.size() + l.size();
                l.append((block - 1 - end % block) % block, ' ');
            }
            stream.insert(stream.end(), l.begin(), l.end());
            if (k % 3 == 0 || k == 39) {
                if (k == 3) crlf_at = stream.size();
                stream.push_back('\r');
                if (k != 39) stream.push_back('\n');
            } else if (k % 3 == 1) {
                stream.push_back('\n');
            } else {
                stream.push_back('\r');
            }
        }
        CHECK(crlf_at % block == block - 1 && stream[crlf_at] == '\r' && stream[crlf_at + 1] == '\n' && stream.back() == '\r');
        CHECK(lines_of(stream).size() == 40);
        carry_stream(stream, block);
    }
}

int main() {
    test_xxh32();
    test_index_valid();
    test_fixtures();
    test_refusals();
    test_truncation();
    test_writer_and_measure();
    test_carry();
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("lz4 frame logic OK\n");
    return 0;
}
