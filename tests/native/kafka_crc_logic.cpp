// Host-side checks of the CRC-32C arithmetic the GPU verifies Kafka record batches with
// (csrc/ysb_kafka_crc.h): mulmod and the powers of x against the bitwise definition, the
// combine identity, the sliced host kafka_crc32c against the byte loop it replaced (kept here),
// and kafka_crc_lanes_host -- the kernel's 64-lane decomposition as a plain loop -- over every
// range length 0..2200 at every start residue mod 16.  Every range lives in a heap buffer that is
// exactly the 16-byte vectors the decomposition may read, so the same program built with
// -fsanitize=address,undefined (tests/test_kafka_crc_logic.py) shows any read outside them.
// Built and run by tests/test_kafka_crc_logic.py with g++ (no GPU, no HIP header).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "ysb_kafka.h"

using namespace ysb;

static int fails = 0;
#define CHECK(...) do { if (!(__VA_ARGS__)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #__VA_ARGS__); ++fails; } } while (0)

// ---- the definitions, written apart from the header -------------------------------------------
// the register bit by bit (no table)
static u32 bit_reg(const u8* p, u64 n, u32 reg = 0) {
    for (u64 i = 0; i < n; ++i) {
        reg ^= p[i];
        for (int k = 0; k < 8; ++k) reg = (reg >> 1) ^ ((reg & 1) ? 0x82F63B78u : 0u);
    }
    return reg;
}
static u32 bit_crc(const u8* p, u64 n) { return ~bit_reg(p, n, 0xFFFFFFFFu); }
// the byte-at-a-time table loop that csrc/ysb_kafka.h had
static u32 old_crc32c(const u8* p, u64 n, u32 crc = 0) {
    static u32 t[256];
    if (!t[1])
        for (u32 i = 0; i < 256; ++i) {
            u32 c = i;
            for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1) ? 0x82F63B78u : 0u);
            t[i] = c;
        }
    crc = ~crc;
    for (u64 i = 0; i < n; ++i) crc = t[(crc ^ p[i]) & 255] ^ (crc >> 8);
    return ~crc;
}
// a * b mod P with the polynomials unreflected: a carry-less 64-bit product, then long division
static u32 rev32(u32 v) {
    u32 r = 0;
    for (int i = 0; i < 32; ++i) r |= ((v >> i) & 1u) << (31 - i);
    return r;
}
static u32 slow_mulmod(u32 a, u32 b) {
    const u64 A = rev32(a), B = rev32(b), P = 0x11EDC6F41ull;
    u64 prod = 0;
    for (int i = 0; i < 32; ++i)
        if ((A >> i) & 1) prod ^= B << i;
    for (int i = 62; i >= 32; --i)
        if ((prod >> i) & 1) prod ^= P << (i - 32);
    return rev32((u32)prod);
}

static u32 rng_state = 0x9E3779B9u;
static u32 rng() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 17;
    rng_state ^= rng_state << 5;
    return rng_state;
}

// p[0, n) at residue r mod 16 inside a heap block that is exactly the vectors holding [p - pre, p + n)
struct Placed {
    u8* block = nullptr;
    u8* p = nullptr;
    Placed(u32 r, u32 pre, const u8* src, u32 n) {
        const u64 bytes = ((u64)r + pre + n + 15) & ~15ull;
        void* m = nullptr;
        if (posix_memalign(&m, 16, bytes ? bytes : 1)) std::abort();
        block = static_cast<u8*>(m);
        for (u64 i = 0; i < bytes; ++i) block[i] = (u8)rng();   // what lies around the range is never trusted
        p = block + r + pre;
        if (n) std::memcpy(p, src, n);
    }
    ~Placed() { std::free(block); }
};

static void vectors() {
    CHECK(kafka_crc32c(nullptr, 0) == 0);
    const char* d = "123456789";
    CHECK(kafka_crc32c(reinterpret_cast<const u8*>(d), 9) == 0xE3069283u);
    u8 b[48];
    std::memset(b, 0, 32);
    CHECK(kafka_crc32c(b, 32) == 0x8A9136AAu);                         // RFC 3720 B.4
    std::memset(b, 0xFF, 32);
    CHECK(kafka_crc32c(b, 32) == 0x62A8AB43u);
    for (int i = 0; i < 32; ++i) b[i] = (u8)i;
    CHECK(kafka_crc32c(b, 32) == 0x46DD794Eu);
    for (int i = 0; i < 32; ++i) b[i] = (u8)(31 - i);
    CHECK(kafka_crc32c(b, 32) == 0x113FDB5Cu);
    const u8 pdu[48] = {0x01, 0xc0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0x14, 0, 0, 0, 0, 0, 0x04, 0,
                        0, 0, 0, 0x14, 0, 0, 0, 0x18, 0x28, 0, 0, 0, 0, 0, 0, 0, 0x02, 0, 0, 0, 0, 0, 0, 0};
    CHECK(kafka_crc32c(pdu, 48) == 0xD9963A56u);                        // the iSCSI SCSI Read (10) PDU
    // the same vectors through the lanes, at every residue
    for (u32 r = 0; r < 16; ++r) {
        Placed z(r, 0, b, 0), s(r, 0, reinterpret_cast<const u8*>(d), 9), q(r, 4, pdu, 48);
        CHECK(kafka_crc_lanes_host(z.p, 0, 0) == 0);
        CHECK(kafka_crc_lanes_host(s.p, 0, 9) == 0xE3069283u);
        CHECK(kafka_crc_lanes_host(q.p, 4, 48) == 0xD9963A56u);
    }
}

static void arithmetic() {
    CHECK(crc_mulmod(CRC_ONE, 0x12345678u) == 0x12345678u && crc_mulx(CRC_ONE) == 0x40000000u);
    for (int i = 0; i < 2000; ++i) {
        const u32 a = rng(), b = rng();
        CHECK(crc_mulmod(a, b) == slow_mulmod(a, b));
        CHECK(crc_divx(crc_mulx(a)) == a && crc_mulx(crc_divx(a)) == a);
    }
    // x^(8n): the register CRC_ONE after n zero bytes; and its inverse
    u32 reg = CRC_ONE;
    const u8 zero = 0;
    for (u32 n = 0; n < 3000; ++n) {
        CHECK(crc_xpow8(n) == reg);
        CHECK(crc_mulmod(crc_xpow8(n), crc_xpow8_inv(n)) == CRC_ONE);
        reg = bit_reg(&zero, 1, reg);
    }
    for (u64 n : {65536ull, 1048579ull, 0x7FFFFFFFull, 0xFFFFFFFFFull})
        CHECK(crc_mulmod(crc_xpow8(n), crc_xpow8_inv(n)) == CRC_ONE && crc_mulmod(crc_xpow8(n), crc_xpow8(5)) == crc_xpow8(n + 5));
    // the four bytes that leave the init value behind them
    u8 k[4] = {(u8)CRC_INIT_BYTES, (u8)(CRC_INIT_BYTES >> 8), (u8)(CRC_INIT_BYTES >> 16), (u8)(CRC_INIT_BYTES >> 24)};
    CHECK(bit_reg(k, 4) == 0xFFFFFFFFu);
    // reg(A || B) for every split of 300 bytes
    std::vector<u8> buf(300);
    for (u8& v : buf) v = (u8)rng();
    const u32 whole = bit_reg(buf.data(), 300);
    for (u32 cut = 0; cut <= 300; ++cut)
        CHECK(crc_combine(bit_reg(buf.data(), cut), bit_reg(buf.data() + cut, 300 - cut), 300 - cut) == whole);
    // the tables: entry v of table j is the register of v and dist - 1 - j zero bytes
    std::vector<u32> t(CRC_TABLE_WORDS);
    for (u32 dist : {16u, CRC_WIN}) {
        crc_fill_tables(t.data(), dist);
        std::vector<u8> m(dist, 0);
        for (u32 j = 0; j < 16; ++j)
            for (u32 v : {1u, 0x80u, 0xA5u, 0xFFu}) {
                m[0] = (u8)v;
                CHECK(t[j * 256 + v] == bit_reg(m.data(), dist - j));
            }
    }
}

static void sliced_host() {
    std::vector<u8> buf(5000);
    for (u8& v : buf) v = (u8)rng();
    for (u32 n = 0; n <= 700; ++n)
        for (u32 at : {0u, 1u, 7u}) CHECK(kafka_crc32c(buf.data() + at, n) == old_crc32c(buf.data() + at, n));
    CHECK(kafka_crc32c(buf.data(), 5000) == old_crc32c(buf.data(), 5000) && old_crc32c(buf.data(), 5000) == bit_crc(buf.data(), 5000));
    // continued: the second half from the first half's value
    CHECK(kafka_crc32c(buf.data() + 1234, 3766, kafka_crc32c(buf.data(), 1234)) == old_crc32c(buf.data(), 5000));
}

static void lanes() {
    std::vector<u8> src((1u << 20) + 3);
    for (u8& v : src) v = (u8)rng();
    for (u32 n = 0; n <= 2200; ++n) {
        const u32 want = kafka_crc32c(src.data(), n);
        for (u32 r = 0; r < 16; ++r) {
            Placed a(r, 0, src.data(), n);
            CHECK(kafka_crc_lanes_host(a.p, 0, n) == want);
        }
    }
    // as a record batch has it: the stored CRC's four bytes in front
    for (u32 n : {40u, 41u, 975u, 976u, 977u, 1999u, 2000u, 2001u})
        for (u32 r = 0; r < 16; ++r) {
            Placed a(r, 4, src.data(), n);
            CHECK(kafka_crc_lanes_host(a.p, 4, n) == kafka_crc32c(src.data(), n));
        }
    for (u32 n : {65535u, 65536u, 65537u, (1u << 20) + 3})
        for (u32 r : {0u, 1u, 15u}) {
            Placed a(r, 0, src.data(), n), b(r, 4, src.data(), n);
            const u32 want = kafka_crc32c(src.data(), n);
            CHECK(want == old_crc32c(src.data(), n));
            CHECK(kafka_crc_lanes_host(a.p, 0, n) == want && kafka_crc_lanes_host(b.p, 4, n) == want);
        }
}

int main() {
    vectors();
    arithmetic();
    sliced_host();
    lanes();
    std::printf(fails ? "FAILED %d\n" : "OK\n", fails);
    return fails ? 1 : 0;
}
