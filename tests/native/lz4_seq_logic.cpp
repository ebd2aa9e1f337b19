// The generated sequence corpus (tests/lz4_seqgen.py) through the host side of csrc/ysb_lz4.h and
// csrc/ysb_lz4_frame.h: the sequence reader the kernels share, the host decoder with the
// one-wave kernel's in-place checks, and the measure walk.  argv[1] is the corpus file that
// tests/test_lz4_seq_logic.py writes: u32 count, then per block u32 comp_len, raw, valid, the
// compressed bytes and (valid blocks only) the bytes they decode to.  Every input and output
// lives in a heap buffer of its exact size, so the same program built with
// -fsanitize=address,undefined shows any read or write one byte out of range -- the gate for
// sending the corpus, its malformed blocks included, to a GPU.
// Built and run by tests/test_lz4_seq_logic.py with g++ (no GPU, no HIP header).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <vector>
#include "ysb_lz4_frame.h"

using namespace ysb;

static int fails = 0;
#define CHECK(i, ...) do { if (!(__VA_ARGS__)) { std::printf("FAIL block %u: %s\n", (unsigned)(i), #__VA_ARGS__); ++fails; } } while (0)

int main(int argc, char** argv) {
    if (argc != 2) { std::printf("usage: lz4_seq_logic CORPUS\n"); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    const std::vector<u8> file((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    size_t at = 0;
    auto word = [&]() -> u32 {
        if (file.size() - at < 4) { std::printf("FAIL: the corpus file ends early\n"); std::exit(1); }
        u32 v;
        std::memcpy(&v, file.data() + at, 4);
        at += 4;
        return v;
    };
    const u32 count = word();
    u32 n_valid = 0, n_bad = 0, n_measured = 0;
    for (u32 i = 0; i < count; ++i) {
        const u32 comp = word(), raw = word(), valid = word();
        const size_t need = (size_t)comp + (valid ? raw : 0);
        if (file.size() - at < need) { std::printf("FAIL: the corpus file ends inside block %u\n", i); return 1; }
        const u8* cbytes = file.data() + at;
        const u8* want = cbytes + comp;
        at += need;
        // exact-size heap copies: the decoder's input and output, the measure walk's input
        std::unique_ptr<u8[]> in(new u8[comp ? comp : 1]), in2(new u8[comp ? comp : 1]), out(new u8[raw ? raw : 1]);
        std::memcpy(in.get(), cbytes, comp);
        std::memcpy(in2.get(), cbytes, comp);
        const ysb_lz4_block e{comp, raw};
        bool in_place = true;
        const bool ok = lz4_decode_block(in.get(), e, out.get(), &in_place);
        CHECK(i, ok == (valid != 0));
        const u32 measured = lz4_measure_block(in2.get(), comp);
        CHECK(i, measured <= LZ4_MAX_RAW);
        n_measured += measured != 0;
        if (valid) {
            ++n_valid;
            CHECK(i, ok && std::memcmp(out.get(), want, raw) == 0);
            CHECK(i, in_place);          // the one-wave kernel's in-place checks never fire for a valid block
            CHECK(i, measured == raw);
        } else {
            ++n_bad;
            // the one size that could make the block valid is not the corpus's
            CHECK(i, measured != raw);
        }
    }
    if (at != file.size()) { std::printf("FAIL: %zu bytes behind the last block\n", file.size() - at); ++fails; }
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("%u valid and %u invalid blocks, %u measured: lz4 seq logic OK\n", n_valid, n_bad, n_measured);
    return 0;
}
