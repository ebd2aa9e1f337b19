// Host-side checks of the layout sampling's rules (ysb_layout.h): which scan instantiation a
// line, a sample of lines and two successive samples name.  Counts never depend on these
// choices, so only this test sees a wrong rule as anything but speed.
// Built and run by tests/test_capi.py with g++ (no GPU, no library).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "ysb_layout.h"

using namespace ysb;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static const char* KEYS[7] = {"user_id", "page_id", "ad_id", "ad_type", "event_type", "event_time", "ip_address"};
static const char* VALS[7] = {"0f8c1e7a-1111-4222-8333-944455556666", "1f8c1e7a-1111-4222-8333-944455556666",
                              "2f8c1e7a-1111-4222-8333-944455556666", "banner", "view", "1700000000000", "1.2.3.4"};
static const u32 REORDER[7] = {3, 5, 2, 6, 0, 4, 1};   // GEN_V_REORDER's key order

// A flat object of the keys in `order`, compact or with the generator's spaces.
static std::string make_line(const std::vector<u32>& order, bool compact) {
    std::string s = "{";
    for (size_t k = 0; k < order.size(); ++k) {
        if (k) s += compact ? "," : ", ";
        s += std::string("\"") + KEYS[order[k]] + (compact ? "\":\"" : "\": \"") + VALS[order[k]] + "\"";
    }
    return s + "}\n";
}

// Event i as the generator writes it in layout `variant`.
static std::string gen_line(u32 variant, u64 i) {
    GenSpec s{};
    s.seed = s.ev_seed = 5; s.n_campaigns = 100; s.ads_per_campaign = 10; s.t0_ms = 1700000000000LL;
    s.events_per_sec = 1000; s.n_pick = 1000; s.variant = variant;
    char buf[400];
    const u32 n = gen_line_write(s, i, gen_event(s, i), buf);
    return std::string(buf, n);
}

static int learn(const std::string& l, u32 req, LearnDesc* d) {
    return learn_layout(reinterpret_cast<const u8*>(l.data()), l.size(), req, d);
}
static int learn(const std::string& l, u32 req = 0x3F) {
    LearnDesc d{};
    return learn(l, req, &d);
}
static bool is_order(const LearnDesc& d, const std::vector<u32>& order, u32 cp) {
    bool ok = d.n == order.size() && d.cp == cp;
    for (size_t k = 0; k < order.size() && ok; ++k) ok = d.order[k] == order[k];
    return ok;
}
static bool is_zero(const LearnDesc& d) {
    const LearnDesc z{};
    return std::memcmp(&d, &z, sizeof z) == 0;
}

static int decide(const std::vector<std::string>& ls, LearnDesc* d, u32 req = 0x3F) {
    std::vector<std::pair<const u8*, u64>> v;
    for (const auto& l : ls) v.push_back({reinterpret_cast<const u8*>(l.data()), l.size()});
    return decide_layout(req, v, d);
}

static void test_learn_layout() {
    const std::vector<u32> re(REORDER, REORDER + 7);
    for (u64 i = 0; i < 50; ++i) {
        CHECK(learn(gen_line(0, i)) == 0);
        CHECK(learn(gen_line(0, i), 0x7F) == 0);
        CHECK(learn(gen_line(GEN_V_COMPACT, i)) == 1);
        for (u32 cp = 0; cp < 2; ++cp) {
            LearnDesc d{};
            CHECK(learn(gen_line(GEN_V_REORDER | (cp ? (u32)GEN_V_COMPACT : 0u), i), 0x3F, &d) == 3);
            CHECK(is_order(d, re, cp));
        }
    }
    CHECK(learn(make_line({0, 1, 2, 3, 4, 5, 6}, false)) == 0);
    CHECK(learn(make_line({0, 1, 2, 3, 4, 5, 6}, true)) == 1);
    // a subset: the generator's order without ip_address is a learned order, unless required
    LearnDesc d{};
    CHECK(learn(make_line({0, 1, 2, 3, 4, 5}, false), 0x3F, &d) == 3);
    CHECK(is_order(d, {0, 1, 2, 3, 4, 5}, 0));
    CHECK(learn(make_line({0, 1, 2, 3, 4, 5}, false), 0x7F) == 2);
    CHECK(learn(make_line({5, 4, 2}, true), 0, &d) == 3 && is_order(d, {5, 4, 2}, 1));
    // ad_id, event_type and event_time are needed whatever the mask
    CHECK(learn(make_line({0, 1, 3, 4, 5, 6}, false), 0) == 2);
    CHECK(learn(make_line({0, 1, 2, 3, 5, 6}, false), 0) == 2);
    CHECK(learn(make_line({0, 1, 2, 3, 4, 6}, false), 0) == 2);
    // mixed spacing within a line: after a key, after a value
    std::string l = make_line(re, false);
    l.erase(l.find(": \"", 20) + 1, 1);
    CHECK(learn(l) == 2);
    l = make_line(re, true);
    l.insert(l.find("\",\"", 20) + 2, " ");
    CHECK(learn(l) == 2);
    // an id value of 35 bytes
    l = make_line(re, false);
    l.erase(l.find(VALS[2]), 1);
    CHECK(learn(l) == 2);
    // a repeated key, a backslash in a value, an unknown key, more than the closing brace missing
    CHECK(learn(make_line({3, 5, 2, 6, 0, 4, 1, 3}, false)) == 2);
    CHECK(learn(make_line({3, 5, 2, 3, 0, 4, 1}, false)) == 2);
    l = make_line(re, false);
    l.replace(l.find("banner"), 6, "ban\\ner");
    CHECK(learn(l) == 2);
    l = make_line(re, false);
    l.replace(l.find("ad_type"), 7, "ad_kind");
    CHECK(learn(l) == 2);
    l = make_line(re, false);
    CHECK(learn(l.substr(0, l.size() - 3)) == 2);
    // shorter than 2 bytes; not an object
    CHECK(learn("") == 2);
    CHECK(learn("{") == 2);
    CHECK(learn_layout(nullptr, 0, 0x3F, &d) == 2);
    CHECK(learn("[" + make_line(re, false)) == 2);
}

static void test_sample_index() {
    for (u64 n : {0ull, 1ull, 63ull, 64ull})
        for (u32 j = 0; j < SAMPLE_LINES; ++j) CHECK(sample_index(n, j) == (n ? std::min<u64>(j, n - 1) : 0));
    for (u64 n : {65ull, 1000ull, (1ull << 31) - 1}) {
        for (u32 j = 0; j < SAMPLE_LINES; ++j) {
            const u64 q = j >> 1, i = sample_index(n, j);
            CHECK(i < n);
            CHECK(i >= n * q / 32 && i < n * (q + 1) / 32);
            if (j & 1) CHECK(i == sample_index(n, j - 1) + 1);
            if (j) CHECK(i > sample_index(n, j - 1));
        }
        CHECK(sample_index(n, 0) == 0);
    }
}

static void test_decide_layout() {
    static_assert(SAMPLE_LINES == 64 && SAMPLE_AGREE == 46, "the cases below are written for 46 of 64");
    const std::vector<u32> re(REORDER, REORDER + 7), other{2, 5, 4, 0, 1, 3, 6};
    const std::string G = gen_line(0, 1), C = gen_line(GEN_V_COMPACT, 2), A = make_line(re, false),
                      B = make_line(other, false);
    LearnDesc d{};
    CHECK(decide({}, &d) == 0);
    CHECK(decide(std::vector<std::string>(64, G), &d) == 0);
    // 46 of 64 keep the majority's instantiation, wherever the others are
    std::vector<std::string> v(46, G);
    v.insert(v.end(), 18, C);
    CHECK(decide(v, &d) == 0);
    v.assign(18, C);
    v.insert(v.end(), 46, G);
    CHECK(decide(v, &d) == 0);
    v.assign(64, A);
    d = LearnDesc{};
    CHECK(decide(v, &d) == 3 && is_order(d, re, 0));
    // 45 + 19 in runs of two (one pair mixed): no majority, 31 of 32 pairs alike: the dispatch
    v.clear();
    for (int p = 0; p < 22; ++p) { v.push_back(G); v.push_back(G); }
    for (int p = 0; p < 9; ++p) { v.push_back(C); v.push_back(C); }
    v.push_back(G);
    v.push_back(C);
    d = LearnDesc{{1, 2, 3}, 3, 1};   // (to be cleared: the sample names no learned order)
    CHECK(v.size() == 64 && decide(v, &d) == 4 && is_zero(d));
    // 3 of 4 pairs alike is the bound: 24 of 32 pairs the dispatch, 23 the flat tier
    for (int alike : {24, 23}) {
        v.clear();
        for (int p = 0; p < 32; ++p) {
            v.push_back(p & 1 ? G : C);
            v.push_back(p < alike ? v.back() : (p & 1 ? C : G));
        }
        CHECK(decide(v, &d) == (alike == 24 ? 4 : 2));
    }
    // two layouts alternating line by line: every tile would be mixed, the flat tier
    v.clear();
    for (int p = 0; p < 32; ++p) { v.push_back(G); v.push_back(C); }
    CHECK(decide(v, &d) == 2);
    // runs of three producers, two of them with learned orders: the dispatch with the more
    // frequent order (which comes later in the sample)
    v.assign(30, G);
    v.insert(v.end(), 14, B);
    v.insert(v.end(), 20, A);
    d = LearnDesc{};
    CHECK(decide(v, &d) == 4 && is_order(d, re, 0));
    // fewer lines than SAMPLE_AGREE: all of them must agree
    CHECK(decide({C, C, C}, &d) == 1);
    CHECK(decide({A, A, A}, &d) == 3 && is_order(d, re, 0));
    CHECK(decide({G}, &d) == 0);
    // the require mask reaches every line
    CHECK(decide(std::vector<std::string>(64, make_line({0, 1, 2, 3, 4, 5}, false)), &d, 0x3F) == 3);
    CHECK(decide(std::vector<std::string>(64, make_line({0, 1, 2, 3, 4, 5}, false)), &d, 0x7F) == 2);
}

static void test_sniff() {
    const std::vector<u32> re(REORDER, REORDER + 7);
    LearnDesc d{};
    auto raw = [&](const std::string& b, u32 req = 0x3F) {
        return sniff_raw(req, reinterpret_cast<const u8*>(b.data()), b.size(), &d);
    };
    std::string buf, crlf;
    std::vector<u32> off;
    for (u64 i = 0; i < 3000; ++i) {
        off.push_back((u32)buf.size());
        buf += gen_line(0, i);
        crlf += gen_line(0, i);
        crlf.insert(crlf.size() - 1, "\r");
    }
    CHECK(raw(buf) == 0);
    CHECK(raw(crlf) == 0);
    CHECK(raw("") == 2);   // (an empty batch is never sampled: its one "line" has no bytes)
    // no terminator at all: the buffer is its single line
    std::string one = make_line(re, true);
    one.pop_back();
    CHECK(raw(one) == 3 && is_order(d, re, 1));
    // a lone '\r' ends the first line but does not start a sampled pair: what follows it is
    // not a line of the sample
    std::string cr = gen_line(GEN_V_COMPACT, 7);
    cr.back() = '\r';
    CHECK(raw(cr + "not a line at all") == 1);
    for (int i = 0; i < 100; ++i) cr += make_line(re, false).replace(make_line(re, false).size() - 1, 1, "\r");
    CHECK(raw(cr) == 1);
    // a host batch with offsets: the same decision, and bad offsets name nothing (0)
    auto host = [&](const std::string& b, const std::vector<u32>& o) {
        return sniff_layout(0x3F, reinterpret_cast<const u8*>(b.data()), b.size(), o.data(), o.size(), &d);
    };
    CHECK(host(buf, off) == 0);
    std::string rbuf;
    std::vector<u32> roff;
    for (u64 i = 0; i < 3000; ++i) {
        roff.push_back((u32)rbuf.size());
        rbuf += gen_line(i % 512 < 256 ? 0u : (u32)GEN_V_REORDER, i);
    }
    CHECK(host(rbuf, roff) == 4 && is_order(d, re, 0));   // two producers in runs of 256 lines
    CHECK(raw(rbuf) == 4 && is_order(d, re, 0));
    std::vector<u32> bad = off;
    bad[1] = bad[0];
    CHECK(host(buf, bad) == 0);
    bad = off;
    bad.back() = (u32)buf.size() + 1;
    CHECK(host(buf, bad) == 0);
    // the flags' hint: flat-first keeps the flat tier unless the sample names a key order
    for (int lay : {-1, 0, 1, 2, 3, 4}) {
        CHECK(hinted_layout(false, lay) == lay);
        CHECK(hinted_layout(true, lay) == (lay == 0 || lay == 1 ? 2 : lay));
    }
}

static void test_settled_layout() {
    LearnDesc a{{3, 5, 2, 6, 0, 4, 1}, 7, 0}, b = a, none{}, d{};
    b.cp = 1;
    // no older decision: the previous one
    CHECK(settled_layout(-1, none, 1, none, &d) == 1 && is_zero(d));
    CHECK(settled_layout(-1, none, 3, a, &d) == 3 && std::memcmp(&d, &a, sizeof a) == 0);
    CHECK(settled_layout(-1, b, 4, a, &d) == 4 && std::memcmp(&d, &a, sizeof a) == 0);
    // equal: that one
    CHECK(settled_layout(0, none, 0, none, &d) == 0 && is_zero(d));
    CHECK(settled_layout(3, a, 3, a, &d) == 3 && std::memcmp(&d, &a, sizeof a) == 0);
    CHECK(settled_layout(2, none, 2, none, &d) == 2);
    // (only layout 3 compares the order: two dispatch decisions agree whatever their orders)
    CHECK(settled_layout(4, a, 4, b, &d) == 4 && std::memcmp(&d, &b, sizeof b) == 0);
    // otherwise the dispatch, with the newer sample's learned order if it has one
    d = a;
    CHECK(settled_layout(0, none, 1, none, &d) == 4 && is_zero(d));
    CHECK(settled_layout(3, a, 0, none, &d) == 4 && is_zero(d));
    CHECK(settled_layout(0, none, 3, a, &d) == 4 && std::memcmp(&d, &a, sizeof a) == 0);
    CHECK(settled_layout(1, none, 4, b, &d) == 4 && std::memcmp(&d, &b, sizeof b) == 0);
    // two decisions of layout 3 whose orders (here: spacing) differ disagree
    CHECK(settled_layout(3, a, 3, b, &d) == 4 && std::memcmp(&d, &b, sizeof b) == 0);
    CHECK(!same_decision(3, a, 3, b) && same_decision(3, b, 3, b) && !same_decision(0, none, 1, none));
}

int main() {
    test_learn_layout();
    test_sample_index();
    test_decide_layout();
    test_sniff();
    test_settled_layout();
    std::printf("%s\n", fails ? "FAILED" : "OK");
    return fails ? 1 : 0;
}
