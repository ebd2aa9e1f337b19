// ysb_layout.h -- the layout sampling's rules: which scan instantiation a batch's sampled
// lines name.  Plain host logic over ysb_common.h and the standard library (no HIP, no
// context), so tests/native/layout_logic.cpp checks it without a GPU; ysb_submit.cpp holds
// the sample buffers, the sample kernel's launch and the waits around it.  Only a choice of
// instantiation: every instantiation counts every line exactly.
#pragma once
#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

#include "ysb_common.h"

namespace ysb {

// A key order read off a batch's first line (layout 3, learn_layout).
struct LearnDesc {
    u32 order[8];
    u32 n;
    u32 cp;
};

// The JSON layout of a batch's first line l[0, len): 0 the generator's (core.clj:90-96), 1
// the generator's keys in its order as compact JSON, 3 another key order or subset of
// DeserializeBolt's keys with one consistent spacing (", " / ": " or "," / ":") and plain
// string values (36 bytes for the three ids) -- d then holds the order for the scan's
// learned-order instantiation -- and 2 anything else (the flat-object tier first).  Only a
// choice of instantiation: every instantiation counts every line exactly.
inline int learn_layout(const u8* l, u64 len, u32 require_mask, LearnDesc* d) {
    static const char* keys[7] = {"user_id", "page_id", "ad_id", "ad_type", "event_type", "event_time", "ip_address"};
    if (len < 2 || l[0] != '{' || l[1] != '"') return 2;
    auto plain_end = [&](u64 q) {   // the closing quote of a plain string from q (len: none)
        while (q < len && l[q] != '"' && l[q] != '\\' && l[q] >= 0x20) ++q;
        return (q < len && l[q] == '"') ? q : len;
    };
    u64 p = 2;
    int cp = -1;
    u32 seen = 0, n = 0, order[8] = {0};
    for (;;) {
        u64 q = plain_end(p);
        if (q >= len) return 2;
        int id = -1;
        for (int i = 0; i < 7; ++i)
            if (std::strlen(keys[i]) == q - p && std::memcmp(l + p, keys[i], q - p) == 0) id = i;
        if (id < 0 || ((seen >> id) & 1u) || n >= 7) return 2;
        seen |= 1u << id;
        order[n++] = (u32)id;
        p = q + 1;
        int c1;
        if (p + 2 < len && l[p] == ':' && l[p + 1] == ' ' && l[p + 2] == '"') { c1 = 0; p += 3; }
        else if (p + 1 < len && l[p] == ':' && l[p + 1] == '"') { c1 = 1; p += 2; }
        else return 2;
        if (cp < 0) cp = c1;
        else if (cp != c1) return 2;
        q = plain_end(p);
        if (q >= len || (id <= 2 && q - p != 36)) return 2;
        p = q + 1;
        if (p < len && l[p] == '}') break;
        if (cp == 0 && p + 2 < len && l[p] == ',' && l[p + 1] == ' ' && l[p + 2] == '"') p += 3;
        else if (cp == 1 && p + 1 < len && l[p] == ',' && l[p + 1] == '"') p += 2;
        else return 2;
    }
    // key index i is bit i of the required-key mask (ysb_scan.hip K_*)
    if ((seen & require_mask) != require_mask || !((seen >> 2) & 1u) || !((seen >> 4) & 1u) || !((seen >> 5) & 1u))
        return 2;
    bool gen_order = n == 7;
    for (u32 i = 0; i < n; ++i) gen_order &= order[i] == i;
    if (gen_order) return cp ? 1 : 0;
    d->n = n;
    d->cp = (u32)cp;
    for (u32 i = 0; i < 8; ++i) d->order[i] = order[i];
    return 3;
}

// The batch's layout from SAMPLE_LINES of its lines (round 4; until round 3 the first line
// only): line 0 and one line at a hashed position in each of the other strata of
// [0, n).  If at least SAMPLE_AGREE of them name the same layout (for 3 the same key order
// and spacing), that one; otherwise several producers are interleaved and the flat-object
// tier, which takes every layout alike, runs first (2).  Only a choice of instantiation:
// every instantiation counts every line exactly.
// 46 of 64 (72 %): a producer writing most of the batch keeps its instantiation (its lines at
// full speed, the others through the tiers); a batch half of one layout (four producers, two
// of them in the generator's layout) reaches 46 of 64 in ~0.03 % of samples (with 32 lines
// and 23 of them: 0.4 %, which a bench seed hit)
constexpr u32 SAMPLE_LINES = 64, SAMPLE_AGREE = 46;
static_assert(SAMPLE_LINES <= (u32)SAMPLE_MAX, "device samples: one SampleSegs entry per line");
#ifndef YSB_MIXED_TILE
#define YSB_MIXED_TILE 1   // round 4: a sample without a majority layout takes the per-tile dispatch (4), not the flat tier (2)
#endif

// Sample line j: pairs of adjacent lines, one pair per stratum of [0, n) in SAMPLE_LINES / 2
// strata (lines 0 and 1, then a hashed position in each other stratum and the line after it)
// -- so the sample also tells producers writing in runs (adjacent lines alike) from a
// line-by-line interleave.
inline u64 sample_index(u64 n, u32 j) {
    if (n <= SAMPLE_LINES) return std::min<u64>(j, n ? n - 1 : 0);
    const u64 P = SAMPLE_LINES / 2, q = j >> 1;
    const u64 a = n * q / P, b = n * (q + 1) / P;   // stratum q
    const u64 base = q == 0 ? 0 : a + mix64(0x51ED27u + q) % std::max<u64>(1, b - a - 1);
    return std::min<u64>(base + (j & 1u), n - 1);
}

// req: the required-key mask (0x7F with YSB_F_REQUIRE_IP, else 0x3F)
inline int decide_layout(u32 req, const std::vector<std::pair<const u8*, u64>>& lines, LearnDesc* d) {
    std::vector<std::pair<int, LearnDesc>> got;
    for (const auto& l : lines) {
        LearnDesc di{};
        const int lay = learn_layout(l.first, l.second, req, &di);
        got.push_back({lay, lay == 3 ? di : LearnDesc{}});
    }
    if (got.empty()) return 0;
    u32 best_learned = 0;
    for (const auto& g : got) {   // the most frequent (layout, order) of the sample
        u32 k = 0;
        for (const auto& h : got) k += h.first == g.first && std::memcmp(&h.second, &g.second, sizeof(LearnDesc)) == 0;
        if (k >= std::min<u32>(SAMPLE_AGREE, (u32)got.size())) {
            *d = g.second;
            return g.first;
        }
        if (g.first == 3 && k > best_learned) {   // the most frequent learned order, for layout 4
            best_learned = k;
            *d = g.second;
        }
    }
#if YSB_MIXED_TILE
    // several producers.  Writing in runs (3 of 4 adjacent sample pairs alike): the per-tile
    // dispatch (4) -- tiles of one producer take its path (the learned order: the sample's
    // most frequent one), mixed tiles the flat tier; interleaved line by line: every tile
    // would be mixed, so the flat tier without the dispatch (2)
    u32 pairs = 0, alike = 0;
    for (size_t i = 0; i + 1 < got.size(); i += 2, ++pairs)
        alike += got[i].first == got[i + 1].first &&
                 std::memcmp(&got[i].second, &got[i + 1].second, sizeof(LearnDesc)) == 0;
    if (4 * alike >= 3 * pairs) {
        if (!best_learned) *d = LearnDesc{};
        return 4;
    }
#endif
    return 2;
}

// A host batch (held in the pinned slot).
inline int sniff_layout(u32 req, const uint8_t* bytes, u64 nbytes, const u32* off, u64 n, LearnDesc* d) {
    std::vector<std::pair<const u8*, u64>> lines;
    for (u32 j = 0; j < SAMPLE_LINES && j < n; ++j) {
        const u64 i = sample_index(n, j);
        const u64 s = off[i], e = i + 1 < n ? (u64)off[i + 1] : nbytes;
        if (s >= e || e > nbytes) return 0;   // bad offsets: the scan defers them anyway
        lines.push_back({bytes + s, std::min<u64>(e - s, SAMPLE_BYTES)});
    }
    return decide_layout(req, lines, d);
}

// The layout of a raw batch (host bytes): its first line and the first complete line after
// each of SAMPLE_LINES - 1 spread byte positions, decided as sniff_layout decides.
inline int sniff_raw(u32 req, const u8* b, u64 nbytes, LearnDesc* d) {
    auto line_at = [&](u64 p) -> std::pair<const u8*, u64> {   // the line starting at p
        const u64 lim = std::min<u64>(nbytes, p + SAMPLE_BYTES);
        u64 e = p;
        while (e < lim && b[e] != '\n' && b[e] != '\r') ++e;
        return {b + p, std::min<u64>(e + 1, nbytes) - p};
    };
    // pairs of adjacent lines (as sample_index): the first two, then the two after a '\n' at
    // each other stratum's start (a lone '\r' only ends lines elsewhere)
    auto next_start = [&](u64 p) -> u64 {   // past the '\n' at or after p (nbytes: none near)
        const u64 lim = std::min<u64>(nbytes, p + 4096);
        while (p < lim && b[p] != '\n') ++p;
        return p + 1 < lim ? p + 1 : nbytes;
    };
    std::vector<std::pair<const u8*, u64>> lines;
    for (u32 q = 0; q < SAMPLE_LINES / 2; ++q) {
        const u64 s0 = q == 0 ? 0 : next_start(nbytes * q / (SAMPLE_LINES / 2));
        if (s0 >= nbytes) continue;
        const u64 s1 = next_start(s0);
        if (s1 >= nbytes) continue;   // a pair or nothing
        lines.push_back(line_at(s0));
        lines.push_back(line_at(s1));
    }
    if (lines.empty()) lines.push_back(line_at(0));
    return decide_layout(req, lines, d);
}

// The sampled layout under the flags' hint: YSB_F_FLAT_FIRST keeps the flat-object tier
// first unless the first line names a key order (3: the learned-order instantiation, whose
// lines off that order go to the same flat tier).
inline int hinted_layout(bool flat_first, int sampled) {
    if (flat_first && sampled >= 0 && sampled != 3 && sampled != 4) return 2;
    return sampled;
}

inline bool same_decision(int a, const LearnDesc& la, int b, const LearnDesc& lb) {
    return a == b && (a != 3 || std::memcmp(&la, &lb, sizeof(LearnDesc)) == 0);
}

// A device launch queued behind other work runs on the two samples before its own (see
// sample_device_layout): the previous launch's decision `prev` if the one before it (`older`,
// -1: none -- the first two launches) decided the same; if they disagree (producers
// alternating by batch, or a producer that just changed its layout), the per-tile dispatch
// (4) with the newer sample's learned order, if it has one, until two samples agree again.
inline int settled_layout(int older, const LearnDesc& older_learn, int prev, const LearnDesc& prev_learn, LearnDesc* d) {
    if (older < 0 || same_decision(older, older_learn, prev, prev_learn)) {
        *d = prev_learn;
        return prev;
    }
    *d = prev == 3 || prev == 4 ? prev_learn : LearnDesc{};
    return 4;
}

}  // namespace ysb
