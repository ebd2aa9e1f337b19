// arrow_logic.cpp -- csrc/ysb_arrow.h on the CPU: the schema binding over every accepted and
// refused format, the row rule and its host model over a hand-made corpus, and the host form's
// copy plan (exactly the bytes the rows need; the model on the packed copy equals the model on
// the original with every other source byte poisoned).  Stand-alone: g++ alone, and again with
// -fsanitize=address,undefined (exact-size heap buffers, so a read past a plan's range faults).
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "ysb_arrow.h"

using namespace ysb;

static int g_fail = 0;
#define CHECK(x)                                                                  \
    do {                                                                          \
        if (!(x)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #x); ++g_fail; } \
    } while (0)

// ---- a little builder of Arrow C structs over exact-size heap buffers ---------------------------
struct Buf {
    std::unique_ptr<u8[]> p;
    size_t n = 0;
    Buf() = default;
    explicit Buf(const std::vector<u8>& v) : p(v.empty() ? nullptr : new u8[v.size()]), n(v.size()) {
        if (n) std::memcpy(p.get(), v.data(), n);
    }
};
struct Arr {
    std::vector<Buf> bufs;
    std::vector<const void*> ptrs;
    std::vector<std::unique_ptr<Arr>> kids;
    std::vector<ArrowArray*> kid_ptrs;
    std::unique_ptr<Arr> dict;
    ArrowArray a{};
    void finish(int64_t length, int64_t offset) {
        ptrs.clear();
        for (auto& b : bufs) ptrs.push_back(b.p.get());
        kid_ptrs.clear();
        for (auto& k : kids) kid_ptrs.push_back(&k->a);
        a.length = length;
        a.null_count = -1;
        a.offset = offset;
        a.n_buffers = (int64_t)bufs.size();
        a.buffers = ptrs.data();
        a.n_children = (int64_t)kids.size();
        a.children = kid_ptrs.data();
        a.dictionary = dict ? &dict->a : nullptr;
    }
};
static std::vector<u8> bitmap_of(const std::vector<int>& valid) {
    std::vector<u8> b((valid.size() + 7) / 8, 0);
    for (size_t i = 0; i < valid.size(); ++i)
        if (valid[i]) b[i / 8] |= (u8)(1u << (i % 8));
    return b;
}
template <class T>
static std::vector<u8> bytes_of(const std::vector<T>& v) {
    std::vector<u8> b(v.size() * sizeof(T));
    if (!v.empty()) std::memcpy(b.data(), v.data(), b.size());
    return b;
}
static std::unique_ptr<Arr> strings(const std::vector<std::string>& v, const std::vector<int>* valid, int64_t offset, int64_t length) {
    auto r = std::make_unique<Arr>();
    std::vector<int32_t> off(1, 0);
    std::vector<u8> data;
    for (auto& s : v) {
        data.insert(data.end(), s.begin(), s.end());
        off.push_back((int32_t)data.size());
    }
    r->bufs.emplace_back(valid ? bitmap_of(*valid) : std::vector<u8>());
    r->bufs.emplace_back(bytes_of(off));
    r->bufs.emplace_back(data);
    r->finish(length, offset);
    return r;
}
template <class T>
static std::unique_ptr<Arr> values(const std::vector<T>& v, const std::vector<int>* valid, int64_t offset, int64_t length) {
    auto r = std::make_unique<Arr>();
    r->bufs.emplace_back(valid ? bitmap_of(*valid) : std::vector<u8>());
    r->bufs.emplace_back(bytes_of(v));
    r->finish(length, offset);
    return r;
}
static std::unique_ptr<Arr> batch_of(std::unique_ptr<Arr> ad, std::unique_ptr<Arr> ty, std::unique_ptr<Arr> tm,
                                     const std::vector<int>* valid, int64_t offset, int64_t length) {
    auto r = std::make_unique<Arr>();
    r->bufs.emplace_back(valid ? bitmap_of(*valid) : std::vector<u8>());
    r->kids.push_back(std::move(ad));
    r->kids.push_back(std::move(ty));
    r->kids.push_back(std::move(tm));
    r->finish(length, offset);
    return r;
}

// ---- schemas -----------------------------------------------------------------------------------
struct Sch {
    ArrowSchema s{};
    std::vector<std::unique_ptr<Sch>> kids;
    std::vector<ArrowSchema*> kid_ptrs;
    std::unique_ptr<Sch> dict;
    std::string fmt, name;
};
static std::unique_ptr<Sch> field(const std::string& name, const std::string& fmt, const char* dict_fmt = nullptr) {
    auto r = std::make_unique<Sch>();
    r->fmt = fmt;
    r->name = name;
    r->s.format = r->fmt.c_str();
    r->s.name = r->name.c_str();
    if (dict_fmt) {
        r->dict = field("", dict_fmt);
        r->s.dictionary = &r->dict->s;
    }
    return r;
}
static std::unique_ptr<Sch> schema_of(const char* top, std::vector<std::unique_ptr<Sch>> kids) {
    auto r = field("", top);
    r->kids = std::move(kids);
    for (auto& k : r->kids) r->kid_ptrs.push_back(&k->s);
    r->s.n_children = (int64_t)r->kids.size();
    r->s.children = r->kid_ptrs.data();
    return r;
}
static int bind3(const char* ad, const char* ty, const char* tm, ysb_arrow_binding* b, std::string* err,
                 const char* ty_dict = nullptr, const char* top = "+s", const char* tm_name = "event_time") {
    std::vector<std::unique_ptr<Sch>> k;
    k.push_back(field("other", "l"));
    k.push_back(field("event_time" == std::string(tm_name) ? "event_time" : tm_name, tm));
    k.push_back(field("ad_id", ad));
    k.push_back(field("event_type", ty, ty_dict));
    auto s = schema_of(top, std::move(k));
    return arrow_bind(&s->s, b, err);
}

static void test_binding() {
    ysb_arrow_binding b;
    std::string e;
    for (const char* ad : {"u", "z"})
        for (const char* ty : {"u", "z"})
            for (const char* tm : {"u", "z", "l", "tsm:", "tsm:UTC"}) {
                CHECK(bind3(ad, ty, tm, &b, &e) == YSB_OK);
                CHECK(b.n_children == 4 && b.child[0] == 2 && b.child[1] == 3 && b.child[2] == 1);
                CHECK(b.kind[0] == YSB_ARROW_STRING && b.kind[1] == YSB_ARROW_STRING);
                CHECK(b.kind[2] == ((tm[0] == 'l' || tm[0] == 't') ? YSB_ARROW_INT64 : YSB_ARROW_STRING));
            }
    for (const char* d : {"u", "z"}) CHECK(bind3("u", "i", "l", &b, &e, d) == YSB_OK && b.kind[1] == YSB_ARROW_DICT);
    struct Bad { const char *ad, *ty, *tm, *dict, *field, *fmt; };
    const Bad bad[] = {
        {"U", "u", "u", nullptr, "ad_id", "'U'"},       {"Z", "u", "u", nullptr, "ad_id", "'Z'"},
        {"vu", "u", "u", nullptr, "ad_id", "'vu'"},     {"u", "vz", "u", nullptr, "event_type", "'vz'"},
        {"w:36", "u", "u", nullptr, "ad_id", "'w:36'"}, {"u", "u", "tss:", nullptr, "event_time", "'tss:'"},
        {"u", "u", "tsu:UTC", nullptr, "event_time", "'tsu:UTC'"}, {"u", "u", "tsn:", nullptr, "event_time", "'tsn:'"},
        {"u", "u", "i", nullptr, "event_time", "'i'"},  {"u", "l", "u", nullptr, "event_type", "'l'"},
        {"u", "s", "u", "u", "event_type", "'s'"},      {"u", "c", "u", "u", "event_type", "'c'"},
        {"u", "l", "u", "u", "event_type", "'l'"},      {"u", "i", "u", "U", "event_type", "'U'"},
        {"u", "i", "u", "l", "event_type", "'l'"},      {"u", "u", "g", nullptr, "event_time", "'g'"},
    };
    for (const Bad& x : bad) {
        e.clear();
        CHECK(bind3(x.ad, x.ty, x.tm, &b, &e, x.dict) == YSB_ERR_FORMAT);
        CHECK(e.find(x.field) != std::string::npos && e.find(x.fmt) != std::string::npos && e.find("cast") != std::string::npos);
    }
    CHECK(bind3("u", "u", "u", &b, &e, nullptr, "+l") == YSB_ERR_FORMAT && e.find("+l") != std::string::npos && e.find("struct") != std::string::npos);
    CHECK(bind3("u", "u", "u", &b, &e, nullptr, "+s", "time") == YSB_ERR_FORMAT && e.find("event_time") != std::string::npos && e.find("missing") != std::string::npos);
    // a dictionary anywhere but on event_type
    {
        std::vector<std::unique_ptr<Sch>> k;
        k.push_back(field("ad_id", "i", "u"));
        k.push_back(field("event_type", "u"));
        k.push_back(field("event_time", "u"));
        auto s = schema_of("+s", std::move(k));
        CHECK(arrow_bind(&s->s, &b, &e) == YSB_ERR_FORMAT && e.find("ad_id") != std::string::npos && e.find("cast") != std::string::npos);
    }
    CHECK(arrow_bind(nullptr, &b, &e) == YSB_ERR_ARG);
}

// ---- the model ---------------------------------------------------------------------------------
static const std::map<std::string, u32>& the_map() {
    static const std::map<std::string, u32> m = {{"", 0}, {std::string(35, 'a'), 1}, {std::string(36, 'b'), 2},
                                                 {std::string(37, 'c'), 3}, {std::string(56, 'd'), 4}};
    return m;
}
static ArrowCounts run(const ysb_arrow_cols& A, i64 div = 10000, u32 rank = 0, u32 nr = 1) {
    ArrowCounts r;
    arrow_count_rows(A, div, rank, nr, [&](const u8* k, u32 n) {
        auto it = the_map().find(std::string(reinterpret_cast<const char*>(k), n));
        return it == the_map().end() ? (u32)EMPTY_SLOT : it->second;
    }, &r);
    return r;
}
static bool same(const ArrowCounts& a, const ArrowCounts& b) {
    return a.events == b.events && a.views == b.views && a.joined == b.joined && a.misses == b.misses &&
           a.parse_errors == b.parse_errors && a.time_errors == b.time_errors && a.foreign == b.foreign &&
           a.invalid[1] == b.invalid[1] && a.invalid[2] == b.invalid[2] && a.invalid[3] == b.invalid[3] && a.cells == b.cells;
}
static ysb_arrow_binding bound(u32 ty = YSB_ARROW_STRING, u32 tm = YSB_ARROW_STRING) {
    ysb_arrow_binding b{};
    b.n_children = 3;
    b.child[0] = 0; b.child[1] = 1; b.child[2] = 2;
    b.kind[0] = YSB_ARROW_STRING; b.kind[1] = ty; b.kind[2] = tm;
    return b;
}
static ysb_arrow_cols view_of(const ysb_arrow_binding& b, const Arr& batch) {
    ysb_arrow_cols C{};
    std::string e;
    CHECK(arrow_view(b, &batch.a, &C, &e) == YSB_OK);
    return C;
}

static void test_parse_long() {
    struct T { const char* s; bool ok; i64 v; };
    const T t[] = {{"+1", true, 1}, {"-0", true, 0}, {"9223372036854775807", true, INT64_MAX}, {"9223372036854775808", false, 0},
                   {"-9223372036854775808", true, INT64_MIN}, {"-9223372036854775809", false, 0},
                   {"09223372036854775807", true, INT64_MAX}, {"19223372036854775807", false, 0},
                   {"0000000000000000000000000123456", true, 123456}, {"", false, 0}, {" ", false, 0}, {"12a4", false, 0},
                   {"+", false, 0}, {"-", false, 0}, {"1500000000000", true, 1500000000000LL}};
    for (const T& x : t) {
        i64 v = 0;
        const bool ok = arrow_parse_long(reinterpret_cast<const u8*>(x.s), std::strlen(x.s), &v);
        CHECK(ok == x.ok && (!ok || v == x.v));
    }
}

static void test_model_corpus() {
    const std::string B36(36, 'b'), T = "1500000012345";
    // ad ids of 0, 35, 36, 37, 56, 57 and 200 bytes
    {
        std::vector<std::string> ads = {"", std::string(35, 'a'), B36, std::string(37, 'c'), std::string(56, 'd'),
                                        std::string(57, 'e'), std::string(200, 'f'), std::string(36, 'z')};
        const size_t n = ads.size();
        auto b = batch_of(strings(ads, nullptr, 0, n), strings(std::vector<std::string>(n, "view"), nullptr, 0, n),
                          strings(std::vector<std::string>(n, T), nullptr, 0, n), nullptr, 0, n);
        const ArrowCounts r = run(view_of(bound(), *b));
        CHECK(r.events == 8 && r.views == 8 && r.joined == 5 && r.misses == 3 && r.parse_errors == 0 && r.cells.size() == 5);
        for (u32 c = 0; c < 5; ++c) CHECK(r.cells.count({c, 150000001}) == 1);
        // a sharded context: the 57- and 200-byte keys stay join misses, the unknown 36-byte key is foreign on one rank
        const ArrowCounts s0 = run(view_of(bound(), *b), 10000, 0, 2), s1 = run(view_of(bound(), *b), 10000, 1, 2);
        CHECK(s0.misses + s0.foreign == 3 && s1.misses + s1.foreign == 3 && s0.foreign + s1.foreign == 1 && s0.misses >= 2 && s1.misses >= 2);
    }
    // types: only the four bytes `view`
    {
        std::vector<std::string> ty = {"view", "viewer", "vie", "View", "", "click"};
        const size_t n = ty.size();
        auto b = batch_of(strings(std::vector<std::string>(n, B36), nullptr, 0, n), strings(ty, nullptr, 0, n),
                          strings(std::vector<std::string>(n, T), nullptr, 0, n), nullptr, 0, n);
        const ArrowCounts r = run(view_of(bound(), *b));
        CHECK(r.events == 6 && r.views == 1 && r.joined == 1);
    }
    // string times (time errors only after the join) and int64 times
    {
        std::vector<std::string> tm = {"+1", "-0", "9223372036854775807", "9223372036854775808", "-9223372036854775808",
                                       "-9223372036854775809", "0000000000000000000000000123456", "", " ", "12a4"};
        const size_t n = tm.size();
        std::vector<std::string> ads(n, B36);
        ads[9] = std::string(36, 'z');   // a miss: its bad time is never looked at
        auto b = batch_of(strings(ads, nullptr, 0, n), strings(std::vector<std::string>(n, "view"), nullptr, 0, n),
                          strings(tm, nullptr, 0, n), nullptr, 0, n);
        const ArrowCounts r = run(view_of(bound(), *b));
        CHECK(r.views == 10 && r.joined == 9 && r.misses == 1 && r.time_errors == 4);
        CHECK(r.cells.at({2, 0}) == 2 && r.cells.at({2, 12}) == 1 && r.cells.at({2, INT64_MAX / 10000}) == 1 && r.cells.at({2, INT64_MIN / 10000}) == 1);
        std::vector<i64> it = {0, -1, -9999, -10000, 9999, 10000, INT64_MAX, INT64_MIN};
        auto bi = batch_of(strings(std::vector<std::string>(it.size(), B36), nullptr, 0, it.size()),
                           strings(std::vector<std::string>(it.size(), "view"), nullptr, 0, it.size()), values(it, nullptr, 0, it.size()),
                           nullptr, 0, it.size());
        const ArrowCounts ri = run(view_of(bound(YSB_ARROW_STRING, YSB_ARROW_INT64), *bi));
        CHECK(ri.joined == 8 && ri.time_errors == 0 && ri.cells.at({2, 0}) == 4 && ri.cells.at({2, -1}) == 1 && ri.cells.at({2, 1}) == 1);
        CHECK(run(view_of(bound(YSB_ARROW_STRING, YSB_ARROW_INT64), *bi), 7).cells.at({2, -1428}) == 2);   // -9999 / 7, -10000 / 7
    }
    // nulls in each column and at struct level; every bitmap's first bit used is bit 3 of a byte
    {
        const size_t k = 12, lead = 3;
        std::vector<int> v[4];
        for (int j = 0; j < 4; ++j) {
            v[j].assign(lead, 1);
            for (size_t i = 0; i < k; ++i) v[j].push_back((int)(i % 5) != j);
        }
        std::vector<std::string> ads(lead + k, B36), ty(lead + k, "view"), tm(lead + k, T);
        auto b = batch_of(strings(ads, &v[1], 0, lead + k), strings(ty, &v[2], 0, lead + k), strings(tm, &v[3], 0, lead + k), &v[0], lead, k);
        const ArrowCounts r = run(view_of(bound(), *b));
        CHECK(r.events == 12 && r.parse_errors == 10 && r.invalid[AR_NULL] == 10 && r.joined == 2 && r.views == 2);
    }
    // a dictionary: duplicate `view` entries, a null value, indices -1 and dict_len
    {
        std::vector<std::string> dv = {"view", "click", "view", "purchase", "viewer"};
        std::vector<int> dvalid = {1, 1, 1, 0, 1};
        std::vector<int32_t> idx = {0, 1, 2, 3, 4, -1, 5, 2, 0, 1 << 30};
        const size_t n = idx.size();
        auto ty = values(idx, nullptr, 0, n);
        ty->dict = strings(dv, &dvalid, 0, dv.size());
        ty->finish(n, 0);
        auto b = batch_of(strings(std::vector<std::string>(n, B36), nullptr, 0, n), std::move(ty),
                          strings(std::vector<std::string>(n, T), nullptr, 0, n), nullptr, 0, n);
        const ArrowCounts r = run(view_of(bound(YSB_ARROW_DICT), *b));
        CHECK(r.events == 10 && r.views == 4 && r.joined == 4 && r.parse_errors == 4 && r.invalid[AR_DICT] == 3 && r.invalid[AR_NULL] == 1);
    }
    // offsets that run backwards or past data_bytes (the data over-allocated with countable bytes)
    {
        const size_t k = 8;
        std::vector<int32_t> ao, to, mo;
        for (size_t i = 0; i <= k; ++i) { ao.push_back((int32_t)(36 * i)); to.push_back((int32_t)(4 * i)); mo.push_back((int32_t)(13 * i)); }
        ao[3] = ao[2] - 5;    // row 2 runs backwards; row 3 is 77 bytes: a join miss
        mo[k] += 13;          // the last row ends past data_bytes
        to[0] = -4;           // a negative first offset
        std::string ad, ty, tm;
        for (size_t i = 0; i < k + 4; ++i) { ad += B36; ty += "view"; tm += T; }
        Buf abuf(bytes_of(ao)), tbuf(bytes_of(to)), mbuf(bytes_of(mo));
        Buf ad_d(std::vector<u8>(ad.begin(), ad.end())), ty_d(std::vector<u8>(ty.begin(), ty.end())), tm_d(std::vector<u8>(tm.begin(), tm.end()));
        ysb_arrow_cols C{};
        C.n_rows = k;
        const Buf* o[3] = {&abuf, &tbuf, &mbuf};
        const Buf* d[3] = {&ad_d, &ty_d, &tm_d};
        const u64 stated[3] = {36 * k, 4 * k, 13 * k};
        for (int c = 0; c < 3; ++c) {
            C.col[c].kind = YSB_ARROW_STRING;
            C.col[c].offsets = o[c]->p.get();
            C.col[c].data = d[c]->p.get();
            C.col[c].data_bytes = stated[c];
        }
        const ArrowCounts r = run(C);
        CHECK(r.events == 8 && r.parse_errors == 3 && r.invalid[AR_OFFSETS] == 3 && r.views == 5 && r.joined == 4 && r.misses == 1);
        // data_first: the same bytes addressed from offset 36 on make row 0 of ad_id invalid too ... which it is already
        C.col[0].data_first = 36;
        C.col[0].data = ad_d.p.get() + 36;
        const ArrowCounts r2 = run(C);
        CHECK(r2.parse_errors == 3 && r2.joined == 4);
        C.col[1].data_first = 8;   // rows 0 and 1 of event_type now lie below the stated bytes
        C.col[1].data = ty_d.p.get() + 8;
        CHECK(run(C).parse_errors == 4);
    }
}

// ---- the plan ----------------------------------------------------------------------------------
static void test_plan() {
    const size_t total = 200;
    std::vector<std::string> ads, ty, tm;
    std::vector<i64> ti;
    std::vector<int32_t> idx;
    std::vector<int> va, vy, vm, vs;
    const char* types[3] = {"view", "click", "purchase"};
    for (size_t i = 0; i < total; ++i) {
        ads.push_back(i % 7 == 0 ? std::string(35, 'a') : i % 7 == 1 ? std::string(37, 'c') : std::string(36, 'b'));
        ty.push_back(types[i % 3]);
        tm.push_back(std::to_string(1500000000000LL + (i64)i * 777));
        ti.push_back(1500000000000LL + (i64)i * 777);
        idx.push_back((int32_t)(i % 3));
        va.push_back(i % 11 != 1);
        vy.push_back(i % 13 != 2);
        vm.push_back(i % 17 != 3);
        vs.push_back(i % 19 != 4);
    }
    for (int enc = 0; enc < 3; ++enc)            // strings, int64 times, dictionary types
        for (int bitmaps = 0; bitmaps < 2; ++bitmaps)
            for (int64_t off : {0, 1, 7, 67})
                for (int64_t n : {0, 1, 64, 100}) {
                    // the struct's offset and the children's own add up: split `off` between them
                    const int64_t bo = off / 2, co = off - bo;
                    auto a = strings(ads, bitmaps ? &va : nullptr, co, (int64_t)total - co);
                    std::unique_ptr<Arr> y, m;
                    if (enc == 2) {
                        y = values(idx, bitmaps ? &vy : nullptr, co, (int64_t)total - co);
                        std::vector<int> dvalid = {1, 1, 1};
                        y->dict = strings({"view", "click", "purchase"}, bitmaps ? &dvalid : nullptr, 0, 3);
                        y->finish((int64_t)total - co, co);
                    } else {
                        y = strings(ty, bitmaps ? &vy : nullptr, co, (int64_t)total - co);
                    }
                    m = enc == 1 ? values(ti, bitmaps ? &vm : nullptr, co, (int64_t)total - co)
                                 : strings(tm, bitmaps ? &vm : nullptr, co, (int64_t)total - co);
                    auto b = batch_of(std::move(a), std::move(y), std::move(m), bitmaps ? &vs : nullptr, bo, n);
                    const ysb_arrow_binding bd = bound(enc == 2 ? YSB_ARROW_DICT : YSB_ARROW_STRING, enc == 1 ? YSB_ARROW_INT64 : YSB_ARROW_STRING);
                    const ArrowCounts want = run(view_of(bd, *b));
                    CHECK(want.events == (u64)n);
                    ArrowPlan p;
                    std::string e;
                    CHECK(arrow_plan(bd, &b->a, &p, &e) == YSB_OK);
                    // exactly the bytes the rows need: per column the offsets [elem, elem + n], the
                    // data between the first and last of them, the bitmap bytes over the rows
                    u64 need = 0;
                    const u64 elem = (u64)off;
                    auto bm = [&](u64 e0, u64 cnt) { return bitmaps && cnt ? (((e0 & 7) + cnt + 7) >> 3) : 0; };
                    if (n) {
                        need += bm((u64)bo, (u64)n);
                        for (int c = 0; c < 3; ++c) {
                            need += bm(elem, (u64)n);
                            const Arr& k = *b->kids[c];
                            if (bd.kind[c] == YSB_ARROW_STRING) {
                                const u8* o = k.bufs[1].p.get();
                                need += 4 * ((u64)n + 1) + (arrow_u32_at(o, elem + (u64)n) - arrow_u32_at(o, elem));
                            } else {
                                need += (bd.kind[c] == YSB_ARROW_INT64 ? 8 : 4) * (u64)n;
                            }
                        }
                        if (enc == 2) need += bm(0, 3) + 4 * 4 + 17;
                    }
                    u64 got = 0, at = 0;
                    for (const ArrowRange& q : p.r) {
                        got += q.bytes;
                        CHECK(q.dst % AR_ALIGN == 0 && q.dst >= at && q.bytes > 0);
                        at = q.dst + q.bytes;
                    }
                    CHECK(got == need && p.total >= at && p.total % AR_ALIGN == 0 && p.total < at + AR_ALIGN);
                    // the packed copy, in an exact-size buffer ...
                    std::unique_ptr<u8[]> image(new u8[p.total ? p.total : 1]);
                    std::memset(image.get(), 0xEE, p.total);
                    for (const ArrowRange& q : p.r) std::memcpy(image.get() + q.dst, q.src, q.bytes);
                    // ... and then every source byte poisoned: the model on the copy is the model on the original
                    std::function<void(Arr&)> poison = [&](Arr& x) {
                        for (Buf& bf : x.bufs)
                            for (size_t i = 0; i < bf.n; ++i) bf.p[i] = (u8)(0x5A ^ i);
                        for (auto& k : x.kids) poison(*k);
                        if (x.dict) poison(*x.dict);
                    };
                    poison(*b);
                    CHECK(same(run(arrow_plan_cols(p, image.get())), want));
                }
    // the argument errors
    {
        const int64_t n = 10;
        auto mk = [&]() {
            return batch_of(strings(std::vector<std::string>(n, "x"), nullptr, 0, n), strings(std::vector<std::string>(n, "view"), nullptr, 0, n),
                            strings(std::vector<std::string>(n, "1"), nullptr, 0, n), nullptr, 0, n);
        };
        ArrowPlan p;
        std::string e;
        auto b = mk();
        b->a.n_children = 2;
        CHECK(arrow_plan(bound(), &b->a, &p, &e) == YSB_ERR_ARG && e.find("n_children") != std::string::npos);
        b = mk(); b->a.length = -1;
        CHECK(arrow_plan(bound(), &b->a, &p, &e) == YSB_ERR_ARG);
        b = mk(); b->a.offset = -1;
        CHECK(arrow_plan(bound(), &b->a, &p, &e) == YSB_ERR_ARG);
        b = mk(); b->a.length = (int64_t)1 << 31;
        CHECK(arrow_plan(bound(), &b->a, &p, &e) == YSB_ERR_ARG);
        b = mk(); b->a.length = n + 1;   // the children are shorter
        CHECK(arrow_plan(bound(), &b->a, &p, &e) == YSB_ERR_ARG && e.find("shorter") != std::string::npos);
        b = mk(); b->kids[0]->ptrs[1] = nullptr;
        CHECK(arrow_plan(bound(), &b->a, &p, &e) == YSB_ERR_ARG && e.find("offsets") != std::string::npos);
        b = mk(); b->kids[2]->ptrs[2] = nullptr;
        CHECK(arrow_plan(bound(), &b->a, &p, &e) == YSB_ERR_ARG && e.find("data") != std::string::npos);
        b = mk();
        const int32_t neg = -1;
        std::memcpy(b->kids[1]->bufs[1].p.get() + 4 * n, &neg, 4);
        CHECK(arrow_plan(bound(), &b->a, &p, &e) == YSB_ERR_ARG && e.find("below the first") != std::string::npos);
        b = mk(); b->a.length = 0;       // an empty batch plans nothing
        CHECK(arrow_plan(bound(), &b->a, &p, &e) == YSB_OK && p.r.empty() && p.total == 0);
    }
}

int main() {
    test_binding();
    test_parse_long();
    test_model_corpus();
    test_plan();
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("arrow_logic OK\n");
    return 0;
}
