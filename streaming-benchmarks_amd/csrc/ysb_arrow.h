// ysb_arrow.h -- Apache Arrow record batches (include/ysb_hip.h "Arrow record batches"): the
// row rule, the schema binding, the host form's copy plan and a host model of the count.  No
// HIP here: the kernel (ysb_count_arrow.h, in the scan unit) follows the rule below and uses
// the YSB_HD predicates; tests/native/arrow_logic.cpp runs everything else on the CPU.
//
// A batch is three columns of n_rows rows -- ad_id, event_type, event_time -- described by a
// ysb_arrow_cols.  Row i is element `offset + i` of a column's offsets / values and bit
// `validity_offset + i` of its bitmap (bit k = bit k % 8 of byte k / 8; an absent bitmap means
// all valid) -- for an Arrow child both are batch.offset + child.offset; the host form's packed
// copy keeps the rows' elements from 0 and only the bitmap bytes over them, so there they differ.
//
// THE ROW RULE.  Per row, in order:
//   1. events += 1.
//   2. The row is invalid -- parse_errors += 1 and nothing else, the row getString would have
//      thrown on (AdvertisingTopologyNative.java:263-272) -- when, checked in this order,
//        (null)    the struct's bit or the bit of any of the three columns is zero;
//        (dict)    a dictionary index is outside [0, dict_len);
//        (null)    the dictionary value it names is null;
//        (offsets) a string value's offsets (ad_id, then event_type or its dictionary value,
//                  then event_time) break data_first <= off[k] <= off[k+1] <= data_bytes.
//   3. The row is a view iff its event_type value is exactly the four bytes `view`; views += 1.
//   4. The key is the ad_id value's bytes.  Above 56 bytes: a join miss (never foreign, never
//      parked: no table can hold it).  36 bytes: the cuckoo table, then the general table
//      where that is partial.  Other lengths: the general table.  A miss is join_misses, or
//      foreign_shard when a sharded context does not own the key; with parking the view is
//      parked with the time's parse outcome.
//   5. joined += 1.  An int64 time is taken as it is; a string time is Long.parseLong's
//      [+-]?[0-9]+ within int64 at any length (parse_digits, ysb_scan.hip).  A rejected time:
//      time_errors += 1 and no count.
//   6. bucket = div_trunc(time, divisor); counts[(campaign, bucket)] += 1.
// deferred never changes.
#pragma once
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ysb_hip.h"
#include "ysb_common.h"

namespace ysb {

enum : u32 { AR_AD = 0, AR_TYPE = 1, AR_TIME = 2, AR_DICTV = 3 };          // the columns (3: the dictionary)
enum : u32 { AR_OK = 0, AR_NULL = 1, AR_OFFSETS = 2, AR_DICT = 3 };        // why a row is invalid
constexpr u64 AR_MAX_ROWS = 0x7FFFFFFFull;
constexpr u64 AR_MAX_DICT = (1ull << 30) - 2;      // (dict_len + 1) * 4 bytes of offsets stay below 4 GiB
constexpr u64 AR_MAX_DATA = (1ull << 31) - 64;     // a string column's bytes: positions stay ints
constexpr u64 AR_ALIGN = 16;                       // the host form places every range at such a boundary

// ---- the predicates of rule 2 (host and device) --------------------------------------------
YSB_HD bool arrow_bit(u32 byte, u64 k) { return (byte >> (k & 7)) & 1u; }   // byte = bitmap[k / 8]
YSB_HD bool arrow_span_ok(u32 o0, u32 o1, u32 data_first, u64 data_bytes) {   // (offsets as stored: int32)
    const i64 a = (i64)(int32_t)o0, b = (i64)(int32_t)o1;
    return (i64)data_first <= a && a <= b && (u64)b <= data_bytes;
}
YSB_HD bool arrow_index_ok(u32 idx, u64 dict_len) { return (int32_t)idx >= 0 && (u64)idx < dict_len; }

#if !defined(__HIP_DEVICE_COMPILE__)

// ---- host readers --------------------------------------------------------------------------
inline bool arrow_valid_at(const u8* bm, u64 k) { return !bm || arrow_bit(bm[k >> 3], k); }
inline u32 arrow_u32_at(const u8* p, u64 k) { u32 v; std::memcpy(&v, p + 4 * k, 4); return v; }
inline i64 arrow_i64_at(const u8* p, u64 k) { i64 v; std::memcpy(&v, p + 8 * k, 8); return v; }

// Long.parseLong on n bytes (the host restatement of parse_digits).
inline bool arrow_parse_long(const u8* p, u64 n, i64* out) {
    u64 k = 0;
    if (n == 0) return false;
    bool neg = false;
    if (p[0] == '-') { neg = true; k = 1; }
    else if (p[0] == '+') k = 1;
    if (k >= n) return false;
    u64 acc = 0;
    const u32 last_max = neg ? 8u : 7u;
    for (; k < n; ++k) {
        const u32 d = (u32)p[k] - '0';
        if (d > 9u) return false;
        if (acc >= 922337203685477580ULL && (acc > 922337203685477580ULL || d > last_max)) return false;
        acc = acc * 10u + d;
    }
    *out = neg ? (i64)(0 - acc) : (i64)acc;
    return true;
}

// One value of a string column: its bytes, or false when its offsets break the rule.
struct ArrowValue { const u8* p = nullptr; u64 n = 0; };
inline bool arrow_value(const ysb_arrow_col& c, u64 elem, ArrowValue* v) {
    const u32 o0 = arrow_u32_at(c.offsets, elem), o1 = arrow_u32_at(c.offsets, elem + 1);
    if (!arrow_span_ok(o0, o1, c.data_first, c.data_bytes)) return false;
    v->p = c.data + (o0 - c.data_first);
    v->n = o1 - o0;
    return true;
}

// Rule 2 for row i, and the row's three values when it is valid.
struct ArrowRow {
    ArrowValue ad, type, time;   // time: a string time's bytes
    i64 time_i64 = 0;            // an int64 time
};
inline u32 arrow_row(const ysb_arrow_cols& A, u64 i, ArrowRow* r) {
    if (!arrow_valid_at(A.validity, A.offset + i)) return AR_NULL;
    for (int c = 0; c < 3; ++c)
        if (!arrow_valid_at(A.col[c].validity, A.col[c].validity_offset + i)) return AR_NULL;
    const ysb_arrow_col* ty = &A.col[AR_TYPE];
    u64 ty_elem = ty->offset + i;
    if (ty->kind == YSB_ARROW_DICT) {
        const u32 idx = arrow_u32_at(ty->data, ty_elem);
        if (!arrow_index_ok(idx, A.dict_len)) return AR_DICT;
        ty = &A.dict;
        ty_elem = A.dict.offset + idx;
        if (!arrow_valid_at(ty->validity, A.dict.validity_offset + idx)) return AR_NULL;
    }
    if (!arrow_value(A.col[AR_AD], A.col[AR_AD].offset + i, &r->ad)) return AR_OFFSETS;
    if (!arrow_value(*ty, ty_elem, &r->type)) return AR_OFFSETS;
    const ysb_arrow_col& tm = A.col[AR_TIME];
    if (tm.kind == YSB_ARROW_INT64) r->time_i64 = arrow_i64_at(tm.data, tm.offset + i);
    else if (!arrow_value(tm, tm.offset + i, &r->time)) return AR_OFFSETS;
    return AR_OK;
}

// ---- the host model ------------------------------------------------------------------------
struct ArrowCounts {
    u64 events = 0, views = 0, joined = 0, misses = 0, parse_errors = 0, time_errors = 0, foreign = 0;
    u64 invalid[4] = {0, 0, 0, 0};                     // by AR_NULL / AR_OFFSETS / AR_DICT
    std::map<std::pair<u32, i64>, u64> cells;          // (campaign, bucket) -> count
};

// find(key bytes, length <= 56) -> campaign or EMPTY_SLOT: ad_campaign.get(ad_id).
template <class Find>
void arrow_count_rows(const ysb_arrow_cols& A, i64 divisor, u32 shard_rank, u32 shard_n, Find&& find, ArrowCounts* out) {
    const DivMagic div = div_magic(divisor);
    for (u64 i = 0; i < A.n_rows; ++i) {
        out->events++;
        ArrowRow r;
        const u32 why = arrow_row(A, i, &r);
        if (why != AR_OK) { out->parse_errors++; out->invalid[why]++; continue; }
        if (!(r.type.n == 4 && std::memcmp(r.type.p, "view", 4) == 0)) continue;
        out->views++;
        u32 ci = EMPTY_SLOT;
        const bool keyed = r.ad.n <= MAX_KEY_BYTES;
        if (keyed) ci = find(r.ad.p, (u32)r.ad.n);
        if (ci == EMPTY_SLOT) {
            bool foreign = false;
            if (keyed && shard_n > 1u) {
                u32 kw[KEY_WORDS] = {};
                std::memcpy(kw, r.ad.p, r.ad.n);
                foreign = key_shard(key_hash(kw, (u32)r.ad.n), shard_n) != shard_rank;
            }
            ++(foreign ? out->foreign : out->misses);
            continue;
        }
        out->joined++;
        i64 t = r.time_i64;
        if (A.col[AR_TIME].kind != YSB_ARROW_INT64 && !arrow_parse_long(r.time.p, r.time.n, &t)) {
            out->time_errors++;
            continue;
        }
        out->cells[{ci, div_trunc(t, div)}]++;
    }
}

// ---- the schema binding --------------------------------------------------------------------
inline bool arrow_is_string_format(const char* f) { return f && (!std::strcmp(f, "u") || !std::strcmp(f, "z")); }

inline int arrow_refuse(std::string* err, const char* field, const char* fmt, const char* way_out) {
    char b[320];
    std::snprintf(b, sizeof b, "field '%s' has Arrow format '%s': %s", field, fmt ? fmt : "(null)", way_out);
    *err = b;
    return YSB_ERR_FORMAT;
}

inline int arrow_bind(const ArrowSchema* s, ysb_arrow_binding* out, std::string* err) {
    static const char* const NAME[3] = {"ad_id", "event_type", "event_time"};
    if (!s || !out) { *err = "NULL schema or binding"; return YSB_ERR_ARG; }
    if (!s->format || std::strcmp(s->format, "+s"))
        return arrow_refuse(err, s->name && *s->name ? s->name : "(top level)", s->format,
                            "a record batch is a struct (+s) of columns; export the batch, not one array");
    if (s->n_children < 0 || (s->n_children && !s->children)) { *err = "struct schema without children"; return YSB_ERR_ARG; }
    ysb_arrow_binding b{};
    b.n_children = s->n_children;
    for (int c = 0; c < 3; ++c) {
        b.child[c] = -1;
        for (int64_t k = 0; k < s->n_children; ++k)
            if (s->children[k] && s->children[k]->name && !std::strcmp(s->children[k]->name, NAME[c])) { b.child[c] = k; break; }
        if (b.child[c] < 0) return arrow_refuse(err, NAME[c], "(missing)", "the batch needs columns ad_id, event_type and event_time");
        const ArrowSchema* f = s->children[b.child[c]];
        const char* fmt = f->format ? f->format : "";
        if (f->dictionary) {
            if (c != (int)AR_TYPE)
                return arrow_refuse(err, NAME[c], fmt, "only event_type may be dictionary-encoded; decode it (cast to string)");
            if (std::strcmp(fmt, "i"))
                return arrow_refuse(err, NAME[c], fmt, "dictionary indices must be int32 (i); cast the indices to int32");
            if (!arrow_is_string_format(f->dictionary->format))
                return arrow_refuse(err, NAME[c], f->dictionary->format, "the dictionary's values must be utf8 (u) or binary (z); cast to string");
            b.kind[c] = YSB_ARROW_DICT;
        } else if (arrow_is_string_format(fmt)) {
            b.kind[c] = YSB_ARROW_STRING;
        } else if (c == (int)AR_TIME && (!std::strcmp(fmt, "l") || !std::strncmp(fmt, "tsm:", 4))) {
            b.kind[c] = YSB_ARROW_INT64;
        } else if (!std::strcmp(fmt, "U") || !std::strcmp(fmt, "Z")) {
            return arrow_refuse(err, NAME[c], fmt, "64-bit offsets are not read; cast to string (utf8) or binary");
        } else if (!std::strcmp(fmt, "vu") || !std::strcmp(fmt, "vz")) {
            return arrow_refuse(err, NAME[c], fmt, "string views are not read; cast to string (utf8) or binary");
        } else if (!std::strncmp(fmt, "w:", 2)) {
            return arrow_refuse(err, NAME[c], fmt, "fixed-size binary is not read; cast to binary");
        } else if (c == (int)AR_TIME && !std::strncmp(fmt, "ts", 2)) {
            return arrow_refuse(err, NAME[c], fmt, "only millisecond timestamps are read; cast to timestamp[ms], int64 or string");
        } else if (c == (int)AR_TIME) {
            return arrow_refuse(err, NAME[c], fmt, "event_time must be utf8 (u), binary (z), int64 (l) or timestamp[ms] (tsm:); cast to int64 or string");
        } else {
            return arrow_refuse(err, NAME[c], fmt, "the column must be utf8 (u) or binary (z); cast to string");
        }
    }
    *out = b;
    return YSB_OK;
}

// ---- the host form's copy plan -------------------------------------------------------------
// What ysb_submit_arrow copies of a batch, and nothing else is touched: for each range `bytes`
// bytes at src go to byte `dst` of the packed image (dst a multiple of AR_ALIGN).  `what` says
// which buffer of the packed batch the range is (arrow_plan_cols).
enum : u32 { AP_VALIDITY = 0, AP_OFFSETS = 1, AP_DATA = 2 };
struct ArrowRange {
    const u8* src;
    u64 bytes, dst;
    u32 col;      // AR_AD / AR_TYPE / AR_TIME / AR_DICTV, or 4: the struct's validity
    u32 what;     // AP_*
};
struct ArrowPlan {
    std::vector<ArrowRange> r;
    u64 total = 0;             // bytes of the packed image
    ysb_arrow_cols cols{};     // the packed batch, every pointer still NULL (arrow_plan_cols sets them)
};

inline void arrow_plan_add(ArrowPlan* p, const void* src, u64 bytes, u32 col, u32 what) {
    p->r.push_back({static_cast<const u8*>(src), bytes, p->total, col, what});
    p->total = (p->total + bytes + AR_ALIGN - 1) / AR_ALIGN * AR_ALIGN;
}
// the bitmap bytes that cover elements [elem, elem + n); *new_off <- the first one's bit in them
inline void arrow_plan_bitmap(ArrowPlan* p, const void* bm, u64 elem, u64 n, u32 col, u64* new_off) {
    *new_off = bm ? (elem & 7) : 0;
    if (bm && n) arrow_plan_add(p, static_cast<const u8*>(bm) + (elem >> 3), ((elem & 7) + n + 7) >> 3, col, AP_VALIDITY);
}
// a string array's elements [elem, elem + n): offsets [elem, elem + n] and the bytes between the
// first and the last of them
inline int arrow_plan_strings(ArrowPlan* p, const ArrowArray* a, u64 elem, u64 n, u32 col, ysb_arrow_col* out,
                              const char* name, std::string* err) {
    out->kind = YSB_ARROW_STRING;
    out->offset = 0;
    if (n == 0) return YSB_OK;
    if (a->n_buffers < 3 || !a->buffers || !a->buffers[1]) { *err = std::string(name) + ": NULL offsets buffer"; return YSB_ERR_ARG; }
    const u8* offs = static_cast<const u8*>(a->buffers[1]);
    const int32_t first = (int32_t)arrow_u32_at(offs, elem), last = (int32_t)arrow_u32_at(offs, elem + n);
    if (first < 0 || last < first) { *err = std::string(name) + ": the last offset lies below the first"; return YSB_ERR_ARG; }
    if (last > first && !a->buffers[2]) { *err = std::string(name) + ": NULL data buffer"; return YSB_ERR_ARG; }
    arrow_plan_add(p, offs + 4 * elem, 4 * (n + 1), col, AP_OFFSETS);
    if (last > first) arrow_plan_add(p, static_cast<const u8*>(a->buffers[2]) + first, (u64)(last - first), col, AP_DATA);
    out->data_first = (u32)first;
    out->data_bytes = (u64)last;
    return YSB_OK;
}

inline int arrow_plan(const ysb_arrow_binding& b, const ArrowArray* batch, ArrowPlan* p, std::string* err) {
    static const char* const NAME[3] = {"ad_id", "event_type", "event_time"};
    *p = ArrowPlan{};
    if (!batch) { *err = "NULL batch"; return YSB_ERR_ARG; }
    if (batch->n_children != b.n_children || (b.n_children && !batch->children)) { *err = "the batch's n_children does not match the binding"; return YSB_ERR_ARG; }
    if (batch->length < 0 || batch->offset < 0) { *err = "negative batch length or offset"; return YSB_ERR_ARG; }
    if ((u64)batch->length > AR_MAX_ROWS) { *err = "more than 2^31 - 1 rows"; return YSB_ERR_ARG; }
    const u64 n = (u64)batch->length, bo = (u64)batch->offset;
    ysb_arrow_cols& C = p->cols;
    C.n_rows = n;
    arrow_plan_bitmap(p, batch->n_buffers > 0 && batch->buffers ? batch->buffers[0] : nullptr, bo, n, 4, &C.offset);
    for (u32 c = 0; c < 3; ++c) {
        const ArrowArray* a = b.child[c] >= 0 && b.child[c] < batch->n_children ? batch->children[b.child[c]] : nullptr;
        if (!a) { *err = std::string(NAME[c]) + ": NULL child array"; return YSB_ERR_ARG; }
        if (a->length < 0 || a->offset < 0) { *err = std::string(NAME[c]) + ": negative length or offset"; return YSB_ERR_ARG; }
        if ((u64)a->length < bo + n) { *err = std::string(NAME[c]) + ": the child is shorter than the batch"; return YSB_ERR_ARG; }
        if ((u64)a->offset + bo + n > AR_MAX_ROWS) { *err = std::string(NAME[c]) + ": elements past 2^31 - 1"; return YSB_ERR_ARG; }
        const u64 elem = bo + (u64)a->offset;
        ysb_arrow_col& o = C.col[c];
        u64 voff = 0;
        arrow_plan_bitmap(p, a->n_buffers > 0 && a->buffers ? a->buffers[0] : nullptr, elem, n, c, &voff);
        if (b.kind[c] == YSB_ARROW_STRING) {
            if (int rc = arrow_plan_strings(p, a, elem, n, c, &o, NAME[c], err)) return rc;
            o.validity_offset = voff;
        } else {
            const u64 w = b.kind[c] == YSB_ARROW_INT64 ? 8 : 4;
            o.kind = b.kind[c];
            o.validity_offset = voff;
            if (b.kind[c] == YSB_ARROW_DICT) C.dict.kind = YSB_ARROW_STRING;
            if (n) {
                if (a->n_buffers < 2 || !a->buffers || !a->buffers[1]) { *err = std::string(NAME[c]) + ": NULL values buffer"; return YSB_ERR_ARG; }
                arrow_plan_add(p, static_cast<const u8*>(a->buffers[1]) + w * elem, w * n, c, AP_DATA);
                o.data_bytes = w * n;
            }
            if (b.kind[c] == YSB_ARROW_DICT && n) {
                const ArrowArray* d = a->dictionary;
                if (!d || d->length < 0 || d->offset < 0) { *err = std::string(NAME[c]) + ": missing or negative dictionary"; return YSB_ERR_ARG; }
                if ((u64)d->length > AR_MAX_DICT || (u64)d->offset + (u64)d->length > AR_MAX_ROWS) { *err = std::string(NAME[c]) + ": dictionary above 2^30 - 2 values"; return YSB_ERR_CAPACITY; }
                u64 dv = 0;
                arrow_plan_bitmap(p, d->n_buffers > 0 && d->buffers ? d->buffers[0] : nullptr, (u64)d->offset, (u64)d->length, AR_DICTV, &dv);
                if (int rc = arrow_plan_strings(p, d, (u64)d->offset, (u64)d->length, AR_DICTV, &C.dict, "event_type's dictionary", err)) return rc;
                C.dict.validity_offset = dv;
                C.dict_len = (u64)d->length;
            }
        }
    }
    // the ranges' places, now that every size is final
    u64 at = 0;
    for (ArrowRange& q : p->r) { q.dst = at; at = (at + q.bytes + AR_ALIGN - 1) / AR_ALIGN * AR_ALIGN; }
    p->total = at;
    return YSB_OK;
}

// The packed batch with its image at `base` (a host copy for the model, the slot's device buffer
// for the kernel).
inline ysb_arrow_cols arrow_plan_cols(const ArrowPlan& p, const u8* base) {
    ysb_arrow_cols C = p.cols;
    for (const ArrowRange& q : p.r) {
        const u8* at = base + q.dst;
        if (q.col == 4) { C.validity = at; continue; }
        ysb_arrow_col& o = q.col == AR_DICTV ? C.dict : C.col[q.col];
        (q.what == AP_VALIDITY ? o.validity : q.what == AP_OFFSETS ? o.offsets : o.data) = at;
    }
    return C;
}

// The whole batch viewed in place (host pointers, nothing copied): what the host model reads of
// an ArrowArray.  A string column's data ends at its array's last offset.
inline int arrow_view(const ysb_arrow_binding& b, const ArrowArray* batch, ysb_arrow_cols* out, std::string* err) {
    ArrowPlan p;
    if (int rc = arrow_plan(b, batch, &p, err)) return rc;   // (the same argument checks)
    ysb_arrow_cols C{};
    const u64 bo = (u64)batch->offset;
    C.n_rows = (u64)batch->length;
    C.validity = batch->n_buffers > 0 && batch->buffers ? static_cast<const u8*>(batch->buffers[0]) : nullptr;
    C.offset = bo;
    auto view = [](const ArrowArray* a, u32 kind, u64 elem, ysb_arrow_col* o) {
        o->kind = kind;
        o->validity = a->n_buffers > 0 && a->buffers ? static_cast<const u8*>(a->buffers[0]) : nullptr;
        o->offset = o->validity_offset = elem;
        if (kind == YSB_ARROW_STRING) {
            o->offsets = a->n_buffers > 1 ? static_cast<const u8*>(a->buffers[1]) : nullptr;
            o->data = a->n_buffers > 2 ? static_cast<const u8*>(a->buffers[2]) : nullptr;
            o->data_bytes = o->offsets ? arrow_u32_at(o->offsets, (u64)a->offset + (u64)a->length) : 0;
        } else {
            o->data = a->n_buffers > 1 ? static_cast<const u8*>(a->buffers[1]) : nullptr;
            o->data_bytes = ((u64)a->offset + (u64)a->length) * (kind == YSB_ARROW_INT64 ? 8 : 4);
        }
    };
    for (u32 c = 0; c < 3; ++c) {
        const ArrowArray* a = batch->children[b.child[c]];
        view(a, b.kind[c], bo + (u64)a->offset, &C.col[c]);
        if (b.kind[c] == YSB_ARROW_DICT && a->dictionary) {
            view(a->dictionary, YSB_ARROW_STRING, (u64)a->dictionary->offset, &C.dict);
            C.dict_len = (u64)a->dictionary->length;
        }
    }
    *out = C;
    return YSB_OK;
}

#endif  // !__HIP_DEVICE_COMPILE__

}  // namespace ysb
