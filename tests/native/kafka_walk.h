// The walk kernel's order of work (kafka_walk_kernel, csrc/ysb_kafka.hip) on the host, for the
// native programs that compare it with the serial model of csrc/ysb_kafka.h: kafka_logic.cpp and
// kafka_seq_logic.cpp.
#pragma once
#include <algorithm>
#include "ysb_kafka.h"

// The chain of lengths for up to KAFKA_GROUP records, then their bodies; the smallest bad record
// wins.  Must equal the serial model's verdict.  ct (optional): the counters of a good batch.
static inline ysb::u32 walk_like_kernel(const ysb::u8* rec, ysb::u32 n, ysb::u32 nrec, ysb::u32* bad_rec, ysb::u64* total,
                                        ysb_kafka_counters* ct = nullptr) {
    using namespace ysb;
    KafkaHostIn in{rec};
    u32 pos = 0, done = 0;
    *total = 0;
    while (done < nrec) {
        const u32 want = std::min(nrec - done, KAFKA_GROUP);
        u32 m = 0, body[KAFKA_GROUP], end[KAFKA_GROUP], chain = KAFKA_OK;
        while (m < want) {
            if (pos >= n) { chain = KAFKA_R_COUNT; break; }
            chain = kafka_read_len(in, pos, n, &body[m], &end[m]);
            if (chain) break;
            pos = end[m++];
        }
        for (u32 j = 0; j < m; ++j) {
            KafkaRec r{};
            const u32 rule = kafka_read_body(in, body[j], end[j], &r);
            if (rule) { *bad_rec = done + j; return rule; }
            *total += r.val_len;
            if (ct) {
                ct->records += 1;
                ct->null_values += r.null_value;
                ct->keyed += r.keyed;
                ct->headers += r.headers;
            }
        }
        if (chain) { *bad_rec = done + m; return chain; }
        done += m;
    }
    *bad_rec = nrec;
    return pos == n ? KAFKA_OK : KAFKA_R_COUNT;
}
