// ysb_kafka.hip -- Kafka record batches unframed on the GPU (ysb_submit_kafka,
// ysb_kafka_unframe_device; the format, its ONE record reader and the host model: ysb_kafka.h).
// This is the deserialisation loop a consumer runs on a CPU between the fetch response and the
// first operator (KafkaSpout / FlinkKafkaConsumer in the reference): here the framed bytes cross
// PCIe and the values are found and gathered where they are scanned.
//
// Three launches, no workgroup waits for another:
//   kafka_walk_kernel    one wave per Kafka batch.  The chain of record lengths is the only
//                        serial part: `length` is decoded from a two-window LDS ring (windows of
//                        KAFKA_WIN bytes, the one behind them already requested into registers),
//                        every position wave-uniform.  Every 64 record starts (or at the batch's
//                        end) the lanes parse 64 record bodies at once, one per lane, with the
//                        shared reader; a wave prefix sum of the value lengths gives each record's
//                        output offset within its batch.  Record i of a batch lands at index
//                        first_record + i: the host's index holds that sum, so no device-wide scan
//                        over records is needed.
//   kafka_base_kernel    one workgroup: the exclusive scan of the batches' totals and the verdict.
//   kafka_gather_kernel  a workgroup per run of KAFKA_RUN records, whose output range is
//                        contiguous: staged through LDS, stored as 16-byte vectors between the
//                        first and last 16-byte boundary inside its own range and as single bytes
//                        at the two edges -- no vector shared with a neighbouring workgroup is
//                        read-modify-written (lz4_move's edge rule).
//
// Malformed input cannot fault or hang: every byte the walk reads lies in the 16-byte vectors
// that hold [records_off, records_off + records_bytes) (the host checked that extent against the
// buffer), every read of the parser is bounded by the reader's checks against the record's
// extent inside it, and every step of the chain moves on by at least 7 bytes.  The gather runs
// only on a call whose every batch the reader accepted.
//
// LZ4-compressed batches (ysb_kafka_lz4.h; ysb_submit_kafka_lz4) put four launches in front of
// the walk and one behind it, on the same stream:
//   lz4_measure_kernel         (ysb_lz4.hip, unchanged) each block's raw size, 0 for a bad block
//   kafka_inflate_plan_kernel  one workgroup: the decode's descriptors and the walk's index
//   lz4_decode_kernel / _wide  (ysb_lz4.hip) into the context's inflated buffer
//   kafka_walk_kernel          P.bytes the inflated buffer, P.batches the planned index
//   kafka_codec_kernel         the batches with a bad block become rule 8 in bout, whatever the
//                              walk made of their undecoded bytes; then base and gather as above.
// Snappy-compressed batches (codec 2; ysb_snappy.h, ysb_snappy.hip) take the same chain: their
// blocks carry YSB_SNAPPY_BLOCK in comp, the LZ4 measure and decode kernels skip those,
// snappy_preamble_kernel writes their raw sizes in front of the plan and snappy_decode_kernel
// decodes them behind the LZ4 decode -- a call may hold blocks of both kinds.  The plan also calls
// a batch bad whose extent would pass the inflated buffer (infl_cap): a snappy block's size is
// what its bytes say, and mapped bytes may change under the host's capacity check.
// The inflated extents lie at any byte alignment and the walk loads whole 16-byte vectors around
// an extent.  That is safe: the inflated buffer is 256-byte aligned with 64 bytes of slack
// behind the last extent, and the decode is complete before the walk (the same stream).  A batch
// the decode left unwritten is walked over whatever the buffer held; the reader's bounds hold
// for any bytes, and its verdict is replaced.
#include "ysb_kernels.h"
#include "ysb_kafka.h"
#include "ysb_lz4.h"

namespace ysb {

constexpr u32 KAFKA_TPB = 64;                 // the walk: one wave
constexpr u32 KAFKA_RING = 2 * KAFKA_WIN;     // two windows resident
static_assert(KAFKA_WIN == KAFKA_TPB * 16, "a window is one 16-byte vector per lane");
static_assert(KAFKA_GROUP == KAFKA_TPB, "one record body per lane");

// The chain's input: the batch's bytes through a ring of two windows in LDS.  Window w holds
// the bytes [w * KAFKA_WIN, (w + 1) * KAFKA_WIN) counted from the 16-byte boundary at or in
// front of the batch's first record byte; windows cur and cur + 1 are resident, cur + 2 is in
// flight in `next`.  byte() is wave-uniform: pos is, and every lane reads the same LDS byte.
struct KafkaWaveIn {
    const u8* ga;      // the 16-byte boundary at or in front of the first record byte
    u32 mis;           // the first record byte's distance from it
    u32 vend;          // mis + records_bytes rounded up to 16: no vector at or past it is loaded
    u8* lds;
    u32 lane;
    u32 cur;
    uint4 next;

    __device__ __forceinline__ uint4 load(u32 w) const {
        const u32 a = w * KAFKA_WIN + lane * 16;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (a < vend) v = *reinterpret_cast<const uint4*>(ga + a);
        return v;
    }
    __device__ __forceinline__ void put(u32 w, uint4 v) {
        *reinterpret_cast<uint4*>(lds + (w & 1u) * KAFKA_WIN + lane * 16) = v;
    }
    // windows w and w + 1 resident, where w holds pos (a varint is 5 bytes: it ends in w + 1 at most)
    __device__ __forceinline__ void ensure(u32 pos) {
        const u32 w = (pos + mis) / KAFKA_WIN;
        if (w == cur) return;
        __syncthreads();   // (one wave: every read of the ring so far is done)
        if (w == cur + 1) {
            put(w + 1, next);
        } else {
            put(w, load(w));
            put(w + 1, load(w + 1));
        }
        next = load(w + 2);
        cur = w;
        __syncthreads();
    }
    __device__ __forceinline__ u32 byte(u32 pos) const {
        return (u32)__builtin_amdgcn_readfirstlane((int)lds[(pos + mis) & (KAFKA_RING - 1)]);
    }
};

// The bodies' input: a lane's own record, straight from global memory (the chain's windows
// have just pulled those lines into the cache).
struct KafkaLaneIn {
    const u8* g;
    __device__ __forceinline__ u32 byte(u32 pos) const { return g[pos]; }
};

__device__ __forceinline__ u32 wave_sum(u32 v) {
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__global__ __launch_bounds__(KAFKA_TPB) void kafka_walk_kernel(const KafkaParams P) {
    __shared__ __align__(16) u8 ring[KAFKA_RING];
    const u32 lane = threadIdx.x, bi = blockIdx.x;
    const ysb_kafka_batch b = P.batches[bi];
    const u8* g = P.bytes + b.records_off;
    const u32 n = b.records_bytes, nrec = b.n_records;
    const u32 mis = (u32)(reinterpret_cast<uintptr_t>(g) & 15);
    KafkaWaveIn in{g - mis, mis, (mis + n + 15) & ~15u, ring, lane, 0xFFFFFFF0u, make_uint4(0, 0, 0, 0)};
    const KafkaLaneIn body_in{g};

    u32 pos = 0, rec = 0, total = 0, nulls = 0, keyed = 0, headers = 0;
    u32 bad_rec = 0, rule = KAFKA_OK;
    while (rec < nrec) {
        // the chain: up to 64 record starts, lane m keeps record rec + m's
        const u32 want = nrec - rec < KAFKA_GROUP ? nrec - rec : KAFKA_GROUP;
        u32 m = 0, my_body = 0, my_end = 0, chain_rule = KAFKA_OK;
        while (m < want) {
            if (pos >= n) {
                chain_rule = KAFKA_R_COUNT;
                break;
            }
            in.ensure(pos);
            u32 rb = 0, re = 0;
            chain_rule = kafka_read_len(in, pos, n, &rb, &re);
            if (chain_rule) break;
            if (lane == m) {
                my_body = rb;
                my_end = re;
            }
            pos = re;
            ++m;
        }
        // the bodies, one per lane
        KafkaRec r{};
        u32 br = KAFKA_OK;
        if (lane < m) br = kafka_read_body(body_in, my_body, my_end, &r);
        const unsigned long long badmask = __ballot(br != KAFKA_OK);
        if (badmask) {   // the smallest bad record lies in front of where the chain stopped
            const int j = __ffsll((long long)badmask) - 1;
            bad_rec = rec + (u32)j;
            rule = (u32)__shfl((int)br, j);
            break;
        }
        if (chain_rule) {
            bad_rec = rec + m;
            rule = chain_rule;
            break;
        }
        const u32 len = lane < m ? r.val_len : 0;
        u32 incl = len;
        for (int d = 1; d < 64; d <<= 1) {
            const u32 up = (u32)__shfl_up((int)incl, d);
            if ((int)lane >= d) incl += up;
        }
        if (lane < m) P.meta[b.first_record + rec + lane] = make_uint4(r.val_pos, total + incl - len, len, bi);
        total += (u32)__shfl((int)incl, 63);
        nulls += wave_sum(lane < m ? r.null_value : 0);
        keyed += wave_sum(lane < m ? r.keyed : 0);
        headers += wave_sum(lane < m ? r.headers : 0);
        rec += m;
    }
    if (rule == KAFKA_OK && pos != n) {   // bytes behind the last record
        bad_rec = nrec;
        rule = KAFKA_R_COUNT;
    }
    if (lane == 0) P.bout[bi] = KafkaBatchOut{total, bad_rec, rule, nulls, keyed, headers, 0};
}

constexpr u32 KAFKA_BASE_TPB = 256;

__global__ __launch_bounds__(KAFKA_BASE_TPB) void kafka_base_kernel(const KafkaParams P) {
    __shared__ u64 sh[KAFKA_BASE_TPB];
    __shared__ unsigned long long s_nulls, s_keyed, s_headers;
    __shared__ u32 s_bad, s_first;
    const u32 tid = threadIdx.x;
    if (tid == 0) {
        s_nulls = s_keyed = s_headers = 0;
        s_bad = 0;
        s_first = KAFKA_NONE;
    }
    __syncthreads();
    u64 carry = 0;
    for (u32 c0 = 0; c0 < P.n_batches; c0 += KAFKA_BASE_TPB) {
        const u32 k = c0 + tid;
        KafkaBatchOut o{};
        if (k < P.n_batches) o = P.bout[k];
        const bool bad = k < P.n_batches && o.rule != KAFKA_OK;
        const u64 v = bad ? 0 : o.total;
        sh[tid] = v;
        __syncthreads();
        for (u32 d = 1; d < KAFKA_BASE_TPB; d <<= 1) {
            const u64 add = tid >= d ? sh[tid - d] : 0;
            __syncthreads();
            sh[tid] += add;
            __syncthreads();
        }
        if (k < P.n_batches) P.base[k] = carry + sh[tid] - v;
        carry += sh[KAFKA_BASE_TPB - 1];
        __syncthreads();
        if (bad) {
            atomicAdd(&s_bad, 1u);
            atomicMin(&s_first, k);
        } else if (k < P.n_batches) {
            if (o.nulls) atomicAdd(&s_nulls, (unsigned long long)o.nulls);
            if (o.keyed) atomicAdd(&s_keyed, (unsigned long long)o.keyed);
            if (o.headers) atomicAdd(&s_headers, (unsigned long long)o.headers);
        }
    }
    __syncthreads();
    if (tid == 0) {
        KafkaHead h{};
        h.out_bytes = carry;
        h.n_lines = P.n_records;
        h.bad_batches = s_bad;
        h.first_bad = s_first;
        if (s_bad) {
            h.bad_rec = P.bout[s_first].bad_rec;
            h.rule = P.bout[s_first].rule;
        }
        h.nulls = s_nulls;
        h.keyed = s_keyed;
        h.headers = s_headers;
        h.overflow = (carry > P.out_cap || carry > 0xFFFFFFFFull) ? 1u : 0u;
        *P.head = h;
    }
}

constexpr u32 KAFKA_G_TPB = 256;
constexpr u32 KAFKA_RUN = 256;       // records per gather workgroup: one per thread
constexpr u32 KAFKA_CHUNK = 16384;   // output bytes staged in LDS at a time (a multiple of 16)

__global__ __launch_bounds__(KAFKA_G_TPB) void kafka_gather_kernel(const KafkaParams P) {
    __shared__ __align__(16) u8 buf[KAFKA_CHUNK];
    __shared__ u64 s_src[KAFKA_RUN];
    __shared__ u32 s_out[KAFKA_RUN], s_len[KAFKA_RUN];
    const KafkaHead hd = *P.head;
    if (hd.bad_batches || hd.overflow) return;   // (the same in every thread)
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 r0 = (u64)blockIdx.x * KAFKA_RUN;
    if (P.n_records == 0) {
        if (blockIdx.x == 0 && tid == 0) P.line_off[0] = 0;
        return;
    }
    const u32 cnt = (u32)(P.n_records - r0 < KAFKA_RUN ? P.n_records - r0 : KAFKA_RUN);
    if (tid < cnt) {
        const uint4 m = P.meta[r0 + tid];
        const u64 o = P.base[m.w] + m.y;
        s_src[tid] = P.batches[m.w].records_off + m.x;
        s_out[tid] = (u32)o;
        s_len[tid] = m.z;
        P.line_off[r0 + tid] = (u32)o;
        if (r0 + tid == P.n_records - 1) P.line_off[P.n_records] = (u32)(o + m.z);
    }
    __syncthreads();
    // the run's output range [start, end) and where it lies against 16-byte boundaries: position
    // v of the range's widened form is the byte at gbase + v, gbase 16-byte aligned
    const u32 start = s_out[0], end = s_out[cnt - 1] + s_len[cnt - 1];
    if (end == start) return;
    const u32 mis = (u32)(reinterpret_cast<uintptr_t>(P.out + start) & 15);
    u8* gbase = P.out + start - mis;
    const u32 span = mis + (end - start);
    for (u32 c0 = 0; c0 < span; c0 += KAFKA_CHUNK) {
        const u32 c1 = c0 + KAFKA_CHUNK < span ? c0 + KAFKA_CHUNK : span;
        // fill: a wave per record that reaches into [c0, c1)
        for (u32 r = wave; r < cnt; r += KAFKA_G_TPB / 64) {
            const u32 v0 = s_out[r] - start + mis, v1 = v0 + s_len[r];
            const u32 lo = v0 > c0 ? v0 : c0, hi = v1 < c1 ? v1 : c1;
            if (lo < hi) {
                const u8* src = P.bytes + s_src[r] + (lo - v0);
                for (u32 j = lane; j < hi - lo; j += 64) buf[lo - c0 + j] = src[j];
            }
        }
        __syncthreads();
        // store: bytes up to the first 16-byte boundary inside the range, vectors, bytes behind the last
        const u32 vlo = c0 > mis ? c0 : mis;
        u32 a = (vlo + 15) & ~15u;
        if (a > c1) a = c1;
        u32 z = c1 & ~15u;
        if (z < a) z = a;
        for (u32 v = vlo + tid; v < a; v += KAFKA_G_TPB) gbase[v] = buf[v - c0];
        for (u32 v = a + tid * 16; v < z; v += KAFKA_G_TPB * 16)
            *reinterpret_cast<uint4*>(gbase + v) = *reinterpret_cast<const uint4*>(buf + (v - c0));
        for (u32 v = z + tid; v < c1; v += KAFKA_G_TPB) gbase[v] = buf[v - c0];
        __syncthreads();
    }
}

// ---- compressed batches: the plan between the measure pass and the decode ---------------------
// Phase 1, KAFKA_PLAN_STEP blocks per step: a wave-shuffle inclusive scan of (raw size, measured
// 0) inside each wave, the four waves' totals through LDS, two running prefixes carried from
// step to step.  desc[i].out_off is block i's place in the inflated buffer.  Phase 2, a thread
// per Kafka batch: its extent is [out_off of its first block, out_off + raw of its last); a
// batch whose zero count moves, or whose extent would end past P.infl_cap, is bad -- its smallest
// such block is the verdict and its blocks' descriptors get raw 0, so the decode writes nothing of it.  Every index read is bounded by
// the host's checks (kafka_lz4_entries); all values leave through ordinary vector stores.
static_assert(KAFKA_PLAN_STEP == 256, "four waves per step");

__global__ __launch_bounds__(KAFKA_PLAN_STEP) void kafka_inflate_plan_kernel(const KafkaPlanParams P) {
    __shared__ u32 w_raw[4], w_zero[4];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    u64 run = 0;
    u32 zrun = 0;
    for (u32 at = 0; at < P.n_blocks; at += KAFKA_PLAN_STEP) {
        const u32 i = at + tid;
        const u32 r = i < P.n_blocks ? P.raw[i] : 0u;
        const u32 z = (i < P.n_blocks && r == 0u) ? 1u : 0u;
        u32 ir = r, iz = z;
        for (int d = 1; d < 64; d <<= 1) {
            const u32 ur = (u32)__shfl_up((int)ir, d), uz = (u32)__shfl_up((int)iz, d);
            if ((int)lane >= d) {
                ir += ur;
                iz += uz;
            }
        }
        if (lane == 63) {
            w_raw[wave] = ir;
            w_zero[wave] = iz;
        }
        __syncthreads();
        u32 pr = 0, pz = 0, tr = 0, tz = 0;
        for (u32 w = 0; w < 4; ++w) {
            if (w < wave) {
                pr += w_raw[w];
                pz += w_zero[w];
            }
            tr += w_raw[w];
            tz += w_zero[w];
        }
        if (i < P.n_blocks) {
            const Lz4FrameBlock b = P.blocks[i];
            P.desc[i] = Lz4Desc{b.offset, run + (pr + ir - r), b.comp, r};
            P.zeros[i] = zrun + (pz + iz - z);
            P.block_bad[i] = 0u;
        }
        run += tr;
        zrun += tz;
        __syncthreads();   // the waves' totals are rewritten by the next step
    }
    if (tid == 0) {
        P.zeros[P.n_blocks] = zrun;
        *P.head = KafkaPlanHead{{LZ4_NO_BAD, 0u}, zrun, 0u, run};
    }
    __threadfence();
    __syncthreads();   // phase 2 reads desc[] and zeros[] that other threads of this workgroup wrote
    for (u32 k = tid; k < P.n_batches; k += KAFKA_PLAN_STEP) {
        const ysb_kafka_frame f = P.frames[k];
        ysb_kafka_batch b = P.batches[k];
        u64 off = 0;
        u32 bytes = 0, bad = KAFKA_NONE;
        if (f.n_blocks) {
            const u64 first = f.first_block, last = first + f.n_blocks - 1;
            off = P.desc[first].out_off;
            bytes = (u32)(P.desc[last].out_off + P.raw[last] - off);
            // (a block past the inflated buffer: the host sized it by what it read, and mapped
            // bytes may have changed since; an LZ4 call's 64 KiB per block never gets here)
            const bool over = P.desc[last].out_off + P.raw[last] > P.infl_cap;
            if (over || P.zeros[last + 1] != P.zeros[first]) {
                for (u32 j = 0; j < f.n_blocks; ++j)
                    if (P.raw[first + j] == 0u || P.desc[first + j].out_off + P.raw[first + j] > P.infl_cap) {
                        bad = j;
                        break;
                    }
                for (u32 j = 0; j < f.n_blocks; ++j) P.desc[first + j].raw = 0u;
                bytes = 0;
            }
        }
        b.records_off = off;
        b.records_bytes = bytes;
        P.planned[k] = b;
        P.codec_bad[k] = bad;
    }
}

// The codec verdict, a thread per Kafka batch: the plan's bad block, else (only when the decode
// recorded a bad block at all) the smallest block of the batch that the decoder flagged.
__global__ __launch_bounds__(256) void kafka_codec_kernel(const KafkaPlanParams P, KafkaBatchOut* bout) {
    const u32 k = blockIdx.x * 256 + threadIdx.x;
    if (k >= P.n_batches) return;
    u32 j = P.codec_bad[k];
    if (j == KAFKA_NONE && P.head->bad[1] != 0u) {
        const ysb_kafka_frame f = P.frames[k];
        u32 n = 0;
        for (u32 i = 0; i < f.n_blocks; ++i)
            if (P.block_bad[f.first_block + i]) {
                if (j == KAFKA_NONE) j = i;
                ++n;
            }
        if (n) atomicAdd(&P.head->decoder_bad, n);
    }
    if (j != KAFKA_NONE) bout[k] = KafkaBatchOut{0, j, KAFKA_R_CODEC, 0, 0, 0, 0};
}

// ---- CRC-32C of the indexed batches (ysb_kafka_crc.h: the arithmetic, the layout, the host model) ----
// The tables are copied into LDS once per workgroup; each wave then takes batches wave-id,
// wave-id + waves, ...  (wave w of workgroup g has id w * gridDim + g, so a call of few large
// batches spreads over the CUs before it doubles up inside one).  Per batch: the walk's own
// geometry, a window of 1024 bytes as one 16-byte vector per lane, two windows' loads in flight;
// per window one round of 16 independent LDS lookups; behind the last window one multiplication
// by the lane's constant, an xor over the wave and the final xor.  Nothing outside the vectors
// that hold [records_off - 44, records_off + records_bytes) is loaded; the bytes of the first and
// the last vector that lie outside the range are masked (crc_edge), the stored CRC's four among
// them, which lane 0 reads by themselves.  Every extent is the host's (kafka_entry_ok, records_off
// >= 44): no byte decides an address or a trip count.
static_assert(CRC_WIN == KAFKA_WIN && CRC_LANES == 64, "the walk's window, one vector per lane");

__device__ __forceinline__ CrcVec crc_load(const u8* g0, i64 off, u32 span) {
    CrcVec v{{0, 0, 0, 0}};
    if (off >= 0 && off < (i64)span) {
        const uint4 q = *reinterpret_cast<const uint4*>(g0 + off);
        v.w[0] = q.x;
        v.w[1] = q.y;
        v.w[2] = q.z;
        v.w[3] = q.w;
    }
    return v;
}

__global__ __launch_bounds__(KAFKA_CRC_TPB) void kafka_crc_kernel(const KafkaCrcParams P) {
    __shared__ __align__(16) u32 tab[CRC_TABLE_WORDS];
    const u32 tid = threadIdx.x, lane = tid & 63;
    const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    for (u32 i = tid; i < CRC_TABLE_WORDS / 4; i += KAFKA_CRC_TPB)
        reinterpret_cast<uint4*>(tab)[i] = reinterpret_cast<const uint4*>(P.tables)[i];
    __syncthreads();
    const u32* consts = P.tables + CRC_TABLE_WORDS;
    const u64 waves = (u64)gridDim.x * (KAFKA_CRC_TPB / 64);
    for (u64 k = (u64)wave * gridDim.x + blockIdx.x; k < P.n_batches; k += waves) {
        const ysb_kafka_batch b = P.batches[k];
        const u8* from = P.bytes + b.records_off - KAFKA_CRC_STORED;   // the stored CRC, then the range
        const CrcGrid g = crc_grid((u64)reinterpret_cast<uintptr_t>(from), KAFKA_CRC_STORED - KAFKA_CRC_COVERED,
                                   b.records_bytes + KAFKA_CRC_COVERED);   // (g.first is 0: four bytes lie in front)
        const u8* g0 = from - (reinterpret_cast<uintptr_t>(from) & 15);
        i64 off = crc_vec_off(g, 0, lane);
        CrcVec v0 = crc_load(g0, off, g.span), v1 = crc_load(g0, off + CRC_WIN, g.span);
        u32 s = 0;
        for (u32 w = 0; w < g.windows; ++w) {
            const CrcVec v2 = crc_load(g0, off + 2 * (i64)CRC_WIN, g.span);
            if (off >= 0 && crc_is_edge(g, (u32)off)) crc_edge(g, (u32)off, &v0);
            s = crc_step16(tab, s, v0);
            v0 = v1;
            v1 = v2;
            off += CRC_WIN;
        }
        u32 t = crc_lane_finish(consts, g, lane, s);
        for (int d = 32; d; d >>= 1) t ^= (u32)__shfl_xor((int)t, d);
        if (lane == 0) {
            const u32 got = ~t, want = (u32)from[0] << 24 | (u32)from[1] << 16 | (u32)from[2] << 8 | (u32)from[3];
            P.crc[k] = make_uint2(got, want);
            if (P.bout && got != want) P.bout[k] = KafkaBatchOut{0, 0, KAFKA_R_CRC, 0, 0, 0, 0};
        }
    }
}

hipError_t launch_kafka_crc(const KafkaCrcParams& p, u32 cus, hipStream_t s) {
    const u32 need = (p.n_batches + KAFKA_CRC_TPB / 64 - 1) / (KAFKA_CRC_TPB / 64), cap = cus * KAFKA_CRC_WGS_PER_CU;
    hipLaunchKernelGGL(kafka_crc_kernel, dim3(need < cap ? need : cap), dim3(KAFKA_CRC_TPB), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_kafka_plan(const KafkaPlanParams& p, hipStream_t s) {
    hipLaunchKernelGGL(kafka_inflate_plan_kernel, dim3(1), dim3(KAFKA_PLAN_STEP), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_kafka_codec(const KafkaPlanParams& p, KafkaBatchOut* bout, hipStream_t s) {
    if (!p.n_batches) return hipSuccess;
    hipLaunchKernelGGL(kafka_codec_kernel, dim3((p.n_batches + 255) / 256), dim3(256), 0, s, p, bout);
    return hipGetLastError();
}

hipError_t launch_kafka_walk(const KafkaParams& p, hipStream_t s) {
    hipLaunchKernelGGL(kafka_walk_kernel, dim3(p.n_batches), dim3(KAFKA_TPB), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_kafka_base(const KafkaParams& p, hipStream_t s) {
    hipLaunchKernelGGL(kafka_base_kernel, dim3(1), dim3(KAFKA_BASE_TPB), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_kafka_gather(const KafkaParams& p, hipStream_t s) {
    const u64 grid = p.n_records ? (p.n_records + KAFKA_RUN - 1) / KAFKA_RUN : 1;
    hipLaunchKernelGGL(kafka_gather_kernel, dim3((u32)grid), dim3(KAFKA_G_TPB), 0, s, p);
    return hipGetLastError();
}

}  // namespace ysb
