"""Kafka record batches laid out on purpose, not by a packer's habits: the corpus of
tests/test_kafka_seq_logic.py (CPU: the models, the host entries and the sanitized native program
tests/native/kafka_seq_logic.cpp) and tests/test_gpu_kafka_seq.py (the five Kafka kernels of
csrc/ysb_kafka.hip).  Every function is a pure function of its arguments; nothing is drawn at
random, so the corpus is the same bytes everywhere and the CPU test pins its SHA-256.

  fault_cases()     each malformed record of kafka_model.malformed_corpus() at record k of a
                    batch, k around the walk's rounds of GROUP records; two faults of both kinds
                    in one round and in adjacent rounds; the count rule at a round's boundary;
  cut_cases()       one valid 130-record batch cut at chosen bytes;
  window_batches()  valid batches for ONE launch: at each of the 16 residues of the first record
                    byte, a `length` varint of every width split at every byte across the
                    walk's window edges, the skip path followed by a straddling `length`, many
                    steps fed from the prefetched window, batch ends at every residue;
  base_calls()      calls of more batches than the base kernel scans per step, with counters that
                    differ in every chunk, and bad batches on both sides of the carry;
  gather_calls()    runs that share one 16-byte vector, empty runs, record counts at the run's
                    size, ranges that end next to a staging chunk's edge;
  serialize(...)    every batch as tests/native/kafka_seq_logic.cpp reads it.
"""
import collections
import functools
import struct

import kafka_model as M

# The kernels' geometry these cases aim at.  tests/test_kafka_seq_logic.py reads the constexpr
# lines of the sources named here and fails when one differs.
GROUP = 64         # KAFKA_GROUP      csrc/ysb_kafka.h: record bodies per round of the walk
WIN = 1024         # KAFKA_WIN        csrc/ysb_kafka.h: a window of the walk's ring (two resident)
BASE_STEP = 256    # KAFKA_BASE_TPB   csrc/ysb_kafka.hip: batches per step of the base kernel's scan
RUN = 256          # KAFKA_RUN        csrc/ysb_kafka.hip: records per gather workgroup
CHUNK = 16384      # KAFKA_CHUNK      csrc/ysb_kafka.hip: output bytes a gather workgroup stages at a time
PLAN_STEP = 256    # KAFKA_PLAN_STEP  csrc/ysb_kernels.h: blocks per step of the inflate plan's scan
CONSTANTS = {"KAFKA_GROUP": GROUP, "KAFKA_WIN": WIN, "KAFKA_BASE_TPB": BASE_STEP, "KAFKA_RUN": RUN,
             "KAFKA_CHUNK": CHUNK, "KAFKA_PLAN_STEP": PLAN_STEP}

FAULT_AT = (0, 1, 63, 64, 65, 127, 128, 129, 200)
EDGES = (WIN, 2 * WIN, 3 * WIN, 4 * WIN)
OUT_SHIFTS = (0, 1, 15, 16, 17)       # what tests/test_gpu_kafka_seq.py gives every gather call

# One batch: its record bytes as they are and its recordsCount; expect None (valid) or the
# (record, rule number) that makes it bad; totals (valid only) = (value bytes, null values,
# keyed records, headers), counted from the Record objects, not by a reader; mis: the residue
# modulo 16 its first record byte is meant for (window batches), else None.
Batch = collections.namedtuple("Batch", "name raw count expect totals mis")
# One call: its batches in order; verdict None or (bad_batches, first_bad, record, rule).
Call = collections.namedtuple("Call", "name batches verdict")


def value(i, n):
    return bytes((i * 7 + j) % 251 for j in range(n))


def records_bytes(records):
    return M.pack_batch(records)[M.HEADER:]


def totals_of(records):
    return (sum(len(r.value or b"") for r in records), sum(r.value is None for r in records),
            sum(r.key is not None for r in records), sum(len(r.headers) for r in records))


def valid_batch(name, records, mis=None):
    return Batch(name, records_bytes(records), len(records), None, totals_of(records), mis)


def good_record(i):
    """Record i of a good prefix: value lengths 5 .. 94, a key every third, a null value every
    eleventh, 0 .. 2 headers."""
    v = None if i % 11 == 10 else value(i, 5 + (13 * i) % 90)
    return M.Record(v, key=(b"k%d" % i) if i % 3 == 0 else None,
                    headers=((b"h", None), (b"trace", b"%d" % i))[:i % 3 if i % 5 == 0 else 0], ts_delta=i - 7)


@functools.lru_cache(maxsize=None)
def good_prefix(k):
    return records_bytes([good_record(i) for i in range(k)])


def record_spanning(total, seed, **kw):
    """A record (no key, no headers, offsetDelta 0) whose `length` and body take exactly `total`
    bytes; kw: length_pad."""
    n = total - 12
    for _ in range(4):
        r = M.Record(value(seed, n), offset_delta=0, **kw)
        span = len(records_bytes([r]))
        if span == total:
            return r
        n += total - span
    raise AssertionError("no record of %d bytes" % total)


def blob_of(batches, base_offset=0):
    """The batches as one buffer of whole Kafka batches, base offsets consecutive."""
    out = bytearray()
    for b in batches:
        out += M.pack_batch(None, base_offset=base_offset, records_count=b.count, raw_records=b.raw)
        base_offset += max(b.count, 1)
    return bytes(out)


# ---- 1. a bad record at record k ---------------------------------------------------------------

def _remainders():
    """malformed_corpus() without its leading good record: [(name, rule name, count - 1, bytes)]."""
    good = M.Record(b'{"a":1}', key=b"k", headers=[(b"h", None)], ts_delta=-3).body(0)
    g = M.varint(len(good)) + good
    out = []
    for name, rule, count, rec in M.malformed_corpus():
        assert rec[:len(g)] == g, name
        out.append((name, rule, count - 1, rec[len(g):]))
    assert len(out) == 15
    return out


def _remainder(name):
    return [r for r in _remainders() if r[0] == name][0][3]


@functools.lru_cache(maxsize=None)
def fault_cases(ks=FAULT_AT):
    """[Batch], each bad by construction with the stated (record, rule)."""
    out = []
    for k in ks:
        for name, rule, more, rem in _remainders():
            # more: how many records the corpus entry states behind its good one -- 1 for a
            # broken record, 2 for "a record short" (a good record, then nothing), 0 for "a
            # record over" (a good record the count does not cover)
            count = k + more
            record = k + 1 if more == 2 else k
            out.append(Batch("%s at record %d" % (name, k), good_prefix(k) + rem, count, (record, M.RULE[rule]), None, None))
    body, neg, five = _remainder("key past the record"), _remainder("negative length"), _remainder("length 5")
    mid = lambda a, b: records_bytes([good_record(i) for i in range(a, b)])   # noqa: E731
    out += [
        Batch("a body fault at 70, a length fault at 75", good_prefix(70) + body + mid(71, 75) + five, 76,
              (70, M.RULE["key"]), None, None),
        Batch("a length fault at 66, a body fault at 70 behind it", good_prefix(66) + neg + mid(67, 70) + body, 71,
              (66, M.RULE["length"]), None, None),
        Batch("a body fault at 63, a length fault at 64", good_prefix(63) + body + five, 65, (63, M.RULE["key"]), None, None),
        Batch("the batch ends behind record 63, count 65", good_prefix(64), 65, (64, M.RULE["count"]), None, None),
        Batch("count 64, 65 records present", good_prefix(65), 64, (64, M.RULE["count"]), None, None),
        Batch("count 0 over 20 record bytes", records_bytes([record_spanning(20, 3)]), 0, (0, M.RULE["count"]), None, None),
    ]
    assert len(out[-1].raw) == 20
    return tuple(out)


def two_fault_cases():
    return fault_cases()[-6:-3]


# ---- 2. a valid batch cut at chosen bytes --------------------------------------------------------

FRONT = M.pack_batch([M.Record(b"ok")])                       # the good batch in front of a fault or cut case
BACK_RECORDS = [M.Record(b"after")]
CASE_MIS = (len(FRONT) + M.HEADER) % 16                       # the case batch's first record byte, in a 16-byte aligned buffer


def with_neighbours(b):
    """A fault or cut case as the GPU tests send it: a good batch in front and one behind."""
    return FRONT + M.pack_batch(None, base_offset=1, records_count=b.count, raw_records=b.raw) + \
        M.pack_batch(BACK_RECORDS, base_offset=1000)


def record_fields(raw):
    """[(start, body, key length at, value length at, end)] of the records of valid record bytes."""
    out, pos = [], 0
    while pos < len(raw):
        length, body = M.read_varint(raw, pos, len(raw))
        p = body + 1
        _, p = M.read_varint(raw, p, len(raw), 10, 64)
        _, p = M.read_varint(raw, p, len(raw))
        key_at = p
        klen, p = M.read_varint(raw, p, len(raw))
        p += max(klen, 0)
        out.append((pos, body, key_at, p, body + length))
        pos = body + length
    return out


@functools.lru_cache(maxsize=None)
def cut_cases():
    """The 130-record good prefix with a 2-byte key length and value length in records 63 .. 65
    and 128, cut at about 40 places.  The expected verdict is derived from where the cut falls:
    at a record's first byte the count rule, inside its `length` the varint rule, behind it the
    record runs past the batch."""
    recs = [good_record(i) for i in range(130)]
    for i in (63, 64, 65, 128):
        recs[i] = M.Record(value(i, 100 + i), key=value(i + 1, 70), ts_delta=i, length_pad=1)
    raw = records_bytes(recs)
    f = record_fields(raw)
    assert len(f) == 130 and len(raw) > 3 * WIN
    cuts = set()
    for i in (63, 64, 65, 128):
        start, body, key_at, val_at, end = f[i]
        assert body - start == 3
        cuts |= {start, end - 1, start + 1, start + 2, key_at + 1, val_at + 1}
    for edge in (WIN, 2 * WIN, 3 * WIN):
        cuts |= {edge - CASE_MIS + d for d in (-1, 0, 1)}
    cuts |= {0, 1, f[1][0], f[129][0], len(raw) - 1}
    out = []
    for c in sorted(cuts):
        i = max(j for j in range(130) if f[j][0] <= c)
        start, body = f[i][0], f[i][1]
        rule = "count" if c == start else "varint" if c < body else "past_batch"
        out.append(Batch("130 records cut at byte %d" % c, raw[:c], 130, (i, M.RULE[rule]), None, None))
    assert 35 <= len(out) <= 45, len(out)
    return tuple(out)


# ---- 3. the walk's window ring -----------------------------------------------------------------

def ensure_trace(raw, mis):
    """What KafkaWaveIn::ensure does at every record start of valid record bytes whose first byte
    lies mis bytes behind a 16-byte boundary: [(pos, width of `length`, window, path)], path one
    of "first", "stay", "step" (window cur + 1: the prefetched vector becomes resident) and
    "skip" (a later window: both loaded anew)."""
    out, pos, cur = [], 0, None
    while pos < len(raw):
        w = (pos + mis) // WIN
        path = "first" if cur is None else "stay" if w == cur else "step" if w == cur + 1 else "skip"
        cur = w
        length, body = M.read_varint(raw, pos, len(raw))
        out.append((pos, body - pos, w, path))
        pos = body + length
    return out


def straddles(raw, mis):
    """[(edge, width, split, path)] for every `length` of the trace that touches a window edge:
    split = how many of its bytes lie in front of the edge (0: it starts on the edge, width: it
    ends there)."""
    out = []
    for pos, width, w, path in ensure_trace(raw, mis):
        a = pos + mis
        edge = (a + WIN - 1) // WIN * WIN
        if edge and edge - a <= width:
            out.append((edge, width, edge - a, path))
    return out


def _tail(seed):
    return [M.Record(value(seed, 9), key=b"t"), M.Record(value(seed + 1, 31), headers=[(b"h", b"v")])]


def _straddle_batch(mis, edge, L, s):
    """The second record's `length` of L bytes starts s bytes in front of the edge."""
    first = record_spanning(edge - mis - s, edge // WIN + L + s)
    # L = 1: a body below 64 bytes; from 2 on a body whose minimal `length` has two groups
    second = M.Record(value(L * 8 + s, 20 if L == 1 else 150 + 7 * s), offset_delta=1, length_pad=0 if L == 1 else L - 2)
    return valid_batch("mis %d: length of %d bytes, %d in front of %d" % (mis, L, s, edge), [first, second] + _tail(s), mis)


def _skip_batches(mis):
    """A lead record into window 1 (a step), a record of 2.5 windows that ends s bytes in front
    of window 4's start, a 5-byte `length` across that edge (the skip path loads windows 3 and 4),
    a body of most of a window and a record of a window (the next two starts step into windows 4
    and 5: what the skip path prefetched, and what the step behind it did)."""
    out = []
    for s in (1, 4):
        lead = record_spanning(4 * WIN - mis - s - (2 * WIN + WIN // 2), 40 + s)
        long_ = record_spanning(2 * WIN + WIN // 2, 50 + s)
        over = M.Record(value(60 + s, WIN - 100 + s), offset_delta=2, length_pad=3)
        out.append(valid_batch("mis %d: skip, then a 5-byte length %d in front of %d" % (mis, s, 4 * WIN),
                               [lead, long_, over] + _tail(70 + s) + [record_spanning(WIN, 75 + s)] + _tail(80 + s), mis))
    return out


def _steps_batch(mis):
    recs = [record_spanning(WIN + 1 + (5 * i + mis) % 9, 80 + i) for i in range(9)]
    assert len({len(r.value) for r in recs}) == 9
    recs += [M.Record(value(100 + i, 3 + (7 * i) % 40), key=b"s" if i % 4 == 0 else None) for i in range(30)]
    return valid_batch("mis %d: nine steps from the prefetched window, then 30 short records" % mis, recs, mis)


def _end_batches(mis):
    """Record bytes ending at mis + n = r (mod 16) for every r; one ending on a window edge, one a
    byte behind it."""
    out = []
    for r in range(16):
        n = 24 + (r - mis - 24) % 16
        out.append(valid_batch("mis %d: the records end at residue %d" % (mis, r),
                               [record_spanning(12, r), record_spanning(n - 12, r + 1)], mis))
        assert (mis + len(out[-1].raw)) % 16 == r
    for d in (0, 1):
        out.append(valid_batch("mis %d: the records end %d behind a window edge" % (mis, d),
                               [record_spanning(700, d), record_spanning(WIN - mis + d - 700, 9)], mis))
        assert mis + len(out[-1].raw) == WIN + d
    return out


ALL_EDGES_AT = tuple(range(16))     # every edge at every residue: the full set of the issue (no reduction taken)


@functools.lru_cache(maxsize=None)
def window_batches():
    out = []
    for mis in range(16):
        for edge in EDGES:
            if mis not in ALL_EDGES_AT and edge != 2 * WIN:
                continue
            for L in range(1, 6):
                for s in range(L + 1):
                    out.append(_straddle_batch(mis, edge, L, s))
        out += _skip_batches(mis)
        out.append(_steps_batch(mis))
        out += _end_batches(mis)
    return tuple(out)


def _filler(at, mis, i):
    """A one-record batch at byte `at` whose value is padded until the batch behind it has its
    first record byte at residue mis."""
    for p in range(16):
        b = valid_batch("filler %d" % i, [M.Record(value(i, p))])
        if (at + M.HEADER + len(b.raw) + M.HEADER) % 16 == mis:
            return b
    raise AssertionError("no filler")


def place(batches, start=0):
    """The batches of one call, a filler in front of each that has a `mis`, so that its first
    record byte lies at that residue in a buffer whose byte `start` is 16-byte aligned:
    [Batch] with the fillers."""
    out, at = [], start
    for i, b in enumerate(batches):
        if b.mis is not None:
            f = _filler(at, b.mis, i)
            out.append(f)
            at += M.HEADER + len(f.raw)
            assert (at + M.HEADER) % 16 == b.mis
        out.append(b)
        at += M.HEADER + len(b.raw)
    return out


# ---- 4. the base kernel past its first chunk ---------------------------------------------------

def _base_batch(i):
    """Batch i of a base call: 1 .. 3 records; keys with period 4, null values with period 5,
    0 .. 3 headers with period 7 -- every counter's total differs in every chunk of 256."""
    recs = []
    for j in range(1 + i % 3):
        x = 3 * i + j
        recs.append(M.Record(None if x % 5 == 0 else value(x, 4 + x % 29), key=b"key" if x % 4 == 0 else None,
                             headers=[(b"h%d" % h, None if h == 1 else b"v") for h in range(x % 7 % 4)]))
    return valid_batch("base batch %d" % i, recs)


def _bad_base_batch(i, name):
    """Batch i with the corpus entry `name` behind its good records."""
    good = _base_batch(i)
    rule = [r for r in _remainders() if r[0] == name][0][1]
    return Batch("base batch %d: %s" % (i, name), good.raw + _remainder(name), good.count + 1,
                 (good.count, M.RULE[rule]), None, None)


BASE_VALID = (255, 256, 257, 513, 600)
BASE_BAD = (((0, "key past the record"),), ((255, "value past the record"),), ((256, "key length -2"),),
            ((599, "bytes behind the headers"),),
            ((300, "negative headers count"), (10, "value past the record")),
            ((256, "length 5"), (257, "timestamp delta of eleven bytes"), (599, "record past the batch")))


@functools.lru_cache(maxsize=None)
def base_calls():
    """[Call]: the valid calls, then the 600-batch call with the bad batches of BASE_BAD."""
    good = [_base_batch(i) for i in range(600)]
    out = [Call("%d batches" % n, tuple(good[:n]), None) for n in BASE_VALID]
    for bad in BASE_BAD:
        batches = list(good)
        for i, name in bad:
            batches[i] = _bad_base_batch(i, name)
        first = min(i for i, _ in bad)
        out.append(Call("600 batches, bad at %s" % ", ".join(str(i) for i, _ in bad), tuple(batches),
                        (len(bad), first) + batches[first].expect))
    return tuple(out)


# ---- 5. the gather's edges ---------------------------------------------------------------------

def _call_of_values(name, values, per_batch=128):
    batches = [valid_batch("%s: batch %d" % (name, i // per_batch), [M.Record(v) for v in values[i:i + per_batch]])
               for i in range(0, len(values), per_batch)]
    return Call(name, tuple(batches), None)


def chunk_run(k, d):
    """RUN value lengths that sum to k * CHUNK + d with value boundaries 0, 1 and 15 bytes in
    front of every multiple of CHUNK inside the run (the out_shift residues of OUT_SHIFTS move
    the range's start by as much against the staging chunks)."""
    total = k * CHUNK + d
    marks = sorted({j * CHUNK - m for j in range(1, k + 1) for m in (0, 1, 15)} | {total})
    marks = [m for m in marks if m <= total]
    small = [(3 * i) % 50 for i in range(RUN - len(marks))]        # some of them empty
    lens = small + [marks[0] - sum(small)] + [b - a for a, b in zip(marks, marks[1:])]
    assert len(lens) == RUN and sum(lens) == total and min(lens) >= 0
    return lens


def value_boundaries(call):
    """The value boundaries of a valid call's first run of RUN records, counted from the run's
    start, the run's end included."""
    blob = blob_of(call.batches)
    return M.unframe(blob, M.index(blob)[0])[1][1:RUN + 1]


@functools.lru_cache(maxsize=None)
def gather_calls():
    """[Call], all valid.  gather_calls()[0] is the shared-vector call."""
    out = []
    out.append(_call_of_values("5 bytes per run, the rest empty",
                               [value(i, 5) if i % RUN == 7 else b"" for i in range(4 * RUN)]))
    out.append(_call_of_values("runs 0 and 2 empty or null",
                               [(None if i % 2 else b"") if (i // RUN) % 2 == 0 else value(i, i % 23) for i in range(4 * RUN)]))
    for n in (RUN, RUN + 1, 2 * RUN):
        out.append(_call_of_values("%d records" % n, [value(i, (11 * i) % 37) for i in range(n)]))
    for k in (1, 2):
        for d in (-1, 0, 1):
            lens = chunk_run(k, d) + [(5 * i) % 19 for i in range(RUN)]
            out.append(_call_of_values("a run of %d * CHUNK %+d bytes" % (k, d), [value(i, n) for i, n in enumerate(lens)]))
    out.append(_call_of_values("40000 bytes alone in a run",
                               [value(i, 40000) if i == RUN + 100 else b"" if RUN <= i < 2 * RUN else value(i, i % 9)
                                for i in range(3 * RUN)]))
    return tuple(out)


def chunk_calls():
    return [c for c in gather_calls() if "CHUNK" in c.name]


# ---- the corpus as the native program reads it -----------------------------------------------------

def corpus():
    """Every distinct batch of every part, in a fixed order."""
    out = list(fault_cases()) + list(cut_cases()) + list(window_batches())
    seen = set()
    for call in base_calls() + gather_calls():
        for b in call.batches:
            if (b.name, b.count) not in seen:
                seen.add((b.name, b.count))
                out.append(b)
    return out


def serialize(batches):
    """u32 count, then per batch: u32 name length, the name, u32 recordsCount, u32 bad record, u32
    rule (0: valid), u64 value bytes, u32 null values, keyed, headers (zeros for a bad batch), u32
    record bytes, the record bytes.  Little-endian."""
    parts = [struct.pack("<I", len(batches))]
    for b in batches:
        name = b.name.encode()
        rec, rule = b.expect or (b.count, 0)
        t = b.totals or (0, 0, 0, 0)
        parts += [struct.pack("<I", len(name)), name, struct.pack("<IIIQIIII", b.count, rec, rule, t[0], t[1], t[2], t[3],
                                                                  len(b.raw)), b.raw]
    return b"".join(parts)
