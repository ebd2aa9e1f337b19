"""GPU: Kafka record batches unframed on the device (csrc/ysb_kafka.hip) -- the unframing alone
(ysb_kafka_unframe_device) against the host model and the pure-Python model over record shapes,
batch sizes and the walk's window edges; counts through the slots (ysb_submit_kafka,
ysb_submit_kafka_mapped) against ysb_submit of the same lines on the same configuration;
malformed input (the corpus the sanitized native program has walked); capacity and growth."""
import numpy as np
import pytest

import golden_data as gd
import kafka_model as M
from test_gpu_mapped import aligned, ctx_for
from test_gpu_parity import make_ctx
from ysb_amd import GenParams, YsbError, kafka

pytestmark = pytest.mark.gpu

SLOT = 8 << 20   # max_batch_bytes of the tests' contexts (the pinned slots are allocated whole)


@pytest.fixture(scope="module")
def ctx():
    with make_ctx(max_batch_bytes=SLOT, timing=True) as c:
        yield c


def unframe_device(c, blob, idx, out_shift=3, nval=None):
    """blob in a device allocation of its exact size (so the last batch ends at the allocation's
    last byte), unframed to an output that starts at an odd address: (values, offsets, info).
    The bytes in front of the output and the spare byte behind it are pre-filled and must stay."""
    blob = np.frombuffer(bytes(blob), dtype=np.uint8)
    nrec = int(idx["n_records"].sum()) if idx.size else 0
    if nval is None:
        nval = kafka.unframe_host(blob, idx, sizes_only=True)[2]["value_bytes"]
    d_in = c.device_alloc(max(blob.size, 1))
    d_out = c.device_alloc(nval + out_shift + 1)
    d_off = c.device_alloc(4 * (nrec + 1))
    try:
        if blob.size:
            c.h2d(d_in, blob)
        c.h2d(d_out, np.full(nval + out_shift + 1, 0xA5, dtype=np.uint8))
        n, nb = c.kafka_unframe_device(d_in, blob.size, idx, d_out + out_shift, nval, d_off, nrec + 1)
        assert (n, nb) == (nrec, nval)
        whole = c.d2h(np.empty(nval + out_shift + 1, dtype=np.uint8), d_out)
        assert (whole[:out_shift] == 0xA5).all(), "bytes in front of the output were written"
        assert whole[out_shift + nval] == 0xA5, "the byte behind the output was written"
        out = whole[out_shift:out_shift + nval]
        off = c.d2h(np.empty(nrec + 1, dtype=np.uint32), d_off)
        return out, off, c.kafka_info()
    finally:
        for p in (d_in, d_out, d_off):
            c.device_free(p)


def check_device(c, blob, expect_records=None):
    idx, info = kafka.index(blob, check_crc=True)
    assert info["consumed"] == len(blob)
    want, woff, wct = kafka.unframe_host(blob, idx)
    mout, moff, mct = M.unframe(blob, M.index(blob)[0])
    assert want.tobytes() == mout and list(woff) == moff and wct == mct
    out, off, ki = unframe_device(c, blob, idx)
    assert out.tobytes() == mout, "value bytes differ"
    assert list(off) == moff, "offsets differ"
    for k in ("records", "null_values", "keyed", "headers", "value_bytes"):
        assert ki[k] == wct[k], k
    assert ki["batches"] == idx.size and ki["framed_bytes"] == len(blob) and ki["verdict"]["first_bad"] is None
    if expect_records is not None:
        assert ki["records"] == expect_records
    return ki


def value(i, n):
    return bytes((i * 7 + j) % 251 for j in range(n))


# ---- 1. the unframing alone against the models -------------------------------------------------

def test_record_shapes(ctx):
    """Value lengths that make `length` 1, 2 and 3 bytes, null and empty values, a 5 KB value
    across several windows; keys null / empty / 1 / 36 / 300 bytes; 0, 1 and 3 headers with a null
    value; negative and 10-byte timestamp deltas; offset-delta gaps; non-minimal varints."""
    recs = []
    for i, vlen in enumerate((20, 254, 9000, 0, None, 5000)):
        for key in (None, b"", b"k", b"u" * 36, b"K" * 300):
            for headers in ((), ((b"a", b"1"),), ((b"a", b"1"), (b"b", None), (b"", b""))):
                recs.append(M.Record(None if vlen is None else value(len(recs), vlen), key=key, headers=headers,
                                     ts_delta=(-1, -2**63, 2**62, 5)[len(recs) % 4], offset_delta=3 * len(recs),
                                     pad=1 if len(recs) % 4 in (0, 3) else 0,   # (a padded 10-byte delta would be illegal)
                                     length_pad=(len(recs) // 2) % 2))
    blob = b"".join(M.pack_batch(recs[i:i + 7], base_offset=i) for i in range(0, len(recs), 7))
    ki = check_device(ctx, blob, 90)
    assert ki["null_values"] == 15 and ki["walk_ms"] > 0 and ki["gather_ms"] > 0


@pytest.mark.parametrize("per_batch", [1, 63, 64, 65, 129])
def test_batch_sizes(ctx, per_batch):
    """Batches of 1, 63, 64, 65 and 129 records (the walk parses 64 bodies at a time; the gather
    takes 256 records per workgroup), values of every length 0..299 and every alignment."""
    vals = [value(i, i % 300) for i in range(per_batch * 5)]
    check_device(ctx, M.pack(vals, per_batch, key=b"k"), len(vals))


def record_spanning(total, seed):
    """A record (no key, no headers) whose `length` and body take exactly `total` bytes."""
    n = total - 16
    for _ in range(3):
        r = M.Record(value(seed, n))
        span = len(M.varint(len(r.body(0)))) + len(r.body(0))
        if span == total:
            return r
        n += total - span
    raise AssertionError("no record of %d bytes" % total)


def test_window_edges(ctx):
    """A record header and a value boundary at each offset in -2 .. +2 around the walk's window
    edges (the first, the ring's wrap at the second, the third), the window's size from
    ysb_kafka_info.  A window starts on the 16-byte boundary in front of the batch's first record."""
    W = ctx.kafka_info()["window_bytes"]
    assert W >= 64 and W % 16 == 0
    mis = M.HEADER % 16          # the device allocation is 16-byte aligned and holds one batch
    klen = 40
    r1 = M.Record(value(2, 300), key=b"q" * klen)
    lead = 2 + 1 + 1 + 1 + 1 + klen + 2     # r1's length, attributes, two deltas, key length, key, value length
    body = r1.body(1)
    assert len(M.varint(len(body))) == 2 and body[lead - 2:lead - 2 + 300] == r1.value
    for edge in (W, 2 * W, 3 * W):
        for d in range(-2, 3):
            target = edge - mis + d          # in record bytes from the batch's first
            # (a) the second record's header at target
            check_device(ctx, M.pack_batch([record_spanning(target, d), M.Record(b"second", key=b"k2"),
                                            M.Record(value(1, 700))]), 3)
            # (b) the second record's value starting at target
            check_device(ctx, M.pack_batch([record_spanning(target - lead, d), r1, M.Record(b"third")]), 3)


def test_many_small_batches_and_empty(ctx):
    """300 one-record batches; an empty index; a batch of no records."""
    check_device(ctx, M.pack([value(i, 30 + i % 7) for i in range(300)], 1), 300)
    idx = np.zeros(0, dtype=kafka.BATCH)
    out, off, ki = unframe_device(ctx, b"", idx)
    assert out.size == 0 and list(off) == [0] and ki["records"] == 0 and ki["batches"] == 0
    check_device(ctx, M.pack_batch([]) + M.pack_batch([M.Record(b"x")]), 1)


def test_large_values_cross_gather_chunks(ctx):
    """600 records of up to 9000 bytes: several gather workgroups, each with several LDS chunks."""
    vals = [value(i, (9000, 3, 4097, 0, 16384 + i % 5)[i % 5]) for i in range(600)]
    check_device(ctx, M.pack(vals, 129), 600)


# ---- 2. counts through the slots ----------------------------------------------------------------

def fixture_lines(stem, strip=False):
    raw, offs = gd.events(stem)
    ends = list(offs[1:]) + [len(raw)]
    lines = [raw[a:b] for a, b in zip(offs, ends)]
    if strip:
        lines = [l.rstrip(b"\r\n") for l in lines]
    data = b"".join(lines)
    off = np.cumsum([0] + [len(l) for l in lines[:-1]]).astype(np.uint32)
    return data, off, lines


def counts_and_stats(c):
    """The counts and every stat but `deferred`: which tier took a line follows the layout sample
    (ysb_submit samples 64 lines spread over the batch by their offsets, a Kafka batch the first
    batch's first values), and counts never depend on it."""
    c.sync()
    return c.drain_buckets(), {k: v for k, v in c.stats().items() if k != "deferred"}


@pytest.mark.parametrize("stem,strip", [("gen_s7", False), ("edge", False), ("edge_orgjson", False), ("edge_long", False),
                                        ("gen_s7", True)])
def test_slot_counts_equal_ysb_submit(stem, strip):
    """submit_kafka and submit_kafka_mapped (from an odd byte address, alternating slots) give
    exactly the counts and stats of ysb_submit with the same lines and offsets on the same
    configuration; gen_s7 with its terminators stripped also equals gen_s7.expected.csv."""
    data, off, lines = fixture_lines(stem, strip)
    blob = M.pack(lines, 37, key=b"k", headers=[(b"h", None)])
    idx, _ = kafka.index(blob, check_crc=True)
    with make_ctx(max_batch_bytes=SLOT) as ref:
        ref.submit(data, off)
        want = counts_and_stats(ref)
    if strip:
        rows, st = gd.expected("gen_s7")
        assert want[0] == rows and all(want[1][k] == v for k, v in st.items())
    with make_ctx(max_batch_bytes=SLOT) as a:
        a.submit_kafka(blob, idx)
        got = counts_and_stats(a)
        assert got == want
        ki = a.kafka_info()
        assert ki["records"] == len(lines) and ki["batches"] == idx.size and ki["framed_bytes"] == len(blob)
    # the same bytes in runs of whole batches, mapped at odd addresses, slots alternating: the
    # reference takes the same runs of lines through ysb_submit, one submit each
    cuts = [0, 1, idx.size // 3, idx.size // 2, idx.size]
    cuts = sorted(set(cuts))
    buf = aligned(len(blob) + 64 * len(cuts))
    runs, pos = [], 0
    for i, (x, y) in enumerate(zip(cuts[:-1], cuts[1:])):
        pos += (2 * i + 1 - pos) % 16
        b0 = int(idx[x]["records_off"]) - M.HEADER
        b1 = int(idx[y - 1]["records_off"]) + int(idx[y - 1]["records_bytes"])
        buf[pos:pos + b1 - b0] = np.frombuffer(blob[b0:b1], dtype=np.uint8)
        sub = idx[x:y].copy()
        sub["records_off"] -= b0
        sub["first_record"] -= sub["first_record"][0]
        runs.append((pos, b1 - b0, sub, int(idx[x]["first_record"]), int(sub["n_records"].sum())))
        pos += b1 - b0
    assert all(p % 2 == 1 for p, _, _, _, _ in runs)
    with make_ctx(max_batch_bytes=SLOT) as ref, make_ctx(max_batch_bytes=SLOT) as m:
        ends = np.append(off[1:], len(data)).astype(np.int64)
        for i, (_, _, _, first, n) in enumerate(runs):
            a0, a1 = int(off[first]), int(ends[first + n - 1])
            ref.submit(data[a0:a1], off[first:first + n] - a0, slot=i % 2)
        want_runs = counts_and_stats(ref)
        m.host_register(buf)
        for i, (p, nb, sub, _, _) in enumerate(runs):
            m.submit_kafka_mapped(buf, p, nb, sub, slot=i % 2)
        got = counts_and_stats(m)
        m.host_unregister(buf)
    assert got == want_runs and got[0] == want[0]


def test_kafka_between_raw_batches_keeps_order():
    """raw, Kafka, raw in alternating slots: the three batches launch in submission order and
    count like the same three through ysb_submit_raw alone."""
    g = GenParams(events_per_sec=100_000, with_skew=2)
    data, off = g.events_host(0, 6000)
    ends = np.append(off[1:], len(data)).astype(np.int64)
    parts = [(0, 2000), (2000, 4000), (4000, 6000)]
    chunk = [bytes(data[int(off[a]):int(ends[b - 1])]) for a, b in parts]
    mid_lines = [bytes(data[int(off[i]):int(ends[i])]) for i in range(2000, 4000)]
    blob = kafka.pack(chunk[1], off[2000:4000] - off[2000], batch_bytes=16384)
    assert M.unframe(blob.tobytes(), M.index(blob.tobytes())[0])[0] == b"".join(mid_lines)
    idx, _ = kafka.index(blob)
    with ctx_for(g, max_batch_bytes=SLOT) as ref, ctx_for(g, max_batch_bytes=SLOT) as c:
        for i in range(3):
            ref.submit_raw(chunk[i], slot=i % 2)
        want = counts_and_stats(ref)
        c.submit_raw(chunk[0], slot=0)
        c.submit_kafka(blob, idx, slot=1)
        c.submit_raw(chunk[2], slot=0)
        assert counts_and_stats(c) == want and want[1]["events"] == 6000
        c.truth_accumulate(g, 0, 6000)
        mism, truth, ring = c.truth_compare()
        assert mism == 0 and truth == ring > 0


# ---- 3. malformed input -------------------------------------------------------------------------

def test_malformed_verdicts_equal_the_model(ctx):
    """Every case of the corpus that the sanitized native program has walked, a good batch in front
    and behind: the device's verdict (batch, record, rule) is the model's, nothing is written."""
    front, back = M.pack_batch([M.Record(b"ok")]), M.pack_batch([M.Record(b"after")], base_offset=9)
    for name, rule, count, rec in M.malformed_corpus():
        blob = front + M.pack_batch(None, base_offset=1, records_count=count, raw_records=rec) + back
        idx, _ = kafka.index(blob, check_crc=True)
        want = M.verdict(blob, M.index(blob)[0])
        assert want is not None and want[0] == 1 and want[2] == M.RULE[rule], name
        assert kafka.verdict(blob, idx)["record"] == want[1]
        with pytest.raises(YsbError) as e:
            unframe_device(ctx, blob, idx, nval=len(blob))
        assert e.value.code == -5 and "ysb_kafka_unframe_device: Kafka batch 1 (baseOffset 1), record %d" % want[1] in str(e.value), (name, str(e.value))
        v = ctx.kafka_info()["verdict"]
        assert (v["bad_batches"], v["first_bad"], v["record"], v["rule"]) == (1,) + want, (name, v, want)


def test_bad_batch_drops_the_slot_batch_until_reset():
    """A bad Kafka batch in a slot batch: nothing of it is counted, YSB_ERR_FORMAT names the Kafka
    batch and the record, the error is sticky until ysb_reset, and a good batch counts exactly
    afterwards."""
    data, off, lines = fixture_lines("gen_s7")
    good = M.pack(lines, 50)
    gidx, _ = kafka.index(good)
    name, rule, count, rec = M.malformed_corpus()[8]
    bad = M.pack(lines[:100], 50) + M.pack_batch(None, base_offset=100, records_count=count, raw_records=rec)
    bidx, _ = kafka.index(bad, check_crc=True)
    want = M.verdict(bad, M.index(bad)[0])
    assert want[0] == 2
    rows, st = gd.expected("gen_s7")
    with make_ctx(max_batch_bytes=SLOT) as c:
        c.submit_kafka(bad, bidx, slot=0)
        with pytest.raises(YsbError) as e:
            c.sync()
        assert e.value.code == -5 and "Kafka batch 2 (baseOffset 100), record %d" % want[1] in str(e.value), str(e.value)
        with pytest.raises(YsbError) as e2:
            c.submit_kafka(good, gidx, slot=1)
        assert e2.value.code == -5 and "Kafka batch 2" in str(e2.value)
        v = c.kafka_info(check=False)["verdict"]
        assert (v["first_bad"], v["record"], v["rule"]) == want
        c.reset()
        assert c.stats()["events"] == 0
        c.submit_kafka(good, gidx, slot=1)
        c.sync()
        got = c.drain_buckets()
        assert got == rows and all(c.stats()[k] == x for k, x in st.items())


# ---- 4. capacity and growth ---------------------------------------------------------------------

def test_too_many_records_is_a_capacity_error_at_the_submit():
    vals = [b"{}"] * 3000
    blob = M.pack(vals, 500)
    idx, _ = kafka.index(blob)
    with make_ctx(max_batch_bytes=64 << 10, max_batch_events=16) as c:      # 2048 lines per slot
        with pytest.raises(YsbError) as e:
            c.submit_kafka(blob, idx)
        assert e.value.code == -4 and "3000 records" in str(e.value)
        with pytest.raises(YsbError) as e:
            c.submit_kafka(blob + bytes(70 << 10), idx)
        assert e.value.code == -4
        c.submit_kafka(blob[:int(idx[3]["records_off"]) - M.HEADER], idx[:3])   # 1500 records fit
        c.sync()
        assert c.stats()["events"] == 1500


def test_staging_grows_with_the_index_and_the_records():
    """A small batch, then 2000 one-record Kafka batches (the pinned index grows), then 20000
    records (the device scratch grows): every batch exact against ysb_submit_raw."""
    g = GenParams(events_per_sec=100_000, with_skew=2)
    data, off = g.events_host(0, 22_100)
    ends = np.append(off[1:], len(data)).astype(np.int64)
    parts = [(0, 100, 50), (100, 2100, 1), (2100, 22_100, 500)]
    with ctx_for(g, max_batch_bytes=SLOT) as ref, ctx_for(g, max_batch_bytes=SLOT) as c:
        for i, (a, b, per) in enumerate(parts):
            chunk = data[int(off[a]):int(ends[b - 1])]
            ref.submit_raw(chunk, slot=i % 2)
            blob = kafka.pack(chunk, off[a:b] - off[a], batch_bytes=0, batch_records=per)
            idx, _ = kafka.index(blob)
            assert idx.size == (b - a + per - 1) // per
            c.submit_kafka(blob, idx, slot=i % 2)
        assert counts_and_stats(c) == counts_and_stats(ref)
        c.truth_accumulate(g, 0, 22_100)
        mism, truth, ring = c.truth_compare()
        assert mism == 0 and truth == ring > 0
