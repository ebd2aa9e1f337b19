"""GPU: the window arithmetic off the 10 s, positive-time path -- bucket = parseLong(t) / d for
runtime divisors from 1 to Long.MAX, rings that straddle bucket 0 or lie below it, negative
window_ms, side-map keys the map cannot express and the ring's auto-base from a negative
first event.  Everything is exact: counts and counters equal the jdiv model
(tests/windows_corpus.py) or the C oracle bit for bit.

The d = 1 runs keep |t| <= 2^62: include/ysb_hip.h (time_divisor_ms) wants every bucket in
(INT64_MIN + W, INT64_MAX - W)."""
import functools

import numpy as np
import pytest

import windows_corpus as wc
from oracle import oracle
from ysb_amd import GenParams, YsbContext

pytestmark = pytest.mark.gpu

COUNTERS = ("events", "views", "joined", "join_misses", "parse_errors", "time_errors")
W = 16
# The corpus has fewer than 1024 lines (asserted on the reference), so at most that many
# distinct out-of-ring cells: the side map (2 * 1024 slots) and the fallback list (1024 entries)
# each hold all of them, whichever of the two a cell goes to.
OVERFLOW = 1024
RING_BASE = -8           # [-8, 8): buckets on both sides of zero live in the ring


def bound_of(d):
    return 1 << 62 if d == 1 else None


def open_ctx(d, fmt="json", **kw):
    kw.setdefault("n_campaigns", 10)
    kw.setdefault("window_ring", W)
    kw.setdefault("overflow_capacity", OVERFLOW)
    kw.setdefault("max_batch_bytes", 1 << 20)
    kw.setdefault("max_batch_events", 1 << 12)
    ctx = YsbContext(time_divisor_ms=d, input_format=fmt, **kw)
    ctx.load_ad_map(*wc.ad_arrays())
    return ctx


def gpu_rows(lines, d, ctx=None, **ctx_kw):
    """One context (or a reset one of the same configuration), one submit, drain() and stats():
    ({(campaign, window_ms): count}, stats, launch_info)."""
    own = ctx is None
    ctx = open_ctx(d, **ctx_kw) if own else ctx
    try:
        if not own:
            ctx.reset()
        raw, offs = wc.batch(lines)
        ctx.submit(raw, offs, slot=0)
        return ctx.drain(), ctx.stats(), ctx.launch_info()
    finally:
        if own:
            ctx.close()


def check_rows(got, recs, d, what):
    """got {(campaign, window_ms): count} against bucket * d from the model; the message names
    the differing cells and the corpus lines that count into them."""
    exp = {(c, b * d): v for (c, b), v in wc.rows_of(recs, d).items()}
    if got == exp:
        return
    diff = sorted(k for k in set(got) | set(exp) if got.get(k) != exp.get(k))
    cells = {(c, wc.jdiv(w, d)) for c, w in diff if w % d == 0}
    msg = ["%s: %d cells differ (campaign, window_ms): gpu / model" % (what, len(diff))]
    msg += ["  %r: %r / %r" % (k, got.get(k), exp.get(k)) for k in diff[:20]]
    msg += ["  line %d: %r" % il for il in wc.lines_of_cells(recs, d, cells)[:20]]
    raise AssertionError("\n".join(msg))


def check_stats(st, recs, d, lo, what):
    for k, v in wc.stats_of(recs).items():
        assert st[k] == v, (what, k, st[k], v)
    assert st["overflow_dropped"] == 0, what
    outside = sum(1 for _, _, t in recs if not lo <= wc.jdiv(t, d) < lo + W)
    assert st["out_of_ring"] == outside, (what, st["out_of_ring"], outside)


# -- a. the boundary corpus -------------------------------------------------------------------

@pytest.mark.parametrize("lds", [True, False])
@pytest.mark.parametrize("d", wc.D)
def test_boundary_corpus(d, lds):
    """Every form of every boundary time, in every layout, at divisor d: one context per input
    format, reset between the JSON layouts."""
    seen = {}
    ctxs = {}
    try:
        for fmt, layout in wc.LAYOUTS:
            recs = wc.records(d, fmt, layout, bound=bound_of(d))
            buckets = {wc.jdiv(t, d) for _, _, t in recs}
            assert 0 in buckets and min(buckets) < 0 and len(recs) < OVERFLOW
            if fmt not in ctxs:
                ctxs[fmt] = open_ctx(d, fmt, lds_count=lds, ring_base_bucket=RING_BASE)
            got, st, info = gpu_rows([r[0] for r in recs], d, ctx=ctxs[fmt])
            what = "d=%d %s/%s lds=%s" % (d, fmt, layout, lds)
            seen[layout] = (info["layout"], info["tbl"], st["deferred"], st["out_of_ring"])
            check_rows(got, recs, d, what)
            check_stats(st, recs, d, RING_BASE, what)
            assert info["tbl"] == (fmt == "tbl") and info["record_mode"] == 0
            assert ctxs[fmt].ring_range() == (RING_BASE, W)
            assert min(w for _, w in got) < 0                  # negative window_ms = bucket * d
    finally:
        for c in ctxs.values():
            c.close()
    print("corpus d=%d lds=%s: layout -> (scan layout, tbl, deferred, out_of_ring) %r" % (d, lds, seen))
    # the scan instantiation the layout sample chose (launch_info: 0 generator, 1 compact,
    # 3 learned key order), so each layout's own tier parsed these times; the lines with an
    # escape in the time string cannot take a fast tier and go to the deferred-line kernel
    assert [seen[k][0] for k in ("generator", "compact", "reordered", "tbl")] == [0, 1, 3, 0]
    assert seen["escape"][2] == len(recs) and all(seen[k][2] == 0 for k in seen if k != "escape")


def test_tbl_fastdiv_guard_both_sides():
    """The .tbl scan's 32-bit shortcut is taken on `P.div.d == 10000` (ysb_scan_flat.h,
    canonical_bucket<true>): the same rows -- the corpora of d = 10000 and d = 10001 together,
    so both divisors' bucket edges in 13 digits -- counted under both divisors."""
    for lds in (True, False):
        for d in (10000, 10001):
            recs = wc.records(10000, "tbl", "tbl") + wc.records(10001, "tbl", "tbl")
            got, st, info = gpu_rows([r[0] for r in recs], d, fmt="tbl", lds_count=lds, ring_base_bucket=170_000_000 - 4)
            what = "tbl d=%d lds=%s" % (d, lds)
            check_rows(got, recs, d, what)
            check_stats(st, recs, d, 170_000_000 - 4, what)
            thirteen = sum(1 for ln, _, _ in recs if len(ln.rstrip(b"\n").split(b"|")[5]) == 13)
            assert info["tbl"] == 1 and thirteen > 40
            print("%s: %d rows, %d with 13 time bytes, deferred %d" % (what, len(recs), thirteen, st["deferred"]))


# -- b. side-map keys the map cannot express ----------------------------------------------------

@pytest.mark.parametrize("base", [0, -8])
@pytest.mark.parametrize("d", [2, 3])
def test_unexpressible_side_map_keys_arrive_exactly(d, base):
    """At 10 campaigns side_add's key holds buckets in [-2^59, 2^59): Long.MAX / d, Long.MIN / d
    and +-2^62 / d lie outside for d = 2 and 3, so their views take the fallback list."""
    for fmt, layout in (("json", "generator"), ("tbl", "tbl")):
        for lds in (True, False):
            recs = wc.records(d, fmt, layout)
            huge = [r for r in recs if abs(wc.jdiv(r[2], d)) >= 1 << 59]
            assert {r[2] for r in huge} >= {wc.LONG_MAX, wc.LONG_MIN, 1 << 62, -(1 << 62)}
            got, st, _ = gpu_rows([r[0] for r in recs], d, fmt=fmt, lds_count=lds, ring_base_bucket=base)
            what = "d=%d %s base=%d lds=%s" % (d, fmt, base, lds)
            check_rows(got, recs, d, what)
            check_stats(st, recs, d, base, what)
            for (c, b), v in wc.rows_of(huge, d).items():
                assert got[(c, b * d)] == v
            assert st["out_of_ring"] >= len(huge) > 0


# -- c. auto-base from a negative first event ----------------------------------------------------

@pytest.mark.parametrize("d,fmt,layout", [(d, "json", "generator") for d in wc.D]
                         + [(d, "tbl", "tbl") for d in (1, 3, 10000, 10001)]
                         + [(1000, "json", "reordered"), (1000, "json", "escape")])
def test_auto_base_from_a_negative_first_event(d, fmt, layout):
    recs = wc.records(d, fmt, layout, bound=bound_of(d), smallest_first=True)
    first = min(wc.jdiv(t, d) for _, _, t in recs[:256])        # every line is a joined view
    assert first < 0 and first == min(wc.jdiv(t, d) for _, _, t in recs)
    with open_ctx(d, fmt) as ctx:
        got, st, _ = gpu_rows([r[0] for r in recs], d, ctx=ctx)
        assert ctx.ring_range() == (first - W // 8, W)
    check_rows(got, recs, d, "auto-base d=%d %s/%s" % (d, fmt, layout))
    check_stats(st, recs, d, first - W // 8, "auto-base d=%d" % d)


# -- d. generated streams against the C oracle -----------------------------------------------------

N_STREAM = 40_000
# events per second of event time: 40,000 events span 10 s (d = 1), 286 ms plus the +-50 ms skew
# (d = 7), 40 s, 400 s and 2000 s: 10,000 / 55 / 40 / 40 / 33 buckets
RATES = {1: 4000, 7: 140_000, 1000: 1000, 10001: 100, 60000: 20}
T0_LATE = 1_700_000_000_000


def t0_straddling(d):
    return max(-20 * d, -600_000)


def stream_gen(d, t0, fmt="json"):
    return GenParams(seed=31 + d % 7, n_campaigns=10, ads_per_campaign=10, t0_ms=t0, events_per_sec=RATES[d],
                     with_skew=2, fmt=fmt)


@functools.lru_cache(maxsize=None)
def stream_case(d, t0, fmt):
    """(generator, host bytes, offsets, oracle rows, oracle stats) -- computed once."""
    g = stream_gen(d, t0, fmt)
    raw, offs = g.events_host(0, N_STREAM)
    rows, st = oracle.run(oracle.AdMap(g.ids()[1], g.ad_campaign_index()), raw, offs, divisor=d, fmt=fmt, threads=8)
    raw.setflags(write=False)
    return g, raw, offs, rows, st


@pytest.mark.parametrize("late", [False, True], ids=["straddle", "t1.7e12"])
@pytest.mark.parametrize("d", sorted(RATES))
def test_generated_streams_vs_oracle(d, late):
    t0 = T0_LATE if late else t0_straddling(d)
    report = []
    for fmt in ("json", "tbl"):
        g, raw, offs, rows, ost = stream_case(d, t0, fmt)
        buckets = {b for _, b in rows}
        assert len(buckets) >= 20 and ost["joined"] > N_STREAM // 4 and ost["parse_errors"] == ost["time_errors"] == 0
        if not late:
            assert min(buckets) < 0 < max(buckets) and 0 in buckets
        exp = {(c, b * d): v for (c, b), v in rows.items()}
        for lds in (True, False):
            for ring in (16, 1024):
                with YsbContext(n_campaigns=10, time_divisor_ms=d, window_ring=ring, lds_count=lds, input_format=fmt,
                                max_batch_bytes=16 << 20, max_batch_events=1 << 16) as ctx:
                    ctx.load_ad_map(g.ids()[1], g.ad_campaign_index())
                    what = "d=%d t0=%d %s lds=%s ring=%d" % (d, t0, fmt, lds, ring)
                    # host submit
                    ctx.submit(raw, offs)
                    got, st = ctx.drain(), ctx.stats()
                    lo, _ = ctx.ring_range()
                    inside = sum(v for (c, b), v in rows.items() if lo <= b < lo + ring)
                    info = ctx.launch_info()
                    report.append((what, "host", info["layout"], st["deferred"], st["out_of_ring"]))
                    assert got == exp, what
                    for k in COUNTERS:
                        assert st[k] == ost[k], (what, k, st[k], ost[k])
                    assert st["overflow_dropped"] == 0 and st["out_of_ring"] == ost["joined"] - inside, what
                    if late:
                        # 13-digit times: every generator line has the fast tiers' length (JSON:
                        # ysb_scan_canon.h CanonGeo::MINLEN / MAXLEN, line 109 and 122; .tbl: the
                        # MINLEN of line 333 and `c.tlen = 13`, line 417), as at d = 10000
                        assert st["deferred"] == 0, what
                    # device generator + submit_device, and the generator truth
                    ctx.reset()
                    cap = N_STREAM * g.max_line_bytes()
                    d_b, d_o = ctx.device_alloc(cap), ctx.device_alloc(4 * N_STREAM)
                    nb = ctx.gen_events_device(g, 0, N_STREAM, d_b, cap, d_o)
                    assert nb == raw.size
                    assert np.array_equal(ctx.d2h(np.empty(nb, dtype=np.uint8), d_b), raw)
                    ctx.submit_device(d_b, nb, d_o, N_STREAM)
                    ctx.sync()
                    ctx.truth_accumulate(g, 0, N_STREAM)
                    mism, truth, in_ring = ctx.truth_compare()
                    got, st = ctx.drain(), ctx.stats()
                    report.append((what, "device", ctx.launch_info()["layout"], st["deferred"], st["out_of_ring"]))
                    assert ctx.ring_range() == (lo, ring)
                    assert got == exp, what
                    for k in COUNTERS:
                        assert st[k] == ost[k], (what, k, st[k], ost[k])
                    # truth_total counts every view of the generator, ring_total the ring's cells:
                    # equal to the oracle's joined where the ring holds every bucket
                    assert mism == 0 and truth == ost["joined"] and in_ring == inside, (what, mism, truth, in_ring)
                    if len(buckets) < ring * 3 // 4 and ring == 1024:
                        assert truth == in_ring == ost["joined"], what
                    ctx.device_free(d_b)
                    ctx.device_free(d_o)
    for r in report:
        print("stream %s %s: layout %d deferred %d out_of_ring %d" % r)


# -- e. ring position ----------------------------------------------------------------------------

@pytest.mark.parametrize("base", [-64, -32, -1, 0, -37])
def test_ring_position_and_drain_ranges(base):
    d, ring = 1000, 64
    g, raw, offs, rows, ost = stream_case(d, t0_straddling(d), "json")
    exp = {(c, b * d): v for (c, b), v in rows.items()}
    lo_b, hi_b = min(b for _, b in rows), max(b for _, b in rows)
    assert lo_b < -5 and hi_b > 5
    k = max(-lo_b, hi_b) + 1

    def part(lo, hi):
        return {(c, b * d): v for (c, b), v in rows.items() if lo <= b < hi}
    with YsbContext(n_campaigns=10, time_divisor_ms=d, window_ring=ring, ring_base_bucket=base,
                    max_batch_bytes=16 << 20, max_batch_events=1 << 16) as ctx:
        ctx.load_ad_map(g.ids()[1], g.ad_campaign_index())
        ctx.submit(raw, offs)
        assert ctx.ring_range() == (base, ring)
        inside = sum(v for (c, b), v in rows.items() if base <= b < base + ring)
        assert ctx.stats()["out_of_ring"] == ost["joined"] - inside
        # [-k, 0) and [0, k) partition the full drain
        full = ctx.drain()
        neg, pos = ctx.drain(bucket_lo=-k, bucket_hi=0), ctx.drain(bucket_lo=0, bucket_hi=k)
        assert full == exp and neg == part(-k, 0) and pos == part(0, k)
        assert not set(neg) & set(pos) and len(neg) + len(pos) == len(full)
        # a clearing drain of a negative range, then the rest exactly once
        first = ctx.drain(bucket_lo=-7, bucket_hi=-2, clear=True)
        assert first == part(-7, -2) and len(first) > 0
        rest = ctx.drain(clear=True)
        assert rest == {c: v for c, v in exp.items() if c not in first}
        assert ctx.drain() == {}
        # an asynchronous flush of [-5, 5) -- the ring's part of it -- and a later drain sum to
        # the oracle, each cell in exactly one of the two
        ctx.submit(raw, offs, slot=1)
        ctx.flush_begin(-5, 5)
        flushed, more = ctx.flush_end(wait=True)
        assert not more and flushed == part(max(-5, base), min(5, base + ring)) and len(flushed) > 0
        later = ctx.drain(clear=True)
        assert later == {c: v for c, v in exp.items() if c not in flushed}


def test_ring_advance_across_zero_and_back():
    d, ring = 1000, 16
    g, raw, offs, rows, _ = stream_case(d, t0_straddling(d), "json")
    cuts = [0, N_STREAM // 3, 2 * N_STREAM // 3, N_STREAM]
    ends = list(offs) + [raw.size]

    def piece(i):
        a, b = cuts[i], cuts[i + 1]
        return raw[ends[a]:ends[b]], offs[a:b] - offs[a]
    am = oracle.AdMap(g.ids()[1], g.ad_campaign_index())
    again, _ = oracle.run(am, *piece(0), divisor=d)
    with YsbContext(n_campaigns=10, time_divisor_ms=d, window_ring=ring, ring_base_bucket=-30,
                    max_batch_bytes=16 << 20, max_batch_events=1 << 16) as ctx:
        ctx.load_ad_map(g.ids()[1], g.ad_campaign_index())
        ctx.submit(*piece(0))
        ctx.ring_advance(-5)                      # up: the ring straddles zero
        assert ctx.ring_range() == (-5, ring)
        ctx.submit(*piece(1), slot=1)
        ctx.ring_advance(3)                       # up across zero
        assert ctx.ring_range() == (3, ring)
        ctx.submit(*piece(2))
        assert ctx.drain_buckets() == rows
        ctx.ring_advance(-20)                     # and back down across zero
        assert ctx.ring_range() == (-20, ring)
        assert ctx.drain_buckets() == rows
        ctx.submit(*piece(0), slot=1)
        total = dict(rows)
        for c, v in again.items():
            total[c] = total.get(c, 0) + v
        assert ctx.drain() == {(c, b * d): v for (c, b), v in total.items()}
        assert ctx.stats()["overflow_dropped"] == 0


# -- f. record mode ------------------------------------------------------------------------------

@pytest.mark.timeout(300)
def test_record_mode_with_negative_buckets():
    """The map and event counts of tests/test_gpu_records.py's big_map (the smallest shape with
    the bucket-layout table), from t0 = -15 s at d = 1000 with a 16-bucket ring: records,
    rec_fallback and the out-of-ring views all see negative buckets."""
    d = 1000
    g = GenParams(seed=11, n_campaigns=200_000, ads_per_campaign=2, events_per_sec=1000, with_skew=True,
                  t0_ms=-15_000)
    _, aids = g.ids()
    camp = g.ad_campaign_index()
    raw, offs = g.events_host(0, 300_000)
    rows, ost = oracle.run(oracle.AdMap(aids, camp), raw, offs, divisor=d, threads=8)
    exp = {(c, b * d): v for (c, b), v in rows.items()}
    assert min(b for _, b in rows) <= -15 and max(b for _, b in rows) > 200
    for record in (True, False):
        with YsbContext(n_campaigns=200_000, time_divisor_ms=d, window_ring=16, record_count=record,
                        max_batch_bytes=raw.size + 64, max_batch_events=offs.size + 1) as ctx:
            ctx.load_ad_map(aids, camp)
            ctx.submit(raw, offs)
            got, st = ctx.drain(), ctx.stats()
            lo, _ = ctx.ring_range()
            nrec = ctx.path_time()[2]
            info = ctx.launch_info()
        print("record=%s: ring_lo %d record launches %d launch_info %r deferred %d out_of_ring %d"
              % (record, lo, nrec, info, st["deferred"], st["out_of_ring"]))
        assert nrec == (1 if record else 0)
        assert lo < 0 and st["out_of_ring"] > 0 and st["overflow_dropped"] == 0
        assert got == exp
        for k in COUNTERS:
            assert st[k] == ost[k], (record, k, st[k], ost[k])
