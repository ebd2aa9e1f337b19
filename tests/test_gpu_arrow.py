"""GPU: the Arrow count (ysb_submit_arrow_device / ysb_submit_arrow) against its CPU model
(tests/arrow_model.py), the committed pyarrow buffers, and -- where the rows have a JSON form --
ysb_submit of their JSON rendering in a second context.  No pyarrow needed.  Device buffers are
uploaded one by one, each at an odd address inside its own allocation, so every pointer the
kernel gets is unaligned."""
import numpy as np
import pytest

import arrow_model as am
import golden_data as gd
import windows_corpus as wc
from oracle import dostats
from ysb_amd import YsbContext, YsbError, arrow

pytestmark = pytest.mark.gpu

SMALL = dict(window_ring=16, max_batch_events=1 << 12, max_batch_bytes=1 << 20, overflow_capacity=1 << 10)
EIGHT = am.STATS


class Dev:
    """Device copies of a batch's buffers, freed together.  misalign: each buffer's first byte sits
    that many bytes past its allocation's (16-byte aligned) start."""

    def __init__(self, c, misalign=1):
        self.c, self.ptrs, self.mis = c, [], misalign

    def put(self, a):
        a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        d = self.c.device_alloc(a.size + self.mis + 16)
        self.ptrs.append(d)
        pad = np.concatenate([np.full(self.mis, 0xA5, dtype=np.uint8), a, np.full(16, 0xA5, dtype=np.uint8)])
        self.c.h2d(d, pad)
        return d + self.mis

    def free(self):
        for p in self.ptrs:
            self.c.device_free(p)
        self.ptrs = []


def run_device(c, b, misalign=1):
    dev = Dev(c, misalign)
    try:
        c.submit_arrow_device(am.to_cols(b, dev.put))
        got, st = c.drain_buckets(), c.stats()
    finally:
        dev.free()
    return got, st


def run_host(c, b, slot=0):
    c.submit_arrow(am.to_node(b), slot=slot)
    return c.drain_buckets(), c.stats()


def assert_model(got, st, want, wst, batches=1):
    assert got == want
    for k in EIGHT:
        assert st[k] == wst[k], (k, st[k], wst[k])
    assert st["batches"] == batches and st["overflow_dropped"] == 0


def assert_json(c2, b, want, wst):
    """The rows' JSON rendering through ysb_submit in a second context gives the same counts; the
    rows without a JSON form are left out of this comparison only."""
    lines, formless = am.render_json(b)
    raw = b"".join(lines)
    offs = np.cumsum([0] + [len(x) for x in lines[:-1]]).astype(np.uint32) if lines else np.zeros(0, dtype=np.uint32)
    c2.reset()
    if lines:
        c2.submit(np.frombuffer(raw, dtype=np.uint8), offs)
    got, st = c2.drain_buckets(), c2.stats()
    assert got == want
    for k in ("views", "joined", "join_misses", "time_errors", "foreign_shard"):
        assert st[k] == wst[k], (k, st[k], wst[k])
    assert st["events"] == wst["events"] - formless and st["parse_errors"] == wst["parse_errors"] - formless


@pytest.fixture(scope="module")
def world():
    class W:
        pass
    w = W()
    w.ads, w.camp = gd.ad_arrays()
    w.keys = [a.encode() for a in w.ads]
    w.map = dict(zip(w.keys, w.camp))
    w.full = am.fixture("gen_s7_strings")
    w.rows = [am.row(w.full, i)[1] for i in range(w.full.n_rows)]   # (ad, type, time) bytes
    w.t_in = int(w.rows[0][2])
    return w


@pytest.fixture(scope="module")
def ctx(world):
    with YsbContext(n_campaigns=100, **SMALL) as c:
        c.load_ad_map(world.ads, world.camp)
        yield c


@pytest.fixture(scope="module")
def ctx_json(world):
    with YsbContext(n_campaigns=100, **SMALL) as c:
        c.load_ad_map(world.ads, world.camp)
        yield c


@pytest.fixture(scope="module")
def cctx():
    """The hand-made corpus's map (keys of 0, 35, 36, 37 and 56 bytes), and its JSON twin."""
    m = am.corpus_map()
    with YsbContext(n_campaigns=10, **SMALL) as c, YsbContext(n_campaigns=10, **SMALL) as c2:
        for x in (c, c2):
            x.load_ad_map(list(m), list(m.values()))
        yield c, c2, m


encode = am.encode


# ---- the committed pyarrow buffers ----------------------------------------------------------------

@pytest.mark.parametrize("name", am.FIXTURES)
def test_fixtures(ctx, ctx_json, world, name):
    b = am.fixture(name)
    want, wst = am.count(b, world.map)
    if name.startswith("gen_s7") and "slice" not in name:
        assert want == gd.expected("gen_s7")[0] and wst["views"] == 506
    for form in (run_device, run_host):
        ctx.reset()
        got, st = form(ctx, b)
        assert_model(got, st, want, wst)
        info = ctx.arrow_launch_info()
        assert info["rows"] == b.n_rows and info["per_lane_tiles"] == 0 and info["lds_counters"] == 1
        assert info["kind"] == (1, b.typ.kind, b.time.kind) and info["invalid_null"] == wst["parse_errors"]
    assert_json(ctx_json, b, want, wst)


# ---- small shapes ------------------------------------------------------------------------------------

@pytest.mark.parametrize("off", [0, 1, 7, 64, 67])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129])
def test_small_shapes(ctx, world, n, off):
    """Every buffer is over-allocated and filled on both sides of the rows with countable views of
    a known ad: a read outside the rows shows as extra counts."""
    filler = (world.keys[0], b"view", str(world.t_in).encode())
    for kind in ("strings", "int64", "dict"):
        b = encode(world.rows[100:100 + n], kind, lead=off, tail=70, filler=filler, bitmaps=(off % 2 == 1))
        want, wst = am.count(b, world.map)
        assert wst["events"] == n
        for form in (run_device, run_host):
            ctx.reset()
            got, st = form(ctx, b)
            assert_model(got, st, want, wst)
        if n:
            assert ctx.arrow_launch_info()["tiles"] == (n + 63) // 64


# ---- the hand-made corpus ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["plain", "int64", "nulls", "dict", "offsets"])
def test_corpus(cctx, name):
    c, c2, m = cctx
    b = am.corpus()[name]
    inv = {}
    want, wst = am.count(b, m, invalid=inv)
    forms = (run_device,) if name == "offsets" else (run_device, run_host)   # (lying offsets: no ArrowArray says data_bytes)
    for form in forms:
        c.reset()
        got, st = form(c, b)
        assert_model(got, st, want, wst)
        info = c.arrow_launch_info()
        assert (info["invalid_null"], info["invalid_offsets"], info["invalid_dict"]) == (inv["null"], inv["offsets"], inv["dict"])
    assert_json(c2, b, want, wst)


def test_lying_offsets_are_not_followed(ctx, world):
    """Each lying offset points inside the test's own over-allocated buffer but beyond the stated
    data_bytes, at bytes that would count: the rows are invalid and nothing else moves."""
    k = 70
    rows = [(world.keys[i % 50], b"view", str(world.t_in + i).encode()) for i in range(k)]
    good = encode(rows, "strings")
    bad = encode(rows, "strings")
    extra = np.frombuffer(world.keys[0] * 8, dtype=np.uint8)
    end = bad.ad.data_bytes
    bad.ad = am.Col(am.STRING, np.array(bad.ad.offsets), np.concatenate([bad.ad.data, extra]), data_bytes=end)
    bad.ad.offsets[k] = end + 36           # the last row ends past data_bytes
    bad.ad.offsets[5] = end + 72           # row 4 ends past it, row 5 starts there and runs backwards
    want, wst = am.count(bad, world.map)
    gwant, gst = am.count(good, world.map)
    assert wst["parse_errors"] == 3 and gst["parse_errors"] == 0 and wst["views"] == gst["views"] - 3
    ctx.reset()
    got, st = run_device(ctx, bad)
    assert_model(got, st, want, wst)
    info = ctx.arrow_launch_info()
    assert info["invalid_offsets"] == 3 and info["per_lane_tiles"] == 2


# ---- tile content ---------------------------------------------------------------------------------------------

def test_tile_content(ctx, ctx_json, world):
    t = str(world.t_in).encode()
    long_id = [(b"L" * 200, b"view", t)] * 64                              # one tile of 200-byte ids: per-lane
    # 63 x 48 + 36 = 3060 bytes of ids, just under the cap of 3072 - 7: staged
    mixed = [(world.keys[i % 50] + b"x" * 12, b"view", t) for i in range(63)] + [(world.keys[3], b"view", t)]
    over = [(world.keys[i % 50] + b"x" * 12, b"view", t) for i in range(64)]   # 3072: per-lane
    nonviews = [(world.keys[i % 50], b"click", t) for i in range(64)]
    for rows, lane_tiles in ((long_id, 1), (mixed, 0), (over, 1), (nonviews, 0), (long_id + mixed + nonviews, 1)):
        b = encode(rows, "strings")
        want, wst = am.count(b, world.map)
        ctx.reset()
        got, st = run_device(ctx, b)
        assert_model(got, st, want, wst)
        assert ctx.arrow_launch_info()["per_lane_tiles"] == lane_tiles
    assert wst["views"] == 128 and wst["joined"] == 1
    b = encode(mixed, "strings", bitmaps=True)
    b.validity = am.bitmap([False] * 64)                                   # an all-null tile
    want, wst = am.count(b, world.map)
    assert wst["parse_errors"] == 64
    ctx.reset()
    got, st = run_device(ctx, b)
    assert_model(got, st, want, wst)
    assert_json(ctx_json, b, want, wst)


# ---- wrap: every workgroup takes several tiles ---------------------------------------------------------------------

def test_wrap(world):
    """64 * (3 * resident_grid + 1) + 5 rows: mixed hits, misses, out-of-ring times and a moving
    LDS window, against the model."""
    with YsbContext(n_campaigns=100, window_ring=16, max_batch_events=1 << 12, max_batch_bytes=1 << 20,
                    overflow_capacity=1 << 12, ring_base_bucket=world.t_in // 10000) as c:
        c.load_ad_map(world.ads, world.camp)
        run_device(c, encode(world.rows[:1], "strings"))
        res = c.arrow_launch_info()["resident_grid"]
        n = 64 * (3 * res + 1) + 5
        assert n < 400_000 * max(1, res // 2048)
        rng = np.random.default_rng(5)
        ad_i = rng.integers(0, len(world.keys) + 7, n)                     # some miss
        kind = rng.integers(0, 3, n)
        # the window moves by a bucket every 40,000 rows; one row in 1,000 lies far outside the ring
        tms = world.t_in + (np.arange(n) // 40_000) * 10_000 + rng.integers(0, 10_000, n)
        tms[rng.integers(0, n, n // 1000)] += 10_000 * 500
        ads = [world.keys[i] if i < len(world.keys) else b"m" * 36 for i in ad_i]
        rows = list(zip(ads, [(b"view", b"click", b"purchase")[k] for k in kind], [str(t).encode() for t in tms]))
        want, wst = am.count(encode(rows, "strings"), world.map)   # (the same rows in either encoding)
        for k in ("strings", "int64"):
            b = encode(rows, k)
            c.reset()
            got, st = run_device(c, b)
            assert_model(got, st, want, wst)
            info = c.arrow_launch_info()
            assert info["grid"] == res and info["tiles"] == 3 * res + 2 and info["per_lane_tiles"] == 0
        assert wst["join_misses"] > 0 and st["out_of_ring"] > 0


# ---- tables and parking ---------------------------------------------------------------------------------------------

def test_partial_cuckoo_table(world):
    keep = [i for i in range(len(world.ads)) if i % 10]
    amap = {world.keys[i]: world.camp[i] for i in keep}
    b = am.fixture("gen_s7_dict")
    want, wst = am.count(b, amap)
    with YsbContext(n_campaigns=100, sparse_fast_join=True, **SMALL) as c:
        c.load_ad_map([world.ads[i] for i in keep], [world.camp[i] for i in keep])
        got, st = run_device(c, b)
    assert wst["join_misses"] > 0 and wst["joined"] > 0
    assert_model(got, st, want, wst)


def test_hbm_bucket_table():
    """Above 262,144 36-byte keys the cuckoo table is the HBM bucket layout (the SERIAL probe)."""
    from ysb_amd import GenParams
    g = GenParams(seed=23, n_campaigns=150_000, ads_per_campaign=2, events_per_sec=1000)
    ads = g.ids_packed()[1].reshape(-1, 36)
    camp = g.ad_campaign_index_array()
    raw, offs = g.events_host(0, 5000)
    lines = dostats.split_lines(raw.tobytes())[0]
    ev = [dostats.parse_event(ln) for ln in lines]
    rows = [(e["ad_id"].encode(), e["event_type"].encode(), e["event_time"].encode()) for e in ev]
    amap = {bytes(a): int(c) for a, c in zip(ads, camp)}
    b = encode(rows, "strings")
    want, wst = am.count(b, amap)
    with YsbContext(n_campaigns=150_000, **SMALL) as c:
        c.load_ad_map_packed(ads.reshape(-1), camp)
        got, st = run_device(c, b)
        info = c.arrow_launch_info()
    assert info["hbm_table"] == 1 and info["lds_counters"] == 0 and wst["joined"] > 1000
    assert_model(got, st, want, wst)


def test_sharded_table(world):
    from ysb_amd import ad_shard
    mine = [i for i, a in enumerate(world.ads) if ad_shard(a, 2) == 0]
    amap = {world.keys[i]: world.camp[i] for i in mine}
    b = am.fixture("gen_s7_int64")
    want, wst = am.count(b, amap, shard=(0, 2))
    assert wst["foreign_shard"] > 0 and wst["joined"] > 0 and wst["join_misses"] == 0
    for strict in (False, True):
        with YsbContext(n_campaigns=100, strict=strict, **SMALL) as c:
            c.load_ad_map(world.ads, world.camp, shard=(0, 2))
            dev = Dev(c)
            c.submit_arrow_device(am.to_cols(b, dev.put))
            if strict:
                with pytest.raises(YsbError) as e:
                    c.sync()
                assert e.value.code == -8
            else:
                assert_model(c.drain_buckets(), c.stats(), want, wst)
            dev.free()


def test_parking_with_bad_times(world):
    """Views of ads the map lacks are parked with the time's parse outcome; after the resolve,
    counts and stats equal a run whose map was complete."""
    known = [i for i in range(len(world.ads)) if i % 3]
    rows = []
    for i, r in enumerate(world.rows[:600]):
        rows.append((r[0], r[1], b"12x" if i % 5 == 0 else r[2]))   # every fifth time does not parse
    b = encode(rows, "strings")
    want, wst = am.count(b, world.map)
    assert wst["time_errors"] > 0
    with YsbContext(n_campaigns=100, **SMALL) as c:
        c.load_ad_map([world.ads[i] for i in known], [world.camp[i] for i in known])
        c.park_misses(1 << 12)
        dev = Dev(c)
        c.submit_arrow_device(am.to_cols(b, dev.put))
        c.sync()
        assert c.stats()["join_misses"] == 0
        c.resolve_parked_with(lambda keys: [world.map.get(k) for k in keys])
        got, st = c.drain_buckets(), c.stats()
        dev.free()
    assert_model(got, st, want, wst)


@pytest.mark.parametrize("div", [10000, 7, 1])
def test_window_arithmetic(world, div):
    """Negative times and divisors other than 10000 (tests/windows_corpus.py), as strings and int64."""
    times = wc.boundary_times(div)
    texts = {"strings": [(t, f.encode()) for t in times for f in wc.forms(t)], "int64": [(t, str(t).encode()) for t in times]}
    for kind in ("strings", "int64"):
        rows = [(world.keys[(7 * i) % len(world.keys)], b"view", f) for i, (_, f) in enumerate(texts[kind])]
        b = encode(rows, kind)
        want, wst = am.count(b, world.map, divisor=div)
        assert wst["joined"] == len(rows) and set(bk for _, bk in want) == {wc.jdiv(t, div) for t in times}
        with YsbContext(n_campaigns=100, time_divisor_ms=div, ring_base_bucket=-1, **SMALL) as c:
            c.load_ad_map(world.ads, world.camp)
            got, st = run_device(c, b)
        assert_model(got, st, want, wst)
        assert st["out_of_ring"] == sum(v for (_, bk), v in want.items() if not -1 <= bk < 15) > 0


def test_ring_auto_base(world):
    n = 300
    rows = [(world.keys[i % 50], b"view" if i % 3 == 0 else b"click", str((105 + i % 5) * 10000 + i).encode()) for i in range(n)]
    rows[12] = (b"f" * 36, b"view", b"500000")                 # a view that joins nothing
    rows[201] = (rows[201][0], b"view", b"1009999")            # the smallest counted bucket of rows 0..255
    rows[202] = (rows[202][0], b"view", b"9x")                 # joined, but its time does not parse
    rows[260] = (rows[260][0], b"view", b"900000")             # smaller, but past the first 256 rows
    b = encode(rows, "strings")
    want, wst = am.count(b, world.map)
    with YsbContext(n_campaigns=100, **SMALL) as c:
        c.load_ad_map(world.ads, world.camp)
        got, st = run_device(c, b)
        assert c.ring_range() == (100 - 2, 16)
    assert_model(got, st, want, wst)
    assert st["out_of_ring"] == 1 and st["join_misses"] == 1 and st["time_errors"] == 1


# ---- errors ---------------------------------------------------------------------------------------------------------------

def test_strict_invalid_row(world):
    b = am.fixture("nulls")
    with YsbContext(n_campaigns=100, strict=True, **SMALL) as c:
        c.load_ad_map(world.ads, world.camp)
        c.submit_arrow(am.to_node(b))
        with pytest.raises(YsbError) as e:
            c.sync()
        assert e.value.code == -8


def test_errors(ctx, world):
    b = encode(world.rows[:64], "strings")
    node = am.to_node(b)
    bd = arrow.bind(node.schema)
    with YsbContext(n_campaigns=10, **SMALL) as c:   # no ad map
        for call in (lambda: c.submit_arrow(node), lambda: c.submit_arrow_device(am.to_cols(b)), c.arrow_launch_info):
            with pytest.raises(YsbError) as e:
                call()
            assert e.value.code == -3 and "ysb_load_ad_map" in str(e.value)
    big = encode(world.rows * 20, "strings")        # 30,000 rows x 36 B of ids alone pass max_batch_bytes = 1 MiB
    with pytest.raises(YsbError) as e:
        ctx.submit_arrow(am.to_node(big))
    assert e.value.code == -4 and "max_batch_bytes" in str(e.value)

    def broken(change):
        nd = am.to_node(b)
        change(nd)
        with pytest.raises(YsbError) as e:
            ctx.submit_arrow(nd, binding=bd)
        assert e.value.code == -1, str(e.value)
        return str(e.value)
    def null_offsets(nd):
        nd.keep[1][1]._bufs[1] = None
    def backwards(nd):
        nd.keep[1][1].keep[0][1][64] = -1
    assert "offsets" in broken(null_offsets)
    assert "n_children" in broken(lambda nd: setattr(nd.array, "n_children", 3))
    assert "negative" in broken(lambda nd: setattr(nd.array, "length", -1))
    assert "negative" in broken(lambda nd: setattr(nd.array, "offset", -1))
    assert "2^31" in broken(lambda nd: setattr(nd.array, "length", 1 << 31))
    assert "below the first" in broken(backwards)
    cols = am.to_cols(b)
    cols.col[2].kind = 7
    with pytest.raises(YsbError) as e:
        ctx.submit_arrow_device(cols)
    assert e.value.code == -1 and "kinds" in str(e.value)


def test_pending_frame_carry_refuses_arrow(world):
    from ysb_amd import lz4
    raw, _ = gd.events("gen_s7")
    frame = lz4.frame_pack(bytes(raw[:100_000]))
    blocks, _ = lz4.frame_index(frame)
    b = encode(world.rows[:10], "strings")
    with YsbContext(n_campaigns=100, **SMALL) as c:
        c.load_ad_map(world.ads, world.camp)
        c.submit_lz4_blocks(frame, blocks[:1], slot=0, more=True)
        for call in (lambda: c.submit_arrow(am.to_node(b), slot=1), lambda: c.submit_arrow_device(am.to_cols(b))):
            with pytest.raises(YsbError) as e:
                call()
            assert e.value.code == -3 and "carry" in str(e.value)


def test_layout_sampling_is_left_alone(world):
    """An Arrow submit between two text submits leaves the layout the sampling chose as it was."""
    raw, offs = gd.events("gen_s7")
    b = am.fixture("gen_s7_strings")
    want = gd.expected("gen_s7")[0]
    with YsbContext(n_campaigns=100, timing=True, **SMALL) as c:
        c.load_ad_map(world.ads, world.camp)
        c.submit(raw, offs)
        info = c.launch_info()
        dev = Dev(c)
        c.submit_arrow_device(am.to_cols(b, dev.put))   # no sync between them
        assert c.launch_info() == info
        c.submit(raw, offs)
        assert c.launch_info() == info
        got, st = c.drain_buckets(), c.stats()
        ms, launches = c.kernel_time()
        assert launches == 3 and ms > 0 and c.path_time()[1] == 3
        dev.free()
    assert got == {k: 3 * v for k, v in want.items()} and st["batches"] == 3 and st["events"] == 4500
