"""GPU: the columnar count (ysb_submit_columns_device / ysb_submit_columns) against its CPU
model (tests/colcount_model.py) and the oracle.  Every image is built on the host with numpy
over a 0xA5 canary; before the upload, rows [n_rows, batch_rows) of every column and the
validity bits >= n_rows are filled with countable views of a known ad, so a kernel that reads
past n_rows shows up as extra counts."""
import ctypes as C

import numpy as np
import pytest

import colcount_model as ccm
import columns_model as cm
import golden_data as gd
from oracle import dostats, oracle
from ysb_amd import GenParams, YsbContext, YsbError, _lib, columns_layout, columns_read_ranges, device_sync

pytestmark = pytest.mark.gpu

SMALL = dict(window_ring=16, max_batch_events=1 << 12, max_batch_bytes=1 << 20, overflow_capacity=1 << 10)
JAVA, VALID = _lib.YSB_COL_JAVA_ORDER, _lib.YSB_COL_VALIDITY
FIVE = ("events", "views", "joined", "join_misses", "parse_errors")
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


@pytest.fixture(scope="module")
def world():
    """The gen_s7 fixture once: its lines, ads, the model's map, and a time inside its buckets."""
    class W:
        pass
    w = W()
    raw, offs = gd.events("gen_s7")
    w.raw, w.offs = raw, offs
    w.lines = dostats.split_lines(raw)[0]
    w.ads, w.camp = gd.ad_arrays()
    w.keys = [a.encode() for a in w.ads]
    w.map = dict(zip(w.keys, w.camp))
    w.t_in = int(cm._fields(w.lines[0])["event_time"])
    w.corpus = cm.mutation_corpus(w.lines)
    return w


@pytest.fixture(scope="module")
def ctx10(world):
    with YsbContext(n_campaigns=100, **SMALL) as c:   # the fixture's 100 campaigns
        c.load_ad_map(world.ads, world.camp)
        yield c


def run_device(c, image, rows, n, flags=0):
    """One columnar submit of a host image through HBM: (drained rows, stats)."""
    d = c.device_alloc(image.size)
    try:
        c.h2d(d, image)
        assert d % 16 == 0
        c.submit_columns_device(d, rows, n, flags)
        got, st = c.drain_buckets(), c.stats()
    finally:
        c.device_free(d)
    return got, st


def assert_model(got, st, want, wst, batches=1):
    assert got == want
    for k in FIVE + ("foreign_shard",):
        assert st[k] == wst[k], (k, st[k], wst[k])
    assert st["deferred"] == 0 and st["time_errors"] == 0 and st["batches"] == batches
    assert st["overflow_dropped"] == 0


def gen_image(world, n, rows, java, lines=None):
    image, _, _ = cm.build((lines or world.lines)[:n], batch_rows=rows, java_order=java, canary=0xA5)
    return ccm.fill_past(image, rows, n, world.keys[0], world.t_in, java_order=java, validity=True)


# ---- geometry ------------------------------------------------------------------------------------

@pytest.mark.parametrize("java", [False, True])
@pytest.mark.parametrize("extra", [0, 100])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 1500])
def test_geometry(ctx10, world, n, extra, java):
    rows = n + extra
    image = gen_image(world, n, rows, java)
    for flags in ((JAVA if java else 0), (JAVA if java else 0) | VALID):
        ctx10.reset()
        want, wst = ccm.count(image, rows, n, world.map, java_order=java, validity=bool(flags & VALID))
        got, st = run_device(ctx10, image, rows, n, flags)
        assert_model(got, st, want, wst)
        info = ctx10.columns_launch_info()
        assert info == {"rows": n, "lds_counters": 1, "hbm_table": 0, "java_order": int(java),
                        "validity": int(bool(flags & VALID))}
    if n == 1500:
        assert (want, wst["views"]) == (gd.expected("gen_s7")[0], 506)


def test_empty_submit_is_a_batch(ctx10, world):
    ctx10.reset()
    image = gen_image(world, 0, 64, False)
    got, st = run_device(ctx10, image, 64, 0, VALID)
    assert got == {} and st["events"] == 0 and st["batches"] == 1


# ---- decode -> count, never leaving HBM ---------------------------------------------------------

def decode_then_count(c, lines, rows):
    data, offs = cm.pack(lines)
    n = len(lines)
    total = columns_layout(rows)["start"][8]
    d_b, d_o, d_out = c.device_alloc(data.size), c.device_alloc(4 * n), c.device_alloc(total)
    try:
        c.h2d(d_b, data)
        c.h2d(d_o, offs)
        c.h2d(d_out, np.full(total, 0xA5, dtype=np.uint8))
        info = c.decode_columns_device(d_b, data.size, d_o, n, d_out, rows)
        c.submit_columns_device(d_out, rows, n, VALID)
        got, st = c.drain_buckets(), c.stats()
    finally:
        for p in (d_b, d_o, d_out):
            c.device_free(p)
    return got, st, info


def test_decode_then_count_equals_the_oracle(ctx10, world):
    ctx10.reset()
    got, st, info = decode_then_count(ctx10, world.lines, 1500)
    want, wst = oracle.run(oracle.AdMap(world.ads, world.camp), world.raw, world.offs)
    assert info["valid"] == 1500 and got == want
    for k in wst:
        assert st[k] == wst[k], k
    assert st["deferred"] == 0 and st["batches"] == 1


def test_decode_then_count_on_the_mutation_corpus(ctx10, world):
    ctx10.reset()
    lines = [ln for ln, _, _ in world.corpus]
    got, st, _ = decode_then_count(ctx10, lines, 1600)
    image, _, _ = cm.build(lines, batch_rows=1600)
    want, wst = ccm.count(image, 1600, 1500, world.map, validity=True)
    assert wst["parse_errors"] == 498
    assert_model(got, st, want, wst)


# ---- counting paths --------------------------------------------------------------------------------

@pytest.mark.parametrize("n_campaigns,lds_count,lds", [(10, True, 1), (100, True, 1), (200, True, 0), (10, False, 0)])
def test_counting_paths(world, n_campaigns, lds_count, lds):
    camp = [i % n_campaigns for i in range(len(world.ads))]
    amap = dict(zip(world.keys, camp))
    image = gen_image(world, 1500, 1600, False)
    want, wst = ccm.count(image, 1600, 1500, amap, validity=True)
    with YsbContext(n_campaigns=n_campaigns, lds_count=lds_count, **SMALL) as c:
        c.load_ad_map(world.ads, camp)
        got, st = run_device(c, image, 1600, 1500, VALID)
        assert c.columns_launch_info()["lds_counters"] == lds
    assert_model(got, st, want, wst)
    assert wst["joined"] == 506


# ---- partial cuckoo table ---------------------------------------------------------------------------

def test_partial_cuckoo_table(world):
    keep = [i for i in range(len(world.ads)) if i % 10]
    amap = {world.keys[i]: world.camp[i] for i in keep}
    image = gen_image(world, 1500, 1500, True)
    want, wst = ccm.count(image, 1500, 1500, amap, java_order=True)
    with YsbContext(n_campaigns=100, sparse_fast_join=True, **SMALL) as c:
        c.load_ad_map([world.ads[i] for i in keep], [world.camp[i] for i in keep])
        got, st = run_device(c, image, 1500, 1500, JAVA)
    assert wst["join_misses"] > 0 and wst["joined"] > 0
    assert_model(got, st, want, wst)


# ---- HBM bucket table --------------------------------------------------------------------------------

class Big:
    """n_campaigns x 2 generated 36-byte ads and 20,000 generated events as host bytes (the
    device generator's are the same bytes)."""
    cache = {}

    def __init__(self, n_campaigns):
        self.g = GenParams(seed=23, n_campaigns=n_campaigns, ads_per_campaign=2, events_per_sec=1000)
        self.ads = self.g.ids_packed()[1].reshape(-1, 36)
        self.camp = self.g.ad_campaign_index_array()
        self.n = 20_000
        self.raw, self.offs = self.g.events_host(0, self.n)

    @classmethod
    def of(cls, n_campaigns):
        if n_campaigns not in cls.cache:
            cls.cache[n_campaigns] = cls(n_campaigns)
        return cls.cache[n_campaigns]


@pytest.mark.parametrize("n_campaigns,withheld,hbm", [(150_000, False, 1), (150_000, True, 0), (300_000, True, 1)])
def test_hbm_bucket_table(n_campaigns, withheld, hbm):
    """The bucket layout is chosen above 262,144 36-byte keys IN THE CUCKOO TABLE, and
    sparse_fast_join thins that table to every other key before the choice.  300,000 ads with
    the full map are buckets; the same ads with every tenth withheld and sparse_fast_join leave
    135,000 keys in the cuckoo table, which is the slot layout (hbm_table 0, counts still the
    oracle's); 600,000 ads thinned the same way leave 270,000: the partial BUCKET table, whose
    misses go to the general table in the lane."""
    big = Big.of(n_campaigns)
    keep = np.arange(big.ads.shape[0]) % 10 != 0 if withheld else np.ones(big.ads.shape[0], dtype=bool)
    ads, camp = big.ads[keep], big.camp[keep]
    want, wst = oracle.run(oracle.AdMap([bytes(a) for a in ads], camp), big.raw, big.offs)
    n, rows = big.n, big.n + 50
    cap = n * big.g.max_line_bytes()
    total = columns_layout(rows)["start"][8]
    with YsbContext(n_campaigns=n_campaigns, sparse_fast_join=withheld, **SMALL) as c:
        c.load_ad_map_packed(ads.reshape(-1), camp)
        d_b, d_o, d_out = c.device_alloc(cap), c.device_alloc(4 * n), c.device_alloc(total)
        nb = c.gen_events_device(big.g, 0, n, d_b, cap, d_o)
        assert nb == big.raw.size
        assert c.decode_columns_device(d_b, nb, d_o, n, d_out, rows)["valid"] == n
        c.submit_columns_device(d_out, rows, n, VALID)
        got, st = c.drain_buckets(), c.stats()
        info = c.columns_launch_info()
        for p in (d_b, d_o, d_out):
            c.device_free(p)
    assert info["hbm_table"] == hbm and info["lds_counters"] == 0
    assert got == want
    for k in wst:
        assert st[k] == wst[k], k
    assert st["deferred"] == 0 and (st["join_misses"] > 0) == withheld and st["joined"] > 5000


# ---- sharded table --------------------------------------------------------------------------------------

def test_sharded_table(world):
    from ysb_amd import ad_shard
    mine = [i for i, a in enumerate(world.ads) if ad_shard(a, 2) == 0]
    amap = {world.keys[i]: world.camp[i] for i in mine}
    image = gen_image(world, 1500, 1500, False)
    want, wst = ccm.count(image, 1500, 1500, amap, shard=(0, 2))
    assert wst["foreign_shard"] > 0 and wst["joined"] > 0 and wst["join_misses"] == 0
    for strict in (False, True):
        with YsbContext(n_campaigns=100, strict=strict, **SMALL) as c:
            c.load_ad_map(world.ads, world.camp, shard=(0, 2))
            d = c.device_alloc(image.size)
            c.h2d(d, image)
            c.submit_columns_device(d, 1500, 1500, 0)
            if strict:
                with pytest.raises(YsbError) as e:
                    c.sync()
                assert e.value.code == -8
            else:
                assert_model(c.drain_buckets(), c.stats(), want, wst)
            c.device_free(d)


# ---- window arithmetic -----------------------------------------------------------------------------------

@pytest.mark.parametrize("java", [False, True])
@pytest.mark.parametrize("div", [10000, 7, 1])
def test_window_arithmetic(world, div, java):
    times = [k * div + d for k in (-40, -3, -2, -1, 0, 1, 2, 13, 14, 15, 40) for d in (-1, 0, 1)]
    times += [I64_MIN + 100, I64_MAX - 100] if div == 1 else [I64_MIN, I64_MIN + 1, I64_MAX]
    n = len(times)
    ads = [world.keys[(7 * i) % len(world.keys)] for i in range(n)]
    image = ccm.make_image(ads, [b"view"] * n, times, n + 30, java_order=java, valid=[True] * n)
    ccm.fill_past(image, n + 30, n, world.keys[0], 0, java_order=java, validity=True)
    want, wst = ccm.count(image, n + 30, n, world.map, divisor=div, java_order=java, validity=True)
    assert wst["joined"] == n
    with YsbContext(n_campaigns=100, time_divisor_ms=div, ring_base_bucket=-1, **SMALL) as c:
        c.load_ad_map(world.ads, world.camp)
        got, st = run_device(c, image, n + 30, n, VALID | (JAVA if java else 0))
    assert_model(got, st, want, wst)
    outside = sum(v for (_, b), v in want.items() if not -1 <= b < 15)
    assert st["out_of_ring"] == outside > 0


# ---- ring auto-base ------------------------------------------------------------------------------------------

def test_ring_auto_base(world):
    n = 300
    ads = [world.keys[i % 50] for i in range(n)]
    types = [b"view" if i % 3 == 0 else b"clic" for i in range(n)]
    times = [(105 + i % 5) * 10000 + i for i in range(n)]
    ads[12], types[12], times[12] = b"f" * 36, b"view", 50 * 10000        # a view that joins nothing
    types[13], times[13] = b"purc", 60 * 10000                            # no view
    types[201], times[201] = b"view", 100 * 10000 + 9999                  # the smallest joined bucket of rows 0..255
    types[260], times[260] = b"view", 90 * 10000                          # smaller, but past the first 256 rows
    image = ccm.make_image(ads, types, times, n)
    want, wst = ccm.count(image, n, n, world.map)
    with YsbContext(n_campaigns=100, **SMALL) as c:
        c.load_ad_map(world.ads, world.camp)
        got, st = run_device(c, image, n, n, 0)
        assert c.ring_range() == (100 - 2, 16)
    assert_model(got, st, want, wst)
    assert st["out_of_ring"] == 1 and st["join_misses"] == 1
    assert want[(world.map[ads[260]], 90)] == 1


# ---- out-of-ring emptying across a chain of submits -------------------------------------------------------------

def test_out_of_ring_map_is_emptied_between_columnar_submits(world):
    camp = [i % 200 for i in range(len(world.ads))]
    amap = dict(zip(world.keys, camp))
    want = {}
    with YsbContext(n_campaigns=200, ring_base_bucket=0, **SMALL) as c:   # overflow_capacity 1024
        c.load_ad_map(world.ads, camp)
        d = c.device_alloc(columns_layout(512)["start"][8])
        for s in range(8):   # 8 x 512 distinct out-of-ring cells: 4096 > the map's 2048 + the list's 1024
            ads = [world.keys[r % len(world.keys)] for r in range(512)]
            times = [(1000 + 512 * s + r) * 10000 for r in range(512)]
            image = ccm.make_image(ads, [b"view"] * 512, times, 512)
            cells, _ = ccm.count(image, 512, 512, amap)
            assert len(cells) == 512 and not set(cells) & set(want)
            want.update(cells)
            c.h2d(d, image)
            c.submit_columns_device(d, 512, 512, 0)
            device_sync(c.device)   # not ysb_sync: only the submits themselves may empty the map
        got, st = c.drain_buckets(), c.stats()
        c.device_free(d)
    assert st["overflow_dropped"] == 0 and st["out_of_ring"] == 4096 and st["batches"] == 8
    assert got == want and len(got) == 4096


# ---- the host form ---------------------------------------------------------------------------------------------------

def outside_ranges(image, rows, n, flags, value):
    """image with every byte outside columns_read_ranges set to value."""
    keep = np.zeros(image.size, dtype=bool)
    for off, nb in columns_read_ranges(rows, n, flags):
        keep[off:off + nb] = True
    out = image.copy()
    out[~keep] = value
    return out


@pytest.mark.parametrize("own", [False, True])
def test_host_form(ctx10, world, own):
    flags = (VALID | JAVA) if own else 0
    lay = columns_layout(64)
    size = lay["start"][8] if flags & VALID else lay["image_bytes"]
    images, want, wst = [], {}, dict.fromkeys(ccm.STATS, 0)
    for k in range(6):
        img, _, _ = cm.build(world.lines[64 * k:64 * k + 64], batch_rows=64, java_order=bool(flags & JAVA), canary=0xA5)
        images.append(img)
        cells, s = ccm.count(img, 64, 64, world.map, java_order=bool(flags & JAVA), validity=bool(flags & VALID))
        for key, v in cells.items():
            want[key] = want.get(key, 0) + v
        for key in s:
            wst[key] += s[key]
    assert wst["joined"] > 50
    for value in (0xA5, 0):
        ctx10.reset()
        for k, img in enumerate(images):
            slot = k & 1
            src = outside_ranges(img, 64, 64, flags, value)[:size]
            ctx10.wait(slot)
            if own:
                addr = ctx10.slot_buffers(slot)[0]
                np.ctypeslib.as_array((C.c_uint8 * size).from_address(addr))[:] = src
                ctx10.submit_columns(addr, 64, 64, slot=slot, flags=flags)
            else:
                ctx10.submit_columns(src, 64, 64, slot=slot, flags=flags)
        assert_model(ctx10.drain_buckets(), ctx10.stats(), want, wst, batches=6)


def test_host_form_capacity(ctx10):
    rows = 10_000   # 36 B x 10,000 rows x 3 columns alone pass max_batch_bytes = 1 MiB
    assert columns_layout(rows)["image_bytes"] > 1 << 20
    with pytest.raises(YsbError) as e:
        ctx10.submit_columns(np.zeros(64, dtype=np.uint8), rows, 1)
    assert e.value.code == -4 and "max_batch_bytes" in str(e.value)


# ---- mixing with JSON submits, timing ---------------------------------------------------------------------------------

def test_mixing_with_a_json_submit(world):
    image, _, _ = cm.build(world.lines)
    want, _ = gd.expected("gen_s7")
    with YsbContext(n_campaigns=100, timing=True, **SMALL) as c:
        c.load_ad_map(world.ads, world.camp)
        d = c.device_alloc(image.size)
        c.h2d(d, image)
        c.submit(world.raw, world.offs)
        info = c.launch_info()
        c.submit_columns_device(d, 1500, 1500, VALID)   # no sync between the two
        got, st = c.drain_buckets(), c.stats()
        assert c.launch_info() == info and info["tbl"] == 0 and info["record_mode"] == 0
        ms, launches = c.kernel_time()
        assert launches == 2 and ms > 0 and c.path_time()[1] == 2 and c.path_time()[0] >= ms
        c.device_free(d)
    assert got == {k: 2 * v for k, v in want.items()}
    assert st["events"] == 3000 and st["views"] == 1012 and st["joined"] == 1012 and st["batches"] == 2


# ---- errors --------------------------------------------------------------------------------------------------------------

def test_errors(ctx10):
    d = ctx10.device_alloc(columns_layout(64)["start"][8])
    try:
        with YsbContext(n_campaigns=10, **SMALL) as c:   # no ad map
            with pytest.raises(YsbError) as e:
                c.submit_columns_device(d, 64, 64)
            assert e.value.code == -3 and "ysb_load_ad_map" in str(e.value)
            with pytest.raises(YsbError) as e:
                c.columns_launch_info()
            assert e.value.code == -3 and "no columnar launch" in str(e.value)
        for args, code, word in (((d, 64, 65, 0), -4, "do not fit"), ((d, 0, 0, 0), -1, "batch_rows"),
                                 ((d, 1 << 31, 1, 0), -1, "batch_rows"), ((d + 8, 64, 64, 0), -1, "aligned"),
                                 ((0, 64, 64, 0), -1, "NULL"), ((d, 64, 64, 4), -1, "flags")):
            with pytest.raises(YsbError) as e:
                ctx10.submit_columns_device(*args)
            assert e.value.code == code and word in str(e.value), args
            assert _lib.ERRORS[code] in str(e.value)
    finally:
        ctx10.device_free(d)
