"""GPU: the joined-views call (ysb_join_device) against its CPU model (tests/join_model.py: the
oracle run one line at a time) and against the counting path on a second context of the same
configuration.  Every output buffer is filled with a 0xA5 canary before the call and every byte
outside rows [0, rows_written) of each column must still hold it afterwards."""
import json

import numpy as np
import pytest

import golden_data as gd
import join_model as jm
from ysb_amd import GenParams, YsbContext, YsbError, YSB_JOIN_KEYS, ad_shard, joined_columns, joined_layout

pytestmark = pytest.mark.gpu

SMALL = dict(window_ring=16, max_batch_events=1 << 12, max_batch_bytes=1 << 20, overflow_capacity=1 << 10)
SEVEN = ("events", "views", "joined", "join_misses", "parse_errors", "time_errors", "foreign_shard")
CANARY = 0xA5
ERR_ARG, ERR_STATE, ERR_CAPACITY = -1, -3, -4


class World:
    """The committed fixtures once: the map, its model, each fixture's lines and expected stream."""

    def __init__(self):
        self.ads, self.camp = gd.ad_arrays()
        self.model = jm.Model(self.ads, self.camp)
        self._want = {}

    def batch(self, stem, require_ip=False):
        key = (stem, require_ip)
        if key not in self._want:
            tbl = stem in gd.TBL_FILES
            raw, offs = gd.tbl_events(stem) if tbl else gd.events(stem)
            cols, st = self.model.batch(raw, offs, fmt="tbl" if tbl else "json", require_ip=require_ip)
            self._want[key] = (raw, offs, cols, st)
        return self._want[key]

    def lines(self, want):
        """(raw, offs, expected columns, stats) of chosen gen_s7 lines: want(line index, joined)."""
        raw, offs, cols, _ = self.batch("gen_s7")
        joined = set(int(r) for r in cols["row"])
        all_lines = jm.lines_of(raw, offs)
        pick = [ln for i, ln in enumerate(all_lines) if want(i, i in joined)]
        data = b"".join(pick)
        o = np.cumsum([0] + [len(ln) for ln in pick[:-1]]).astype(np.uint32) if pick else np.zeros(0, dtype=np.uint32)
        return (data, o) + self.model.batch(data, o)


@pytest.fixture(scope="module")
def world():
    return World()


def context(world, fmt="json", require_ip=False, load=True, **kw):
    c = YsbContext(n_campaigns=100, input_format=fmt, require_ip=require_ip, **{**SMALL, **kw})
    if load:
        c.load_ad_map(world.ads, world.camp)
    return c


def run_join(c, raw, offs, keys=False, cap_rows=None):
    """One join of a host batch through HBM over a canary: (columns, info, return code)."""
    buf = np.frombuffer(raw, dtype=np.uint8) if isinstance(raw, (bytes, bytearray)) else np.ascontiguousarray(raw, dtype=np.uint8)
    off = np.ascontiguousarray(offs, dtype=np.uint32)
    n = off.size
    cap = n if cap_rows is None else cap_rows
    flags = YSB_JOIN_KEYS if keys else 0
    lay = joined_layout(cap, flags)
    image = np.full(max(lay["start"][6], 16), CANARY, dtype=np.uint8)
    d_b, d_o, d_out = c.device_alloc(max(buf.size, 16)), c.device_alloc(max(4 * n, 16)), c.device_alloc(image.size)
    try:
        if buf.size:
            c.h2d(d_b, buf)
        if n:
            c.h2d(d_o, off)
        c.h2d(d_out, image)
        rc = 0
        try:
            info = c.join_device(d_b, buf.size, d_o, n, d_out, cap, flags)
        except YsbError as e:
            rc, info = e.code, e.info
        c.d2h(image, d_out)
    finally:
        for p in (d_b, d_o, d_out):
            c.device_free(p)
    rows = info["rows_written"]
    assert rows == min(info["joined"], cap)
    cols = joined_columns(image, lay, rows)
    for j in range(lay["n_cols"]):   # the canary behind each column's last written row, up to the next column
        tail = image[lay["start"][j] + lay["width"][j] * rows:lay["start"][j + 1]]
        assert (tail == CANARY).all(), "column %d written past row %d" % (j, rows)
    assert (image[lay["start"][6]:] == CANARY).all()
    return cols, info, rc


def assert_stream(cols, info, want, wst, rows=None):
    rows = len(want["row"]) if rows is None else rows
    for k in ("campaign", "row", "event_time", "time_ok"):
        assert np.array_equal(cols[k], want[k][:rows]), k
    for k in jm.STATS:
        assert info[k] == wst[k], (k, info[k], wst[k])
    assert info["foreign_shard"] == 0 and info["rows_written"] == rows


def counting_path(c2, raw, offs):
    """(drain_buckets(), stats()) of the same batch through ysb_submit_device on c2."""
    buf = np.frombuffer(raw, dtype=np.uint8) if isinstance(raw, (bytes, bytearray)) else np.ascontiguousarray(raw, dtype=np.uint8)
    off = np.ascontiguousarray(offs, dtype=np.uint32)
    d_b, d_o = c2.device_alloc(max(buf.size, 16)), c2.device_alloc(max(4 * off.size, 16))
    try:
        c2.h2d(d_b, buf)
        c2.h2d(d_o, off)
        c2.submit_device(d_b, buf.size, d_o, off.size)
        return c2.drain_buckets(), c2.stats()
    finally:
        c2.device_free(d_b)
        c2.device_free(d_o)


def assert_counting(cols, info, got, st, divisor=10000):
    for k in SEVEN:
        assert info[k] == st[k], (k, info[k], st[k])
    assert jm.histogram(cols, divisor) == got


# ---- fixtures ------------------------------------------------------------------------------------

@pytest.mark.parametrize("keys", [False, True])
@pytest.mark.parametrize("stem,require_ip", gd.FIXTURES + [(s, False) for s in gd.TBL_FIXTURES])
def test_fixtures(world, stem, require_ip, keys):
    raw, offs, want, wst = world.batch(stem, require_ip)
    fmt = "tbl" if stem in gd.TBL_FILES else "json"
    with context(world, fmt, require_ip) as c, context(world, fmt, require_ip) as c2:
        cols, info, rc = run_join(c, raw, offs, keys)
        assert rc == 0
        assert_stream(cols, info, want, wst)
        assert_counting(cols, info, *counting_path(c2, raw, offs))
        if keys:
            lines = jm.lines_of(raw, offs)
            ids = [bytes(cols["key"][i][:cols["key_len"][i]]) for i in range(len(cols["row"]))]
            assert all((cols["key"][i][cols["key_len"][i]:] == 0).all() for i in range(len(ids)))   # zero-padded
            if ids:
                camp, _ = c.lookup_ads(ids)
                assert np.array_equal(camp, cols["campaign"])
            checked = 0
            for i, r in enumerate(cols["row"]):
                if fmt == "tbl":
                    assert ids[i] == lines[r].split(b"|")[2]
                    checked += 1
                    continue
                try:
                    ad = json.loads(lines[r].decode())["ad_id"]
                except (ValueError, KeyError, TypeError):
                    continue
                if not isinstance(ad, str):
                    continue
                assert ids[i] == ad.encode(), r
                checked += 1
            assert checked > 0   # (few of edge_orgjson's lines are JSON to Python)


# ---- geometry ------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129])
def test_prefixes(world, n):
    raw, offs, _, _ = world.batch("gen_s7")
    data, o = bytes(raw[:int(offs[n])] if n < len(offs) else raw), offs[:n]
    want, wst = world.model.batch(data, o)
    with context(world) as c:
        for keys in (False, True):
            cols, info, rc = run_join(c, data, o, keys)
            assert rc == 0 and info["tiles"] == (n + 63) // 64
            assert_stream(cols, info, want, wst)


def test_first_two_tiles_without_a_view_and_a_batch_of_joined_views_only(world):
    with context(world) as c, context(world) as c2:
        # no view among the first 128 lines: two tiles own no output row
        seen = [0]

        def late(i, joined):
            if not joined:
                seen[0] += 1
                return True
            return seen[0] >= 128
        data, o, want, wst = world.lines(late)
        assert len(want["row"]) > 100 and want["row"][0] >= 128
        cols, info, rc = run_join(c, data, o, True)
        assert rc == 0
        assert_stream(cols, info, want, wst)
        # every line a joined view: every tile owns 64 rows
        data, o, want, wst = world.lines(lambda i, joined: joined)
        assert len(want["row"]) == len(o) == 506
        cols, info, rc = run_join(c, data, o, True)
        assert rc == 0 and np.array_equal(cols["row"], np.arange(506, dtype=np.uint32))
        assert_stream(cols, info, want, wst)
        assert_counting(cols, info, *counting_path(c2, data, o))


@pytest.mark.parametrize("fmt", ["json", "tbl"])
def test_generated_batches_one_tile_and_several_tiles_per_workgroup(fmt):
    """Two device-generated batches sized from the kernel's own grid limit (info["max_grid"] of a
    first small call): one of 64 lines per workgroup the kernel can launch, where no workgroup
    takes a second tile (64 x 7 x 256 = 114,688 JSON lines on an MI355X), and one ten times that plus a ragged
    tail, where every workgroup takes several.  Checked against the generator truth's view
    count, row strictly ascending, and the counting path."""
    g = GenParams(seed=11, n_campaigns=100, ads_per_campaign=10, events_per_sec=100_000, fmt=fmt)
    _, ads = g.ids()
    big = dict(window_ring=64, max_batch_events=1 << 23, max_batch_bytes=1 << 20, overflow_capacity=1 << 10)
    with YsbContext(n_campaigns=100, input_format=fmt, **big) as c, YsbContext(n_campaigns=100, input_format=fmt, **big) as c2:
        for x in (c, c2):
            x.load_ad_map(ads, g.ad_campaign_index())
        probe = np.zeros(16, dtype=np.uint8)
        max_grid = run_join(c, probe[:0], np.zeros(0, dtype=np.uint32))[1]["max_grid"]
        assert max_grid > 0
        n1 = 64 * max_grid
        n2 = 10 * n1 + 37
        print("max_grid %d: batches of %d and %d lines" % (max_grid, n1, n2))
        cap = n2 * g.max_line_bytes()
        lay = joined_layout(n2, 0)
        d_b, d_o, d_out = c.device_alloc(cap), c.device_alloc(4 * n2), c.device_alloc(lay["start"][6])
        e_b, e_o = c2.device_alloc(cap), c2.device_alloc(4 * n2)
        try:
            for n in (n1, n2):
                nb = c.gen_events_device(g, 0, n, d_b, cap, d_o)
                assert c2.gen_events_device(g, 0, n, e_b, cap, e_o) == nb
                info = c.join_device(d_b, nb, d_o, n, d_out, n2)
                assert info["tiles"] == (n + 63) // 64 and info["grid"] == min(info["tiles"], max_grid)
                if n == n1:
                    assert info["tiles"] <= info["grid"]          # no workgroup takes a second tile
                else:
                    assert info["tiles"] >= 10 * info["grid"]     # every workgroup takes several
                rows = info["rows_written"]
                assert rows == info["joined"] == info["views"] and info["fast_rows"] == n
                image = np.empty(lay["start"][6], dtype=np.uint8)
                c.d2h(image, d_out)
                cols = joined_columns(image, lay, rows)
                assert (cols["row"][1:] > cols["row"][:-1]).all() and cols["row"][-1] < n and (cols["time_ok"] == 1).all()
                c2.reset()
                c2.submit_device(e_b, nb, e_o, n)
                c2.truth_accumulate(g, 0, n)
                mism, truth, counted = c2.truth_compare()
                assert mism == 0 and truth == counted == rows     # the generator truth's view count
                assert_counting(cols, info, c2.drain_buckets(), c2.stats())
        finally:
            for p in (d_b, d_o, d_out):
                c.device_free(p)
            for p in (e_b, e_o):
                c2.device_free(p)


# ---- capacity ------------------------------------------------------------------------------------

@pytest.mark.parametrize("keys", [False, True])
def test_capacity(world, keys):
    raw, offs, want, wst = world.batch("gen_s7")
    joined = len(want["row"])
    with context(world) as c:
        for cap in (0, 1, joined - 1, joined):
            cols, info, rc = run_join(c, raw, offs, keys, cap_rows=cap)
            assert rc == (ERR_CAPACITY if cap < joined else 0)
            assert_stream(cols, info, want, wst, rows=cap)   # the first cap rows exact, info complete
            assert info["joined"] == joined


# ---- state ---------------------------------------------------------------------------------------

def test_join_leaves_the_counting_state_alone(world):
    raw, offs, want, wst = world.batch("edge")
    g_raw, g_offs, _, _ = world.batch("gen_s7")
    with context(world, load=False) as c:
        c.load_ad_map(world.ads[1::2], world.camp[1::2])
        c.park_misses(4096)
        c.submit(g_raw, g_offs)
        before = (c.stats(), c.drain(), c.ring_range(), c.parked_info())
        assert before[3]["parked"] > 0
        for keys in (False, True):
            run_join(c, raw, offs, keys)
            run_join(c, g_raw, g_offs, keys)
        after = (c.stats(), c.drain(), c.ring_range(), c.parked_info())
        assert before == after


def test_withheld_ads_are_misses_until_upserted(world):
    raw, offs, want, wst = world.batch("gen_s7")
    held = set(range(0, len(world.ads), 7))
    keep = [i for i in range(len(world.ads)) if i not in held]
    part = jm.Model([world.ads[i] for i in keep], [world.camp[i] for i in keep])
    pwant, pst = part.batch(raw, offs)
    assert 0 < len(pwant["row"]) < len(want["row"]) and pst["join_misses"] > 0
    with context(world, load=False) as c:
        c.load_ad_map([world.ads[i] for i in keep], [world.camp[i] for i in keep])
        cols, info, rc = run_join(c, raw, offs, True)
        assert_stream(cols, info, pwant, pst)
        c.upsert_ad_map([world.ads[i] for i in sorted(held)], [world.camp[i] for i in sorted(held)])
        cols, info, rc = run_join(c, raw, offs, True)
        assert_stream(cols, info, want, wst)


# ---- table layouts -------------------------------------------------------------------------------

class Big:
    """n_campaigns x 2 generated 36-byte ads and 20,000 generated events (tests/test_gpu_colcount.py's)."""
    cache = {}

    def __init__(self, n_campaigns):
        self.g = GenParams(seed=23, n_campaigns=n_campaigns, ads_per_campaign=2, events_per_sec=1000)
        self.ads = self.g.ids_packed()[1].reshape(-1, 36)
        self.camp = self.g.ad_campaign_index_array()
        self.n = 20_000

    @classmethod
    def of(cls, n_campaigns):
        if n_campaigns not in cls.cache:
            cls.cache[n_campaigns] = cls(n_campaigns)
        return cls.cache[n_campaigns]


@pytest.mark.parametrize("n_campaigns,withheld,hbm", [(150_000, False, 1), (150_000, True, 0), (300_000, True, 1)])
def test_hbm_bucket_table(n_campaigns, withheld, hbm):
    """The bucket layout above 262,144 36-byte keys in the cuckoo table, as
    tests/test_gpu_colcount.py::test_hbm_bucket_table builds it: the full bucket table, the slot
    table thinned by sparse_fast_join, and the partial bucket table whose misses go to the
    general table in the lane.  Every tenth ad withheld: those views are misses."""
    big = Big.of(n_campaigns)
    keep = np.arange(big.ads.shape[0]) % 10 != 0 if withheld else np.ones(big.ads.shape[0], dtype=bool)
    ads, camp = big.ads[keep], big.camp[keep]
    cfg = dict(window_ring=16, max_batch_events=1 << 15, max_batch_bytes=1 << 20, overflow_capacity=1 << 10)
    n = big.n
    cap = n * big.g.max_line_bytes()
    lay = joined_layout(n, YSB_JOIN_KEYS)
    with YsbContext(n_campaigns=n_campaigns, sparse_fast_join=withheld, **cfg) as c, \
            YsbContext(n_campaigns=n_campaigns, sparse_fast_join=withheld, **cfg) as c2:
        for x in (c, c2):
            x.load_ad_map_packed(ads.reshape(-1), camp)
        assert c.ad_map_info()["buckets"] == hbm
        d_b, d_o, d_out = c.device_alloc(cap), c.device_alloc(4 * n), c.device_alloc(lay["start"][6])
        e_b, e_o = c2.device_alloc(cap), c2.device_alloc(4 * n)
        try:
            nb = c.gen_events_device(big.g, 0, n, d_b, cap, d_o)
            assert c2.gen_events_device(big.g, 0, n, e_b, cap, e_o) == nb
            info = c.join_device(d_b, nb, d_o, n, d_out, n, YSB_JOIN_KEYS)
            image = np.empty(lay["start"][6], dtype=np.uint8)
            c.d2h(image, d_out)
            cols = joined_columns(image, lay, info["rows_written"])
            c2.submit_device(e_b, nb, e_o, n)
            assert_counting(cols, info, c2.drain_buckets(), c2.stats())
        finally:
            for p in (d_b, d_o, d_out):
                c.device_free(p)
            for p in (e_b, e_o):
                c2.device_free(p)
    assert info["joined"] > 5000 and (info["join_misses"] > 0) == withheld and (cols["key_len"] == 36).all()
    assert (cols["row"][1:] > cols["row"][:-1]).all()
    # the key is the ad's, the campaign its campaign: ad a -> campaign a // 2, ads in generation order
    index = {bytes(a): i for i, a in enumerate(big.ads[:4000])}
    hits = [(index[bytes(k[:36])], int(cc)) for k, cc in zip(cols["key"][:2000], cols["campaign"][:2000]) if bytes(k[:36]) in index]
    assert all(cc == a // 2 for a, cc in hits)


def test_sparse_fast_join(world):
    raw, offs, want, wst = world.batch("gen_s7")
    with context(world, sparse_fast_join=True) as c:
        assert c.ad_map_info()["partial"] == 1
        cols, info, rc = run_join(c, raw, offs, True)
        assert rc == 0
        assert_stream(cols, info, want, wst)


def test_ids_of_other_lengths(world):
    """The fixture's ads renamed to ids of 4..56 bytes (and some of 57, which no table can hold):
    the general table joins them; the key column carries them."""
    raw, offs, _, _ = world.batch("gen_s7")
    names = {}
    for i, a in enumerate(world.ads):
        ln = 57 if i % 50 == 3 else 4 + i % 53
        names[a] = (("%d_" % i) + "x" * 57)[:ln]
    assert len(set(names.values())) == len(names)
    data = bytes(raw)
    pieces = []
    for ln in jm.lines_of(data, offs):
        ad = json.loads(ln.decode())["ad_id"]
        pieces.append(ln.replace(ad.encode(), names[ad].encode()) if ad in names else ln)
    data = b"".join(pieces)
    o = np.cumsum([0] + [len(p) for p in pieces[:-1]]).astype(np.uint32)
    ads = [names[a] for a in world.ads if len(names[a]) <= 56]
    camp = [cc for a, cc in zip(world.ads, world.camp) if len(names[a]) <= 56]
    model = jm.Model(ads, camp)
    want, wst = model.batch(data, o)
    assert len(want["row"]) > 400 and wst["join_misses"] > 0
    with context(world, load=False) as c, context(world, load=False) as c2:
        for x in (c, c2):
            x.load_ad_map(ads, camp)
        cols, info, rc = run_join(c, data, o, True)
        assert rc == 0
        assert_stream(cols, info, want, wst)
        assert_counting(cols, info, *counting_path(c2, data, o))
        lines = jm.lines_of(data, o)
        for i, r in enumerate(cols["row"]):
            assert bytes(cols["key"][i][:cols["key_len"][i]]) == json.loads(lines[r].decode())["ad_id"].encode()
        assert len(set(int(k) for k in cols["key_len"])) > 20


def test_sharded_table(world):
    raw, offs, want, wst = world.batch("gen_s7")
    mine = [i for i, a in enumerate(world.ads) if ad_shard(a, 2) == 0]
    part = jm.Model([world.ads[i] for i in mine], [world.camp[i] for i in mine])
    pwant, pst = part.batch(raw, offs)
    with context(world, load=False) as c, context(world, load=False) as c2:
        for x in (c, c2):
            x.load_ad_map(world.ads, world.camp, shard=(0, 2))
        cols, info, rc = run_join(c, raw, offs, True)
        assert rc == 0
        for k in ("campaign", "row", "event_time", "time_ok"):
            assert np.array_equal(cols[k], pwant[k]), k
        # the other shard's views are foreign, not misses, and are not emitted
        assert info["foreign_shard"] == pst["join_misses"] - wst["join_misses"] > 0
        assert info["join_misses"] == wst["join_misses"]
        assert info["joined"] == pst["joined"] == len(pwant["row"]) > 0
        assert_counting(cols, info, *counting_path(c2, raw, offs))


# ---- refusals ------------------------------------------------------------------------------------

def test_refusals(world):
    raw, offs, _, _ = world.batch("gen_s7")
    buf, off = np.frombuffer(raw, dtype=np.uint8), np.ascontiguousarray(offs, dtype=np.uint32)
    with context(world) as c:
        d_b, d_o, d_out = c.device_alloc(buf.size), c.device_alloc(4 * off.size), c.device_alloc(joined_layout(1 << 13)["start"][6])
        c.h2d(d_b, buf)
        c.h2d(d_o, off)

        def refused(code, word, *a):
            with pytest.raises(YsbError) as e:
                c.join_device(*a)
            assert e.value.code == code and word in str(e.value), str(e.value)
        try:
            refused(ERR_ARG, "d_out", d_b, buf.size, d_o, off.size, d_out + 4, off.size)
            refused(ERR_ARG, "d_bytes", d_b + 8, buf.size - 8, d_o, off.size, d_out, off.size)
            refused(ERR_ARG, "flags", d_b, buf.size, d_o, off.size, d_out, off.size, 2)
            refused(ERR_CAPACITY, "n_events", d_b, buf.size, d_o, (1 << 12) + 1, d_out, 1 << 13)
            assert c.join_device(d_b, buf.size, d_o, off.size, d_out, off.size)["joined"] == 506   # still usable
            c.group_init_host_fns(0, 1, lambda a: None, lambda s, n, w: np.frombuffer(s, dtype={1: np.uint8, 4: np.uint32, 8: np.uint64}[w])[:n])
            refused(ERR_STATE, "ysb_group_init", d_b, buf.size, d_o, off.size, d_out, off.size)
        finally:
            for p in (d_b, d_o, d_out):
                c.device_free(p)
    with context(world, load=False) as c:
        with pytest.raises(YsbError) as e:
            c.join(raw, offs)
        assert e.value.code == ERR_STATE and "ysb_load_ad_map" in str(e.value)


def test_host_convenience(world):
    raw, offs, want, wst = world.batch("edge")
    with context(world) as c:
        cols, info = c.join(raw, offs, keys=True)
        assert_stream(cols, info, want, wst)
        assert cols["key"].shape == (len(want["row"]), 56)
