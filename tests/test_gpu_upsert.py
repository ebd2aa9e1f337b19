"""GPU: the live map (ysb_ad_map_upsert, ysb_ad_map_lookup, ysb_ad_map_info) -- ads added
to and re-pointed in the device join tables between two launches.  Everything is checked
against a plain dict of the map; counts against the oracle on the full map and against a
fresh context loaded with the full map, through the scan's own (untouched) probes."""
import numpy as np
import pytest

from oracle import oracle
from ysb_amd import GenParams, YsbContext, YsbError, _lib
from ysb_amd.generator import ad_shard, json_to_tbl

pytestmark = pytest.mark.gpu

ABSENT = 0xFFFFFFFF
ERR_STATE, ERR_FORMAT = -3, -5   # include/ysb_hip.h YSB_ERR_STATE, YSB_ERR_FORMAT
SMALL = dict(window_ring=16, max_batch_events=1 << 15, max_batch_bytes=8 << 20, overflow_capacity=1 << 12)
PLACED = ("cuckoo_first", "cuckoo_second", "cuckoo_moved", "cuckoo_left_out")


def check_lookup(ctx, truth, absent=()):
    """lookup_ads of every key of the dict (and of ids that are not in it): the campaigns, and
    where in (1, 2) for a 36-byte key unless left out, 3 for any other.  Returns where."""
    keys = list(truth) + list(absent)
    camp, where = ctx.lookup_ads(keys)
    want = np.array([truth.get(k, ABSENT) for k in keys], dtype=np.uint32)
    assert (camp == want).all(), np.flatnonzero(camp != want)[:8]
    assert (where[len(truth):] == 0).all() and (where[:len(truth)] != 0).all()
    assert (where <= 3).all()
    n36 = np.array([len(k) == 36 for k in keys])
    assert (where[~n36 & (where != 0)] == 3).all()
    return dict(zip(keys, where.tolist()))


def assert_counts(got, st, want, wst):
    assert got == want
    for k, v in wst.items():
        assert st[k] == v, (k, st[k], v)
    assert st["overflow_dropped"] == 0


def run_paths(prepare, raw, offs, n_campaigns, paths=("submit", "device", "tbl", "columns"), **kw):
    """The batch through each path, every one on a context of its own that `prepare` gives its
    map: {path: (drained buckets, stats)}."""
    out = {}
    for path in paths:
        with YsbContext(n_campaigns=n_campaigns, input_format="tbl" if path == "tbl" else "json",
                        **dict(SMALL, **kw)) as ctx:
            prepare(ctx)
            if path == "submit":
                ctx.submit(raw, offs)
            elif path == "tbl":
                ctx.submit(*json_to_tbl(raw, offs))
            elif path == "device":
                d_b, d_o = ctx.device_alloc(raw.size), ctx.device_alloc(4 * offs.size)
                ctx.h2d(d_b, raw)
                ctx.h2d(d_o, offs)
                ctx.submit_device(d_b, raw.size, d_o, offs.size)
            else:
                image, valid, _ = ctx.decode_columns(raw, offs)
                assert valid.all()
                d = ctx.device_alloc(image.size)
                ctx.h2d(d, image)
                ctx.submit_columns_device(d, offs.size, offs.size, _lib.YSB_COL_VALIDITY)
            out[path] = (ctx.drain_buckets(), ctx.stats())
    return out


@pytest.fixture(scope="module")
def small_map():
    """100 campaigns x 10 ads, 20,000 events, the oracle's counts on the full map."""
    g = GenParams(seed=3, n_campaigns=100, ads_per_campaign=10, events_per_sec=1000)
    _, ads = g.ids()
    camp = g.ad_campaign_index()
    raw, offs = g.events_host(0, 20_000)
    want = oracle.run(oracle.AdMap(ads, camp), raw, offs)
    return g, ads, camp, raw, offs, want


@pytest.fixture(scope="module")
def big_map():
    g = GenParams(seed=11, n_campaigns=200_000, ads_per_campaign=2, events_per_sec=1000, with_skew=True)
    _, ads = g.ids()
    raw, offs = g.events_host(0, 300_000)
    return g, ads, g.ad_campaign_index(), raw, offs


# 1
def test_contention_at_the_smallest_table():
    g = GenParams(seed=8, n_campaigns=8, ads_per_campaign=5)
    _, ads = g.ids()
    camp = g.ad_campaign_index()
    with YsbContext(n_campaigns=8, **SMALL) as ctx:
        ctx.load_ad_map([], [])
        d = ctx.ad_map_info()
        assert (d["table_slots"], d["ctable_slots"], d["keys"], d["keys36"], d["buckets"]) == (64, 64, 0, 0, 0)
        info = ctx.upsert_ad_map(ads[:16], camp[:16])
        assert info["rebuilt"] == 0 and info["inserted"] == 16 and info["updated"] == 0 and info["entries"] == 16
        assert sum(info[k] for k in PLACED) == 16
        truth = dict(zip(ads[:16], camp[:16]))
        where = check_lookup(ctx, truth, absent=ads[16:])
        assert sum(w in (1, 2) for w in where.values()) == 16 - info["cuckoo_left_out"]
        assert info["partial"] == int(info["cuckoo_left_out"] > 0)
        d = ctx.ad_map_info()
        assert (d["keys"], d["keys36"], d["ctable_slots"]) == (16, 16 - info["cuckoo_left_out"], 64)
        assert d["partial"] == info["partial"]
        info = ctx.upsert_ad_map(ads[16:17], camp[16:17])
        assert info["rebuilt"] == 1 and info["inserted"] == 1 and info["device_ms"] == 0
        d = ctx.ad_map_info()
        assert (d["ctable_slots"], d["keys"], d["keys36"], d["partial"]) == (128, 17, 17, 0)
        truth[ads[16]] = camp[16]
        where = check_lookup(ctx, truth, absent=ads[17:])
        assert all(w in (1, 2) for k, w in where.items() if k in truth)


# 2
def test_slot_layout_in_place_then_rebuild(small_map):
    g, ads, camp, raw, offs, (want, wst) = small_map
    infos = []

    def fresh(ctx):
        ctx.load_ad_map(ads, camp)

    def upserted(ctx):
        ctx.load_ad_map(ads[:600], camp[:600])
        d = ctx.ad_map_info()
        assert (d["table_slots"], d["ctable_slots"], d["buckets"]) == (2048, 4096, 0)
        info = ctx.upsert_ad_map(ads[600:], camp[600:])
        assert info["rebuilt"] == 0 and info["inserted"] == 400 and sum(info[k] for k in PLACED) == 400
        assert info["cuckoo_left_out"] == 0 and info["partial"] == 0 and info["device_ms"] > 0
        assert ctx.ad_map_info()["keys36"] == 1000
        infos.append(info)

    got, ref = run_paths(upserted, raw, offs, 100), run_paths(fresh, raw, offs, 100)
    twst = oracle.run(oracle.AdMap(ads, camp), *json_to_tbl(raw, offs), fmt="tbl")
    assert twst[0] == want
    for path in got:
        assert_counts(*got[path], want, twst[1] if path == "tbl" else wst)
        assert got[path][0] == ref[path][0] and got[path][1] == ref[path][1], path
    print("placement of 400 into 600:", {k: infos[0][k] for k in PLACED})

    # 100 more new ads: 1100 > 4096 / 4, a rebuild; the same equality on the larger map
    g2 = GenParams(seed=3, n_campaigns=110, ads_per_campaign=10, events_per_sec=1000)
    _, ads2 = g2.ids()
    camp2 = g2.ad_campaign_index()
    assert ads2[:1000] == ads
    raw2, offs2 = g2.events_host(0, 20_000)
    want2, wst2 = oracle.run(oracle.AdMap(ads2, camp2), raw2, offs2)

    def rebuilt(ctx):
        upserted(ctx)
        info = ctx.upsert_ad_map(ads2[1000:], camp2[1000:])
        assert info["rebuilt"] == 1 and info["inserted"] == 100
        d = ctx.ad_map_info()
        assert (d["keys"], d["keys36"], d["ctable_slots"], d["table_slots"]) == (1100, 1100, 8192, 4096)

    def fresh2(ctx):
        ctx.load_ad_map(ads2, camp2)

    got, ref = run_paths(rebuilt, raw2, offs2, 110), run_paths(fresh2, raw2, offs2, 110)
    twst2 = oracle.run(oracle.AdMap(ads2, camp2), *json_to_tbl(raw2, offs2), fmt="tbl")
    for path in got:
        assert_counts(*got[path], want2, twst2[1] if path == "tbl" else wst2)
        assert got[path][0] == ref[path][0] and got[path][1] == ref[path][1], path


# 3
@pytest.mark.timeout(300)
def test_bucket_layout_in_place(big_map):
    g, ads, camp, raw, offs = big_map
    want, wst = oracle.run(oracle.AdMap(ads, camp), raw, offs)
    truth = dict(zip(ads, camp))
    for record in (True, False):
        with YsbContext(n_campaigns=200_000, window_ring=16, record_count=record,
                        max_batch_bytes=raw.size + 64, max_batch_events=offs.size + 1) as ctx:
            ctx.load_ad_map(ads[:300_000], camp[:300_000])
            d = ctx.ad_map_info()
            assert (d["buckets"], d["ctable_slots"], d["table_slots"]) == (1, 1 << 20, 1 << 20)
            info = ctx.upsert_ad_map(ads[300_000:], camp[300_000:])
            assert info["rebuilt"] == 0 and info["inserted"] == 100_000 and sum(info[k] for k in PLACED) == 100_000
            assert info["cuckoo_left_out"] == 0 and info["partial"] == 0
            print("placement of 100,000 into 300,000 (buckets):", {k: info[k] for k in PLACED},
                  "%.3f ms" % info["device_ms"])
            ctx.submit(raw, offs)
            assert_counts(ctx.drain_buckets(), ctx.stats(), want, wst)
            assert ctx.launch_info()["hbm_table"] == 1
            assert ctx.launch_info()["record_mode"] == int(record)
            if record:
                where = check_lookup(ctx, truth)
                assert all(w in (1, 2) for w in where.values())
                d = ctx.ad_map_info()
                assert (d["keys"], d["keys36"], d["buckets"], d["ctable_slots"]) == (400_000, 400_000, 1, 1 << 20)


# 4
@pytest.mark.timeout(300)
def test_layout_switch_by_rebuild(big_map):
    g, ads, camp, raw, offs = big_map
    with YsbContext(n_campaigns=200_000, **SMALL) as ctx:
        ctx.load_ad_map(ads[:262_000], camp[:262_000])
        d = ctx.ad_map_info()
        assert (d["buckets"], d["ctable_slots"]) == (0, 1 << 20)   # 2^20 slots x 64 B = 64 MiB: not above it
        info = ctx.upsert_ad_map(ads[262_000:263_000], camp[262_000:263_000])
        assert info["rebuilt"] == 1 and info["inserted"] == 1000   # 263,000 > 2^20 / 4
        d = ctx.ad_map_info()
        assert d["buckets"] == 1 and d["keys"] == d["keys36"] == 263_000
        where = check_lookup(ctx, dict(zip(ads[:263_000], camp[:263_000])), absent=ads[263_000:263_100])
        assert all(w in (1, 2) for k, w in where.items() if w)


# 5
@pytest.mark.parametrize("raw_batch", [False, True])
def test_stream_order(small_map, raw_batch):
    g, ads, camp, raw, offs, (want_new, _) = small_map
    want_old, _ = oracle.run(oracle.AdMap(ads[:600], camp[:600]), raw, offs)
    want = dict(want_old)
    for k, v in want_new.items():
        want[k] = want.get(k, 0) + v
    with YsbContext(n_campaigns=100, **SMALL) as ctx:
        ctx.load_ad_map(ads[:600], camp[:600])
        if raw_batch:
            ctx.submit_raw(raw, slot=0)      # its launch is still pending at the upsert
        else:
            d_b, d_o = ctx.device_alloc(raw.size), ctx.device_alloc(4 * offs.size)
            ctx.h2d(d_b, raw)
            ctx.h2d(d_o, offs)
            ctx.submit_device(d_b, raw.size, d_o, offs.size)
        info = ctx.upsert_ad_map(ads[600:], camp[600:])
        assert info["rebuilt"] == 0 and info["inserted"] == 400
        if raw_batch:
            ctx.submit_raw(raw, slot=1)
        else:
            ctx.submit_device(d_b, raw.size, d_o, offs.size)
        ctx.sync()
        assert ctx.drain_buckets() == want
        assert ctx.stats()["events"] == 2 * offs.size


# 6
def test_update(small_map):
    g, ads, camp, raw, offs, _ = small_map
    moved = list(range(0, 1000, 20))                    # 50 known ads, to other campaigns
    ids = [ads[i] for i in moved] + [ads[moved[7]]]     # one of them twice: the last entry wins
    cs = [(camp[i] + 37) % 100 for i in moved] + [5]
    truth = dict(zip(ads, camp))
    truth.update(zip(ids, cs))
    assert truth[ads[moved[7]]] == 5 != (camp[moved[7]] + 37) % 100
    want, wst = oracle.run(oracle.AdMap(list(truth), list(truth.values())), raw, offs)

    def prepare(ctx):
        ctx.load_ad_map(ads, camp)
        info = ctx.upsert_ad_map(ids, cs)
        assert (info["updated"], info["duplicates"], info["inserted"], info["rebuilt"]) == (50, 1, 0, 0)
        assert info["entries"] == 51 and sum(info[k] for k in PLACED) == 0
        check_lookup(ctx, truth)

    for path, (got, st) in run_paths(prepare, raw, offs, 100, paths=("submit", "columns")).items():
        assert_counts(got, st, want, wst)
    assert want != oracle.run(oracle.AdMap(ads, camp), raw, offs)[0]


# 7
def test_sharded(small_map):
    g, ads, camp, raw, offs, _ = small_map
    # the ads up to this shard's 250th: with the 600 loaded first the shard's cuckoo table has
    # 1024 slots (room for 256 keys), so the upsert works in place
    mine = [i for i in range(1000) if ad_shard(ads[i], 4) == 1][:250]
    upto = mine[-1] + 1
    g1 = GenParams(seed=3, n_campaigns=100, ads_per_campaign=10, events_per_sec=1000, ad_subset=mine)
    raw1, offs1 = g1.events_host(0, 20_000)
    want, wst = oracle.run(oracle.AdMap([ads[i] for i in mine], [camp[i] for i in mine]), raw1, offs1)
    assert wst["join_misses"] == 0 and wst["joined"] > 0
    with YsbContext(n_campaigns=100, strict=True, **SMALL) as ctx:
        ctx.load_ad_map(ads[:600], camp[:600], shard=(1, 4))
        n_old = sum(i < 600 for i in mine)
        d = ctx.ad_map_info()
        assert (d["keys"], d["ctable_slots"]) == (n_old, 1024) and 600 < upto
        info = ctx.upsert_ad_map(ads[:upto], camp[:upto])   # ads of all shards
        assert info["foreign"] == upto - len(mine)
        assert (info["updated"], info["inserted"], info["rebuilt"]) == (n_old, len(mine) - n_old, 0)
        d = ctx.ad_map_info()
        assert (d["keys"], d["shard_rank"], d["shard_n"]) == (len(mine), 1, 4)
        ctx.submit(raw1, offs1)
        ctx.sync()                                      # strict: no foreign view, no error
        st = ctx.stats()
        assert_counts(ctx.drain_buckets(), st, want, wst)
        assert st["foreign_shard"] == 0
        camp_got, where = ctx.lookup_ads(ads)
        assert ((where != 0) == np.isin(np.arange(1000), mine)).all()   # (no other shard's ad, none past upto)


# 8
def test_partial_path():
    g = GenParams(seed=21, n_campaigns=4, ads_per_campaign=4, events_per_sec=1000)
    _, ads = g.ids()
    camp = g.ad_campaign_index()
    raw, offs = g.events_host(0, 5000)
    want, wst = oracle.run(oracle.AdMap(ads, camp), raw, offs)
    with YsbContext(n_campaigns=4, sparse_fast_join=True, **SMALL) as ctx:
        ctx.load_ad_map(ads[:10], camp[:10])
        assert ctx.ad_map_info()["keys36"] == 5
        info = ctx.upsert_ad_map(ads[10:], camp[10:])
        assert (info["rebuilt"], info["inserted"], info["partial"]) == (0, 6, 1)
        assert info["cuckoo_left_out"] == 3 and info["cuckoo_first"] + info["cuckoo_second"] + info["cuckoo_moved"] == 3
        where = check_lookup(ctx, dict(zip(ads, camp)))
        assert sorted(where[a] for a in ads[10:]).count(3) == 3     # the left-out new keys: general table only
        assert ctx.ad_map_info()["partial"] == 1
        ctx.submit(raw, offs)
        st = ctx.stats()
        assert st["deferred"] > 0
        assert_counts(ctx.drain_buckets(), st, want, wst)


# 9
def test_other_key_lengths(small_map):
    g, ads, camp, raw, offs, _ = small_map
    odd = [b"", b"short", b"z" * 56]
    lines = raw.tobytes().split(b"\n")[:3000]
    for i, line in enumerate(lines):
        if i % 7 == 0:                                   # these lines carry one of the other ids
            at = line.index(b'"ad_id": "') + 10
            lines[i] = line[:at] + odd[(i // 7) % 3] + line[at + 36:]
    data = np.frombuffer(b"".join(l + b"\n" for l in lines), dtype=np.uint8)
    loffs = np.cumsum([0] + [len(l) + 1 for l in lines[:-1]]).astype(np.uint32)
    truth = dict(zip([a.encode() for a in ads], camp))
    truth.update(zip(odd, (11, 22, 33)))
    want, wst = oracle.run(oracle.AdMap(list(truth), list(truth.values())), data, loffs)
    assert wst["join_misses"] == 0
    with YsbContext(n_campaigns=100, **SMALL) as ctx:
        ctx.load_ad_map(ads, camp)
        info = ctx.upsert_ad_map(odd, (11, 22, 33))
        assert (info["inserted"], info["rebuilt"]) == (3, 0) and sum(info[k] for k in PLACED) == 0
        where = check_lookup(ctx, truth, absent=[b"shor", b"z" * 55])
        assert [where[k] for k in odd] == [3, 3, 3]
        ctx.submit(data, loffs)
        assert_counts(ctx.drain_buckets(), ctx.stats(), want, wst)


# 10
def test_errors(small_map):
    g, ads, camp, raw, offs, _ = small_map
    lib = _lib.lib()
    assert lib.ysb_upsert_info_size() == _lib.C.sizeof(_lib.YsbUpsertInfo)
    assert lib.ysb_admap_desc_size() == _lib.C.sizeof(_lib.YsbAdmapDesc)
    with YsbContext(n_campaigns=100, **SMALL) as ctx:
        for call in (lambda: ctx.upsert_ad_map(ads[:1], camp[:1]), lambda: ctx.lookup_ads(ads[:1]), ctx.ad_map_info):
            with pytest.raises(YsbError) as e:
                call()
            assert e.value.code == ERR_STATE and _lib.ERRORS[ERR_STATE] == "YSB_ERR_STATE"
        ctx.load_ad_map(ads[:600], camp[:600])
        truth = dict(zip(ads[:600], camp[:600]))
        before = ctx.ad_map_info()
        for ids, cs in ((ads[600:610] + [ads[0]], [1] * 10 + [100]),    # a campaign index == n_campaigns
                        (ads[600:610] + ["x" * 57], [1] * 11)):         # a 57-byte id
            with pytest.raises(YsbError) as e:
                ctx.upsert_ad_map(ids, cs)
            assert e.value.code == ERR_FORMAT and _lib.ERRORS[ERR_FORMAT] == "YSB_ERR_FORMAT"
            assert ctx.ad_map_info() == before
            check_lookup(ctx, truth, absent=ads[600:610])
        info = ctx.upsert_ad_map([], [])
        assert info == dict.fromkeys(info, 0)
        assert ctx.ad_map_info() == before
        check_lookup(ctx, truth, absent=ads[600:610])
