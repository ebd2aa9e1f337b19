"""GPU: parked views (ysb_parked_enable / _keys / _resolve / _info) -- the views of ads the
device tables do not hold, parked at the deferred-line kernel's and the columnar count's miss,
their distinct keys, and the resolve after an upsert.  Expectations come from the plain model
(tests/parked_model.py), from the oracle on the full map and from a fresh context loaded with
the full map."""
import ctypes as C

import numpy as np
import pytest

import parked_model as pm
from oracle import oracle
from ysb_amd import GenParams, YsbContext, YsbError, _lib
from ysb_amd.generator import json_to_tbl

pytestmark = pytest.mark.gpu

ERR_STATE, ERR_CAPACITY = -3, -4   # include/ysb_hip.h YSB_ERR_STATE, YSB_ERR_CAPACITY
SMALL = dict(window_ring=16, max_batch_events=1 << 15, max_batch_bytes=8 << 20, overflow_capacity=1 << 12)
PATHS = ("submit", "device", "tbl", "columns")
SAME = ("events", "views", "joined", "join_misses", "time_errors", "out_of_ring")
NC = 8


def context(path="submit", n_campaigns=NC, **kw):
    return YsbContext(n_campaigns=n_campaigns, input_format="tbl" if path == "tbl" else "json", **dict(SMALL, **kw))


def send(ctx, path, raw, offs):
    """The batch through one of the four paths (columns: decoded on the device, with validity)."""
    if path == "submit":
        ctx.submit(raw, offs)
    elif path == "tbl":
        ctx.submit(*json_to_tbl(raw, offs))
    elif path == "device":
        d_b, d_o = ctx.device_alloc(raw.size), ctx.device_alloc(4 * offs.size)
        ctx.h2d(d_b, raw)
        ctx.h2d(d_o, offs)
        ctx.submit_device(d_b, raw.size, d_o, offs.size)
        ctx.sync()
        ctx.device_free(d_b)
        ctx.device_free(d_o)
    else:
        image, valid, _ = ctx.decode_columns(raw, offs)
        assert valid.all()
        d = ctx.device_alloc(image.size)
        ctx.h2d(d, image)
        ctx.submit_columns_device(d, offs.size, offs.size, _lib.YSB_COL_VALIDITY)
        ctx.sync()
        ctx.device_free(d)


def fresh(path, ads, camp, raw, offs, n_campaigns=NC, **kw):
    """(drained buckets, stats) of a context loaded with the whole map, parking off."""
    with context(path, n_campaigns, **kw) as ctx:
        ctx.load_ad_map(ads, camp)
        send(ctx, path, raw, offs)
        return ctx.drain_buckets(), ctx.stats()


def same_stats(st, want, keys=SAME):
    for k in keys:
        assert st[k] == want[k], (k, st[k], want[k])


def invariant(ctx):
    st, info = ctx.stats(), ctx.parked_info()
    assert st["views"] == st["joined"] + st["join_misses"] + st["foreign_shard"] + info["parked"]
    return st, info


def batch_of(lines):
    data = np.frombuffer(b"".join(lines), dtype=np.uint8)
    offs = np.cumsum([0] + [len(l) for l in lines[:-1]]).astype(np.uint32)
    return data, offs


def with_ad(line, ad_id):
    at = line.index(b'"ad_id": "') + 10
    return line[:at] + ad_id + line[line.index(b'"', at):]


def with_time(line, text):
    at = line.index(b'"event_time": "') + 15
    return line[:at] + text + line[line.index(b'"', at):]


def is_view(line):
    return b'"event_type": "view"' in line


@pytest.fixture(scope="module")
def small():
    """8 campaigns x 5 ads, 3,000 skewed events over four windows, the oracle on the full map."""
    g = GenParams(seed=8, n_campaigns=NC, ads_per_campaign=5, events_per_sec=100, with_skew=True)
    _, ads = g.ids()
    camp = g.ad_campaign_index()
    raw, offs = g.events_host(0, 3000)
    want, wst = oracle.run(oracle.AdMap(ads, camp), raw, offs)
    assert len({b for _, b in want}) >= 3 and wst["join_misses"] == 0
    return g, ads, camp, raw, offs, want, wst


# 1
@pytest.mark.parametrize("path", PATHS)
def test_cold_start(small, path):
    g, ads, camp, raw, offs, want, wst = small
    model = pm.ParkedModel({}, capacity=4096)
    model.submit(pm.lines_of(raw, offs))
    with context(path) as ctx:
        ctx.load_ad_map([], [])
        ctx.park_misses(4096)
        send(ctx, path, raw, offs)
        st, info = invariant(ctx)
        assert st["joined"] == st["join_misses"] == 0 and info["parked"] == st["views"] == wst["views"]
        assert (info["capacity"], info["dropped"], info["parked_total"]) == (4096, 0, st["views"])
        assert ctx.drain_buckets() == {}
        keys = ctx.parked_keys()
        assert len(keys) == len(set(keys)) and set(keys) == model.keys()
        assert ctx.parked_info()["distinct_keys"] == len(keys)
        ctx.upsert_ad_map(ads, camp)
        info = ctx.resolve_parked()
        assert (info["resolved_joined"], info["resolved_missed"], info["parked"]) == (wst["views"], 0, 0)
        assert info["resolve_ms"] > 0 and info["parked_total"] == wst["views"]
        got, st = ctx.drain_buckets(), ctx.stats()
        assert ctx.parked_keys() == [] and ctx.parked_info()["parked"] == 0
        # the base a resolve fixes: the smallest bucket it counted minus W / 8
        assert ctx.ring_range() == (min(b for _, b in want) - 2, 16)
    assert got == want
    ref, rst = fresh(path, ads, camp, raw, offs)
    assert ref == want
    same_stats(st, rst)
    assert st["time_errors"] == 0 and st["overflow_dropped"] == 0


# 2
@pytest.mark.parametrize("path", ["submit", "columns"])
def test_three_kinds_of_ad(small, path):
    g, ads, camp, raw, offs, _, _ = small
    known, redis, nowhere = slice(0, 20), slice(20, 30), slice(30, 40)
    have = dict(zip(ads[:30], camp[:30]))
    want, wst = oracle.run(oracle.AdMap(list(have), list(have.values())), raw, offs)
    lost = oracle.run(oracle.AdMap(ads[nowhere], camp[nowhere]), raw, offs)[1]["joined"]
    assert lost > 0
    with context(path) as ctx:
        ctx.load_ad_map(ads[known], camp[known])
        ctx.park_misses(4096)
        send(ctx, path, raw, offs)
        st, info = invariant(ctx)
        assert st["join_misses"] == 0 and info["parked"] == st["views"] - st["joined"] > lost
        assert set(ctx.parked_keys()) == {a.encode() for a in ads[20:]}
        redis_map = dict(zip((a.encode() for a in ads[redis]), camp[redis]))
        info = ctx.resolve_parked_with(lambda keys: [redis_map.get(k) for k in keys])
        assert info["resolved_missed"] == lost and info["parked"] == 0
        st, _ = invariant(ctx)
        assert ctx.drain_buckets() == want
        same_stats(st, wst, ("events", "views", "joined", "join_misses", "time_errors"))
        assert st["join_misses"] == lost
        _, where = ctx.lookup_ads(ads)
        assert (where[:30] != 0).all() and (where[30:] == 0).all()   # null from the lookup: nothing cached


# 3
def test_hand_written_lines(small):
    g, ads, camp, raw, offs, _, _ = small
    views = [l for l in pm.lines_of(raw, offs) if is_view(l)]
    found, lost = b"F" * 36, b"L" * 36
    escaped = b"\\u0065sc\\u0061ped-" + b"e" * 28                       # "escaped-eeee...": 36 bytes decoded
    one, wide, too_wide = b"1", b"w" * 56, b"W" * 57
    lines = [with_ad(views[0], found),
             with_time(with_ad(views[1], found), b"12x45"),            # found later: a time error then
             with_time(with_ad(views[2], lost), b"nope"),              # never found: a join miss, time unseen
             with_ad(views[3], lost),
             with_ad(views[4], escaped),
             with_time(with_ad(views[5], escaped), b"+1700000000000"),
             with_ad(views[6], one), with_ad(views[7], wide), with_ad(views[8], too_wide),
             with_time(with_ad(views[9], one), b"9223372036854775808"),   # 2^63: parseLong rejects it
             views[10]]                                                   # a known ad
    data, loffs = batch_of(lines)
    decoded = b"escaped-" + b"e" * 28
    redis = {found: 1, decoded: 2, one: 3, wide: 4, too_wide: 5}
    model = pm.ParkedModel(dict(zip(ads, camp)), capacity=64)
    model.submit(lines)
    assert model.keys() == {found, lost, decoded, one, wide} and model.stats["join_misses"] == 1
    with context() as ctx:
        ctx.load_ad_map(ads, camp)
        ctx.park_misses(64)
        ctx.submit(data, loffs)
        st, info = invariant(ctx)
        assert (info["parked"], st["join_misses"], st["time_errors"], st["joined"]) == (9, 1, 0, 1)
        assert set(ctx.parked_keys()) == model.keys()                  # the escaped id parks decoded, 57 bytes never
        model.put([k for k in redis if len(k) <= 56], [c for k, c in redis.items() if len(k) <= 56])
        model.resolve()
        info = ctx.resolve_parked_with(lambda keys: [redis.get(k) for k in keys])
        assert (info["resolved_joined"], info["resolved_missed"], info["resolved_time_errors"]) == (7, 2, 2)
        assert info == dict(info, **model.last)
        st, _ = invariant(ctx)
        same_stats(st, model.stats, pm.STATS)
        assert ctx.drain_buckets() == model.counts
        assert (st["join_misses"], st["time_errors"]) == (3, 2)


# 4
@pytest.mark.parametrize("path", ["submit", "columns"])
@pytest.mark.parametrize("k", [1, 63, 64, 65, 129])
def test_wave_edges(small, path, k):
    g, ads, camp, raw, offs, _, _ = small
    lines = pm.lines_of(raw, offs)[:640]
    unknown = "0badc0de-0000-4000-8000-%012d" % k
    at = [i for i, l in enumerate(lines) if is_view(l) and i >= 40][:k]   # from inside tile 0 across its end
    assert len(at) == k and at[0] < 64 and (k == 1 or at[-1] >= 64)
    for i in at:
        lines[i] = with_ad(lines[i], unknown.encode())
    data, loffs = batch_of(lines)
    full = dict(zip(ads + [unknown], camp + [3]))
    want, wst = oracle.run(oracle.AdMap(list(full), list(full.values())), data, loffs)
    with context(path) as ctx:
        ctx.load_ad_map(ads, camp)
        ctx.park_misses(256)
        send(ctx, path, data, loffs)
        st, info = invariant(ctx)
        assert info["parked"] == k and st["join_misses"] == 0 and info["dropped"] == 0
        assert ctx.parked_keys() == [unknown.encode()]
        ctx.upsert_ad_map([unknown], [3])
        info = ctx.resolve_parked()
        assert (info["resolved_joined"], info["resolved_missed"], info["parked"]) == (k, 0, 0)
        st, _ = invariant(ctx)
        assert ctx.drain_buckets() == want                             # no record lost or doubled
        same_stats(st, wst, ("events", "views", "joined", "join_misses", "time_errors"))


# 5
@pytest.mark.parametrize("capacity", [1, 64])
def test_capacity(small, capacity):
    g, ads, camp, raw, offs, _, _ = small
    lines = pm.lines_of(raw, offs)[:900]
    at = [i for i, l in enumerate(lines) if is_view(l)][:200]
    assert len(at) == 200
    for n, i in enumerate(at):
        lines[i] = with_ad(lines[i], b"unknown-ad-%02d" % (n % 7))
    data, loffs = batch_of(lines)
    with context() as ctx:
        ctx.load_ad_map(ads, camp)
        ctx.park_misses(capacity)
        ctx.submit(data, loffs)
        with pytest.raises(YsbError) as e:
            ctx.sync()
        assert e.value.code == ERR_CAPACITY and _lib.ERRORS[ERR_CAPACITY] == "YSB_ERR_CAPACITY"
        st, info = invariant(ctx)
        assert (info["parked"], info["dropped"], st["join_misses"]) == (capacity, 200 - capacity, 200 - capacity)
        assert len(ctx.parked_keys()) <= min(capacity, 7)
        info = ctx.resolve_parked()                                     # still works; the loss stays told
        assert (info["parked"], info["resolved_missed"], info["dropped"]) == (0, capacity, 200 - capacity)
        with pytest.raises(YsbError) as e:
            ctx.sync()
        assert e.value.code == ERR_CAPACITY
        ctx.reset()
        ctx.sync()
        assert ctx.parked_info() == dict(ctx.parked_info(), capacity=capacity, parked=0, parked_total=0, dropped=0)
        one, ooffs = batch_of([lines[at[0]], next(l for i, l in enumerate(lines) if i not in at)])
        ctx.submit(one, ooffs)
        ctx.sync()
        st, info = invariant(ctx)
        assert (info["parked"], info["dropped"], info["parked_total"], st["join_misses"]) == (1, 0, 1, 0)


# 6
def test_two_batches_then_one_resolve(small):
    g, ads, camp, _, _, _, _ = small
    batches = [g.events_host(1500 * i, 1500) for i in range(3)]
    model = pm.ParkedModel(dict(zip(ads[:10], camp[:10])), capacity=4096)
    with context() as ctx:
        ctx.load_ad_map(ads[:10], camp[:10])
        ctx.park_misses(4096)
        for raw, offs in batches[:2]:
            ctx.submit(raw, offs)
            model.submit(pm.lines_of(raw, offs))
        keys = ctx.parked_keys()
        assert len(keys) == len(set(keys)) and set(keys) == model.keys() == {a.encode() for a in ads[10:]}
        assert ctx.parked_info()["parked"] == len(model.log) > len(keys)
        every = dict(zip((a.encode() for a in ads), camp))
        ctx.resolve_parked_with(lambda ks: [every[k] for k in ks])
        model.put(ads, camp)
        model.resolve()
        raw, offs = batches[2]
        ctx.submit(raw, offs)                                           # joins directly now
        model.submit(pm.lines_of(raw, offs))
        st, info = invariant(ctx)
        assert info["parked"] == 0 and info["parked_total"] == model.parked_total and not model.log
        _, where = ctx.lookup_ads(ads)
        assert np.isin(where, (1, 2)).all()
        assert ctx.drain_buckets() == model.counts
        same_stats(st, model.stats, pm.STATS)
    allraw = np.concatenate([b[0] for b in batches])
    alloffs = np.concatenate([b[1] + np.uint32(sum(x[0].size for x in batches[:i])) for i, b in enumerate(batches)])
    assert model.counts == oracle.run(oracle.AdMap(ads, camp), allraw, alloffs)[0]


# 7
@pytest.mark.parametrize("path", ["submit", "columns"])
def test_sharded(small, path):
    from ysb_amd import ad_shard
    g, ads, camp, raw, offs, _, _ = small
    mine = [a for a in ads if ad_shard(a, 2) == 1]
    assert 0 < len(mine) < len(ads)
    model = pm.ParkedModel({}, capacity=4096, shard=(1, 2))
    model.submit(pm.lines_of(raw, offs))
    with context(path) as ctx:
        ctx.load_ad_map([], [], shard=(1, 2))
        ctx.park_misses(4096)
        send(ctx, path, raw, offs)
        st, info = invariant(ctx)
        assert st["foreign_shard"] == model.stats["foreign_shard"] > 0 and info["parked"] == len(model.log) > 0
        keys = ctx.parked_keys()
        assert set(keys) == model.keys() and set(keys) <= {a.encode() for a in mine}
        up = ctx.upsert_ad_map(ads, camp)                               # the other shard's ads are skipped
        assert up["foreign"] == len(ads) - len(mine)
        model.put(mine, [camp[ads.index(a)] for a in mine])
        ctx.resolve_parked()
        model.resolve()
        st, _ = invariant(ctx)
        same_stats(st, model.stats, pm.STATS)
        assert ctx.drain_buckets() == model.counts and st["join_misses"] == 0


# 8
def test_late_views_outside_the_ring(small):
    g, ads, camp, raw, offs, _, _ = small
    lines = pm.lines_of(raw, offs)[:1200]
    late_ad = ads[-1].encode()
    n_late = 0
    for i, l in enumerate(lines):
        if is_view(l) and late_ad in l and i > 300:
            t = int(l[l.index(b'"event_time": "') + 15:].split(b'"')[0])
            lines[i] = with_time(l, b"%d" % (t - 1_000_000 * (1 + n_late % 3)))   # 100, 200, 300 windows back
            n_late += 1
    assert n_late >= 3
    data, loffs = batch_of(lines)
    ref, rst = fresh("submit", ads, camp, data, loffs)
    assert rst["out_of_ring"] == n_late and ref == oracle.run(oracle.AdMap(ads, camp), data, loffs)[0]
    with context() as ctx:
        ctx.load_ad_map(ads[:-1], camp[:-1])
        ctx.park_misses(1024)
        ctx.submit(data, loffs)
        st, info = invariant(ctx)
        assert st["out_of_ring"] == 0 and info["parked"] > n_late
        ctx.upsert_ad_map(ads[-1:], camp[-1:])
        ctx.resolve_parked()
        st, _ = invariant(ctx)
        assert ctx.drain_buckets() == ref
        same_stats(st, rst)


# 9
@pytest.mark.timeout(300)
def test_hbm_table_in_record_mode():
    # the smallest load that gets the bucket layout: more than 2^18 36-byte keys (ysb_admap.h)
    n_campaigns = 132_400
    g = GenParams(seed=13, n_campaigns=n_campaigns, ads_per_campaign=2, events_per_sec=1000, with_skew=True)
    _, ads = g.ids()
    camp = g.ad_campaign_index()
    held = set(range(0, len(ads), 100))                                # 1 % of the ads are withheld
    kept = [i for i in range(len(ads)) if i not in held]
    assert len(kept) == (1 << 18) + 8
    raw, offs = g.events_host(0, 100_000)
    kw = dict(window_ring=16, record_count=True, max_batch_bytes=raw.size + 64, max_batch_events=offs.size + 1)
    with YsbContext(n_campaigns=n_campaigns, **kw) as ctx:
        ctx.load_ad_map(ads, camp)
        ctx.submit(raw, offs)
        ref, rst = ctx.drain_buckets(), ctx.stats()
        assert ctx.launch_info()["record_mode"] == 1
    with YsbContext(n_campaigns=n_campaigns, **kw) as ctx:
        ctx.load_ad_map([ads[i] for i in kept], [camp[i] for i in kept])
        assert ctx.ad_map_info()["buckets"] == 1
        ctx.park_misses(1 << 12)
        ctx.submit(raw, offs)
        st, info = invariant(ctx)
        assert ctx.launch_info()["record_mode"] == 1 and ctx.launch_info()["hbm_table"] == 1
        assert 0 < info["parked"] == rst["joined"] - st["joined"] and st["join_misses"] == 0
        keys = ctx.parked_keys()
        held_ids = {ads[i].encode(): camp[i] for i in held}
        assert set(keys) <= set(held_ids) and len(keys) == len(set(keys))
        info = ctx.resolve_parked_with(lambda ks: [held_ids[k] for k in ks])
        assert info["resolved_missed"] == 0 and info["parked"] == 0
        st, _ = invariant(ctx)
        assert ctx.ad_map_info()["buckets"] == 1
        assert ctx.drain_buckets() == ref
        same_stats(st, rst)


# 10
@pytest.mark.parametrize("path", PATHS)
def test_complete_map_parks_nothing(small, path):
    g, ads, camp, raw, offs, want, _ = small
    ref, rst = fresh(path, ads, camp, raw, offs)
    with context(path) as ctx:
        ctx.load_ad_map(ads, camp)
        ctx.park_misses(64)
        send(ctx, path, raw, offs)
        got, st = ctx.drain_buckets(), ctx.stats()
        info = ctx.resolve_parked()
        assert info["parked_total"] == 0 and info["parked"] == 0 and ctx.parked_keys() == []
        assert ctx.stats() == st
    assert got == ref == want
    same_stats(st, rst, [k for k in rst if k != "deferred"])


# 11
def test_state_errors(small):
    g, ads, camp, raw, offs, _, _ = small
    lib = _lib.lib()
    assert lib.ysb_parked_info_size() == C.sizeof(_lib.YsbParkedDesc)

    def state_error(call):
        with pytest.raises(YsbError) as e:
            call()
        assert e.value.code == ERR_STATE and _lib.ERRORS[ERR_STATE] == "YSB_ERR_STATE"

    def amax(user, data, n):
        return 0

    def rsum(user, send, recv, count, width):
        C.memmove(recv, send, count * width)
        return 0

    ops = _lib.YsbCollectives(_lib.ALLREDUCE_MAX_FN(amax), _lib.REDUCE_SCATTER_FN(rsum), None)
    with context() as ctx:
        state_error(lambda: ctx.park_misses(16))                       # before a load
        assert ctx.parked_info() == dict.fromkeys(ctx.parked_info(), 0)
        state_error(ctx.parked_keys)                                   # parking is off
        state_error(ctx.resolve_parked)
        ctx.load_ad_map(ads[:20], camp[:20])
        ctx.park_misses(4096)
        ctx.submit(raw, offs)
        assert ctx.parked_info()["parked"] > 0
        state_error(lambda: ctx.park_misses(0))                        # records are parked
        state_error(lambda: ctx.park_misses(8192))
        state_error(lambda: ctx._c(lib.ysb_group_init_host(ctx._h, 0, 1, C.byref(ops))))   # parking is enabled
        ctx.resolve_parked()
        ctx.park_misses(0)                                             # now it may go
        assert ctx.parked_info()["capacity"] == 0
        send(ctx, "submit", raw, offs)
        assert ctx.stats()["join_misses"] > 0                          # misses are misses again
        ctx._c(lib.ysb_group_init_host(ctx._h, 0, 1, C.byref(ops)))
        state_error(lambda: ctx.park_misses(16))                       # after a group init
