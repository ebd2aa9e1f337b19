"""CPU: the parked views' model (tests/parked_model.py) against oracle.run on the full map --
park with a map that lacks ads, put them, resolve: the counts and stats of a run whose map was
complete from the start -- on the generator fixture and on the hand-written edge fixtures
(escapes, bad times, other key lengths)."""
import pytest

import golden_data as gd
import parked_model as pm
from oracle import oracle
from ysb_amd import ad_shard

ORACLE_STATS = ("events", "views", "joined", "join_misses", "parse_errors", "time_errors")


def full_map():
    ads, camp = gd.ad_arrays()
    return dict(zip(ads, camp))


def oracle_on(ad_map, raw, offs):
    return oracle.run(oracle.AdMap(list(ad_map), list(ad_map.values())), raw, offs)


def invariant(m):
    s = m.stats
    assert s["views"] == s["joined"] + s["join_misses"] + s["foreign_shard"] + len(m.log)


@pytest.mark.parametrize("stem", ["gen_s7", "edge", "edge_orgjson", "edge_long"])
@pytest.mark.parametrize("known", ["none", "half"])
def test_park_then_resolve_equals_the_full_map(stem, known):
    raw, offs = gd.events(stem)
    lines = pm.lines_of(raw, offs)
    full = full_map()
    want, wst = oracle_on(full, raw, offs)
    start = {} if known == "none" else dict(list(full.items())[::2])
    m = pm.ParkedModel(start, capacity=len(lines))
    m.submit(lines)
    invariant(m)
    partial, pst = oracle_on(start, raw, offs)
    # before the resolve: exactly what the partial map joins; every other keyed view is parked
    assert m.counts == partial and m.stats["joined"] == pst["joined"]
    assert m.stats["join_misses"] + len(m.log) == pst["join_misses"]
    assert all(len(k) <= 56 and k not in m.map for k in m.keys())
    found = {k: c for k, c in full.items() if pm.key_bytes(k) in m.keys()}   # what the lookup knows
    m.put(list(found), list(found.values()))
    info = m.resolve()
    invariant(m)
    assert m.counts == want and not m.log
    for k in ORACLE_STATS:
        assert m.stats[k] == wst[k], k
    assert info["resolved_joined"] + info["resolved_missed"] == m.parked_total
    assert m.info()["parked"] == 0 and m.info()["dropped"] == 0


def test_three_kinds_of_ad_and_a_full_log():
    raw, offs = gd.events("gen_s7")
    lines = pm.lines_of(raw, offs)
    ads = list(full_map().items())
    known, redis, nowhere = dict(ads[:50]), dict(ads[50:75]), dict(ads[75:])
    want, wst = oracle_on({**known, **redis}, raw, offs)
    m = pm.ParkedModel(known, capacity=len(lines))
    m.submit(lines)
    assert m.keys() and m.keys() <= {pm.key_bytes(a) for a in {**redis, **nowhere}}
    m.put(list(redis), list(redis.values()))
    m.resolve()
    assert m.counts == want
    for k in ORACLE_STATS:
        assert m.stats[k] == wst[k], k
    assert m.stats["join_misses"] == oracle_on(nowhere, raw, offs)[1]["joined"] > 0

    # capacity 7: the first 7 unknown-ad views park, the rest are join misses and dropped
    m = pm.ParkedModel(known, capacity=7)
    m.submit(lines)
    unknown = oracle_on(known, raw, offs)[1]["join_misses"]
    assert (len(m.log), m.dropped, m.stats["join_misses"]) == (7, unknown - 7, unknown - 7)
    invariant(m)
    # parking off: the oracle on the map as it is
    m = pm.ParkedModel(known, capacity=0)
    m.submit(lines)
    got, gst = oracle_on(known, raw, offs)
    assert m.counts == got and all(m.stats[k] == gst[k] for k in ORACLE_STATS) and not m.log


def test_sharded_model_parks_its_own_keys_only():
    raw, offs = gd.events("gen_s7")
    lines = pm.lines_of(raw, offs)
    full = full_map()
    mine = {a: c for a, c in full.items() if ad_shard(a, 2) == 0}
    assert 0 < len(mine) < len(full)
    m = pm.ParkedModel({}, capacity=len(lines), shard=(0, 2))
    m.submit(lines)
    invariant(m)
    assert m.keys() and m.keys() <= {pm.key_bytes(a) for a in mine}
    assert m.stats["foreign_shard"] == oracle_on({a: c for a, c in full.items() if a not in mine}, raw, offs)[1]["joined"]
    m.put(list(mine), list(mine.values()))
    m.resolve()
    assert m.counts == oracle_on(mine, raw, offs)[0] and m.stats["join_misses"] == 0
