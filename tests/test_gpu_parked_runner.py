"""GPU: the native runner's --join-redis (bin/ysb_topology, batch mode) -- the join as
RedisAdCampaignCache runs it: an empty map file, the `<ad_id> -> campaign_id` strings and the
`campaigns` set in Redis (core.clj:160, :213), every batch's unknown ads looked up with GET,
upserted and resolved.  The windows are read back through Redis as the topology test reads
them (check-correct)."""
import subprocess
from collections import defaultdict

import pytest

import golden_data as gd
import parked_model as pm
from fake_redis import FakeRedis
from test_redis_sink import dostats_shape
from test_topology import EXE, last_json, write_conf
from ysb_amd.redis_sink import RespClient, check_correct

pytestmark = pytest.mark.gpu


def seeded_redis(without=()):
    """A server holding what the generator's setup writes: SET ad campaign per ad (but those in
    `without`), SADD campaigns."""
    srv = FakeRedis()
    cli = RespClient("127.0.0.1", srv.port)
    with open(gd.path("gen_s7.ad_to_campaign.csv")) as f:
        for ln in f.read().splitlines():
            ad, campaign = ln.split(",")
            if ad not in without:
                cli.execute("SET", ad, campaign)
    for c in gd.campaigns():
        cli.execute("SADD", "campaigns", c)
    return srv, cli


def cold_model():
    """The fixture's views against an empty map: the model with every seen ad parked."""
    raw, offs = gd.events("gen_s7")
    model = pm.ParkedModel({}, capacity=1 << 20)
    model.submit(pm.lines_of(raw, offs))
    return model


def run_join_redis(tmp_path, srv, *extra):
    empty = tmp_path / "empty_map.csv"
    empty.write_bytes(b"")
    conf = write_conf(tmp_path, gd.path("gen_s7.jsonl"), str(empty))
    r = subprocess.run([EXE, "--confPath", conf, "--join-redis", "--sink", "redis:127.0.0.1:%d" % srv.port,
                        "--flush-ms", "0"] + list(extra), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return last_json(r)


@pytest.mark.parametrize("extra", [[], ["--batch-bytes", "20000", "--batch-events", "50", "--io", "mmap"]])
def test_cold_map_fills_itself_from_redis(tmp_path, extra):
    srv, cli = seeded_redis()
    try:
        out = run_join_redis(tmp_path, srv, *extra)
        res = check_correct(cli, dostats_shape())
        assert res and all(s == "CORRECT" for _, _, s, _ in res)
        assert sum(n for _, _, _, n in res) == out["joined"]               # and no window beside them
    finally:
        cli.close()
        srv.close()
    _, st = gd.expected("gen_s7")
    for k, v in st.items():
        assert out[k] == v, k
    assert out["join_redis"] is True and out["parked_missed"] == 0 and out["parked_joined"] > 0
    assert out["parked_found"] == out["parked_keys"] == len(cold_model().keys())   # every ad seen is asked for once
    if extra:
        assert out["join_round_trips"] > 2                                   # many batches, most with new ads


def test_ads_redis_does_not_know_are_join_misses(tmp_path):
    ads, camp = gd.ad_arrays()
    model = cold_model()
    seen = sorted(k.decode() for k in model.keys())
    gone = seen[3], seen[-7]
    model.put([a for a in ads if a not in gone], [c for a, c in zip(ads, camp) if a not in gone])
    model.resolve()
    assert model.stats["join_misses"] > 0
    camps = gd.campaigns()
    want = defaultdict(dict)
    for (c, b), n in model.counts.items():
        want[camps[c]][b] = n
    srv, cli = seeded_redis(without=gone)
    try:
        out = run_join_redis(tmp_path, srv)
        res = check_correct(cli, want)
        assert res and all(s == "CORRECT" for _, _, s, _ in res)
        assert sum(n for _, _, _, n in res) == out["joined"] == model.stats["joined"]
    finally:
        cli.close()
        srv.close()
    for k in ("events", "views", "joined", "join_misses", "parse_errors", "time_errors"):
        assert out[k] == model.stats[k], k
    assert out["parked_missed"] == model.stats["join_misses"] and out["parked_keys"] == len(seen)
    assert out["parked_found"] == len(seen) - 2


def test_a_campaign_outside_the_index_space_ends_the_run(tmp_path):
    srv, cli = seeded_redis()
    try:
        ad = sorted(k.decode() for k in cold_model().keys())[0]          # an ad with views: it is asked for
        cli.execute("SET", ad, "not-a-known-campaign")
        empty = tmp_path / "empty_map.csv"
        empty.write_bytes(b"")
        conf = write_conf(tmp_path, gd.path("gen_s7.jsonl"), str(empty))
        r = subprocess.run([EXE, "--confPath", conf, "--join-redis", "--sink", "redis:127.0.0.1:%d" % srv.port],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "not-a-known-campaign" in r.stderr and ad in r.stderr
    finally:
        cli.close()
        srv.close()
