"""GPU: the native runner's --lz4 and --lz4 --io mapped (bin/ysb_topology, batch mode) over the
standard LZ4 frame that bin/ysb_gen --lz4-frame writes: the same CSV, stats and Redis traffic as
the uncompressed run on the same seed; a frame the library does not take is refused with the
index's message."""
import os
import subprocess

import pytest

import golden_data as gd
from fake_redis import FakeRedis
from test_capi import ROOT
from test_gpu_lz4_runner import GEN, STATS, run
from test_redis_sink import dostats_shape
from test_topology import last_json, write_conf
from ysb_amd import lz4
from ysb_amd.redis_sink import RespClient, check_correct

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """ysb_gen --lz4-frame --tbl: 30,000 events as kafka-json.txt / events.tbl and their .lz4 frames."""
    d = tmp_path_factory.mktemp("lz4frame")
    r = subprocess.run([GEN, "-d", str(d), "-n", "30000", "--seed", "11", "--campaigns", "10", "--ads-per-campaign", "10",
                        "--with-skew", "--tbl", "--lz4-frame"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return d


@pytest.mark.parametrize("io", [[], ["--io", "mapped"]])
@pytest.mark.parametrize("name,extra", [("kafka-json.txt", []), ("kafka-json.txt", ["--batch-bytes", "300000"]),
                                        ("events.tbl", ["--batch-bytes", "140000"])])
def test_frame_runner_equals_the_uncompressed_run(dump, tmp_path, name, extra, io):
    """One batch, runs of three blocks and one block per batch (MORE on all but the last: lines
    straddle every batch edge): CSV rows and stats equal the uncompressed run's."""
    plain = dump / name
    frame = (dump / (name + ".lz4")).read_bytes()
    assert lz4.is_frame(frame)
    index, info = lz4.frame_index(frame)
    raw_bytes = plain.stat().st_size
    assert info["frames"] == 1 and info["content_bytes"] == raw_bytes and index.size == -(-raw_bytes // 65536)
    assert len(frame) < raw_bytes
    admap = str(dump / "ad-to-campaign.csv")
    outs, rows = {}, {}
    for kind, events, opts in (("plain", plain, []), ("lz4", dump / (name + ".lz4"), ["--lz4"] + io)):
        sub = tmp_path / kind
        sub.mkdir()
        conf = write_conf(sub, str(events), admap)
        out_csv = sub / "windows.csv"
        r = run(conf, "--sink", "csv:%s" % out_csv, *(opts + extra))
        assert r.returncode == 0, r.stderr
        outs[kind] = last_json(r)
        with open(out_csv) as f:
            rows[kind] = sorted(f.read().splitlines())
    assert rows["lz4"] == rows["plain"] and len(rows["plain"]) > 1
    for k in STATS:
        assert outs["lz4"][k] == outs["plain"][k], k
    assert outs["plain"]["events"] == 30000 and outs["lz4"]["format"] == outs["plain"]["format"]
    assert outs["lz4"]["lz4"] is True and outs["lz4"]["lz4_raw_bytes"] == raw_bytes
    assert outs["lz4"]["lz4_io"] == ("mapped" if io else "slot")
    if extra:
        per = (int(extra[1]) // 65536) - 1
        assert outs["lz4"]["batches"] == -(-index.size // per) > 2


@pytest.mark.parametrize("io", [[], ["--io", "mapped"]])
def test_frame_runner_golden_through_redis(tmp_path, io):
    """The golden fixture as a frame of 4096-byte blocks written through the Python binding, and
    the liblz4-made fixture frame's own lines: the Redis sink's windows read CORRECT, as the
    uncompressed runner's do; the stats are the golden expectations."""
    with open(gd.path("gen_s7.jsonl"), "rb") as f:
        data = f.read()
    path = tmp_path / "gen_s7.jsonl.lz4"
    lz4.frame_write(path, data, block_bytes=4096, threads=2)
    conf = write_conf(tmp_path, str(path), gd.path("gen_s7.ad_to_campaign.txt"))
    srv = FakeRedis()
    try:
        r = run(conf, "--lz4", "--sink", "redis:127.0.0.1:%d" % srv.port, "--batch-bytes", "200000", *io)
        assert r.returncode == 0, r.stderr
        cli = RespClient("127.0.0.1", srv.port)
        res = check_correct(cli, dostats_shape())
        cli.close()
        assert res and all(s == "CORRECT" for _, _, s, _ in res)
    finally:
        srv.close()
    out = last_json(r)
    for k, v in gd.expected("gen_s7")[1].items():
        assert out[k] == v, k
    assert out["batches"] > 2


def test_frame_runner_refuses_what_the_index_refuses(tmp_path):
    admap = gd.path("gen_s7.ad_to_campaign.txt")
    linked = os.path.join(ROOT, "tests", "golden", "lz4frame", "small_linked.lz4")
    r = run(write_conf(tmp_path, linked, admap), "--lz4")
    assert r.returncode == 1 and "lz4 -BI" in r.stderr and "byte 4" in r.stderr
