"""GPU: the native runner's --lz4 (bin/ysb_topology, batch mode) over the compressed replay file
that bin/ysb_gen --lz4 writes: the same CSV, stats and sink traffic as the uncompressed run on
the same seed, and the runner's refusals."""
import os
import subprocess

import pytest

import golden_data as gd
from fake_redis import FakeRedis
from test_capi import ROOT
from test_gpu_topology import read_csv
from test_redis_sink import dostats_shape
from test_topology import EXE, last_json, write_conf
from ysb_amd import lz4
from ysb_amd.redis_sink import RespClient, check_correct

pytestmark = pytest.mark.gpu

GEN = os.path.join(ROOT, "streaming-benchmarks_amd", "bin", "ysb_gen")
STATS = ("events", "views", "joined", "join_misses", "parse_errors", "time_errors", "out_of_ring", "overflow_dropped")


def run(conf, *extra):
    return subprocess.run([EXE, "--confPath", conf, "--flush-ms", "0"] + list(extra), capture_output=True, text=True,
                          timeout=120)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """ysb_gen --lz4 --tbl: 30,000 events as kafka-json.txt / events.tbl and their .lz4 files."""
    d = tmp_path_factory.mktemp("lz4gen")
    r = subprocess.run([GEN, "-d", str(d), "-n", "30000", "--seed", "11", "--campaigns", "10", "--ads-per-campaign", "10",
                        "--with-skew", "--tbl", "--lz4", "--lz4-block", "4096"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return d


@pytest.mark.parametrize("name,extra", [("kafka-json.txt", []), ("kafka-json.txt", ["--batch-bytes", "70000"]),
                                        ("events.tbl", ["--batch-bytes", "9000"])])
def test_lz4_runner_equals_the_uncompressed_run(dump, tmp_path, name, extra):
    plain = dump / name
    flags, raw_bytes, blocks, directory = lz4.read_file(dump / (name + ".lz4"))
    assert flags & lz4.FILE_LINE_ALIGNED and raw_bytes == plain.stat().st_size and (directory[:, 1] <= 4096).all()
    assert blocks.size < raw_bytes
    admap = str(dump / "ad-to-campaign.csv")
    outs, rows = {}, {}
    for kind, events, opts in (("plain", plain, []), ("lz4", dump / (name + ".lz4"), ["--lz4"])):
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
    assert outs["lz4"]["lz4_comp_bytes"] == blocks.size
    if extra:
        assert outs["lz4"]["batches"] > 2


def test_lz4_runner_golden_through_redis(tmp_path):
    """The golden fixture as a container written through the Python binding: the Redis sink's
    windows read CORRECT, as the uncompressed runner's do."""
    with open(gd.path("gen_s7.jsonl"), "rb") as f:
        data = f.read()
    path = tmp_path / "gen_s7.jsonl.lz4"
    lz4.write_file(path, data, block_bytes=16384, threads=2)
    conf = write_conf(tmp_path, str(path), gd.path("gen_s7.ad_to_campaign.txt"))
    srv = FakeRedis()
    try:
        r = run(conf, "--lz4", "--sink", "redis:127.0.0.1:%d" % srv.port, "--batch-bytes", "100000")
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


@pytest.mark.parametrize("other,word", [("--stream", "--stream"), ("--columns", "--columns"),
                                        ("--from-columns", "--from-columns")])
def test_lz4_refusals(tmp_path, other, word):
    conf = write_conf(tmp_path, gd.path("gen_s7.jsonl"), gd.path("gen_s7.ad_to_campaign.txt"))
    r = run(conf, "--lz4", other)
    assert r.returncode == 2 and "--lz4" in r.stderr and word in r.stderr and len(r.stderr.strip().splitlines()) == 1


def test_lz4_container_must_be_line_aligned_and_a_container(tmp_path):
    with open(gd.path("gen_s7.jsonl"), "rb") as f:
        data = f.read()
    path = tmp_path / "unaligned.lz4"
    lz4.write_file(path, data, block_bytes=4096, line_aligned=False)
    assert not lz4.read_file(path)[0] & lz4.FILE_LINE_ALIGNED
    admap = gd.path("gen_s7.ad_to_campaign.txt")
    r = run(write_conf(tmp_path, str(path), admap), "--lz4")
    assert r.returncode == 1 and "line-aligned" in r.stderr and len(r.stderr.strip().splitlines()) == 1
    r = run(write_conf(tmp_path, gd.path("gen_s7.jsonl"), admap), "--lz4")   # plain lines are no container
    assert r.returncode == 1 and "not a compressed replay file" in r.stderr
