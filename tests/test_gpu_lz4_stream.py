"""GPU: the native runner with compressed bytes read in place (ysb_submit_lz4_mapped) -- the
streaming replay's --stream-lz4 (host/ysb_replay_lz4.hpp: the cycle compressed batch by batch,
registered in place of the raw one) exact against the generator truth like the uncompressed
stream, its refusals, and the file runner's --lz4 --io mapped over the containers bin/ysb_gen
--lz4 writes against the uncompressed run."""
import os
import subprocess
import sys

import pytest

from test_capi import ROOT
from test_gpu_lz4_runner import GEN, STATS, run
from test_topology import EXE, last_json, write_conf
from ysb_amd import lz4

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("replay,shards,skew", [("mapped", 1, 2), ("mapped-raw", 1, 2), ("mapped", 2, 1)])
def test_compressed_stream_is_exact(replay, shards, skew):
    """test_native_stream_mode_exact's run and assertions with the cycle compressed: a 2 M-line
    cycle played three times (the rebase on decoded bytes at two cycle wraps), every (campaign,
    window) read back through Redis equal to the generator truth; fewer bytes per event cross
    the link than a raw line holds."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_stream
    r = bench_stream.stream_native(device=0, seconds=1.5, speedup=20.0, event_rate=200_000, slot_mb=16, batch_ms=100,
                                   shards=shards, skew=skew, threads=8, replay=replay, stream_lz4=True)
    c = r["check"]
    print({k: r[k] for k in ("events_per_s", "pcie_bytes_per_event", "raw_bytes_per_event", "copy_busy_frac",
                             "lz4_comp_bytes_per_cycle", "lz4_raw_bytes_per_cycle")}, r["runner"]["cycles"])
    assert r["replay"] == replay and r["stream_lz4"] is True and r["lz4_block"] == 8192
    assert r["exact_vs_generator_truth"], c
    assert c["truth_mismatched_cells"] == 0 and c["counted_views"] == c["truth_views"] > 0
    assert c["parse_errors"] == 0 and c["join_misses"] == 0 and c["overflow_dropped"] == 0
    assert r["flushes"] >= 20 and r["windows_closed"] >= 1
    assert 100 <= r["get_stats"]["samples_closed_windows"] <= 100 * r["windows_closed"]
    assert len(r["runner"]["cycles"]) == shards and min(r["runner"]["cycles"]) >= 2   # two cycle wraps at least
    assert 0 < r["lz4_comp_bytes_per_cycle"] < r["lz4_raw_bytes_per_cycle"]
    assert 0 < r["pcie_bytes_per_event"] < r["raw_bytes_per_event"]


@pytest.mark.parametrize("args,word", [(["--stream-lz4"], "--stream"),
                                       (["--stream", "--stream-lz4", "--replay", "copy"], "--replay copy")])
def test_stream_lz4_refusals(args, word):
    r = subprocess.run([EXE] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--stream-lz4" in r.stderr and word in r.stderr
    assert len(r.stderr.strip().splitlines()) == 1 and not r.stdout


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """ysb_gen --lz4 --tbl: 30,000 events as kafka-json.txt / events.tbl and their .lz4 files."""
    d = tmp_path_factory.mktemp("lz4gen_mapped")
    r = subprocess.run([GEN, "-d", str(d), "-n", "30000", "--seed", "11", "--campaigns", "10", "--ads-per-campaign", "10",
                        "--with-skew", "--tbl", "--lz4", "--lz4-block", "4096"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return d


@pytest.mark.parametrize("name,batch_bytes", [("kafka-json.txt", 13000), ("events.tbl", 9000)])
def test_file_runner_in_place_equals_the_uncompressed_run(dump, tmp_path, name, batch_bytes):
    """--lz4 --io mapped: the container mapped and registered, runs of 1-3 blocks of 4 KiB
    submitted where they lie; CSV rows and stats equal the uncompressed run's."""
    plain = dump / name
    flags, raw_bytes, blocks, directory = lz4.read_file(dump / (name + ".lz4"))
    assert flags & lz4.FILE_LINE_ALIGNED and raw_bytes == plain.stat().st_size
    admap = str(dump / "ad-to-campaign.csv")
    outs, rows = {}, {}
    for kind, events, opts in (("plain", plain, []), ("mapped", dump / (name + ".lz4"), ["--lz4", "--io", "mapped"]),
                               ("slot", dump / (name + ".lz4"), ["--lz4"])):
        sub = tmp_path / kind
        sub.mkdir()
        conf = write_conf(sub, str(events), admap)
        out_csv = sub / "windows.csv"
        r = run(conf, "--sink", "csv:%s" % out_csv, "--batch-bytes", str(batch_bytes), *opts)
        assert r.returncode == 0, r.stderr
        outs[kind] = last_json(r)
        with open(out_csv) as f:
            rows[kind] = sorted(f.read().splitlines())
    assert rows["mapped"] == rows["plain"] and len(rows["plain"]) > 1
    for k in STATS:
        assert outs["mapped"][k] == outs["plain"][k], k
    assert outs["plain"]["events"] == 30000 and outs["mapped"]["format"] == outs["plain"]["format"]
    assert outs["mapped"]["lz4"] is True and outs["mapped"]["lz4_io"] == "mapped" and outs["slot"]["lz4_io"] == "slot"
    assert outs["mapped"]["lz4_comp_bytes"] == blocks.size and outs["mapped"]["lz4_raw_bytes"] == raw_bytes
    # runs of one to three blocks: a 4 KiB block always fits, a fourth never does
    n = directory.shape[0]
    assert n / 3 <= outs["mapped"]["batches"] <= n and outs["mapped"]["batches"] == outs["slot"]["batches"]
