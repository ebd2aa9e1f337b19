"""GPU: the native runner's --kafka --kafka-codec lz4 (slot copies and --io mapped, batch mode)
over the compressed log segment that bin/ysb_gen --kafka --kafka-codec lz4 writes: the same CSV and
stats as the plain run of kafka-json.txt on the same seed; the Python
KafkaLogDataSource(codecs=("lz4",)) on the same file; plain --kafka still refuses the compressed
segment, and the runner with the option refuses a gzip batch by name and byte."""
import subprocess

import pytest

import kafka_lz4_model as Z
import kafka_model as M
from test_gpu_lz4_runner import GEN, STATS, run
from test_gpu_parity import make_ctx
from test_topology import last_json, write_conf
from ysb_amd import KafkaLogDataSource, YsbError, kafka

pytestmark = pytest.mark.gpu

N = 20000


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """ysb_gen --kafka --kafka-batch 16384 --kafka-codec lz4: 20,000 events as kafka-json.txt and a
    compressed kafka-json.log."""
    d = tmp_path_factory.mktemp("kafka_lz4")
    r = subprocess.run([GEN, "-d", str(d), "-n", str(N), "--seed", "11", "--campaigns", "10", "--ads-per-campaign", "10",
                        "--with-skew", "--kafka", "--kafka-batch", "16384", "--kafka-codec", "lz4"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return d


@pytest.fixture(scope="module")
def plain_run(dump, tmp_path_factory):
    sub = tmp_path_factory.mktemp("plain")
    conf = write_conf(sub, str(dump / "kafka-json.txt"), str(dump / "ad-to-campaign.csv"))
    out_csv = sub / "windows.csv"
    r = run(conf, "--sink", "csv:%s" % out_csv)
    assert r.returncode == 0, r.stderr
    with open(out_csv) as f:
        return last_json(r), sorted(f.read().splitlines())


def test_gen_writes_a_compressed_segment_the_model_reads(dump):
    blob = (dump / "kafka-json.log").read_bytes()
    txt = (dump / "kafka-json.txt").read_bytes()
    mi, mf, mb, info = Z.index(blob, check_crc=True)      # the model checks every CRC over the wire bytes
    assert info["n_records"] == N and info["consumed"] == len(blob) and info["compressed_batches"] == len(mi) > 100
    assert all(n == 1 and codec == 3 for _, n, codec in mf)   # a 16 KiB batch is one block
    assert [b["base_offset"] for b in mi] == [b["first_record"] for b in mi]
    lines = txt.split(b"\n")
    assert Z.unframe(blob, mi[:40], mf[:40], mb)[0] == b"".join(lines[:mi[40]["first_record"]])   # (pure Python: the first 40)
    idx, fr, bl, _ = kafka.index_lz4(blob, check_crc=True)
    assert kafka.unframe_lz4_host(blob, idx, fr, bl)[0].tobytes() == b"".join(lines)
    assert len(blob) < 0.8 * len(txt)                      # the events compress


@pytest.mark.parametrize("io", [[], ["--io", "mapped"]])
@pytest.mark.parametrize("extra", [[], ["--batch-bytes", "524288"]])
def test_kafka_lz4_runner_equals_the_plain_run(dump, plain_run, tmp_path, io, extra):
    """Runs cut by the capacity rule at the default slot and at a 512 KiB slot (eight Kafka batches
    per slot batch): CSV rows and stats equal the plain run's."""
    want, want_rows = plain_run
    conf = write_conf(tmp_path, str(dump / "kafka-json.log"), str(dump / "ad-to-campaign.csv"))
    out_csv = tmp_path / "windows.csv"
    r = run(conf, "--kafka", "--kafka-codec", "lz4", "--sink", "csv:%s" % out_csv, *(io + extra))
    assert r.returncode == 0, r.stderr
    out = last_json(r)
    with open(out_csv) as f:
        assert sorted(f.read().splitlines()) == want_rows and len(want_rows) > 1
    for k in STATS:
        assert out[k] == want[k], k
    assert out["events"] == N and out["kafka"] is True and out["kafka_records"] == N and out["kafka_codec"] == "lz4"
    assert out["kafka_io"] == ("mapped" if io else "slot")
    assert out["kafka_framed_bytes"] == (dump / "kafka-json.log").stat().st_size
    assert out["kafka_compressed_batches"] == out["kafka_batches"] > 100
    assert out["kafka_inflated_bytes"] > out["kafka_framed_bytes"]
    if extra:
        assert out["batches"] >= out["kafka_batches"] // 8


def test_python_source_counts_the_compressed_segment(dump, plain_run):
    want, _ = plain_run
    ids = [l.split(",") for l in (dump / "ad-to-campaign.csv").read_text().splitlines() if l]
    camps = sorted({c for _, c in ids})
    with pytest.raises(YsbError) as e:
        KafkaLogDataSource(dump / "kafka-json.log")
    assert "codec = 3" in str(e.value)
    with make_ctx(n_campaigns=len(camps), ads=([a for a, _ in ids], [camps.index(c) for _, c in ids]),
                  max_batch_bytes=1 << 20) as c, KafkaLogDataSource(dump / "kafka-json.log", check_crc=True,
                                                                    codecs=("lz4",)) as src:
        assert src.run(c, 1 << 20) == src.size and src.batches > 4
        st = c.stats()
        assert c.kafka_lz4_info()["calls"] == src.batches
    for k in STATS:
        assert st[k] == want[k], k


def test_plain_kafka_still_refuses_and_the_option_refuses_gzip(dump, tmp_path):
    conf = write_conf(tmp_path, str(dump / "kafka-json.log"), str(dump / "ad-to-campaign.csv"))
    r = run(conf, "--kafka")
    assert r.returncode == 1 and "codec = 3" in r.stderr and "at byte 0" in r.stderr
    blob = bytearray((dump / "kafka-json.log").read_bytes()[:200000])
    idx, _, _, _ = kafka.index_lz4(bytes(blob))
    at = int(idx[2]["records_off"]) - M.HEADER
    blob[at + 22] = 1   # a gzip batch
    bad = tmp_path / "bad.log"
    bad.write_bytes(bytes(blob))
    r = run(write_conf(tmp_path, str(bad), str(dump / "ad-to-campaign.csv")), "--kafka", "--kafka-codec", "lz4")
    assert r.returncode == 1 and "codec = 1" in r.stderr and "gzip" in r.stderr and "at byte %d" % at in r.stderr
