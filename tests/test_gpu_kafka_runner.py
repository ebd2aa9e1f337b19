"""GPU: the native runner's --kafka and --kafka --io mapped (bin/ysb_topology, batch mode) over
the log segment that bin/ysb_gen --kafka writes: the same CSV and stats as the plain run of
kafka-json.txt on the same seed; the Python KafkaLogDataSource on the same file; a segment the
index refuses is refused with the index's message."""
import subprocess

import pytest

import kafka_model as M
from test_gpu_lz4_runner import GEN, STATS, run
from test_gpu_parity import make_ctx
from test_topology import last_json, write_conf
from ysb_amd import KafkaLogDataSource, kafka

pytestmark = pytest.mark.gpu

N = 20000


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """ysb_gen --kafka --kafka-batch 16384: 20,000 events as kafka-json.txt and kafka-json.log."""
    d = tmp_path_factory.mktemp("kafka")
    r = subprocess.run([GEN, "-d", str(d), "-n", str(N), "--seed", "11", "--campaigns", "10", "--ads-per-campaign", "10",
                        "--with-skew", "--kafka", "--kafka-batch", "16384"], capture_output=True, text=True, timeout=120)
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


def test_gen_writes_a_segment_a_consumer_would_accept(dump):
    blob = (dump / "kafka-json.log").read_bytes()
    txt = (dump / "kafka-json.txt").read_bytes()
    midx, info = M.index(blob, check_crc=True)            # the model checks every CRC
    assert info["n_records"] == N and info["consumed"] == len(blob) and len(midx) > 100
    assert all(b["records_bytes"] + M.HEADER <= 16384 for b in midx)
    assert [b["base_offset"] for b in midx] == [b["first_record"] for b in midx]
    assert M.unframe(blob, midx)[0] == txt.replace(b"\n", b"")
    assert 1.0 < len(blob) / len(txt) < 1.06              # the framing's cost at the producer's default batch size


@pytest.mark.parametrize("io", [[], ["--io", "mapped"]])
@pytest.mark.parametrize("extra", [[], ["--batch-bytes", "100000"]])
def test_kafka_runner_equals_the_plain_run(dump, plain_run, tmp_path, io, extra):
    """One slot batch, and runs of about six Kafka batches per slot batch: CSV rows and stats equal
    the plain run's."""
    want, want_rows = plain_run
    conf = write_conf(tmp_path, str(dump / "kafka-json.log"), str(dump / "ad-to-campaign.csv"))
    out_csv = tmp_path / "windows.csv"
    r = run(conf, "--kafka", "--sink", "csv:%s" % out_csv, *(io + extra))
    assert r.returncode == 0, r.stderr
    out = last_json(r)
    with open(out_csv) as f:
        assert sorted(f.read().splitlines()) == want_rows and len(want_rows) > 1
    for k in STATS:
        assert out[k] == want[k], k
    assert out["events"] == N and out["kafka"] is True and out["kafka_records"] == N
    assert out["kafka_io"] == ("mapped" if io else "slot")
    assert out["kafka_framed_bytes"] == (dump / "kafka-json.log").stat().st_size
    if extra:
        assert out["batches"] > 20


def test_python_source_counts_the_segment(dump, plain_run):
    want, _ = plain_run
    ids = [l.split(",") for l in (dump / "ad-to-campaign.csv").read_text().splitlines() if l]
    camps = sorted({c for _, c in ids})
    with make_ctx(n_campaigns=len(camps), ads=([a for a, _ in ids], [camps.index(c) for _, c in ids]),
                  max_batch_bytes=1 << 20) as c, KafkaLogDataSource(dump / "kafka-json.log", check_crc=True) as src:
        assert src.run(c, 1 << 20) == src.size and src.batches > 4
        st = c.stats()
    for k in STATS:
        assert st[k] == want[k], k


def test_runner_refuses_what_the_index_refuses(dump, tmp_path):
    blob = bytearray((dump / "kafka-json.log").read_bytes()[:200000])
    idx, _ = kafka.index(bytes(blob))
    at = int(idx[2]["records_off"]) - M.HEADER
    blob[at + 22] = 3   # an LZ4 batch
    bad = tmp_path / "bad.log"
    bad.write_bytes(bytes(blob))
    r = run(write_conf(tmp_path, str(bad), str(dump / "ad-to-campaign.csv")), "--kafka")
    assert r.returncode == 1 and "codec = 3" in r.stderr and "at byte %d" % at in r.stderr
