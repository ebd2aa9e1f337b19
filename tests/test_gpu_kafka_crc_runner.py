"""GPU: the native runner's --kafka-check-crc (bin/ysb_topology --kafka, batch mode) over the log
segment that bin/ysb_gen --kafka writes: `device` and `host` give every counter of the run without
the flag; one flipped bit ends the run with the message that names the batch; the Python
KafkaLogDataSource(check_crc="device") on the same file."""
import subprocess

import pytest

import kafka_model as M
from test_gpu_lz4_runner import GEN, STATS, run
from test_gpu_parity import make_ctx
from test_topology import last_json, write_conf
from ysb_amd import KafkaLogDataSource, YsbError, kafka

pytestmark = pytest.mark.gpu

N = 20000


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    d = tmp_path_factory.mktemp("kafka_crc")
    r = subprocess.run([GEN, "-d", str(d), "-n", str(N), "--seed", "11", "--campaigns", "10", "--ads-per-campaign", "10",
                        "--with-skew", "--kafka", "--kafka-batch", "16384"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return d


@pytest.fixture(scope="module")
def unchecked_run(dump, tmp_path_factory):
    sub = tmp_path_factory.mktemp("off")
    conf = write_conf(sub, str(dump / "kafka-json.log"), str(dump / "ad-to-campaign.csv"))
    out_csv = sub / "windows.csv"
    r = run(conf, "--kafka", "--batch-bytes", "100000", "--sink", "csv:%s" % out_csv)
    assert r.returncode == 0, r.stderr
    with open(out_csv) as f:
        return last_json(r), sorted(f.read().splitlines())


@pytest.mark.parametrize("mode,io", [("device", []), ("device", ["--io", "mapped"]), ("host", [])])
def test_checked_run_equals_the_run_without_the_flag(dump, unchecked_run, tmp_path, mode, io):
    want, want_rows = unchecked_run
    conf = write_conf(tmp_path, str(dump / "kafka-json.log"), str(dump / "ad-to-campaign.csv"))
    out_csv = tmp_path / "windows.csv"
    r = run(conf, "--kafka", "--kafka-check-crc", mode, "--batch-bytes", "100000", "--sink", "csv:%s" % out_csv, *io)
    assert r.returncode == 0, r.stderr
    out = last_json(r)
    with open(out_csv) as f:
        assert sorted(f.read().splitlines()) == want_rows and len(want_rows) > 1
    for k in STATS:
        assert out[k] == want[k], k
    assert out["events"] == N and out["kafka_records"] == N == want["kafka_records"]
    assert out["kafka_framed_bytes"] == want["kafka_framed_bytes"]


def flipped(dump, tmp_path):
    """The segment with one bit flipped in the last byte of its batch 40: (path, batch, baseOffset)."""
    blob = bytearray((dump / "kafka-json.log").read_bytes())
    idx, _ = kafka.index(bytes(blob), check_crc=True)
    k = 40
    blob[int(idx[k]["records_off"]) + int(idx[k]["records_bytes"]) - 2] ^= 0x01     # inside the last record's value
    assert kafka.verdict(bytes(blob), idx)["bad_batches"] == 0                       # the framing stays whole
    bad = tmp_path / "flipped.log"
    bad.write_bytes(bytes(blob))
    return bad, idx, k


def test_flipped_bit_ends_the_run_naming_the_batch(dump, tmp_path):
    bad, idx, k = flipped(dump, tmp_path)
    conf = write_conf(tmp_path, str(bad), str(dump / "ad-to-campaign.csv"))
    # without the flag the flipped byte goes through, as before
    assert run(conf, "--kafka").returncode == 0
    r = run(conf, "--kafka", "--kafka-check-crc", "device")                   # one slot batch: the entry is k
    assert r.returncode != 0 and "Kafka batch %d (baseOffset %d)" % (k, int(idx[k]["base_offset"])) in r.stderr, r.stderr
    assert "stored" in r.stderr and "computed" in r.stderr and "CRC-32C" in r.stderr
    r = run(conf, "--kafka", "--kafka-check-crc", "host")
    assert r.returncode != 0 and "crc" in r.stderr and "at byte %d" % (int(idx[k]["records_off"]) - M.HEADER) in r.stderr


def test_python_source_device_mode(dump, unchecked_run, tmp_path):
    want, _ = unchecked_run
    ids = [l.split(",") for l in (dump / "ad-to-campaign.csv").read_text().splitlines() if l]
    camps = sorted({c for _, c in ids})
    ads = ([a for a, _ in ids], [camps.index(c) for _, c in ids])
    with make_ctx(n_campaigns=len(camps), ads=ads, max_batch_bytes=1 << 20) as c, \
            KafkaLogDataSource(dump / "kafka-json.log", check_crc="device") as src:
        assert src.run(c, 1 << 20) == src.size and src.batches > 4 and src.summary["crc_checked"] == 0
        st = c.stats()
        ci = c.kafka_crc_info()
        assert ci["calls"] == src.batches and ci["bad_batches"] == 0
        assert ci["mode"] == 0        # the source turned the check on for its own submits and put the caller's setting back
    for k in STATS:
        assert st[k] == want[k], k
    bad, idx, k = flipped(dump, tmp_path)
    with make_ctx(n_campaigns=len(camps), ads=ads, max_batch_bytes=1 << 20) as c, \
            KafkaLogDataSource(bad, check_crc="device") as src:
        with pytest.raises(YsbError) as e:
            src.run(c, 1 << 20)
        assert e.value.code == -5 and "baseOffset %d)" % int(idx[k]["base_offset"]) in str(e.value) and "stored" in str(e.value)
