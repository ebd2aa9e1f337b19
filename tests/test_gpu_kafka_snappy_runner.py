"""GPU: the native runner's --kafka --kafka-codec snappy (slot copies and --io mapped, batch mode)
over the snappy log segments that bin/ysb_gen --kafka --kafka-codec snappy writes, in both framings:
the same CSV and stats as the plain run of kafka-json.txt on the same seed; the Python
KafkaLogDataSource(codecs=("lz4", "snappy")) on the same file; --kafka-codec lz4 and plain --kafka
still refuse the snappy segment by name."""
import subprocess

import pytest

import snappy_model as S
from test_gpu_lz4_runner import GEN, STATS, run
from test_gpu_parity import make_ctx
from test_topology import last_json, write_conf
from ysb_amd import KafkaLogDataSource, YsbError, kafka

pytestmark = pytest.mark.gpu

N = 5000


def gen(d, *extra):
    r = subprocess.run([GEN, "-d", str(d), "-n", str(N), "--seed", "11", "--campaigns", "10", "--ads-per-campaign", "10",
                        "--with-skew", "--kafka", "--kafka-codec", "snappy", *extra], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return d


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """ysb_gen --kafka --kafka-batch 100000 --kafka-codec snappy: 5,000 events as kafka-json.txt and a
    kafka-json.log of xerial streams of four 32 KiB chunks each."""
    return gen(tmp_path_factory.mktemp("kafka_snappy"), "--kafka-batch", "100000")


@pytest.fixture(scope="module")
def dump_raw(tmp_path_factory):
    """The same events, a raw block per 16 KiB batch (--kafka-snappy-framing raw)."""
    return gen(tmp_path_factory.mktemp("kafka_snappy_raw"), "--kafka-snappy-framing", "raw")


@pytest.fixture(scope="module")
def plain_run(dump, tmp_path_factory):
    sub = tmp_path_factory.mktemp("plain")
    conf = write_conf(sub, str(dump / "kafka-json.txt"), str(dump / "ad-to-campaign.csv"))
    out_csv = sub / "windows.csv"
    r = run(conf, "--sink", "csv:%s" % out_csv)
    assert r.returncode == 0, r.stderr
    with open(out_csv) as f:
        return last_json(r), sorted(f.read().splitlines())


def test_gen_writes_snappy_segments_the_model_reads(dump, dump_raw):
    txt = (dump / "kafka-json.txt").read_bytes()
    lines = txt.split(b"\n")
    assert (dump_raw / "kafka-json.txt").read_bytes() == txt
    for d, xerial in ((dump, True), (dump_raw, False)):
        blob = (d / "kafka-json.log").read_bytes()
        mi, mf, mb, info = S.index(blob, check_crc=True)      # the model checks every CRC over the wire bytes
        assert info["n_records"] == N and info["consumed"] == len(blob) and info["compressed_batches"] == len(mi) > 5
        assert all(codec == 2 for _, _, codec in mf) and (max(n for _, n, _ in mf) == 4) == xerial
        assert (blob[61:69] == S.XERIAL_MAGIC) == xerial
        assert S.unframe(blob, mi[:2], mf[:2], mb)[0] == b"".join(lines[:mi[2]["first_record"]])   # (pure Python: two batches)
        idx, fr, bl, _ = kafka.index_lz4(blob, check_crc=True, accept_snappy=True)
        assert kafka.unframe_lz4_host(blob, idx, fr, bl)[0].tobytes() == b"".join(lines)
        assert len(blob) < 0.8 * len(txt)                      # the events compress


@pytest.mark.parametrize("io", [[], ["--io", "mapped"]])
@pytest.mark.parametrize("framing", ["xerial", "raw"])
def test_kafka_snappy_runner_equals_the_plain_run(dump, dump_raw, plain_run, tmp_path, io, framing):
    """CSV rows and stats equal the plain run's, through the slot's copy and in place; the xerial
    segment at a 512 KiB slot, so that the capacity rule (the preambles' sizes) cuts the runs."""
    want, want_rows = plain_run
    d = dump if framing == "xerial" else dump_raw
    conf = write_conf(tmp_path, str(d / "kafka-json.log"), str(d / "ad-to-campaign.csv"))
    out_csv = tmp_path / "windows.csv"
    extra = ["--batch-bytes", "524288"] if framing == "xerial" else []
    r = run(conf, "--kafka", "--kafka-codec", "snappy", "--sink", "csv:%s" % out_csv, *(io + extra))
    assert r.returncode == 0, r.stderr
    out = last_json(r)
    with open(out_csv) as f:
        assert sorted(f.read().splitlines()) == want_rows and len(want_rows) > 1
    for k in STATS:
        assert out[k] == want[k], k
    assert out["events"] == N and out["kafka"] is True and out["kafka_records"] == N and out["kafka_codec"] == "snappy"
    assert out["kafka_io"] == ("mapped" if io else "slot")
    assert out["kafka_framed_bytes"] == (d / "kafka-json.log").stat().st_size
    assert out["kafka_compressed_batches"] == out["kafka_batches"] > 5
    assert out["kafka_inflated_bytes"] > out["kafka_framed_bytes"]
    if extra:
        assert out["batches"] >= 3      # about 1.3 MB of records by their preambles, 512 KiB a run


def test_python_source_counts_the_snappy_segment(dump, plain_run):
    want, _ = plain_run
    ids = [l.split(",") for l in (dump / "ad-to-campaign.csv").read_text().splitlines() if l]
    camps = sorted({c for _, c in ids})
    for codecs in ((), ("lz4",)):
        with pytest.raises(YsbError) as e:
            KafkaLogDataSource(dump / "kafka-json.log", codecs=codecs)
        assert "codec = 2" in str(e.value)
    with make_ctx(n_campaigns=len(camps), ads=([a for a, _ in ids], [camps.index(c) for _, c in ids]),
                  max_batch_bytes=1 << 20) as c, KafkaLogDataSource(dump / "kafka-json.log", check_crc=True,
                                                                    codecs=("lz4", "snappy")) as src:
        assert src.run(c, 1 << 19) == src.size and src.batches >= 3
        st = c.stats()
        li = c.kafka_lz4_info()
        assert li["calls"] == src.batches and li["snappy_blocks"] == li["blocks"] > 0
    for k in STATS:
        assert st[k] == want[k], k


def test_the_other_options_still_refuse_the_snappy_segment(dump, tmp_path):
    conf = write_conf(tmp_path, str(dump / "kafka-json.log"), str(dump / "ad-to-campaign.csv"))
    for opts, word in ((["--kafka"], "codec 0 only"), (["--kafka", "--kafka-codec", "lz4"], "snappy-compressed")):
        r = run(conf, *opts)
        assert r.returncode == 1 and "codec = 2" in r.stderr and word in r.stderr and "at byte 0" in r.stderr
