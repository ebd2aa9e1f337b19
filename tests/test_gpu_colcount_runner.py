"""GPU: bin/ysb_topology --from-columns, the consumer of --columns: the <shared_file>_<k> images
of WindowedArrowFormatBolter (AdvertisingTopologyNative.java:278-356) counted from their columns
give the batch runner's CSV over the same rows."""
import os
import subprocess

import pytest

import golden_data as gd
from oracle import dostats
from test_topology import EXE, last_json

pytestmark = pytest.mark.gpu

WINDOW = 64


def write_conf(tmp_path, events, shared, name="benchmarkConf.yaml"):
    p = tmp_path / name
    p.write_text("""ad_to_campaign_path: "%s"
events_path: "%s"
window.size: %d
shared_file: "%s"
""" % (gd.path("gen_s7.ad_to_campaign.csv"), events, WINDOW, shared))
    return str(p)


def run(conf, *args):
    return subprocess.run([EXE, "--confPath", conf] + list(args), capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def images(tmp_path_factory):
    """--columns over the first 200 .tbl rows of gen_s7: three images and a tail that never fires."""
    tmp = tmp_path_factory.mktemp("colcount_runner")
    raw, _ = gd.events("gen_s7", ".tbl")
    rows = dostats.split_lines(raw)[0][:200]
    events = tmp / "events.tbl"
    events.write_bytes(b"".join(rows))
    shared = str(tmp / "shared")
    conf = write_conf(tmp, str(events), shared)
    r = run(conf, "--columns", "--batch-bytes", str(1 << 20))
    assert r.returncode == 0, r.stderr
    return tmp, rows, shared, conf


def test_from_columns_equals_the_batch_runner(images):
    tmp, rows, shared, conf = images
    out_csv = tmp / "from_columns.csv"
    r = run(conf, "--from-columns", "--sink", "csv:%s" % out_csv, "--window-ring", "16")
    assert r.returncode == 0, r.stderr
    out = last_json(r)
    assert out["mode"] == "from_columns" and out["files"] == 3 and out["rows"] == 192
    # the batch runner over an events file holding the first 192 rows
    events192 = tmp / "events192.tbl"
    events192.write_bytes(b"".join(rows[:192]))
    want_csv = tmp / "batch.csv"
    conf192 = write_conf(tmp, str(events192), shared, "conf192.yaml")
    b = run(conf192, "--sink", "csv:%s" % want_csv, "--window-ring", "16", "--batch-bytes", str(1 << 20))
    assert b.returncode == 0, b.stderr
    bout = last_json(b)
    assert bout["events"] == 192 and bout["views"] == out["views"] > 0 and bout["joined"] == out["joined"] > 0
    assert out_csv.read_text() == want_csv.read_text() and len(out_csv.read_text().splitlines()) > 3


def test_truncated_image_fails_the_job_and_is_named(images):
    tmp, _, shared, conf = images
    whole = open(shared + "_1", "rb").read()
    try:
        with open(shared + "_1", "wb") as f:
            f.write(whole[:-4096])
        r = run(conf, "--from-columns")
        assert r.returncode != 0 and os.path.basename(shared) + "_1" in r.stderr
    finally:
        with open(shared + "_1", "wb") as f:
            f.write(whole)


def test_from_columns_is_not_combined(images):
    _, _, _, conf = images
    for other in ("--columns", "--stream"):
        r = run(conf, "--from-columns", other)
        assert r.returncode == 2 and "--from-columns" in r.stderr
