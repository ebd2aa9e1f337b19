"""GPU: bin/ysb_topology --columns -- the reference's commented chain
(AdvertisingTopologyNative.java:106-109): every window.size rows of the events file become one
<shared_file>_<k> holding WindowedArrowFormatBolter's image (:278-356), compared byte for byte
with the CPU model (Java byte order, stamp 10, zero padding)."""
import os
import subprocess

import pytest

import columns_model as cm
import golden_data as gd
from oracle import dostats
from test_topology import EXE, last_json

pytestmark = pytest.mark.gpu

WINDOW = 64


def write_conf(tmp_path, events, shared):
    p = tmp_path / "benchmarkConf.yaml"
    p.write_text("""ad_to_campaign_path: "%s"
events_path: "%s"
window.size: %d
shared_file: "%s"
""" % (gd.path("gen_s7.ad_to_campaign.csv"), events, WINDOW, shared))
    return str(p)


def tbl_rows(n):
    raw, _ = gd.events("gen_s7", ".tbl")
    return dostats.split_lines(raw)[0][:n]


def run_columns(conf):
    return subprocess.run([EXE, "--confPath", conf, "--columns", "--batch-bytes", str(1 << 20)],
                          capture_output=True, text=True, timeout=120)


def test_columns_files_equal_the_model(tmp_path):
    rows = tbl_rows(200)   # three whole windows and a tail of 8 that never fires
    events = tmp_path / "events.tbl"
    events.write_bytes(b"".join(rows))
    shared = str(tmp_path / "shared")
    r = run_columns(write_conf(tmp_path, str(events), shared))
    assert r.returncode == 0, r.stderr
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("shared")) == ["shared_0", "shared_1", "shared_2"]
    lay = cm.layout(WINDOW)
    for k in range(3):
        want, valid, _ = cm.build(rows[WINDOW * k:WINDOW * (k + 1)], batch_rows=WINDOW, fmt="tbl", stamp=10,
                                  java_order=True)
        assert valid.all()
        got = open(shared + "_%d" % k, "rb").read()
        assert len(got) == lay["image_bytes"]
        assert got == bytes(want[:lay["image_bytes"]])
    out = last_json(r)
    assert out["mode"] == "columns" and out["files"] == 3 and out["rows"] == 192 and out["dropped_tail_rows"] == 8


def test_columns_short_row_fails_the_job(tmp_path):
    rows = tbl_rows(200)
    rows[64 + 37] = b"short|row\n"   # ArrayIndexOutOfBounds in the reference's flatMap
    events = tmp_path / "events.tbl"
    events.write_bytes(b"".join(rows))
    shared = str(tmp_path / "shared")
    r = run_columns(write_conf(tmp_path, str(events), shared))
    assert r.returncode != 0
    assert "file index 1" in r.stderr and "row 37" in r.stderr
    assert not os.path.exists(shared + "_1") and not os.path.exists(shared + "_2")
