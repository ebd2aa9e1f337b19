"""GPU: a plain `bench.py` run (no --full) and its --dump-outputs files.  The line holds the
headline keys with `steps` timed steps and none of the legs --full adds; the dumped rows are
the context's table after the warm-up and timed steps (the steps never reset it), so they
equal (warmup + steps) x the C oracle's counts of one pass over the host generator's same
events, and two runs with the same arguments write identical files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle
from ysb_amd import GenParams

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, WARMUP, STEPS, RATE = 250_000, 1, 2, 10_000   # 25 s of event time: 3 windows; 4 ragged batches


def run_bench(out_dir):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "LOCAL_WORLD_SIZE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--events", str(N), "--segment", "70001", "--rate", str(RATE),
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    line = run_bench(tmp_path / "a")
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["n_gpus"] == 1
    assert line["unit"] == "events/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["ms_per_step"] > 0
    # ms_per_step is printed to 1e-4 ms: within 1 % of the value's own step time from 0.005 ms up
    assert line["ms_per_step"] >= 0.005
    assert line["value"] == pytest.approx(N / (line["ms_per_step"] * 1e-3), rel=1e-2)
    assert line["config"]["batches_per_step"] == 4
    assert line["check"] is None and line["cpu_baseline"] is None and "extras_summary" not in line

    counts = np.load(tmp_path / "a" / "counts.npy")
    stats = np.load(tmp_path / "a" / "stats.npy")
    assert counts.dtype == np.float64 and counts.ndim == 2 and counts.shape[1] == 3
    assert stats.dtype == np.float64

    g = GenParams(seed=42, n_campaigns=100, ads_per_campaign=10, events_per_sec=RATE)
    _, ads = g.ids()
    raw, offs = g.events_host(0, N)
    rows, ost = oracle.run(oracle.AdMap(ads, g.ad_campaign_index()), raw, offs)
    passes = WARMUP + STEPS
    want = np.array(sorted((c, b * 10000, v * passes) for (c, b), v in rows.items()), dtype=np.float64)
    assert len(want) > 200 and np.array_equal(counts, want)
    names = ("events", "views", "joined", "join_misses", "parse_errors", "time_errors", "out_of_ring",
             "overflow_dropped")
    assert [stats[i] for i in range(len(names))] == [ost.get(k, 0) * passes for k in names]
    assert stats[0] == N * passes and stats[1] == counts[:, 2].sum()

    run_bench(tmp_path / "b")
    for name in ("counts.npy", "stats.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)), name
