#!/usr/bin/env python
"""Times the columnar decode (ysb_decode_columns_device) on device-generated events, in the
generator's JSON layout and as .tbl rows, beside the counting scan on the same batch.

    python tools/bench_columns.py [--events N] [--warmup W] [--iters K] [--device D] [--append-log]

Prints one JSON line: per format kernel_ms (median of K, HIP events around the kernel),
events/s, the algorithmic bytes (input + 4 B offset + 132 B of columns + 1/8 B of validity per
row), their rate as a fraction of the 8 TB/s HBM peak, and the counting scan's time on the same
batch (ysb_kernel_time).  --append-log adds the line as an entry to profiles/AB_LOG.md.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "streaming-benchmarks_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from ysb_amd import GenParams, YsbContext, columns_layout  # noqa: E402

HBM_PEAK = 8.0e12


def leg(fmt, n, warmup, iters, device):
    g = GenParams(seed=11, n_campaigns=100, ads_per_campaign=10, events_per_sec=1_000_000, fmt=fmt)
    _, ads = g.ids()
    with YsbContext(device=device, n_campaigns=100, timing=True, input_format=fmt, layout_auto=False,
                    max_batch_events=1 << 12, max_batch_bytes=1 << 20) as ctx:
        ctx.load_ad_map(ads, g.ad_campaign_index())
        cap = n * g.max_line_bytes()
        lay = columns_layout(n)
        d_b, d_o, d_out = ctx.device_alloc(cap), ctx.device_alloc(4 * n), ctx.device_alloc(lay["start"][8])
        nb = ctx.gen_events_device(g, 0, n, d_b, cap, d_o)
        info = None
        for _ in range(warmup):
            info = ctx.decode_columns_device(d_b, nb, d_o, n, d_out, n)
        ms = []
        for _ in range(iters):
            info = ctx.decode_columns_device(d_b, nb, d_o, n, d_out, n)
            ms.append(info["kernel_ms"])
        assert info["valid"] == n and info["fast_rows"] == n, info
        for _ in range(warmup):
            ctx.submit_device(d_b, nb, d_o, n)
        ctx.sync()
        ctx.kernel_time()
        for _ in range(iters):
            ctx.submit_device(d_b, nb, d_o, n)
        ctx.sync()
        scan_ms, launches = ctx.kernel_time()
        for p in (d_b, d_o, d_out):
            ctx.device_free(p)
    k_ms = statistics.median(ms)
    alg = nb + 4 * n + 132 * n + n / 8.0
    return {"kernel_ms": round(k_ms, 4), "kernel_ms_min": round(min(ms), 4), "kernel_ms_max": round(max(ms), 4),
            "events_per_s": round(n / (k_ms * 1e-3), 1), "input_bytes": nb, "algorithmic_bytes": int(alg),
            "bytes_per_s": round(alg / (k_ms * 1e-3), 1), "hbm_fraction": round(alg / (k_ms * 1e-3) / HBM_PEAK, 4),
            "scan_kernel_ms": round(scan_ms / max(launches, 1), 4),
            "scan_hbm_fraction": round((nb + 4 * n) / (scan_ms / max(launches, 1) * 1e-3) / HBM_PEAK, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=10_000_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--append-log", action="store_true")
    a = ap.parse_args()
    out = {"tool": "bench_columns", "events": a.events, "warmup": a.warmup, "iters": a.iters,
           "json": leg("json", a.events, a.warmup, a.iters, a.device),
           "tbl": leg("tbl", a.events, a.warmup, a.iters, a.device)}
    line = json.dumps(out)
    print(line)
    if a.append_log:
        with open(os.path.join(ROOT, "profiles", "AB_LOG.md"), "a") as f:
            f.write("\n## columnar decode, %s (tools/bench_columns.py)\n\n```\n%s\n```\n"
                    % (time.strftime("%Y-%m-%d"), line))


if __name__ == "__main__":
    main()
