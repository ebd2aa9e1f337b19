#!/usr/bin/env python
"""Times the joined-views call (ysb_join_device) on device-generated events, in the generator's
JSON layout and as .tbl rows, with and without YSB_JOIN_KEYS, beside the counting scan
(ysb_submit_device) on the same batch in the same run.

    python tools/bench_join.py [--events N] [--warmup W] [--iters K] [--device D] [--out PATH]
                               [--formats json,tbl]

Prints one JSON line and writes it to profiles/join_bench.json: per leg the three kernels' times
(median of K, HIP event pairs), events/s over their sum, the algorithmic bytes -- input + 4 B
offset per line + the output rows (17 B each, 74 B with keys) -- and their rate in TB/s, and
the counting scan's kernel time and rate on the same batch (ysb_kernel_time).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "streaming-benchmarks_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from ysb_amd import GenParams, YsbContext, YSB_JOIN_KEYS, joined_layout  # noqa: E402


def leg(fmt, keys, n, warmup, iters, device):
    g = GenParams(seed=11, n_campaigns=100, ads_per_campaign=10, events_per_sec=1_000_000, fmt=fmt)
    _, ads = g.ids()
    flags = YSB_JOIN_KEYS if keys else 0
    with YsbContext(device=device, n_campaigns=100, timing=True, input_format=fmt, layout_auto=False,
                    max_batch_events=max(n, 1 << 12), max_batch_bytes=1 << 20) as ctx:
        ctx.load_ad_map(ads, g.ad_campaign_index())
        cap = n * g.max_line_bytes()
        lay = joined_layout(n, flags)
        d_b, d_o, d_out = ctx.device_alloc(cap), ctx.device_alloc(4 * n), ctx.device_alloc(lay["start"][6])
        nb = ctx.gen_events_device(g, 0, n, d_b, cap, d_o)
        info = None
        for _ in range(warmup):
            info = ctx.join_device(d_b, nb, d_o, n, d_out, n, flags)
        ms = {"join_ms": [], "prefix_ms": [], "pack_ms": []}
        for _ in range(iters):
            info = ctx.join_device(d_b, nb, d_o, n, d_out, n, flags)
            for k in ms:
                ms[k].append(info[k])
        assert info["fast_rows"] == n and info["joined"] == info["views"] == info["rows_written"], info
        for _ in range(warmup):
            ctx.submit_device(d_b, nb, d_o, n)
        ctx.sync()
        ctx.kernel_time()
        for _ in range(iters):
            ctx.submit_device(d_b, nb, d_o, n)
        ctx.sync()
        scan_ms, launches = ctx.kernel_time()
        st = ctx.stats()
        assert st["joined"] == info["joined"] * (warmup + iters), (st, info)   # the same events, the same join
        for p in (d_b, d_o, d_out):
            ctx.device_free(p)
    med = {k: statistics.median(v) for k, v in ms.items()}
    total = sum(med.values())
    scan = scan_ms / max(launches, 1)
    row_bytes = sum(lay["width"])
    alg = nb + 4 * n + row_bytes * info["joined"]
    return {"join_ms": round(med["join_ms"], 4), "prefix_ms": round(med["prefix_ms"], 4), "pack_ms": round(med["pack_ms"], 4),
            "total_ms": round(total, 4), "join_ms_min": round(min(ms["join_ms"]), 4), "join_ms_max": round(max(ms["join_ms"]), 4),
            "events_per_s": round(n / (total * 1e-3), 1), "joined": info["joined"], "row_bytes": row_bytes,
            "input_bytes": nb, "algorithmic_bytes": int(alg), "TB_per_s": round(alg / (total * 1e-3) / 1e12, 4),
            "grid": info["grid"], "tiles": info["tiles"],
            "scan_kernel_ms": round(scan, 4), "scan_events_per_s": round(n / (scan * 1e-3), 1),
            "scan_TB_per_s": round((nb + 4 * n) / (scan * 1e-3) / 1e12, 4),
            "extra_traffic_over_scan": round(row_bytes * info["joined"] / (nb + 4 * n), 4),
            "time_over_scan": round(total / scan, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=10_000_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "join_bench.json"))
    ap.add_argument("--formats", default="json,tbl", help="the legs' input formats")
    a = ap.parse_args()
    out = {"tool": "bench_join", "events": a.events, "warmup": a.warmup, "iters": a.iters}
    for fmt in a.formats.split(","):
        for keys in (False, True):
            out[fmt + ("_keys" if keys else "")] = leg(fmt, keys, a.events, a.warmup, a.iters, a.device)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
