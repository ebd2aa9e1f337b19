#!/usr/bin/env python
"""Times the columnar decode (ysb_decode_columns_device) on device-generated events, in the
generator's JSON layout and as .tbl rows, beside the counting scan on the same batch.

    python tools/bench_columns.py [--events N] [--warmup W] [--iters K] [--device D] [--append-log]
                                  [--no-decode] [--no-count] [--no-big]

Prints one JSON line: per format kernel_ms (median of K, HIP events around the kernel),
events/s, the algorithmic bytes (input + 4 B offset + 132 B of columns + 1/8 B of validity per
row), their rate as a fraction of the 8 TB/s HBM peak, and the counting scan's time on the same
batch (ysb_kernel_time).  --append-log adds the line as an entry to profiles/AB_LOG.md.

The counting leg ("count"): the same device-generated JSON events decoded once, then the columnar
count (ysb_submit_columns_device with the validity bitmap) timed per launch with YSB_F_TIMING's
HIP events (median of K), in a context of 100 campaigns (LDS window counters) and one of 1M
campaigns / 10M ads (HBM bucket table, ring atomics; --no-big leaves it out).  Reported: events/s,
the fraction of the 8 TB/s HBM peak on the 48.125 B a row it reads, and the JSON counting scan
on the same events in the same run as the yardstick.
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

from ysb_amd import GenParams, YsbContext, _lib, columns_layout  # noqa: E402

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


def per_launch_ms(ctx, submit, warmup, iters):
    """Per-launch kernel ms (YSB_F_TIMING's HIP events), one launch at a time."""
    for _ in range(warmup):
        submit()
    ctx.sync()
    ctx.kernel_time()
    ms = []
    for _ in range(iters):
        submit()
        ctx.sync()
        t, k = ctx.kernel_time()
        assert k == 1
        ms.append(t)
    return ms


def count_leg(n_campaigns, ads_per_campaign, ring, n, warmup, iters, device):
    g = GenParams(seed=11, n_campaigns=n_campaigns, ads_per_campaign=ads_per_campaign, events_per_sec=1_000_000)
    with YsbContext(device=device, n_campaigns=n_campaigns, window_ring=ring, timing=True, layout_auto=False,
                    max_batch_events=1 << 12, max_batch_bytes=1 << 20) as ctx:
        ctx.load_ad_map_packed(g.ids_packed()[1], g.ad_campaign_index_array())
        cap = n * g.max_line_bytes()
        lay = columns_layout(n)
        d_b, d_o, d_out = ctx.device_alloc(cap), ctx.device_alloc(4 * n), ctx.device_alloc(lay["start"][8])
        nb = ctx.gen_events_device(g, 0, n, d_b, cap, d_o)
        info = ctx.decode_columns_device(d_b, nb, d_o, n, d_out, n)
        assert info["valid"] == n, info
        ms = per_launch_ms(ctx, lambda: ctx.submit_columns_device(d_out, n, n, _lib.YSB_COL_VALIDITY), warmup, iters)
        cinfo = ctx.columns_launch_info()
        st_cols = ctx.stats()
        ctx.reset()
        scan = per_launch_ms(ctx, lambda: ctx.submit_device(d_b, nb, d_o, n), warmup, iters)
        sinfo = ctx.launch_info()
        st_scan = ctx.stats()
        for k in ("events", "views", "joined", "join_misses"):   # the same events, the same counts
            assert st_cols[k] == st_scan[k], (k, st_cols[k], st_scan[k])
        for p in (d_b, d_o, d_out):
            ctx.device_free(p)
    k_ms, s_ms = statistics.median(ms), statistics.median(scan)
    alg = 48.125 * n
    return {"campaigns": n_campaigns, "ads": n_campaigns * ads_per_campaign, "window_ring": ring,
            "kernel_ms": round(k_ms, 4), "kernel_ms_min": round(min(ms), 4), "kernel_ms_max": round(max(ms), 4),
            "events_per_s": round(n / (k_ms * 1e-3), 1), "bytes_per_row": 48.125,
            "hbm_fraction": round(alg / (k_ms * 1e-3) / HBM_PEAK, 4), "lds_counters": cinfo["lds_counters"],
            "hbm_table": cinfo["hbm_table"], "views": st_cols["views"] // (warmup + iters),
            "scan_kernel_ms": round(s_ms, 4), "scan_events_per_s": round(n / (s_ms * 1e-3), 1),
            "scan_input_bytes": nb, "scan_record_mode": sinfo["record_mode"],
            "speedup_over_scan": round(s_ms / k_ms, 3)}


def host_leg(rows, submits, device):
    """Rows/s of ysb_submit_columns over the two pinned slots (each holding one image of `rows`
    rows, longs little-endian, with the bitmap): wall clock over `submits` double-buffered submits,
    and the bytes that cross the bus per row."""
    import ctypes as C
    import numpy as np
    g = GenParams(seed=11, n_campaigns=100, ads_per_campaign=10, events_per_sec=1_000_000)
    lay = columns_layout(rows)
    total = lay["start"][8]
    with YsbContext(device=device, n_campaigns=100, timing=True, layout_auto=False, max_batch_events=1 << 12,
                    max_batch_bytes=total) as ctx:
        ctx.load_ad_map_packed(g.ids_packed()[1], g.ad_campaign_index_array())
        cap = rows * g.max_line_bytes()
        d_b, d_o, d_out = ctx.device_alloc(cap), ctx.device_alloc(4 * rows), ctx.device_alloc(total)
        nb = ctx.gen_events_device(g, 0, rows, d_b, cap, d_o)
        assert ctx.decode_columns_device(d_b, nb, d_o, rows, d_out, rows)["valid"] == rows
        addr = [ctx.slot_buffers(s)[0] for s in (0, 1)]
        for s in (0, 1):
            ctx.d2h(np.ctypeslib.as_array((C.c_uint8 * total).from_address(addr[s])), d_out)
        flags = _lib.YSB_COL_VALIDITY
        for k in range(4):
            ctx.submit_columns(addr[k & 1], rows, rows, slot=k & 1, flags=flags)
        ctx.sync()
        ctx.copy_time()
        t0 = time.perf_counter()
        for k in range(submits):
            ctx.wait(k & 1)
            ctx.submit_columns(addr[k & 1], rows, rows, slot=k & 1, flags=flags)
        ctx.sync()
        el = time.perf_counter() - t0
        copy_ms, copies, copy_bytes = ctx.copy_time()
        for p in (d_b, d_o, d_out):
            ctx.device_free(p)
    return {"rows_per_image": rows, "submits": submits, "rows_per_s": round(rows * submits / el, 1),
            "bytes_copied_per_row": round(copy_bytes / (rows * submits), 3), "image_bytes_per_row": 132,
            "copy_GBs": round(copy_bytes / (copy_ms * 1e-3) / 1e9, 2) if copy_ms else 0.0,
            "copy_busy_frac": round(copy_ms * 1e-3 / el, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=10_000_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--append-log", action="store_true")
    ap.add_argument("--no-decode", action="store_true", help="skip the decode legs")
    ap.add_argument("--no-count", action="store_true", help="skip the counting legs")
    ap.add_argument("--no-big", action="store_true", help="skip the 1M-campaign / 10M-ad counting leg")
    ap.add_argument("--host-rows", type=int, default=1_000_000, help="rows per image of the host-form leg (0: skip)")
    a = ap.parse_args()
    out = {"tool": "bench_columns", "events": a.events, "warmup": a.warmup, "iters": a.iters}
    if not a.no_decode:
        out["json"] = leg("json", a.events, a.warmup, a.iters, a.device)
        out["tbl"] = leg("tbl", a.events, a.warmup, a.iters, a.device)
    if not a.no_count:
        out["count"] = {"c100": count_leg(100, 10, 1024, a.events, a.warmup, a.iters, a.device)}
        if not a.no_big:
            out["count"]["c1m"] = count_leg(1_000_000, 10, 128, a.events, a.warmup, a.iters, a.device)
        if a.host_rows:
            out["count"]["host"] = host_leg(a.host_rows, 40, a.device)
    line = json.dumps(out)
    print(line)
    if a.append_log:
        with open(os.path.join(ROOT, "profiles", "AB_LOG.md"), "a") as f:
            f.write("\n## columnar decode and count, %s (tools/bench_columns.py)\n\n```\n%s\n```\n"
                    % (time.strftime("%Y-%m-%d"), line))


if __name__ == "__main__":
    main()
