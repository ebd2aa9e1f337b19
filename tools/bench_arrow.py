#!/usr/bin/env python
"""Times the Arrow count (ysb_submit_arrow_device) on generator rows resident in HBM, beside the
columnar count (ysb_submit_columns_device) on the same rows in the same process.

    python tools/bench_arrow.py [--events N] [--warmup W] [--iters K] [--rounds R] [--device D] [--out PATH]

The rows: N device-generated events decoded once into the seven-column layout (the reference
leg's input), their ad_id / event_type / event_time read back and re-laid as Arrow buffers with
numpy -- int32 offsets and bytes per string column, the type also dictionary-encoded, the time
also as 13-digit strings -- and uploaded.  Legs: the Arrow count with string times, with int64
times, with a dictionary type; the reference leg.  The four are alternated R times; each turn
times K launches one by one with YSB_F_TIMING's HIP events.  Per leg: the median over all its
launches, rows/s, the bytes the leg must read per row, and GB/s of those.  Prints one JSON line
and writes it to profiles/arrow_bench.json.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "streaming-benchmarks_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from ysb_amd import GenParams, YsbContext, arrow, columns_layout  # noqa: E402

VOCAB = (b"view", b"click", b"purchase")


def arrow_buffers(ctx, d_out, n):
    """The decoded columns of rows [0, n) as host Arrow buffers."""
    st = columns_layout(n)["start"]
    ad = ctx.d2h(np.empty(36 * n, dtype=np.uint8), d_out + st[2])
    et = ctx.d2h(np.empty(4 * n, dtype=np.uint8), d_out + st[4]).reshape(n, 4)
    tm = ctx.d2h(np.empty(8 * n, dtype=np.uint8), d_out + st[5]).view("<i8")
    idx = np.select([et[:, 0] == ord("v"), et[:, 0] == ord("c")], [0, 1], 2).astype(np.int32)   # the layout cut the type to 4 bytes
    lens = np.array([len(v) for v in VOCAB], dtype=np.int32)[idx]
    ty_off = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(lens, out=ty_off[1:])
    vocab = np.frombuffer(b"".join(VOCAB), dtype=np.uint8)
    vstart = np.array([0, 4, 9], dtype=np.int32)[idx]
    pos = np.arange(int(ty_off[-1]), dtype=np.int32) - np.repeat(ty_off[:-1], lens)
    ty_data = vocab[np.repeat(vstart, lens) + pos]
    w = len(str(int(tm.max())))   # every time has as many digits (13 for the generator's)
    assert tm.min() >= 10 ** (w - 1)
    digits = ((tm[:, None] // (10 ** np.arange(w - 1, -1, -1, dtype=np.int64))[None, :]) % 10 + 48).astype(np.uint8).reshape(-1)
    fixed = lambda w: (np.arange(n + 1, dtype=np.int64) * w).astype(np.int32)
    d_off = np.array([0, 4, 9, 17], dtype=np.int32)
    return {"ad_off": fixed(36), "ad": ad, "ty_off": ty_off, "ty": ty_data, "idx": idx, "dict_off": d_off, "dict": vocab.copy(),
            "tm_off": fixed(w), "tm": digits, "tm64": np.ascontiguousarray(tm)}


def per_launch_ms(ctx, submit, warmup, iters):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=10_000_000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "arrow_bench.json"))
    a = ap.parse_args()
    n = a.events
    g = GenParams(seed=11, n_campaigns=100, ads_per_campaign=10, events_per_sec=1_000_000)
    with YsbContext(device=a.device, n_campaigns=100, timing=True, layout_auto=False, max_batch_events=1 << 12,
                    max_batch_bytes=1 << 20) as ctx:
        ctx.load_ad_map_packed(g.ids_packed()[1], g.ad_campaign_index_array())
        cap = n * g.max_line_bytes()
        d_b, d_o, d_out = ctx.device_alloc(cap), ctx.device_alloc(4 * n), ctx.device_alloc(columns_layout(n)["start"][8])
        nb = ctx.gen_events_device(g, 0, n, d_b, cap, d_o)
        assert ctx.decode_columns_device(d_b, nb, d_o, n, d_out, n)["valid"] == n
        h = arrow_buffers(ctx, d_out, n)
        for p in (d_b, d_o):
            ctx.device_free(p)
        d = {}
        for k, v in h.items():
            d[k] = ctx.device_alloc(v.nbytes)
            ctx.h2d(d[k], v)
        ad = arrow.col(arrow.STRING, offsets=d["ad_off"], data=d["ad"], data_bytes=h["ad"].nbytes)
        ty = arrow.col(arrow.STRING, offsets=d["ty_off"], data=d["ty"], data_bytes=h["ty"].nbytes)
        ti = arrow.col(arrow.DICT, data=d["idx"], data_bytes=h["idx"].nbytes)
        dv = arrow.col(arrow.STRING, offsets=d["dict_off"], data=d["dict"], data_bytes=h["dict"].nbytes)
        ts = arrow.col(arrow.STRING, offsets=d["tm_off"], data=d["tm"], data_bytes=h["tm"].nbytes)
        t64 = arrow.col(arrow.INT64, data=d["tm64"], data_bytes=h["tm64"].nbytes)
        ty_b = 4 + h["ty"].nbytes / n
        legs = {
            "arrow_string_times": (arrow.cols(n, ad, ty, ts), 40 + ty_b + 4 + h["tm"].nbytes / n),
            "arrow_int64_times": (arrow.cols(n, ad, ty, t64), 40 + ty_b + 8),
            "arrow_dict_type": (arrow.cols(n, ad, ti, ts, dv, 3), 40 + 4 + 4 + h["tm"].nbytes / n),
            "columns": (None, 48.0),
        }
        ms = {k: [] for k in legs}
        stats = {}
        for _ in range(a.rounds):
            for name, (cols, _) in legs.items():
                ctx.reset()
                sub = (lambda: ctx.submit_columns_device(d_out, n, n, 0)) if cols is None else (lambda c=cols: ctx.submit_arrow_device(c))
                ms[name] += per_launch_ms(ctx, sub, a.warmup, a.iters)
                st = ctx.stats()
                stats[name] = {k: st[k] // (a.warmup + a.iters) for k in ("events", "views", "joined", "join_misses", "parse_errors", "time_errors")}
        info = ctx.arrow_launch_info()
        for name in legs:   # the same rows, the same counts
            assert stats[name] == stats["columns"], (name, stats[name], stats["columns"])
        for p in list(d.values()) + [d_out]:
            ctx.device_free(p)
    out = {"tool": "bench_arrow", "events": n, "warmup": a.warmup, "iters": a.iters, "rounds": a.rounds,
           "views": stats["columns"]["views"], "grid": info["grid"], "per_lane_tiles": info["per_lane_tiles"], "legs": {}}
    for name, (_, bpr) in legs.items():
        m = statistics.median(ms[name])
        out["legs"][name] = {"kernel_ms": round(m, 4), "kernel_ms_min": round(min(ms[name]), 4), "kernel_ms_max": round(max(ms[name]), 4),
                             "rows_per_s": round(n / (m * 1e-3), 1), "bytes_per_row": round(bpr, 3),
                             "GB_per_s": round(bpr * n / (m * 1e-3) / 1e9, 1)}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
