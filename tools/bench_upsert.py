#!/usr/bin/env python3
"""ysb_ad_map_upsert on the configs[2] table (10M ads, 1M campaigns, packed loader).

In one run on one GPU:
  * 9M ads loaded, then 1, 1,000 and 100,000 new ads upserted in place (disjoint ranges of the
    last million), the 9M reloaded and the whole last million upserted in place: host wall time,
    device_ms and the placement counters of each call;
  * the yardstick: the only other way to the same map, a full ysb_load_ad_map_packed -- of the
    9M (the smallest merged map of any case, so the strictest yardstick for the small cases) and
    of all 10M (the merged map of the 1M case);
  * configs[2]'s counting leg on two tables alternated in one process: a fresh load of all 10M,
    and 9M loaded plus 1M upserted.

Prints a markdown table (stderr) and one JSON line (stdout).
  python tools/bench_upsert.py [--device 0] [--events 33333334] [--rounds 3] [--steps 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "streaming-benchmarks_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

N_CAMPAIGNS, ADS_PER = 1_000_000, 10
LOADED = 9_000_000
PLACED = ("cuckoo_first", "cuckoo_second", "cuckoo_moved", "cuckoo_left_out")


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return r, time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--events", type=int, default=33_333_334, help="events per step of the counting leg")
    ap.add_argument("--segment", type=int, default=16_666_667)
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the two tables (>= 3)")
    ap.add_argument("--steps", type=int, default=5, help="timed steps per table and round")
    args = ap.parse_args()
    from ysb_amd import GenParams, YsbContext

    g = GenParams(seed=42, n_campaigns=N_CAMPAIGNS, ads_per_campaign=ADS_PER, events_per_sec=100_000)
    _, ab = g.ids_packed()
    camp = g.ad_campaign_index_array()
    keys = ab.reshape(-1, 36)
    kw = dict(device=args.device, n_campaigns=N_CAMPAIGNS, window_ring=128, timing=True,
              max_batch_bytes=1 << 20, max_batch_events=1 << 12)
    out = {"table": "configs[2]: 10M ads, 1M campaigns", "loaded": LOADED, "cases": []}

    def upsert(ctx, lo, n):
        info, wall = timed(lambda: ctx.upsert_ad_map_packed(keys[lo:lo + n], camp[lo:lo + n]))
        assert info["rebuilt"] == 0 and info["inserted"] == n and info["cuckoo_left_out"] == 0, info
        case = {"new_ads": n, "wall_ms": round(wall * 1e3, 3), "device_ms": round(info["device_ms"], 3)}
        case.update({k: info[k] for k in PLACED})
        out["cases"].append(case)
        log("upsert %9d: %10.3f ms wall, %9.3f ms device, %s" % (n, wall * 1e3, info["device_ms"],
                                                                 {k: info[k] for k in PLACED}))

    with YsbContext(**kw) as up, YsbContext(**kw) as fresh:
        _, load9 = timed(lambda: up.load_ad_map_packed(keys[:LOADED], camp[:LOADED]))
        out["reload_9M_s"] = round(load9, 3)
        out["admap"] = up.ad_map_info()
        lo = LOADED
        for n in (1, 1000, 100_000):
            upsert(up, lo, n)
            lo += n
        _, load9b = timed(lambda: up.load_ad_map_packed(keys[:LOADED], camp[:LOADED]))
        upsert(up, LOADED, 1_000_000)
        _, load10 = timed(lambda: fresh.load_ad_map_packed(keys, camp))
        out["reload_9M_again_s"] = round(load9b, 3)
        out["reload_10M_s"] = round(load10, 3)
        yard = min(load9, load9b) * 1e3
        out["every_case_below_reload"] = all(c["wall_ms"] < yard for c in out["cases"])
        assert up.ad_map_info()["keys"] == fresh.ad_map_info()["keys"] == 10_000_000

        # the counting leg: the same device batches through both tables, alternated
        segs, first = [], 0
        while first < args.events:
            n = min(args.segment, args.events - first)
            cap = n * g.max_line_bytes()
            d_b, d_o = up.device_alloc(cap), up.device_alloc(4 * n + 64)
            segs.append((d_b, up.gen_events_device(g, first, n, d_b, cap, d_o), d_o, n))
            first += n
        n_chk = 1_000_000   # a batch small enough to compare cell by cell
        c_b, c_o = up.device_alloc(n_chk * g.max_line_bytes()), up.device_alloc(4 * n_chk + 64)
        chk = [(c_b, up.gen_events_device(g, 0, n_chk, c_b, n_chk * g.max_line_bytes(), c_o), c_o, n_chk)]
        segs_all = segs + chk
        up.sync()   # the batches are generated on this context's stream and read by both
        ms = {"fresh_10M": [], "9M_plus_1M_upserted": []}
        for ctx in (fresh, up):   # warm-up
            for _ in range(3):
                ctx.submit_device_segments(segs)
            ctx.sync()
        for _ in range(max(3, args.rounds)):
            for name, ctx in (("fresh_10M", fresh), ("9M_plus_1M_upserted", up)):
                t = time.perf_counter()
                for _ in range(args.steps):
                    ctx.submit_device_segments(segs)
                ctx.sync()
                ms[name].append((time.perf_counter() - t) / args.steps * 1e3)
        timed_launch = up.launch_info()
        for ctx in (fresh, up):
            ctx.reset()
            ctx.submit_device_segments(chk)
        same = fresh.drain_buckets() == up.drain_buckets() and fresh.stats() == up.stats()
        leg = {"events_per_step": args.events, "counts_equal": same,
               "record_mode": timed_launch["record_mode"], "hbm_table": timed_launch["hbm_table"]}
        for name, v in ms.items():
            leg[name] = {"ms_per_step": [round(x, 3) for x in v], "median": round(statistics.median(v), 3),
                         "G_events_per_s": round(args.events / statistics.median(v) / 1e6, 3)}
        f, u = ms["fresh_10M"], statistics.median(ms["9M_plus_1M_upserted"])
        leg["upserted_median_inside_fresh_range"] = min(f) <= u <= max(f)
        leg["gap_pct_of_fresh_median"] = round((u / statistics.median(f) - 1) * 100, 2)
        out["counting_leg"] = leg
        for (d_b, _, d_o, _) in segs_all:
            up.device_free(d_b)
            up.device_free(d_o)

    log("\n| new ads | wall ms | device ms | first | second | moved | left out |\n|---:|---:|---:|---:|---:|---:|---:|")
    for c in out["cases"]:
        log("| %d | %.3f | %.3f | %d | %d | %d | %d |" % (c["new_ads"], c["wall_ms"], c["device_ms"], c["cuckoo_first"],
                                                         c["cuckoo_second"], c["cuckoo_moved"], c["cuckoo_left_out"]))
    log("| full reload of 9M / 9M again / 10M | %.0f / %.0f / %.0f | | | | | |"
        % (load9 * 1e3, load9b * 1e3, load10 * 1e3))
    log("counting leg:", json.dumps(out["counting_leg"]))
    print(json.dumps(out))
    return 0 if out["every_case_below_reload"] and same else 1


if __name__ == "__main__":
    sys.exit(main())
