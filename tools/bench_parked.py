#!/usr/bin/env python3
"""Parked views (ysb_parked_enable / _keys / _resolve): first measurements, no target set.

In one run on one GPU, on a device-generated batch (1,000 campaigns x 10 ads by default):
  * the launch with parking off and on, the map complete (nothing parks): what the route
    through the deferred-line kernel's park site costs when there is nothing to park;
  * a cold start: an empty map, every view parked -- the launch, the distinct kernel and, after
    an upsert of every ad, the resolve, in device ms and ns per record;
  * a 1 %-unknown stream: one ad in a hundred withheld from the load, then the same.
Launch times are wall times around submit_device + sync (median of --steps); the distinct and
resolve times are the library's own HIP-event times (ysb_parked_desc).

Prints a markdown table (stderr) and one JSON line (stdout), and writes the JSON to
profiles/parked_bench.json.
  python tools/bench_parked.py [--device 0] [--events 4000000] [--steps 5]
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


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--events", type=int, default=4_000_000)
    ap.add_argument("--campaigns", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "parked_bench.json"))
    args = ap.parse_args()
    from ysb_amd import GenParams, YsbContext

    g = GenParams(seed=42, n_campaigns=args.campaigns, ads_per_campaign=10, events_per_sec=100_000)
    _, ads = g.ids()
    camp = g.ad_campaign_index()
    n = args.events
    out = {"events": n, "campaigns": args.campaigns, "ads": len(ads), "steps": args.steps, "cases": []}

    def case(name, loaded, capacity):
        """Median launch ms over --steps launches of the batch on a map of the ads `loaded`; with
        parking each is followed by a resolve without an upsert (every record a join miss), and
        one more launch by the whole loop: keys, an upsert of every ad, the resolve that joins."""
        with YsbContext(device=args.device, n_campaigns=args.campaigns, window_ring=128,
                        max_batch_bytes=1 << 20, max_batch_events=1 << 12) as ctx:
            ctx.load_ad_map([ads[i] for i in loaded], [camp[i] for i in loaded])
            cap = n * g.max_line_bytes()
            d_b, d_o = ctx.device_alloc(cap), ctx.device_alloc(4 * n)
            nb = ctx.gen_events_device(g, 0, n, d_b, cap, d_o)
            if capacity:
                ctx.park_misses(capacity)
            ctx.submit_device(d_b, nb, d_o, n)     # warm-up: code objects, buffers, the ring's base
            ctx.sync()
            if capacity:
                ctx.resolve_parked()
            ctx.reset()
            ms, row = [], {"case": name, "loaded_ads": len(loaded), "capacity": capacity}
            for step in range(args.steps):
                t = time.perf_counter()
                ctx.submit_device(d_b, nb, d_o, n)
                ctx.sync()
                ms.append((time.perf_counter() - t) * 1e3)
                if capacity:
                    info = ctx.resolve_parked()    # nothing upserted: every record a join miss
                    row.update(resolve_all_missed_ms=info["resolve_ms"])
                    assert info["dropped"] == 0
            if capacity:                           # once more, now with the lookup loop: keys, upsert, resolve
                ctx.submit_device(d_b, nb, d_o, n)
                ctx.sync()
                t = time.perf_counter()
                keys = ctx.parked_keys()
                keys_ms = (time.perf_counter() - t) * 1e3
                info = ctx.parked_info()
                row.update(parked=info["parked"], distinct_keys=len(keys), distinct_ms=info["distinct_ms"],
                           keys_wall_ms=keys_ms)
                t = time.perf_counter()
                up = ctx.upsert_ad_map(ads, camp) if keys else None
                row.update(upsert_wall_ms=(time.perf_counter() - t) * 1e3, upsert_rebuilt=up["rebuilt"] if up else 0)
                t = time.perf_counter()
                info = ctx.resolve_parked()
                row.update(resolve_ms=info["resolve_ms"], resolve_wall_ms=(time.perf_counter() - t) * 1e3,
                           resolved_joined=info["resolved_joined"], resolved_missed=info["resolved_missed"])
                k = info["resolved_missed"] + info["resolved_joined"]
                if k:
                    row.update(distinct_ns_per_record=row["distinct_ms"] * 1e6 / k,
                               resolve_ns_per_record=row["resolve_ms"] * 1e6 / k)
            row.update(launch_ms=[round(x, 4) for x in ms], launch_ms_median=statistics.median(ms),
                       events_per_s=n / (statistics.median(ms) * 1e-3), stats=ctx.stats())
            out["cases"].append(row)
            log("| %s | %d | %.3f | %s | %s | %s | %s |" % (
                name, row["loaded_ads"], row["launch_ms_median"], row.get("parked", "-"), row.get("distinct_keys", "-"),
                "%.3f" % row["distinct_ms"] if "distinct_ms" in row else "-",
                "%.3f" % row["resolve_ms"] if "resolve_ms" in row else "-"))

    every = list(range(len(ads)))
    log("| case | ads loaded | launch ms (median) | parked | distinct keys | distinct ms | resolve ms |")
    log("|---|---:|---:|---:|---:|---:|---:|")
    case("parking off, complete map", every, 0)
    case("parking on, complete map", every, 1 << 16)
    case("parking off, 1 % of the ads unknown", [i for i in every if i % 100], 0)
    case("parking on, 1 % of the ads unknown", [i for i in every if i % 100], n)
    case("parking on, cold start (every view parks)", [], n)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
