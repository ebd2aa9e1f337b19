"""The drop-in path fed with Kafka record batches, timed against itself fed with raw lines.

Same staging as `bench_lz4.py`: two distinct batches of configs[1]'s events, generated once,
resubmitted alternately through the double-buffered slots, each leg with a generator-truth check.
One leg submits the raw lines (ysb_submit_raw: the yardstick), one the same events framed as
Kafka record batches through the slots' pinned buffers (ysb_submit_kafka: the framed bytes and the
index cross PCIe, the GPU unframes), one the same framed bytes read in place from a registered
array (ysb_submit_kafka_mapped).  The legs alternate --repeats times in one process, for every
Kafka batch size of --batch-sizes (16 KiB is a producer's default).  Plus the unframing alone
(ysb_kafka_unframe_device: the three kernels timed with HIP events); --unframe-only skips the
chain legs.

Per leg: events/s, bytes over PCIe per event, the copy queue's busy share.  Everything goes to
profiles/kafka_bench.json and, as one JSON line, to stdout.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "streaming-benchmarks_amd"))

import numpy as np  # noqa: E402


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def view(addr, n):
    return np.ctypeslib.as_array((C.c_uint8 * n).from_address(addr))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--events", type=int, default=40_000_000, help="events per timed leg")
    ap.add_argument("--slot-mb", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch-sizes", default="16384,65536,1048576")
    ap.add_argument("--unframe-only", action="store_true", help="skip the chain legs: the three kernels alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kafka_bench.json"))
    a = ap.parse_args()

    from ysb_amd import GenParams, YsbContext, kafka
    from ysb_amd._lib import check, lib
    sizes = [int(x) for x in a.batch_sizes.split(",") if x]
    g = GenParams(seed=42, events_per_sec=100_000)
    _, aids = g.ids()
    slot_bytes = a.slot_mb << 20
    per = int(slot_bytes // (g.max_line_bytes() + 16))   # (the framing's few bytes per record fit the slot too)
    res = {"events_per_batch": per, "slot_MB": a.slot_mb, "repeats": a.repeats, "batch_sizes": sizes, "legs": [],
           "unframe_alone": []}
    with YsbContext(device=a.device, n_campaigns=100, window_ring=1024, timing=True, max_batch_bytes=slot_bytes,
                    max_batch_events=per, ring_base_bucket=g.c.t0_ms // 10000 - 8) as ctx:
        ctx.load_ad_map(aids, g.ad_campaign_index())
        raw, offs = [], []
        for s in (0, 1):   # two distinct batches, generated on the device, kept on the host
            cap = per * g.max_line_bytes()
            d_b, d_o = ctx.device_alloc(cap), ctx.device_alloc(4 * per + 64)
            nb = ctx.gen_events_device(g, s * per, per, d_b, cap, d_o)
            raw.append(ctx.d2h(np.empty(nb, dtype=np.uint8), d_b))
            offs.append(ctx.d2h(np.empty(per, dtype=np.uint32), d_o))
            ctx.device_free(d_b)
            ctx.device_free(d_o)
        raw_bytes = sum(r.size for r in raw)
        slot = [view(ctx.slot_buffers(s)[0], slot_bytes) for s in (0, 1)]

        def leg(kind, blobs, idxs, reg, at):
            for s in (0, 1):   # staged once per leg: the slot's pinned buffer holds what crosses PCIe
                ctx.wait(s)
                if kind in ("raw", "kafka"):
                    src = raw[s] if kind == "raw" else blobs[s]
                    slot[s][:src.size] = src

            def submit(s):
                if kind == "raw":
                    check(lib().ysb_submit_raw(ctx._h, s, C.c_void_p(slot[s].ctypes.data), raw[s].size), ctx._h)
                elif kind == "kafka":
                    check(lib().ysb_submit_kafka(ctx._h, s, C.c_void_p(slot[s].ctypes.data), blobs[s].size,
                                                 C.c_void_p(idxs[s].ctypes.data), idxs[s].size), ctx._h)
                else:
                    ctx.submit_kafka_mapped(reg, at[s], blobs[s].size, idxs[s], slot=s)
            for s in (0, 1, 0, 1):   # warmup
                submit(s)
            ctx.sync()
            ctx.kernel_time()
            ctx.copy_time()
            ctx.reset()
            nsub = max(2, -(-a.events // per))
            t = time.perf_counter()
            for i in range(nsub):
                submit(i & 1)   # waits for the slot's previous H2D inside
            ctx.sync()
            el = time.perf_counter() - t
            kms, launches = ctx.kernel_time()
            cms, copies, cbytes = ctx.copy_time()
            st = ctx.stats()
            info = ctx.kafka_info() if kind != "raw" else None
            for i in range(nsub):
                ctx.truth_accumulate(g, (i & 1) * per, per)
            mism, truth, counted = ctx.truth_compare()
            n = nsub * per
            out = {"leg": kind, "events": n, "batches": nsub, "seconds": round(el, 4), "events_per_s": round(n / el, 1),
                   "h2d_bytes": cbytes, "pcie_bytes_per_event": round(cbytes / n, 2),
                   "h2d_GBs": round(cbytes / (cms * 1e-3) / 1e9, 2) if cms else 0.0,
                   "copy_busy_frac": round(cms * 1e-3 / el, 4), "scan_ms_per_batch": round(kms / max(launches, 1), 4),
                   "check": {"truth_mismatched_cells": mism, "truth_views": truth, "counted_views": counted,
                             "events": st["events"], "parse_errors": st["parse_errors"]}}
            if info:
                out.update(walk_ms_last_batch=round(info["walk_ms"], 4), base_ms_last_batch=round(info["base_ms"], 4),
                           gather_ms_last_batch=round(info["gather_ms"], 4), kafka_batches_last_batch=info["batches"],
                           bad_batches=info["verdict"]["bad_batches"])
            log(json.dumps(out))
            return out

        d_out = ctx.device_alloc(raw[0].size + 64)
        d_off = ctx.device_alloc(4 * (per + 1) + 64)
        for size in sizes:
            t0 = time.perf_counter()
            blobs = [kafka.pack(r, o, batch_bytes=size) for r, o in zip(raw, offs)]
            t_pack = time.perf_counter() - t0
            t0 = time.perf_counter()
            idxs = [np.ascontiguousarray(kafka.index(b)[0]) for b in blobs]
            t_index = time.perf_counter() - t0
            framed = sum(b.size for b in blobs)
            head = {"batch_bytes": size, "framed_bytes": framed, "raw_bytes": raw_bytes,
                    "framing_overhead": round(framed / raw_bytes - 1, 5), "kafka_batches": [int(i.size) for i in idxs],
                    "pack_seconds": round(t_pack, 3), "index_seconds": round(t_index, 4)}
            log(json.dumps(head))
            # the unframing alone, device to device
            d_in = ctx.device_alloc(blobs[0].size)
            ctx.h2d(d_in, blobs[0])
            ms = []
            for _ in range(7):
                n, nb = ctx.kafka_unframe_device(d_in, blobs[0].size, idxs[0], d_out, raw[0].size, d_off, per + 1)
                assert (n, nb) == (per, raw[0].size)
                ki = ctx.kafka_info()
                ms.append((ki["walk_ms"], ki["base_ms"], ki["gather_ms"]))
            same = bool((ctx.d2h(np.empty(raw[0].size, dtype=np.uint8), d_out) == raw[0]).all()) and \
                bool((ctx.d2h(np.empty(per, dtype=np.uint32), d_off) == offs[0]).all())
            w, b, gt = (statistics.median(x[k] for x in ms[2:]) for k in range(3))
            res["unframe_alone"].append(dict(head, walk_ms=round(w, 4), base_ms=round(b, 4), gather_ms=round(gt, 4),
                                             GBs_in=round(blobs[0].size / ((w + b + gt) * 1e-3) / 1e9, 2),
                                             walk_GBs_in=round(blobs[0].size / (w * 1e-3) / 1e9, 2),
                                             gather_GBs_out=round(raw[0].size / (gt * 1e-3) / 1e9, 2), output_equal=same))
            log(json.dumps(res["unframe_alone"][-1]))
            ctx.device_free(d_in)
            if a.unframe_only:
                continue
            at, pos = [], 0
            for p in blobs:
                at.append(pos)
                pos += (p.size + 63) // 64 * 64 + 64 + 1   # (the second batch at an odd address)
            reg = np.empty(pos + 8192, dtype=np.uint8)
            reg = reg[(-reg.ctypes.data) % 4096:][:(pos + 4095) // 4096 * 4096]
            for o, p in zip(at, blobs):
                reg[o:o + p.size] = p
            ctx.host_register(reg)
            for rep in range(a.repeats):
                for kind in ("raw", "kafka", "kafka_mapped"):
                    res["legs"].append(dict(leg(kind, blobs, idxs, reg, at), batch_bytes=size, round=rep))
            ctx.sync()
            ctx.host_unregister(reg)
        ctx.device_free(d_out)
        ctx.device_free(d_off)

    def summary(size, kind):
        v = [l for l in res["legs"] if l["leg"] == kind and l["batch_bytes"] == size]
        e = [l["events_per_s"] for l in v]
        return {"median": statistics.median(e), "min": min(e), "max": max(e),
                "pcie_bytes_per_event": statistics.median(l["pcie_bytes_per_event"] for l in v),
                "copy_busy_frac": statistics.median(l["copy_busy_frac"] for l in v)}
    res["summary"] = {"unframe_alone": [{k: u[k] for k in ("batch_bytes", "walk_ms", "base_ms", "gather_ms", "GBs_in", "output_equal")}
                                        for u in res["unframe_alone"]],
                      "all_unframed_equal": all(u["output_equal"] for u in res["unframe_alone"])}
    if not a.unframe_only:
        for size in sizes:
            r, k, m = (summary(size, x) for x in ("raw", "kafka", "kafka_mapped"))
            res["summary"][str(size)] = {"raw": r, "kafka": k, "kafka_mapped": m,
                                         "kafka_over_raw_median": round(k["median"] / r["median"], 4),
                                         "mapped_over_raw_median": round(m["median"] / r["median"], 4),
                                         "raw_over_framed_bytes": round(r["pcie_bytes_per_event"] / k["pcie_bytes_per_event"], 4)}
        res["summary"]["all_checks_exact"] = all(l["check"]["truth_mismatched_cells"] == 0 and
                                                 l["check"]["truth_views"] == l["check"]["counted_views"] and
                                                 l["check"]["events"] == l["events"] for l in res["legs"])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["summary"]), flush=True)


if __name__ == "__main__":
    main()
