"""The drop-in path with LZ4-compressed batches, timed against itself uncompressed.

Same staging as `bench_dropin.py staged --raw`: two distinct ~256 MB batches of configs[1]'s
events, generated once, resubmitted alternately through the pinned double-buffered slots, each
leg with a generator-truth check.  One leg submits the raw lines (ysb_submit_raw: the parent's
path, the yardstick), the other the same batches compressed on the host by blocks
(ysb_submit_raw_lz4: compressed bytes over PCIe, decoded on the GPU).  Two more legs read the
same batches in place from one registered array each, without the pinned slots: `mapped` the
compressed ones (ysb_submit_lz4_mapped) and `raw_mapped` the raw lines (ysb_submit_raw_mapped).
The legs alternate --repeats times in one process.  Plus the decode alone (ysb_lz4_decode_device) at several
block sizes, and a standard frame of 64 KiB blocks through the measure pass and the decode
(ysb_lz4_decode_blocks_device).  --decoder picks the decode kernel; --decoder both runs the
one-wave and the several-wave kernel at every block size, alternated --repeats times -- the
crossover table of DESIGN.md §6 -- and writes it with the frame table to
profiles/lz4_frame_bench.json; --decode-only skips the chain legs.
--legs picks the chain legs; `frame` submits each batch as one standard frame of 64 KiB blocks
(ysb_submit_lz4_blocks): `--legs raw,lz4,frame` is the run of profiles/lz4_frame_chain.json.

Per leg: events/s, the H2D rate (bytes copied / copy time, HIP events on the copy stream), the
copy queue's busy share; for the compressed leg the compression ratio and the decode's rate in
GB/s of output.  Everything goes to profiles/lz4_bench.json and, as one JSON line, to stdout.
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
    ap.add_argument("--block", type=int, default=None, help="LZ4 block size of the chain legs (default: the tools')")
    ap.add_argument("--decode-blocks", default="4096,8192,16384,65536")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--decoder", default="auto", choices=["auto", "narrow", "wide", "both"],
                    help="the decode kernel (ysb_lz4_set_decoder); both: the decode-alone table runs the one-wave and "
                         "the several-wave kernel at every block size, alternated --repeats times (the crossover)")
    ap.add_argument("--legs", default="raw,lz4,raw_mapped,mapped",
                    help="the chain legs, alternated; `frame`: the batches as standard frames of 64 KiB blocks "
                         "(ysb_submit_lz4_blocks); with another set than the default the summary is the legs' medians")
    ap.add_argument("--decode-only", action="store_true", help="skip the chain legs: the decode-alone and frame tables only")
    ap.add_argument("--frame-out", default=os.path.join(ROOT, "profiles", "lz4_frame_bench.json"),
                    help="where --decoder both / --decode-only write their tables")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lz4_bench.json"))
    a = ap.parse_args()

    from ysb_amd import GenParams, YsbContext, lz4
    from ysb_amd._lib import check, lib
    block = a.block or lz4.DEFAULT_BLOCK
    threads = max(1, min(a.threads, 16))
    g = GenParams(seed=42, events_per_sec=100_000)
    _, aids = g.ids()
    per = int((a.slot_mb << 20) // g.max_line_bytes())
    res = {"events_per_batch": per, "slot_MB": a.slot_mb, "block_bytes": block, "repeats": a.repeats, "legs": []}
    with YsbContext(device=a.device, n_campaigns=100, window_ring=1024, timing=True, max_batch_bytes=a.slot_mb << 20,
                    max_batch_events=per, ring_base_bucket=g.c.t0_ms // 10000 - 8) as ctx:
        ctx.load_ad_map(aids, g.ad_campaign_index())
        DEC = {"auto": 0, "narrow": 1, "wide": 2}
        ctx.lz4_set_decoder(DEC.get(a.decoder, 0))
        raw = []
        for s in (0, 1):   # two distinct batches, generated on the device, kept on the host
            cap = per * g.max_line_bytes()
            d_b, d_o = ctx.device_alloc(cap), ctx.device_alloc(4 * per + 64)
            nb = ctx.gen_events_device(g, s * per, per, d_b, cap, d_o)
            raw.append(ctx.d2h(np.empty(nb, dtype=np.uint8), d_b))
            ctx.device_free(d_b)
            ctx.device_free(d_o)
        t0 = time.perf_counter()
        comp = [lz4.pack(r, block, line_aligned=True, threads=threads) for r in raw]
        t_pack = time.perf_counter() - t0
        raw_bytes = sum(r.size for r in raw)
        comp_bytes = sum(b.size for b, _ in comp)
        res["compress"] = {"threads": threads, "seconds": round(t_pack, 3), "GBs_in": round(raw_bytes / t_pack / 1e9, 3),
                           "raw_bytes": raw_bytes, "comp_bytes": comp_bytes, "ratio": round(raw_bytes / comp_bytes, 4),
                           "blocks": [int(d.shape[0]) for _, d in comp],
                           "stored_blocks": [int((d[:, 0] >> 31).sum()) for _, d in comp]}
        log("compressed %d B -> %d B (%.3fx) in %.2f s" % (raw_bytes, comp_bytes, raw_bytes / comp_bytes, t_pack))
        slot = [view(ctx.slot_buffers(s)[0], a.slot_mb << 20) for s in (0, 1)]
        dirs = [np.ascontiguousarray(d, dtype=np.uint32) for _, d in comp]

        def registered(parts):
            """The parts in one 4096-byte aligned array, each at a 64-byte boundary, registered
            with the context: (array, [offset of each part])."""
            at, pos = [], 0
            for p in parts:
                at.append(pos)
                pos += (p.size + 63) // 64 * 64 + 64
            buf = np.empty(pos + 8192, dtype=np.uint8)
            buf = buf[(-buf.ctypes.data) % 4096:][:(pos + 4095) // 4096 * 4096]
            for o, p in zip(at, parts):
                buf[o:o + p.size] = p
            ctx.host_register(buf)
            return buf, at
        reg_comp, at_comp = registered([b for b, _ in comp])
        reg_raw, at_raw = registered(raw)

        legs = [k for k in a.legs.split(",") if k]
        frames = []
        if "frame" in legs and not a.decode_only:   # each batch as one standard frame; its span starts at the first block's data
            for r in raw:
                f = lz4.frame_pack(r, 65536, threads=threads)
                idx, _ = lz4.frame_index(f)
                first = int(idx[0]["offset"])
                frames.append((f[first:], np.ascontiguousarray(idx), first))
            res["frame"] = {"ratio": round(raw_bytes / sum(f.size + fst for f, _, fst in frames), 4),
                            "blocks": [int(i.size) for _, i, _ in frames]}

        def leg(kind):
            for s in (0, 1):   # staged once per leg: the slot's pinned buffer holds what crosses PCIe
                ctx.wait(s)
                if kind in ("raw", "lz4", "frame"):
                    src = raw[s] if kind == "raw" else comp[s][0] if kind == "lz4" else frames[s][0]
                    slot[s][:src.size] = src

            def submit(s):
                if kind == "raw":
                    check(lib().ysb_submit_raw(ctx._h, s, C.c_void_p(slot[s].ctypes.data), raw[s].size), ctx._h)
                elif kind == "raw_mapped":
                    ctx.submit_raw_mapped(reg_raw, at_raw[s], raw[s].size, slot=s)
                elif kind == "frame":   # (base: where the frame's byte 0 would lie in front of the slot's span)
                    check(lib().ysb_submit_lz4_blocks(ctx._h, s, C.c_void_p(slot[s].ctypes.data - frames[s][2]),
                                                      C.c_void_p(frames[s][1].ctypes.data), frames[s][1].size, 0), ctx._h)
                elif kind == "mapped":
                    ctx.submit_lz4_mapped(reg_comp, at_comp[s], comp[s][0].size, dirs[s], slot=s)
                else:
                    check(lib().ysb_submit_raw_lz4(ctx._h, s, C.c_void_p(slot[s].ctypes.data), comp[s][0].size,
                                                   C.c_void_p(dirs[s].ctypes.data), dirs[s].shape[0]), ctx._h)
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
            info = ctx.lz4_info() if kind in ("lz4", "mapped") else ctx.lz4_frame_info() if kind == "frame" else None
            for i in range(nsub):
                ctx.truth_accumulate(g, (i & 1) * per, per)
            mism, truth, counted = ctx.truth_compare()
            n = nsub * per
            out = {"leg": kind, "events": n, "batches": nsub, "seconds": round(el, 4), "events_per_s": round(n / el, 1),
                   "h2d_bytes": cbytes, "h2d_GBs": round(cbytes / (cms * 1e-3) / 1e9, 2) if cms else 0.0,
                   "copy_busy_frac": round(cms * 1e-3 / el, 4), "scan_ms_per_batch": round(kms / max(launches, 1), 4),
                   "check": {"truth_mismatched_cells": mism, "truth_views": truth, "counted_views": counted,
                             "events": st["events"], "parse_errors": st["parse_errors"]}}
            if info:
                out["decode_ms_last_batch"] = round(info["decode_ms"], 4)
                out["decode_GBs_out_last_batch"] = round(info["raw_bytes"] / (info["decode_ms"] * 1e-3) / 1e9, 2) \
                    if info["decode_ms"] else 0.0
                out["bad_blocks"] = info["bad_blocks"]
            log(json.dumps(out))
            return out

        for _ in range(0 if a.decode_only else a.repeats):
            for kind in legs:
                res["legs"].append(leg(kind))
        ctx.sync()
        ctx.host_unregister(reg_comp)
        ctx.host_unregister(reg_raw)

        # the decode alone, device to device, at several block sizes
        res["decode_alone"] = []
        d_out = ctx.device_alloc(raw[0].size + 64)

        def timed_decode(d_in, blob, d):
            ms = []
            for _ in range(7):
                got, bad = ctx.lz4_decode_device(d_in, blob.size, d, d_out, raw[0].size)
                assert got == raw[0].size and bad is None
                ms.append(ctx.lz4_info()["decode_ms"])
            same = bool((ctx.d2h(np.empty(raw[0].size, dtype=np.uint8), d_out) == raw[0]).all())
            med = statistics.median(ms[2:])
            return {"ms": [round(x, 4) for x in ms], "median_ms": round(med, 4),
                    "GBs_out": round(raw[0].size / (med * 1e-3) / 1e9, 2),
                    "GBs_in": round(blob.size / (med * 1e-3) / 1e9, 2), "output_equal": same}

        for bb in [int(x) for x in a.decode_blocks.split(",") if x]:
            blob, d = (comp[0] if bb == block else lz4.pack(raw[0], bb, line_aligned=True, threads=threads))
            d_in = ctx.device_alloc(blob.size + 64)
            ctx.h2d(d_in, blob)
            head = {"block_bytes": bb, "blocks": int(d.shape[0]), "ratio": round(raw[0].size / blob.size, 4)}
            if a.decoder == "both":   # the two kernels alternated: the crossover table
                for rep in range(a.repeats):
                    for name in ("narrow", "wide"):
                        ctx.lz4_set_decoder(DEC[name])
                        res["decode_alone"].append(dict(head, decoder=name, round=rep, **timed_decode(d_in, blob, d)))
                        log(json.dumps(res["decode_alone"][-1]))
                ctx.lz4_set_decoder(0)
            else:
                res["decode_alone"].append(dict(head, decoder=a.decoder, **timed_decode(d_in, blob, d)))
                log(json.dumps(res["decode_alone"][-1]))
            ctx.device_free(d_in)

        # a standard frame of 64 KiB blocks (what lz4 -B4 -BI writes): the measure pass, the
        # descriptors and the decode, device to device (ysb_lz4_decode_blocks_device)
        res["frame_alone"] = []
        frame = lz4.frame_pack(raw[0], 65536, threads=threads)
        index, finfo = lz4.frame_index(frame)
        d_in = ctx.device_alloc(frame.size + 64)
        ctx.h2d(d_in, frame)
        for rep in range(a.repeats if a.decoder == "both" else 1):
            for name in (("narrow", "wide") if a.decoder == "both" else (a.decoder,)):
                ctx.lz4_set_decoder(DEC[name])
                mm, dm = [], []
                for _ in range(7):
                    got, bad = ctx.lz4_decode_blocks_device(d_in, index, d_out, raw[0].size)
                    assert got == raw[0].size and bad is None
                    fi = ctx.lz4_frame_info()
                    mm.append(fi["measure_ms"])
                    dm.append(fi["decode_ms"])
                same = bool((ctx.d2h(np.empty(raw[0].size, dtype=np.uint8), d_out) == raw[0]).all())
                m, dd = statistics.median(mm[2:]), statistics.median(dm[2:])
                res["frame_alone"].append({"decoder": name, "round": rep, "blocks": int(index.size),
                                           "ratio": round(raw[0].size / frame.size, 4),
                                           "measure_ms": round(m, 4), "decode_ms": round(dd, 4),
                                           "measure_GBs_in": round(frame.size / (m * 1e-3) / 1e9, 2),
                                           "GBs_out": round(raw[0].size / ((m + dd) * 1e-3) / 1e9, 2),
                                           "decoder_ran": fi["decoder"], "output_equal": same})
                log(json.dumps(res["frame_alone"][-1]))
        ctx.lz4_set_decoder(DEC.get(a.decoder, 0))
        ctx.device_free(d_in)
        ctx.device_free(d_out)

    if a.decode_only or a.decoder == "both":
        os.makedirs(os.path.dirname(a.frame_out), exist_ok=True)
        with open(a.frame_out, "w") as f:
            json.dump({k: res[k] for k in ("events_per_batch", "slot_MB", "compress", "decode_alone", "frame_alone")}, f, indent=1)
            f.write("\n")
        if a.decode_only:
            print(json.dumps({"decode_alone": len(res["decode_alone"]), "frame_alone": len(res["frame_alone"])}), flush=True)
            return

    def summary(kind):
        v = [l["events_per_s"] for l in res["legs"] if l["leg"] == kind]
        return {"median": statistics.median(v), "min": min(v), "max": max(v)}
    if legs != ["raw", "lz4", "raw_mapped", "mapped"]:
        res["summary"] = {k + "_events_per_s": summary(k) for k in legs}
        res["summary"]["all_checks_exact"] = all(l["check"]["truth_mismatched_cells"] == 0 and
                                                 l["check"]["truth_views"] == l["check"]["counted_views"] for l in res["legs"])
        if "frame" in legs and "raw" in legs:
            res["summary"]["frame_over_raw_median"] = round(summary("frame")["median"] / summary("raw")["median"], 4)
            res["summary"]["frame_median_above_raw_max"] = summary("frame")["median"] > summary("raw")["max"]
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps(res["summary"]), flush=True)
        return
    r, z, rm, zm = summary("raw"), summary("lz4"), summary("raw_mapped"), summary("mapped")
    h2d = statistics.median(l["h2d_GBs"] for l in res["legs"] if l["leg"] == "raw")
    dec = next((x["GBs_out"] for x in res["decode_alone"] if x["block_bytes"] == block), None)
    busy = {k: statistics.median(l["copy_busy_frac"] for l in res["legs"] if l["leg"] == k)
            for k in ("raw", "lz4", "raw_mapped", "mapped")}
    res["summary"] = {"raw_events_per_s": r, "lz4_events_per_s": z, "raw_mapped_events_per_s": rm,
                      "lz4_mapped_events_per_s": zm, "copy_busy_frac_median": busy,
                      "mapped_over_lz4_median": round(zm["median"] / z["median"], 4),
                      # the expectation: in place is not below the slot leg by more than that leg's own spread
                      "mapped_within_lz4_spread": zm["median"] >= z["median"] - (z["max"] - z["min"]),
                      "mapped_over_raw_mapped_median": round(zm["median"] / rm["median"], 4),
                      "ratio": res["compress"]["ratio"],
                      "lz4_over_raw_median": round(z["median"] / r["median"], 4),
                      "lz4_median_above_raw_max": z["median"] > r["max"],
                      "raw_h2d_GBs": h2d, "decode_GBs_out": dec,
                      "decoder_bound": (dec is not None and dec < h2d * res["compress"]["ratio"]),
                      "all_checks_exact": all(l["check"]["truth_mismatched_cells"] == 0 and
                                              l["check"]["truth_views"] == l["check"]["counted_views"] for l in res["legs"])}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["summary"]), flush=True)


if __name__ == "__main__":
    main()
