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

With --lz4 the same batches also go LZ4-compressed (attributes codec 3, ysb_submit_kafka_lz4 and
_mapped), alternating with the three legs above in the same process.  The capacity rule of the
compressed submits is 65536 bytes per block, so a slot batch holds slot / 65536 blocks: the
compressed legs submit the first Kafka batches of each staged batch that fit, and say how many.
Per compressed leg also the wire bytes per event, the measured compression ratio, the Kafka batches
per slot batch and which stage bounds it; plus the six kernels alone (measure, plan, decode, walk,
base, gather by HIP events, the median of five after two warm-ups).  Those figures go to
profiles/kafka_lz4_bench.json.

With --snappy (which turns --lz4 on, for the comparison) the same batches also go snappy-compressed
(attributes codec 2 as the Java client's xerial stream of 32 KiB chunks; ysb_kafka_set_codecs, then
the same two submits), alternating with all the legs above in the same process.  A snappy block
counts what its preamble says in the capacity rule, so a slot batch holds every Kafka batch of the
staged one.  Per leg the figures of the LZ4 legs, each also as a ratio to the LZ4 leg of the same
run; plus the chain's kernels alone with the preamble kernel in the measure pass's place.  Those
figures go to profiles/kafka_snappy_bench.json.

With --crc every Kafka leg (with --lz4 the compressed ones too) also runs with each batch's CRC-32C verified: on the device
(ysb_kafka_set_crc: one more launch between the walk and the scan of the totals) and on the host at
index time (ysb_kafka_index with YSB_KAFKA_CHECK_CRC inside the timed loop, once per submit),
alternating with the unverified legs in the same process; plus the CRC kernel alone
(ysb_kafka_crc_device, HIP events).  Per batch size the medians, each verified leg as a ratio to
the unverified leg of the same run, and whether the device leg's median lies within the spread of
the unverified leg's repeats.  Those figures go to profiles/kafka_crc_bench.json.
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
    ap.add_argument("--lz4", action="store_true", help="add the LZ4-compressed legs (profiles/kafka_lz4_bench.json)")
    ap.add_argument("--lz4-out", default=os.path.join(ROOT, "profiles", "kafka_lz4_bench.json"))
    ap.add_argument("--snappy", action="store_true", help="add the snappy legs beside the LZ4 ones (profiles/kafka_snappy_bench.json)")
    ap.add_argument("--snappy-out", default=os.path.join(ROOT, "profiles", "kafka_snappy_bench.json"))
    ap.add_argument("--crc", action="store_true", help="add the CRC-verified legs (profiles/kafka_crc_bench.json)")
    ap.add_argument("--crc-out", default=os.path.join(ROOT, "profiles", "kafka_crc_bench.json"))
    a = ap.parse_args()
    a.lz4 = a.lz4 or a.snappy

    from ysb_amd import GenParams, YsbContext, kafka
    from ysb_amd._lib import check, lib
    sizes = [int(x) for x in a.batch_sizes.split(",") if x]
    g = GenParams(seed=42, events_per_sec=100_000)
    _, aids = g.ids()
    slot_bytes = a.slot_mb << 20
    per = int(slot_bytes // (g.max_line_bytes() + 16))   # (the framing's few bytes per record fit the slot too)
    res = {"events_per_batch": per, "slot_MB": a.slot_mb, "repeats": a.repeats, "batch_sizes": sizes, "legs": [],
           "unframe_alone": []}
    zres = {"events_per_raw_batch": per, "slot_MB": a.slot_mb, "repeats": a.repeats, "batch_sizes": sizes,
            "blocks_per_slot_batch_cap": slot_bytes // 65536, "legs": [], "kernels_alone": []}
    sres = {"events_per_raw_batch": per, "slot_MB": a.slot_mb, "repeats": a.repeats, "batch_sizes": sizes,
            "framing": "xerial, 32 KiB chunks", "legs": [], "kernels_alone": []}
    cres = {"events_per_batch": per, "slot_MB": a.slot_mb, "repeats": a.repeats, "batch_sizes": sizes, "legs": [],
            "kernel_alone": []}
    with YsbContext(device=a.device, n_campaigns=100, window_ring=1024, timing=True, max_batch_bytes=slot_bytes,
                    max_batch_events=per, ring_base_bucket=g.c.t0_ms // 10000 - 8) as ctx:
        ctx.load_ad_map(aids, g.ad_campaign_index())
        if a.snappy:
            ctx.kafka_set_codecs(("lz4", "snappy"))
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

        def leg(kind, blobs, idxs, reg, at, crc="off"):
            ctx.kafka_set_crc(1 if crc == "device" else 0)
            for s in (0, 1):   # staged once per leg: the slot's pinned buffer holds what crosses PCIe
                ctx.wait(s)
                if kind in ("raw", "kafka"):
                    src = raw[s] if kind == "raw" else blobs[s]
                    slot[s][:src.size] = src

            def submit(s):
                if crc == "host":   # what a caller without the device check does per fetch response: a pass over the bytes
                    assert kafka.index(blobs[s], check_crc=True)[1]["crc_checked"] == idxs[s].size
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
            cinfo = ctx.kafka_crc_info() if crc == "device" else None
            ctx.kafka_set_crc(0)
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
            if crc != "off":
                out["leg"] = kind + "+crc_" + crc
            if cinfo:
                out.update(crc_ms_last_batch=round(cinfo["crc_ms"], 4), crc_batches_last_batch=cinfo["batches"],
                           crc_bad_batches=cinfo["bad_batches"], crc_calls=cinfo["calls"])
            log(json.dumps(out))
            return out

        def leg_lz4(kind, z, reg, at, crc="off"):
            """A compressed leg: z holds per staged batch the wire bytes, the three index arrays and
            the events of the Kafka batches that fit a slot batch by the capacity rule."""
            ctx.kafka_set_crc(1 if crc == "device" else 0)
            for s in (0, 1):
                ctx.wait(s)
                if kind in ("kafka_lz4", "kafka_snappy"):
                    slot[s][:z["blobs"][s].size] = z["blobs"][s]

            def submit(s):
                b, i, f, k = z["blobs"][s], z["idx"][s], z["frames"][s], z["blocks"][s]
                if crc == "host":
                    assert kafka.index_lz4(b, check_crc=True, accept_snappy=a.snappy)[3]["crc_checked"] == i.size
                if kind in ("kafka_lz4", "kafka_snappy"):
                    check(lib().ysb_submit_kafka_lz4(ctx._h, s, C.c_void_p(slot[s].ctypes.data), b.size, C.c_void_p(i.ctypes.data),
                                                     C.c_void_p(f.ctypes.data), i.size, C.c_void_p(k.ctypes.data), k.size), ctx._h)
                else:
                    ctx.submit_kafka_lz4_mapped(reg, at[s], b.size, i, f, k, slot=s)
            for s in (0, 1, 0, 1):   # warmup
                submit(s)
            ctx.sync()
            ctx.kernel_time()
            ctx.copy_time()
            ctx.reset()
            ev = z["events"]
            nsub = max(2, -(-a.events // min(ev)))
            t = time.perf_counter()
            for i in range(nsub):
                submit(i & 1)
            ctx.sync()
            el = time.perf_counter() - t
            kms, launches = ctx.kernel_time()
            cms, copies, cbytes = ctx.copy_time()
            st = ctx.stats()
            info, li = ctx.kafka_info(), ctx.kafka_lz4_info()
            cinfo = ctx.kafka_crc_info() if crc == "device" else None
            ctx.kafka_set_crc(0)
            for i in range(nsub):
                ctx.truth_accumulate(g, (i & 1) * per, ev[i & 1])
            mism, truth, counted = ctx.truth_compare()
            n = sum(ev[i & 1] for i in range(nsub))
            stages = {k: round(v, 4) for k, v in (("measure", li["measure_ms"]), ("plan", li["plan_ms"]), ("decode", li["decode_ms"]),
                                                   ("walk", info["walk_ms"]), ("base", info["base_ms"]), ("gather", info["gather_ms"]))}
            if li["snappy_blocks"]:
                stages["preamble"] = round(li["preamble_ms"], 4)
            chain_ms = sum(stages.values())
            busy = cms * 1e-3 / el
            chain_share = chain_ms * 1e-3 * nsub / el     # (the last batch's kernels, taken for every batch)
            bound = "the copy queue" if busy >= 0.9 else \
                ("the %s kernel (the chain's kernels take %.0f%% of the leg)" % (max(stages, key=stages.get), 100 * chain_share)
                 if chain_share >= 0.6 else "the host's submit path (copy queue %.0f%% busy, chain kernels %.0f%%)" % (100 * busy, 100 * chain_share))
            out = {"leg": kind, "events": n, "batches": nsub, "seconds": round(el, 4), "events_per_s": round(n / el, 1),
                   "h2d_bytes": cbytes, "wire_bytes_per_event": round(cbytes / n, 2),
                   "h2d_GBs": round(cbytes / (cms * 1e-3) / 1e9, 2) if cms else 0.0, "copy_busy_frac": round(busy, 4),
                   "scan_ms_per_batch": round(kms / max(launches, 1), 4), "stage_ms_last_batch": stages,
                   "chain_ms_last_batch": round(chain_ms, 4), "bound": bound, "kafka_batches_per_slot_batch": int(z["idx"][0].size),
                   "blocks_last_batch": li["blocks"], "inflated_bytes_last_batch": li["inflated_bytes"],
                   "compression_ratio": round(li["inflated_bytes"] / max(li["wire_bytes"], 1), 4), "decoder": li["decoder"],
                   "bad_batches": info["verdict"]["bad_batches"],
                   "check": {"truth_mismatched_cells": mism, "truth_views": truth, "counted_views": counted,
                             "events": st["events"], "parse_errors": st["parse_errors"]}}
            if crc != "off":
                out["leg"] = kind + "+crc_" + crc
            if cinfo:
                out.update(crc_ms_last_batch=round(cinfo["crc_ms"], 4), crc_batches_last_batch=cinfo["batches"],
                           crc_bad_batches=cinfo["bad_batches"], crc_calls=cinfo["calls"])
            log(json.dumps(out))
            return out

        def lz4_staging(size, codec="lz4"):
            """The staged batches compressed, cut to the Kafka batches a slot batch may hold."""
            z = {"blobs": [], "idx": [], "frames": [], "blocks": [], "events": [], "batch_bytes": size}
            t0 = time.perf_counter()
            for r, o in zip(raw, offs):
                blob = kafka.pack(r, o, batch_bytes=size, codec=codec)
                idx, fr, bl, _ = kafka.index_lz4(blob, accept_snappy=codec == "snappy")
                ends = np.cumsum(kafka.inflate_bounds(blob, idx, fr, bl))   # the capacity rule: 65536 per block, a snappy block its preamble
                keep = int(np.searchsorted(ends, slot_bytes, side="right"))
                keep = min(keep, idx.size)
                nblk = int(fr["n_blocks"][:keep].sum())
                end = int(idx[keep - 1]["records_off"]) + int(idx[keep - 1]["records_bytes"])
                z["blobs"].append(np.ascontiguousarray(blob[:end]))
                z["idx"].append(np.ascontiguousarray(idx[:keep]))
                z["frames"].append(np.ascontiguousarray(fr[:keep]))
                z["blocks"].append(np.ascontiguousarray(bl[:nblk]))
                z["events"].append(int(idx["n_records"][:keep].sum()))
            z["pack_seconds"] = round(time.perf_counter() - t0, 3)
            return z

        def lz4_kernels_alone(z):
            """measure, plan, decode, walk, base, gather of the first staged batch, device to device."""
            b, i, f, k, n = z["blobs"][0], z["idx"][0], z["frames"][0], z["blocks"][0], z["events"][0]
            nval = int(offs[0][n]) if n < per else raw[0].size
            d_in = ctx.device_alloc(b.size)
            ctx.h2d(d_in, b)
            rows = []
            for _ in range(7):
                got = ctx.kafka_unframe_lz4_device(d_in, b.size, i, f, k, d_out, raw[0].size, d_off, per + 1)
                assert got == (n, nval), (got, n, nval)
                ki, li = ctx.kafka_info(), ctx.kafka_lz4_info()
                rows.append((li["measure_ms"], li["plan_ms"], li["decode_ms"], ki["walk_ms"], ki["base_ms"], ki["gather_ms"],
                             li["preamble_ms"]))
            same = bool((ctx.d2h(np.empty(nval, dtype=np.uint8), d_out) == raw[0][:nval]).all()) and \
                bool((ctx.d2h(np.empty(n, dtype=np.uint32), d_off) == offs[0][:n]).all())
            med = [statistics.median(r[c] for r in rows[2:]) for c in range(6)]
            pre_ms = statistics.median(r[6] for r in rows[2:])
            out = {"batch_bytes": z["batch_bytes"], "kafka_batches": int(i.size), "blocks": int(k.size), "events": n,
                   "wire_bytes": int(b.size), "inflated_bytes": li["inflated_bytes"], "value_bytes": nval,
                   "compression_ratio": round(li["inflated_bytes"] / b.size, 4), "decoder": li["decoder"],
                   "output_equal": same}
            out.update({nm + "_ms": round(v, 4) for nm, v in zip(("measure", "plan", "decode", "walk", "base", "gather"), med)})
            if li["snappy_blocks"]:
                out.update(snappy_blocks=li["snappy_blocks"], preamble_ms=round(pre_ms, 4))
                med = med + [pre_ms]
            out["decode_GBs_out"] = round(li["inflated_bytes"] / (med[2] * 1e-3) / 1e9, 2) if med[2] else 0.0
            out["chain_GBs_out"] = round(li["inflated_bytes"] / (sum(med) * 1e-3) / 1e9, 2) if sum(med) else 0.0
            ctx.device_free(d_in)
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
            if a.crc:   # the CRC kernel alone over the same bytes
                cms_ = []
                for _ in range(7):
                    got, stored = ctx.kafka_crc_device(d_in, blobs[0].size, idxs[0])
                    cms_.append(ctx.kafka_crc_info()["crc_ms"])
                ci = ctx.kafka_crc_info()
                cm = statistics.median(cms_[2:])
                cres["kernel_alone"].append({"batch_bytes": size, "kafka_batches": int(idxs[0].size), "verified_bytes": ci["bytes"],
                                             "crc_ms": round(cm, 4), "GBs": round(ci["bytes"] / (cm * 1e-3) / 1e9, 2) if cm else 0.0,
                                             "all_equal_stored": bool((got == stored).all()), "grid_waves": ci["grid_waves"]})
                log(json.dumps(cres["kernel_alone"][-1]))
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
            z = zreg = zat = y = yreg = yat = None
            if a.snappy:   # the snappy staging, its kernels alone, its registered copy
                y = lz4_staging(size, "snappy")
                sres["kernels_alone"].append(lz4_kernels_alone(y))
                yat, ypos = [], 0
                for p in y["blobs"]:
                    yat.append(ypos)
                    ypos += (p.size + 63) // 64 * 64 + 64 + 1
                yreg = np.empty(ypos + 8192, dtype=np.uint8)
                yreg = yreg[(-yreg.ctypes.data) % 4096:][:(ypos + 4095) // 4096 * 4096]
                for o, p in zip(yat, y["blobs"]):
                    yreg[o:o + p.size] = p
                ctx.host_register(yreg)
            if a.lz4:   # the compressed staging, its kernels alone, its registered copy (the second batch at an odd address)
                z = lz4_staging(size)
                zres["kernels_alone"].append(lz4_kernels_alone(z))
                zat, zpos = [], 0
                for p in z["blobs"]:
                    zat.append(zpos)
                    zpos += (p.size + 63) // 64 * 64 + 64 + 1
                zreg = np.empty(zpos + 8192, dtype=np.uint8)
                zreg = zreg[(-zreg.ctypes.data) % 4096:][:(zpos + 4095) // 4096 * 4096]
                for o, p in zip(zat, z["blobs"]):
                    zreg[o:o + p.size] = p
                ctx.host_register(zreg)
            for rep in range(a.repeats):
                for kind in ("raw", "kafka", "kafka_mapped"):
                    res["legs"].append(dict(leg(kind, blobs, idxs, reg, at), batch_bytes=size, round=rep))
                    if z and kind == "raw":
                        zres["legs"].append(dict(res["legs"][-1]))
                    if y and kind == "raw":
                        sres["legs"].append(dict(res["legs"][-1]))
                if a.crc:
                    for kind, crc in (("kafka", "device"), ("kafka", "host"), ("kafka_mapped", "device"), ("kafka_mapped", "host")):
                        cres["legs"].append(dict(leg(kind, blobs, idxs, reg, at, crc), batch_bytes=size, round=rep))
                for kind in (("kafka_lz4", "kafka_lz4_mapped") if z else ()):
                    zres["legs"].append(dict(leg_lz4(kind, z, zreg, zat), batch_bytes=size, round=rep))
                    if y:
                        sres["legs"].append(dict(zres["legs"][-1]))
                    if a.crc:
                        for crc in ("device", "host"):
                            cres["legs"].append(dict(leg_lz4(kind, z, zreg, zat, crc), batch_bytes=size, round=rep))
                for kind in (("kafka_snappy", "kafka_snappy_mapped") if y else ()):
                    sres["legs"].append(dict(leg_lz4(kind, y, yreg, yat), batch_bytes=size, round=rep))
            ctx.sync()
            ctx.host_unregister(reg)
            if z:
                ctx.host_unregister(zreg)
            if y:
                ctx.host_unregister(yreg)
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
    if a.crc:
        cs = {"kernel_alone": cres["kernel_alone"]}
        for size in (sizes if not a.unframe_only else []):
            cs[str(size)] = {}
            for kind in ("kafka", "kafka_mapped") + (("kafka_lz4", "kafka_lz4_mapped") if a.lz4 else ()):
                off = [l["events_per_s"] for l in res["legs"] + zres["legs"] if l["leg"] == kind and l["batch_bytes"] == size]
                row = {"off": {"median": statistics.median(off), "min": min(off), "max": max(off)}}
                for crc in ("device", "host"):
                    e = [l["events_per_s"] for l in cres["legs"] if l["leg"] == kind + "+crc_" + crc and l["batch_bytes"] == size]
                    row[crc] = {"median": statistics.median(e), "min": min(e), "max": max(e),
                                "over_off_median": round(statistics.median(e) / statistics.median(off), 4)}
                row["device_median_within_off_spread"] = min(off) <= row["device"]["median"] <= max(off)
                cms_ = [l["crc_ms_last_batch"] for l in cres["legs"] if l["leg"] == kind + "+crc_device" and l["batch_bytes"] == size]
                row["crc_ms_last_batch_median"] = statistics.median(cms_)
                cs[str(size)][kind] = row
        cs["all_checks_exact"] = all(l["check"]["truth_mismatched_cells"] == 0 and l["check"]["truth_views"] == l["check"]["counted_views"]
                                     and l["check"]["events"] == l["events"] and l.get("crc_bad_batches", 0) == 0
                                     for l in cres["legs"])
        cres["summary"] = cs
        with open(a.crc_out, "w") as f:
            json.dump(cres, f, indent=1)
            f.write("\n")
        print(json.dumps(cs), flush=True)
    if a.lz4 and not a.unframe_only:
        zs = {"kernels_alone": zres["kernels_alone"], "all_inflated_equal": all(u["output_equal"] for u in zres["kernels_alone"])}
        for size in sizes:
            def of(kind):
                return [l for l in zres["legs"] if l["leg"] == kind and l["batch_bytes"] == size]
            rawm = statistics.median(l["events_per_s"] for l in of("raw"))
            zs[str(size)] = {"raw_median_events_per_s": rawm}
            for kind in ("kafka_lz4", "kafka_lz4_mapped"):
                v = of(kind)
                e = [l["events_per_s"] for l in v]
                zs[str(size)][kind] = {
                    "M_events_per_s": {"min": round(min(e) / 1e6, 2), "median": round(statistics.median(e) / 1e6, 2),
                                       "max": round(max(e) / 1e6, 2)},
                    "over_raw_median": round(statistics.median(e) / rawm, 4),
                    "wire_bytes_per_event": statistics.median(l["wire_bytes_per_event"] for l in v),
                    "compression_ratio": statistics.median(l["compression_ratio"] for l in v),
                    "copy_busy_frac": statistics.median(l["copy_busy_frac"] for l in v),
                    "kafka_batches_per_slot_batch": v[0]["kafka_batches_per_slot_batch"],
                    "events_per_slot_batch": v[0]["events"] // v[0]["batches"], "bound": v[-1]["bound"]}
        zs["all_checks_exact"] = all(l["check"]["truth_mismatched_cells"] == 0 and l["check"]["truth_views"] == l["check"]["counted_views"]
                                     and l["check"]["events"] == l["events"] and l.get("bad_batches", 0) == 0 for l in zres["legs"])
        zres["summary"] = zs
        with open(a.lz4_out, "w") as f:
            json.dump(zres, f, indent=1)
            f.write("\n")
        print(json.dumps(zs), flush=True)
    if a.snappy and not a.unframe_only:
        ss = {"kernels_alone": sres["kernels_alone"], "all_inflated_equal": all(u["output_equal"] for u in sres["kernels_alone"])}
        for size in sizes:
            def sof(kind):
                return [l for l in sres["legs"] if l["leg"] == kind and l["batch_bytes"] == size]
            rawm = statistics.median(l["events_per_s"] for l in sof("raw"))
            ss[str(size)] = {"raw_median_events_per_s": rawm}
            for kind, other in (("kafka_snappy", "kafka_lz4"), ("kafka_snappy_mapped", "kafka_lz4_mapped")):
                v = sof(kind)
                e = [l["events_per_s"] for l in v]
                lz = statistics.median(l["events_per_s"] for l in sof(other))
                ss[str(size)][kind] = {
                    "M_events_per_s": {"min": round(min(e) / 1e6, 2), "median": round(statistics.median(e) / 1e6, 2),
                                       "max": round(max(e) / 1e6, 2)},
                    "over_raw_median": round(statistics.median(e) / rawm, 4),
                    "over_" + other + "_median": round(statistics.median(e) / lz, 4),
                    other + "_M_events_per_s_median": round(lz / 1e6, 2),
                    "wire_bytes_per_event": statistics.median(l["wire_bytes_per_event"] for l in v),
                    other + "_wire_bytes_per_event": statistics.median(l["wire_bytes_per_event"] for l in sof(other)),
                    "compression_ratio": statistics.median(l["compression_ratio"] for l in v),
                    "copy_busy_frac": statistics.median(l["copy_busy_frac"] for l in v),
                    "kafka_batches_per_slot_batch": v[0]["kafka_batches_per_slot_batch"],
                    "events_per_slot_batch": v[0]["events"] // v[0]["batches"], "bound": v[-1]["bound"]}
        ss["all_checks_exact"] = all(l["check"]["truth_mismatched_cells"] == 0 and l["check"]["truth_views"] == l["check"]["counted_views"]
                                     and l["check"]["events"] == l["events"] and l.get("bad_batches", 0) == 0 for l in sres["legs"])
        sres["summary"] = ss
        with open(a.snappy_out, "w") as f:
            json.dump(sres, f, indent=1)
            f.write("\n")
        print(json.dumps(ss), flush=True)
    print(json.dumps(res["summary"]), flush=True)


if __name__ == "__main__":
    main()
