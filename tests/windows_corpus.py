"""Boundary corpus and model of the window arithmetic: bucket = Long.parseLong(event_time) /
time_divisor (Java long division, truncating toward zero), for any divisor >= 1 and for
negative, zero and huge event times.

Pure Python and numpy: nothing of the library or of the oracles is imported here, so the
expected rows rest on `jdiv` alone.  The carrier lines are the joined views of
tests/golden/gen_s7.* (every boundary time lands on a line that is counted)."""
from __future__ import annotations

import functools
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LONG_MAX = (1 << 63) - 1
LONG_MIN = -(1 << 63)

# every divisor the corpus is built for (tests/test_windows_corpus.py, tests/test_gpu_windows.py)
D = [1, 2, 3, 7, 1000, 9999, 10000, 10001, 60000, 86_400_000, (1 << 40) + 3, (1 << 62) + 12345, LONG_MAX]

# (fmt, layout): the generator's JSON, compact JSON (no spaces), another key order (the flat /
# learned-order tier), the fork's .tbl rows, and generator lines whose time string carries a
# \u00XX escape (span_long's decode_str branch, the deferred-line kernel)
LAYOUTS = [("json", "generator"), ("json", "compact"), ("json", "reordered"), ("tbl", "tbl"), ("json", "escape")]

KEYS = ("user_id", "page_id", "ad_id", "ad_type", "event_type", "event_time", "ip_address")
REORDERED = ("event_time", "ad_id", "user_id", "event_type", "page_id", "ip_address", "ad_type")


def jdiv(t: int, d: int) -> int:
    """Java long division on Python ints: the magnitude floor-divided, the sign restored."""
    q = abs(t) // d
    return -q if t < 0 else q


def boundary_times(d: int):
    """The event times (ms) around every edge of the arithmetic for divisor d, in the long range."""
    out = []
    for k in list(range(-3, 4)) + [-170_000_000, 170_000_000]:
        out += [k * d + e for e in (-1, 0, 1)]
    edge = (1_700_000_000_000 // d + 1) * d            # a bucket edge near 1.7e12
    out += [edge - 1, edge]
    out += [999999999999, 1000000000000, 9999999999999]   # 12 / 13 digits: the SWAR tier's edges
    out += [1 << 62, -(1 << 62), (1 << 62) - 1, LONG_MAX - 1, LONG_MIN + 1]
    if d >= 2:                                          # at d = 1 the bucket Long.MAX has no [lo, hi) range
        out += [LONG_MAX, LONG_MIN]
    seen, uniq = set(), []
    for t in out:
        if LONG_MIN <= t <= LONG_MAX and t not in seen:
            seen.add(t)
            uniq.append(t)
    return uniq


def forms(t: int):
    """The strings Long.parseLong reads as t.  Their lengths select the three parsers: exactly
    13 bytes (the SWAR digits; with a sign among them the fallback), <= 20 (registers), > 20
    (the byte loop)."""
    mag = str(abs(t))
    out = []
    if t >= 0:
        out += [mag, "+" + mag, "0" + mag, "000" + mag]
        out += [mag.rjust(w, "0") for w in (13, 19, 20, 21) if len(mag) <= w]
        if len(mag) <= 12:
            out.append("+" + mag.rjust(12, "0"))         # 13 bytes, one of them a sign
        if t == 0:
            out += ["-0", "-" + "0" * 12]
    else:
        out += ["-" + mag, "-0" + mag, "-000" + mag]
        out += ["-" + mag.rjust(w, "0") for w in (13, 19, 20) if len(mag) <= w]
        if len(mag) <= 12:
            out.append("-" + mag.rjust(12, "0"))         # 13 bytes, one of them a sign
    uniq = []
    for s in out:
        if s not in uniq:
            uniq.append(s)
    assert all(int(s) == t for s in uniq)
    return uniq


@functools.lru_cache(maxsize=None)
def campaign_index():
    with open(os.path.join(GOLDEN, "gen_s7.campaign_ids.txt")) as f:
        return {ln.strip(): i for i, ln in enumerate(x for x in f if x.strip())}


@functools.lru_cache(maxsize=None)
def _ad_map():
    """ad uuid -> campaign index (gen_s7.ad_to_campaign.txt: one {"AD": "CAMPAIGN"} per line)."""
    idx = campaign_index()
    m = {}
    with open(os.path.join(GOLDEN, "gen_s7.ad_to_campaign.txt")) as f:
        for ln in f:
            if ln.strip():
                for a, c in json.loads(ln).items():
                    m[a] = idx[c]
    return m


def ad_arrays():
    """(ad ids, campaign indices) of the fixture's map, as load_ad_map / oracle.AdMap take them."""
    m = _ad_map()
    return list(m), list(m.values())


@functools.lru_cache(maxsize=None)
def _carriers():
    """The generator events of gen_s7.jsonl that are views of an ad in the map, as dicts."""
    m = _ad_map()
    out = []
    with open(os.path.join(GOLDEN, "gen_s7.jsonl"), "rb") as f:
        for ln in f.read().split(b"\n"):
            if ln:
                ev = json.loads(ln)
                if ev["event_type"] == "view" and ev["ad_id"] in m:
                    assert list(ev) == list(KEYS)
                    out.append(ev)
    return out


def _escape_first_digit(s: str) -> str:
    for i, ch in enumerate(s):
        if ch.isdigit():
            return s[:i] + "\\u00%02x" % ord(ch) + s[i + 1:]
    raise ValueError(s)


def _render(ev, time_str, layout):
    v = dict(ev, event_time=time_str)
    if layout == "tbl":
        return ("|".join(v[k] for k in KEYS[:6]) + "\n").encode()
    if layout == "compact":
        return ("{" + ",".join('"%s":"%s"' % (k, v[k]) for k in KEYS) + "}\n").encode()
    if layout == "escape":
        v["event_time"] = _escape_first_digit(time_str)
    order = REORDERED if layout == "reordered" else KEYS
    return ("{" + ", ".join('"%s": "%s"' % (k, v[k]) for k in order) + "}\n").encode()


def carrier_lines(fmt, layout):
    """The carrier events rendered in a layout with their own times: (line, campaign) pairs,
    every one a view of an ad in the map."""
    _check(fmt, layout)
    m = _ad_map()
    return [(_render(ev, ev["event_time"], layout), m[ev["ad_id"]]) for ev in _carriers()]


def _check(fmt, layout):
    if (fmt, layout) not in LAYOUTS:
        raise ValueError("unknown (fmt, layout): %r" % ((fmt, layout),))


def records(d, fmt, layout, bound=None, smallest_first=False):
    """[(line, campaign, t)]: every form of every boundary time of d on a carrier of its own
    (the carriers repeat when the forms outnumber them).  bound: only times with |t| <= bound
    (the GPU's d = 1 runs stay inside +-2^62: include/ysb_hip.h, the bucket range).
    smallest_first: the smallest time's lines moved to the front."""
    _check(fmt, layout)
    m = _ad_map()
    evs = _carriers()
    times = [t for t in boundary_times(d) if bound is None or abs(t) <= bound]
    if smallest_first:
        times.sort()
    out = []
    for t in times:
        for s in forms(t):
            ev = evs[len(out) % len(evs)]
            out.append((_render(ev, s, layout), m[ev["ad_id"]], t))
    return out


def rows_of(recs, d):
    """{(campaign, bucket): count} of records, by jdiv alone."""
    rows = {}
    for _, c, t in recs:
        k = (c, jdiv(t, d))
        rows[k] = rows.get(k, 0) + 1
    return rows


def stats_of(recs):
    n = len(recs)
    return {"events": n, "views": n, "joined": n, "join_misses": 0, "parse_errors": 0, "time_errors": 0}


def build(d, fmt, layout, **kw):
    """(lines, expected_rows {(campaign, bucket): count}, expected_stats)."""
    recs = records(d, fmt, layout, **kw)
    return [r[0] for r in recs], rows_of(recs, d), stats_of(recs)


def batch(lines):
    """(raw bytes as a uint8 array, uint32 line offsets) of lines submitted as one batch."""
    raw = np.frombuffer(b"".join(lines), dtype=np.uint8)
    offs = np.cumsum([0] + [len(x) for x in lines[:-1]]).astype(np.uint32)
    return raw, offs


def lines_of_cells(recs, d, cells):
    """The records that count into any of `cells` (for a failure message)."""
    cells = set(cells)
    return [(i, r[0]) for i, r in enumerate(recs) if (r[1], jdiv(r[2], d)) in cells]
