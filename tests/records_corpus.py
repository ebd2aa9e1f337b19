"""Lines for the record-mode tests, written by the test so that every cell's count is known by
construction: generator lines as carriers (their user_id, page_id and ad_type kept), with the
ad_id, event_type and event_time substituted -- the generator's layout byte for byte, so the
scan's first tier takes every line.  Pure numpy over the generator's host side: no GPU.

A corpus is described per line by (ad index, event type, event time); the expected table is the
Counter of (campaign of the ad, time / divisor) over the views of ads in the map."""
from __future__ import annotations

import json
from collections import Counter

import numpy as np

DIVISOR = 10_000                     # ysb_config_default's time_divisor_ms
BUCKET_1E12 = 170_000_000            # the bucket of t = 1.7e12 ms: 13-digit positive times
EVENT_TYPES = ("view", "click", "purchase")
VIEW, CLICK, PURCHASE = 0, 1, 2


def time_in_bucket(bucket, k=0):
    """An event time (ms) whose Java quotient by DIVISOR is `bucket`: the k-th of its DIVISOR
    (2 * DIVISOR - 1 for bucket 0) times, counted away from zero."""
    bucket = np.asarray(bucket, dtype=np.int64)
    k = np.asarray(k, dtype=np.int64) % DIVISOR
    return np.where(bucket < 0, bucket * DIVISOR - k, bucket * DIVISOR + k)


def bucket_of_time(t):
    t = np.asarray(t, dtype=np.int64)
    return np.where(t < 0, -((-t) // DIVISOR), t // DIVISOR)


class LineWriter:
    """Renders lines from carriers: one generator line per ad_type (five line lengths)."""

    def __init__(self, gen, ads_packed):
        self.ads = np.ascontiguousarray(ads_packed, dtype=np.uint8).reshape(-1, 36)
        raw, offs = gen.events_host(0, 256)
        ends = list(offs[1:]) + [raw.size]
        seen = {}
        for a, b in zip(offs.tolist(), ends):
            ev = json.loads(bytes(raw[a:b]))
            seen.setdefault(ev["ad_type"], ev)
        assert len(seen) == 5, "the first 256 generator lines hold every ad_type"
        self.tpl, self.t_off = [], []
        for ev in seen.values():                       # carrier j
            for et in EVENT_TYPES:                     # kind = 3 * j + event type
                head = '{"user_id": "%s", "page_id": "%s", "ad_id": "' % (ev["user_id"], ev["page_id"])
                assert len(head) == 113
                mid = '", "ad_type": "%s", "event_type": "%s", "event_time": "' % (ev["ad_type"], et)
                line = head + "x" * 36 + mid + "0" * 13 + '", "ip_address": "1.2.3.4"}\n'
                self.tpl.append(np.frombuffer(line.encode(), dtype=np.uint8))
                self.t_off.append(len(head) + 36 + len(mid))
        self.n_carriers = len(seen)

    @staticmethod
    def time_bytes(t):
        """13 bytes per time: thirteen digits, or '-' and twelve (zero padded: parseLong reads both)."""
        t = np.asarray(t, dtype=np.int64)
        mag = np.abs(t)
        assert (mag[t >= 0] < 10 ** 13).all() and (mag[t < 0] < 10 ** 12).all()
        out = np.empty((t.size, 13), dtype=np.uint8)
        for j in range(13):
            out[:, 12 - j] = 48 + mag % 10
            mag = mag // 10
        out[t < 0, 0] = ord("-")
        return out

    def render(self, ad, etype, t, carrier=None):
        """(raw uint8 bytes, uint32 line offsets) of the lines (ad index, event type, time);
        carrier: per line 0..4 (default: line index mod 5)."""
        ad, etype, t = (np.asarray(x, dtype=np.int64) for x in (ad, etype, t))
        n = ad.size
        carrier = np.arange(n, dtype=np.int64) % self.n_carriers if carrier is None else np.asarray(carrier, dtype=np.int64)
        kind = 3 * carrier + etype
        width = np.array([x.size for x in self.tpl], dtype=np.int64)[kind]
        offs = np.concatenate([[0], np.cumsum(width)[:-1]]).astype(np.int64)
        out = np.empty(int(width.sum()), dtype=np.uint8)
        tb = self.time_bytes(t)
        for k in np.unique(kind).tolist():
            rows = np.flatnonzero(kind == k)
            w = self.tpl[k].size
            for lo in range(0, rows.size, 32768):
                r = rows[lo:lo + 32768]
                block = np.tile(self.tpl[k], (r.size, 1))
                block[:, 113:149] = self.ads[ad[r]]
                block[:, self.t_off[k]:self.t_off[k] + 13] = tb[r]
                if r.size and r[-1] - r[0] + 1 == r.size and (kind[r[0]:r[-1] + 1] == k).all():
                    out[offs[r[0]]:offs[r[0]] + r.size * w] = block.reshape(-1)   # a contiguous run of one kind
                else:
                    out[offs[r][:, None] + np.arange(w)] = block
        assert offs.size == 0 or offs[-1] < 1 << 32
        return out, offs.astype(np.uint32)


class Corpus:
    """Lines described per line, with what they must count to."""

    def __init__(self, ad, etype, t, camp_of_ad, n_map):
        self.ad, self.etype, self.t = (np.asarray(x, dtype=np.int64) for x in (ad, etype, t))
        self.camp_of_ad = np.asarray(camp_of_ad, dtype=np.int64)
        self.n_map = n_map                              # ads [0, n_map) are in the map, the rest miss
        self.bucket = bucket_of_time(self.t)
        view, known = self.etype == VIEW, self.ad < n_map
        self.camp = np.where(view & known, self.camp_of_ad[np.minimum(self.ad, self.camp_of_ad.size - 1)], -1)

    def __len__(self):
        return self.ad.size

    def part(self, lo, hi):
        return Corpus(self.ad[lo:hi], self.etype[lo:hi], self.t[lo:hi], self.camp_of_ad, self.n_map)

    def expected(self):
        """The plain Counter of (campaign, bucket) over the joined views."""
        j = self.camp >= 0
        return dict(Counter(zip(self.camp[j].tolist(), self.bucket[j].tolist())))

    def stats(self):
        view, known = self.etype == VIEW, self.ad < self.n_map
        return {"events": len(self), "views": int(view.sum()), "joined": int((view & known).sum()),
                "join_misses": int((view & ~known).sum()), "parse_errors": 0, "time_errors": 0}

    def oracle_map(self, ads_str):
        """(ad ids, campaigns) of the map's ads these lines name: the oracle's map (equal to the
        whole map on every key in the bytes)."""
        used = np.unique(self.ad[self.ad < self.n_map])
        return [ads_str(i) for i in used.tolist()], self.camp_of_ad[used].tolist()


def geometry_corpus(rng, n_lines, n_campaigns, n_ads, n_map, base, W, camp_of_ad):
    """About n_lines lines for a geometry test: views spread over all campaigns (the first and
    the last campaign of the table among them) and 12 buckets from the ring's base, a tenth
    non-views, a few join misses (ads [n_map, n_ads)) and a few views on either side of the ring."""
    ad = rng.integers(0, n_map, n_lines)
    by_camp = {}
    for c in (0, n_campaigns - 1, n_campaigns // 2):
        hit = np.flatnonzero(camp_of_ad[:n_map] == c)
        assert hit.size, "campaign %d has no ad" % c
        by_camp[c] = hit[0]
    ad[:24] = np.repeat(list(by_camp.values()), 8)
    etype = np.where(rng.random(n_lines) < 0.1, rng.integers(1, 3, n_lines), VIEW)
    etype[:24] = VIEW
    bucket = base + rng.integers(0, 12, n_lines)
    out = rng.choice(n_lines - 24, 40, replace=False) + 24
    bucket[out[:20]] = base - 1 - rng.integers(0, 3, 20)
    bucket[out[20:]] = base + W + rng.integers(0, 3, 20)
    miss = rng.choice(n_lines - 24, 16, replace=False) + 24
    ad[miss] = rng.integers(n_map, n_ads, 16)
    t = time_in_bucket(bucket, rng.integers(0, DIVISOR, n_lines))
    return Corpus(ad, etype, t, camp_of_ad, n_map)
