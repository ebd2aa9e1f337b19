"""CPU model of the joined-views call (ysb_join_device): the ordered stream of joined views a
batch must give -- RedisJoinBolt.flatMap's Tuple3 stream (flink-benchmarks/.../
AdvertisingTopologyNative.java:460-474) -- and the stats it must report.

Everything comes from the existing oracle (oracle/ysb_oracle.c) run one line at a time with
divisor = 1: a line's single bucket is then its event_time, its campaign is the row's, and the
line's stats say whether it joined and whether its time parsed.  The reference parses the time
only after the join (CampaignProcessorCommon.java:58), so a joined view with a bad time is still
a row (time_ok 0, event_time 0); the oracle gives no bucket for it, and its campaign is found by
asking the oracle again with one campaign's ads at a time.  Nothing from the library."""
from __future__ import annotations

import numpy as np

from oracle import oracle

STATS = ("events", "views", "joined", "join_misses", "parse_errors", "time_errors")


def lines_of(raw, offs):
    raw = bytes(raw) if not isinstance(raw, (bytes, bytearray)) else raw
    offs = [int(o) for o in offs]
    return [raw[a:b] for a, b in zip(offs, offs[1:] + [len(raw)])]


class Model:
    def __init__(self, ads, camp):
        self.ads, self.camp = list(ads), [int(c) for c in camp]
        self.map = oracle.AdMap(self.ads, self.camp)
        self._by_campaign = {}

    def _campaign_map(self, c):
        if c not in self._by_campaign:
            self._by_campaign[c] = oracle.AdMap([a for a, k in zip(self.ads, self.camp) if k == c], [c] * self.camp.count(c))
        return self._by_campaign[c]

    def line(self, ln, fmt="json", require_ip=False):
        """(row or None, stats): row = (campaign, event_time, time_ok)."""
        rows, st = oracle.run(self.map, ln, [0], divisor=1, require_ip=require_ip, fmt=fmt)
        assert st["events"] == 1
        if not st["joined"]:
            assert not rows
            return None, st
        if not st["time_errors"]:
            ((c, t), k), = rows.items()
            assert k == 1
            return (c, t, 1), st
        assert not rows
        found = [c for c in sorted(set(self.camp))
                 if oracle.run(self._campaign_map(c), ln, [0], divisor=1, require_ip=require_ip, fmt=fmt)[1]["joined"]]
        assert len(found) == 1
        return (found[0], 0, 0), st

    def batch(self, raw, offs, fmt="json", require_ip=False):
        """({"campaign", "row", "event_time", "time_ok"} numpy columns in stream order, stats)."""
        tot = dict.fromkeys(STATS, 0)
        out = []
        for i, ln in enumerate(lines_of(raw, offs)):
            row, st = self.line(ln, fmt, require_ip)
            for k in STATS:
                tot[k] += st[k]
            if row is not None:
                out.append((row[0], i, row[1], row[2]))
        cols = {"campaign": np.array([r[0] for r in out], dtype=np.uint32),
                "row": np.array([r[1] for r in out], dtype=np.uint32),
                "event_time": np.array([r[2] for r in out], dtype=np.int64),
                "time_ok": np.array([r[3] for r in out], dtype=np.uint8)}
        return cols, tot


def histogram(cols, divisor=10000):
    """{(campaign, bucket): count} over the time_ok rows, bucket = event_time / divisor in Java
    long division: what the counting path's drain_buckets() gives for the same batch."""
    ok = cols["time_ok"] != 0
    camp, t = cols["campaign"][ok], cols["event_time"][ok]
    if len(t) > 100_000:   # generated batches: times are positive
        assert (t >= 0).all()
        key = camp.astype(np.int64) * (1 << 40) + t // divisor
        ks, ns = np.unique(key, return_counts=True)
        return {(int(k >> 40), int(k & ((1 << 40) - 1))): int(n) for k, n in zip(ks, ns)}
    out = {}
    for c, x in zip(camp, t):
        x = int(x)
        b = abs(x) // divisor * (1 if x >= 0 else -1)
        out[(int(c), b)] = out.get((int(c), b), 0) + 1
    return out
