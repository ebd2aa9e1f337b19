"""CPU model of parked views (ysb_parked_enable / _keys / _resolve): the stats and the
(campaign, bucket) counts that park-then-resolve must give, as plain dicts and lists, from the
lines alone -- oracle/dostats.py's parser, Long.parseLong and division, nothing from the
library but the shard classifier (the ysb_ad_shard binding), which is the partitioning's
definition.

Per line, as oracle/dostats.run: events, parse_errors, the view filter, views.  Then, for a view:
  1. ad_id in the map -> joined, then time_errors or counts[(campaign, bucket)] += 1.
  2. Otherwise the final miss verdict.  With parking on, an ad_id of at most 56 bytes (UTF-8)
     that is, on a sharded model, of this rank's shard is appended to the log as (key bytes,
     whether Long.parseLong(event_time) succeeded, the value): nothing else moves.  A full log
     makes it a join miss and dropped += 1.  A foreign key is foreign_shard, any other view a
     join miss -- as with parking off.
resolve() walks the log against the map as it is then (the caller has put what its lookup
found): found -> joined, then time_errors or a count; not found -> join_misses.  The log is
then empty.  At every moment views == joined + join_misses + foreign_shard + len(log)."""
from __future__ import annotations

from oracle import dostats

STATS = ("events", "views", "joined", "join_misses", "parse_errors", "time_errors", "foreign_shard")
MAX_KEY_BYTES = 56


def key_bytes(ad_id):
    return ad_id if isinstance(ad_id, bytes) else ad_id.encode("utf-8", errors="surrogateescape")


class ParkedModel:
    def __init__(self, ad_map, capacity, divisor=10000, shard=None, fmt="json"):
        """ad_map: {ad id (str or bytes): campaign}; capacity 0: parking off."""
        self.map = {key_bytes(k): v for k, v in ad_map.items()}
        self.capacity, self.divisor, self.shard, self.fmt = capacity, divisor, shard, fmt
        self.stats = dict.fromkeys(STATS, 0)
        self.counts = {}
        self.log = []            # (key bytes, time ok, time)
        self.parked_total = self.dropped = 0
        self.last = dict(resolved_joined=0, resolved_missed=0, resolved_time_errors=0)

    def put(self, ad_ids, campaigns):
        """ysb_ad_map_upsert: HashMap.put in order."""
        self.map.update(zip(map(key_bytes, ad_ids), campaigns))

    def _count(self, campaign, ok, t):
        s = self.stats
        s["joined"] += 1
        if not ok:
            s["time_errors"] += 1
            return
        cell = (campaign, dostats.java_div(t, self.divisor))
        self.counts[cell] = self.counts.get(cell, 0) + 1

    @staticmethod
    def _time(text):
        try:
            return True, dostats.parse_long(text)
        except ValueError:
            return False, 0

    def submit(self, lines):
        s = self.stats
        for line in lines:
            s["events"] += 1
            try:
                ev = dostats.parse_tbl(line) if self.fmt == "tbl" else dostats.parse_event(line)
            except dostats.ParseError:
                s["parse_errors"] += 1
                continue
            if ev["event_type"] != "view":
                continue
            s["views"] += 1
            key = key_bytes(ev["ad_id"])
            campaign = self.map.get(key)
            if campaign is not None:
                self._count(campaign, *self._time(ev["event_time"]))
                continue
            keyed = len(key) <= MAX_KEY_BYTES
            if keyed and self.shard is not None and self.shard[1] > 1:
                from ysb_amd import ad_shard
                if ad_shard(key, self.shard[1]) != self.shard[0]:
                    s["foreign_shard"] += 1
                    continue
            if not keyed or not self.capacity:
                s["join_misses"] += 1
            elif len(self.log) >= self.capacity:
                s["join_misses"] += 1
                self.dropped += 1
            else:
                self.log.append((key,) + self._time(ev["event_time"]))
                self.parked_total += 1

    def keys(self):
        """ysb_parked_keys, as a set."""
        return {k for k, _, _ in self.log}

    def resolve(self):
        before = dict(self.stats)
        for key, ok, t in self.log:
            campaign = self.map.get(key)
            if campaign is None:
                self.stats["join_misses"] += 1
            else:
                self._count(campaign, ok, t)
        self.log = []
        self.last = dict(resolved_joined=self.stats["joined"] - before["joined"],
                         resolved_missed=self.stats["join_misses"] - before["join_misses"],
                         resolved_time_errors=self.stats["time_errors"] - before["time_errors"])
        return self.last

    def info(self):
        return dict(capacity=self.capacity, parked=len(self.log), parked_total=self.parked_total,
                    dropped=self.dropped, **self.last)


def lines_of(raw, offs):
    """The batch's lines as bytes (each with its terminator)."""
    data = bytes(raw)
    ends = list(offs[1:]) + [len(data)]
    return [data[int(a):int(b)] for a, b in zip(offs, ends)]
