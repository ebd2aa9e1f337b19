"""CPU model of the columnar count (ysb_submit_columns / ysb_submit_columns_device): the
(campaign, bucket) counts and the stats a column batch must give, from its bytes alone, with
numpy and oracle/dostats.py's java_div -- nothing from the library but the shard classifier
(the ysb_ad_shard binding), which is the partitioning's definition.

A batch is a buffer in the layout columns_model.layout(batch_rows); rows [0, n_rows) count.
Per row, in order:
  1. events += 1.
  2. With validity (the bitmap at start[7]: bit i % 64 of little-endian u64 word i / 64) a row
     whose bit is zero adds 1 to parse_errors and nothing else.
  3. The row is a view iff the four bytes of column 4 equal b"view" (the layout cut event_type
     to four bytes: "viewer" is a view here); views += 1.
  4. The key is the 36 bytes of column 2; a key outside the map is a join miss, or with
     shard = (rank, nranks) a foreign_shard when the key belongs to another rank; a hit adds 1
     to joined.
  5. event_time is column 5 as an int64, little-endian or (java_order) big-endian;
     bucket = java_div(t, divisor).
  6. counts[(campaign, bucket)] += 1.
time_errors and deferred never change."""
from __future__ import annotations

import numpy as np

import columns_model as cm
from oracle import dostats

STATS = ("events", "views", "joined", "join_misses", "parse_errors", "time_errors", "deferred", "foreign_shard")


def read_ranges(batch_rows, n_rows, validity=False):
    """[(offset, bytes)]: the only bytes of a batch the count may read."""
    st = cm.layout(batch_rows)["start"]
    out = [(st[2], 36 * n_rows), (st[4], 4 * n_rows), (st[5], 8 * n_rows)]
    if validity:
        out.append((st[7], 8 * ((n_rows + 63) // 64)))
    return out


def count(image, batch_rows, n_rows, ad_map, divisor=10000, java_order=False, validity=False, shard=None):
    """({(campaign, bucket): count}, stats) of rows [0, n_rows) of image; ad_map: bytes -> campaign."""
    assert 0 <= n_rows <= batch_rows
    image = np.ascontiguousarray(image, dtype=np.uint8)
    st = cm.layout(batch_rows)["start"]
    ad = image[st[2]:st[2] + 36 * n_rows].reshape(n_rows, 36)
    et = image[st[4]:st[4] + 4 * n_rows].reshape(n_rows, 4)
    tm = image[st[5]:st[5] + 8 * n_rows].view(">i8" if java_order else "<i8")
    bits = None
    if validity:
        words = image[st[7]:st[7] + 8 * ((n_rows + 63) // 64)].view("<u8")
        bits = [(int(words[i // 64]) >> (i % 64)) & 1 for i in range(n_rows)]
    s = dict.fromkeys(STATS, 0)
    cells = {}
    for i in range(n_rows):
        s["events"] += 1
        if bits is not None and not bits[i]:
            s["parse_errors"] += 1
            continue
        if et[i].tobytes() != b"view":
            continue
        s["views"] += 1
        key = ad[i].tobytes()
        c = ad_map.get(key)
        if c is None:
            if shard is not None and shard[1] > 1:
                from ysb_amd import ad_shard
                if ad_shard(key, shard[1]) != shard[0]:
                    s["foreign_shard"] += 1
                    continue
            s["join_misses"] += 1
            continue
        s["joined"] += 1
        b = dostats.java_div(int(tm[i]), divisor)
        cells[(c, b)] = cells.get((c, b), 0) + 1
    return cells, s


def make_image(ads, types, times, batch_rows, java_order=False, valid=None, canary=0xA5):
    """An image over `canary` bytes: row i holds ads[i] (36 bytes), types[i] (4 bytes) and
    times[i] in columns 2, 4 and 5 -- the other four columns and the padding keep the canary --
    and, with valid (bools), the validity words of the rows given (the rest of the bitmap
    keeps the canary too)."""
    n = len(ads)
    assert n == len(types) == len(times) <= batch_rows
    lay = cm.layout(batch_rows)
    st = lay["start"]
    image = np.full(st[8], canary, dtype=np.uint8)
    if n:
        image[st[2]:st[2] + 36 * n] = np.frombuffer(b"".join(ads), dtype=np.uint8)
        image[st[4]:st[4] + 4 * n] = np.frombuffer(b"".join(types), dtype=np.uint8)
        image[st[5]:st[5] + 8 * n] = np.asarray(times, dtype=">i8" if java_order else "<i8").view(np.uint8)
    if valid is not None:
        words = np.zeros((n + 63) // 64, dtype="<u8")
        for i, v in enumerate(valid):
            if v:
                words[i // 64] |= np.uint64(1 << (i % 64))
        image[st[7]:st[7] + 8 * words.size] = words.view(np.uint8)
    return image


def fill_past(image, batch_rows, n_rows, ad, time, java_order=False, validity=False):
    """Rows [n_rows, batch_rows) of EVERY column, and (validity) the bitmap's bits >= n_rows up
    to the last word of the batch, become countable views of `ad` at `time`: a kernel that
    reads past n_rows shows as extra counts."""
    st = cm.layout(batch_rows)["start"]
    k = batch_rows - n_rows
    if k:
        for j in (0, 1, 2):
            image[st[j] + 36 * n_rows:st[j] + 36 * batch_rows] = np.frombuffer(ad * k, dtype=np.uint8)
        for j in (3, 4):
            image[st[j] + 4 * n_rows:st[j] + 4 * batch_rows] = np.frombuffer(b"view" * k, dtype=np.uint8)
        t8 = np.asarray([time] * k, dtype=">i8" if java_order else "<i8").view(np.uint8)
        for j in (5, 6):
            image[st[j] + 8 * n_rows:st[j] + 8 * batch_rows] = t8
    if validity:
        nw = (batch_rows + 63) // 64
        words = image[st[7]:st[7] + 8 * nw].view("<u8")
        for w in range(n_rows // 64, nw):
            keep = (1 << (n_rows - 64 * w)) - 1 if 64 * w < n_rows else 0
            words[w] = np.uint64((int(words[w]) & keep) | (~keep & ((1 << 64) - 1)))
    return image
