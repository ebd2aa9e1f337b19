"""CPU model of the columnar decode (ysb_decode_columns_device): the image, validity and
counts a batch of lines must give, built from oracle/dostats.py (parse_event / parse_tbl /
parse_long) and numpy only -- nothing from the library.

The layout is the fork's WindowedArrowFormatBolter (flink-benchmarks/.../
AdvertisingTopologyNative.java:278-356): seven columns of widths {36,36,36,4,4,8,8}, each
starting on a 4096-byte page (:291-302), then a validity bitmap (bit i % 64 of little-endian
u64 word i / 64).  A row is valid iff the reference would not throw on it: the line parses,
the five String values have at least their column's width in UTF-8 bytes
(put(bytes, 0, entry_len[j]), :325-331) and Long.parseLong(event_time) succeeds.

Also the tagged mutation corpus the GPU tests decode (mutation_corpus)."""
from __future__ import annotations

import json
import struct

import numpy as np

from oracle import dostats

WIDTH = (36, 36, 36, 4, 4, 8, 8)
PAGE = 4096
KEYS = ("user_id", "page_id", "ad_id", "ad_type", "event_type")


def page_align(b):
    return (b + PAGE - 1) // PAGE * PAGE


def layout(rows):
    """{"start": 9 offsets (columns, [7] validity, [8] total), "image_bytes": start[7]}."""
    start, at = [], 0
    for w in WIDTH:
        start.append(at)
        at += page_align(w * rows)
    start.append(at)
    start.append(at + page_align((rows + 63) // 64 * 8))
    return {"rows": rows, "start": start, "width": list(WIDTH), "image_bytes": at}


def decode_line(line: bytes, fmt="json", require_ip=False):
    """([5 value prefixes], event_time) of a valid row, None where the reference throws."""
    try:
        ev = dostats.parse_tbl(line) if fmt == "tbl" else dostats.parse_event(line, require_ip)
        t = dostats.parse_long(ev["event_time"])
    except (dostats.ParseError, ValueError):
        return None
    vals = []
    for k, w in zip(KEYS, WIDTH):
        b = ev[k].encode("utf-8", errors="surrogateescape")
        if len(b) < w:
            return None
        vals.append(b[:w])
    return vals, t


def build(lines, batch_rows=None, fmt="json", require_ip=False, stamp=10, java_order=False, canary=None):
    """(image uint8[start[8]], valid bool[n], {"rows", "valid"}) for lines as rows 0..n-1 of a
    batch of batch_rows rows.  Bytes the decode does not write (page padding, rows >= n, validity
    words >= ceil(n / 64)) hold `canary` (default 0)."""
    n = len(lines)
    rows = max(n, 1) if batch_rows is None else batch_rows
    assert n <= rows
    lay = layout(rows)
    st = lay["start"]
    image = np.full(st[8], 0 if canary is None else canary, dtype=np.uint8)
    valid = np.zeros(n, dtype=np.bool_)
    for j, w in enumerate(WIDTH):
        image[st[j]:st[j] + w * n] = 0
    image[st[7]:st[7] + 8 * ((n + 63) // 64)] = 0
    order = ">q" if java_order else "<q"
    for i, ln in enumerate(lines):
        d = decode_line(ln, fmt, require_ip)
        if d is None:
            continue
        vals, t = d
        valid[i] = True
        for j in range(5):
            image[st[j] + WIDTH[j] * i:st[j] + WIDTH[j] * (i + 1)] = np.frombuffer(vals[j], dtype=np.uint8)
        image[st[5] + 8 * i:st[5] + 8 * i + 8] = np.frombuffer(struct.pack(order, t), dtype=np.uint8)
        image[st[6] + 8 * i:st[6] + 8 * i + 8] = np.frombuffer(struct.pack(order, stamp), dtype=np.uint8)
        image[st[7] + i // 8] |= np.uint8(1 << (i % 8))   # bit i % 64 of little-endian word i / 64
    return image, valid, {"rows": n, "valid": int(valid.sum())}


def pack(lines, shift=0):
    """(bytes, uint32 offsets) of lines packed back to back after `shift` filler bytes."""
    offs, at = [], shift
    for ln in lines:
        offs.append(at)
        at += len(ln)
    return np.frombuffer(b"#" * shift + b"".join(lines), dtype=np.uint8), np.asarray(offs, dtype=np.uint32)


# ---- the mutation corpus ---------------------------------------------------------------------
# Each class rewrites one generator line (core.clj:90-97's layout); its tag says whether the
# reference would decode the result.

def _fields(line):
    return json.loads(line.decode())


def _render(d, sep=(": ", ", "), q='"', raw=None, drop=(), extra=None, tail="\n"):
    raw = raw or {}
    parts = []
    for k, v in d.items():
        if k in drop:
            continue
        parts.append(q + k + q + sep[0] + raw.get(k, q + v + q))
        if extra and extra[0] == k:
            parts.append(extra[1])
    return ("{" + sep[1].join(parts) + "}" + tail).encode()


TWO_BYTE = "é"   # C3 A9

CLASSES = [
    ("as_is", True, lambda ln, d: ln),
    ("u_escape_user_id", True,
     lambda ln, d: _render(d, raw={"user_id": '"\\u%04x%s"' % (ord(d["user_id"][0]), d["user_id"][1:])})),
    ("escaped_slash_ad_type", True,
     lambda ln, d: _render(d, raw={"ad_type": '"%s\\/%s"' % (d["ad_type"][:2], d["ad_type"][2:])})),
    ("compact", True, lambda ln, d: _render(d, sep=(":", ","))),
    ("single_quoted", True, lambda ln, d: _render(d, q="'")),
    ("unquoted_event_type", True, lambda ln, d: _render(d, raw={"event_type": d["event_type"]})),
    ("nested_key_with_brace", True, lambda ln, d: _render(d, extra=("ad_id", '"extra": {"a": "x}y", "b": [1, "]"]}'))),
    ("two_byte_user_id_36", True, lambda ln, d: _render(dict(d, user_id=TWO_BYTE * 17 + "ab"))),
    ("plus_time", True, lambda ln, d: _render(dict(d, event_time="+" + d["event_time"]))),
    ("trailing_bytes", True, lambda ln, d: _render(d, tail=' trailing "}{ bytes\n')),
    ("trailing_cr", True, lambda ln, d: _render(d, tail="\r\n")),
    ("no_ip_address", True, lambda ln, d: _render(d, drop=("ip_address",))),
    ("numeric_event_time", False, lambda ln, d: _render(d, raw={"event_time": d["event_time"]})),
    ("duplicate_key", False, lambda ln, d: _render(d, extra=("ad_type", '"ad_type": "mail"'))),
    ("short_ad_type", False, lambda ln, d: _render(dict(d, ad_type="ab"))),
    ("two_byte_user_id_34", False, lambda ln, d: _render(dict(d, user_id=TWO_BYTE * 17))),
    ("time_overflow", False, lambda ln, d: _render(dict(d, event_time="9999999" + d["event_time"]))),
    ("null_user_id", False, lambda ln, d: _render(d, raw={"user_id": "null"})),
]
NEEDS_IP = {"no_ip_address"}   # valid classes that turn invalid under require_ip


def mutation_corpus(lines):
    """[(line, class name, tagged valid)]: class i % 18 applied to generator line i."""
    out = []
    for i, ln in enumerate(lines):
        name, ok, fn = CLASSES[i % len(CLASSES)]
        out.append((fn(ln, _fields(ln)), name, ok))
    return out
