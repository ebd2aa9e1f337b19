"""CPU model of the Arrow count (ysb_submit_arrow / ysb_submit_arrow_device): the (campaign,
bucket) counts and the stats an Arrow batch must give, from its buffers alone, with numpy and
oracle/dostats.py's parse_long and java_div -- nothing from the library but the shard classifier
(the ysb_ad_shard binding), which is the partitioning's definition.

A batch (Batch) is three columns (Col) of n_rows rows over numpy buffers.  Row i is element
`offset + i` of a column's offsets / values and bit `validity_offset + i` of its bitmap (bit k =
bit k % 8 of byte k / 8; no bitmap: all valid).  Per row, in order:
  1. events += 1.
  2. The row is invalid -- parse_errors += 1 and nothing else -- when, in this order: the
     struct's bit or a column's bit is zero (null); a dictionary index is outside [0, dict_len)
     (dict); the dictionary value it names is null (null); a string value's offsets break
     data_first <= off[k] <= off[k+1] <= data_bytes (offsets).
  3. The row is a view iff its event_type value is exactly b"view"; views += 1.
  4. The key is the ad_id value's bytes; above 56 bytes or outside the map it is a join miss, or
     with shard = (rank, nranks) and at most 56 bytes a foreign_shard when another rank owns it.
  5. joined += 1; an int64 time is taken as it is, a string time is parse_long's; a rejected
     time adds 1 to time_errors and counts nothing.
  6. counts[(campaign, java_div(time, divisor))] += 1.
deferred never changes."""
from __future__ import annotations

import numpy as np

from oracle import dostats

STRING, INT64, DICT = 1, 2, 3
STATS = ("events", "views", "joined", "join_misses", "parse_errors", "time_errors", "deferred", "foreign_shard")


class Col:
    """kind STRING: offsets (int32), data (uint8: the bytes from data_first on), data_bytes (the
    stated end; default: all of data).  INT64 / DICT: data holds the int64 values / int32 indices."""

    def __init__(self, kind, offsets=None, data=None, validity=None, offset=0, validity_offset=None, data_first=0,
                 data_bytes=None):
        self.kind = kind
        self.offsets = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.int32)
        dt = {STRING: np.uint8, INT64: np.int64, DICT: np.int32}[kind]
        self.data = np.ascontiguousarray(data if data is not None else [], dtype=dt)
        self.validity = None if validity is None else np.ascontiguousarray(validity, dtype=np.uint8)
        self.offset = offset
        self.validity_offset = offset if validity_offset is None else validity_offset
        self.data_first = data_first
        self.data_bytes = (data_first + self.data.size if kind == STRING else self.data.nbytes) if data_bytes is None else data_bytes


class Batch:
    def __init__(self, n_rows, ad, typ, time, dictionary=None, dict_len=0, validity=None, offset=0):
        self.n_rows, self.ad, self.typ, self.time = n_rows, ad, typ, time
        self.dict, self.dict_len = dictionary, dict_len
        self.validity = None if validity is None else np.ascontiguousarray(validity, dtype=np.uint8)
        self.offset = offset


def strings(values, validity=None, **kw):
    """A STRING Col of bytes values (validity: bools per element, or None)."""
    offs = np.zeros(len(values) + 1, dtype=np.int32)
    offs[1:] = np.cumsum([len(v) for v in values])
    return Col(STRING, offs, np.frombuffer(b"".join(values), dtype=np.uint8).copy(), bitmap(validity), **kw)


def bitmap(valid, lead=0, fill=False):
    """bools -> a bitmap whose bit `lead` is valid[0] (the `lead` bits in front and the bits behind
    hold `fill`); None -> None."""
    if valid is None:
        return None
    bits = [fill] * lead + [bool(v) for v in valid]
    bits += [fill] * (-len(bits) % 8)
    return np.packbits(np.asarray(bits, dtype=np.bool_), bitorder="little")


def _bit(bm, k):
    return True if bm is None else bool((int(bm[k >> 3]) >> (k & 7)) & 1)


def _value(c, elem):
    o0, o1 = int(c.offsets[elem]), int(c.offsets[elem + 1])
    if not c.data_first <= o0 <= o1 <= c.data_bytes:
        return None
    return c.data[o0 - c.data_first:o1 - c.data_first].tobytes()


def row(b, i):
    """("null" | "dict" | "offsets", None) for an invalid row, else (None, (ad, type, time)):
    bytes values, the time an int for an int64 column."""
    if not _bit(b.validity, b.offset + i):
        return "null", None
    for c in (b.ad, b.typ, b.time):
        if not _bit(c.validity, c.validity_offset + i):
            return "null", None
    ty, ty_elem = b.typ, b.typ.offset + i
    if ty.kind == DICT:
        idx = int(ty.data[ty_elem])
        if not 0 <= idx < b.dict_len:
            return "dict", None
        if not _bit(b.dict.validity, b.dict.validity_offset + idx):
            return "null", None
        ty, ty_elem = b.dict, b.dict.offset + idx
    ad = _value(b.ad, b.ad.offset + i)
    et = _value(ty, ty_elem)
    tm = int(b.time.data[b.time.offset + i]) if b.time.kind == INT64 else _value(b.time, b.time.offset + i)
    if ad is None or et is None or tm is None:
        return "offsets", None
    return None, (ad, et, tm)


def count(b, ad_map, divisor=10000, shard=None, invalid=None):
    """({(campaign, bucket): count}, stats); ad_map: bytes -> campaign.  invalid: a dict that
    receives the invalid rows by cause."""
    s = dict.fromkeys(STATS, 0)
    why_n = {"null": 0, "offsets": 0, "dict": 0}
    cells = {}
    for i in range(b.n_rows):
        s["events"] += 1
        why, v = row(b, i)
        if why:
            s["parse_errors"] += 1
            why_n[why] += 1
            continue
        ad, et, tm = v
        if et != b"view":
            continue
        s["views"] += 1
        c = ad_map.get(ad) if len(ad) <= 56 else None
        if c is None:
            if shard is not None and shard[1] > 1 and len(ad) <= 56:
                from ysb_amd import ad_shard
                if ad_shard(ad, shard[1]) != shard[0]:
                    s["foreign_shard"] += 1
                    continue
            s["join_misses"] += 1
            continue
        s["joined"] += 1
        if not isinstance(tm, int):
            try:
                tm = dostats.parse_long(tm.decode("latin-1"))
            except ValueError:
                s["time_errors"] += 1
                continue
        k = (c, dostats.java_div(tm, divisor))
        cells[k] = cells.get(k, 0) + 1
    if invalid is not None:
        invalid.update(why_n)
    return cells, s


# ---- the same batch for the library ----------------------------------------------------------

def to_cols(b, put=lambda a: a):
    """The batch as a ysb_arrow_cols.  put(array) -> what the struct should point at: the array
    itself (host), or a device address of its uploaded copy."""
    from ysb_amd import arrow

    def col(c):
        if c is None:
            return None
        return arrow.col(c.kind, offsets=None if c.offsets is None else put(c.offsets),
                         data=put(c.data) if c.data.size else None,
                         validity=None if c.validity is None else put(c.validity), data_bytes=c.data_bytes,
                         offset=c.offset, validity_offset=c.validity_offset, data_first=c.data_first)
    return arrow.cols(b.n_rows, col(b.ad), col(b.typ), col(b.time), col(b.dict), b.dict_len,
                      None if b.validity is None else put(b.validity), b.offset)


def to_node(b, names=("ad_id", "event_type", "event_time"), extra=True):
    """The batch as the package's own ArrowArray / ArrowSchema pair (the host form's input).  Needs
    what the C data interface can say: one offset per column (validity_offset == offset), whole
    data buffers (data_first 0).  extra: a fourth column the library must ignore."""
    from ysb_amd import arrow

    bo, n = b.offset, b.offset + b.n_rows   # a child: its own offset on top of the struct's, at least bo + n_rows long

    def node(c):
        assert c.validity_offset == c.offset >= bo and c.data_first == 0
        if c.kind == STRING:
            return arrow.string_array(c.offsets, c.data, c.validity, c.offset - bo, n)
        if c.kind == INT64:
            return arrow.int64_array(c.data, c.validity, c.offset - bo, n)
        d = b.dict
        assert d.validity_offset == d.offset and d.data_first == 0
        return arrow.dict_array(c.data, arrow.string_array(d.offsets, d.data, d.validity, d.offset, b.dict_len),
                                c.validity, c.offset - bo, n)
    kids = {}
    if extra:
        kids["user_id"] = arrow.strings([b"x"] * n)
    for nm, c in zip(names, (b.ad, b.typ, b.time)):
        kids[nm] = node(c)
    return arrow.batch(kids, validity=b.validity, offset=bo, length=b.n_rows)


def render_json(b):
    """(lines, n_formless): each row that has a JSON form as the line
    {"user_id":"x","page_id":"x","ad_id":V,"ad_type":"x","event_type":V,"event_time":V} -- a null
    is rendered as null, an int64 time as its decimal string.  Rows invalid by offsets or by
    dictionary index have no JSON form and are left out."""
    lines, formless = [], 0
    for i in range(b.n_rows):
        why, v = row(b, i)
        if why in ("offsets", "dict"):
            formless += 1
            continue
        if why == "null":
            vals = [b"null"] * 3
            # render what is not null, so that the line is what a producer would have written
            svalid = _bit(b.validity, b.offset + i)
            if svalid:
                vals = []
                for c in (b.ad, b.typ, b.time):
                    if not _bit(c.validity, c.validity_offset + i):
                        vals.append(b"null")
                    else:
                        vals.append(b'"x"')
                if vals.count(b"null") == 0:   # the dictionary's value is the null
                    vals[1] = b"null"
        else:
            ad, et, tm = v
            tmb = str(tm).encode() if isinstance(tm, int) else tm
            vals = [b'"' + x + b'"' for x in (ad, et, tmb)]
        lines.append(b'{"user_id":"x","page_id":"x","ad_id":' + vals[0] + b',"ad_type":"x","event_type":' + vals[1] +
                     b',"event_time":' + vals[2] + b'}\n')
    return lines, formless


# ---- rows in the three encodings -------------------------------------------------------------

def encode(rows, kind, lead=0, tail=0, filler=None, bitmaps=False):
    """rows [(ad, type, time)] as a Batch in one of the three encodings ("strings", "int64",
    "dict"), with `lead` / `tail` filler elements around them in every buffer (the batch's rows
    start at element `lead`); bitmaps: all-ones validity at every level."""
    allr = [filler] * lead + list(rows) + [filler] * tail
    n = len(allr)
    ones = bitmap([True] * n) if bitmaps else None
    ad = strings([r[0] for r in allr])
    ad.validity, ad.offset, ad.validity_offset = ones, lead, lead
    d, dl = None, 0
    if kind == "dict":
        vals = sorted({r[1] for r in allr})
        ty = Col(DICT, data=[vals.index(r[1]) for r in allr], validity=ones, offset=lead)
        d, dl = strings(vals), len(vals)
    else:
        ty = strings([r[1] for r in allr])
        ty.validity, ty.offset, ty.validity_offset = ones, lead, lead
    if kind == "int64":
        tm = Col(INT64, data=[int(r[2]) for r in allr], validity=ones, offset=lead)
    else:
        tm = strings([r[2] for r in allr])
        tm.validity, tm.offset, tm.validity_offset = ones, lead, lead
    return Batch(len(rows), ad, ty, tm, d, dl, validity=ones, offset=lead if bitmaps else 0)


# ---- the committed pyarrow buffers (tests/golden/arrow/make_arrow_golden.py) -------------------

FIXTURES = ("gen_s7_strings", "gen_s7_int64", "gen_s7_dict", "gen_s7_slice67", "nulls")


def fixture(name):
    """tests/golden/arrow/<name>.npz as a Batch, read with numpy alone."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "arrow", name + ".npz"))

    def col(p):
        off = int(z[p + "offset"])
        val = z[p + "validity"] if p + "validity" in z else None
        if p + "offsets" in z:
            data = z[p + "data"] if p + "data" in z else np.zeros(0, dtype=np.uint8)
            return Col(STRING, z[p + "offsets"].view(np.int32), data, val, offset=off)
        if p + "dict_length" in z:
            return Col(DICT, data=z[p + "values"].view(np.int32), validity=val, offset=off)
        return Col(INT64, data=z[p + "values"].view(np.int64), validity=val, offset=off)
    ty = col("event_type_")
    d = col("event_type_dict_") if ty.kind == DICT else None
    return Batch(int(z["n_rows"]), col("ad_id_"), ty, col("event_time_"), d,
                 int(z["event_type_dict_length"]) if d else 0)


# ---- the hand-made corpus ---------------------------------------------------------------------

I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)
TIMES = [b"+1", b"-0", b"9223372036854775807", b"9223372036854775808", b"-9223372036854775808",
         b"-9223372036854775809", b"09223372036854775807", b"19223372036854775807", b"0" * 25 + b"123456",
         b"", b" ", b"12a4", b"1500000000000"]
TYPES = [b"view", b"viewer", b"vie", b"View", b""]


def corpus_map():
    """Keys of 0, 35, 36, 37 and 56 bytes (and the 57- and 200-byte ones no table can hold)."""
    return {b"": 0, b"a" * 35: 1, b"b" * 36: 2, b"c" * 37: 3, b"d" * 56: 4}


def corpus_rows():
    """[(ad, type, time)]: every ad length x a view at a good time, every type, every time on a
    known ad -- 7 + 5 + 13 rows, then views that miss."""
    ads = [b"", b"a" * 35, b"b" * 36, b"c" * 37, b"d" * 56, b"e" * 57, b"f" * 200]
    rows = [(a, b"view", b"1500000012345") for a in ads]
    rows += [(b"b" * 36, t, b"1500000012345") for t in TYPES]
    rows += [(b"b" * 36, b"view", t) for t in TIMES]
    rows += [(b"z" * 36, b"view", b"1"), (b"z" * 7, b"view", b"x"), (b"b" * 36, b"click", b"1")]
    return rows


def corpus():
    """{name: Batch}: the hand-made cases of the CPU and the GPU tests."""
    rows = corpus_rows()
    n = len(rows)
    ads, tys, tms = ([r[k] for r in rows] for k in range(3))
    out = {}
    out["plain"] = Batch(n, strings(ads), strings(tys), strings(tms))
    # int64 times: every row a view of a known ad, the times around zero and at the bounds
    it = [0, 1, -1, 9999, 10000, -9999, -10000, I64_MAX, I64_MIN, 1500000012345]
    out["int64"] = Batch(len(it), strings([b"b" * 36] * len(it)), strings([b"view"] * len(it)), Col(INT64, data=it))
    # nulls in each column and at struct level; every bitmap's first bit is bit 3 of a byte
    k = 12
    valid = {c: [(i % 5) != j for i in range(k)] for j, c in enumerate("satm")}
    def col3(values, v):
        c = strings([b"q"] * 3 + values)   # three elements in front of the rows
        c.offset = 3
        c.validity = bitmap(v, lead=3, fill=True)
        c.validity_offset = 3
        return c
    out["nulls"] = Batch(k, col3([b"b" * 36] * k, valid["a"]), col3([b"view"] * k, valid["t"]),
                         col3([b"1500000012345"] * k, valid["m"]), validity=bitmap(valid["s"], lead=3, fill=True), offset=3)
    # a dictionary: duplicate `view` entries, a null value, indices -1 and dict_len
    dvals = [b"view", b"click", b"view", b"purchase", b"viewer"]
    d = strings(dvals, validity=[True, True, True, False, True])
    idx = [0, 1, 2, 3, 4, -1, 5, 2, 0, 1 << 30]
    out["dict"] = Batch(len(idx), strings([b"b" * 36] * len(idx)), Col(DICT, data=idx), strings([b"1500000012345"] * len(idx)),
                        dictionary=d, dict_len=len(dvals))
    # offsets that run backwards or past data_bytes: the data buffer is over-allocated with
    # countable bytes, so following a lying offset would count
    k = 8
    good = strings([b"b" * 36] * k)
    lying = np.array(good.offsets, dtype=np.int32)
    lying[3] = lying[2] - 5            # row 2 runs backwards, row 3 starts below its neighbour's end
    big = np.frombuffer(b"b" * 36 * (k + 4), dtype=np.uint8)
    ad = Col(STRING, lying, big, data_bytes=36 * k)
    tm = strings([b"1500000012345"] * k)
    tl = np.array(tm.offsets, dtype=np.int32)
    tl[k] = tl[k] + 13                 # the last row ends past data_bytes (inside the allocation)
    tmc = Col(STRING, tl, np.frombuffer(b"1500000012345" * (k + 2), dtype=np.uint8), data_bytes=13 * k)
    neg = strings([b"view"] * k)
    no = np.array(neg.offsets, dtype=np.int32)
    no[0] = -4                          # a negative first offset
    out["offsets"] = Batch(k, ad, Col(STRING, no, neg.data), tmc)
    return out
