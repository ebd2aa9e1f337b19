"""Apache Arrow record batches (include/ysb_hip.h "Arrow record batches").

The two structs of the Arrow C data interface as ctypes mirrors, bind(schema), and builders that
make an ArrowArray / ArrowSchema pair from numpy buffers -- nothing here needs pyarrow.  A
pyarrow RecordBatch (or any object with __arrow_c_array__) is taken through export().
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import (ArrowArray, ArrowSchema, YsbArrowBinding, YsbArrowCol, YsbArrowCols, YsbArrowRange, check, lib)

STRING, INT64, DICT = 1, 2, 3
NAMES = ("ad_id", "event_type", "event_time")
STATS = ("events", "views", "joined", "join_misses", "parse_errors", "time_errors", "foreign_shard")

_RELEASE = C.CFUNCTYPE(None, C.c_void_p)(lambda p: None)   # the builders' structs own nothing
_RELEASE_PTR = C.cast(_RELEASE, C.c_void_p)


class Node:
    """One ArrowArray with its ArrowSchema, and what keeps their buffers alive."""

    def __init__(self, fmt, length, buffers, offset=0, children=(), dictionary=None, name=b"", null_count=-1):
        self.keep = [buffers, children, dictionary]
        self.array, self.schema = ArrowArray(), ArrowSchema()
        a, s = self.array, self.schema
        fmt = fmt.encode() if isinstance(fmt, str) else fmt
        name = name.encode() if isinstance(name, str) else name
        s.format, s.name, s.metadata, s.flags = fmt, name, None, 2
        a.length, a.null_count, a.offset = int(length), int(null_count), int(offset)
        a.n_buffers = len(buffers)
        self._bufs = (C.c_void_p * max(len(buffers), 1))()
        for i, b in enumerate(buffers):
            self._bufs[i] = None if b is None else (b if isinstance(b, int) else b.ctypes.data)
        a.buffers = C.cast(self._bufs, C.POINTER(C.c_void_p))
        n = len(children)
        a.n_children = s.n_children = n
        self._ac = (C.POINTER(ArrowArray) * max(n, 1))()
        self._sc = (C.POINTER(ArrowSchema) * max(n, 1))()
        for i, ch in enumerate(children):
            self._ac[i] = C.pointer(ch.array)
            self._sc[i] = C.pointer(ch.schema)
        a.children = C.cast(self._ac, C.POINTER(C.POINTER(ArrowArray)))
        s.children = C.cast(self._sc, C.POINTER(C.POINTER(ArrowSchema)))
        if dictionary is not None:
            a.dictionary = C.pointer(dictionary.array)
            s.dictionary = C.pointer(dictionary.schema)
        a.release = s.release = _RELEASE_PTR

    def named(self, name):
        self.schema.name = name.encode() if isinstance(name, str) else name
        return self


def _bitmap(valid):
    """A validity bitmap (uint8 array) from bools, None (absent) or a ready uint8 array."""
    if valid is None:
        return None
    valid = np.asarray(valid)
    return valid if valid.dtype == np.uint8 else np.packbits(valid.astype(np.bool_), bitorder="little")


def string_array(offsets, data, validity=None, offset=0, length=None, fmt="u"):
    """A utf8 / binary array over int32 offsets and uint8 data (validity: bools of ALL elements,
    a bitmap, or None)."""
    offsets = np.ascontiguousarray(offsets, dtype=np.int32)
    data = np.ascontiguousarray(data, dtype=np.uint8)
    length = offsets.size - 1 - offset if length is None else length
    return Node(fmt, length, [_bitmap(validity), offsets, data], offset)


def strings(values, validity=None, offset=0, length=None, fmt="u"):
    """The same from a list of bytes values."""
    offs = np.zeros(len(values) + 1, dtype=np.int32)
    offs[1:] = np.cumsum([len(v) for v in values])
    return string_array(offs, np.frombuffer(b"".join(values), dtype=np.uint8), validity, offset, length, fmt)


def int64_array(values, validity=None, offset=0, length=None, fmt="l"):
    values = np.ascontiguousarray(values, dtype=np.int64)
    return Node(fmt, values.size - offset if length is None else length, [_bitmap(validity), values], offset)


def dict_array(indices, dictionary, validity=None, offset=0, length=None, fmt="i"):
    """A dictionary-encoded array: int32 indices into `dictionary` (a string Node)."""
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    return Node(fmt, indices.size - offset if length is None else length, [_bitmap(validity), indices], offset,
                dictionary=dictionary)


def batch(columns, validity=None, offset=0, length=None):
    """A record batch (a struct) of {name: Node}; length defaults to the shortest child's."""
    kids = [n.named(k) for k, n in columns.items()]
    if length is None:
        length = min(k.array.length for k in kids) - offset if kids else 0
    return Node("+s", length, [_bitmap(validity)], offset, children=kids)


class Exported:
    """A batch exported by its producer (pyarrow's _export_to_c / the PyCapsule protocol): the two
    structs, released when this object goes."""

    def __init__(self, obj):
        self.array, self.schema = ArrowArray(), ArrowSchema()
        self.keep = [obj]
        if hasattr(obj, "__arrow_c_array__"):
            sc, ac = obj.__arrow_c_array__()
            self.keep += [sc, ac]   # the capsules own the structs
            get = C.pythonapi.PyCapsule_GetPointer
            get.restype, get.argtypes = C.c_void_p, [C.py_object, C.c_char_p]
            self.array = ArrowArray.from_address(get(ac, b"arrow_array"))
            self.schema = ArrowSchema.from_address(get(sc, b"arrow_schema"))
            self.array._keep, self.schema._keep = (ac, obj), (sc, obj)   # either struct alone keeps its capsule
            self._owned = False
        else:
            obj._export_to_c(C.addressof(self.array), C.addressof(self.schema))
            self._owned = True

    def __del__(self):
        if getattr(self, "_owned", False):
            for st in (self.array, self.schema):
                if st.release:
                    C.CFUNCTYPE(None, C.c_void_p)(st.release)(C.addressof(st))


def export(obj):
    """obj as something with .array / .schema: a builder Node as it is, anything else exported."""
    return obj if isinstance(obj, Node) else Exported(obj)


def bind(schema):
    """ysb_arrow_bind: where ad_id, event_type and event_time are in a struct schema and how each
    is stored.  schema: an ArrowSchema, or anything export() takes."""
    if not isinstance(schema, ArrowSchema):
        schema = export(schema).schema
    b = YsbArrowBinding()
    check(lib().ysb_arrow_bind(C.byref(schema), C.byref(b)), None)
    return b


def _addr(x):
    return None if x is None else (int(x) if isinstance(x, (int, np.integer)) else x.ctypes.data)


def col(kind, offsets=None, data=None, validity=None, data_bytes=None, offset=0, validity_offset=None, data_first=0):
    """A ysb_arrow_col from numpy arrays (host) or integer addresses (device)."""
    c = YsbArrowCol()
    c.kind, c.data_first = kind, data_first
    c.validity, c.offsets, c.data = _addr(validity), _addr(offsets), _addr(data)
    c.data_bytes = (data.nbytes + data_first if hasattr(data, "nbytes") else 0) if data_bytes is None else data_bytes
    c.offset = offset
    c.validity_offset = offset if validity_offset is None else validity_offset
    c._keep = (offsets, data, validity)
    return c


def cols(n_rows, ad, typ, time, dictionary=None, dict_len=0, validity=None, offset=0):
    """A ysb_arrow_cols of three col()s (and the dictionary's)."""
    A = YsbArrowCols()
    A.n_rows, A.validity, A.offset = n_rows, _addr(validity), offset
    for i, c in enumerate((ad, typ, time)):
        A.col[i] = c
    if dictionary is not None:
        A.dict = dictionary
    A.dict_len = dict_len
    A._keep = (ad, typ, time, dictionary, validity)
    return A


def view(binding, exported):
    """ysb_arrow_view: the whole batch in place as a ysb_arrow_cols of host pointers."""
    A = YsbArrowCols()
    check(lib().ysb_arrow_view(C.byref(binding), C.byref(exported.array), C.byref(A)), None)
    A._keep = exported
    return A


def plan(binding, exported):
    """ysb_arrow_plan: ([(src address, bytes, dst, col, what)], total bytes of the packed image)."""
    n, total = C.c_uint64(), C.c_uint64()
    r = (YsbArrowRange * 24)()
    check(lib().ysb_arrow_plan(C.byref(binding), C.byref(exported.array), r, 24, C.byref(n), C.byref(total)), None)
    return [(r[i].src or 0, r[i].bytes, r[i].dst, r[i].col, r[i].what) for i in range(n.value)], total.value


def pack(binding, exported):
    """ysb_arrow_pack: (image, ysb_arrow_cols into it) -- the host form's packed copy."""
    _, total = plan(binding, exported)
    image = np.zeros(max(total, 1), dtype=np.uint8)
    A = YsbArrowCols()
    check(lib().ysb_arrow_pack(C.byref(binding), C.byref(exported.array), image.ctypes.data, total, C.byref(A)), None)
    A._keep = image
    return image, A


def count_host(A, ad_map, divisor=10000, shard=None):
    """ysb_arrow_count_host: the native host model.  ad_map: {key bytes: campaign}.
    -> ({(campaign, bucket): count}, stats, {null, offsets, dict: invalid rows})."""
    keys = list(ad_map)
    koff = np.zeros(len(keys) + 1, dtype=np.uint32)
    koff[1:] = np.cumsum([len(k) for k in keys])
    kb = np.frombuffer(b"".join(keys) + b"\0", dtype=np.uint8)
    camp = np.asarray([ad_map[k] for k in keys] + [0], dtype=np.uint32)
    st, inv, n = (C.c_uint64 * 8)(), (C.c_uint64 * 3)(), C.c_uint64()
    cap = int(A.n_rows) + 1
    cells = np.zeros(3 * cap, dtype=np.int64)
    rank, nr = shard if shard else (0, 1)
    check(lib().ysb_arrow_count_host(C.byref(A), kb.ctypes.data, koff.ctypes.data, camp.ctypes.data, len(keys), divisor,
                                     rank, nr, st, inv, cells.ctypes.data, cap, C.byref(n)), None)
    out = {(int(cells[3 * i]), int(cells[3 * i + 1])): int(cells[3 * i + 2]) for i in range(n.value)}
    return out, dict(zip(STATS, st)), dict(zip(("null", "offsets", "dict"), inv))
