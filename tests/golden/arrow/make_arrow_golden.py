"""Writes the Arrow fixtures beside this script: the raw buffers that pyarrow produces for the
1,500 rows of ../gen_s7.jsonl as a record batch -- string times, int64 times, event_type
dictionary-encoded --, for a slice of it at offset 67, and for a small sliced batch with nulls in
each column.  Each .npz holds the buffers as uint8 arrays and the arrays' offset,
length and dictionary length, so the tests read them with numpy alone and an independent writer
made the offsets, bitmaps and dictionary.  Data only; the versions are recorded in versions.txt.
Run from anywhere: python tests/golden/arrow/make_arrow_golden.py"""
import json
import os

import numpy as np
import pyarrow as pa

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("ad_id", "event_type", "event_time")


def buffers(arr, out, prefix):
    """arr's buffers as uint8 arrays (an absent one: not stored), its offset and length."""
    names = ("validity", "values") if pa.types.is_integer(arr.type) or pa.types.is_dictionary(arr.type) else ("validity", "offsets", "data")
    for nm, b in zip(names, arr.buffers()):
        if b is not None:
            out[prefix + nm] = np.frombuffer(b, dtype=np.uint8).copy()
    out[prefix + "offset"] = np.int64(arr.offset)
    out[prefix + "length"] = np.int64(len(arr))
    if pa.types.is_dictionary(arr.type):
        buffers(arr.dictionary, out, prefix + "dict_")


def save(name, rb):
    out = {"n_rows": np.int64(rb.num_rows)}
    for nm in NAMES:
        buffers(rb.column(nm), out, nm + "_")
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print(name, rb.num_rows, os.path.getsize(os.path.join(HERE, name + ".npz")))


def main():
    with open(os.path.join(HERE, "..", "gen_s7.jsonl"), "rb") as f:
        ev = [json.loads(ln) for ln in f if ln.strip()]
    ad, ty, tm = ([e[k] for e in ev] for k in NAMES)
    other = pa.array([e["user_id"] for e in ev])
    strs = pa.record_batch({"user_id": other, "ad_id": pa.array(ad), "event_type": pa.array(ty), "event_time": pa.array(tm)})
    save("gen_s7_strings", strs)
    save("gen_s7_int64", pa.record_batch({"ad_id": pa.array(ad), "event_type": pa.array(ty),
                                          "event_time": pa.array([int(t) for t in tm], type=pa.int64())}))
    save("gen_s7_dict", pa.record_batch({"ad_id": pa.array(ad), "event_time": pa.array(tm),
                                         "event_type": pa.array(ty).dictionary_encode()}))
    save("gen_s7_slice67", strs.slice(67, 1000))
    k = 40
    nul = pa.record_batch({
        "ad_id": pa.array([None if i % 7 == 1 else ad[i] for i in range(k)], type=pa.string()),
        "event_type": pa.array([None if i % 7 == 2 else ty[i] for i in range(k)], type=pa.string()),
        "event_time": pa.array([None if i % 7 == 3 else tm[i] for i in range(k)], type=pa.string())})
    save("nulls", nul.slice(3, 33))
    with open(os.path.join(HERE, "versions.txt"), "w") as f:
        f.write("pyarrow %s\nnumpy %s\n" % (pa.__version__, np.__version__))


if __name__ == "__main__":
    main()
