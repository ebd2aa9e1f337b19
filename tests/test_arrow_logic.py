"""CPU: the Arrow rules (csrc/ysb_arrow.h: the row rule and its host model, the schema binding,
the host form's copy plan) -- as a stand-alone native program, tests/native/arrow_logic.cpp, plain
and under the host sanitizers, and through the C ABI's host entries with the package's own
ArrowArray / ArrowSchema builders.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import arrow_model as am
from test_capi import ROOT, run_native
from ysb_amd import YsbError, arrow


def test_arrow_logic_native(tmp_path):
    """Every accepted and refused format; Long.parseLong's cases; the model over the hand-made
    corpus (ad ids of 0..200 bytes, the five types, the times, nulls with bitmaps from bit 3,
    dictionary indices -1 and dict_len, duplicate `view` entries, lying offsets); the plan over
    sliced batches (offsets 0, 1, 7, 67; with and without bitmaps; three encodings): exactly the
    rows' bytes, and the model on the packed copy with every source byte poisoned."""
    run_native(tmp_path, "arrow_logic")


def test_arrow_logic_native_sanitized(tmp_path):
    """The same program with -fsanitize=address,undefined, as a stand-alone program: every buffer
    is an exact-size heap allocation, so a read outside a stated buffer or a planned range faults."""
    exe = tmp_path / "arrow_logic_san"
    inc = [a for d in (("streaming-benchmarks_amd", "csrc"), ("include",)) for a in ("-I", os.path.join(ROOT, *d))]
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
                   + inc + [os.path.join(ROOT, "tests", "native", "arrow_logic.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK") and not r.stderr, r.stdout + r.stderr


def schema(ad="u", ty="u", tm="u", ty_dict=None, top="+s", names=arrow.NAMES):
    """A schema alone: empty arrays of the given formats."""
    e32, e8 = np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.uint8)
    kids = []
    for nm, fmt, d in zip(names, (ad, ty, tm), (None, ty_dict, None)):
        dn = arrow.Node(d, 0, [None, e32, e8]) if d else None
        kids.append(arrow.Node(fmt, 0, [None, e32, e8], dictionary=dn, name=nm))
    return arrow.Node(top, 0, [None], children=kids)


ACCEPTED = [("u", "u", "u", None), ("z", "z", "z", None), ("u", "u", "l", None), ("u", "z", "tsm:", None),
            ("u", "u", "tsm:Europe/Berlin", None), ("u", "i", "u", "u"), ("z", "i", "l", "z")]
REFUSED = [("U", "u", "u", None, "ad_id", "U"), ("u", "Z", "u", None, "event_type", "Z"), ("vu", "u", "u", None, "ad_id", "vu"),
           ("u", "u", "vz", None, "event_time", "vz"), ("w:36", "u", "u", None, "ad_id", "w:36"),
           ("u", "u", "tss:", None, "event_time", "tss:"), ("u", "u", "tsu:UTC", None, "event_time", "tsu:UTC"),
           ("u", "u", "tsn:", None, "event_time", "tsn:"), ("u", "s", "u", "u", "event_type", "s"),
           ("u", "l", "u", "u", "event_type", "l"), ("u", "C", "u", "u", "event_type", "C"),
           ("u", "i", "u", "U", "event_type", "U"), ("u", "u", "i", None, "event_time", "i"), ("u", "+r", "u", None, "event_type", "+r")]


@pytest.mark.parametrize("ad,ty,tm,d", ACCEPTED)
def test_bind_accepts(ad, ty, tm, d):
    b = arrow.bind(schema(ad, ty, tm, d).schema)
    want = [arrow.STRING, arrow.DICT if d else arrow.STRING, arrow.INT64 if tm[0] in "lt" else arrow.STRING]
    assert list(b.kind) == want and list(b.child) == [0, 1, 2] and b.n_children == 3


@pytest.mark.parametrize("ad,ty,tm,d,field,fmt", REFUSED)
def test_bind_refuses_naming_field_format_and_way_out(ad, ty, tm, d, field, fmt):
    with pytest.raises(YsbError) as e:
        arrow.bind(schema(ad, ty, tm, d).schema)
    assert e.value.code == -5 and "'%s'" % field in str(e.value) and "'%s'" % fmt in str(e.value) and "cast" in str(e.value)


def test_bind_refuses_a_missing_field_and_a_top_level_that_is_no_struct():
    with pytest.raises(YsbError) as e:
        arrow.bind(schema(names=("ad_id", "event_type", "time")).schema)
    assert e.value.code == -5 and "'event_time'" in str(e.value) and "missing" in str(e.value)
    with pytest.raises(YsbError) as e:
        arrow.bind(schema(top="+l").schema)
    assert e.value.code == -5 and "'+l'" in str(e.value) and "struct" in str(e.value)
    with pytest.raises(YsbError) as e:
        arrow.bind(arrow.strings([b"x"]).schema)
    assert e.value.code == -5 and "'u'" in str(e.value)


@pytest.mark.parametrize("bitmaps", [False, True])
@pytest.mark.parametrize("off", [0, 1, 7, 67])
def test_plan_touches_only_the_rows_bytes(off, bitmaps):
    """The planned ranges lie inside the batch's buffers, cover the rows' offsets, data and bitmap
    bytes and nothing of the 70 filler elements in front of and behind them beyond the bitmap
    bytes they share; with every byte outside the plan poisoned, the packed copy still gives the
    original's counts."""
    m = am.corpus_map()
    rows = am.corpus_rows()
    filler = (b"b" * 36, b"view", b"1500000012345")
    for kind in ("strings", "dict"):
        b = am.encode(rows, kind, lead=off, tail=70, filler=filler, bitmaps=bitmaps)
        want, wst = am.count(b, m)
        node = am.to_node(b, extra=False)
        bd = arrow.bind(node.schema)
        ranges, total = arrow.plan(bd, node)
        bufs = [x for c in (b.ad, b.typ, b.time, b.dict) if c is not None for x in (c.offsets, c.data, c.validity) if x is not None]
        bufs += [b.validity] if b.validity is not None else []
        bufs = list({id(x): x for x in bufs}.values())   # (the all-ones bitmap is one array at every level)
        keep = {id(x): np.zeros(x.nbytes, dtype=bool) for x in bufs}
        for src, nb, dst, _, _ in ranges:
            owner = [x for x in bufs if x.ctypes.data <= src and src + nb <= x.ctypes.data + x.nbytes]
            assert len(owner) == 1 and dst % 16 == 0
            keep[id(owner[0])][src - owner[0].ctypes.data:src - owner[0].ctypes.data + nb] = True
        n = len(rows)
        assert keep[id(b.ad.offsets)].sum() == 4 * (n + 1) and keep[id(b.ad.data)].sum() == sum(len(r[0]) for r in rows)
        if bitmaps:
            assert keep[id(b.ad.validity)].sum() == ((off % 8) + n + 7) // 8
        for x in bufs:   # poison what the plan does not name
            x.view(np.uint8).reshape(-1)[~keep[id(x)]] = 0x5A
        _, packed = arrow.pack(bd, node)
        cells, st, _ = arrow.count_host(packed, m)
        assert cells == want and all(st[k] == wst[k] for k in arrow.STATS)
