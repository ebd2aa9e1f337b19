"""CPU: the columnar count's model (tests/colcount_model.py) against the golden expectation, the
mutation corpus' tags and hand-made rows; ysb_columns_read_ranges (a host function) against the
layout."""
import numpy as np
import pytest

import colcount_model as ccm
import columns_model as cm
import golden_data as gd
from oracle import dostats
from ysb_amd import YsbError, _lib, columns_read_ranges


def fixture_lines(stem="gen_s7"):
    raw, _ = gd.events(stem)
    return dostats.split_lines(raw)[0]


def ad_map():
    ads, camp = gd.ad_arrays()
    return {a.encode(): c for a, c in zip(ads, camp)}


@pytest.mark.parametrize("java_order", [False, True])
@pytest.mark.parametrize("validity", [False, True])
def test_model_equals_golden(java_order, validity):
    lines = fixture_lines()
    image, valid, _ = cm.build(lines, java_order=java_order)
    assert valid.all()
    cells, st = ccm.count(image, 1500, 1500, ad_map(), java_order=java_order, validity=validity)
    want, wst = gd.expected("gen_s7")
    assert cells == want and len(cells) == 80 and len({b for _, b in cells}) == 8
    assert (st["events"], st["views"], st["joined"], st["join_misses"], st["parse_errors"]) == (1500, 506, 506, 0, 0)
    for k in ("events", "views", "joined", "join_misses", "parse_errors", "time_errors"):
        assert st[k] == wst[k], k


def test_model_on_the_mutation_corpus():
    corpus = cm.mutation_corpus(fixture_lines())
    image, valid, _ = cm.build([ln for ln, _, _ in corpus])
    cells, st = ccm.count(image, 1500, 1500, ad_map(), validity=True)
    tagged_invalid = sum(not ok for _, _, ok in corpus)
    assert st["parse_errors"] == tagged_invalid == 498 == int((~valid).sum())
    assert st["events"] == 1500 and st["views"] == 329 and st["events"] - st["parse_errors"] == 1002
    assert st["joined"] + st["join_misses"] == st["views"] and sum(cells.values()) == st["joined"]
    # without the bitmap the invalid rows' zero bytes are plain non-views
    cells2, st2 = ccm.count(image, 1500, 1500, ad_map())
    assert cells2 == cells and st2["parse_errors"] == 0 and st2["views"] == 329


def test_the_filter_sees_the_cut_value():
    m = ad_map()
    ad = next(iter(m))
    image = ccm.make_image([ad] * 4, [b"view", b"view", b"vie\0", b"clic"], [10000, 25000, 10000, 10000], 4)
    # ("viewer" cut to its four bytes is row 1's "view")
    cells, st = ccm.count(image, 4, 4, m)
    assert st["views"] == 2 and st["joined"] == 2 and cells == {(m[ad], 1): 1, (m[ad], 2): 1}
    line = fixture_lines()[0]
    d = cm._fields(line)
    img, valid, _ = cm.build([cm._render(dict(d, event_type="viewer")), cm._render(dict(d, event_type="vie"))])
    assert valid.tolist() == [True, False]
    _, st = ccm.count(img, 2, 2, m, validity=True)
    assert st["views"] == 1 and st["parse_errors"] == 1
    r = dostats.run([cm._render(dict(d, event_type="viewer"))], gd.ad_map())
    assert r.views == 0 and not r.counts   # the JSON path: "viewer" is no view


@pytest.mark.parametrize("rows,n", [(1, 1), (64, 64), (5000, 5000), (5000, 37), (1 << 20, 999_999)])
@pytest.mark.parametrize("validity", [False, True])
def test_read_ranges_against_the_layout(rows, n, validity):
    flags = _lib.YSB_COL_VALIDITY if validity else 0
    got = columns_read_ranges(rows, n, flags)
    assert got == ccm.read_ranges(rows, n, validity) and len(got) == (4 if validity else 3)
    assert columns_read_ranges(rows, n, flags | _lib.YSB_COL_JAVA_ORDER) == got
    lay = cm.layout(rows)
    ends = lay["start"][1:] + [None]
    for off, nb in got:   # each range inside its column, ascending, page-aligned starts
        j = lay["start"].index(off)
        assert off % 4096 == 0 and off + nb <= ends[j]
    assert [o for o, _ in got] == sorted(o for o, _ in got)
    assert sum(nb for _, nb in got[:3]) == 48 * n


def test_read_ranges_argument_errors():
    for args, code in (((0, 0, 0), -1), ((1 << 31, 1, 0), -1), ((64, 1, 4), -1), ((64, 65, 0), -4)):
        with pytest.raises(YsbError) as e:
            columns_read_ranges(*args)
        assert e.value.code == code, args
    assert columns_read_ranges(64, 0, _lib.YSB_COL_VALIDITY) == [(o, 0) for o, _ in ccm.read_ranges(64, 0, True)]
