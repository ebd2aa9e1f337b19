"""CPU: the Arrow count's Python model (tests/arrow_model.py) against the native host model
(csrc/ysb_arrow.h, through ysb_arrow_count_host), the oracle on the rows' JSON rendering, the
committed pyarrow buffers and the expected counts of gen_s7; the package's own ArrowArray builders
and, where pyarrow is installed, a live RecordBatch through bind, view and the copy plan.  No GPU."""
import numpy as np
import pytest

import arrow_model as am
import golden_data as gd
from oracle import oracle
from ysb_amd import YsbError, arrow

CMP = ("events", "views", "joined", "join_misses", "parse_errors", "time_errors", "foreign_shard")


@pytest.fixture(scope="module")
def gen_map():
    ads, camp = gd.ad_arrays()
    return dict(zip([a.encode() for a in ads], camp))


def native(A, ad_map, **kw):
    cells, st, inv = arrow.count_host(A, ad_map, **kw)
    return cells, st, inv


def assert_native(b, ad_map, expressible=True, **kw):
    """The Python model equals the native one on the batch's buffers as they are, viewed through
    the package's own ArrowArray, and on the host form's packed copy."""
    inv = {}
    want, wst = am.count(b, ad_map, invalid=inv, **kw)
    forms = [am.to_cols(b)]
    if expressible:
        node = am.to_node(b)
        bd = arrow.bind(node.schema)
        assert list(bd.child) == [1, 2, 3] and bd.n_children == 4     # user_id is ignored
        forms += [arrow.view(bd, node), arrow.pack(bd, node)[1]]
    for A in forms:
        cells, st, ginv = native(A, ad_map, **kw)
        assert cells == want and ginv == inv
        for k in CMP:
            assert st[k] == wst[k], k
    return want, wst


def assert_oracle(b, ad_map, want, wst):
    """The oracle on the rows' JSON rendering; rows invalid by offsets or by dictionary index
    have no JSON form and are left out of this comparison only."""
    lines, formless = am.render_json(b)
    raw = b"".join(lines)
    offs = np.cumsum([0] + [len(x) for x in lines[:-1]]) if lines else []
    rows, ost = oracle.run(oracle.AdMap(list(ad_map), list(ad_map.values())), raw, offs)
    assert rows == want
    for k in ("views", "joined", "join_misses", "time_errors"):
        assert ost[k] == wst[k], k
    assert ost["events"] == wst["events"] - formless and ost["parse_errors"] == wst["parse_errors"] - formless


@pytest.mark.parametrize("name", ["plain", "int64", "nulls", "dict", "offsets"])
def test_corpus(name):
    m = am.corpus_map()
    b = am.corpus()[name]
    want, wst = assert_native(b, m, expressible=name != "offsets")
    assert_oracle(b, m, want, wst)
    if name == "plain":
        assert (wst["views"], wst["joined"], wst["join_misses"], wst["time_errors"]) == (23, 19, 4, 6)
    if name == "nulls":
        assert wst["parse_errors"] == 10 and wst["joined"] == 2
    if name == "dict":
        assert wst["parse_errors"] == 4 and wst["views"] == 4      # both `view` entries are views
    if name == "offsets":
        assert wst["parse_errors"] == 3


@pytest.mark.parametrize("name", am.FIXTURES)
def test_fixtures(gen_map, name):
    b = am.fixture(name)
    want, wst = assert_native(b, gen_map)
    assert_oracle(b, gen_map, want, wst)
    if name in ("gen_s7_strings", "gen_s7_int64", "gen_s7_dict"):
        exp, est = gd.expected("gen_s7")
        assert want == exp
        for k in ("events", "views", "joined", "join_misses", "parse_errors", "time_errors"):
            assert wst[k] == est[k], k
    if name == "gen_s7_slice67":
        assert b.ad.offset == 67 and b.n_rows == 1000
    if name == "nulls":
        assert b.ad.offset == 3 and wst["parse_errors"] == 13


@pytest.mark.parametrize("kind", ["strings", "int64", "dict"])
@pytest.mark.parametrize("off", [0, 1, 7, 67])
def test_slices_in_the_three_encodings(gen_map, kind, off):
    full = am.fixture("gen_s7_strings")
    rows = [am.row(full, i)[1] for i in range(200)]
    filler = (rows[0][0], b"view", rows[0][2])
    for n in (0, 1, 65):
        b = am.encode(rows[100:100 + n], kind, lead=off, tail=9, filler=filler, bitmaps=off % 2 == 1)
        _, wst = assert_native(b, gen_map)
        assert wst["events"] == n


def test_sharded_model(gen_map):
    b = am.fixture("gen_s7_int64")
    from ysb_amd import ad_shard
    mine = {k: v for k, v in gen_map.items() if ad_shard(k, 2) == 0}
    _, wst = assert_native(b, mine, shard=(0, 2))
    assert wst["foreign_shard"] > 0 and wst["join_misses"] == 0


def test_pyarrow_record_batch(gen_map):
    """A live RecordBatch and a slice of it through _export_to_c, bind, view and the plan: the real
    C structs."""
    pa = pytest.importorskip("pyarrow")
    full = am.fixture("gen_s7_strings")
    rows = [am.row(full, i)[1] for i in range(300)]
    cols = {"ad_id": pa.array([r[0].decode() for r in rows]), "pad": pa.array(list(range(300))),
            "event_time": pa.array([int(r[2]) for r in rows], type=pa.timestamp("ms")),
            "event_type": pa.array([r[1].decode() for r in rows]).dictionary_encode()}
    rb = pa.record_batch(cols)
    for batch, lo in ((rb, 0), (rb.slice(67, 150), 67)):
        ex = arrow.export(batch)
        bd = arrow.bind(ex.schema)
        assert list(bd.child) == [0, 3, 2] and list(bd.kind) == [arrow.STRING, arrow.DICT, arrow.INT64]
        want, wst = am.count(am.encode(rows[lo:lo + batch.num_rows], "int64"), gen_map)
        ranges, total = arrow.plan(bd, ex)
        assert total % 16 == 0 and all(r[2] % 16 == 0 for r in ranges)
        for A in (arrow.view(bd, ex), arrow.pack(bd, ex)[1]):
            cells, st, _ = native(A, gen_map)
            assert cells == want and st["views"] == wst["views"] and st["events"] == batch.num_rows
    ex = arrow.export(pa.record_batch({"ad_id": cols["ad_id"], "event_type": cols["event_type"],
                                       "event_time": pa.array([1] * 300, type=pa.timestamp("us"))}))
    with pytest.raises(YsbError) as e:
        arrow.bind(ex.schema)
    assert e.value.code == -5 and "event_time" in str(e.value) and "tsu:" in str(e.value)
