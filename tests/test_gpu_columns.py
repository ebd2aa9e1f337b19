"""GPU: ysb_decode_columns_device against the CPU model (tests/columns_model.py).  Every
decode starts from an output buffer filled with 0xA5 and the WHOLE buffer -- columns, page
padding, rows past the batch, the validity words -- is compared with the model's image laid
over the same canary, so a byte written where none may be shows as much as a wrong value."""
import numpy as np
import pytest

import columns_model as cm
import golden_data as gd
from oracle import dostats
from ysb_amd import YsbContext, YsbError, _lib, columns_layout

pytestmark = pytest.mark.gpu

CANARY = 0xA5
SMALL = dict(n_campaigns=10, window_ring=16, max_batch_events=1 << 12, max_batch_bytes=1 << 20,
             overflow_capacity=1 << 10)


def fixture_lines(stem, ext=".jsonl"):
    raw, _ = gd.events(stem, ext)
    return dostats.split_lines(raw)[0]


@pytest.fixture(scope="module")
def ctx():   # JSON; no ad map is ever loaded: the decode needs none
    with YsbContext(**SMALL) as c:
        yield c


@pytest.fixture(scope="module")
def ctx_ip():
    with YsbContext(require_ip=True, **SMALL) as c:
        yield c


@pytest.fixture(scope="module")
def ctx_tbl():
    with YsbContext(input_format="tbl", **SMALL) as c:
        yield c


@pytest.fixture(scope="module")
def corpus():
    return cm.mutation_corpus(fixture_lines("gen_s7"))


def decode(c, lines, batch_rows=None, stamp=10, flags=0, shift=0):
    """(image of all start[8] bytes over the canary, info) of one decode."""
    data, offs = cm.pack(lines, shift)
    n = len(lines)
    rows = max(n, 1) if batch_rows is None else batch_rows
    total = columns_layout(rows)["start"][8]
    image = np.full(total, CANARY, dtype=np.uint8)
    d_b, d_o, d_out = c.device_alloc(data.size), c.device_alloc(4 * n), c.device_alloc(total)
    try:
        c.h2d(d_b, data)
        c.h2d(d_o, offs)
        c.h2d(d_out, image)
        assert d_b % 16 == 0 and d_out % 16 == 0
        info = c.decode_columns_device(d_b, data.size, d_o, n, d_out, rows, stamp=stamp, flags=flags)
        c.d2h(image, d_out)
    finally:
        for p in (d_b, d_o, d_out):
            c.device_free(p)
    return image, info


def check(c, lines, fmt="json", require_ip=False, **kw):
    want, valid, counts = cm.build(lines, batch_rows=kw.get("batch_rows"), fmt=fmt, require_ip=require_ip,
                                   stamp=kw.get("stamp", 10),
                                   java_order=bool(kw.get("flags", 0) & _lib.YSB_COL_JAVA_ORDER), canary=CANARY)
    got, info = decode(c, lines, **kw)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "first differing bytes at %s (of %d)" % (bad[:8].tolist(), got.size)
    assert info["rows"] == counts["rows"] and info["valid"] == counts["valid"]
    assert info["kernel_ms"] > 0
    return info, counts


def test_generator_json_all_fast(ctx):
    lines = fixture_lines("gen_s7")
    assert len(lines) == 1500   # 23 full tiles + 28
    info, counts = check(ctx, lines)
    assert counts["valid"] == 1500 and info["fast_rows"] == 1500


@pytest.mark.parametrize("stem", ["gen_s7", "edge_tbl"])
def test_tbl_fixtures(ctx_tbl, stem):
    lines = fixture_lines(stem, ".tbl")
    info, counts = check(ctx_tbl, lines, fmt="tbl")
    if stem == "gen_s7":
        assert counts["valid"] == 1500 and info["fast_rows"] == 1500


def test_edge_json(ctx):
    _, counts = check(ctx, fixture_lines("edge"))
    assert counts["valid"] == 28


def test_edge_json_require_ip(ctx_ip):
    _, counts = check(ctx_ip, fixture_lines("edge"), require_ip=True)
    assert 0 < counts["valid"] < 28


@pytest.mark.parametrize("extra", [0, 100])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 1500])
def test_mutation_corpus(ctx, corpus, n, extra):
    lines = [ln for ln, _, _ in corpus[:n]]
    info, counts = check(ctx, lines, batch_rows=n + extra)
    assert counts["valid"] == sum(ok for _, _, ok in corpus[:n])
    if n >= 18:   # fast and general lanes inside every tile
        assert 0 < info["fast_rows"] < n


def test_mutation_corpus_require_ip(ctx_ip, corpus):
    lines = [ln for ln, _, _ in corpus[:200]]
    _, counts = check(ctx_ip, lines, require_ip=True)
    assert counts["valid"] == sum(ok and name not in cm.NEEDS_IP for _, name, ok in corpus[:200])


@pytest.mark.parametrize("shift", [7, 16, 33])
def test_first_line_not_tile_aligned(ctx, corpus, shift):
    check(ctx, [ln for ln, _, _ in corpus[:200]], shift=shift)


def test_line_longer_than_a_tile(ctx):
    gen = fixture_lines("gen_s7")[:150]
    d = cm._fields(gen[70])
    long_line = cm._render(d, extra=("ad_id", '"pad": "%s"' % ("x" * 20000)))   # > 64 * 272 bytes of LDS
    assert cm.decode_line(long_line) is not None
    lines = gen[:70] + [long_line] + gen[71:]
    info, counts = check(ctx, lines)
    assert counts["valid"] == 150 and 64 <= info["fast_rows"] < 150


@pytest.mark.parametrize("where", ["first_item", "seventh_item"])
def test_tbl_row_longer_than_a_tile(ctx_tbl, where):
    gen = fixture_lines("gen_s7", ".tbl")[:150]
    row = gen[70].rstrip(b"\n")
    pad = b"x" * 20000   # > 64 * 160 bytes of LDS: the row is split straight from HBM
    long_row = (pad + row[row.index(b"|"):] if where == "first_item" else row + b"|" + pad) + b"\n"
    lines = gen[:70] + [long_row] + gen[71:]
    info, counts = check(ctx_tbl, lines, fmt="tbl")
    assert counts["valid"] == 150 and 64 <= info["fast_rows"] < 150


def test_java_order_swaps_only_the_longs(ctx, corpus):
    lines = [ln for ln, _, _ in corpus[:130]]
    check(ctx, lines, flags=_lib.YSB_COL_JAVA_ORDER)
    le, _ = decode(ctx, lines)
    be, _ = decode(ctx, lines, flags=_lib.YSB_COL_JAVA_ORDER)
    st = columns_layout(130)["start"]
    assert (le[:st[5]] == be[:st[5]]).all() and (le[st[7]:] == be[st[7]:]).all()
    for j in (5, 6):
        a = le[st[j]:st[j] + 8 * 130].reshape(130, 8)
        b = be[st[j]:st[j] + 8 * 130].reshape(130, 8)
        assert (a == b[:, ::-1]).all()
        assert (le[st[j] + 8 * 130:st[j + 1]] == CANARY).all()


@pytest.mark.parametrize("stamp", [10, -(1 << 63) + 12345])
def test_stamp(ctx, corpus, stamp):
    check(ctx, [ln for ln, _, _ in corpus[:70]], stamp=stamp)
    check(ctx, [ln for ln, _, _ in corpus[:70]], stamp=stamp, flags=_lib.YSB_COL_JAVA_ORDER)


def test_decode_leaves_the_counting_state_alone(corpus):
    ads, camp = gd.ad_arrays()
    raw, offs = gd.events("gen_s7")
    with YsbContext(**SMALL) as c:
        c.load_ad_map(ads, camp)
        c.submit(raw, offs)
        before = (c.drain_buckets(), c.stats(), c.ring_range())
        assert before[1]["events"] == 1500 and before[0]
        check(c, [ln for ln, _, _ in corpus[:300]])
        assert (c.drain_buckets(), c.stats(), c.ring_range()) == before


def test_decode_without_an_ad_map(corpus):
    with YsbContext(**SMALL) as c:
        info, _ = check(c, [ln for ln, _, _ in corpus[:64]])
        assert c.stats()["events"] == 0 and c.stats()["batches"] == 0


def test_more_events_than_rows_is_a_capacity_error(ctx):
    lines = fixture_lines("gen_s7")[:65]
    with pytest.raises(YsbError) as e:
        decode(ctx, lines, batch_rows=64)
    assert e.value.code == -4
    data, offs = cm.pack(lines)
    total = columns_layout(64)["start"][8]
    image = np.full(total, CANARY, dtype=np.uint8)
    d_b, d_o, d_out = ctx.device_alloc(data.size), ctx.device_alloc(4 * 65), ctx.device_alloc(total)
    try:
        ctx.h2d(d_b, data)
        ctx.h2d(d_o, offs)
        ctx.h2d(d_out, image)
        with pytest.raises(YsbError):
            ctx.decode_columns_device(d_b, data.size, d_o, 65, d_out, 64)
        assert (ctx.d2h(np.zeros(total, dtype=np.uint8), d_out) == CANARY).all()
    finally:
        for p in (d_b, d_o, d_out):
            ctx.device_free(p)


def test_argument_errors(ctx):
    d = ctx.device_alloc(8192 * 9)
    try:
        for args in ((d, 0, d, 0, d, 0), (d, 0, d, 0, d, 1 << 31), (d + 4, 0, d, 0, d, 64), (d, 0, d, 0, d + 8, 64),
                     (d, 0, d, 0, 0, 64)):
            with pytest.raises(YsbError) as e:
                ctx.decode_columns_device(*args)
            assert e.value.code == -1
        with pytest.raises(YsbError):
            ctx.decode_columns_device(d, 0, d, 0, d, 64, flags=2)
        info = ctx.decode_columns_device(d, 0, d, 0, d, 64)   # an empty batch writes nothing
        assert info["rows"] == 0 and info["valid"] == 0 and info["fast_rows"] == 0
    finally:
        ctx.device_free(d)


def test_decode_columns_convenience(ctx, corpus):
    lines = [ln for ln, _, _ in corpus[:100]]
    data, offs = cm.pack(lines)
    image, valid, info = ctx.decode_columns(data, offs, batch_rows=128)
    want, wvalid, counts = cm.build(lines, batch_rows=128)
    assert (image == want).all() and (valid == wvalid).all() and valid.dtype == np.bool_
    assert info["valid"] == counts["valid"] == int(valid.sum())
