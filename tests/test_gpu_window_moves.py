"""GPU: one list of views whose buckets make the per-workgroup LDS window start, move forwards,
meet views behind it and end on its final flush -- through all three counting front ends: JSON
lines (ysb_submit), a seven-column image (ysb_submit_columns_device) and an Arrow record batch
(ysb_submit_arrow).  Every front end's cells equal the oracle's, and one another's.

At these sizes (five tiles, three tiles) the launches give every tile a workgroup of its own, so
on the GPU each workgroup steps one tile: what runs is each tile's first step (no window yet: ring
adds and a request) and the out-of-ring cell, in contexts with windows of 16 and of 2 buckets.
The same tiles stepped one after the other by one window are tests/native/window_logic.cpp's
model, and a workgroup walking several tiles on the GPU is test_gpu_arrow.py::test_wrap."""
import numpy as np
import pytest

import arrow_model as am
import colcount_model as ccm
import golden_data as gd
from oracle import oracle
from ysb_amd import YsbContext

pytestmark = pytest.mark.gpu

SLOTS = dict(max_batch_events=1 << 12, max_batch_bytes=1 << 20, overflow_capacity=1 << 10)


def tiled_buckets():
    """263 views, four full 64-row tiles and a 7-row one, for a window of 16 buckets in a ring of
    buckets 0..63:
    tile 0: buckets 0..3 -- no window yet: ring adds and the first request (3: the window -4..11);
    tile 1: buckets 2..9 -- all inside the re-centred window;
    tile 2: buckets 20..40 and a few at 5 -- ahead of the window and inside it in one tile; the
            second request (40: the window 33..48);
    tile 3: buckets 30..45 -- some inside the new window, 30..32 behind it (no request);
    tile 4: 35..39 and 47, which only the final flush brings out, and 70, outside the ring."""
    b = [r % 4 for r in range(64)]
    b += [2 + r % 8 for r in range(64)]
    b += [5 if r % 16 == 3 else 20 + r % 21 for r in range(64)]
    b += [30 + r % 16 for r in range(64)]
    b += [35, 36, 37, 70, 38, 39, 47]
    return b


def walking_buckets():
    """130 views walking buckets 0..15 one by one, for the smallest window (two buckets, where the
    re-centred base is the request itself)."""
    return [r * 16 // 130 for r in range(130)]


@pytest.fixture(scope="module")
def world():
    class W:
        pass
    w = W()
    w.ads, w.camp = gd.ad_arrays()
    w.keys = [a.encode() for a in w.ads]
    return w


def three_ways(world, camp, buckets, n_campaigns, window_ring, lds_count):
    """The views (ad r of the fixture, bucket buckets[r]) through the three front ends, each in a
    context of its own: [(cells, stats, lds_counters or None)], and the oracle's (cells, stats)."""
    n = len(buckets)
    rows = [(world.keys[(7 * r) % len(world.keys)], b"view", str(bk * 10000 + r % 10000).encode()) for r, bk in enumerate(buckets)]
    batch = am.encode(rows, "strings")
    lines, formless = am.render_json(batch)
    assert formless == 0 and len(lines) == n
    raw = np.frombuffer(b"".join(lines), dtype=np.uint8)
    offs = np.cumsum([0] + [len(x) for x in lines[:-1]]).astype(np.uint32)
    image = ccm.make_image([r[0] for r in rows], [r[1] for r in rows], [int(r[2]) for r in rows], n)
    want = oracle.run(oracle.AdMap(world.ads, camp), raw, offs)

    def json_lines(c):
        c.submit(raw, offs)
        return None

    def columns(c):
        d = c.device_alloc(image.size)
        try:
            c.h2d(d, image)
            c.submit_columns_device(d, n, n, 0)
            c.sync()
        finally:
            c.device_free(d)
        return c.columns_launch_info()["lds_counters"]

    def arrow(c):
        c.submit_arrow(am.to_node(batch), slot=0)
        return c.arrow_launch_info()["lds_counters"]

    out = []
    for submit in (json_lines, columns, arrow):
        with YsbContext(n_campaigns=n_campaigns, window_ring=window_ring, ring_base_bucket=0, lds_count=lds_count, **SLOTS) as c:
            c.load_ad_map(world.ads, camp)
            lds = submit(c)
            out.append((c.drain_buckets(), c.stats(), lds))
    return out, want


@pytest.mark.parametrize("lds_count", [True, False])
def test_window_moves_through_all_front_ends(world, lds_count):
    """lds_count False is the control: the same cells without any window."""
    buckets = tiled_buckets()
    assert len(buckets) == 263
    camp = [i % 10 for i in range(len(world.ads))]
    got, (cells, ost) = three_ways(world, camp, buckets, 10, 64, lds_count)
    assert ost["joined"] == 263 and sum(cells.values()) == 263 and {b for _, b in cells} == set(buckets)
    for g, st, lds in got:
        assert g == cells
        assert lds in (None, 1 if lds_count else 0)   # 10 campaigns, ring 64: a window of 16 buckets
        assert st["events"] == st["views"] == st["joined"] == 263
        assert st["out_of_ring"] == 1 and st["overflow_dropped"] == 0
    assert got[0][0] == got[1][0] == got[2][0]


def test_smallest_window_walks_its_ring(world):
    """100 campaigns in a ring of 16: a window of two buckets."""
    buckets = walking_buckets()
    assert len(buckets) == 130 and sorted(set(buckets)) == list(range(16))
    got, (cells, ost) = three_ways(world, world.camp, buckets, 100, 16, True)
    assert ost["joined"] == 130
    for g, st, lds in got:
        assert g == cells
        assert lds in (None, 1)
        assert st["joined"] == 130 and st["out_of_ring"] == 0 and st["overflow_dropped"] == 0
    assert got[0][0] == got[1][0] == got[2][0]
