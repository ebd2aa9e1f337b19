"""CPU: the plain model of record-mode counting (tests/records_model.py) against the plain Counter
of its inputs and the C oracle on the rendered bytes, for every geometry the GPU tests run
(tests/test_gpu_record_geometry.py), and its u8 byte / u64 ring / dirty sequence on hand-written
cases around 255."""
import numpy as np
import pytest

import records_corpus as rc
import records_model as rm
from oracle import oracle
from ysb_amd import GenParams

# (campaigns, ring) -> (level-2 blocks, S, bins): the plans of the GPU geometry corpus
GEOS = {(129, 16): (1, 1, 1), (2049, 16): (2, 1, 2), (16384, 16): (8, 1, 8), (16385, 16): (9, 2, 5),
        (200001, 16): (98, 16, 7), (1000, 1024): (32, 4, 8), (300, 32768): (300, 64, 5),
        (2048, 32768): (2048, 256, 8)}
CUS = 256
COUNTERS = ("events", "views", "joined", "join_misses", "parse_errors", "time_errors")


@pytest.fixture(scope="module")
def writer():
    g = GenParams(n_campaigns=2000, ads_per_campaign=2)
    ads = g.ids_packed()[1]
    return rc.LineWriter(g, ads)


def camp_map(n_ads, n_map, C):
    f = np.arange(n_ads, dtype=np.int64) * C // n_ads if C > n_ads else np.arange(n_ads, dtype=np.int64) % C
    f[0], f[n_map // 2], f[n_map - 1] = 0, C // 2, C - 1
    return f


def test_plan_of_restates_the_geometries():
    for (C, W), (blocks, S, bins) in GEOS.items():
        p = rm.plan_of(C, W, 313, 1)
        assert (p["n_blocks"], 1 << p["sub_log2"], p["bins"]) == (blocks, S, bins), (C, W, p)
        assert p["cap"] == (64 if bins == 1 else 32) and (1 << p["blk_shift"]) * W == rm.REC_BLOCK_CELLS
    assert rm.plan_of(200, 65536, 64, 1) is None                    # W > REC_BLOCK_CELLS
    assert rm.plan_of(4096, 32768, 64, 1)["sub_log2"] == 9 and rm.plan_of(4097, 32768, 64, 1) is None
    assert rm.plan_of(200000, 16, 8192, 3) and rm.plan_of(200000, 16, 8193, 3) is None


def test_tile_split_and_slices():
    for segs, grid in (([64 * 16], 16), ([6400], 100), ([1, 65, 64 * 7 + 1], 5), ([64 * 2048 * 3 + 1], 2048),
                       ([100, 7000, 3], 2048), ([64 * 300], 7)):
        wg = rm.tile_split(segs, grid)
        assert wg.size == sum(segs) and wg.min() >= 0 and wg.max() < grid
        pos = 0
        for n in segs:
            w = wg[pos:pos + n]
            pos += n
            assert (np.diff(w) >= 0).all()                           # a workgroup's tiles are consecutive
            q, r = divmod(rm.n_tiles(n), grid)
            tiles = np.bincount(w[::64], minlength=grid)             # the first line of every tile
            assert (tiles == np.where(np.arange(grid) < r, q + 1, q)).all()
        sl = rm.slice_of_wg(grid)
        assert (np.diff(sl) >= 0).all() and sl.max() < rm.REC_QUARTERS
        for q in range(rm.REC_QUARTERS):
            lo, hi = q * grid // rm.REC_QUARTERS, (q + 1) * grid // rm.REC_QUARTERS
            assert (np.flatnonzero(sl == q) == np.arange(lo, hi)).all()
    assert rm.grid_of([64 * 16], CUS) == 16 and rm.grid_of([64 * 2048 * 3 + 1], CUS) == 2048
    assert rm.grid_of([64 * 2048 * 129], CUS) == 4096                # a second round of resident workgroups
    assert rm.tiles_per_wg_max([64 * 2048 * 3 + 1], 2048) == 4 and rm.tiles_per_wg_max([64, 6400, 64 * 4096], 2048) == 4


@pytest.mark.parametrize("base", [rc.BUCKET_1E12 - 2, -5])
@pytest.mark.parametrize("geo", sorted(GEOS))
def test_model_table_equals_counter_and_oracle(writer, geo, base):
    C, W = geo
    n_ads, n_map = writer.ads.shape[0], writer.ads.shape[0] - 16
    f = camp_map(n_ads, n_map, C)
    rng = np.random.default_rng(C * 31 + W)
    cor = rc.geometry_corpus(rng, 5000, C, n_ads, n_map, base, W, f)
    raw, offs = writer.render(cor.ad, cor.etype, cor.t)
    exp = cor.expected()
    ads_str = lambda i: bytes(writer.ads[i]).decode()
    rows, ost = oracle.run(oracle.AdMap(*cor.oracle_map(ads_str)), raw, offs, divisor=rc.DIVISOR)
    assert rows == exp
    for k, v in cor.stats().items():
        assert ost[k] == v, (k, ost[k], v)
    assert min(b for _, b in exp) < base and max(b for _, b in exp) >= base + W
    if base < 0:
        assert any(b < 0 for _, b in exp)
    # one launch; three segments in one launch; two launches with a clearing drain between
    cuts = [0, 1700, 1700 + 3001, len(cor)]
    for segs in ([len(cor)], [b - a for a, b in zip(cuts, cuts[1:])]):
        grid = rm.grid_of(segs, CUS)
        plan = rm.plan_of(C, W, grid, rm.tiles_per_wg_max(segs, grid))
        m = rm.RecordsModel(C, W, base)
        L = m.launch(cor.camp, cor.bucket, plan, segs)
        assert m.table() == exp
        assert L.views.sum() == L.rec_n.sum() + L.fallback == L.total.sum() + L.fallback
        outside = int(((cor.camp >= 0) & ((cor.bucket < base) | (cor.bucket >= base + W))).sum())
        assert 20 < L.outside == outside and L.views.sum() + L.outside == cor.stats()["joined"]
        assert L.dirty == (1 if L.fallback else 0) and L.spills == 0
    m = rm.RecordsModel(C, W, base)
    got = {}
    for a, b in ((0, 2048), (2048, len(cor))):
        grid = rm.grid_of([b - a], CUS)
        m.launch(cor.camp[a:b], cor.bucket[a:b], rm.plan_of(C, W, grid, rm.tiles_per_wg_max([b - a], grid)), [b - a])
        for k, v in m.table().items():
            got[k] = got.get(k, 0) + v
        m.clear()
    assert got == exp and m.table() == {}


def one_cell(m, plan, n, campaign=3, bucket=7, others=()):
    """A launch of n views of one cell (and `others`: (campaign, bucket, n) triples)."""
    camp = [campaign] * n
    buck = [bucket] * n
    for c, b, k in others:
        camp += [c] * k
        buck += [b] * k
    return m.launch(camp, buck, plan, [len(camp)])


def test_add16_sequences_by_hand():
    C, W = 129, 16
    plan = rm.plan_of(C, W, 64, 128)      # a capacity no case below reaches: every view a record
    assert plan["cap"] >= 70_000 * 3 // 4 // 64
    cell = 3 * W + 7

    def state(m):
        return m.byte.get(cell, 0), m.ring[cell], m.dirty
    # 254, then 1, 1, 1: the byte reaches 255 and stays; 256 spills the whole sum; then 1 on a
    # ring cell that is already non-zero
    m = rm.RecordsModel(C, W, 0)
    seq = []
    for n in (254, 1, 1, 1):
        one_cell(m, plan, n)
        seq.append(state(m))
    assert seq == [(254, 0, 0), (255, 0, 0), (0, 256, 1), (1, 256, 1)]
    assert m.table() == {(3, 7): 257}
    # 255 in one launch stays in the byte, 256 does not
    m = rm.RecordsModel(C, W, 0)
    one_cell(m, plan, 255)
    assert state(m) == (255, 0, 0)
    m = rm.RecordsModel(C, W, 0)
    L = one_cell(m, plan, 256)
    assert state(m) == (0, 256, 1) and L.spills == 1
    # 255 + 255
    m = rm.RecordsModel(C, W, 0)
    one_cell(m, plan, 255)
    one_cell(m, plan, 255)
    assert state(m) == (0, 510, 1) and m.table() == {(3, 7): 510}
    # 200 + 200 + 200: without a fold the second launch spills, with one after the first the third
    m = rm.RecordsModel(C, W, 0)
    seq = []
    for _ in range(3):
        one_cell(m, plan, 200)
        seq.append(state(m))
    assert seq == [(200, 0, 0), (0, 400, 1), (200, 400, 1)]
    m = rm.RecordsModel(C, W, 0)
    one_cell(m, plan, 200)
    m.fold()
    assert state(m) == (0, 200, 0)
    seq = []
    for _ in range(2):
        one_cell(m, plan, 200)
        seq.append(state(m))
    assert seq == [(200, 200, 0), (0, 600, 1)] and m.table() == {(3, 7): 600}
    # 70,000 in one launch, neighbours untouched by the spill
    m = rm.RecordsModel(C, W, 0)
    one_cell(m, plan, 70_000, others=[(3, 6, 5), (3, 8, 5)])
    assert state(m) == (0, 70_000, 1) and m.byte == {cell - 1: 5, cell + 1: 5}
    assert m.table() == {(3, 7): 70_000, (3, 6): 5, (3, 8): 5}
    # a negative ring base: slot -> bucket of [base, base + W)
    m = rm.RecordsModel(C, W, -5)
    one_cell(m, plan, 3, bucket=-5, others=[(3, 10, 2), (3, 11, 4), (3, -6, 1)])
    assert m.table() == {(3, -5): 3, (3, 10): 2, (3, 11): 4, (3, -6): 1}
    assert m.cell_of(3, -5) == 3 * W + 11 and m.cell_of(3, 10) == 3 * W + 10


def test_capacity_fallback_and_dense_rule_by_hand():
    C, W = 2049, 16
    # one tile per workgroup over two bins: cap 32
    plan = rm.plan_of(C, W, 4, 1)
    assert plan["cap"] == 32 and plan["bins"] == 2 and plan["n_blocks"] == 2
    m = rm.RecordsModel(C, W, 0)
    camp = [5] * 33 + [None] * 31 + [2048] + [7] * 32 + [None] * 31 + [9] * 128
    L = m.launch(camp, [1] * len(camp), plan, [len(camp)])
    assert L.views.tolist() == [[33, 0], [32, 1], [64, 0], [64, 0]]
    assert L.rec_n.tolist() == [[32, 0], [32, 1], [32, 0], [32, 0]] and L.fallback == 1 + 32 + 32
    assert L.dirty == 1 and not L.ambiguous
    assert L.total.tolist() == [128, 1]
    assert L.dense.tolist() == [False, True]          # 128 * 16 < 32768 cells; 1 * 16 >= 16 cells
    assert m.table() == {(5, 1): 33, (2048, 1): 1, (7, 1): 32, (9, 1): 128}
    # the dense rule at its edge: 2047 records in 32768 cells sparse, 2048 dense
    plan = rm.plan_of(C, W, 64, 128)
    for n, dense in ((2047, False), (2048, True)):
        m = rm.RecordsModel(C, W, 0)
        L = m.launch([i % 2048 for i in range(n)], [0] * n, plan, [n])
        assert L.fallback == 0 and L.total.tolist() == [n, 0] and L.dense.tolist() == [dense, False]
