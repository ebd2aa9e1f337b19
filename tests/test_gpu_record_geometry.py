"""GPU: record-mode counting (csrc/ysb_count.hip, the REC staging of ysb_scan.hip, csrc/ysb_recplan.h)
across its geometry and at u8 saturation -- one to eight level-1 bins, one to 256 blocks per
bin, rings of 16 to 32,768 slots, last blocks of one campaign, grids below the slice count,
full sub-buffers, the partition's direct store, the dense / sparse boundary and delta cells at
exactly 254 .. 257 -- with proof from ysb_record_info of which path ran: the plan, the records
each (workgroup, bin) sub-buffer kept, the runs per (block, slice) and the dirty flag, all equal
to the plain model (tests/records_model.py).

The lines are written by the test (tests/records_corpus.py: generator lines as carriers), so
each cell's count is known by construction; every case compares the drain with that Counter, with
the model and with the C oracle on the same bytes.  One ad list for the module (400,000 ads, the
smallest map with the bucket-layout join table), re-mapped per case with campaign = ad mod C."""
from collections import Counter

import numpy as np
import pytest

import records_corpus as rc
import records_model as rm
from oracle import oracle
from ysb_amd import GenParams, YsbContext, YsbError

pytestmark = pytest.mark.gpu

COUNTERS = ("events", "views", "joined", "join_misses", "parse_errors", "time_errors")
N_ADS = 400_000
N_MAP = N_ADS - 16            # the last 16 ads stay out of the map: join misses
Q = rm.REC_QUARTERS
POS, NEG = rc.BUCKET_1E12 - 2, -5     # ring bases: 13-digit times, and a ring straddling bucket 0


class World:
    def __init__(self):
        g = GenParams(n_campaigns=200_000, ads_per_campaign=2)
        self.ads = g.ids_packed()[1].reshape(-1, 36)
        assert self.ads.shape[0] == N_ADS
        self.writer = rc.LineWriter(g, self.ads)
        self.idx = np.arange(N_ADS, dtype=np.int64)

    def ad_str(self, i):
        return bytes(self.ads[i]).decode()


@pytest.fixture(scope="module")
def world():
    return World()


class Case:
    """One context of C campaigns x W ring slots with campaign = ad mod C, its model, and the
    sums of what its launches must count to."""

    def __init__(self, world, C, W, base, record=True):
        self.w, self.C, self.W, self.base = world, C, W, base
        self.f = world.idx % C
        self.ctx = YsbContext(n_campaigns=C, window_ring=W, ring_base_bucket=base, record_count=record,
                              max_batch_bytes=1 << 20, max_batch_events=1 << 12)
        self.ctx.load_ad_map_packed(world.ads[:N_MAP].reshape(-1), self.f[:N_MAP].astype(np.uint32))
        self.start()

    def start(self):
        self.model = rm.RecordsModel(self.C, self.W, self.base)
        self.exp, self.rows, self.ost, self.outside = Counter(), Counter(), Counter(), 0

    def reset(self):
        self.ctx.reset()
        self.start()

    def close(self):
        self.ctx.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def corpus(self, camp, bucket, seed=1):
        """Lines given per line as (campaign or -1, bucket): a view of ad `campaign`, or a click."""
        camp, bucket = np.asarray(camp, dtype=np.int64), np.asarray(bucket, dtype=np.int64)
        k = np.random.default_rng(seed).integers(0, rc.DIVISOR, camp.size)
        return rc.Corpus(np.maximum(camp, 0), np.where(camp >= 0, rc.VIEW, rc.CLICK), rc.time_in_bucket(bucket, k),
                         self.f, N_MAP)

    def submit(self, cor, seg_lines, carrier=None, rendered=None):
        """Renders the corpus (or takes its rendered bytes), uploads it and launches its segments in
        one launch; the buffers to free."""
        ctx = self.ctx
        raw, offs = rendered if rendered is not None else self.w.writer.render(cor.ad, cor.etype, cor.t, carrier)
        n = offs.size
        cuts = np.concatenate([[0], np.cumsum(seg_lines)]).astype(np.int64)
        assert cuts[-1] == n
        d_b, d_o = ctx.device_alloc(raw.size + 64 * len(seg_lines) + 64), ctx.device_alloc(4 * n + 64)
        segs, pos = [], 0
        for a, b in zip(cuts[:-1].tolist(), cuts[1:].tolist()):
            lo = int(offs[a])
            hi = int(offs[b]) if b < n else raw.size
            ctx.h2d(d_b + pos, raw[lo:hi])
            ctx.h2d(d_o + 4 * a, (offs[a:b] - lo).astype(np.uint32))
            segs.append((d_b + pos, hi - lo, d_o + 4 * a, b - a))
            pos += (hi - lo + 15) // 16 * 16
        if len(segs) == 1:
            ctx.submit_device(*segs[0])
        else:
            ctx.submit_device_segments(segs)
        # what this launch must add: by construction, and by the oracle on the same bytes
        self.exp.update(cor.expected())
        rows, ost = oracle.run(oracle.AdMap(*cor.oracle_map(self.w.ad_str)), raw, offs, divisor=rc.DIVISOR, threads=8)
        self.rows.update(rows)
        self.ost.update(ost)
        return d_b, d_o

    def launch(self, cor, seg_lines=None, arrays=True, carrier=None, rendered=None):
        """One record-mode launch and its evidence: (descriptor, rec_n, runs, the model's Launch)."""
        ctx = self.ctx
        seg_lines = [len(cor)] if seg_lines is None else list(seg_lines)
        before = ctx.path_time()[2]
        bufs = self.submit(cor, seg_lines, carrier, rendered)
        desc, rec_n, runs = ctx.record_info(arrays=arrays)       # (waits for the launch)
        for p in bufs:
            ctx.device_free(p)
        info = ctx.launch_info()
        assert ctx.path_time()[2] == before + 1, "the launch did not run in record mode"
        assert info == {"layout": 0, "record_mode": 1, "hbm_table": 1, "tbl": 0}, info
        L = self.model.launch(cor.camp, cor.bucket, desc, seg_lines)
        self.outside += L.outside
        assert desc["grid"] == max(1, min(max(rm.n_tiles(n) for n in seg_lines), desc["grid"]))
        assert desc["cap"] == rm.plan_of(self.C, self.W, desc["grid"], rm.tiles_per_wg_max(seg_lines, desc["grid"]))["cap"]
        if arrays:
            assert np.array_equal(rec_n, L.rec_n), "records kept per (workgroup, bin)"
            check_runs(desc, runs, L)
        assert desc["dirty"] == L.dirty, (desc["dirty"], L.dirty, L.fallback, L.spills)
        return desc, rec_n, runs, L

    def check_counts(self, what, clear=False):
        """The drain against the construction Counter, the model and the oracle; then every counter."""
        got = self.ctx.drain_buckets(clear=clear)
        st = self.ctx.stats()
        exp = dict(self.exp)
        if got != exp:
            diff = sorted(k for k in set(got) | set(exp) if got.get(k) != exp.get(k))
            raise AssertionError("%s: %d cells differ (campaign, bucket): gpu / expected: %s" % (
                what, len(diff), ", ".join("%r: %r / %r" % (k, got.get(k), exp.get(k)) for k in diff[:12])))
        assert got == self.model.table(), what
        assert got == dict(self.rows), what
        for k in COUNTERS:
            assert st[k] == self.ost[k], (what, k, st[k], self.ost[k])
        assert st["deferred"] == 0 and st["overflow_dropped"] == 0 and st["out_of_ring"] == self.outside, (what, st)
        if clear:
            self.model.clear()
            self.exp, self.rows = Counter(), Counter()
        return st


def check_runs(desc, runs, L):
    """The partition's runs: lengths equal to the model's (per block where the model can tell
    which records a full sub-buffer kept, per bin otherwise); every offset 32-aligned inside its
    (bin, slice) area, no two runs overlapping, the last one ending inside the area."""
    S, bins, area, n_blocks = 1 << desc["sub_log2"], desc["bins"], desc["area"], desc["n_blocks"]
    assert runs.shape == (n_blocks, Q, 2) and desc["slices"] == Q
    length = runs[:, :, 1].astype(np.int64)
    if not L.ambiguous:
        assert np.array_equal(length, L.run_len), "run length per (block, slice)"
    for b in range(bins):
        blk = slice(b * S, min((b + 1) * S, n_blocks))
        assert np.array_equal(length[blk].sum(axis=0), L.run_len[blk].sum(axis=0)), "records per (bin, slice)"
        start = runs[blk, :, 0].astype(np.int64) - (b * Q + np.arange(Q, dtype=np.int64)) * area
        ln = length[blk]
        order = np.argsort(start, axis=0, kind="stable")
        start, ln = np.take_along_axis(start, order, 0), np.take_along_axis(ln, order, 0)
        end = start + (ln + 31) // 32 * 32
        assert (start % 32 == 0).all() and (start >= 0).all()
        assert (start[1:] >= end[:-1]).all(), "runs overlap"
        assert (end[-1] <= area).all() and (start + ln <= area).all(), "a run ends past its area"
    assert desc["part"] == bins * Q * area


def plan_line(desc):
    return "L2C %d blocks %d S %d bins %d cap %d grid %d area %d" % (
        1 << desc["blk_shift"], desc["n_blocks"], 1 << desc["sub_log2"], desc["bins"], desc["cap"], desc["grid"],
        desc["area"])


# -- a. the geometry corpus --------------------------------------------------------------------

# (campaigns, ring) -> (L2C, level-2 blocks, S, bins, campaigns of the last block)
GEOS = [((129, 16), (2048, 1, 1, 1, 129)), ((2049, 16), (2048, 2, 1, 2, 1)), ((16384, 16), (2048, 8, 1, 8, 2048)),
        ((16385, 16), (2048, 9, 2, 5, 1)), ((200001, 16), (2048, 98, 16, 7, 1345)), ((1000, 1024), (32, 32, 4, 8, 8)),
        ((300, 32768), (1, 300, 64, 5, 1)), ((2048, 32768), (1, 2048, 256, 8, 1))]


@pytest.mark.parametrize("k", range(len(GEOS)), ids=["%dx%d" % g[0] for g in GEOS])
def test_geometry_corpus(world, k):
    (C, W), (l2c, blocks, S, bins, last) = GEOS[k]
    base = NEG if k % 2 else POS
    rng = np.random.default_rng(1000 + k)
    with Case(world, C, W, base) as case:
        cor = rc.geometry_corpus(rng, 20_000, C, N_ADS, N_MAP, base, W, case.f)
        assert {0, C - 1} <= set(cor.camp.tolist()) and (cor.bucket[cor.camp >= 0] < base).any()
        if base < 0:
            assert (cor.t < 0).any() and (cor.bucket[cor.camp >= 0] < 0).any()
        ways = []
        # one launch
        desc, rec_n, runs, L = case.launch(cor)
        assert (1 << desc["blk_shift"], desc["n_blocks"], 1 << desc["sub_log2"], desc["bins"]) == (l2c, blocks, S, bins)
        assert C - (blocks - 1) * l2c == last and 1 << desc["w_log2"] == W
        assert desc["grid"] == 313 and desc["cap"] == (64 if bins == 1 else 32)
        # (2049 x 16 keeps 32 of a workgroup's ~57 views of bin 0: the rest fall back)
        assert not L.ambiguous and L.total.sum() > 9_000 and L.total[-1] > 0
        assert L.total.sum() + L.fallback + L.outside == cor.stats()["joined"]
        ways.append(("1 launch", desc, L))
        case.check_counts("%dx%d one launch" % (C, W))
        # three segments in one launch
        case.reset()
        desc, rec_n, runs, L = case.launch(cor, [6000, 7001, 6999])
        assert desc["grid"] == 110 and desc["n_blocks"] == blocks
        ways.append(("3 segments", desc, L))
        case.check_counts("%dx%d three segments" % (C, W))
        # two launches with a clearing drain between
        case.reset()
        desc, rec_n, runs, L = case.launch(cor.part(0, 8000))
        case.check_counts("%dx%d first of two launches" % (C, W), clear=True)
        desc, rec_n, runs, L2 = case.launch(cor.part(8000, len(cor)))
        ways.append(("2 launches", desc, L2))
        case.check_counts("%dx%d second of two launches" % (C, W), clear=True)
        assert case.ctx.drain_buckets() == {}
    for name, d, l in ways:
        print("geometry %dx%d base %d %s: %s | records %d fallback %d (ambiguous %s) outside %d dense blocks %d/%d dirty %d"
              % (C, W, base, name, plan_line(d), l.total.sum(), l.fallback, l.ambiguous, l.outside,
                 int(l.dense.sum()), blocks, l.dirty))


# -- b. sub-buffer capacity ----------------------------------------------------------------------

def all_views(case, n_lines, rng, bin_of_tile=None, shift=0):
    """n_lines in-ring joined views: campaigns over the whole table, or (bin_of_tile) every tile's
    views in one bin, tile t in bin t mod bins."""
    if bin_of_tile is None:
        camp = rng.integers(0, case.C, n_lines)
    else:
        tile = np.arange(n_lines) // rm.TILE_LINES
        camp = ((tile % bin_of_tile) << shift) + rng.integers(0, 1 << shift, n_lines)
    return case.corpus(camp, case.base + rng.integers(0, 12, n_lines))


@pytest.mark.parametrize("shape", [(129, 16), (16384, 16)], ids=["1bin", "8bins"])
def test_sub_buffer_capacity(world, shape):
    C, W = shape
    bins = 1 if C == 129 else 8
    rng = np.random.default_rng(7 + C)
    report = []
    with Case(world, C, W, POS) as case:
        big = all_views(case, (2048 * 3 + 1) * 64, rng, None if bins == 1 else bins, 11)
        # (one carrier: lines of one length, so a prefix of the rendered bytes is a batch)
        raw, offs = world.writer.render(big.ad, big.etype, big.t, np.zeros(len(big), dtype=np.int64))
        width = int(offs[1])

        def prefix(n):
            return raw[:n * width], offs[:n]
        # one bin: every line of a workgroup in its one sub-buffer; eight bins: each tile's 64 views
        # in one bin of cap 32
        for tiles in (16, 100, 2048 * 3, 2048 * 3 + 1):
            case.reset()
            cor = big.part(0, tiles * 64)
            desc, rec_n, runs, L = case.launch(cor, rendered=prefix(len(cor)))
            assert desc["bins"] == bins and desc["grid"] == min(tiles, 2048)
            in_ring = int((cor.camp >= 0).sum())
            assert in_ring == tiles * 64 and L.outside == 0
            assert (rec_n == desc["cap"]).any(), "no sub-buffer reached its capacity"
            fallback = in_ring - int(rec_n.sum())
            assert fallback == L.fallback and desc["dirty"] == (1 if fallback else 0)
            # (one tile per workgroup over one bin: cap 64 = the tile's lines, nothing falls back)
            assert (fallback > 0) == (bins > 1 or tiles > 2048)
            report.append((tiles, plan_line(desc), int((rec_n == desc["cap"]).sum()), fallback, desc["dirty"]))
            case.check_counts("%dx%d %d tiles" % (C, W, tiles))
        # the four batches as segments of one launch: every workgroup past its capacity
        case.reset()
        segs = [16 * 64, 100 * 64, 2048 * 64, 2049 * 64]
        cor = big.part(0, sum(segs))
        desc, rec_n, runs, L = case.launch(cor, segs, rendered=prefix(len(cor)))
        assert desc["grid"] == 2048 and L.fallback > 0 and (rec_n == desc["cap"]).any() and desc["dirty"] == 1
        report.append(("4 segments", plan_line(desc), int((rec_n == desc["cap"]).sum()), L.fallback, desc["dirty"]))
        case.check_counts("%dx%d four segments" % (C, W))
        if bins == 8:
            # exactly cap, then cap + 1 records in one (workgroup, bin): lines placed by the model's split
            for extra, (w, b) in ((0, (3, 2)), (1, (5, 4))):
                case.reset()
                n = 16 * 64
                wg = rm.tile_split([n], 16)
                camp = np.full(n, -1, dtype=np.int64)
                mine = np.flatnonzero(wg == w)
                camp[mine[:32 + extra]] = (b << 11) + rng.integers(0, 2048, 32 + extra)
                camp[mine[40:50]] = ((b + 1) << 11) + rng.integers(0, 2048, 10)      # another bin, below its cap
                others = np.flatnonzero((wg != w) & (np.arange(n) % 3 == 0))        # ~21 views per workgroup
                camp[others] = rng.integers(0, C, others.size)
                cor = case.corpus(camp, case.base + rng.integers(0, 12, n))
                desc, rec_n, runs, L = case.launch(cor)
                assert desc["cap"] == 32 and rec_n[w, b] == 32 and L.views[w, b] == 32 + extra
                assert L.fallback == extra == int((cor.camp >= 0).sum()) - int(rec_n.sum()) and desc["dirty"] == extra
                report.append(("cap + %d" % extra, plan_line(desc), int((rec_n == 32).sum()), L.fallback, desc["dirty"]))
                case.check_counts("%dx%d cap + %d" % (C, W, extra))
    for r in report:
        print("capacity %dx%d %s: %s | sub-buffers at cap %d fallback %d dirty %d" % ((C, W) + r))


# -- c. partition shapes ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape,n_segs", [((16385, 16), 4), ((1000, 1024), 6)], ids=["S2", "S4"])
def test_partition_shapes(world, shape, n_segs):
    """n_segs segments of 128 tiles in one launch: 128 workgroups of n_segs tiles (cap 64), two per
    slice.  Slice 1 (workgroups 2 and 3) holds runs of exactly 31, 32, 33, 64 and 65 records, an
    empty block, and one sub-buffer with 40 records of one block: the partition wave that reads
    it claims positions 0 .. 39 of that block in one round, so 32 .. 39 take the direct store."""
    C, W = shape
    G = 128
    rng = np.random.default_rng(C)
    with Case(world, C, W, NEG) as case:
        plan = rm.plan_of(C, W, G, n_segs)
        S, l2c, bins = 1 << plan["sub_log2"], 1 << plan["blk_shift"], plan["bins"]
        assert plan["cap"] == 64 and S == (2 if C == 16385 else 4)
        n = n_segs * G * 64
        wg = rm.tile_split([G * 64] * n_segs, G)
        camp = np.full(n, -1, dtype=np.int64)
        # the other slices: views on 30 % of the lines, far below 64 per (workgroup, bin)
        other = np.flatnonzero(((wg < 2) | (wg > 3)) & (rng.random(n) < 0.3))
        camp[other] = rng.integers(0, C, other.size)
        # slice 1: per block the records of workgroup 2 and of workgroup 3
        if S == 2:      # bins of blocks {0,1} {2,3} {4,5} {6,7} {8}
            want = {0: (31, 0), 1: (32, 0), 2: (33, 0), 3: (31, 33), 4: (33, 32), 5: (0, 0), 6: (40, 0), 7: (0, 5), 8: (2, 3)}
        else:           # bins of blocks {0..3} {4..7} ...
            want = {0: (31, 0), 1: (32, 0), 2: (0, 0), 3: (0, 33), 4: (33, 31), 5: (0, 33), 8: (33, 32), 9: (0, 0),
                    12: (40, 0), 13: (0, 5), 31: (2, 3)}
        exact = {0: 31, 1: 32, (2 if S == 2 else 3): 33, (3 if S == 2 else 4): 64, (4 if S == 2 else 8): 65,
                 (5 if S == 2 else 9): 0, (6 if S == 2 else 12): 40}
        free = {2: list(rng.permutation(np.flatnonzero(wg == 2))), 3: list(rng.permutation(np.flatnonzero(wg == 3)))}
        for blk, counts in want.items():
            for w, k in zip((2, 3), counts):
                lo, hi = blk * l2c, min((blk + 1) * l2c, C)
                for _ in range(k):
                    camp[free[w].pop()] = rng.integers(lo, hi)
        cor = case.corpus(camp, case.base + rng.integers(0, 12, n))
        desc, rec_n, runs, L = case.launch(cor, [G * 64] * n_segs)
        assert desc["grid"] == G and desc["cap"] == 64 and 1 << desc["sub_log2"] == S
        assert L.fallback == 0 and not L.ambiguous and desc["dirty"] == 0
        for blk, k in exact.items():
            assert runs[blk, 1, 1] == k == L.run_len[blk, 1], (blk, runs[blk, 1], k)
        hot = (6 if S == 2 else 12) // S
        assert rec_n[2, hot] == 40 and L.views[3, hot] == 5
        print("partition %dx%d: %s | slice 1 runs %s | 40 of block %d in sub-buffer (2, %d)" % (
            C, W, plan_line(desc), {b: int(runs[b, 1, 1]) for b in want}, hot * S, hot))
        case.check_counts("%dx%d partition shapes" % (C, W))
        # grids below the slice count and not a multiple of it: most slices hold nobody
        for tiles in (16, 100):
            case.reset()
            nl = tiles * 64
            cam = np.where(rng.random(nl) < 0.4, rng.integers(0, C, nl), -1)
            desc, rec_n, runs, L = case.launch(case.corpus(cam, case.base + rng.integers(0, 12, nl)))
            sl = rm.slice_of_wg(tiles)
            empty = Q - np.unique(sl).size
            assert desc["grid"] == tiles and empty == (48 if tiles == 16 else 0) and not L.ambiguous
            assert (runs[:, np.setdiff1d(np.arange(Q), sl), 1] == 0).all()
            print("partition %dx%d %d tiles: %s | empty slices %d, widest %d, records %d fallback %d" % (
                C, W, tiles, plan_line(desc), empty, np.bincount(sl).max(), L.total.sum(), L.fallback))
            case.check_counts("%dx%d %d tiles" % (C, W, tiles))


# -- d. the dense / sparse boundary ------------------------------------------------------------------

@pytest.mark.parametrize("n_rec", [2047, 2048])
def test_dense_sparse_boundary(world, n_rec):
    """(2049, 16): block 0 has 32,768 cells, so 2,048 records make it dense and 2,047 leave it
    sparse; block 1 is one campaign's 16 cells and dense with a single record.  An earlier launch
    left counts in delta lines the second launch does not touch, in lines it touches and in the
    vectors next to the ones it adds to: all of them survive."""
    C, W = 2049, 16
    rng = np.random.default_rng(n_rec)
    with Case(world, C, W, POS) as case:
        # first launch: 4 views each in cells of campaigns 8 .. 15 (a 128-B delta line the second
        # launch leaves alone), 16 .. 17 (a line it adds to) and 2047, plus one in block 1
        c1 = np.repeat([8, 11, 15, 16, 17, 2047, 2048], 4)
        b1 = case.base + np.repeat([0, 3, 15, 7, 9, 15, 4], 4)
        first = np.full(2 * 64, -1, dtype=np.int64)
        fb = np.zeros(2 * 64, dtype=np.int64)
        first[:c1.size], fb[:c1.size] = c1, b1
        desc, _, _, L = case.launch(case.corpus(first, fb))
        assert L.total.tolist() == [24, 4] and L.dense.tolist() == [False, True]
        # second launch: 64 tiles of 32 views (cap 32, nothing falls back), n_rec of them in block 0
        # on distinct cells of campaigns 18 .. 2040 except line 1 (campaigns 8 .. 15), one in block 1
        n = 64 * 64
        camp = np.full(n, -1, dtype=np.int64)
        buck = np.full(n, case.base, dtype=np.int64)
        cells = rng.choice(np.arange(18 * W, 2040 * W), n_rec, replace=False)
        slots = np.flatnonzero(np.arange(n) % 2 == 0)[:2048]
        take = slots[:n_rec]
        camp[take] = cells // W
        buck[take] = case.base + ((cells % W - case.base) % W)
        camp[slots[2047] + 1] = 2048                       # (an odd line of the last tile: bin 1)
        cor = case.corpus(camp, buck)
        desc, rec_n, runs, L = case.launch(cor)
        assert desc["grid"] == 64 and desc["cap"] == 32 and L.fallback == 0 and desc["dirty"] == 0
        assert runs[:, :, 1].sum(axis=1).tolist() == [n_rec, 1] == L.total.tolist()
        assert L.dense.tolist() == [n_rec == 2048, True]
        print("dense/sparse %d records: %s | totals %s dense %s" % (n_rec, plan_line(desc), L.total.tolist(), L.dense.tolist()))
        st = case.check_counts("dense/sparse boundary, %d records" % n_rec)
        got = case.ctx.drain_buckets()
        for c, b in zip(c1.tolist(), b1.tolist()):
            assert got[(c, b)] == 4


# -- e. saturation to the cell -----------------------------------------------------------------------

SAT = (1000, 1024)
HOT = (37, 100)               # (campaign, ring slot) of the counted cell


def slot_bucket(base, slot):
    """The bucket of [base, base + W) that lives in ring slot `slot`."""
    return base + ((slot - base) % SAT[1])


def pack_tiles(targets, shift, per_bin=32):
    """Whole tiles of 64 lines holding the views `targets` [(campaign, bucket, n)], at most per_bin
    views of one bin in a tile (one tile per workgroup: no sub-buffer overflows); clicks elsewhere."""
    camp, buck, used, bins = [], [], 0, Counter()

    def close():
        nonlocal used, bins
        camp.extend([-1] * (64 - used))
        buck.extend([0] * (64 - used))
        used, bins = 0, Counter()
    for c, b, n in targets:
        while n:
            room = min(per_bin - bins[c >> shift], 64 - used)
            if room <= 0:
                close()
                continue
            k = min(room, n)
            camp.extend([c] * k)
            buck.extend([b] * k)
            used += k
            bins[c >> shift] += k
            n -= k
    close()
    return np.array(camp, dtype=np.int64), np.array(buck, dtype=np.int64)


def neighbours(base):
    """(0, 5), (5, 0) and a lone 5 at slot 15 of a 16-cell vector, in the hot campaign and the next:
    fold_kernel's pair skip and zero-vector skip beside non-zero neighbours."""
    c = HOT[0]
    return [(k, slot_bucket(base, s), 5) for k, s in ((c, 1), (c, 2), (c, 16 + 15), (c + 1, 100), (c + 1, 64 + 15))]


def sat_launch(case, n_hot, extra=()):
    b = slot_bucket(case.base, HOT[1])
    camp, buck = pack_tiles([(HOT[0], b, n_hot)] + list(extra), 7)      # (1000, 1024): bin = campaign >> 7
    desc, _, _, L = case.launch(case.corpus(camp, buck), arrays=False)
    assert desc["cap"] == 32 and L.fallback == 0 and L.views.sum() == len(extra) * 5 + n_hot
    return desc["dirty"], L


@pytest.mark.parametrize("base", [POS, NEG], ids=["pos", "neg"])
def test_saturation_254_255_256_257(world, base):
    with Case(world, SAT[0], SAT[1], base) as case:
        seq = []
        for i, n in enumerate((254, 1, 1, 1)):
            dirty, L = sat_launch(case, n, neighbours(base) if i == 0 else ())
            seq.append((dirty, L.spills, case.model.byte.get(case.model.cell_of(HOT[0], slot_bucket(base, HOT[1])), 0)))
        print("saturation base %d: (dirty, spills, byte) after 254, +1, +1, +1: %r" % (base, seq))
        assert seq == [(0, 0, 254), (0, 0, 255), (1, 1, 0), (1, 0, 1)]
        case.check_counts("254 + 1 + 1 + 1")
        assert case.ctx.drain_buckets()[(HOT[0], slot_bucket(base, HOT[1]))] == 257


@pytest.mark.parametrize("steps,dirty", [((255,), (0,)), ((256,), (1,)), ((255, 255), (0, 1)),
                                         ((200, "stats", 200, 200), (0, 1, 1)), ((200, "drain", 200, 200), (0, 0, 1))],
                         ids=["255", "256", "255+255", "200x3-stats", "200x3-drain"])
def test_saturation_sequences(world, steps, dirty):
    """stats() waits but does not fold, so 200 + 200 spills at the second launch; a drain between
    folds the first 200 into the u64 ring and the third launch spills."""
    with Case(world, SAT[0], SAT[1], NEG) as case:
        seq, first = [], True
        for s in steps:
            if s == "stats":
                assert case.ctx.stats()["events"] > 0
            elif s == "drain":
                assert case.ctx.drain_buckets()[(HOT[0], slot_bucket(NEG, HOT[1]))] == 200
                case.model.fold()
            else:
                seq.append(sat_launch(case, s, neighbours(NEG) if first else ())[0])
                first = False
        print("saturation %r: dirty %r" % (steps, seq))
        assert tuple(seq) == dirty
        case.check_counts("saturation %r" % (steps,))
        assert case.ctx.drain_buckets()[(HOT[0], slot_bucket(NEG, HOT[1]))] == sum(s for s in steps if isinstance(s, int))


def test_saturation_70000_in_one_launch(world):
    """70,000 records of one cell in one launch: 1,095 workgroups of six tiles (six segments: cap 64),
    64 views of the cell in the first tile of 1,094 of them."""
    G, n_hot = 1095, 70_000
    with Case(world, SAT[0], SAT[1], POS) as case:
        b = slot_bucket(case.base, HOT[1])
        camp = np.full(6 * G * 64, -1, dtype=np.int64)
        buck = np.zeros(camp.size, dtype=np.int64)
        camp[:n_hot], buck[:n_hot] = HOT[0], b
        at = (G - 1) * 64                                  # the first segment's last tile: workgroup 1094
        for c, bb, k in neighbours(case.base):
            camp[at:at + k], buck[at:at + k] = c, bb
            at += k
        cor = case.corpus(camp, buck)
        carrier = np.zeros(len(cor), dtype=np.int64)
        desc, rec_n, runs, L = case.launch(cor, [G * 64] * 6, carrier=carrier)
        assert desc["grid"] == G and desc["cap"] == 64 and L.fallback == 0 and L.spills == 1 and desc["dirty"] == 1
        assert rec_n.sum() == n_hot + 25
        print("saturation 70000: %s | spills %d dirty %d" % (plan_line(desc), L.spills, desc["dirty"]))
        case.check_counts("70,000 in one launch")
        assert case.ctx.drain_buckets()[(HOT[0], b)] == n_hot


# -- f. the cutoffs stay exact -------------------------------------------------------------------------

def atomics_case(world, C, W, what):
    rng = np.random.default_rng(C)
    with Case(world, C, W, NEG) as case:
        cor = rc.geometry_corpus(rng, 20_000, C, N_ADS, N_MAP, NEG, W, case.f)
        bufs = case.submit(cor, [len(cor)])
        case.ctx.sync()
        for p in bufs:
            case.ctx.device_free(p)
        assert case.ctx.path_time()[2] == 0 and case.ctx.launch_info()["record_mode"] == 0
        with pytest.raises(YsbError) as e:
            case.ctx.record_info()
        assert e.value.code == -3                         # YSB_ERR_STATE
        # the atomics count every joined view: the model's table is the plain Counter here
        case.model.side.update(cor.expected())
        case.outside = int(((cor.camp >= 0) & ((cor.bucket < NEG) | (cor.bucket >= NEG + W))).sum())
        case.check_counts(what)
        print("cutoff %s: record launches 0, record_info raises %s" % (what, e.value))


def test_cutoff_ring_wider_than_a_block(world):
    atomics_case(world, 200, 65536, "200x65536 (W > REC_BLOCK_CELLS)")


def test_cutoff_more_blocks_than_the_bins_hold(world):
    """4096 x 32768: 8 bins of 512 blocks, record mode; 4097 x 32768: S would be 1024, atomics."""
    C, W = 4096, 32768
    rng = np.random.default_rng(C)
    with Case(world, C, W, NEG) as case:
        cor = rc.geometry_corpus(rng, 20_000, C, N_ADS, N_MAP, NEG, W, case.f)
        desc, rec_n, runs, L = case.launch(cor)
        assert (desc["n_blocks"], 1 << desc["sub_log2"], desc["bins"]) == (4096, 512, 8) and not L.ambiguous
        print("cutoff 4096x32768: %s | records %d fallback %d" % (plan_line(desc), L.total.sum(), L.fallback))
        case.check_counts("4096x32768")
    atomics_case(world, 4097, 32768, "4097x32768 (S > REC_SUB_MAX)")
