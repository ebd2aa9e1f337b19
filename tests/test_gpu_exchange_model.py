"""GPU: the exchange kernels (csrc/ysb_table.hip xplan / xpack / xpack8 / xunpack / xunpack8)
and their planning (csrc/ysb_group.cpp exchange, align_slot_runs, finish_unpack) as rank r of
N on ONE context, the other N - 1 ranks played by the test (tests/exchange_model.py).

ysb_group_init_host's collectives run on the calling thread on host memory, so the test's
all-reduce(max) callback sets the peers' per-slot maxima (which fix the plan's slots and
width), and its reduce-scatter callback sees the whole send buffer -- every owner's block --
and supplies the peers' summed cells of this rank's block.  Every buffer is compared cell by
cell with the numpy model: the plan kernel's maxima, the packed send buffer (all N blocks,
padding rows zero), count and width, then exchange_info and the drain (owned block + what
stays pending).  The rank's own counts come from the C oracle over the submitted lines, whose
event_time digits are rewritten so that the buckets land on chosen ring slots.
"""
import functools

import numpy as np
import pytest

from exchange_model import ExchangeModel, SimulatedPeers
from oracle import oracle
from ysb_amd import GenParams, YsbContext, YsbError, table_rows

pytestmark = pytest.mark.gpu

ET_KEY = b'"event_time": "'
T0_BUCKET = 1_700_000_000_000 // 10000


def ring_base(W):
    """A ring base that is a multiple of W: bucket base + s lives in ring slot s."""
    return T0_BUCKET // W * W


class Batch:
    """n generator lines with line i's event time moved into ring slot slot_of[i] (the 13
    event_time digits rewritten, as tests/test_gpu_mapped.py time_table locates them), and the
    C oracle's counts of them as a [n_campaigns][W] table."""

    def __init__(self, g, admap, n_campaigns, W, n, weights, first=0, seed=0):
        raw, offs = g.events_host(first, n)
        self.raw, self.offs = raw.copy(), offs.copy()
        data = self.raw.tobytes()
        ends = list(self.offs[1:]) + [len(data)]
        pos = np.array([data.index(ET_KEY, int(s), int(e)) + len(ET_KEY) for s, e in zip(self.offs, ends)],
                       dtype=np.int64)
        slots = np.array(sorted(weights), dtype=np.int64)
        p = np.array([weights[int(s)] for s in slots], dtype=np.float64)
        slot_of = slots[np.random.default_rng(seed).choice(slots.size, n, p=p / p.sum())]
        t = (ring_base(W) + slot_of) * 10000 + np.arange(n) % 10000
        digits = (t[:, None] // 10 ** np.arange(12, -1, -1)[None, :]) % 10 + ord("0")
        self.raw[pos[:, None] + np.arange(13)[None, :]] = digits.astype(np.uint8)
        rows, st = oracle.run(admap, self.raw, self.offs)
        assert st["parse_errors"] == 0 and st["time_errors"] == 0 and st["join_misses"] == 0
        self.table = np.zeros((n_campaigns, W), dtype=np.uint64)
        for (c, b), v in rows.items():
            assert 0 <= b - ring_base(W) < W
            self.table[c, b - ring_base(W)] = v
        assert set(np.nonzero(self.table.any(axis=0))[0].tolist()) <= set(weights)


# ---- the two geometries: 100 campaigns x 10 ads (atomic mode), and the smallest map whose
# launches run in record mode (csrc/ysb_submit.cpp plan_records: the HBM bucket-layout join
# table, i.e. more than 2^18 ads, and no LDS window counters, i.e. more than 128 campaigns)

@functools.lru_cache(maxsize=None)
def small_map():
    g = GenParams(seed=42, n_campaigns=100, ads_per_campaign=10, events_per_sec=100_000)
    _, aids = g.ids()
    camp = g.ad_campaign_index()
    return g, aids, camp, oracle.AdMap(aids, camp)


REC_C = 1003                       # c_pad 1008 at N = 8, 126 rows per owner
REC_HOT = [3 + 50 * k for k in range(20)]   # half of the ads belong to these 20 campaigns


@functools.lru_cache(maxsize=None)
def record_map():
    g = GenParams(seed=11, n_campaigns=REC_C, ads_per_campaign=262, events_per_sec=100_000)
    assert g.n_ads > 1 << 18
    _, ab = g.ids_packed()
    i = np.arange(g.n_ads)
    camp = np.where(i % 2 == 0, np.asarray(REC_HOT)[(i // 2) % len(REC_HOT)], i % REC_C).astype(np.uint32)
    aids = [ab[36 * k:36 * k + 36].tobytes() for k in range(g.n_ads)]
    return g, ab, camp, oracle.AdMap(aids, camp.tolist())


@functools.lru_cache(maxsize=None)
def small_batch(W, n, weights, seed=0, first=0):
    g, _, _, admap = small_map()
    return Batch(g, admap, 100, W, n, dict(weights), first, seed)


@functools.lru_cache(maxsize=None)
def record_batch(W, n, weights, seed=0, first=0):
    g, _, _, admap = record_map()
    return Batch(g, admap, REC_C, W, n, dict(weights), first, seed)


def open_context(**kw):
    return YsbContext(device=0, **kw)


class Rig:
    """One context as rank `rank` of `nranks`, its model and its played peers."""

    def __init__(self, W, nranks, rank, record=False, max_bytes=1 << 20, max_events=1 << 12, seed=1):
        self.W, self.record = W, record
        self.C = REC_C if record else 100
        self.model = ExchangeModel(self.C, W, nranks, rank)
        self.sim = SimulatedPeers(self.model, seed=seed)
        self.ctx = open_context(n_campaigns=self.C, window_ring=W, ring_base_bucket=ring_base(W),
                                max_batch_bytes=max_bytes + 64, max_batch_events=max_events + 1,
                                record_count=True if record else None)
        # the whole ad map, not a shard: this rank counts every campaign
        if record:
            _, ab, camp, _ = record_map()
            self.ctx.load_ad_map_packed(ab, camp)
        else:
            _, aids, camp, _ = small_map()
            self.ctx.load_ad_map(aids, camp)
        self.ctx.group_init_host_fns(rank, nranks, self.sim.allreduce_max, self.sim.reduce_scatter_sum)
        self.submits = 0

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.ctx.close()

    def submit(self, batch):
        self.ctx.submit(batch.raw, batch.offs, slot=self.submits & 1)
        self.submits += 1
        self.model.add(batch.table)

    def peer_max(self, d):
        pm = np.zeros(self.W, dtype=np.uint64)
        for s, v in d.items():
            pm[s] = np.uint64(v)
        return pm

    def exchange(self, peer_max=None, pipelined=False, bound=None, override=None):
        """One exchange against the model; returns the model's description of it."""
        sim, ctx = self.sim, self.ctx
        sim.next_peer_max = self.peer_max(peer_max or {})
        sim.next_pipelined, sim.next_bound, sim.next_override = pipelined, bound, override
        calls, rs = sim.calls, sim.rs_calls
        try:
            (ctx.group_exchange_pipelined if pipelined else ctx.group_reduce_scatter)()
        except YsbError:
            if ctx.callback_error is not None:
                raise ctx.callback_error from None
            raise
        assert ctx.callback_error is None
        cur = sim.cur
        assert sim.calls == calls + 1 and sim.rs_calls == rs + (1 if cur["aligned"] else 0)
        x = ctx.exchange_info()
        assert (x["last_width"], x["last_buckets"]) == (self.model.last_width, self.model.last_buckets)
        assert self.model.conserved()
        return cur

    def check_drain(self):
        got = self.ctx.drain_buckets()
        assert self.ctx.callback_error is None
        exp = table_rows(self.model.drain_table(), ring_base(self.W))
        self.model.fold()   # the drain read the owned table: its u8 accumulator is folded
        assert got == exp, "%d rows differ" % len(set(got.items()) ^ set(exp.items()))
        if self.record:
            assert self.ctx.path_time()[2] == self.submits   # every launch ran in record mode


def runs(*rs):
    return tuple((s, 1.0) for a, b in rs for s in range(a, b))


# ---- 1. N = 8 geometry, width 1, atomic-mode ring: xpack_kernel<u8>, xunpack8 ------------

@pytest.mark.parametrize("rank", [0, 3, 7])
@pytest.mark.parametrize("W", [16, 64])
def test_n8_width1_owned_u8_accumulator_over_three_exchanges(W, rank):
    """100 campaigns pad to 104, 13 rows per owner; rank 7's block ends in four padding rows.
    Three complete exchanges with no read in between: the received bytes (own + seven peers of
    at most 31) carry the owned u8 accumulator past 127 and then 255, the per-byte carry case
    included (checked on the model first, as
    test_owned_u8_accumulator_carries_across_exchanges_without_reads does)."""
    live = (2, 10) if W == 16 else (10, 42)
    b = small_batch(W, 24_000, runs(live))
    assert 0 < int(b.table.max()) * 8 <= 255
    pm = {s: 31 - (s % 3) for s in range(*live)}
    with Rig(W, 8, rank, max_bytes=b.raw.size, max_events=b.offs.size) as rig:
        assert (rig.model.c_pad, rig.model.per) == (104, 13)
        rig.sim.fill, rig.sim.lean = 1.0, 1
        for k in range(3):
            rig.submit(b)
            cur = rig.exchange(pm)
            assert cur["width"] == 1 and cur["aligned"] == list(range(live[0] // 4 * 4, (live[1] + 3) // 4 * 4))
        m = rig.model
        assert m.acc8_past_127 > 0 and m.acc8_past_255 > 0 and m.carry_cases > 0
        rig.check_drain()


# ---- 2. scattered plans -----------------------------------------------------------------

def test_scattered_plan_isolated_merging_last_slot_and_peer_only_slots():
    """W = 64, rank 3 of 8.  Own counts in slot 0, an isolated slot 5, 17-18 and 21 (two runs
    whose groups touch after widening), 33 and 35 (two runs in one group: merged), 62-63 (a run
    ending at W - 1); the peers alone hold counts in 27 and 40-42: this rank sends zeros there
    and receives values.  A second exchange then runs another, shorter plan."""
    own = (0, 5, 17, 18, 21, 33, 35, 62, 63)
    b = small_batch(64, 8_000, tuple((s, 1.0) for s in own))
    b2 = small_batch(64, 3_000, ((9, 1.0), (63, 2.0)), seed=2)
    assert int(b.table.max()) * 8 <= 255 and all(b.table[:, s].any() for s in own)
    with Rig(64, 8, 3, max_bytes=b.raw.size, max_events=b.offs.size) as rig:
        rig.submit(b)
        cur = rig.exchange({27: 9, 40: 31, 41: 1, 42: 30, 5: 12, 63: 31})
        assert cur["width"] == 1 and cur["slots"] == sorted(own + (27, 40, 41, 42))
        assert cur["aligned"] == [0, 1, 2, 3, 4, 5, 6, 7] + list(range(16, 28)) + list(range(32, 36)) + \
            list(range(40, 44)) + list(range(60, 64))
        lo = 3 * 13
        sent = cur["send"][lo:lo + 13]
        for s in (27, 40, 42):   # zeros sent, values received
            k = cur["aligned"].index(s)
            assert not cur["send"][:, k].any() and rig.sim.last_recv[:, k].any() and not sent[:, k].any()
        rig.check_drain()
        rig.submit(b2)
        cur = rig.exchange({50: 3})
        assert cur["aligned"] == [8, 9, 10, 11, 48, 49, 50, 51, 60, 61, 62, 63]
        rig.check_drain()


# ---- 3. width 4 and width 8 ---------------------------------------------------------------

@pytest.mark.parametrize("nranks", [2, 8])
@pytest.mark.parametrize("kind", ["w4_70000", "w4_large_sums", "w8"])
def test_wide_cells_arrive_intact(kind, nranks):
    """A peer maximum of 70 000 makes the cells 4 bytes wide; with a slot whose peer maximum is
    (2^32 - 1) // N every peer holds that maximum in one cell (a sum of (N - 1) x it, above
    2^31 once this rank's own count is added) -- and a peer maximum of 2^33 makes them 8 bytes,
    a cell sum above 2^32 arriving intact in the drain (xpack / xunpack <u32> and <u64>)."""
    W, rank = 16, nranks - 1
    b = small_batch(W, 3_000, runs((1, 7)))
    big = (2 ** 32 - 1) // nranks
    pm = {9: 70_000, 2: 17}
    if kind == "w4_large_sums":
        pm[3] = big
    if kind == "w8":
        pm[3] = 2 ** 33
    per = (100 + nranks - 1) // nranks
    lo = rank * per
    row = int(np.nonzero(b.table[lo:lo + per, 3])[0][0])   # a row of this block with an own count in slot 3

    def every_peer_at_its_maximum(blocks, aligned):
        if 3 in pm:
            blocks[:, row, aligned.index(3)] = np.uint64(pm[3])
        blocks[0, row, aligned.index(9)] = np.uint64(70_000)

    with Rig(W, nranks, rank, max_bytes=b.raw.size, max_events=b.offs.size) as rig:
        rig.submit(b)
        cur = rig.exchange(pm, override=every_peer_at_its_maximum)
        assert cur["width"] == (8 if kind == "w8" else 4)
        assert cur["aligned"] == list(range(0, 12))
        got = int(rig.sim.last_recv[row, 3])
        if kind == "w4_large_sums":
            assert got == (nranks - 1) * big + int(b.table[lo + row, 3]) and 2 ** 31 <= got <= 2 ** 32 - 1
            assert abs(got - (2 ** 32 - 1) * (nranks - 1) // nranks) <= nranks + int(b.table.max())   # near it
        if kind == "w8":
            assert got > 2 ** 32 and got == (nranks - 1) * 2 ** 33 + int(b.table[lo + row, 3])
        rig.check_drain()
        rig.submit(b)            # then narrow cells again, into the same owned cells
        assert rig.exchange({2: 5})["width"] == 1
        rig.check_drain()


# ---- 4. more than 256 planned slots: L > 64 in XLanes ---------------------------------------

@pytest.mark.parametrize("width", [1, 4])
def test_more_than_256_planned_slots(width):
    """W = 512, 333 planned slots in four runs: rows of more than 64 words, one row per wave
    and its lanes striding by 64 (xpack / xunpack's k += 64 loops; at width 1 xunpack8's
    strided words, over three exchanges without a read so that its carry test is reached)."""
    live = ((8, 150), (200, 330), (400, 460), (509, 510))
    b = small_batch(512, 20_000, runs(*live))
    assert int(b.table.max()) * 8 <= 255
    pm = {s: 31 - s % 3 for a, e in live for s in range(a, e)}
    if width == 4:
        pm[100] = 70_000
    with Rig(512, 8, 2, max_bytes=b.raw.size, max_events=b.offs.size) as rig:
        rig.sim.fill, rig.sim.lean = 1.0, 1
        for _ in range(3):
            rig.submit(b)
            cur = rig.exchange(pm)
            assert cur["width"] == width and len(cur["slots"]) == 333 and len(cur["aligned"]) > 4 * 64
        assert width == 4 or rig.model.carry_cases > 0
        rig.check_drain()


# ---- 5. W > 4096: the plan kernel's maxima by global atomics ---------------------------------

def test_ring_of_8192_slots_plans_without_lds():
    own = (0, 1, 777, 2048, 4095, 4096, 4097, 5000, 5001, 5002, 5003, 6006, 8190, 8191) + tuple(range(3000, 3010))
    b = small_batch(8192, 6_000, tuple((s, 1.0) for s in own))
    assert int(b.table.max()) * 8 <= 255 and all(b.table[:, s].any() for s in own)
    pm = {s: 1 + s % 30 for s in (5, 100, 4094, 4100, 7000, 7001, 7002, 7003, 7004, 8000, 8189, 3005)}
    with Rig(8192, 8, 5, max_bytes=b.raw.size, max_events=b.offs.size) as rig:
        rig.submit(b)
        cur = rig.exchange(pm)
        assert cur["width"] == 1 and len(cur["slots"]) == len(set(own) | set(pm)) == 35
        rig.check_drain()


# ---- 6. record mode: the u8 delta ring, xpack8, xplan's register path -------------------------

def test_record_mode_delta_ring_width1():
    """6a.  Rank 5 of 8, 1003 campaigns (126 rows per owner), W = 128: plain counts in the u8
    delta ring, a contiguous run plus scattered slots; the peers alone hold slot 90."""
    own = ((3, 3.0), (127, 3.0)) + runs((40, 60))
    b = record_batch(128, 12_000, own)
    assert 0 < int(b.table.max()) * 8 <= 255
    with Rig(128, 8, 5, record=True, max_bytes=b.raw.size, max_events=b.offs.size) as rig:
        assert (rig.model.c_pad, rig.model.per) == (1008, 126)
        rig.sim.fill = 0.2
        for _ in range(2):
            rig.submit(b)
            cur = rig.exchange({90: 20, 41: 31, 3: 2})
            assert cur["width"] == 1
            assert cur["aligned"] == [0, 1, 2, 3] + list(range(40, 60)) + [88, 89, 90, 91, 124, 125, 126, 127]
        rig.check_drain()


def test_record_mode_u64_ring_in_play_beside_the_delta_ring():
    """6b.  Delta cells of the hot campaigns pass 255 within one launch and hand their sums to
    the u64 ring (*dirty set, ysb_count.hip add16); a second launch adds fresh deltas on top.
    The send buffer is still pending = delta + u64, cell by cell."""
    b = record_batch(16, 60_000, ((2, 6.0), (3, 1.0), (4, 1.0), (9, 1.0), (15, 1.0)))
    b2 = record_batch(16, 6_000, ((2, 1.0), (3, 1.0), (12, 1.0)), seed=3, first=60_000)
    assert int(b.table.max()) > 255 and int((b.table > 255).sum()) >= 10
    assert 0 < int(b2.table[b.table > 255].max())    # a saturated cell gets a fresh delta too
    with Rig(16, 8, 5, record=True, max_bytes=b.raw.size, max_events=b.offs.size) as rig:
        rig.sim.fill = 0.2
        rig.submit(b)
        rig.submit(b2)
        cur = rig.exchange({7: 400})
        assert cur["width"] == 4 and cur["aligned"] == list(range(0, 16))
        rig.check_drain()


# ---- 7. the pipelined exchange's hold-back ----------------------------------------------------

def pipelined_sequence(rig, a, b, c, d, cap):
    """complete (first call) / held back by cap and by plan / caught up / idle / complete."""
    m = rig.model
    rig.submit(a)
    cur = rig.exchange({33: 9, 8: 20}, pipelined=True)
    assert not cur["pipelined"] and cur["width"] == 1           # the first call after init is complete
    rig.submit(b)
    cur = rig.exchange({8: 200, 50: 7}, pipelined=True)         # packs with the first call's plan
    assert cur["pipelined"] and cur["width"] == 1 and cur["cap"] == cap
    assert cur["aligned"] == [8, 9, 10, 11, 20, 21, 22, 23, 32, 33, 34, 35]
    assert m.held_back > 0 and m.held_back_cap_plus_1 > 0 and m.partial_words > 0
    assert int(cur["send"].max()) == cap and m.pending[:, 50].any()   # cells at cap go; slot 50 waits
    held = m.held_back
    rig.submit(c)
    cur = rig.exchange({}, pipelined=True)                      # the second call's plan: 4-byte cells
    assert cur["pipelined"] and cur["width"] == 4 and 50 in cur["slots"] and m.held_back == held
    assert not m.pending.any()
    cur = rig.exchange({21: 3}, pipelined=True)                 # nothing new: the third call's plan
    assert cur["pipelined"] and not cur["send"].any()
    rig.submit(d)
    cur = rig.exchange({21: 3, 60: 1}, pipelined=False)
    assert not cur["pipelined"] and not m.pending.any()
    rig.check_drain()


def test_pipelined_hold_back_atomic_mode():
    """xpack_kernel<u8> under a cap: rank 3 of 8, cap 31.  The second batch's cells in slots
    8-11 sit around the cap (some above, one exactly cap + 1, some at or below it in the same
    group of four) and it fills slot 50, outside the plan."""
    a = small_batch(64, 6_000, runs((8, 12)) + ((20, 1.0),))
    b = small_batch(64, 40_000, ((8, 9.0), (9, 9.0), (10, 7.0), (11, 10.0), (50, 3.0)), seed=1, first=6_000)
    c = small_batch(64, 3_000, ((9, 1.0), (50, 1.0)), seed=2, first=46_000)
    d = small_batch(64, 3_000, ((21, 1.0), (11, 1.0)), seed=3, first=49_000)
    assert int(a.table.max()) <= 31 and (b.table[:, 8:12] == 31).any()
    with Rig(64, 8, 3, max_bytes=b.raw.size, max_events=b.offs.size) as rig:
        pipelined_sequence(rig, a, b, c, d, 31)


@pytest.mark.parametrize("u64_ring", [False, True])
def test_pipelined_hold_back_record_mode(u64_ring):
    """xpack8 under a cap, rank 5 of 8.  Without the u64 ring in play the aligned groups move as
    words: a word with only some of its four bytes above the cap keeps exactly those.  With a
    hot cell that saturates its delta byte (*dirty) the same plan packs cell by cell from
    delta + u64."""
    # shares of a hot campaign's ~500 views: about the cap of 31 in slots 9-11 (and in slot 8,
    # or ~300 there: the delta byte saturates); the rest below 255 a cell in slots outside the plan
    rest = tuple(range(40, 48)) + tuple(range(50, 54))
    w8 = 0.6 if u64_ring else 0.062
    spread = tuple((s, (1.0 - w8 - 0.182) / len(rest)) for s in rest)
    a = record_batch(64, 6_000, runs((8, 12)) + ((20, 1.0),))
    b = record_batch(64, 60_000, ((8, w8), (9, 0.062), (10, 0.05), (11, 0.07)) + spread, seed=1, first=6_000)
    c = record_batch(64, 3_000, ((9, 1.0), (50, 1.0)), seed=2, first=66_000)
    d = record_batch(64, 3_000, ((21, 1.0), (11, 1.0)), seed=3, first=69_000)
    assert int(a.table.max()) <= 31 and (b.table[:, 8:12] == 31).any()
    assert (int(b.table.max()) > 255) == u64_ring
    with Rig(64, 8, 5, record=True, max_bytes=b.raw.size, max_events=b.offs.size) as rig:
        rig.sim.fill = 0.2
        pipelined_sequence(rig, a, b, c, d, 31)
