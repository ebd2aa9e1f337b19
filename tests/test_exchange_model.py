"""CPU: tests/exchange_model.py -- the numpy model of the keyed exchange that
tests/test_gpu_exchange_model.py holds the exchange kernels against -- checked on its own:
its plan against the library's host function, its slot alignment on hand-written cases, and
conservation of counts over sequences of complete and pipelined exchanges with played peers."""
import numpy as np
import pytest

from exchange_model import MAXVAL, ExchangeModel, SimulatedPeers, align, carry_case, peer_blocks, plan
from ysb_amd import exchange_plan


@pytest.mark.parametrize("nranks", [1, 2, 3, 8])
def test_plan_equals_library_host_function(nranks):
    rng = np.random.default_rng(100 + nranks)
    cases = []
    for edge in (255 // nranks, 255 // nranks + 1, (2 ** 32 - 1) // nranks, (2 ** 32 - 1) // nranks + 1,
                 (2 ** 64 - 1) // nranks):
        m = np.zeros(32, dtype=np.uint64)
        m[3], m[17], m[31] = np.uint64(1), np.uint64(edge), np.uint64(min(edge, 7))
        cases.append(m)
    for W in (16, 64, 512):
        for hi in (2, 40, 300, 2 ** 31, 2 ** 40):
            m = rng.integers(0, hi, W, dtype=np.uint64)
            m[rng.random(W) < 0.6] = 0
            cases.append(m)
    cases.append(np.zeros(16, dtype=np.uint64))
    for m in cases:
        slots, width = exchange_plan(m, nranks)
        ms, mw = plan(m, nranks)
        assert ms == [int(s) for s in slots] and mw == width, (m, nranks)
    # the boundaries themselves
    for edge, w in ((255 // nranks, 1), (255 // nranks + 1, 4), ((2 ** 32 - 1) // nranks, 4),
                    ((2 ** 32 - 1) // nranks + 1, 8)):
        m = np.zeros(16, dtype=np.uint64)
        m[5] = np.uint64(edge)
        assert plan(m, nranks) == ([5], w) and exchange_plan(m, nranks)[1] == w


def test_align_hand_written_cases():
    W = 64
    assert align([5], W) == [4, 5, 6, 7]                                   # an isolated slot
    assert align([2, 3, 5], W) == [0, 1, 2, 3, 4, 5, 6, 7]                 # two runs that touch after widening
    assert align([3, 4], W) == list(range(0, 8))                           # one run over a group boundary
    assert align([1, 6], W) == list(range(0, 8))                           # two runs in one..two groups merge
    assert align([1, 2], W) == [0, 1, 2, 3]
    assert align([0, 2], W) == [0, 1, 2, 3]                                # both runs in one group: no duplicates
    assert align([61, 62, 63], W) == [60, 61, 62, 63]                      # a run ending at W - 1
    assert align([63], W) == [60, 61, 62, 63]
    assert align([0], W) == [0, 1, 2, 3]
    assert align([], W) == []                                              # the empty plan
    assert align(list(range(W)), W) == list(range(W))                      # all W slots
    assert align([5, 20, 21, 22, 23, 24, 63], W) == [4, 5, 6, 7] + list(range(20, 28)) + [60, 61, 62, 63]
    rng = np.random.default_rng(3)
    for _ in range(200):
        s = sorted(set(rng.integers(0, W, rng.integers(0, 30)).tolist()))
        a = align(s, W)
        assert len(a) % 4 == 0 and a == sorted(set(a)) and set(s) <= set(a) and all(0 <= x < W for x in a)
        assert all(a[i:i + 4] == list(range(a[i], a[i] + 4)) and a[i] % 4 == 0 for i in range(0, len(a), 4))
        assert {x // 4 for x in a} == {y // 4 for y in s}                    # no group without a planned slot


def test_carry_case_is_the_per_byte_carry_the_word_add_must_see():
    hits = 0
    for o in range(256):
        for v in range(256):
            t = (o & 0x7F) + (v & 0x7F)
            buggy_word_add = (((o & v) | ((o | v) & ~t)) & 0x80) == 0 and o + v > 255
            assert carry_case(o, v) == buggy_word_add
            hits += carry_case(o, v)
    assert hits > 0


def random_table(rng, C, W, slots, hi):
    t = np.zeros((C, W), dtype=np.uint64)
    for s in slots:
        t[:, s] = rng.integers(0, hi + 1, C, dtype=np.uint64) * (rng.random(C) < 0.7)
    return t


@pytest.mark.parametrize("nranks,rank", [(1, 0), (2, 1), (3, 0), (8, 7), (8, 3)])
def test_conservation_over_complete_and_pipelined_exchanges(nranks, rank):
    rng = np.random.default_rng(nranks * 10 + rank)
    C, W = 100, 64
    m = ExchangeModel(C, W, nranks, rank)
    sim = SimulatedPeers(m, seed=5)
    assert m.c_pad % nranks == 0 and m.per * nranks == m.c_pad >= C
    kinds = [False, True, True, False, True, True, True, False]
    his = [20, 25, 200, 10, 3, 70_000, 9, 2]
    for step, (pipelined, hi) in enumerate(zip(kinds, his)):
        slots = sorted({5} | set(rng.choice([0, 1, 2, 9, 10, 11, 20, 40, 41, 42, 63], 4).tolist()))
        m.add(random_table(rng, C, W, slots, hi))
        pm = np.zeros(W, dtype=np.uint64)
        for s in rng.integers(0, W, 4):
            pm[s] = rng.integers(1, 2 * hi + 2)
        if step == 5:
            pm[7] = 2 ** 33
        sim.next_peer_max, sim.next_pipelined = pm, pipelined
        buf = m.slot_max().copy()
        before = m.pending.copy()
        sim.allreduce_max(buf)
        cur = sim.cur
        assert (buf >= pm).all() and (buf >= before.max(axis=0)).all()
        assert cur["pipelined"] == (pipelined and step > 0)
        R = len(cur["aligned"])
        if R:
            send = cur["send"]
            assert send.shape == (m.c_pad, R) and not send[C:].any()
            if cur["cap"] is None:
                assert not m.pending[:, cur["aligned"]].any()           # a complete exchange leaves nothing
            else:
                assert cur["cap"] == MAXVAL[cur["width"]] // nranks
                assert int(send.max()) <= cur["cap"]
                kept = m.pending[:, cur["aligned"]]
                assert ((kept == 0) | (kept > cur["cap"])).all()         # only cells above cap stay
            assert np.array_equal(send + m.pending[:, cur["aligned"]], before[:, cur["aligned"]])
            recv = sim.reduce_scatter_sum(send.astype({1: np.uint8, 4: np.uint32, 8: np.uint64}[cur["width"]], order="C")
                                          .view(np.uint8).ravel(), m.per * R, cur["width"])
            assert recv.size == m.per * R
        if not cur["pipelined"]:
            assert not m.pending.any()
        assert m.conserved(), step
    assert m.held_back > 0 and m.sent_away >= 0 and (nranks == 1 or m.peer_cells > 0)
    lo = rank * m.per
    t = m.drain_table()
    assert int(t.sum()) == int(m.pending[:C].sum()) + int(m.owned[:max(0, min(m.per, C - lo))].sum())
    assert not m.owned[max(0, min(m.per, C - lo)):].any()                # nothing lands in padding rows


def test_pipelined_plan_lags_one_call():
    m = ExchangeModel(100, 16, 8, 2)
    z = np.zeros(16, dtype=np.uint64)
    t = np.zeros((100, 16), dtype=np.uint64)
    t[4, 5] = 3
    m.add(t)
    a = m.begin(z, pipelined=True)              # the first call is complete whatever was asked
    assert not a["pipelined"] and a["aligned"] == [4, 5, 6, 7] and a["width"] == 1 and a["cap"] is None
    m.finish(np.zeros((7, m.per, 4), dtype=np.uint64))
    t[4, 5], t[4, 6], t[50, 12] = 40, 31, 1     # above cap 31; at cap; outside the previous plan
    m.add(t)
    b = m.begin(z, pipelined=True)
    assert b["pipelined"] and b["aligned"] == [4, 5, 6, 7] and b["cap"] == 31
    assert b["send"][4].tolist() == [0, 0, 31, 0] and m.pending[4, 5] == 40 and m.pending[50, 12] == 1
    assert m.held_back == 1 and m.partial_words == 1
    m.finish(np.zeros((7, m.per, 4), dtype=np.uint64))
    c = m.begin(z, pipelined=True)              # the plan of the call before: width 4, both slots' groups
    assert c["width"] == 4 and c["aligned"] == [4, 5, 6, 7, 12, 13, 14, 15] and c["cap"] == (2 ** 32 - 1) // 8
    m.finish(np.zeros((7, m.per, 8), dtype=np.uint64))
    assert not m.pending.any() and m.conserved()
    m.forget_plan()
    assert not m.begin(z, pipelined=True)["pipelined"]


def test_peer_blocks_stay_below_their_maxima_and_reach_them():
    bound = [0, 31, 1, 70_000, (2 ** 32 - 1) // 8, 2 ** 33, 0, 5]
    b = peer_blocks(9, bound, 8, 13, 9)
    assert b.shape == (7, 13, 8) and not b[:, 9:].any()
    for k, v in enumerate(bound):
        assert int(b[:, :, k].max()) == v
    assert peer_blocks(9, bound, 1, 13, 13).shape == (0, 13, 8)
    m = ExchangeModel(100, 16, 8, 0)
    m.begin(np.array([1] + [0] * 15, dtype=np.uint64))
    with pytest.raises(AssertionError):
        m.finish(np.full((7, m.per, 4), 40, dtype=np.uint64))   # 7 x 40 wraps a byte: the model refuses
