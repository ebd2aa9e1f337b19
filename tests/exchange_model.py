"""A plain numpy model of the keyed exchange, with the other ranks played by the test.

Written from the contract in include/ysb_hip.h (ysb_group_reduce_scatter,
ysb_group_exchange_pipelined, ysb_exchange_plan, ysb_group_exchange_info) and the comments
of csrc/ysb_group.cpp (align_slot_runs, exchange) -- no GPU, no library call.  Everything is
an unsigned integer and exact.

One ExchangeModel is rank `rank` of `nranks`: `pending[c_pad][W]` are its counts since its
last exchange (every owner's rows), `owned[per][W]` its owner block.  An exchange is
    begin(peer_max, pipelined)  -> the plan the pack uses and the send buffer [c_pad][R]
    finish(peer_blocks)         -> recv = send[own block] + sum of the peers' blocks, unpacked
so a test's all-reduce callback can call begin and its reduce-scatter callback finish, with
the library's buffers compared in between (SimulatedPeers).
"""
from __future__ import annotations

import numpy as np

U64 = np.uint64
MAXVAL = {1: 0xFF, 4: 0xFFFFFFFF, 8: 0xFFFFFFFFFFFFFFFF}
CELL = {1: np.uint8, 4: np.uint32, 8: np.uint64}


def plan(slot_max, nranks):
    """(slots with max > 0, ascending; the narrowest width whose sum over nranks cannot wrap)."""
    m = [int(v) for v in slot_max]
    slots = [s for s, v in enumerate(m) if v > 0]
    bound = nranks * max(m, default=0)
    assert bound <= MAXVAL[8], "nranks * max does not fit 64 bits"
    return slots, (1 if bound <= MAXVAL[1] else 4 if bound <= MAXVAL[4] else 8)


def align(slots, W):
    """Each run of consecutive slots grown to [floor4(first), ceil4(last + 1)), clipped to W,
    duplicates merged: whole aligned groups of four."""
    out = []
    i = 0
    while i < len(slots):
        j = i
        while j + 1 < len(slots) and slots[j + 1] == slots[j] + 1:
            j += 1
        a, b = slots[i] // 4 * 4, min((slots[j] + 4) // 4 * 4, W)
        out.extend(s for s in range(a, b) if not out or s > out[-1])
        i = j + 1
    return out


def carry_case(o, v):
    """A u8 accumulator add o + v that passes 255 although one byte is below 128 and the low
    seven bits alone carry into bit 7: the adds a per-byte carry test has to get right."""
    return o + v > 255 and ((o ^ v) & 0x80) != 0 and (o & 0x7F) + (v & 0x7F) >= 128


class ExchangeModel:
    def __init__(self, n_campaigns, W, nranks, rank):
        assert 0 <= rank < nranks and W >= 16 and W & (W - 1) == 0
        self.C, self.W, self.N, self.rank = n_campaigns, W, nranks, rank
        self.c_pad = (n_campaigns + nranks - 1) // nranks * nranks
        self.per = self.c_pad // nranks
        self.pending = np.zeros((self.c_pad, W), dtype=U64)
        self.owned = np.zeros((self.per, W), dtype=U64)
        self.acc8 = np.zeros((self.per, W), dtype=U64)   # the owned table's u8 accumulator
        self.carry_cases = 0      # width-1 unpacks that hit carry_case
        self.acc8_past_127 = 0    # accumulator bytes that went from below 128 to 128..255
        self.acc8_past_255 = 0    # accumulator bytes whose sum passed 255
        self.counted = 0          # counts put in
        self.peer_cells = 0       # what the peers sent into this rank's block
        self.sent_away = 0        # what this rank sent into other owners' blocks
        self.have_plan = False
        self.prev_plan = None
        self.cur = None
        self.last_buckets = self.last_width = 0
        self.held_back = 0              # cells a pipelined pack left pending (above cap)
        self.held_back_cap_plus_1 = 0   # ... of exactly cap + 1
        self.partial_words = 0          # aligned 4-cell words with some cells above cap, some sent

    # -- counts -------------------------------------------------------------------------
    def add(self, table):
        t = np.asarray(table, dtype=U64)
        assert t.shape == (self.C, self.W)
        self.pending[:self.C] += t
        self.counted += int(t.sum(dtype=U64))

    def slot_max(self):
        return self.pending.max(axis=0)

    def forget_plan(self):
        """After ysb_reset / ysb_ring_advance the next exchange is complete."""
        self.have_plan = False

    def fold(self):
        """A read of the owned table folds the u8 accumulator."""
        self.acc8[:] = 0

    # -- one exchange -------------------------------------------------------------------
    def begin(self, peer_max, pipelined=False):
        """Plans from max(own maxima, peer_max), packs with that plan (complete) or with the
        previous call's under its cap (pipelined).  Returns the exchange's description."""
        assert self.cur is None
        peer_max = np.asarray(peer_max, dtype=U64)
        agreed = np.maximum(self.slot_max(), peer_max)
        new_plan = plan(agreed, self.N)
        pipelined = pipelined and self.have_plan
        slots, width = self.prev_plan if pipelined else new_plan
        cap = MAXVAL[width] // self.N if pipelined else None
        self.prev_plan, self.have_plan = new_plan, True
        al = align(slots, self.W)
        assert len(al) % 4 == 0
        send = self.pack(al, cap)
        self.last_buckets, self.last_width = len(slots), (width if al else 0)
        cur = {"slots": slots, "aligned": al, "width": width, "cap": cap, "send": send,
               "pipelined": pipelined, "agreed": agreed}
        self.cur = cur if al else None   # an empty plan has no reduce-scatter and no unpack
        return cur

    def pack(self, aligned, cap=None):
        """send[c_pad][R]: the planned cells at most cap, zeroed here; cells above cap stay."""
        idx = np.asarray(aligned, dtype=np.int64)
        cells = self.pending[:, idx]
        if cap is None:
            go = np.ones(cells.shape, dtype=bool)
        else:
            go = cells <= U64(cap)
            self.held_back += int((~go).sum())
            if cap < MAXVAL[8]:
                self.held_back_cap_plus_1 += int((cells == U64(cap + 1)).sum())
            if idx.size:
                w = go.reshape(self.c_pad, -1, 4)
                v = (cells > 0).reshape(self.c_pad, -1, 4)
                self.partial_words += int(((~w).any(axis=2) & (w & v).any(axis=2)).sum())
        send = np.ascontiguousarray(np.where(go, cells, U64(0)), dtype=U64)
        self.pending[:, idx] = np.where(go, U64(0), cells)
        lo, hi = self.rank * self.per, (self.rank + 1) * self.per
        self.sent_away += int(send.sum(dtype=U64)) - int(send[lo:hi].sum(dtype=U64))
        return send

    def finish(self, peer_blocks, bound=None):
        """peer_blocks [nranks - 1][per][R]: the other ranks' cells of this rank's block, each
        at most bound[R] (the peers' agreed per-slot maxima: what keeps the agreed width from
        wrapping).  Returns recv [per][R] = own block + their sum, and unpacks it."""
        cur, self.cur = self.cur, None
        R = len(cur["aligned"])
        pb = np.asarray(peer_blocks, dtype=U64).reshape(self.N - 1, self.per, R)
        if bound is not None:
            for k in range(R):
                assert int(pb[:, :, k].max(initial=0)) <= int(bound[k]), "a peer cell above its slot's maximum"
        assert not pb[:, max(0, min(self.per, self.C - self.rank * self.per)):].any(), "a peer counts a padding campaign"
        lo = self.rank * self.per
        total = cur["send"][lo:lo + self.per].astype(object) + pb.astype(object).sum(axis=0)
        assert int(total.max()) <= MAXVAL[cur["width"]], "the ranks' cells wrap the agreed width"
        recv = total.astype(U64)
        self.peer_cells += int(pb.sum(dtype=U64))
        self.unpack(cur["aligned"], recv, cur["width"])
        return recv

    def unpack(self, aligned, recv, width=1):
        idx = np.asarray(aligned, dtype=np.int64)
        self.owned[:, idx] += recv
        o = self.acc8[:, idx]
        s = o + recv
        over = (s > U64(255)) & (recv > 0)
        if width == 1:
            oi, vi = o.astype(np.int64), recv.astype(np.int64)
            self.carry_cases += int((over & (((oi ^ vi) & 0x80) != 0) & ((oi & 0x7F) + (vi & 0x7F) >= 128)).sum())
        self.acc8_past_127 += int(((o < U64(128)) & (s >= U64(128)) & ~over).sum())
        self.acc8_past_255 += int(over.sum())
        self.acc8[:, idx] = np.where(over, U64(0), s)

    # -- what a drain reports -----------------------------------------------------------
    def drain_table(self):
        """[C][W]: this rank's pending counts plus its owned block (campaign rows only)."""
        t = self.pending[:self.C].copy()
        lo = self.rank * self.per
        hi = min(lo + self.per, self.C)
        if hi > lo:
            t[lo:hi] += self.owned[:hi - lo]
        return t

    def conserved(self):
        """owned + pending + sent to other blocks == counts put in + the peers' cells."""
        have = int(self.owned.sum(dtype=U64)) + int(self.pending.sum(dtype=U64)) + self.sent_away
        return have == self.counted + self.peer_cells


def peer_blocks(seed, bound, nranks, per, valid_rows, fill=0.5, lean=3):
    """N - 1 peer blocks [nranks - 1][per][R] for one rank's rows: every cell at most its
    slot's bound (`bound[R]`: the peers' agreed maximum, or a pipelined pack's cap), rows from
    valid_rows on (the padding campaigns no rank counts) zero.  About `fill` of the cells are
    nonzero, spread over [0, bound] (lean 1: evenly; larger: towards small values); each slot with a nonzero bound holds the bound itself in at least one cell, so
    the maxima are what was agreed."""
    rng = np.random.default_rng(seed)
    b = np.asarray([int(v) for v in bound], dtype=U64)
    R = b.size
    out = np.zeros((max(nranks - 1, 0), per, R), dtype=U64)
    if nranks < 2 or valid_rows <= 0 or R == 0:
        return out
    u = rng.random(out.shape)
    # cells over the whole range [0, bound], a tenth of them at the bound itself
    val = np.floor((u ** lean) * (b.astype(np.float64) + 1.0)).astype(U64)
    val = np.minimum(val, b)
    val = np.where(rng.random(out.shape) < 0.1, b, val)
    val = np.where(rng.random(out.shape) < fill, val, U64(0))
    val[:, valid_rows:, :] = 0
    for k in range(R):
        if b[k]:
            val[rng.integers(0, nranks - 1), rng.integers(0, valid_rows), k] = b[k]
    assert (val <= b).all()
    return val


class SimulatedPeers:
    """The two collectives of YsbContext.group_init_host_fns with the other nranks - 1 ranks
    played by an ExchangeModel and peer_blocks: every buffer the library hands over is
    compared with the model's, cell by cell, and a mismatch raises (the binding keeps it in
    ctx.callback_error and fails the call).

    Before each exchange the test sets
        next_peer_max   uint64[W], the peers' per-slot maxima of this call's plan
        next_pipelined  whether the call is ysb_group_exchange_pipelined
        next_bound      optional {slot: bound} for the peers' cells of this call's pack (default:
                        the maxima the packed plan was agreed with, at most the cap)
        next_override   optional callable(blocks [N-1][per][R], aligned slots) editing the cells
    """

    def __init__(self, model, seed=1):
        self.m = model
        self.seed = seed
        self.calls = 0
        self.rs_calls = 0
        self.next_peer_max = np.zeros(model.W, dtype=U64)
        self.next_pipelined = False
        self.next_bound = None
        self.next_override = None
        self.prev_peer_max = np.zeros(model.W, dtype=U64)
        self.cur = None
        self.last_recv = None
        self.fill, self.lean = 0.5, 3   # peer_blocks' density and spread
        self.log = []

    def allreduce_max(self, buf):
        m = self.m
        if buf.size != m.W:   # the ring-base agreement: one rank's word is everyone's
            return
        own = m.slot_max()
        if not np.array_equal(buf, own):
            bad = np.nonzero(buf != own)[0]
            raise AssertionError("xplan maxima differ from the model at slots %s: %s vs %s"
                                 % (bad[:8], buf[bad[:8]], own[bad[:8]]))
        pm = np.asarray(self.next_peer_max, dtype=U64)
        pipelined = self.next_pipelined and m.have_plan
        used_pm = self.prev_peer_max if pipelined else pm
        self.cur = m.begin(pm, self.next_pipelined)
        self.cur_bound = used_pm
        self.prev_peer_max = pm
        np.maximum(buf, pm, out=buf)
        self.calls += 1
        self.log.append({"aligned": list(self.cur["aligned"]), "width": self.cur["width"],
                         "buckets": len(self.cur["slots"]), "pipelined": self.cur["pipelined"]})

    def reduce_scatter_sum(self, send, count, width):
        m, cur = self.m, self.cur
        self.rs_calls += 1
        assert m.cur is not None, "a reduce-scatter the model does not expect (empty plan)"
        R = len(cur["aligned"])
        assert count == m.per * R, "count %d, the model's per * R is %d * %d" % (count, m.per, R)
        assert width == cur["width"], "width %d, the model's %d" % (width, cur["width"])
        got = send.view(CELL[width]).reshape(m.c_pad, R).astype(U64)
        exp = cur["send"]
        if not np.array_equal(got, exp):
            r, k = np.nonzero(got != exp)
            raise AssertionError("send buffer differs from the model in %d cells, first (row %d, slot %d): %d vs %d"
                                 % (r.size, r[0], cur["aligned"][k[0]], got[r[0], k[0]], exp[r[0], k[0]]))
        assert not got[m.C:].any(), "padding rows must send zeros"
        bound = np.array([int(self.cur_bound[s]) for s in cur["aligned"]], dtype=object)
        if cur["cap"] is not None:
            bound = np.minimum(bound, cur["cap"])
        if self.next_bound:
            for s, v in self.next_bound.items():
                bound[cur["aligned"].index(s)] = v
        lo = m.rank * m.per
        blocks = peer_blocks(self.seed + 1000 * self.calls, bound, m.N, m.per, max(0, min(m.per, m.C - lo)),
                             self.fill, self.lean)
        if self.next_override:
            self.next_override(blocks, cur["aligned"])
        self.last_recv = m.finish(blocks, bound)
        return self.last_recv.astype(CELL[width])
