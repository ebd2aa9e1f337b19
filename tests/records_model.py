"""A plain model of record-mode counting (csrc/ysb_count.hip, the REC staging of ysb_scan.hip,
csrc/ysb_recplan.h): which scan workgroup reads which line, how many records each (workgroup,
bin) sub-buffer keeps and how many views fall back to the atomics, the partition's run length
per (block, slice), whether a count block runs dense or sparse, and every cell's u8 delta byte
and u64 ring cell after each launch -- so a test can tell not only that the counts are exact
but which device path made them so.

Pure Python and numpy: no GPU, no library call.  Everything is an unsigned integer and exact.
Cells are kept sparsely (dicts keyed by the ring cell index campaign * W + (bucket & (W - 1))),
so a 67M-cell ring costs what its touched cells cost.

Two things the device decides by timing are outside the model and a test has to avoid them:
  * which records of a (workgroup, bin) fill its sub-buffer once it overflows, when the bin has
    more than one block (the model keeps the first `cap` in line order; the device the first in
    arrival order within a half tile) -- `Launch.ambiguous` says when the runs depend on it;
  * lines the fast tiers do not take (the deferred-line kernel counts them with atomics and
    sets dirty): a test asserts stats()["deferred"] == 0.
"""
from __future__ import annotations

from collections import Counter

import numpy as np

TILE_LINES = 64
MAX_TILES_PER_BLOCK = 128
REC_BLOCK_CELLS = 32768
REC_BINS_MAX = 8
REC_SUB_MAX = 512
REC_QUARTERS = 64
REC_SLICE_MAX = 128
SCAN_WG_PER_CU = 8


def n_tiles(n_lines):
    return (n_lines + TILE_LINES - 1) // TILE_LINES


def grid_of(seg_lines, cus):
    """The scan's grid for a launch of segments of seg_lines lines on `cus` compute units (static
    split: ysb_submit.cpp make_params): whole rounds of resident workgroups, at most one per tile
    of the largest segment."""
    resident = cus * SCAN_WG_PER_CU
    most = max(n_tiles(n) for n in seg_lines)
    rounds = max(1, (most + resident * MAX_TILES_PER_BLOCK - 1) // (resident * MAX_TILES_PER_BLOCK))
    return max(1, min(most, rounds * resident))


def tiles_per_wg_max(seg_lines, grid):
    """What the plan sizes the sub-buffers by: per segment q tiles, one more where any workgroup
    has one more."""
    return sum(n_tiles(n) // grid + (1 if n_tiles(n) % grid else 0) for n in seg_lines)


def plan_of(c_pad, W, grid, tiles):
    """ysb_recplan.h rec_plan restated: the plan as a dict, or None where record mode cannot run."""
    if W > REC_BLOCK_CELLS or c_pad * W >= 1 << 32:
        return None
    l2c = REC_BLOCK_CELLS // W
    n_blocks = -(-c_pad // l2c)
    S = 1
    while S * REC_BINS_MAX < n_blocks:
        S *= 2
    if S > REC_SUB_MAX:
        return None
    bins = -(-n_blocks // S)
    slices = -(-grid // REC_QUARTERS)
    if slices > REC_SLICE_MAX:
        return None
    per_bin = -(-(tiles * TILE_LINES * 3 // 4) // bins)
    cap = max(32, -(-per_bin // 32) * 32)
    area = -(-(slices * cap + 32 * S) // 32) * 32
    part = bins * REC_QUARTERS * area
    if part >= 1 << 32:
        return None
    return {"w_log2": W.bit_length() - 1, "blk_shift": l2c.bit_length() - 1, "n_blocks": n_blocks,
            "sub_log2": S.bit_length() - 1, "bins": bins, "cap": cap, "grid": grid, "slices": REC_QUARTERS,
            "area": area, "part": part}


def tile_split(seg_lines, grid):
    """The scan workgroup of every line of a launch (static split): for each segment of n lines,
    n_tiles = ceil(n / 64) and workgroup w takes tiles [w * q + min(w, r), ...) with
    q, r = divmod(n_tiles, grid).  int64 array over the segments' lines in order."""
    out = []
    for n in seg_lines:
        q, r = divmod(n_tiles(n), grid)
        tile = np.arange(n, dtype=np.int64) // TILE_LINES
        # tiles [0, r * (q + 1)) belong to the r workgroups of q + 1 tiles
        big = r * (q + 1)
        wg = np.where(tile < big, tile // (q + 1), r + (tile - big) // max(q, 1))
        out.append(wg)
    return np.concatenate(out) if out else np.zeros(0, dtype=np.int64)


def slice_of_wg(grid):
    """The partition slice of every scan workgroup: slice q holds [q * grid / 64, (q + 1) * grid / 64)."""
    lo = np.arange(REC_QUARTERS, dtype=np.int64) * grid // REC_QUARTERS
    return np.searchsorted(lo, np.arange(grid, dtype=np.int64), side="right") - 1


def add16(byte, n):
    """One cell of ysb_count.hip add16: (new byte, added to the u64 ring cell, spilled)."""
    s = byte + n
    if s > 255:
        return 0, s, True
    return s, 0, False


class Launch:
    """What one launch did, as the model sees it."""

    def __init__(self):
        self.views = None        # [grid][bins] in-ring joined views per (workgroup, bin)
        self.rec_n = None        # [grid][bins] records kept = min(views, cap)
        self.fallback = 0        # in-ring joined views counted by the atomics instead
        self.run_len = None      # [n_blocks][REC_QUARTERS] records per (block, slice)
        self.total = None        # [n_blocks] records per block
        self.dense = None        # [n_blocks] bool: total * 16 >= cells
        self.spills = 0          # cells whose byte passed 255 in this launch
        self.outside = 0         # joined views outside the ring (side map / list)
        self.dirty = 0           # *d_dirty after the launch
        self.ambiguous = False   # an overflowing sub-buffer in a bin of several blocks


class RecordsModel:
    def __init__(self, c_pad, W, ring_base):
        assert W >= 16 and W & (W - 1) == 0
        self.c_pad, self.W, self.base = c_pad, W, ring_base
        self.byte = {}            # cell -> u8 delta byte (non-zero only)
        self.ring = Counter()     # cell -> u64 ring cell
        self.side = Counter()     # (campaign, bucket) outside the ring
        self.dirty = 0

    # -- cells ---------------------------------------------------------------------------------
    def cell_of(self, campaign, bucket):
        return campaign * self.W + (bucket & (self.W - 1))

    def cell_key(self, cell):
        """(campaign, bucket) of a ring cell: the one bucket of [base, base + W) in its slot."""
        c, slot = divmod(cell, self.W)
        return c, self.base + ((slot - self.base) & (self.W - 1))

    # -- one launch ----------------------------------------------------------------------------
    def launch(self, camp, bucket, plan, seg_lines):
        """camp: per line the campaign of a joined view, -1 (or None) for any other line;
        bucket: per line its bucket (ignored where camp < 0); plan: record_info's descriptor (or
        plan_of's dict); seg_lines: the segments' line counts, in order."""
        camp = np.array([-1 if c is None else c for c in camp], dtype=np.int64)
        bucket = np.array(bucket, dtype=np.int64)
        assert camp.size == bucket.size == sum(seg_lines)
        assert camp.max(initial=-1) < self.c_pad
        W, grid, bins, cap = self.W, plan["grid"], plan["bins"], plan["cap"]
        assert 1 << plan["w_log2"] == W
        blk_of_cell = plan["w_log2"] + plan["blk_shift"]
        L = Launch()
        wg = tile_split(seg_lines, grid)
        assert wg.size == camp.size and (wg.size == 0 or wg.max() < grid)
        joined = camp >= 0
        inside = joined & (bucket >= self.base) & (bucket < self.base + W)
        for c, b in zip(camp[joined & ~inside].tolist(), bucket[joined & ~inside].tolist()):
            self.side[(c, b)] += 1
        L.outside = int((joined & ~inside).sum())
        idx = np.flatnonzero(inside)
        r_wg, r_camp = wg[idx], camp[idx]
        r_cell = r_camp * W + (bucket[idx] & (W - 1))
        r_bin = r_camp >> (plan["blk_shift"] + plan["sub_log2"])
        assert r_bin.size == 0 or r_bin.max() < bins
        group = r_wg * bins + r_bin
        L.views = np.bincount(group, minlength=grid * bins).reshape(grid, bins)
        L.rec_n = np.minimum(L.views, cap)
        L.fallback = int((L.views - L.rec_n).sum())
        # the records kept: the first `cap` of each (workgroup, bin) in line order
        order = np.argsort(group, kind="stable")
        start = np.concatenate([[0], np.cumsum(L.views.reshape(-1))[:-1]])
        rank = np.empty(group.size, dtype=np.int64)
        rank[order] = np.arange(group.size) - start[group[order]]
        kept = rank < cap
        r_blk = r_cell >> blk_of_cell
        if (~kept).any() and plan["sub_log2"] > 0:
            over = np.unique(group[~kept])
            for gk in over.tolist():
                if np.unique(r_blk[group == gk]).size > 1:
                    L.ambiguous = True
        n_blocks = plan["n_blocks"]
        sl = slice_of_wg(grid)
        L.run_len = np.bincount(r_blk[kept] * REC_QUARTERS + sl[r_wg[kept]],
                                minlength=n_blocks * REC_QUARTERS).reshape(n_blocks, REC_QUARTERS)
        L.total = L.run_len.sum(axis=1)
        l2c = 1 << plan["blk_shift"]
        cells = np.minimum(l2c, self.c_pad - np.arange(n_blocks, dtype=np.int64) * l2c) * W
        L.dense = L.total * 16 >= cells
        # the atomics' share straight into the u64 ring; the records through add16
        for cell in r_cell[~kept].tolist():
            self.ring[cell] += 1
        if L.fallback:
            self.dirty = 1
        for cell, n in Counter(r_cell[kept].tolist()).items():
            b, add, spilled = add16(self.byte.get(cell, 0), n)
            if b:
                self.byte[cell] = b
            else:
                self.byte.pop(cell, None)
            if spilled:
                self.ring[cell] += add
                L.spills += 1
                self.dirty = 1
        L.dirty = self.dirty
        return L

    # -- reads ---------------------------------------------------------------------------------
    def fold(self):
        """What every read of the u64 ring does first: ring += byte, byte = 0."""
        for cell, b in self.byte.items():
            self.ring[cell] += b
        self.byte = {}

    def table(self):
        """{(campaign, bucket): count} as a drain returns it (the fold included)."""
        self.fold()
        out = Counter()
        for cell, v in self.ring.items():
            if v:
                out[self.cell_key(cell)] += v
        for k, v in self.side.items():
            if v:
                out[k] += v
        return dict(out)

    def clear(self):
        """A drain with clear: every count gone (dirty stays: only a reset or an exchange clears it)."""
        self.byte = {}
        self.ring = Counter()
        self.side = Counter()
