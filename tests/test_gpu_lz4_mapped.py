"""GPU: LZ4 batches read in place from registered host memory (ysb_submit_lz4_mapped: the
compressed form of ysb_submit_raw_mapped and ysb_submit_mapped) -- FileBasedDataSource.run
(AdvertisingTopologyNative.java:144-165) over a compressed replay file whose mapping is pinned:
runs of whole blocks at every byte alignment against the slot path (ysb_submit_raw_lz4) and the
generator truth, the rebase behind the decode with the GPU split and with device offsets, block
shapes, a bad block, the argument errors, the bytes that cross the link, the .tbl format, and
the Python container source."""
import numpy as np
import pytest

import golden_data as gd
import lz4_model as M
from test_gpu_mapped import T0, aligned, ctx_for, time_table
from test_gpu_parity import check_against, make_ctx
from ysb_amd import GenParams, Lz4FileDataSource, YsbContext, YsbError, lz4

pytestmark = pytest.mark.gpu

SLOT = 32 << 20   # max_batch_bytes of the tests' contexts (the pinned slots are allocated whole)


def gen(n):
    g = GenParams(events_per_sec=100_000, with_skew=2)
    data, off = g.events_host(0, n)
    return g, data, off


def place_runs(blob, directory, cuts, tail_pad=64):
    """Runs of blocks [cuts[i], cuts[i + 1]) of one packed buffer placed in one 64-byte aligned
    array so that run i starts at byte residue i % 16: (array, [(byte offset, comp bytes, first
    block, blocks)])."""
    comp = (directory[:, 0] & 0x7FFFFFFF).astype(np.int64)
    start = np.concatenate(([0], np.cumsum(comp)))
    runs, pos = [], 0
    for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        pos += (i % 16 - pos) % 16
        nb = int(start[b] - start[a])
        runs.append((pos, nb, a, b - a))
        pos += nb
    buf = aligned(pos + tail_pad)
    for (p, nb, a, _) in runs:
        buf[p:p + nb] = blob[start[a]:start[a] + nb]
    return buf, runs


def pack_parts(data, off, n_parts, block):
    """The lines cut into n_parts batches at line boundaries, each packed on its own: (blob,
    directory, block cuts, [(first line, lines)])."""
    n = off.size
    lines = [n * i // n_parts for i in range(n_parts + 1)]
    ends = np.append(off[1:], len(data)).astype(np.int64)
    blobs, dirs, cuts, parts = [], [], [0], []
    for a, b in zip(lines[:-1], lines[1:]):
        bl, d = lz4.pack(data[off[a]:ends[b - 1]], block)
        blobs.append(bl)
        dirs.append(d)
        cuts.append(cuts[-1] + d.shape[0])
        parts.append((a, b - a))
    return np.concatenate(blobs), np.concatenate(dirs), cuts, parts


def submit_runs(ctx, buf, runs, directory):
    for i, (p, nb, a, k) in enumerate(runs):
        ctx.submit_lz4_mapped(buf, p, nb, directory[a:a + k], slot=i % 2)
    ctx.sync()


def check_truth(ctx, g, n, views=True):
    st = ctx.stats()
    assert st["events"] == n and st["parse_errors"] == 0 and st["deferred"] == 0
    ctx.truth_accumulate(g, 0, n)
    mism, truth, ring = ctx.truth_compare()
    assert mism == 0 and truth == ring and (truth > 0 or not views)


# ---- 1. counts equal the slot path's and the truth, at every alignment -----------------------

def test_runs_at_every_alignment_count_like_the_slot_path():
    g, data, off = gen(60_000)
    blob, d = lz4.pack(data, 8192, line_aligned=True)
    nblk = d.shape[0]
    assert nblk > 200
    # 20 runs of exactly one block, then 32 runs of the rest, cut at block boundaries
    cuts = list(range(21)) + [20 + (nblk - 20) * i // 32 for i in range(1, 33)]
    assert len(cuts) - 1 >= 48 and cuts[-1] == nblk
    buf, runs = place_runs(blob, d, cuts)
    assert {p % 16 for p, _, _, _ in runs} == set(range(16))
    assert any(k == 1 for _, _, _, k in runs)
    before = buf.copy()
    with ctx_for(g, max_batch_bytes=SLOT) as a, ctx_for(g, max_batch_bytes=SLOT) as b:
        a.host_register(buf)
        submit_runs(a, buf, runs, d)
        for i, (p, nb, x, k) in enumerate(runs):
            b.submit_raw_lz4(buf[p:p + nb], d[x:x + k], slot=i % 2)
        b.sync()
        got = a.drain()
        assert got == b.drain() and sum(got.values()) > 0
        sa, sb = a.stats(), b.stats()
        for key in ("events", "parse_errors", "deferred"):
            assert sa[key] == sb[key], key
        ia, ib = a.lz4_info(), b.lz4_info()
        assert ia["batches"] == ib["batches"] == len(runs) and ia["bad_blocks"] == 0
        assert ia["comp_bytes"] == ib["comp_bytes"] == runs[-1][1] and ia["decode_ms"] > 0
        check_truth(a, g, off.size)
        a.host_unregister(buf)
    assert (buf == before).all()   # the source is only read


# ---- 2. the rebase behind the decode ---------------------------------------------------------

@pytest.fixture(scope="module")
def rebase_case():
    """30k events packed line-aligned at 8 KiB, five runs of blocks; every run's raw start, first
    line and lines (a line-aligned run starts at a line start), each line's offset in its run."""
    g, data, off = gen(30_000)
    tab, base = time_table(data, off)
    blob, d = lz4.pack(data, 8192, line_aligned=True)
    nblk = d.shape[0]
    cuts = [nblk * i // 5 for i in range(6)]
    buf, runs = place_runs(blob, d, cuts)
    raw_at = np.concatenate(([0], np.cumsum(d[:, 1].astype(np.int64))))
    lines, lo = [], np.empty(off.size, dtype=np.uint32)
    for a, b in zip(cuts[:-1], cuts[1:]):
        la, lb = int(np.searchsorted(off, raw_at[a])), int(np.searchsorted(off, raw_at[b]))
        assert off[la] == raw_at[a]
        lines.append((la, lb - la))
        lo[la:lb] = off[la:lb] - raw_at[a]
    assert sum(n for _, n in lines) == off.size
    return g, off, tab, base, buf, runs, d, lines, lo


@pytest.mark.parametrize("offsets", [False, True])
@pytest.mark.parametrize("shift", [0, 1, 37])
def test_rebase_behind_the_decode(rebase_case, shift, offsets):
    g, off, tab, base, buf, runs, d, lines, lo = rebase_case
    before = buf.copy()
    with ctx_for(g, max_batch_bytes=SLOT) as ctx:
        ctx.host_register(buf)
        ctx.rebase_table(tab, base)
        d_lo = ctx.device_alloc(lo.nbytes + 64)
        ctx.h2d(d_lo, lo)
        for i, ((p, nb, x, k), (la, n)) in enumerate(zip(runs, lines)):
            if offsets:
                ctx.submit_lz4_mapped(buf, p, nb, d[x:x + k], slot=i % 2, d_off=d_lo + 4 * la, n=n, rebase=(la, shift))
            else:
                ctx.submit_lz4_mapped(buf, p, nb, d[x:x + k], slot=i % 2, rebase=(la, shift))
        ctx.sync()
        check_truth(ctx, GenParams(events_per_sec=100_000, with_skew=2, t0_ms=T0 + shift * 10_000), off.size)
        ctx.device_free(d_lo)
    assert (buf == before).all()


def test_rebase_lines_past_the_table(rebase_case):
    g, off, tab, base, buf, runs, d, lines, lo = rebase_case
    p, nb, x, k = runs[0]
    la, n = lines[0]
    with ctx_for(g, max_batch_bytes=SLOT) as ctx:
        ctx.host_register(buf)
        ctx.rebase_table(tab[:100], base)
        d_lo = ctx.device_alloc(lo.nbytes + 64)
        ctx.h2d(d_lo, lo)
        assert n > 100
        with pytest.raises(YsbError, match="YSB_ERR_ARG"):     # with offsets: at the call
            ctx.submit_lz4_mapped(buf, p, nb, d[x:x + k], d_off=d_lo, n=n, rebase=(0, 1))
        with pytest.raises(YsbError, match="YSB_ERR_ARG"):
            ctx.submit_lz4_mapped(buf, p, nb, d[x:x + k], d_off=d_lo, n=50, rebase=(51, 1))
        assert ctx.stats()["events"] == 0
        ctx.submit_lz4_mapped(buf, p, nb, d[x:x + k], rebase=(0, 1))   # with the split: at the launch
        for call in (ctx.sync, ctx.stats):
            with pytest.raises(YsbError, match="rebase table") as e:
                call()
            assert e.value.code == -1
        ctx.reset()
        ctx.rebase_table(tab, base)
        ctx.submit_lz4_mapped(buf, p, nb, d[x:x + k], rebase=(0, 0))
        assert ctx.stats()["events"] == n
        ctx.device_free(d_lo)


# ---- 3. block shapes ---------------------------------------------------------------------

@pytest.mark.parametrize("block,n", [(64, 3000), (1024, 10_000), (65536, 30_000)])
def test_block_sizes(block, n):
    g, data, off = gen(n)
    blob, d, cuts, parts = pack_parts(data, off, 3, block)
    stored = int(((d[:, 0] & lz4.STORED) != 0).sum())
    if block == 64:
        assert 0 < stored and d.shape[0] > 5000   # mostly stored blocks: some are
    if block == 65536:
        assert int(d[:, 1].max()) == 65536
    buf, runs = place_runs(blob, d, cuts)
    with ctx_for(g, max_batch_bytes=SLOT) as ctx:
        ctx.host_register(buf)
        submit_runs(ctx, buf, runs, d)
        info = ctx.lz4_info()
        assert info["bad_blocks"] == 0 and info["blocks"] == runs[-1][3]
        check_truth(ctx, g, n)


def test_one_line_no_block_and_the_range_end():
    g, data, off = gen(2000)
    one, e1 = lz4.compress_block(bytes(data[:off[1]]))          # one block holding one line
    blob, d = lz4.pack(data, 8192, line_aligned=True)
    for lead in (0, 5, 11):
        # the batch ends `lead` bytes before the end of a registered range of whole 16 bytes:
        # its widened span ends exactly at the range's end
        total = (blob.size + lead + 15) // 16 * 16
        buf = aligned(total)[:total]
        at = total - lead - blob.size
        buf[at:at + blob.size] = blob
        with ctx_for(g, max_batch_bytes=SLOT) as ctx:
            ctx.host_register(buf)
            ctx.submit_lz4_mapped(buf, at, blob.size, d, slot=0)
            ctx.submit_lz4_mapped(buf, 0, 0, np.empty((0, 2), dtype=np.uint32), slot=1)   # n_blocks = 0
            ctx.sync()
            info = ctx.lz4_info()
            assert info["batches"] == 2 and info["blocks"] == 0
            check_truth(ctx, g, off.size)
            with pytest.raises(YsbError, match="registered range"):
                ctx.submit_lz4_mapped(buf, at, blob.size + lead + 1, d)   # one byte past the range
    buf = aligned(len(one) + 32)
    buf[3:3 + len(one)] = np.frombuffer(one, dtype=np.uint8)
    with ctx_for(g, max_batch_bytes=SLOT) as ctx:
        ctx.host_register(buf)
        ctx.submit_lz4_mapped(buf, 3, len(one), np.array([e1], dtype=np.uint32))
        check_truth(ctx, g, 1, views=False)   # (one event: it need not be a view)


# ---- 4. a bad block --------------------------------------------------------------------------

def malformed(name):
    for nm, comp, raw in M.malformed_blocks():
        if nm == name:
            return comp, raw
    raise KeyError(name)


@pytest.mark.parametrize("name", ["offset 0", "a literal length of 64 KiB of 255s", "match length exactly 19, cut at 5"])
def test_a_bad_block_drops_its_batch(name):
    g, data, off = gen(30_000)
    blob, d, cuts, parts = pack_parts(data, off, 2, 8192)
    comp = (d[:, 0] & 0x7FFFFFFF).astype(np.int64)
    start = np.concatenate(([0], np.cumsum(comp)))
    # the second batch with its block 7 replaced by the malformed entry
    k = cuts[1] + 7
    bad_comp, bad_raw = malformed(name)
    bad_blob = np.concatenate([blob[start[cuts[1]]:start[k]], np.frombuffer(bad_comp, dtype=np.uint8), blob[start[k + 1]:]])
    bad_d = d[cuts[1]:].copy()
    bad_d[7] = (len(bad_comp), bad_raw)
    assert M.decode_batch(bad_blob.tobytes(), [(int(c), int(r)) for c, r in bad_d])[1] == 7
    all_blob = np.concatenate([blob, bad_blob])
    all_d = np.concatenate([d, bad_d])
    buf, runs = place_runs(all_blob, all_d, cuts + [all_d.shape[0]])
    good0, good1, bad1 = runs
    with ctx_for(g, max_batch_bytes=SLOT) as ctx:
        ctx.host_register(buf)
        ctx.submit_lz4_mapped(buf, good0[0], good0[1], all_d[good0[2]:good0[2] + good0[3]], slot=0)
        first = ctx.stats()
        assert first["events"] == parts[0][1]
        rows = ctx.drain()
        ctx.submit_lz4_mapped(buf, bad1[0], bad1[1], all_d[bad1[2]:bad1[2] + bad1[3]], slot=1)   # launches nothing yet
        with pytest.raises(YsbError) as e:
            ctx.submit_lz4_mapped(buf, good0[0], good0[1], all_d[good0[2]:good0[2] + good0[3]], slot=0)   # its launch
        assert e.value.code == -5 and "block 7" in str(e.value)
        for call in (ctx.sync, ctx.stats, lambda: ctx.submit_lz4_mapped(buf, good1[0], good1[1], d[cuts[1]:], slot=1)):
            with pytest.raises(YsbError) as e:
                call()
            assert e.value.code == -5 and "block 7" in str(e.value)
        ctx.reset()
        assert ctx.lz4_info()["batches"] == 0
        submit_runs(ctx, buf, [good0, good1], all_d)
        check_truth(ctx, g, off.size)
    # what was counted before the bad batch is the first batch alone: none of the bad one's lines
    with ctx_for(g, max_batch_bytes=SLOT) as ctx:
        ctx.submit_raw(data[:off[parts[1][0]]], slot=0)
        assert ctx.stats() == first and ctx.drain() == rows


def test_each_slot_takes_every_kind_of_batch_in_turn():
    """One context, tests/golden/gen_s7.jsonl in six batches of 250 lines on alternating slots:
    slot 0 takes a plain raw batch, a compressed one in place with device offsets and a rebase,
    a compressed one in place with the GPU split and no rebase; slot 1 a compressed slot batch, a
    mapped raw one with a rebase, a plain raw one.  Nothing of a slot's earlier batch outlives
    its launch: with a rebase of 0 buckets the counts are the file's golden counts, and the
    last compressed batch's figures are the fifth batch's.  Then a malformed compressed batch and a
    plain raw batch behind it on its slot: the error is sticky, and after ysb_reset the plain
    batch alone counts exactly."""
    raw, offs = gd.events("gen_s7")
    exp = gd.expected("gen_s7")
    data = np.frombuffer(raw, dtype=np.uint8)
    off = np.asarray(offs, dtype=np.uint32)
    assert off.size == 1500
    tab, base = time_table(data, off)
    ends = np.append(off[1:], data.size).astype(np.int64)
    part = [data[off[a]:ends[a + 249]] for a in range(0, 1500, 250)]
    packed = {i: lz4.pack(part[i], 64) for i in (1, 2, 4)}
    assert all(d.shape[0] > 500 for _, d in packed.values())   # many blocks each
    # what is read in place, each at another byte residue of one registered array
    items, at, pos = [packed[2][0], part[3], packed[4][0]], [], 0
    for k, it in enumerate(items):
        pos += (4 * k + 3 - pos) % 16
        at.append(pos)
        pos += it.size
    buf = aligned(pos)
    for p, it in zip(at, items):
        buf[p:p + it.size] = it
    lo = (off[500:750] - off[500]).astype(np.uint32)   # batch 3's line offsets in its decoded bytes
    with make_ctx(max_batch_bytes=SLOT) as ctx:
        ctx.host_register(buf)
        ctx.rebase_table(tab, base)
        d_lo = ctx.device_alloc(lo.nbytes + 64)
        ctx.h2d(d_lo, lo)
        ctx.submit_raw(part[0], slot=0)
        ctx.submit_raw_lz4(*packed[1], slot=1)
        ctx.submit_lz4_mapped(buf, at[0], items[0].size, packed[2][1], slot=0, d_off=d_lo, n=250, rebase=(500, 0))
        ctx.submit_raw_mapped(buf, at[1], items[1].size, slot=1, rebase=(750, 0))
        ctx.submit_lz4_mapped(buf, at[2], items[2].size, packed[4][1], slot=0)
        ctx.submit_raw(part[5], slot=1)
        info = ctx.lz4_info()
        blob5, d5 = packed[4]
        assert info["batches"] == 3 and info["bad_blocks"] == 0 and info["first_bad"] is None
        assert info["blocks"] == d5.shape[0] and info["stored_blocks"] == int(((d5[:, 0] & lz4.STORED) != 0).sum())
        assert info["comp_bytes"] == blob5.size and info["raw_bytes"] == part[4].size
        check_against(ctx, *exp)
        bad_comp, bad_raw = malformed("offset 0")
        ctx.submit_raw_lz4(bad_comp, [(len(bad_comp), bad_raw)], slot=1)   # launches nothing yet
        with pytest.raises(YsbError) as e:
            ctx.submit_raw(raw, slot=1)                                    # its slot's earlier batch first: dropped
        assert e.value.code == -5 and "block 0" in str(e.value)
        for call in (ctx.sync, ctx.stats):
            with pytest.raises(YsbError) as e:
                call()
            assert e.value.code == -5 and "block 0" in str(e.value)
        ctx.reset()
        ctx.submit_raw(raw, slot=1)
        check_against(ctx, *exp)
        ctx.device_free(d_lo)


# ---- 5. argument errors --------------------------------------------------------------------

def test_argument_errors():
    g, data, off = gen(2000)
    blob, d = lz4.pack(data, 8192, line_aligned=True)
    buf = aligned(blob.size + 64)
    buf[8:8 + blob.size] = blob
    view = buf[8:8 + blob.size]

    def code(fn):
        with pytest.raises(YsbError) as e:
            fn()
        return e.value.code

    with ctx_for(g, max_batch_bytes=SLOT) as ctx:
        assert code(lambda: ctx.submit_lz4_mapped(buf, 8, blob.size, d)) == -1            # not registered
        ctx.host_register(view)
        with pytest.raises(YsbError, match="registered range"):                            # the widened span leaves it
            ctx.submit_lz4_mapped(view, 0, blob.size, d)
        ctx.host_unregister(view)
        ctx.host_register(buf)
        assert code(lambda: ctx.submit_lz4_mapped(buf, 8, blob.size, d, slot=2)) == -1
        assert code(lambda: ctx.submit_lz4_mapped(buf, 8, blob.size - 1, d)) == -1        # the sums do not match
        assert code(lambda: ctx.submit_lz4_mapped(buf, 8, blob.size, d[:-1])) == -1
        for raw in (0, 65537):
            bad = d.copy()
            bad[1, 1] = raw
            assert code(lambda: ctx.submit_lz4_mapped(buf, 8, blob.size, bad)) == -1, raw
        d_lo = ctx.device_alloc(4 * off.size + 64)
        assert code(lambda: ctx.submit_lz4_mapped(buf, 8, blob.size, d, d_off=d_lo, n=0)) == -1    # d_off without n
        assert code(lambda: ctx.submit_lz4_mapped(buf, 8, blob.size, d, n=off.size)) == -1         # n without d_off
        assert code(lambda: ctx.submit_lz4_mapped(buf, 8, blob.size, d, rebase=(0, 1))) == -3      # no rebase table
        assert code(lambda: ctx.submit_lz4_mapped(buf, 8, blob.size, d, d_off=d_lo, n=off.size, rebase=(0, 1))) == -3
        # none of them left anything behind: the batch counts
        ctx.submit_lz4_mapped(buf, 8, blob.size, d)
        check_truth(ctx, g, off.size)
        ctx.device_free(d_lo)
    with ctx_for(g, max_batch_bytes=1 << 16) as ctx:                                       # decoded total over the slot
        ctx.host_register(buf)
        assert int(d[:, 1].sum()) > 1 << 16 and blob.size > 1 << 16
        assert code(lambda: ctx.submit_lz4_mapped(buf, 8, blob.size, d)) == -4
        k = 1 + (1 << 16) // 8192
        few = int((d[:k, 0] & 0x7FFFFFFF).sum())
        assert few <= 1 << 16 < int(d[:k, 1].sum())                                        # compressed fits, decoded does not
        assert code(lambda: ctx.submit_lz4_mapped(buf, 8, few, d[:k])) == -4
    with YsbContext() as ctx:                                                              # no ad map yet
        ctx.host_register(buf)
        assert code(lambda: ctx.submit_lz4_mapped(buf, 8, blob.size, d)) == -3


# ---- 6. only compressed bytes cross the link -----------------------------------------------

def test_only_compressed_bytes_are_copied():
    g, data, off = gen(30_000)
    blob, d, cuts, parts = pack_parts(data, off, 6, 8192)
    buf, runs = place_runs(blob, d, cuts)
    with ctx_for(g, max_batch_bytes=SLOT) as a, ctx_for(g, max_batch_bytes=SLOT) as b:
        a.host_register(buf)
        a.copy_time()
        b.copy_time()
        submit_runs(a, buf, runs, d)
        for i, (p, nb, x, k) in enumerate(runs):
            b.submit_raw_lz4(buf[p:p + nb], d[x:x + k], slot=i % 2)
        b.sync()
        ms_a, copies_a, bytes_a = a.copy_time()
        ms_b, copies_b, bytes_b = b.copy_time()
        assert copies_a == copies_b == len(runs) and ms_a > 0
        # the blocks and their descriptors, nothing of the raw size
        assert bytes_a == bytes_b and blob.size < bytes_a < blob.size + 64 * d.shape[0] < len(data)
        assert a.stats()["events"] == b.stats()["events"] == off.size


# ---- 7. the .tbl format ------------------------------------------------------------------------

def test_tbl_batches_equal_golden():
    raw, offs = gd.tbl_events("gen_s7_tbl")
    exp = gd.expected("gen_s7_tbl")
    data = np.frombuffer(raw, dtype=np.uint8)
    off = np.asarray(offs, dtype=np.uint32)
    blob, d, cuts, parts = pack_parts(data, off, 4, 1024)
    buf, runs = place_runs(blob, d, cuts)
    with make_ctx(input_format="tbl", max_batch_bytes=SLOT) as ctx:
        ctx.host_register(buf)
        submit_runs(ctx, buf, runs, d)
        check_against(ctx, *exp)


# ---- the Python container source ---------------------------------------------------------------

@pytest.mark.parametrize("cap", [20_000, 1 << 20])
def test_container_source_in_place(tmp_path, cap):
    g, data, off = gen(8000)
    path = tmp_path / "events.json.lz4"
    lz4.write_file(path, data, 4096, line_aligned=True)
    with ctx_for(g, max_batch_bytes=max(cap, 1 << 16)) as ctx:
        with Lz4FileDataSource(str(path)) as src:
            blocks = src.directory.shape[0]
            assert src.run(ctx, cap) == src.size - src.blocks_at
            assert src.batches == len(list(src.runs(cap))) and (cap > 20_000 or src.batches >= blocks // 5)
        check_truth(ctx, g, off.size)
    loose = tmp_path / "loose.json.lz4"
    lz4.write_file(loose, data, 4096, line_aligned=False)
    with pytest.raises(ValueError, match="not line-aligned"):
        Lz4FileDataSource(str(loose))
