"""GPU: LZ4 batches -- the decode kernel alone (ysb_lz4_decode_device) on the CPU tests' corpus
against the pure-Python model tests/lz4_model.py, between canaries and over a pre-filled
buffer; malformed input (only the corpus that tests/test_lz4_logic.py passes through the
sanitized host build of the shared reader); the chain (ysb_submit_raw_lz4 -> split -> scan)
against the golden expectations and ysb_submit_raw on the same bytes; a dropped batch; the
argument and capacity errors."""
import os

import numpy as np
import pytest

import golden_data as gd
import lz4_model as M
from test_gpu_parity import check_against, make_ctx
from ysb_amd import YsbContext, YsbError, lz4

pytestmark = pytest.mark.gpu

CANARY = 4096
FILL = 0x5C


def pack_blocks(blocks):
    """[(compressed bytes, comp field, raw)] -> (blob, directory list)."""
    return b"".join(c for c, _, _ in blocks), [(f, r) for _, f, r in blocks]


def gpu_decode(ctx, blob, directory, out_shift=0, in_shift=0, extra=300):
    """ysb_lz4_decode_device with the output between two 4096-byte canaries of 0xA5 and `extra`
    pre-filled bytes past the raw total; the compressed buffer ends at its allocation's last
    byte.  Returns (output bytes, first bad, the pre-fill past the output)."""
    raw_total = sum(r for _, r in directory)
    span = out_shift + raw_total + extra
    host = np.full(CANARY + span + CANARY, 0xA5, dtype=np.uint8)
    host[CANARY + out_shift:CANARY + span] = FILL
    d_out = ctx.device_alloc(host.size)
    d_in = ctx.device_alloc(in_shift + max(len(blob), 1))
    try:
        ctx.h2d(d_out, host)
        if blob:
            ctx.h2d(d_in + in_shift, np.frombuffer(blob, dtype=np.uint8))
        raw, bad = ctx.lz4_decode_device(d_in + in_shift, len(blob), np.array(directory, dtype=np.uint32).reshape(-1, 2),
                                         d_out + CANARY + out_shift, raw_total + extra)
        assert raw == raw_total
        got = ctx.d2h(np.empty_like(host), d_out)
    finally:
        ctx.device_free(d_out)
        ctx.device_free(d_in)
    assert (got[:CANARY + out_shift] == 0xA5).all() and (got[CANARY + span:] == 0xA5).all(), "canary overwritten"
    assert (got[CANARY + out_shift + raw_total:CANARY + span] == FILL).all(), "bytes past the raw total written"
    return got[CANARY + out_shift:CANARY + out_shift + raw_total].tobytes(), bad


def check_batch(ctx, blob, directory, **kw):
    """The GPU's output against the model's: equal in every good block's range, untouched
    (the pre-fill) in every bad block's; the same first bad block."""
    want, want_bad, ranges = M.decode_batch(blob, directory)
    got, bad = gpu_decode(ctx, blob, directory, **kw)
    assert bad == (None if want_bad == M.NO_BAD else want_bad)
    bad_ranges = 0
    ip = 0
    for (cf, raw), (a, b) in zip(directory, ranges):
        n = cf & ~M.STORED
        if M.is_valid(blob[ip:ip + n], raw, stored=bool(cf & M.STORED)):
            assert got[a:b] == want[a:b], "block at %d decoded wrongly" % a
        else:
            assert got[a:b] == bytes([FILL]) * (b - a), "a bad block wrote into its range"
            bad_ranges += 1
        ip += n
    info = ctx.lz4_info()
    assert info["blocks"] == len(directory) and info["bad_blocks"] == bad_ranges
    assert info["comp_bytes"] == len(blob) and info["raw_bytes"] == len(want)
    assert info["stored_blocks"] == sum(1 for cf, _ in directory if cf & M.STORED)
    return got


@pytest.fixture(scope="module")
def ctx():
    with YsbContext() as c:
        yield c


def packed(data, block, aligned=False, allow_stored=True):
    blob, d = lz4.pack(data, block, aligned, allow_stored)
    return blob.tobytes(), [(int(c), int(r)) for c, r in d]


@pytest.mark.parametrize("name", ["gen_s7.jsonl", "gen_s7.tbl"])
@pytest.mark.parametrize("block,aligned,limit", [(1, False, 700), (13, False, 700 * 13), (64, True, 1 << 16),
                                                  (4096, False, None), (16384, True, None), (65536, False, None)])
def test_decode_round_trips(ctx, name, block, aligned, limit):
    """Block sizes 1, 13, 64, 4096, 16384, 65536: several hundred 1- and 13-byte blocks put
    every block edge inside shared dwords and 16-byte vectors; the output and the compressed
    bytes at odd addresses."""
    with open(gd.path(name), "rb") as f:
        data = f.read()[:limit]
    blob, d = packed(data, block, aligned)
    assert check_batch(ctx, blob, d) == data
    assert check_batch(ctx, blob, d, out_shift=5, in_shift=3) == data


def test_decode_overlapping_matches(ctx):
    """65536 equal bytes (offset 1, 250-odd length extension bytes) and the periods on either
    side of the 4-, 16- and 64-byte copy widths, as one batch with odd block sizes."""
    data = bytes([0x61]) * 65536 + b"".join(M.periodic(p, 5000 + p) for p in (2, 3, 7, 15, 16, 17, 63, 64, 65))
    for block in (65536, 4099):
        blob, d = packed(data, block)
        assert check_batch(ctx, blob, d, out_shift=1) == data


def test_decode_stored_and_compressed_mixed(ctx):
    rnd = M.random_bytes(65536 + 1000)
    with open(gd.path("gen_s7.jsonl"), "rb") as f:
        text = f.read()[:65536 + 50000]
    data = text[:65536] + rnd[:65536] + text[65536:] + rnd[65536:]   # whole blocks of each kind, then a mixed one
    blob, d = packed(data, 65536)
    assert any(cf & M.STORED for cf, _ in d) and any(not cf & M.STORED for cf, _ in d)
    assert check_batch(ctx, blob, d, out_shift=7, in_shift=9) == data
    blob, d = packed(rnd[:65536], 65536, allow_stored=False)   # one literal-only block, larger than its output
    assert not d[0][0] & M.STORED and d[0][0] > 65536
    assert check_batch(ctx, blob, d) == rnd[:65536]


def test_decode_hand_blocks_and_fixtures(ctx):
    blocks = [(c, len(c), len(r)) for _, c, r in M.hand_blocks()]
    want = b"".join(r for _, _, r in M.hand_blocks())
    with open(gd.path("gen_s7.jsonl"), "rb") as f:
        first = f.read()[:65536]
    for fx in ("gen_s7_64k.default.lz4", "gen_s7_64k.hc.lz4"):
        with open(os.path.join(M.GOLDEN, "lz4", fx), "rb") as f:
            c = f.read()
        blocks.append((c, len(c), 65536))
        want += first
    blob, d = pack_blocks(blocks)
    assert check_batch(ctx, blob, d, out_shift=3, in_shift=1) == want
    assert gpu_decode(ctx, b"", [])[0] == b""   # no block: nothing written


def test_decode_malformed_corpus(ctx):
    """Every malformed case between two good blocks, all in one batch: first_bad and the bad
    blocks' count equal the model's, a bad block writes nothing (its range keeps the pre-fill),
    its neighbours and the canaries are intact; the call returns and a following good batch
    decodes.  Bad blocks first and last in a batch of their own as well."""
    good = (bytes([0x10, 0x5A]), 2, 1)
    blocks = [good]
    for _, comp, raw in M.malformed_blocks():
        blocks += [(comp, len(comp), raw), good]
    blocks += [(b"abc", 3 | M.STORED, 4), good, (b"abc", 3 | M.STORED, 2), good]   # stored blocks of another size
    blob, d = pack_blocks(blocks)
    assert M.decode_batch(blob, d)[1] == 1
    check_batch(ctx, blob, d, out_shift=2, in_shift=5)
    bases = [(c, len(c), r) for _, c, r in M.malformed_bases()]
    for batch in ([bases[5], good], [good, good, bases[8]], bases):
        blob, d = pack_blocks(batch)
        check_batch(ctx, blob, d)
    data = M.periodic(17, 30000)
    blob, d = packed(data, 4096)
    assert check_batch(ctx, blob, d) == data


# ---- the chain ----------------------------------------------------------------------------

def line_parts(raw, n):
    """raw cut into n parts at line boundaries."""
    cuts = [0]
    for k in range(1, n):
        at = raw.index(b"\n", len(raw) * k // n) + 1
        cuts.append(at)
    cuts.append(len(raw))
    return [raw[a:b] for a, b in zip(cuts, cuts[1:])]


@pytest.mark.parametrize("stem,fmt", [("gen_s7", "json"), ("gen_s7_tbl", "tbl"), ("edge_orgjson", "json")])
def test_chain_counts_equal_golden_and_submit_raw(stem, fmt):
    """Four batches of 4096-byte blocks that are not line-aligned (lines straddle blocks),
    alternating slots, an empty batch in between: counts and stats equal the golden
    expectations and those of ysb_submit_raw on the same bytes; lz4_info agrees with the
    directory.  edge_orgjson: deferred lines take their path from a decoded batch."""
    raw = gd.tbl_events(stem)[0] if fmt == "tbl" else gd.events(stem)[0]
    exp = gd.expected(stem)
    parts = line_parts(raw, 4)
    with make_ctx(input_format=fmt, timing=True) as ctx:
        for k, part in enumerate(parts):
            blob, d = lz4.pack(part, 4096, line_aligned=False)
            ctx.submit_raw_lz4(blob, d, slot=k & 1)
            if k == 1:
                ctx.submit_raw_lz4(b"", np.empty((0, 2), dtype=np.uint32), slot=0)
        info = ctx.lz4_info()
        assert info["batches"] == 5 and info["blocks"] == d.shape[0] and info["bad_blocks"] == 0
        assert info["first_bad"] is None and info["comp_bytes"] == blob.size and info["raw_bytes"] == len(parts[-1])
        assert info["decode_ms"] > 0
        st_lz4 = ctx.stats()
        check_against(ctx, *exp)
    with make_ctx(input_format=fmt) as ctx:
        for k, part in enumerate(parts):
            ctx.submit_raw(part, slot=k & 1)
        st_raw = ctx.stats()
        check_against(ctx, *exp)
    for k in st_raw:
        if k != "batches":
            assert st_lz4[k] == st_raw[k], k
    assert st_lz4["batches"] == st_raw["batches"] + 1   # the empty batch


def test_dropped_batch_is_a_sticky_format_error():
    """A batch with one corrupted block between two good batches: dropped whole at its launch
    with YSB_ERR_FORMAT naming the block, sticky until reset (counts cannot be read meanwhile, as
    after a raw batch over its line capacity; the first batch's are read before); after reset
    the context counts a good batch exactly."""
    raw = gd.events("gen_s7")[0]
    exp_rows, exp_st = gd.expected("gen_s7")
    parts = line_parts(raw, 2)
    with make_ctx() as ctx:
        blob, d = lz4.pack(parts[0], 4096, line_aligned=False)
        ctx.submit_raw_lz4(blob, d, slot=0)
        first = ctx.stats()
        assert 0 < first["events"] < exp_st["events"]
        bad_blob, bad_d = lz4.pack(parts[1], 4096, line_aligned=False)
        bad_blob = bad_blob.copy()
        at = int((bad_d[:7, 0] & 0x7FFFFFFF).sum())        # block 7's token:
        bad_blob[at] = 0xF0                                   # 15+ literals ...
        bad_blob[at + 1:at + 1 + 20] = 255                    # ... of a length far past the block
        directory = [(int(c), int(r)) for c, r in bad_d]
        assert M.decode_batch(bad_blob.tobytes(), directory)[1] == 7
        ctx.submit_raw_lz4(bad_blob, bad_d, slot=1)           # launches nothing yet
        with pytest.raises(YsbError) as e:
            ctx.submit_raw_lz4(blob, d, slot=0)               # its launch: dropped
        assert e.value.code == -5 and "block 7" in str(e.value)
        for call in (ctx.sync, ctx.stats, lambda: ctx.submit_raw(parts[1], slot=1)):
            with pytest.raises(YsbError) as e:
                call()
            assert e.value.code == -5 and "block 7" in str(e.value)
        ctx.reset()
        info = ctx.lz4_info()
        assert info["batches"] == 0
        for k, part in enumerate(parts):
            blob, d = lz4.pack(part, 4096, line_aligned=False)
            ctx.submit_raw_lz4(blob, d, slot=k & 1)
        check_against(ctx, exp_rows, exp_st)
    # the batches before the bad one are counted, the bad one and what follows are not
    with make_ctx() as ctx:
        ctx.submit_raw(parts[0], slot=0)
        alone = ctx.stats()
    assert {k: v for k, v in first.items()} == alone


def test_argument_and_capacity_errors():
    data = gd.events("gen_s7")[0][:100000]
    blob, d = lz4.pack(data, 16384)
    with make_ctx(max_batch_bytes=1 << 16) as ctx:
        def code(fn):
            with pytest.raises(YsbError) as e:
                fn()
            return e.value.code
        assert code(lambda: ctx.submit_raw_lz4(blob, d, slot=2)) == -1
        assert code(lambda: ctx.submit_raw_lz4(blob, d)) == -4                    # raw total over max_batch_bytes
        rnd = np.frombuffer(M.random_bytes(70000), dtype=np.uint8)
        big = np.array([[35000 | M.STORED, 35000], [35000 | M.STORED, 35000]], dtype=np.uint32)
        assert code(lambda: ctx.submit_raw_lz4(rnd, big)) == -4                   # compressed bytes over it
        one, e1 = lz4.compress_block(data[:1000])
        for bad_dir in ([(len(one), 0)], [(len(one), 65537)], [(len(one) + 1, 1000)], [(len(one) - 1, 1000)]):
            assert code(lambda: ctx.submit_raw_lz4(one, np.array(bad_dir, dtype=np.uint32))) == -1, bad_dir
            assert code(lambda: ctx.lz4_decode_device(0x1000, len(one), np.array(bad_dir, dtype=np.uint32), 0x1000, 1 << 20)) == -1
        assert code(lambda: ctx.lz4_decode_device(0x1000, len(one), np.array([e1], dtype=np.uint32), 0x1000, 999)) == -4
        # none of them left anything behind: a good batch counts
        small, sd = lz4.pack(data[:data.rindex(b"\n", 0, 60000) + 1], 16384)
        ctx.submit_raw_lz4(small, sd)
        assert ctx.stats()["events"] == data[:60000].count(b"\n")
    with YsbContext() as ctx:   # no ad map yet
        with pytest.raises(YsbError) as e:
            ctx.submit_raw_lz4(blob, d)
        assert e.value.code == -3
