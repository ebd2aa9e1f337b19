"""GPU: standard LZ4 frames -- the measure pass (ysb_lz4_measure_device) against the model's raw
sizes on the CPU tests' corpus and the liblz4 frame fixtures; the several-wave decoder, forced
(ysb_lz4_set_decoder), on the shapes of tests/test_gpu_lz4.py against the pure-Python model,
between canaries and over a pre-filled buffer, with the malformed corpus that
tests/test_lz4_frame_logic.py and tests/test_lz4_logic.py pass through the sanitized host builds;
measure + decode of a frame's blocks (ysb_lz4_decode_blocks_device); argument and capacity
errors."""
import os

import numpy as np
import pytest

import golden_data as gd
import lz4_model as M
from test_gpu_lz4 import CANARY, FILL, check_batch, gpu_decode, pack_blocks, packed
from ysb_amd import YsbContext, YsbError, lz4

pytestmark = pytest.mark.gpu

NARROW, WIDE = 1, 2
FRAMES = os.path.join(M.GOLDEN, "lz4frame")


@pytest.fixture(scope="module")
def ctx():
    with YsbContext() as c:
        yield c
        c.lz4_set_decoder(0)


@pytest.fixture
def wide(ctx):
    ctx.lz4_set_decoder(WIDE)
    yield ctx
    ctx.lz4_set_decoder(0)


def golden(name, limit=None):
    with open(gd.path(name), "rb") as f:
        return f.read()[:limit]


def fixture(name):
    with open(os.path.join(FRAMES, name), "rb") as f:
        return f.read()


def frame_of_blocks(blocks, shift=0):
    """[(compressed bytes, comp field)] as a buffer of size words and data (what a frame's block
    area looks like) behind `shift` bytes, and its index."""
    buf = bytearray(shift)
    index = np.zeros(len(blocks), dtype=lz4.FRAME_BLOCK)
    for i, (comp, field) in enumerate(blocks):
        buf += int(field).to_bytes(4, "little")
        index[i] = (len(buf), field, 0)
        buf += comp
    return bytes(buf), index


def model_raw(comp, field):
    """The model's raw size of a frame block: the one size that makes it valid, or 0."""
    if field & M.STORED:
        return len(comp) if 1 <= len(comp) <= M.MAX_RAW else 0
    try:
        want = M.measure_block(comp)             # the Python model's walk, written from the format
    except M.Bad:
        want = 0
    try:
        raw = lz4.measure_block(comp, field)     # the host model (the walk the kernel instantiates) ...
    except YsbError:
        raw = 0
    assert raw == want                           # ... and the Python model agree, on "bad" too
    assert raw == 0 or M.is_valid(comp, raw)
    return raw


def upload(ctx, buf):
    d = ctx.device_alloc(max(len(buf), 1))
    if buf:
        ctx.h2d(d, np.frombuffer(buf, dtype=np.uint8))
    return d


# ---- the measure pass ---------------------------------------------------------------------

def test_measure_corpus(ctx):
    """Hand blocks, round-trip blocks of every size class, stored blocks, the liblz4 block
    fixtures and the whole malformed corpus in one index: raw sizes and the first bad block
    equal the model's; the buffer ends at its allocation's last byte."""
    # (a frame's block is at most 65536 bytes: the hand block with 65532 literals is not one)
    blocks = [(c, len(c)) for _, c, _ in M.hand_blocks() if len(c) <= M.MAX_RAW]
    for block in (1, 13, 64, 4096, 16384, 65536):
        blob, d = packed(golden("gen_s7.jsonl", 700 * block if block < 64 else 200000), block)
        at = 0
        for cf, raw in d[:40]:
            n = cf & ~M.STORED
            blocks.append((blob[at:at + n], cf))
            at += n
    blocks.append((M.random_bytes(65536), 65536 | M.STORED))
    blocks.append((bytes([0x61]) * 3, 3 | M.STORED))
    for fx in ("gen_s7_64k.default.lz4", "gen_s7_64k.hc.lz4"):
        with open(os.path.join(M.GOLDEN, "lz4", fx), "rb") as f:
            c = f.read()
        blocks.append((c, len(c)))
    comp, (field, raw) = lz4.compress_block(bytes([0x61]) * 65536)
    blocks.append((comp, field))
    n_good = len(blocks)
    want = [model_raw(c, f) for c, f in blocks]
    assert all(want) and 65536 in want and 1 in want
    for shift in (0, 3):
        buf, index = frame_of_blocks(blocks, shift)
        d = upload(ctx, buf)
        try:
            raw, bad = ctx.lz4_measure_device(d, index)
        finally:
            ctx.device_free(d)
        assert bad is None and raw.tolist() == want
        info = ctx.lz4_frame_info()
        assert info["blocks"] == n_good and info["raw_bytes"] == sum(want) and info["bad_blocks"] == 0
    # the malformed corpus between good blocks (a cut of no bytes cannot be an index entry)
    good = (bytes([0x10, 0x5A]), 2)
    mixed = [good]
    for _, comp, _ in M.malformed_blocks():
        if 1 <= len(comp) <= M.MAX_RAW:
            mixed += [(comp, len(comp)), good]
    want = [model_raw(c, f) for c, f in mixed]
    assert want.count(0) > 300
    buf, index = frame_of_blocks(mixed, 1)
    d = upload(ctx, buf)
    try:
        raw, bad = ctx.lz4_measure_device(d, index)
    finally:
        ctx.device_free(d)
    assert raw.tolist() == want and bad == want.index(0)
    info = ctx.lz4_frame_info()
    assert info["bad_blocks"] == want.count(0) and info["first_bad"] == bad


def test_measure_fixture_frames(ctx):
    lines = golden("gen_s7.jsonl")
    for name in ("gen_s7_150k.lz4", "small_checksums.lz4", "small_skip_two.lz4"):
        frame = fixture(name)
        index, info = lz4.frame_index(frame)
        d = upload(ctx, frame)
        try:
            raw, bad = ctx.lz4_measure_device(d, index)
        finally:
            ctx.device_free(d)
        want = [model_raw(frame[int(e["offset"]):int(e["offset"]) + (int(e["comp_bytes"]) & ~M.STORED)], int(e["comp_bytes"]))
                for e in index]
        assert bad is None and raw.tolist() == want, name
    assert ctx.lz4_measure_device(0, np.zeros(0, dtype=lz4.FRAME_BLOCK))[0].size == 0


# ---- the several-wave decoder, forced -------------------------------------------------------

@pytest.mark.parametrize("name", ["gen_s7.jsonl", "gen_s7.tbl"])
@pytest.mark.parametrize("block,aligned,limit", [(1, False, 700), (13, False, 700 * 13), (64, True, 1 << 16),
                                                  (4096, False, None), (16384, True, None), (65536, False, None)])
def test_wide_decode_round_trips(wide, name, block, aligned, limit):
    """The shapes of test_gpu_lz4.test_decode_round_trips through the several-wave kernel:
    several hundred 1- and 13-byte blocks put every block edge inside shared dwords and 16-byte
    vectors; the output shifted by 5 and the input by 3."""
    data = golden(name, limit)
    blob, d = packed(data, block, aligned)
    assert check_batch(wide, blob, d) == data
    assert check_batch(wide, blob, d, out_shift=5, in_shift=3) == data


def test_wide_decode_overlapping_matches(wide):
    data = bytes([0x61]) * 65536 + b"".join(M.periodic(p, 5000 + p) for p in (2, 3, 7, 15, 16, 17, 63, 64, 65))
    for block in (65536, 4099):
        blob, d = packed(data, block)
        assert check_batch(wide, blob, d, out_shift=1) == data
    for p in (2, 3, 7, 15, 16, 17, 63, 64, 65):   # a whole block of each period
        blob, d = packed(M.periodic(p), 65536)
        assert check_batch(wide, blob, d, out_shift=p & 15) == M.periodic(p)


def test_wide_decode_stored_and_compressed_mixed(wide):
    rnd = M.random_bytes(65536 + 1000)
    text = golden("gen_s7.jsonl", 65536 + 50000)
    data = text[:65536] + rnd[:65536] + text[65536:] + rnd[65536:]
    blob, d = packed(data, 65536)
    assert any(cf & M.STORED for cf, _ in d) and any(not cf & M.STORED for cf, _ in d)
    assert check_batch(wide, blob, d, out_shift=7, in_shift=9) == data
    blob, d = packed(rnd[:65536], 65536, allow_stored=False)   # one literal-only block, larger than its output
    assert not d[0][0] & M.STORED and d[0][0] > 65536
    assert check_batch(wide, blob, d) == rnd[:65536]


def test_wide_decode_hand_blocks_and_fixtures(wide):
    blocks = [(c, len(c), len(r)) for _, c, r in M.hand_blocks()]
    want = b"".join(r for _, _, r in M.hand_blocks())
    first = golden("gen_s7.jsonl", 65536)
    for fx in ("gen_s7_64k.default.lz4", "gen_s7_64k.hc.lz4"):
        with open(os.path.join(M.GOLDEN, "lz4", fx), "rb") as f:
            c = f.read()
        blocks.append((c, len(c), 65536))
        want += first
    blob, d = pack_blocks(blocks)
    assert check_batch(wide, blob, d, out_shift=3, in_shift=1) == want
    assert gpu_decode(wide, b"", [])[0] == b""


def test_wide_decode_malformed_corpus(wide):
    """The malformed corpus (the one the sanitized host build of the shared reader passes) between
    good blocks, over a pre-filled buffer between canaries: first_bad and the count equal the
    model's, a bad block writes nothing, its neighbours decode, a following good batch decodes."""
    good = (bytes([0x10, 0x5A]), 2, 1)
    blocks = [good]
    for _, comp, raw in M.malformed_blocks():
        blocks += [(comp, len(comp), raw), good]
    blocks += [(b"abc", 3 | M.STORED, 4), good, (b"abc", 3 | M.STORED, 2), good]
    blob, d = pack_blocks(blocks)
    assert M.decode_batch(blob, d)[1] == 1
    check_batch(wide, blob, d, out_shift=2, in_shift=5)
    bases = [(c, len(c), r) for _, c, r in M.malformed_bases()]
    for batch in ([bases[5], good], [good, good, bases[8]], bases):
        blob, d = pack_blocks(batch)
        check_batch(wide, blob, d)
    data = M.periodic(17, 30000)
    blob, d = packed(data, 4096)
    assert check_batch(wide, blob, d) == data


def test_both_decoders_agree_and_auto_picks_by_block_size(ctx):
    data = golden("gen_s7.jsonl", 200000)
    for block in (4096, 65536):
        blob, d = packed(data, block)
        for dec in (NARROW, WIDE, 0):
            ctx.lz4_set_decoder(dec)
            assert check_batch(ctx, blob, d, out_shift=dec) == data
    ctx.lz4_set_decoder(0)
    with pytest.raises(YsbError) as e:
        ctx.lz4_set_decoder(3)
    assert e.value.code == -1


# ---- measure + decode of a frame's blocks -----------------------------------------------------

def decode_blocks(ctx, buf, index, out_shift=0, extra=300, cap=None):
    """ysb_lz4_decode_blocks_device between two canaries over a pre-filled buffer; returns (the
    bytes the call says it decoded, first bad)."""
    span = out_shift + 65536 * index.size + extra
    host = np.full(CANARY + span + CANARY, 0xA5, dtype=np.uint8)
    host[CANARY + out_shift:CANARY + span] = FILL
    d_out, d_in = ctx.device_alloc(host.size), upload(ctx, buf)
    try:
        ctx.h2d(d_out, host)
        raw, bad = ctx.lz4_decode_blocks_device(d_in, index, d_out + CANARY + out_shift, span - out_shift if cap is None else cap)
        got = ctx.d2h(np.empty_like(host), d_out)
    finally:
        ctx.device_free(d_out)
        ctx.device_free(d_in)
    assert (got[:CANARY + out_shift] == 0xA5).all() and (got[CANARY + span:] == 0xA5).all(), "canary overwritten"
    assert (got[CANARY + out_shift + raw:CANARY + span] == FILL).all(), "bytes past the raw total written"
    return got[CANARY + out_shift:CANARY + out_shift + raw].tobytes(), bad


@pytest.mark.parametrize("decoder", [0, NARROW, WIDE])
def test_decode_blocks_device_on_the_liblz4_fixture(ctx, decoder):
    """The fixture frame (liblz4's LZ4F, two full 64 KiB blocks and a short one): the output is
    the golden file's prefix; frame_info tells what ran."""
    ctx.lz4_set_decoder(decoder)
    try:
        frame = fixture("gen_s7_150k.lz4")
        index, _ = lz4.frame_index(frame)
        out, bad = decode_blocks(ctx, frame, index, out_shift=decoder)
        lines = golden("gen_s7.jsonl")
        assert bad is None and 2 * 65536 < len(out) <= 150000 and out == lines[:len(out)]
        info = ctx.lz4_frame_info()
        assert info["blocks"] == 3 and info["raw_bytes"] == len(out) and info["bad_blocks"] == 0
        assert info["comp_bytes"] == int((index["comp_bytes"] & 0x7FFFFFFF).sum())
        assert info["decoder"] == (NARROW if decoder == NARROW else WIDE)   # frame blocks size for 65536
        # the frames with checksums and a skippable frame; our own frames with short blocks
        for name in ("small_checksums.lz4", "small_skip_two.lz4"):
            f = fixture(name)
            idx, _ = lz4.frame_index(f)
            out, bad = decode_blocks(ctx, f, idx)
            assert bad is None and out == lines[:len(out)] and len(out) > 2000, name
        for block in (13, 251, 65536):
            data = lines[:9000 if block == 13 else 180000] + M.random_bytes(1000)
            f = lz4.frame_pack(data, block).tobytes()
            idx, _ = lz4.frame_index(f)
            out, bad = decode_blocks(ctx, f, idx, out_shift=3)
            assert bad is None and out == data, block
    finally:
        ctx.lz4_set_decoder(0)


def test_decode_blocks_device_bad_block_and_errors(ctx):
    """A corrupted block among good ones: it is measured bad (raw 0), takes no room and writes
    nothing; the others decode; YSB_ERR_FORMAT comes back as first_bad.  Capacity and argument
    errors decode nothing."""
    lines = golden("gen_s7.jsonl", 9000)
    frame = bytearray(lz4.frame_pack(lines, 3000).tobytes())
    index, _ = lz4.frame_index(bytes(frame))
    assert index.size == 3
    at = int(index[1]["offset"])
    frame[at] = 0xF0
    frame[at + 1:at + 21] = bytes([255]) * 20   # 15+ literals of a length far past the block
    for dec in (NARROW, WIDE):
        ctx.lz4_set_decoder(dec)
        try:
            out, bad = decode_blocks(ctx, bytes(frame), index)
        finally:
            ctx.lz4_set_decoder(0)
        assert bad == 1 and out == lines[:3000] + lines[6000:]
        info = ctx.lz4_frame_info()
        assert info["bad_blocks"] == 1 and info["first_bad"] == 1 and info["raw_bytes"] == 6000

    def code(fn):
        with pytest.raises(YsbError) as e:
            fn()
        return e.value.code
    good = lz4.frame_pack(lines, 3000).tobytes()
    index, _ = lz4.frame_index(good)
    assert code(lambda: decode_blocks(ctx, good, index, cap=8999)) == -4          # out_cap below the measured total
    big = index.copy()
    big[0]["comp_bytes"] = 65537
    assert code(lambda: ctx.lz4_decode_blocks_device(0x1000, big, 0x1000, 1 << 20)) == -1
    assert code(lambda: ctx.lz4_measure_device(0x1000, big)) == -1
    zero = index.copy()
    zero[2]["comp_bytes"] = M.STORED
    assert code(lambda: ctx.lz4_measure_device(0x1000, zero)) == -1
    assert code(lambda: ctx.lz4_decode_blocks_device(0, index, 0x1000, 1 << 20)) == -1
    out, bad = decode_blocks(ctx, good, index)   # none of them left anything behind
    assert bad is None and out == lines


# ---- frame batches through the slot chain (ysb_submit_lz4_blocks) ------------------------------

from test_gpu_parity import make_ctx  # noqa: E402

CHAIN_MB = 1 << 20   # max_batch_bytes of the chain tests: the fixture's three blocks need (3 + 1) x 65536


def raw_reference(data):
    """Counts and stats of ysb_submit_raw on the decoded bytes, and the oracle's on those lines."""
    from oracle import oracle
    with make_ctx(max_batch_bytes=CHAIN_MB) as ctx:
        ctx.submit_raw(data, slot=0)
        st = ctx.stats()
        rows = ctx.drain_buckets()
    ads, camp = gd.ad_arrays()
    _, offs = gd.dostats.split_lines(data)
    orows, ost = oracle.run(oracle.AdMap(ads, camp), data, offs)
    assert rows == orows
    for k, v in ost.items():
        assert st[k] == v, (k, st[k], v)
    return rows, st


def check_equal(ctx, ref, batches):
    rows, st = ref
    got_st = ctx.stats()
    for k in st:
        if k != "batches":
            assert got_st[k] == st[k], (k, got_st[k], st[k])
    assert got_st["batches"] == batches
    assert ctx.drain_buckets() == rows


@pytest.fixture(scope="module")
def fixture_frame():
    frame = fixture("gen_s7_150k.lz4")
    index, _ = lz4.frame_index(frame)
    data = golden("gen_s7.jsonl")[:149775]
    assert data.endswith(b"\n")
    return frame, index, data, raw_reference(data)


def carry_stream():
    """The stream of the CPU carry test (tests/native/lz4_frame_logic.cpp): 40 golden lines ended
    by '\\n', "\\r\\n" and '\\r' in turn, one line longer than three 251-byte blocks, a "\\r\\n" whose
    '\\r' is a 13-byte block's last byte, the stream ending in a lone '\\r'."""
    src = golden("gen_s7.jsonl", 12000).split(b"\n")
    out = bytearray()
    for k in range(40):
        line = src[k]
        if k == 7:
            line = line + src[8] + src[9] + src[10]
        if k == 3:
            line += b" " * ((13 - 1 - (len(out) + len(line)) % 13) % 13)
        out += line
        if k % 3 == 0 or k == 39:
            if k == 3:
                assert len(out) % 13 == 12
            out += b"\r" if k == 39 else b"\r\n"
        elif k % 3 == 1:
            out += b"\n"
        else:
            out += b"\r"
    return bytes(out)


def registered_copy(ctx, frame):
    """frame in a 4096-byte aligned array registered with the context, at an odd offset."""
    buf = np.empty(len(frame) + 3 + 2 * 4096, dtype=np.uint8)
    buf = buf[(-buf.ctypes.data) % 4096:][:(len(frame) + 3 + 4095) // 4096 * 4096]
    buf[3:3 + len(frame)] = np.frombuffer(frame, dtype=np.uint8)
    ctx.host_register(buf)
    return buf


@pytest.mark.parametrize("mapped", [False, True])
def test_chain_whole_lines(fixture_frame, mapped):
    """The liblz4 fixture frame as one batch, and as one block per batch with MORE on all but the
    last, alternating slots: counts and stats identical to ysb_submit_raw of the decoded bytes
    and to the oracle's counts for those lines; frame_info tells the carries."""
    frame, index, data, ref = fixture_frame
    for per_block in (False, True):
        with make_ctx(max_batch_bytes=CHAIN_MB, timing=True) as ctx:
            if mapped:
                arr = registered_copy(ctx, frame)
                idx = index.copy()
                idx["offset"] += 3
                submit = lambda i, **kw: ctx.submit_lz4_blocks_mapped(arr, i, **kw)
            else:
                idx = index
                submit = lambda i, **kw: ctx.submit_lz4_blocks(frame, i, **kw)
            if per_block:
                for k in range(idx.size):
                    submit(idx[k:k + 1], slot=k & 1, more=k + 1 < idx.size)
                    if k == 0:
                        info = ctx.lz4_frame_info()
                        cut = data.rindex(b"\n", 0, 65536) + 1
                        assert (info["carry_in"], info["carry_out"], info["raw_bytes"]) == (0, 65536 - cut, 65536)
            else:
                submit(idx, slot=0)
            info = ctx.lz4_frame_info()
            assert info["bad_blocks"] == 0 and info["first_bad"] is None and info["carry_out"] == 0
            assert info["batches"] == (idx.size if per_block else 1) and info["decoder"] == WIDE
            assert info["raw_bytes"] == (len(data) - 131072 if per_block else len(data)) and info["decode_ms"] > 0
            check_equal(ctx, ref, idx.size if per_block else 1)
            if mapped:
                ctx.host_unregister(arr)


@pytest.mark.parametrize("mapped", [False, True])
def test_chain_carry(mapped):
    """The 13-byte-block stream of the CPU carry test, one block per batch: a line longer than
    many batches, "\\r\\n" split across two batches, a stream ending in a lone '\\r' -- the same
    counts and stats as ysb_submit_raw of the stream.  The 251-byte blocks too, and two blocks
    per batch."""
    stream = carry_stream()
    ref = raw_reference(stream)
    for block, per in ((13, 1), (251, 1), (64, 2)):
        frame = lz4.frame_pack(stream, block).tobytes()
        index, _ = lz4.frame_index(frame)
        with make_ctx(max_batch_bytes=CHAIN_MB) as ctx:
            if mapped:
                arr = registered_copy(ctx, frame)
                index["offset"] += 3
            n = 0
            for k in range(0, index.size, per):
                more = k + per < index.size
                if mapped:
                    ctx.submit_lz4_blocks_mapped(arr, index[k:k + per], slot=n & 1, more=more)
                else:
                    ctx.submit_lz4_blocks(frame, index[k:k + per], slot=n & 1, more=more)
                n += 1
            assert ctx.lz4_frame_info()["carry_out"] == 0
            check_equal(ctx, ref, n)
            if mapped:
                ctx.host_unregister(arr)


def code_of(fn):
    with pytest.raises(YsbError) as e:
        fn()
    return e.value.code, str(e.value)


def test_chain_dropped_batch_and_reset(fixture_frame):
    """A batch with a corrupted block behind a batch that left a carry: dropped whole, sticky
    YSB_ERR_FORMAT naming the block; ysb_reset clears the carry, so the stream submitted again
    counts exactly (a carry left over would put a broken line in front)."""
    frame, index, data, ref = fixture_frame
    bad = bytearray(frame)
    at = int(index[1]["offset"])
    bad[at] = 0xF0
    bad[at + 1:at + 21] = bytes([255]) * 20
    with make_ctx(max_batch_bytes=CHAIN_MB) as ctx:
        ctx.submit_lz4_blocks(bytes(bad), index[0:1], slot=0, more=True)
        ctx.submit_lz4_blocks(bytes(bad), index[1:3], slot=1, more=True)      # launches nothing of its own yet
        code, msg = code_of(ctx.sync)
        assert code == -5 and "block 0" in msg and "dropped" in msg
        assert code_of(ctx.stats)[0] == -5
        assert code_of(lambda: ctx.submit_lz4_blocks(frame, index, slot=0))[0] == -5
        ctx.reset()
        assert ctx.lz4_frame_info()["batches"] == 0
        ctx.submit_raw(data[:1000], slot=0)        # no carry is pending after the reset: not YSB_ERR_STATE
        ctx.reset()
        for k in range(index.size):
            ctx.submit_lz4_blocks(frame, index[k:k + 1], slot=k & 1, more=k + 1 < index.size)
        assert ctx.lz4_frame_info()["carry_in"] > 0
        check_equal(ctx, ref, index.size)
    # a carry of more than 64 KiB: one line longer than that, with more to follow
    long_line = b"x" * 70000 + b"\n"
    f2 = lz4.frame_pack(long_line, 65536).tobytes()
    i2, _ = lz4.frame_index(f2)
    with make_ctx(max_batch_bytes=CHAIN_MB) as ctx:
        ctx.submit_lz4_blocks(f2, i2[0:1], slot=0, more=True)      # 65536 bytes carried: the most there is room for
        assert ctx.lz4_frame_info()["carry_out"] == 65536
        ctx.submit_lz4_blocks(f2, i2[0:1], slot=1, more=True)      # 131072 bytes without a terminator
        code, msg = code_of(ctx.sync)
        assert code == -4 and "terminator" in msg
        ctx.reset()
        ctx.submit_lz4_blocks(f2, i2, slot=0)
        assert ctx.stats()["events"] == 1
    # 65,537 bytes without a terminator -- one more than the carry holds -- as a 1-byte carry in
    # front of a full block, and as blocks of 65,536 and 1 bytes in one batch
    one = lz4.frame_pack(b"y", 1).tobytes()
    i_one, _ = lz4.frame_index(one)
    full = lz4.frame_pack(b"x" * 65536 + b"z", 65536).tobytes()
    i_full, _ = lz4.frame_index(full)
    assert i_one.size == 1 and i_full.size == 2
    for batches in (((one, i_one), (full, i_full[0:1])), ((full, i_full),)):
        with make_ctx(max_batch_bytes=CHAIN_MB) as ctx:
            for k, (f, i) in enumerate(batches):
                ctx.submit_lz4_blocks(f, i, slot=k & 1, more=True)
            code, msg = code_of(ctx.sync)
            assert code == -4 and "terminator" in msg
            ctx.reset()
            ctx.submit_lz4_blocks(one, i_one, slot=0, more=True)       # the carry was emptied: one byte, not 65,538
            assert ctx.lz4_frame_info()["carry_in"] == 0 and ctx.lz4_frame_info()["carry_out"] == 1


def test_chain_errors(fixture_frame):
    frame, index, data, ref = fixture_frame
    with make_ctx(max_batch_bytes=CHAIN_MB) as ctx:
        # YSB_ERR_STATE: any submit that is not a frame batch while a carry is pending
        ctx.submit_lz4_blocks(frame, index[0:1], slot=0, more=True)
        blob, d = lz4.pack(data[:5000], 4096)
        raw, offs = gd.events("gen_s7")
        few = (raw[:int(offs[10])], offs[:10])
        for call in (lambda: ctx.submit_raw(data[:1000], slot=1),
                     lambda: ctx.submit_raw_lz4(blob, d, slot=1),
                     lambda: ctx.submit(few[0], few[1], slot=1),
                     lambda: ctx.submit_device(0x1000, 16, 0x1000, 1),
                     lambda: ctx.submit_columns_device(0x1000, 16, 16)):
            assert code_of(call)[0] == -3
        ctx.submit_lz4_blocks(frame, index[1:3], slot=1)     # the stream goes on; its end lifts the state
        check_equal(ctx, ref, 2)
        ctx.submit_raw(b"", slot=0)
        # YSB_ERR_ARG
        assert code_of(lambda: ctx.submit_lz4_blocks(frame, index, slot=2))[0] == -1
        assert code_of(lambda: ctx.submit_lz4_blocks(frame, index[::-1].copy()))[0] == -1          # not consecutive
        assert code_of(lambda: ctx.submit_lz4_blocks(frame, index[[0, 0]].copy()))[0] == -1
        big = index.copy()
        big[0]["comp_bytes"] = 65537
        assert code_of(lambda: ctx.submit_lz4_blocks(frame, big))[0] == -1
        from ysb_amd._lib import lib
        assert lib().ysb_submit_lz4_blocks(ctx._h, 0, frame, index.ctypes.data, index.size, 2) == -1  # unknown flag
        arr = np.frombuffer(frame, dtype=np.uint8)
        assert code_of(lambda: ctx.submit_lz4_blocks_mapped(arr, index))[0] == -1                   # not registered
        # none of them left anything behind
        ctx.reset()
        ctx.submit_lz4_blocks(frame, index)
        check_equal(ctx, ref, 1)
    # YSB_ERR_CAPACITY: (n_blocks + 1) x 65536 and the span against max_batch_bytes
    with make_ctx(max_batch_bytes=3 * 65536) as ctx:
        assert code_of(lambda: ctx.submit_lz4_blocks(frame, index))[0] == -4
        ctx.submit_lz4_blocks(frame, index[0:2], more=True)
        ctx.submit_lz4_blocks(frame, index[2:3], slot=1)
        check_equal(ctx, ref, 2)
    with YsbContext() as ctx:   # no ad map yet
        assert code_of(lambda: ctx.submit_lz4_blocks(frame, index))[0] == -3


@pytest.mark.parametrize("cap", [131072, CHAIN_MB])
def test_file_source_takes_a_frame_by_its_magic(tmp_path, fixture_frame, cap):
    """Lz4FileDataSource on a standard frame file (the liblz4 fixture): told from the container
    by its magic, fed in place in runs of blocks that fit cap, MORE on all but the last."""
    from ysb_amd import Lz4FileDataSource
    frame, index, data, ref = fixture_frame
    path = tmp_path / "events.json.lz4"
    path.write_bytes(frame)
    with make_ctx(max_batch_bytes=CHAIN_MB) as ctx:
        with Lz4FileDataSource(str(path)) as src:
            assert src.frame and src.index.size == 3
            runs = list(src.runs(cap))
            assert len(runs) == (3 if cap == 131072 else 1) and sum(k for _, _, _, k in runs) == 3
            src.run(ctx, cap)
            assert src.batches == len(runs)
        check_equal(ctx, ref, len(runs))
