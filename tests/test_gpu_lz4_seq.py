"""GPU: both LZ4 decode kernels and the measure kernel on the generated sequence corpus
(tests/lz4_seqgen.py) against the pure-Python model tests/lz4_model.py, byte for byte: blocks of
exactly k sequences around the several-wave kernel's batch of 64 and its ring of three buffers,
literal runs on both sides of the copier's split, offsets and match lengths around the 64-byte
chunk, every field of a sequence at every position across the readers' window boundaries at
every input alignment, every lz4_move residue, 16,384 sequences in one block, and blocks that
turn bad in a late batch.  The corpus, mutants included, is the one tests/test_lz4_seq_logic.py
passes through the sanitized host build of the shared reader and pins by digest."""
import numpy as np
import pytest

import lz4_model as M
import lz4_seqgen as G
from test_gpu_lz4 import check_batch, pack_blocks
from test_gpu_lz4_frame import NARROW, WIDE, decode_blocks, frame_of_blocks, upload
from ysb_amd import YsbContext

pytestmark = pytest.mark.gpu

DECODERS = [pytest.param(NARROW, id="narrow"), pytest.param(WIDE, id="wide")]
GOOD = (bytes([0x10, 0x5A]), 2, 1)   # the one-literal block


@pytest.fixture(scope="module")
def ctx():
    with YsbContext() as c:
        yield c
        c.lz4_set_decoder(0)


@pytest.fixture
def decoder(ctx, request):
    ctx.lz4_set_decoder(request.param)
    yield ctx
    ctx.lz4_set_decoder(0)


def entries(blocks):
    return [(comp, len(comp), len(raw)) for _, comp, raw in blocks]


def expect(blocks):
    return b"".join(raw for _, _, raw in blocks)


@pytest.fixture(scope="module")
def mutants():
    return G.mutants(G.mutant_bases())


@pytest.mark.parametrize("decoder", DECODERS, indirect=True)
@pytest.mark.parametrize("corpus", ["count_blocks", "straddle_blocks", "extreme_blocks"])
def test_decode_corpus(decoder, corpus):
    """A whole corpus in one launch, between canaries over the pre-fill: the concatenated bytes
    the generator built; shifted, so that the blocks' alignments differ from the first run's."""
    blocks = getattr(G, corpus)()
    blob, d = pack_blocks(entries(blocks))
    assert check_batch(decoder, blob, d) == expect(blocks)
    if corpus != "straddle_blocks":     # (the alignment sweep below shifts the straddles)
        assert check_batch(decoder, blob, d, out_shift=9, in_shift=1) == expect(blocks)


def small_batch():
    """About 45 small blocks: the count blocks up to 65 sequences and the straddles whose first
    offset lies at the 256- and 512-byte boundaries."""
    blocks = [b for b in G.count_blocks() if len(G.fields_of(b[0])) <= 65]
    blocks += [b for b in G.straddle_blocks() if b[0] in
               {"straddle L=%d" % L for L in list(range(250, 261)) + list(range(505, 516))}]
    assert 40 <= len(blocks) <= 50
    return blocks


@pytest.mark.parametrize("decoder", DECODERS, indirect=True)
def test_every_move_residue(decoder):
    """in_shift = k, out_shift = (5k + 3) % 16 for k in 0..15: every residue of the output and
    the input address mod 16, for lz4_move's head and tail rule."""
    blocks = small_batch()
    blob, d = pack_blocks(entries(blocks))
    for k in range(16):
        assert check_batch(decoder, blob, d, in_shift=k, out_shift=(5 * k + 3) % 16) == expect(blocks), k


def test_wide_every_input_and_output_dword_residue(ctx):
    """The several-wave decoder at all 16 pairs of in_shift and out_shift in 0..3: every block at
    every Lz4GlobalIn.mis, so each straddle's fields at 256 - mis and 512 - mis."""
    blocks = small_batch()
    blob, d = pack_blocks(entries(blocks))
    ctx.lz4_set_decoder(WIDE)
    try:
        for i in range(4):
            for o in range(4):
                assert check_batch(ctx, blob, d, in_shift=i, out_shift=o) == expect(blocks), (i, o)
    finally:
        ctx.lz4_set_decoder(0)


@pytest.mark.parametrize("decoder", DECODERS, indirect=True)
@pytest.mark.parametrize("half", [0, 1])
def test_deep_malformed_blocks(decoder, mutants, half):
    """The mutants (half of them per launch) between one-literal good blocks: blocks that turn
    bad at sequence 63 .. 128 or at their end, after matches of earlier batches have run in LDS.
    first_bad and the bad count equal the model's, every bad block's range keeps the pre-fill,
    every neighbour decodes (check_batch), and a good batch decoded afterwards is right."""
    blocks = [GOOD]
    for _, comp, raw in mutants[half::2]:
        blocks += [(comp, len(comp), raw), GOOD]
    blob, d = pack_blocks(blocks)
    check_batch(decoder, blob, d, out_shift=2 + half, in_shift=5)
    assert decoder.lz4_info()["bad_blocks"] == len(blocks) // 2 and decoder.lz4_info()["first_bad"] == 1
    after = [b for b in G.count_blocks() if 63 <= len(G.fields_of(b[0])) <= 129]
    blob, d = pack_blocks(entries(after))
    assert check_batch(decoder, blob, d) == expect(after)


@pytest.mark.parametrize("decoder", DECODERS, indirect=True)
def test_pipeline_depths_in_one_launch(decoder):
    """Blocks of 1, 64, 65 and 16,384 sequences in one launch, the largest first and last: the
    launch's max_raw -- the place of the record area in LDS -- is set by another block than the
    small ones'."""
    big = G.extreme_blocks()[0]
    assert len(G.fields_of(big[0])) == G.MANY
    small = [b for b in G.count_blocks() if len(G.fields_of(b[0])) in (1, 64, 65)]
    assert len(small) == 12
    for blocks in ([big] + small, small + [big], small[:6] + [big] + small[6:]):
        blob, d = pack_blocks(entries(blocks))
        assert check_batch(decoder, blob, d, out_shift=3) == expect(blocks)


def model_measure(comp):
    try:
        return M.measure_block(comp)
    except M.Bad:
        return 0


def test_measure_corpus_and_mutants(ctx, mutants):
    """lz4_measure_device over every valid block and every mutant as one index, the buffer
    shifted by 0..3: the raw sizes and the first bad block are lz4_model.measure_block's.  (A
    mutant cut behind a sequence's literals measures as a shorter valid block, and one with
    another raw size as the block it was: the model decides, not the mutant's flag.)"""
    valid = G.valid_blocks()
    assert all(len(comp) <= M.MAX_RAW for _, comp, _ in valid)
    blocks = [(comp, len(comp)) for _, comp, _ in valid]
    for _, comp, _ in mutants:
        blocks += [(comp, len(comp)), (GOOD[0], 2)]
    want = [model_measure(comp) for comp, _ in blocks]
    assert want[:len(valid)] == [len(raw) for _, _, raw in valid]
    assert want.count(0) > 1000 and sum(1 for w, (_, _, r) in zip(want[len(valid)::2], mutants) if w and w != r) > 20
    for shift in range(4):
        buf, index = frame_of_blocks(blocks, shift)
        d = upload(ctx, buf)
        try:
            raw, bad = ctx.lz4_measure_device(d, index)
        finally:
            ctx.device_free(d)
        assert raw.tolist() == want, shift
        assert bad == want.index(0)
        info = ctx.lz4_frame_info()
        assert info["bad_blocks"] == want.count(0) and info["first_bad"] == bad and info["blocks"] == len(blocks)


@pytest.mark.parametrize("decoder", [pytest.param(0, id="auto")] + DECODERS, indirect=True)
def test_measure_and_decode_together(decoder):
    """lz4_decode_blocks_device over the valid corpus: the measured total, the bytes, and (in
    decode_blocks) the untouched pre-fill past the total and the canaries."""
    valid = G.valid_blocks()
    buf, index = frame_of_blocks([(comp, len(comp)) for _, comp, _ in valid], shift=3)
    out, bad = decode_blocks(decoder, buf, index, out_shift=5)
    assert bad is None and len(out) == sum(len(raw) for _, _, raw in valid)
    assert out == expect(valid)
    info = decoder.lz4_frame_info()
    assert info["blocks"] == len(valid) and info["raw_bytes"] == len(out) and info["bad_blocks"] == 0
