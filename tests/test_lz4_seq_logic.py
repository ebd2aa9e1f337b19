"""CPU: the generated sequence corpus (tests/lz4_seqgen.py) -- its own coverage of the kernels'
structural edges, the pure-Python model on every block, the C ABI's host entries against the
model, and the whole corpus (valid blocks and mutants) through tests/native/lz4_seq_logic.cpp,
plain and under the host sanitizers.  The sanitized run is the gate for sending the mutants to a
GPU (tests/test_gpu_lz4_seq.py); the pinned digest makes what it saw what the GPU gets.  No GPU."""
import hashlib
import os
import subprocess

import pytest

import lz4_model as M
import lz4_seqgen as G
from test_capi import ROOT
from ysb_amd import YsbError, lz4

CORPUS_SHA256 = "a7892a0b3d153472093a965c727c2795b32bd675a4e0c1592519f8ac149d9df6"


@pytest.fixture(scope="module")
def corpus():
    valid = G.valid_blocks()
    return valid, G.mutants(G.mutant_bases())


def build_native(tmp_path, name, flags):
    exe = tmp_path / name
    inc = [a for d in (("streaming-benchmarks_amd", "csrc"), ("include",)) for a in ("-I", os.path.join(ROOT, *d))]
    subprocess.run(["g++", "-std=c++17", "-pthread"] + flags + inc
                   + [os.path.join(ROOT, "tests", "native", "lz4_seq_logic.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def test_corpus_digest_is_pinned(corpus):
    """The serialized corpus is the same bytes on every machine: the native runs below and the
    GPU tests see exactly this."""
    valid, bad = corpus
    assert 1500 <= len(bad) <= 2000 and len(valid) > 1000
    assert all(1 <= len(raw) <= M.MAX_RAW for _, _, raw in valid)
    assert len({name for name, _, _ in valid}) == len(valid)
    assert hashlib.sha256(G.serialize(valid, bad)).hexdigest() == CORPUS_SHA256


def test_lz4_seq_logic_native(tmp_path, corpus):
    """Every block through the host decoder and the measure walk in exact-size heap buffers:
    valid / invalid as flagged, the output as built, the one-wave kernel's in-place checks
    silent on every valid block, the measured size equal to raw."""
    path = tmp_path / "corpus.bin"
    path.write_bytes(G.serialize(*corpus))
    r = subprocess.run([build_native(tmp_path, "lz4_seq_logic", ["-O2"]), str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:]


def test_lz4_seq_logic_native_sanitized(tmp_path, corpus):
    """The same program with -fsanitize=address,undefined, as a stand-alone program.  This is the
    gate of the GPU tests' malformed input."""
    path = tmp_path / "corpus.bin"
    path.write_bytes(G.serialize(*corpus))
    exe = build_native(tmp_path, "lz4_seq_logic_san",
                       ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK") and not r.stderr, r.stdout[-2000:] + r.stderr[-2000:]


def test_model_decodes_every_valid_block(corpus):
    """build() replays the sequence list itself; the model, written from the format, agrees."""
    for name, comp, raw in corpus[0]:
        assert M.decode_block(comp, len(raw)) == raw, name
        assert M.measure_block(comp) == len(raw), name


def test_every_mutant_is_invalid(corpus):
    """A condition, not a measurement: a mutant the model accepts fails here."""
    for name, comp, raw in corpus[1]:
        assert not M.is_valid(comp, raw), name


def host_decode(comp, raw):
    try:
        return lz4.decompress_block(comp, len(comp), raw)
    except YsbError as e:
        assert e.code == -5, e
        return None


def host_measure(comp):
    try:
        return lz4.measure_block(comp)
    except YsbError as e:
        assert e.code == -5, e
        return 0


def model_measure(comp):
    try:
        return M.measure_block(comp)
    except M.Bad:
        return 0


def test_model_measure_against_model_decode():
    """lz4_model.measure_block against lz4_model.decode_block on the hand blocks and the malformed
    corpus of tests/test_lz4_logic.py: the measured size is the one size that decodes; where it
    says Bad, no size does (every size a short block could have; every 97th for a long one)."""
    for name, comp, raw in M.hand_blocks():
        assert M.measure_block(comp) == len(raw), name
    measured = 0
    for name, comp, raw in M.malformed_blocks():
        want = model_measure(comp)
        assert host_measure(comp) == want, name
        if want:
            measured += 1
            assert M.is_valid(comp, want) and not M.is_valid(comp, want + 1) and not M.is_valid(comp, want - 1), name
        else:
            sizes = range(1, min(4 * len(comp) + 20, M.MAX_RAW) + 1, 1 if len(comp) < 64 else 97)
            assert not any(M.is_valid(comp, r) for r in sizes), name
    assert measured >= 10


def test_host_entries_agree_with_the_model(corpus):
    """ysb_lz4_decompress_block and ysb_lz4_measure_block on every block and mutant.  A cut that
    lands behind a sequence's literals measures as a shorter valid block: the model decides."""
    valid, bad = corpus
    for name, comp, raw in valid:
        assert host_decode(comp, len(raw)) == raw, name
        assert host_measure(comp) == len(raw), name
    shorter = 0
    for name, comp, raw in bad:
        assert host_decode(comp, raw) is None, name
        want = model_measure(comp)
        assert host_measure(comp) == want and want != raw, name
        if want:
            shorter += 1
            assert host_decode(comp, want) == M.decode_block(comp, want), name
    assert shorter >= 20


# ---- the generator stays on the edges --------------------------------------------------------

def all_fields(corpus):
    return [(name, G.fields_of(name)) for name, _, _ in corpus[0]]


def test_coverage_of_sequence_counts_and_lengths(corpus):
    fields = all_fields(corpus)
    counts = {len(f) for _, f in fields}
    assert set(G.COUNTS) | {G.MANY} <= counts
    # each count in each style of runs, with the tails
    for k in G.COUNTS:
        styles = {name.split(", ")[1] for name, f in fields if len(f) == k and name.startswith("%d sequences, " % k)}
        assert styles == {s + " runs" for s in G.STYLES}, k
    seqs = [s for _, f in fields for s in f]
    assert set(G.LIT_RUNS) | set(G.LIT_EXT_RUNS) <= {s.lit_len for s in seqs}
    matches = [s for s in seqs if s.match_len]
    assert set(G.OFFSETS) <= {s.offset for s in matches}
    assert set(G.MATCH_LENS) | set(G.MATCH_EXT_LENS) | {529} <= {s.match_len for s in matches}
    rel = {(s.offset, s.match_len - s.offset) for s in matches}
    for off in G.OFFSETS:
        for d in (-1, 0, 1):
            if off + d >= 4:
                assert (off, d) in rel, (off, d)
    # the tails, an empty last sequence behind a match among them
    lasts = {f[-1].lit_len for _, f in fields if len(f) > 1}
    assert set(G.TAILS) <= lasts
    # the batch shapes of the literal copier: 64 runs all short, all long, mixed
    for _, f in fields:
        if len(f) == 64:
            runs = [s.lit_len for s in f]
            short, long_ = all(r <= 32 for r in runs), all(r > 32 for r in runs)
            counts.add("short" if short else "long" if long_ else "mix")
    assert {"short", "long", "mix"} <= counts


def test_coverage_of_match_sources(corpus):
    own = prev = whole = 0
    for _, f in all_fields(corpus):
        for i, s in enumerate(f[:-1]):
            own += 0 < s.offset <= s.lit_len                              # the literals of its own sequence
            prev += i > 0 and s.lit_len == 0 and s.offset <= f[i - 1].match_len   # the match just before it
            whole += s.offset == s.op                                     # everything produced so far
    assert own > 100 and prev > 100 and whole > 20


def test_coverage_of_field_positions(corpus):
    """Each field's first byte at every position from 4 before to 3 behind each boundary of the
    readers' windows (the wide reader's window begins up to 3 bytes in front of the block)."""
    seen = {k: set() for k in ("token", "literal extension", "offset low", "offset high", "match extension")}
    for _, f in all_fields(corpus):
        for s in f:
            seen["token"].add(s.tok)
            if s.lit_ext:
                seen["literal extension"].add(s.tok + 1)
            if s.match_len:
                seen["offset low"].add(s.off_pos)
                seen["offset high"].add(s.off_pos + 1)
                if s.match_ext:
                    seen["match extension"].add(s.off_pos + 2)
    for kind, at in seen.items():
        for b in (64, 256, 512):
            missing = [p for p in range(b - 4, b + 4) if p not in at]
            assert not missing, (kind, b, missing)
    # second and third extension bytes across the boundaries too
    later = set()
    for _, f in all_fields(corpus):
        for s in f:
            later.update(range(s.tok + 2, s.tok + 1 + s.lit_ext))
            if s.match_len:
                later.update(range(s.off_pos + 3, s.off_pos + 2 + s.match_ext))
    for b in (64, 256, 512):
        assert {b - 1, b} <= later, b
    # the wide reader's jump over more than two windows, from a token at every dword residue
    jumps = {s.tok & 3 for _, f in all_fields(corpus) for s in f if s.lit_len >= 600}
    assert jumps == {0, 1, 2, 3}
