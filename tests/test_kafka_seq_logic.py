"""CPU: the generated Kafka corpus (tests/kafka_seqgen.py) -- its own coverage of the kernels'
structural edges as conditions, the pure-Python model on every batch, the C ABI's host entries
against the model on every base call, and the whole corpus through
tests/native/kafka_seq_logic.cpp, plain and under the host sanitizers.  The sanitized run is the
gate for sending the fault and cut cases to a GPU (tests/test_gpu_kafka_seq.py); the pinned digest
makes what it saw what the GPU gets.  No GPU."""
import hashlib
import os
import re
import subprocess

import pytest

import kafka_model as M
import kafka_seqgen as G
from test_capi import ROOT
from test_kafka_logic import model_index_as_array
from ysb_amd import kafka

CORPUS_SHA256 = "f517a7471ab25001b5beb8270560dc0387ba401a0cda0b1fa71e7a3ec624047e"
CSRC = os.path.join(ROOT, "streaming-benchmarks_amd", "csrc")


@pytest.fixture(scope="module")
def corpus():
    return G.corpus()


def build_native(tmp_path, name, flags):
    exe = tmp_path / name
    inc = [a for d in (("streaming-benchmarks_amd", "csrc"), ("include",)) for a in ("-I", os.path.join(ROOT, *d))]
    subprocess.run(["g++", "-std=c++17", "-pthread"] + flags + inc
                   + [os.path.join(ROOT, "tests", "native", "kafka_seq_logic.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def test_constants_match_the_sources():
    """The geometry the generator aims at is the kernels': a retuned kernel fails here, not
    silently past its tests."""
    src = "".join(open(os.path.join(CSRC, f)).read() for f in ("ysb_kafka.h", "ysb_kafka.hip", "ysb_kernels.h"))
    for name, want in G.CONSTANTS.items():
        found = re.findall(r"^constexpr\s+u32\s+%s\s*=\s*(\d+)\s*;" % name, src, flags=re.M)
        assert found == [str(want)], (name, found, want)
    assert G.EDGES == tuple(k * G.WIN for k in (1, 2, 3, 4)) and G.BASE_STEP == G.RUN == G.PLAN_STEP == 256


def test_corpus_digest_is_pinned(corpus):
    """The serialized corpus is the same bytes on every machine: the native runs below and the
    GPU tests see exactly this.  The counts per part are pinned with it."""
    assert len(G.fault_cases()) == 15 * len(G.FAULT_AT) + 6 == 141
    assert len(G.cut_cases()) == 38
    assert len(G.window_batches()) == 16 * (len(G.EDGES) * 20 + 2 + 1 + 18) == 1616
    assert [len(c.batches) for c in G.base_calls()] == [255, 256, 257, 513] + [600] * 7
    assert len(G.gather_calls()) == 12
    assert len({(b.name, b.count) for b in corpus}) == len(corpus) == 2459
    assert hashlib.sha256(G.serialize(corpus)).hexdigest() == CORPUS_SHA256


def test_kafka_seq_logic_native(tmp_path, corpus):
    """Every batch through the serial host model and the kernel's order of work in exact-size
    heap buffers: they agree, give the stated verdict, and valid batches their stated totals."""
    path = tmp_path / "corpus.bin"
    path.write_bytes(G.serialize(corpus))
    r = subprocess.run([build_native(tmp_path, "kafka_seq_logic", ["-O2"]), str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:]


def test_kafka_seq_logic_native_sanitized(tmp_path, corpus):
    """The same program with -fsanitize=address,undefined, as a stand-alone program.  This is the
    gate of the GPU tests' malformed input."""
    path = tmp_path / "corpus.bin"
    path.write_bytes(G.serialize(corpus))
    exe = build_native(tmp_path, "kafka_seq_logic_san",
                       ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK") and not r.stderr, r.stdout[-2000:] + r.stderr[-2000:]


# ---- conditions, not measurements ------------------------------------------------------------

def model_verdict(b):
    blob = G.blob_of([b])
    return M.verdict(blob, M.index(blob, check_crc=True)[0])


def test_every_fault_and_cut_case_is_bad_as_stated():
    """In kafka_model, each with exactly its (record, rule); every rule at every k."""
    for b in G.fault_cases() + G.cut_cases():
        assert model_verdict(b) == (0,) + b.expect, b.name
    for k in G.FAULT_AT:
        rules = {b.expect[1] for b in G.fault_cases() if b.name.endswith(" at record %d" % k)}
        assert rules == set(range(1, 8)), k
    # the cuts: both sides of rounds 1 and 2, inside each varint, at the window edges as sent
    at = {int(b.name.split()[-1]) for b in G.cut_cases()}
    assert {e - G.CASE_MIS + d for e in (G.WIN, 2 * G.WIN) for d in (-1, 0, 1)} <= at
    assert {b.expect[0] for b in G.cut_cases()} >= {0, 1, 63, 64, 65, 128, 129}
    assert {b.expect[1] for b in G.cut_cases()} == {M.RULE["varint"], M.RULE["past_batch"], M.RULE["count"]}
    # as the GPU tests send them: a good batch in front and behind, the case's first record byte at CASE_MIS
    for b in (G.fault_cases()[17], G.cut_cases()[5]):
        blob = G.with_neighbours(b)
        idx = M.index(blob, check_crc=True)[0]
        assert len(idx) == 3 and idx[1]["records_off"] % 16 == G.CASE_MIS
        assert M.verdict_all(blob, idx) == (1, 1) + b.expect


def test_every_valid_part_is_accepted():
    """Every window, base-valid and gather batch: accepted by the model with the totals the
    generator counted from its Record objects."""
    calls = [c for c in G.base_calls() + G.gather_calls() if c.verdict is None]
    assert len(calls) == 5 + 12
    for b in list(G.window_batches()) + [b for c in calls for b in c.batches]:
        blob = G.blob_of([b])
        out, offs, ct = M.unframe(blob, M.index(blob)[0])
        assert (len(out), ct["null_values"], ct["keyed"], ct["headers"], ct["records"]) == b.totals + (b.count,), b.name


def test_window_batches_cover_the_ring():
    """Computed from the batches' layout: all 16 residues; at each, every (width, split) of
    `length` at every edge (the full set: no reduction to four residues was taken); the step path
    and the skip path of ensure() each right in front of a straddling `length` at each residue;
    the ring's wrap; nine consecutive steps; record bytes ending at every residue and on an edge."""
    w = G.window_batches()
    placed = G.place(w)
    blob = G.blob_of(placed)
    idx = M.index(blob)[0]
    assert len(blob) <= 8 << 20 and len(idx) == 2 * len(w)
    for b, e in zip(placed, idx):
        assert b.mis is None or e["records_off"] % 16 == b.mis, b.name
    assert G.ALL_EDGES_AT == tuple(range(16))
    seen, ends, steps = set(), set(), {}
    for b in w:
        trace = G.ensure_trace(b.raw, b.mis)
        for edge, width, split, path in G.straddles(b.raw, b.mis):
            seen.add((b.mis, edge, width, split, path))
        ends.add((b.mis, (b.mis + len(b.raw)) % 16))
        if (b.mis + len(b.raw)) % G.WIN in (0, 1):
            ends.add((b.mis, "edge+%d" % ((b.mis + len(b.raw)) % G.WIN)))
        run = best = 0
        for _, _, _, path in trace:
            run = run + 1 if path == "step" else 0
            best = max(best, run)
        steps[b.mis] = max(steps.get(b.mis, 0), best)
    for mis in range(16):
        for edge in G.EDGES:
            for L in range(1, 6):
                for s in range(L + 1):
                    assert any((mis, edge, L, s, p) in seen for p in ("stay", "step", "skip")), (mis, edge, L, s)
        # a length that really lies across the edge (0 < split < width) behind each path
        for path, edge in (("step", 2 * G.WIN), ("skip", 3 * G.WIN), ("skip", 4 * G.WIN), ("stay", G.WIN)):
            assert {(mis, edge, 5, s, path) for s in (1, 2, 3, 4)} <= seen, (mis, path)
        assert steps[mis] >= 9
        assert {(mis, r) for r in range(16)} | {(mis, "edge+0"), (mis, "edge+1")} <= ends
    # the skip cases: a step first (cur is not 0), then the skip over two windows, then steps again
    for b in w:
        if "skip, then" in b.name:
            paths = [p for _, _, _, p in G.ensure_trace(b.raw, b.mis)]
            assert paths[:3] == ["first", "step", "skip"] and paths.count("step") >= 3, (b.name, paths)


def test_gather_calls_sit_on_the_chunk_edges():
    """Each chunk case has a value boundary within 2 bytes of a multiple of CHUNK counted from
    the first vector of the run's range, for every out_shift the GPU test uses; the run's end is
    within a byte of the edge; the shared-vector call's runs are 5 bytes each."""
    chunk = G.chunk_calls()
    assert len(chunk) == 6
    for c in chunk:
        marks = G.value_boundaries(c)
        assert len(marks) == G.RUN and min(abs(marks[-1] - k * G.CHUNK) for k in (1, 2)) <= 1
        for shift in G.OUT_SHIFTS:
            mis = shift % 16        # the first run starts at the output's first byte
            for k in range(1, round(marks[-1] / G.CHUNK) + 1):
                assert any(abs(mis + m - k * G.CHUNK) <= 2 for m in marks), (c.name, shift, k)
    shared = G.gather_calls()[0]
    blob = G.blob_of(shared.batches)
    offs = M.unframe(blob, M.index(blob)[0])[1]
    assert len(offs) == 4 * G.RUN + 1 and [offs[G.RUN * (j + 1)] - offs[G.RUN * j] for j in range(4)] == [5] * 4
    sizes = sorted(sum(b.count for b in c.batches) for c in G.gather_calls()[2:5])
    assert sizes == [G.RUN, G.RUN + 1, 2 * G.RUN]


def test_base_calls_differ_in_every_chunk():
    """Each counter's total differs between the chunks of BASE_STEP batches of the 600-batch call;
    the bad calls put a bad batch on both sides of the carry and first_bad behind another."""
    call = G.base_calls()[4]
    per_chunk = [tuple(sum(b.totals[k] for b in call.batches[c:c + G.BASE_STEP]) for k in range(4))
                 for c in range(0, 600, G.BASE_STEP)]
    for k in range(4):
        assert len({t[k] for t in per_chunk}) == len(per_chunk) == 3, (k, per_chunk)
    bad = [c for c in G.base_calls() if c.verdict]
    assert [c.verdict[:2] for c in bad] == [(1, 0), (1, 255), (1, 256), (1, 599), (2, 10), (3, 256)]
    rules = [[b.expect[1] for b in c.batches if b.expect] for c in bad]
    assert len(set(rules[4])) == 2 and len(set(rules[5])) == 3


def test_host_entries_agree_with_the_model_on_the_calls():
    """ysb_kafka_unframe_host (kafka.unframe_host, kafka.verdict) against the model on every base
    and gather call: values, offsets, counters; bad_batches, first_bad, record, rule."""
    for c in G.base_calls() + G.gather_calls():
        blob = G.blob_of(c.batches)
        midx = M.index(blob, check_crc=True)[0]
        idx, info = kafka.index(blob, check_crc=True)
        assert info["consumed"] == len(blob) and (idx == model_index_as_array(midx)).all(), c.name
        want = M.verdict_all(blob, midx)
        assert want == c.verdict, c.name
        got = kafka.verdict(blob, idx)
        if want is None:
            assert got["bad_batches"] == 0 and got["first_bad"] is None, c.name
            out, off, ct = kafka.unframe_host(blob, idx)
            mout, moff, mct = M.unframe(blob, midx)
            assert out.tobytes() == mout and list(off) == moff and ct == mct, c.name
        else:
            assert (got["bad_batches"], got["first_bad"], got["record"], got["rule"]) == want, c.name
