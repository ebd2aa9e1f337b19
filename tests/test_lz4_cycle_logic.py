"""CPU: the streaming replay's compressed cycle (host/ysb_replay_lz4.hpp: every batch of a replay
cycle as line-aligned LZ4 blocks that never span batches, one mapping, one directory) -- as a
stand-alone native program, tests/native/lz4_cycle_logic.cpp, built with g++ alone, plain and
under the host sanitizers; and the runner's CPU checks with --stream-lz4.  No GPU."""
import json
import os
import subprocess

import pytest

from test_capi import ROOT, run_native
from test_topology import EXE


def test_lz4_cycle_logic_native(tmp_path):
    """Cycles whose batches close by time and by slot bytes, at block sizes 64 B, 4 KiB and
    64 KiB: every batch's blocks decode to exactly its bytes, end behind a terminator, never span
    batches, stay within the slot; ranges and directory consistent; decode + rebase equals
    fill_batch for cycles 0, 1 and 7, with the raw bytes released as well."""
    run_native(tmp_path, "lz4_cycle_logic")


def test_lz4_cycle_logic_native_sanitized(tmp_path):
    """The same program with -fsanitize=address,undefined, as a stand-alone program."""
    exe = tmp_path / "lz4_cycle_logic_san"
    inc = [a for d in (("streaming-benchmarks_amd", "csrc"), ("streaming-benchmarks_amd", "host"), ("include",))
           for a in ("-I", os.path.join(ROOT, *d))]
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined"] + inc +
                   [os.path.join(ROOT, "tests", "native", "lz4_cycle_logic.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK") and not r.stderr, r.stdout + r.stderr


def check_line(*args):
    r = subprocess.run([EXE] + list(args), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("block", [None, 64, 65536])
def test_self_check_covers_the_compressed_cycle(block):
    """--stream-self-check --stream-lz4: every batch out of its blocks (the host model) equals
    fill_batch's bytes for cycle 0, and decoded and rebased the generator's own lines of cycles
    0, 1, 2, 7 and 1000."""
    s = check_line("--stream-self-check", "--stream-lz4", "--event-rate", "20000", "--batch-mb", "1", "--batch-ms", "130",
                   "--io-threads", "3", *(["--lz4-block", str(block)] if block else []))
    assert s["stream_lz4"] is True and s["lz4_block"] == (block or 8192)
    assert s["mismatched_batches"] == 0 and s["lz4_mismatched_batches"] == 0 and s["batches"] > 100
    assert 0 < s["lz4_comp_bytes"] <= s["lz4_raw_bytes"] and s["lz4_blocks"] >= s["batches"] // 5
    if block != 64:
        assert s["lz4_comp_bytes"] < 0.7 * s["lz4_raw_bytes"]
    plain = check_line("--stream-self-check", "--event-rate", "20000", "--batch-mb", "1", "--batch-ms", "130", "--io-threads", "3")
    assert plain["stream_lz4"] is False and plain["lines"] == s["lines"] and plain["mismatched_batches"] == 0


def test_feed_check_covers_the_compressed_cycle():
    s = check_line("--stream-feed-check", "--stream-lz4", "--shards", "2", "--event-rate", "20000", "--batch-mb", "1",
                   "--feed-seconds", "0.2", "--io-threads", "2")
    assert s["stream_lz4"] is True and s["lz4_mismatched_batches"] == 0 and 0 < s["lz4_comp_bytes"] < s["lz4_raw_bytes"]


@pytest.mark.parametrize("args,word", [(["--stream-lz4"], "--stream"),
                                       (["--stream", "--stream-lz4", "--replay", "copy"], "--replay copy"),
                                       (["--stream", "--stream-lz4", "--lz4-block", "0"], "--lz4-block")])
def test_stream_lz4_refusals_need_no_gpu(args, word):
    r = subprocess.run([EXE] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and word in r.stderr and len(r.stderr.strip().splitlines()) == 1
