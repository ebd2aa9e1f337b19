"""CPU: the LDS window's and the ring base's rules (csrc/ysb_window.h) as a stand-alone native
program, tests/native/window_logic.cpp, plain and under the host sanitizers.  No GPU."""
import os
import subprocess

from test_capi import ROOT, run_native


def test_window_logic_native(tmp_path):
    """The rule functions at WL 2, 16 and 1024 for rel -1, 0, WL - 1 and WL, window set and unset,
    negative buckets; the ring base for (100, 16), (-3, 1024), (7, 4); a tile-by-tile model of
    the window built from the rules against a plain count."""
    run_native(tmp_path, "window_logic")


def test_window_logic_native_sanitized(tmp_path):
    """The same program with -fsanitize=address,undefined, as a stand-alone program."""
    exe = tmp_path / "window_logic_san"
    inc = [a for d in (("streaming-benchmarks_amd", "csrc"), ("include",)) for a in ("-I", os.path.join(ROOT, *d))]
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
                   + inc + [os.path.join(ROOT, "tests", "native", "window_logic.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK") and not r.stderr, r.stdout + r.stderr
