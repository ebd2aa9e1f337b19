"""CPU: the live map's rules (csrc/ysb_admap.h: what ysb_ad_map_upsert decides and places)
as a stand-alone native program, tests/native/upsert_logic.cpp -- no GPU, no HIP header."""
from test_capi import run_native


def test_upsert_logic_native(tmp_path):
    """The host model of an in-place upsert -- the eviction chains, searches and first-fit
    routine the device kernels call -- on tiny colliding tables and at a load's own sizes in
    both layouts, every key looked up by the host restatements of the scan's probes after each
    step; the in-place / rebuild rule at its three limits; the rebuild's merge against a load
    of all entries; later-wins, shards and the rejections of a call's records."""
    run_native(tmp_path, "upsert_logic")
