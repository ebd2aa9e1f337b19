"""CPU: the parked views' rules (csrc/ysb_parked.h: what the park sites, the distinct kernel and
the resolve decide) as a stand-alone native program, tests/native/parked_logic.cpp -- no GPU,
no HIP header."""
from test_capi import run_native


def test_parked_logic_native(tmp_path):
    """The record's pack and unpack at key lengths 0, 1, 36 and 56; the distinct table's insert
    routine (the kernel's, with a plain compare-and-swap) on keys that collide in a 2-slot
    table, on a full table and at a context's capacity; the resolve rule (found with a good
    time, found with a bad time, not found, a foreign key never in the log, a full log); the
    ring-base rule."""
    run_native(tmp_path, "parked_logic")
