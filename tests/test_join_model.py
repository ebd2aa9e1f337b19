"""CPU: the joined-views model (tests/join_model.py) against the committed fixtures.  Summing the
per-line oracle runs reproduces the committed stats, and the expected streams are not empty:
they contain misses and time errors.  No GPU."""
import pytest

import golden_data as gd
import join_model as jm

# fixture -> (lines, joined rows, time errors among them, join misses); None: not pinned here
TOTALS = {"edge": (54, 32, 5, 4), "edge_long": (None, 41, None, None), "edge_orgjson": (None, 34, None, None),
          "gen_s7": (1500, 506, None, None), "edge_tbl": (21, 12, 3, 2)}


@pytest.fixture(scope="module")
def model():
    return jm.Model(*gd.ad_arrays())


def _batch(model, stem, require_ip=False):
    if stem in gd.TBL_FILES:
        raw, offs = gd.tbl_events(stem)
        return jm.lines_of(raw, offs), model.batch(raw, offs, fmt="tbl"), gd.expected(stem)
    raw, offs = gd.events(stem)
    return jm.lines_of(raw, offs), model.batch(raw, offs, require_ip=require_ip), gd.expected(stem, require_ip)


@pytest.mark.parametrize("stem,require_ip", gd.FIXTURES + [(s, False) for s in gd.TBL_FIXTURES])
def test_per_line_runs_sum_to_the_committed_expectation(model, stem, require_ip):
    lines, (cols, st), (rows, est) = _batch(model, stem, require_ip)
    for k in jm.STATS:
        assert st[k] == est[k], k
    assert jm.histogram(cols) == rows
    assert len(cols["row"]) == st["joined"] and int((cols["time_ok"] == 0).sum()) == st["time_errors"]
    assert (cols["row"][1:] > cols["row"][:-1]).all()
    assert (cols["event_time"][cols["time_ok"] == 0] == 0).all()


@pytest.mark.parametrize("stem", sorted(TOTALS))
def test_expected_streams_hold_rows_misses_and_time_errors(model, stem):
    lines, (cols, st), _ = _batch(model, stem)
    n, joined, terr, miss = TOTALS[stem]
    assert len(cols["row"]) == joined
    if n is not None:
        assert len(lines) == n
    if terr is not None:
        assert st["time_errors"] == terr and st["join_misses"] == miss
