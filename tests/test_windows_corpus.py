"""CPU: the boundary corpus of tests/windows_corpus.py -- its jdiv model, the C oracle and the
Python oracle agree at every divisor and layout, and the corpus meets the conditions that
keep the GPU comparison (tests/test_gpu_windows.py) from passing vacuously."""
import pytest

import windows_corpus as wc
from oracle import dostats, oracle


@pytest.fixture(scope="module")
def admap():
    return oracle.AdMap(*wc.ad_arrays())


def test_jdiv_truncates_toward_zero():
    assert [wc.jdiv(t, 10) for t in (-11, -10, -9, -1, 0, 1, 9, 10, 11)] == [-1, -1, 0, 0, 0, 0, 0, 1, 1]
    assert wc.jdiv(wc.LONG_MIN, 1) == wc.LONG_MIN and wc.jdiv(wc.LONG_MIN, wc.LONG_MAX) == -1
    assert wc.jdiv(wc.LONG_MAX, wc.LONG_MAX) == 1 and wc.jdiv(wc.LONG_MAX - 1, wc.LONG_MAX) == 0
    for d in wc.D:
        for t in wc.boundary_times(d):
            q = wc.jdiv(t, d)
            r = t - q * d                      # Java: (t / d) * d + t % d == t, |t % d| < d, sign of t
            assert abs(r) < d and (r == 0 or (r < 0) == (t < 0))
            assert wc.LONG_MIN <= q * d <= wc.LONG_MAX     # window_ms = bucket * d never overflows


def test_boundary_times_and_forms():
    assert wc.LONG_MAX not in wc.boundary_times(1) and wc.LONG_MIN not in wc.boundary_times(1)
    for d in wc.D:
        ts = wc.boundary_times(d)
        assert len(ts) == len(set(ts)) and all(wc.LONG_MIN <= t <= wc.LONG_MAX for t in ts)
        assert {0, 1, -1, d, d - 1, -d, -d + 1, 1 << 62, -(1 << 62), wc.LONG_MAX - 1, wc.LONG_MIN + 1} <= set(ts)
        assert (d < 2) != (wc.LONG_MAX in ts and wc.LONG_MIN in ts)
    lens = {len(s) for s in wc.forms(1_700_000_000_000)}
    assert {13, 14, 19, 20, 21} <= lens
    assert "-0" in wc.forms(0) and "+0" in wc.forms(0) and "0" * 21 in wc.forms(0)
    assert {len(s) for s in wc.forms(-5)} >= {2, 13, 14, 20, 21}
    for t in (0, -5, 7, wc.LONG_MAX, wc.LONG_MIN):
        for s in wc.forms(t):
            assert dostats.parse_long(s) == t


@pytest.mark.parametrize("fmt,layout", wc.LAYOUTS)
def test_carriers_are_joined_views(admap, fmt, layout):
    """The carrier lines themselves, with the fixture's own times: every one a joined view."""
    pairs = wc.carrier_lines(fmt, layout)
    lines = [p[0] for p in pairs]
    raw, offs = wc.batch(lines)
    rows, st = oracle.run(admap, raw, offs, fmt=fmt)
    assert st["joined"] == st["events"] == len(lines) > 300
    assert st["time_errors"] == st["parse_errors"] == st["join_misses"] == 0
    by_campaign = {}
    for _, c in pairs:
        by_campaign[c] = by_campaign.get(c, 0) + 1
    got = {}
    for (c, _), v in rows.items():
        got[c] = got.get(c, 0) + v
    assert got == by_campaign and len(by_campaign) == 10


@pytest.mark.parametrize("fmt,layout", wc.LAYOUTS)
@pytest.mark.parametrize("d", wc.D)
def test_model_and_both_oracles_agree(admap, d, fmt, layout):
    lines, rows, stats = wc.build(d, fmt, layout)
    raw, offs = wc.batch(lines)
    c_rows, c_st = oracle.run(admap, raw, offs, divisor=d, fmt=fmt)
    py = dostats.run(lines, dict(zip(*wc.ad_arrays())), divisor=d, fmt=fmt)
    assert c_st == stats and py.stats() == stats
    assert c_rows == rows and py.counts == rows
    # the conditions of the corpus, on the reference
    assert c_st["joined"] == len(lines) and len(lines) < 1024
    assert c_st["time_errors"] == c_st["parse_errors"] == c_st["join_misses"] == 0
    buckets = {b for _, b in c_rows}
    assert 0 in buckets and min(buckets) < 0
    if d <= 86_400_000:
        assert len({b for b in buckets if b < 0}) >= 3 and len({b for b in buckets if b > 0}) >= 3
    # bucket 0 is the one window 2d - 1 ms wide: both of its ends are in the corpus
    recs = wc.records(d, fmt, layout)
    zero = {t for _, _, t in recs if wc.jdiv(t, d) == 0}
    assert {-(d - 1), d - 1} <= zero


def test_gpu_variants_of_the_corpus():
    """bound (the d = 1 GPU runs) and smallest_first (the auto-base case) select and reorder,
    nothing else."""
    full = wc.records(1, "json", "generator")
    inside = wc.records(1, "json", "generator", bound=1 << 62)
    assert {t for _, _, t in full} - {t for _, _, t in inside} == {wc.LONG_MAX - 1, wc.LONG_MIN + 1}
    assert max(abs(t) for _, _, t in inside) == 1 << 62
    for d in (2, 10000):
        a = wc.records(d, "tbl", "tbl")
        b = wc.records(d, "tbl", "tbl", smallest_first=True)
        assert sorted(t for _, _, t in a) == sorted(t for _, _, t in b)
        assert b[0][2] == min(t for _, _, t in a)
        assert wc.rows_of(b, d).keys() >= {(b[0][1], wc.jdiv(b[0][2], d))}
