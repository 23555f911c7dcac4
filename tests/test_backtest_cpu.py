"""The host half of the device backtest, without a GPU: the fold table of anofox_hip_backtest_folds against api.backtest_fold_bounds
on the full grid, the same function under ASan + UBSan in a stand-alone program, the sizing entry, and the numpy restatement the
GPU tests use (tests/backtest_ref.py) against backtest_metrics.backtest_metric."""
import ctypes as C
import itertools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import backtest_ref as R
from anofox_forecast_amd import api
from anofox_forecast_amd.backtest_metrics import backtest_metric

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS = ("expanding", "fixed", "sliding")
METRICS = ("mae", "mse", "mape", "smape", "bias", "r2", "coverage", "rmse", "no_such_metric")


def test_fold_table_equals_the_mirror_on_the_full_grid(hiplib):
    L = hiplib.load()
    fn = L.anofox_hip_backtest_folds
    buf = (hiplib.AnofoxHipFold * 8)()
    ints = np.frombuffer(buf, dtype=np.int64).reshape(8, 5)
    checked = 0
    grid = itertools.product(range(1, 6), range(1, 7), range(3), (1, 3, 50), (0, 1, 2), (0, 1, 2), (-1, 1, 10), (-1, 1, 3), (False, True))
    for horizon, folds, w, mts, gap, emb, init, skip, clip in grid:
        for n_dates in range(0, 41):
            want = api.backtest_fold_bounds(n_dates, horizon, folds, WINDOWS[w], mts, gap, emb, init, skip, clip)
            n = fn(n_dates, horizon, folds, w, mts, gap, emb, init, skip, clip, buf, 8)
            if n != len(want) or (n and ints[:n].tolist() != [list(t) for t in want]):
                raise AssertionError((n_dates, horizon, folds, WINDOWS[w], mts, gap, emb, init, skip, clip, want, ints[:n].tolist()))
            checked += 1
    assert checked == 41 * 5 * 6 * 3 * 3 * 3 * 3 * 3 * 3 * 2


def test_fold_table_count_call_capacity_and_python_wrapper(hiplib):
    L = hiplib.load()
    args = (30, 4, 5, 0, 1, 0, 0, -1, -1, False)
    want = api.backtest_fold_bounds(30, 4, 5)
    assert L.anofox_hip_backtest_folds(*args, None, 0) == len(want) == 5
    buf = (hiplib.AnofoxHipFold * 5)()
    for f in buf:
        f.fold_id = -7
    assert L.anofox_hip_backtest_folds(*args, buf, 2) == 5
    assert [f.fold_id for f in buf] == [1, 2, -7, -7, -7]
    assert hiplib.backtest_folds(30, 4, 5) == want
    # every window name that is not "expanding" cuts the window, as in the mirror
    assert hiplib.backtest_folds(30, 4, 5, "rolling", 6) == api.backtest_fold_bounds(30, 4, 5, "rolling", 6)


def test_sizes_entry(hiplib):
    folds = api.backtest_fold_bounds(48, 4, 3, "fixed", 5, 1, 2, -1, -1, True)
    tab = hiplib.make_folds(folds)
    assert hiplib.backtest_sizes(tab, len(folds), 67) == R.sizes(folds, 67) == (5, 201, 256)
    assert hiplib.backtest_sizes(tab, len(folds), 0) == (5, 0, 64)
    assert hiplib.backtest_sizes(tab, 0, 5) == (1, 0, 64)
    with pytest.raises(ValueError, match="pairs"):
        hiplib.backtest_sizes(tab, len(folds), 2 ** 31 - 1)
    bad = hiplib.make_folds([(1, -1, 3, 4, 5)])
    with pytest.raises(ValueError, match="negative"):
        hiplib.backtest_sizes(bad, 1, 4)


def test_fold_table_under_address_and_ub_sanitizers():
    """host_semantics.hpp is host-only C++: tests/c_abi/backtest_folds_san.cpp calls backtest_folds from its own main under
    ASan + UBSan (nothing is loaded into Python, nothing is preloaded)."""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "backtest_folds_san")
        subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               os.path.join(ROOT, "tests", "c_abi", "backtest_folds_san.cpp"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("OK "), (r.stdout, r.stderr[-2000:])


def _blocks(seed, n, h):
    rng = np.random.default_rng(seed)
    a = np.round(rng.normal(10.0, 4.0, (n, h)), 3)
    f = a + np.round(rng.normal(0.0, 1.5, (n, h)), 3)
    a[rng.random((n, h)) < 0.15] = 0.0                  # mape's filter
    both = rng.random((n, h)) < 0.1
    a[both] = 0.0
    f[both] = -0.0                                      # smape's filter: |a| + |f| = 0
    lo, hi = f - 1.0, f + 1.0
    return a, f, lo, hi


@pytest.mark.parametrize("metric", METRICS)
def test_reference_score_equals_backtest_metric(metric):
    """backtest_ref.score (plain loops) and backtest_metric (numpy cumulative sums) give the same bits, also on the filters' edge cases."""
    a, f, lo, hi = _blocks(5, 9, 7)
    cases = [(a.ravel(), f.ravel(), lo.ravel(), hi.ravel()), (a[0, :1], f[0, :1], lo[0, :1], hi[0, :1]),
             (np.zeros(5), np.zeros(5), np.zeros(5), np.zeros(5)), (np.full(6, 3.5), f[1, :6], lo[1, :6], hi[1, :6]),
             (np.array([]), np.array([]), np.array([]), np.array([])), (np.array([-0.0, -0.0]), np.array([0.0, 0.0]), np.zeros(2), np.zeros(2))]
    for x, y, l, u in cases:
        want = backtest_metric(metric, x, y, l, u)
        assert R.same_bits(np.array([R.score(metric, x, y, l, u)]), np.array([want])), (metric, len(x), want)


def test_reference_expand_and_collect_against_the_mirror_rules():
    """backtest_ref.expand / collect cut what api.ts_backtest_native's loops cut: the same windows, the same test rows."""
    rng = np.random.default_rng(11)
    folds = api.backtest_fold_bounds(30, 4, 3, "fixed", 5, 1, 2, -1, -1, True)
    lens = [0, 2, 17, 18, 19, 20, 22, 25, 30, 30]
    y = np.zeros((30, 64))
    for s, n in enumerate(lens):
        y[:n, s] = rng.normal(size=n)
    block, len_pairs, n_test = R.expand(y, np.array(lens), folds, len(lens))
    F = len(folds)
    for s, n in enumerate(lens):
        for f, (fid, tr0, tr1, te0, te1) in enumerate(folds):
            p = s * F + f
            if tr1 >= n or te0 >= n or tr0 > tr1:
                assert len_pairs[p] == 0 and n_test[p] == 0 and not block[:, p].any()
                continue
            assert len_pairs[p] == tr1 - tr0 + 1 and n_test[p] == len(range(te0, min(te1, n - 1) + 1))
            assert np.array_equal(block[:len_pairs[p], p], y[tr0:tr1 + 1, s]) and not block[len_pairs[p]:, p].any()
    assert not block[:, len(lens) * F:].any()
    status = np.zeros(len(lens) * F, dtype=np.int32)
    status[8 * F + 1] = 3
    yhat = rng.normal(size=(len(lens) * F, 4))
    actual, error, abs_error, valid, n_rows = R.collect(y, folds, len(lens), n_test, status, yhat)
    assert n_rows[8 * F + 1] == 0 and np.isnan(actual[8 * F + 1]).all()
    assert np.array_equal(n_rows[status == 0], np.minimum(n_test[:len(status)][status == 0], 4))
    assert np.array_equal(valid.astype(bool), ~np.isnan(actual)) and np.array_equal(np.isnan(actual), np.isnan(error))
