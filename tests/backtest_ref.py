"""Naive numpy restatement of the device backtest (expand, collect, fold score) from the fold table and the operator's rules
(ts_backtest_native.cpp:785-790 for the pairs it keeps, :796-830 for the rows, :280-373 for the metric).  Shares no code with the
library; the GPU tests compare the kernels with it bit for bit."""
import math

import numpy as np


def pair_rule(fold, n):
    """(live, window length, test rows) of a series of n rows under fold (fold_id, train_start, train_end, test_start, test_end)."""
    _, tr0, tr1, te0, te1 = fold
    if tr1 >= n or te0 >= n or tr0 > tr1:
        return False, 0, 0
    rows = min(te1, n - 1) - te0 + 1
    if rows <= 0:
        return False, 0, 0
    return True, tr1 - tr0 + 1, rows


def sizes(folds, n_series):
    t_train = max([1] + [f[2] - f[1] + 1 for f in folds])
    n_pairs = n_series * len(folds)
    return t_train, n_pairs, max(64, (n_pairs + 63) // 64 * 64)


def expand(y, lengths, folds, n_series):
    """y [t_rows, ld] time-major -> (block [t_train, ld_pairs], len_pairs, n_test)."""
    F = len(folds)
    t_train, n_pairs, ld_pairs = sizes(folds, n_series)
    block = np.zeros((t_train, ld_pairs))
    len_pairs = np.zeros(ld_pairs, dtype=np.int32)
    n_test = np.zeros(ld_pairs, dtype=np.int32)
    for s in range(n_series):
        n = min(max(int(lengths[s]), 0), y.shape[0])
        for f, fold in enumerate(folds):
            live, L, rows = pair_rule(fold, n)
            if not live:
                continue
            p = s * F + f
            block[:L, p] = y[fold[1]:fold[2] + 1, s]
            len_pairs[p], n_test[p] = L, rows
    return block, len_pairs, n_test


def collect(y, folds, n_series, n_test, status, yhat):
    """-> (actual, error, abs_error, valid, n_rows); rows that do not exist are NaN / 0."""
    F, h = len(folds), yhat.shape[1]
    n_pairs = n_series * F
    actual = np.full((n_pairs, h), np.nan)
    error = np.full((n_pairs, h), np.nan)
    abs_error = np.full((n_pairs, h), np.nan)
    valid = np.zeros((n_pairs, h), dtype=np.uint8)
    n_rows = np.zeros(n_pairs, dtype=np.int32)
    for s in range(n_series):
        for f, fold in enumerate(folds):
            p = s * F + f
            if n_test[p] <= 0 or status[p] != 0:
                continue
            k = min(int(n_test[p]), h)
            actual[p, :k] = y[fold[3]:fold[3] + k, s]
            error[p, :k] = yhat[p, :k] - actual[p, :k]
            abs_error[p, :k] = np.abs(error[p, :k])
            valid[p, :k] = 1
            n_rows[p] = k
    return actual, error, abs_error, valid, n_rows


def fold_rows(f, F, n_series, n_rows, *blocks):
    """The rows of fold index f in the operator's order (series, then steps) of every block."""
    out = [[] for _ in blocks]
    for s in range(n_series):
        p = s * F + f
        for i in range(int(n_rows[p])):
            for o, b in zip(out, blocks):
                o.append(b[p, i])
    return [np.array(o, dtype=np.float64) for o in out]


def score(metric, a, f, lo=None, hi=None):
    """ComputeMetric with plain Python loops: every sum runs in row order, one operation per step."""
    n = len(a)
    if n == 0:
        return math.nan

    def run(terms):
        it = iter(terms)
        total = next(it)
        for v in it:
            total = total + v
        return total
    a = [np.float64(v) for v in a]
    f = [np.float64(v) for v in f]
    with np.errstate(all="ignore"):
        if metric == "mae":
            return run(abs(x - y) for x, y in zip(a, f)) / n
        if metric == "mse":
            return run((x - y) * (x - y) for x, y in zip(a, f)) / n
        if metric == "mape":
            t = [abs((x - y) / x) for x, y in zip(a, f) if x != 0]
            return run(t) / len(t) * 100.0 if t else math.nan
        if metric == "smape":
            t = [abs(x - y) / (abs(x) + abs(y)) for x, y in zip(a, f) if abs(x) + abs(y) > 0]
            return run(t) / len(t) * 200.0 if t else math.nan
        if metric == "bias":
            return run(y - x for x, y in zip(a, f)) / n
        if metric == "r2":
            mean = run(a) / n
            res = run((x - y) * (x - y) for x, y in zip(a, f))
            tot = run((x - mean) * (x - mean) for x in a)
            return 1.0 - res / tot if tot > 0 else math.nan
        if metric == "coverage":
            if lo is None or hi is None:
                return math.nan
            return sum(1 for x, l, u in zip(a, lo, hi) if l <= x <= u) / n
        return float(np.sqrt(run((x - y) * (x - y) for x, y in zip(a, f)) / n))


def same_bits(x, y):
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return x.shape == y.shape and bool(np.all((x.view(np.uint64) == y.view(np.uint64)) | (np.isnan(x) & np.isnan(y))))
