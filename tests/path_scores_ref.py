"""Restatement of the scores of a block of sample paths, independent of the library: THE definition of what the path-score entries
compute, bit for bit.

Scores: the CRPS of a univariate sample in its sorted form (the proper score of the n_paths values of one column at one step), the
rank of the actual among the paths (`below`, `equal`: PIT histograms, ties kept apart), the pinball loss of the sample's quantiles,
and the energy score of a range of columns in the estimator of Panagiotelis et al. 2023 (consecutive paths as the independent
copy).  The names and the contract are this package's own.

All arithmetic is plain fp64, one rounding per operation, nothing fused.  ONE order of addition serves every sum over paths and over
columns, the wave sum W: a_l is the serial sum from 0.0 of the terms t_i with i = l (mod 64), ascending in i (an empty class gives
0.0), and W = ((a_0 + a_1) + a_2) + ... + a_63.  Sums over steps and over paths of the energy score are serial from 0.0.

The scalar functions (`wave_sum`, `crps_one`, `energy_one`) are the statement, in Python floats; `scores` and `energy` are the same
on numpy arrays (elementwise fp64 operations only) and are checked against the scalar ones by tests/test_path_scores_cpu.py.

Nothing here imports the package under test.
"""
from __future__ import annotations

import math
import struct

import numpy as np

OK, NO_ACTUAL, NAN = 0, 1, 2
MAX_PATHS, MAX_LEVELS, MAX_ROWS = 2048, 16, 1 << 30
WAVE = 64


# ---- the order of addition ----
def wave_sum(terms):
    """W(t_0 ... t_{n-1}) in Python floats."""
    a = [0.0] * WAVE
    for i, t in enumerate(terms):
        a[i % WAVE] = a[i % WAVE] + float(t)
    w = a[0]
    for l in range(1, WAVE):
        w = w + a[l]
    return w


def wave_sum_axis0(t):
    """The same along axis 0 of an array [n, ...] -> [...]."""
    t = np.asarray(t, dtype=np.float64)
    a = np.zeros((WAVE,) + t.shape[1:])
    with np.errstate(invalid="ignore", over="ignore"):
        for lo in range(0, t.shape[0], WAVE):
            chunk = t[lo:lo + WAVE]
            a[:chunk.shape[0]] = a[:chunk.shape[0]] + chunk
        w = a[0].copy()
        for l in range(1, WAVE):
            w = w + a[l]
    return w


# ---- the total order of the sort ----
def order_key(x):
    """The total-order key of an fp64 value: unsigned order = value order, -0.0 below +0.0, a NaN beyond the infinity of its sign."""
    bits = struct.unpack("<Q", struct.pack("<d", float(x)))[0]
    return (~bits) & 0xFFFFFFFFFFFFFFFF if bits >> 63 else bits | (1 << 63)


def sort_total(values):
    return sorted([float(v) for v in values], key=order_key)


def _sort_axis0(cube):
    bits = np.ascontiguousarray(cube, dtype=np.float64).view(np.uint64)
    keys = np.sort(np.where(bits >> np.uint64(63) != 0, ~bits, bits | np.uint64(1 << 63)), axis=0)
    return np.ascontiguousarray(np.where(keys >> np.uint64(63) != 0, keys ^ np.uint64(1 << 63), ~keys)).view(np.float64)


# ---- one (column, step) ----
def crps_one(values, y):
    """The CRPS of the sample `values` against the actual y: W(|d_i|) / P - W((2i - P + 1) * d_i) / (P * P) on d_i = x_(i) - y."""
    s = sort_total(values)
    P = len(s)
    d = [x - float(y) for x in s]
    w1 = wave_sum([abs(v) for v in d])
    w2 = wave_sum([float(2 * i - P + 1) * v for i, v in enumerate(d)])
    return w1 / float(P) - w2 / (float(P) * float(P))


def ranks_one(values, y):
    """(below, equal): the paths with x < y and with x == y, IEEE comparisons."""
    return sum(1 for x in values if float(x) < float(y)), sum(1 for x in values if float(x) == float(y))


def compute_quantile(s, q):
    """Level q of a sorted list: s[lo] * (1 - frac) + s[up] * frac at index q * (P - 1); q <= 0 the first value, q >= 1 the last."""
    if q <= 0.0:
        return s[0]
    if q >= 1.0:
        return s[-1]
    n = len(s)
    idx = q * float(n - 1)
    lo = int(math.floor(idx))
    up = min(lo + 1, n - 1)
    frac = idx - float(lo)
    return s[lo] * (1.0 - frac) + s[up] * frac


def pinball_term(y, quantile, tau):
    e = y - quantile
    return tau * e if e >= 0.0 else (tau - 1.0) * e


def column_scores(column, actual_row, levels):
    """One column in Python floats.  column [P][h] (path p, step k), actual_row [h] -> dict of crps [h], below [h], equal [h],
    quantiles [L][h], crps_mean, n_steps, pinball [L], status."""
    P, h = len(column), len(actual_row)
    nan = math.nan
    if any(math.isnan(float(v)) for row in column for v in row):
        return {"crps": [nan] * h, "below": [-1] * h, "equal": [-1] * h, "quantiles": [[nan] * h for _ in levels], "crps_mean": nan,
                "n_steps": nan, "pinball": [nan] * len(levels), "status": NAN}
    crps, below, equal = [nan] * h, [-1] * h, [-1] * h
    quant = [[nan] * h for _ in levels]
    csum, psum, count = 0.0, [0.0] * len(levels), 0
    for k in range(h):
        vals = [float(column[p][k]) for p in range(P)]
        s = sort_total(vals)
        for l, tau in enumerate(levels):
            quant[l][k] = compute_quantile(s, float(tau))
        y = float(actual_row[k])
        if math.isnan(y):
            continue
        crps[k] = crps_one(vals, y)
        below[k], equal[k] = ranks_one(vals, y)
        csum = csum + crps[k]
        for l, tau in enumerate(levels):
            psum[l] = psum[l] + pinball_term(y, quant[l][k], float(tau))
        count += 1
    div = lambda v: v / float(count) if count else nan
    return {"crps": crps, "below": below, "equal": equal, "quantiles": quant, "crps_mean": div(csum), "n_steps": float(count),
            "pinball": [div(v) for v in psum], "status": OK if count else NO_ACTUAL}


# ---- a block ----
def scores(block, actual, horizon, n_paths, levels=(), n_cols=None):
    """block [n_paths * horizon, >= n_cols] time-major (row p * horizon + k), actual [n_cols, horizon] (NaN: no actual at that step).
    -> dict: crps fp64 [n_cols, h]; below, equal int32 [n_cols, h]; quantiles fp64 [L, n_cols, h]; column fp64 [2 + L, n_cols] in the
    rows crps_mean, n_steps, pinball_l; status int32 [n_cols] (OK, NO_ACTUAL: no step with an actual, every mean NaN; NAN: a NaN among
    the column's paths, every figure NaN, below and equal -1 -- it takes precedence)."""
    block = np.asarray(block, dtype=np.float64)
    P, h = int(n_paths), int(horizon)
    n = block.shape[1] if n_cols is None else int(n_cols)
    levels = [float(q) for q in levels]
    L = len(levels)
    cube = block[:P * h, :n].reshape(P, h, n)
    y = np.asarray(actual, dtype=np.float64).reshape(n, h).T             # [h, n]
    have = ~np.isnan(y)
    srt = _sort_axis0(cube)
    with np.errstate(invalid="ignore", over="ignore"):
        d = srt - y[None]
        weight = np.array([float(2 * i - P + 1) for i in range(P)]).reshape(P, 1, 1)
        w1 = wave_sum_axis0(np.abs(d))
        w2 = wave_sum_axis0(weight * d)
        crps = w1 / float(P) - w2 / (float(P) * float(P))
        below = (cube < y[None]).sum(axis=0).astype(np.int32)
        equal = (cube == y[None]).sum(axis=0).astype(np.int32)
        quant = np.empty((L, h, n))
        term = np.empty((L, h, n))
        for l, q in enumerate(levels):
            if q <= 0.0:
                v = srt[0]
            elif q >= 1.0:
                v = srt[P - 1]
            else:
                idx = q * float(P - 1)
                lo = int(math.floor(idx))
                up = min(lo + 1, P - 1)
                frac = idx - float(lo)
                v = srt[lo] * (1.0 - frac) + srt[up] * frac
            quant[l] = v
            e = y - v
            term[l] = np.where(e >= 0.0, q * e, (q - 1.0) * e)
        crps = np.where(have, crps, np.nan)
        below = np.where(have, below, -1).astype(np.int32)
        equal = np.where(have, equal, -1).astype(np.int32)
        column = np.zeros((2 + L, n))
        count = np.zeros(n)
        for k in range(h):                                               # serial over the steps that have an actual, in step order
            column[0] = np.where(have[k], column[0] + crps[k], column[0])
            for l in range(L):
                column[2 + l] = np.where(have[k], column[2 + l] + term[l, k], column[2 + l])
            count = count + have[k]
        column[1] = count
        for r in [0] + list(range(2, 2 + L)):
            column[r] = np.where(count > 0, column[r] / np.where(count > 0, count, 1.0), np.nan)
    status = np.where(count > 0, OK, NO_ACTUAL).astype(np.int32)
    bad = np.isnan(cube).any(axis=(0, 1))
    status[bad] = NAN
    crps, below, equal, quant = crps.T.copy(), below.T.copy(), equal.T.copy(), np.transpose(quant, (0, 2, 1)).copy()
    crps[bad] = np.nan
    below[bad] = -1
    equal[bad] = -1
    quant[:, bad, :] = np.nan
    column[:, bad] = np.nan
    return {"crps": crps, "below": below, "equal": equal, "quantiles": quant, "column": column, "status": status}


# ---- energy score ----
def distance(u, v):
    """sqrt(W((u_j - v_j)^2)): each square one rounded product, the root the correctly rounded one."""
    return math.sqrt(wave_sum([(float(a) - float(b)) * (float(a) - float(b)) for a, b in zip(u, v)]))


def energy_one(rows, y):
    """One step in Python floats: rows [P][m] (path p, column j of the range), y [m] -> es."""
    P = len(rows)
    s1 = 0.0
    for p in range(P):
        s1 = s1 + distance(rows[p], y)
    if P == 1:
        return s1
    s2 = 0.0
    for p in range(P - 1):
        s2 = s2 + distance(rows[p], rows[p + 1])
    return s1 / float(P) - s2 / (2.0 * float(P - 1))


def energy(block, actual, horizon, n_paths, col_begin=0, col_end=None):
    """The energy score of the columns [col_begin, col_end) of a block [n_paths * horizon, ld]; actual [>= col_end, horizon].
    -> dict: es fp64 [h]; es_mean (the serial sum of the non-NaN es in step order over their count es_steps; NaN when that is 0);
    es_steps; d1 fp64 [P, h] and d2 fp64 [P - 1, h], the distances the sums run over."""
    block = np.asarray(block, dtype=np.float64)
    P, h = int(n_paths), int(horizon)
    ce = block.shape[1] if col_end is None else int(col_end)
    cb = int(col_begin)
    assert 0 <= cb < ce <= block.shape[1]
    X = np.moveaxis(block[:P * h, cb:ce].reshape(P, h, ce - cb), 2, 0)   # [m, P, h]
    y = np.asarray(actual, dtype=np.float64)[cb:ce].reshape(ce - cb, 1, h)
    with np.errstate(invalid="ignore", over="ignore"):
        a = X - y
        d1 = np.sqrt(wave_sum_axis0(a * a))                              # [P, h]
        b = X[:, :-1] - X[:, 1:]
        d2 = np.sqrt(wave_sum_axis0(b * b)) if P > 1 else np.zeros((0, h))
        s1 = np.zeros(h)
        for p in range(P):
            s1 = s1 + d1[p]
        s2 = np.zeros(h)
        for p in range(P - 1):
            s2 = s2 + d2[p]
        es = s1 if P == 1 else s1 / float(P) - s2 / (2.0 * float(P - 1))
    total, count = 0.0, 0
    for k in range(h):
        if not math.isnan(float(es[k])):
            total = total + float(es[k])
            count += 1
    return {"es": es, "es_mean": total / float(count) if count else math.nan, "es_steps": count, "d1": d1, "d2": d2}


def same_bits(a, b):
    """Elementwise: equal bit patterns, or both NaN (the payload of a NaN is exempt; the sign of a zero is not)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
