"""CPU checker of the intermittent-demand models (CrostonClassic, CrostonSBA, TSB, ADIDA, IMAPA), vectorised over series.

It restates, operation for operation, what csrc/fit_intermittent.hip computes, so that the GPU results can be compared to it
bit for bit (the library is built with -ffp-contract=off; every step here is one IEEE mul or add, as there).  It belongs to the
tests only: the product never imports it.

For one series y[0..n) (NULLs already interpolated):
  * a demand is any y[t] != 0, at indices i_0 < ... < i_{c-1}; sizes z_j = y[i_j], intervals p_0 = i_0 + 1, p_j = i_j - i_{j-1};
  * SES(x, a): l = x[0]; for t >= 1: e = x[t] - l; sse += e*e; l = l + a*e (the forecast is the final l);
  * CrostonClassic = SES(z, 0.1) / SES(p, 0.1); CrostonSBA = 0.95 * that; TSB = SES(d, 0.1) * SES(z, 0.1), d[t] = (y[t] != 0);
  * K = round half up of (i_{c-1} + 1) / c (the mean interval), in integers: (2 (i_{c-1} + 1) + c) // (2 c);
  * level-k sums: drop the first n % k observations, sum each following block of k, left to right, starting from 0.0;
  * SESopt(x): alpha in [0.1, 0.3] by 16 passes of a 9-point grid refine (first minimum of sse; the bounds are exact grid points);
  * ADIDA = SESopt(level-K sums) / K; IMAPA = (sum over k = 1..K, in level order, of SESopt(level-k sums) / k) / K;
  * no demand at all: every model forecasts 0.0.
"""
from __future__ import annotations

import numpy as np

MODELS = ("CrostonClassic", "CrostonSBA", "TSB", "ADIDA", "IMAPA")
ALPHA = 0.1
SBA_FACTOR = 0.95
GRID_PASSES = 16
GRID_POINTS = 9


def _as_block(series):
    """(S, T) float64 block and lengths from a list of 1-D arrays (ragged: padded with 0.0, never read)."""
    lens = np.array([len(y) for y in series], dtype=np.int64)
    T = int(lens.max()) if len(series) else 0
    Y = np.zeros((len(series), max(T, 1)), dtype=np.float64)
    for s, y in enumerate(series):
        Y[s, :len(y)] = np.asarray(y, dtype=np.float64)
    return Y, lens


def croston_state(Y, lens):
    """One pass over the rows, as croston_kernel: SES levels of sizes, intervals and the demand indicator, the demand count and K."""
    S, T = Y.shape
    lz = np.zeros(S); lp = np.zeros(S); ldem = np.zeros(S)
    c = np.zeros(S, dtype=np.int64)
    last = np.full(S, -1, dtype=np.int64)
    a = ALPHA
    for t in range(T):
        live = t < lens
        v = Y[:, t]
        dem = live & (v != 0.0)
        d = np.where(v != 0.0, 1.0, 0.0)
        if t == 0:
            ldem = np.where(live, d, ldem)
        else:
            e = d - ldem
            ldem = np.where(live, ldem + a * e, ldem)
        p = (t - last).astype(np.float64)
        first = dem & (c == 0)
        upd = dem & (c > 0)
        ez = v - lz
        ep = p - lp
        lz = np.where(first, v, np.where(upd, lz + a * ez, lz))
        lp = np.where(first, p, np.where(upd, lp + a * ep, lp))
        c = np.where(dem, c + 1, c)
        last = np.where(dem, t, last)
    K = np.where(c > 0, (2 * (last + 1) + c) // np.maximum(2 * c, 1), 0)
    return lz, lp, ldem, c, K


def level_sums(Y, lens, k):
    """(S, max blocks) level-k sums (left to right from 0.0) and the block counts; rows past a series' blocks are 0.0."""
    S = Y.shape[0]
    nb = lens // k
    off = lens % k
    B = int(nb.max()) if S else 0
    X = np.zeros((S, max(B, 1)))
    j = np.arange(max(B, 1))
    T = Y.shape[1]
    rows = np.arange(S)[:, None]
    for r in range(k):
        idx = off[:, None] + j[None, :] * k + r
        X = X + np.where(j[None, :] < nb[:, None], Y[rows, np.minimum(idx, T - 1)], 0.0)
    return X, nb


def ses_opt(X, nb):
    """SESopt over the rows of X (row s has nb[s] >= 1 values): the final level at the selected alpha."""
    S, B = X.shape
    lo = np.full(S, 0.1)
    hi = np.full(S, 0.3)
    jstar = np.zeros(S, dtype=np.int64)
    l = np.zeros((GRID_POINTS, S))
    jj = np.arange(GRID_POINTS, dtype=np.float64)[:, None]
    for _ in range(GRID_PASSES):
        step = (hi - lo) / 8.0
        a = lo[None, :] + jj * step[None, :]
        a[8] = hi
        l = np.broadcast_to(X[:, 0], (GRID_POINTS, S)).copy()
        sse = np.zeros((GRID_POINTS, S))
        for b in range(1, B):
            live = (b < nb)[None, :]
            x = X[:, b][None, :]
            e = x - l
            sse = np.where(live, sse + e * e, sse)
            l = np.where(live, l + a * e, l)
        best = sse[0].copy()
        jstar = np.zeros(S, dtype=np.int64)
        for j in range(1, GRID_POINTS):
            u = sse[j] < best
            best = np.where(u, sse[j], best)
            jstar = np.where(u, j, jstar)
        cols = np.arange(S)
        lo_new = a[np.maximum(jstar - 1, 0), cols]
        hi_new = a[np.minimum(jstar + 1, 8), cols]
        lo, hi = lo_new, hi_new
    return l[jstar, np.arange(S)]


def point_forecasts(series, model):
    """One flat point forecast per series (np.float64 array); series of length 0 give NaN."""
    Y, lens = _as_block(series)
    S = len(series)
    lz, lp, ldem, c, K = croston_state(Y, lens)
    out = np.zeros(S)
    has = c > 0
    if model == "CrostonClassic":
        out = np.where(has, lz / np.where(has, lp, 1.0), 0.0)
    elif model == "CrostonSBA":
        out = np.where(has, SBA_FACTOR * (lz / np.where(has, lp, 1.0)), 0.0)
    elif model == "TSB":
        out = np.where(has, ldem * lz, 0.0)
    elif model == "ADIDA":
        for k in np.unique(K[has]):
            sel = np.nonzero(has & (K == k))[0]
            X, nb = level_sums(Y[sel], lens[sel], int(k))
            out[sel] = ses_opt(X, nb) / float(k)
    elif model == "IMAPA":
        acc = np.zeros(S)
        for k in range(1, int(K.max()) + 1 if S and has.any() else 1):
            sel = np.nonzero(has & (K >= k))[0]
            X, nb = level_sums(Y[sel], lens[sel], k)
            acc[sel] = acc[sel] + ses_opt(X, nb) / float(k)
        out = np.where(has, acc / np.maximum(K, 1).astype(np.float64), 0.0)
    else:
        raise ValueError(model)
    out[lens == 0] = np.nan
    return out


def aggregation_level(series):
    """K of every series (0 where there is no demand)."""
    Y, lens = _as_block(series)
    return croston_state(Y, lens)[4]
