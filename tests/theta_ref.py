"""CPU checker of the dynamic Theta models (DynamicTheta, DynamicOptimizedTheta), vectorised over series.

It restates, operation for operation, what csrc/fit_theta.hip computes, so that the GPU results can be compared to it bit for
bit (the library is built with -ffp-contract=off; every step here is one IEEE operation, as there).  It belongs to the tests
only: the product never imports it.

The model is the state-space Theta method of Fiorucci et al. (2016), dynamic form.  For one series y[0..n) (NULLs already
interpolated, seasonally adjusted when the season test says so) and parameters (l0, alpha, theta), with q = 1 - alpha and
k = 1 - 1/theta:
  * start: level = alpha*y0 + q*l0, mean = y0, A = y0, B = 0, p = 1 (p holds (1 - alpha)^t as a running product);
  * step t >= 1 (x = y[t], or mu itself past the end of the series):
        p = p*q;  mu = level + k*(A*p + B*(1 - p*q)/alpha);  e = x - mu;  sse += e*e   (t < n only)
        level = alpha*x + q*level;  B = ((t-1)*B + 6*(x - mean)/(t+1))/(t+2);  mean = (t*mean + x)/(t+1);  A = mean - B*(t+2)/2
  * objective: sse / (n - 1); a non-finite value counts as +inf;
  * forecasts: mu of the steps t = n .. n+h-1.
DynamicTheta: l0 = y0, alpha = 0.1, theta = 2 (no optimiser).  DynamicOptimizedTheta: (l0, alpha, theta) by the project's
bounded Nelder-Mead (nm.hpp semantics: scipy's coefficients, 1.05 simplex, clipping, xatol 1e-4, fatol 1e-8, 600 evaluations /
iterations) from (y0/2, 0.5, 2) within [-1e10, 1e10] x [0.1, 0.99] x [1, 1e10], written as a masked per-series state machine
that evaluates exactly one point per pass, as the kernel does.

Seasonal path (period m > 1, n >= 2m, every y > 0): the season test is |r_m| > 1.645 sqrt((1 + 2 sum_{k<m} r_k^2) / n) on the
autocorrelations r_k of y; when it holds, y is divided by classical multiplicative indices (centred moving average of order m,
a 2 x m one for even m, as a running window sum; mean ratio y / trend per phase t % m; indices scaled to mean 1) and the forecasts
are multiplied by them.  Otherwise the model is fitted on y itself.
"""
from __future__ import annotations

import numpy as np

MODELS = ("DynamicTheta", "DynamicOptimizedTheta")
NOT_SHIPPED = ("Theta", "OptimizedTheta", "AutoTheta")
DSTM_ALPHA = 0.1
DSTM_THETA = 2.0
NM_DIM = 3
NM_MAX = 200 * NM_DIM
LO = np.array([-1.0e10, 0.1, 1.0])
HI = np.array([1.0e10, 0.99, 1.0e10])
SEASON_Z = 1.645

# phases of the Nelder-Mead state machine (csrc/fit_theta.hip)
P_INIT, P_REFL, P_EXP, P_OC, P_IC, P_SHRINK, P_DONE = 0, 1, 2, 3, 4, 5, 6


def _as_block(series):
    """(S, T) float64 block and lengths from a list of 1-D arrays (ragged: padded with 1.0, never read)."""
    lens = np.array([len(y) for y in series], dtype=np.int64)
    T = int(lens.max()) if len(series) else 0
    Y = np.ones((len(series), max(T, 1)), dtype=np.float64)
    for s, y in enumerate(series):
        Y[s, :len(y)] = np.asarray(y, dtype=np.float64)
    return Y, lens


def season_indices(Y, lens, m):
    """(S, m) multiplicative indices and the per-series flag 'adjusted' (theta_season_kernel)."""
    with np.errstate(divide="ignore", invalid="ignore"):        # (series that are not adjusted divide by zeros on the way)
        return _season_indices(Y, lens, m)


def _season_indices(Y, lens, m):
    S, T = Y.shape
    idx = np.ones((S, max(m, 1)))
    if m <= 1:
        return idx, np.zeros(S, dtype=bool)
    n = lens.astype(np.float64)
    live = lambda t: t < lens
    # mean and positivity
    tot = np.zeros(S)
    pos = np.ones(S, dtype=bool)
    for t in range(T):
        lv = live(t)
        tot = np.where(lv, tot + Y[:, t], tot)
        pos = pos & (~lv | (Y[:, t] > 0.0))
    ok = (lens >= 2 * m) & pos
    mean = tot / np.maximum(n, 1.0)
    # autocorrelations r_1..r_m: one sweep per lag
    d = np.zeros(S)
    for t in range(T):
        dv = Y[:, t] - mean
        d = np.where(live(t), d + dv * dv, d)
    acc = np.zeros(S)
    rm = np.zeros(S)
    for k in range(1, m + 1):
        c = np.zeros(S)
        for t in range(k, T):
            c = np.where(live(t), c + (Y[:, t] - mean) * (Y[:, t - k] - mean), c)
        r = c / np.where(d > 0.0, d, 1.0)
        if k < m:
            acc = acc + r * r
        else:
            rm = r
    lim = SEASON_Z * np.sqrt((1.0 + 2.0 * acc) / np.maximum(n, 1.0))
    ok = ok & (d > 0.0) & (np.abs(rm) > lim)
    # centred moving average as a running window sum over [t - hw, t + hw], ratios summed per phase
    hw = m // 2
    even = m % 2 == 0
    W = np.zeros(S)
    for j in range(min(2 * hw, T)):
        W = W + np.where(j < lens, Y[:, j], 0.0)
    sums = np.zeros((S, m))
    for t in range(hw, T - hw):
        cen = (t + hw) < lens
        W = np.where(cen, W + Y[:, t + hw], W)
        tr = (W - 0.5 * Y[:, t - hw] - 0.5 * Y[:, t + hw]) / m if even else W / m
        ph = t % m
        sums[:, ph] = np.where(cen, sums[:, ph] + Y[:, t] / tr, sums[:, ph])
        W = np.where(cen, W - Y[:, t - hw], W)
    # phase counts over t in [hw, n - 1 - hw]
    ssum = np.zeros(S)
    for j in range(m):
        first = hw + ((j - hw) % m)
        last = lens - 1 - hw
        cnt = np.where(last >= first, (last - first) // m + 1, 0).astype(np.float64)
        idx[:, j] = sums[:, j] / np.maximum(cnt, 1.0)
        ssum = ssum + idx[:, j]
    mu = ssum / m
    for j in range(m):
        idx[:, j] = idx[:, j] / mu
    idx = np.where(ok[:, None], idx, 1.0)
    return idx, ok


def _adjusted(Y, lens, m):
    idx, ok = season_indices(Y, lens, m)
    X = Y.copy()
    if m > 1:
        for t in range(Y.shape[1]):
            X[:, t] = np.where(ok, Y[:, t] / idx[:, t % m], Y[:, t])
    return X, idx, ok


def theta_pass(X, lens, l0, alpha, theta, h=0):
    """Objective (sse / (n - 1), non-finite -> +inf) and the h forecasts of the dynamic model, vectorised over series."""
    S, T = X.shape
    q = 1.0 - alpha
    k = 1.0 - 1.0 / theta
    y0 = X[:, 0]
    level = alpha * y0 + q * l0
    mean = y0.copy()
    A = y0.copy()
    B = np.zeros(S)
    p = np.ones(S)
    sse = np.zeros(S)

    def step(t, x, level, mean, A, B, p):
        p = p * q
        mu = level + k * (A * p + B * (1.0 - p * q) / alpha)
        xx = mu if x is None else x
        level_n = alpha * xx + q * level
        B_n = ((t - 1) * B + 6.0 * (xx - mean) / (t + 1)) / (t + 2)
        mean_n = (t * mean + xx) / (t + 1)
        A_n = mean_n - B_n * (t + 2) / 2.0
        return mu, level_n, mean_n, A_n, B_n, p

    for t in range(1, T):
        lv = t < lens
        mu, l2, m2, A2, B2, p2 = step(t, X[:, t], level, mean, A, B, p)
        e = X[:, t] - mu
        sse = np.where(lv, sse + e * e, sse)
        level = np.where(lv, l2, level); mean = np.where(lv, m2, mean)
        A = np.where(lv, A2, A); B = np.where(lv, B2, B); p = np.where(lv, p2, p)
    f = sse / (lens - 1).astype(np.float64)
    f = np.where(np.isfinite(f), f, np.inf)
    fc = np.zeros((S, h))
    # past the end: each series continues from its own length
    for i in range(h):
        t = (lens + i).astype(np.float64)
        mu, level, mean, A, B, p = step(t, None, level, mean, A, B, p)
        fc[:, i] = mu
    return f, fc


def _nm_dotm(X, lens):
    """(l0, alpha, theta) of every series by the masked Nelder-Mead state machine (theta_fit_kernel): one point per series and
    pass; the transitions follow oracle/ets.c nm_minimize exactly."""
    S = X.shape[0]
    D = NM_DIM
    rows = np.arange(S)
    x0 = np.stack([X[:, 0] / 2.0, np.full(S, 0.5), np.full(S, 2.0)], axis=1)
    sim = np.zeros((S, D + 1, D))
    fs = np.zeros((S, D + 1))
    sim[:, 0] = np.minimum(np.maximum(x0, LO), HI)
    for kk in range(D):
        sim[:, kk + 1] = sim[:, 0]
        v = sim[:, 0, kk]
        v = np.where(v != 0.0, 1.05 * v, 0.00025)
        sim[:, kk + 1, kk] = np.minimum(np.maximum(v, LO[kk]), HI[kk])
    phase = np.where(lens >= 2, P_INIT, P_DONE)
    sub = np.zeros(S, dtype=np.int64)
    evals = np.zeros(S, dtype=np.int64)
    iters = np.ones(S, dtype=np.int64)
    xb = np.zeros((S, D)); xr = np.zeros((S, D)); fr = np.zeros(S)

    def clip(v):
        return np.minimum(np.maximum(v, LO), HI)

    def swap(mask, i, j):
        a, b = fs[:, i].copy(), fs[:, j].copy()
        fs[:, i] = np.where(mask, b, a); fs[:, j] = np.where(mask, a, b)
        xa, xc = sim[:, i].copy(), sim[:, j].copy()
        sim[:, i] = np.where(mask[:, None], xc, xa); sim[:, j] = np.where(mask[:, None], xa, xc)

    def sort_all(mask):
        # stable: D bubble passes of strict compare-and-swap
        for _ in range(D):
            for j in range(D):
                swap(mask & (fs[:, j + 1] < fs[:, j]), j, j + 1)

    def accept(mask, xn, fn):
        # replace the worst vertex, one backward bubble pass (the new vertex goes after every equal value)
        sim[:, D] = np.where(mask[:, None], xn, sim[:, D])
        fs[:, D] = np.where(mask, fn, fs[:, D])
        for j in range(D, 0, -1):
            swap(mask & (fs[:, j] < fs[:, j - 1]), j - 1, j)

    def begin_iteration(mask):
        small = np.ones(S, dtype=bool)
        for kk in range(1, D + 1):
            small &= np.all(np.abs(sim[:, kk] - sim[:, 0]) <= 1.0e-4, axis=1)
            small &= np.abs(fs[:, 0] - fs[:, kk]) <= 1.0e-8
        stop = mask & ((evals >= NM_MAX) | (iters >= NM_MAX) | small)
        go = mask & ~stop
        c = sim[:, 0].copy()
        for kk in range(1, D):
            c = c + sim[:, kk]
        xb[:] = np.where(go[:, None], c / float(D), xb)
        phase[:] = np.where(stop, P_DONE, np.where(go, P_REFL, phase))

    def trial(which):
        xw = sim[:, D]
        if which == 0:
            return clip(2.0 * xb - 1.0 * xw)
        if which == 1:
            return clip(3.0 * xb - 2.0 * xw)
        if which == 2:
            return clip(1.5 * xb - 0.5 * xw)
        return clip(0.5 * xb + 0.5 * xw)

    while True:
        ph = phase.copy()
        act = ph != P_DONE
        if not act.any():
            break
        pt = sim[rows, np.minimum(sub, D)].copy()
        for p_, w in ((P_REFL, 0), (P_EXP, 1), (P_OC, 2), (P_IC, 3)):
            msk = ph == p_
            if msk.any():
                pt = np.where(msk[:, None], trial(w), pt)
        f = np.full(S, np.inf)
        a_idx = np.nonzero(act)[0]
        f[a_idx], _ = theta_pass(X[a_idx], lens[a_idx], pt[a_idx, 0], pt[a_idx, 1], pt[a_idx, 2])
        evals = np.where(act, evals + 1, evals)
        end_it = np.zeros(S, dtype=bool)
        shrink = np.zeros(S, dtype=bool)
        # INIT / SHRINK: store the value, next vertex; after the last one sort (and, for INIT, start iterating)
        for p_ in (P_INIT, P_SHRINK):
            m = ph == p_
            if m.any():
                fs[rows[m], sub[m]] = f[m]
                sub = np.where(m, sub + 1, sub)
                fin = m & (sub > D)
                sort_all(fin)
                if p_ == P_INIT:
                    begin_iteration(fin)
                else:
                    end_it |= fin
        m = ph == P_REFL
        if m.any():
            xr = np.where(m[:, None], pt, xr)
            fr = np.where(m, f, fr)
            e_ = m & (f < fs[:, 0])
            keep = m & ~e_ & (f < fs[:, D - 1])
            oc = m & ~e_ & ~keep & (f < fs[:, D])
            ic = m & ~e_ & ~keep & ~oc
            accept(keep, pt, f)
            end_it |= keep
            phase[e_] = P_EXP
            phase[oc] = P_OC
            phase[ic] = P_IC
        m = ph == P_EXP
        if m.any():
            t_e = f < fr
            accept(m, np.where(t_e[:, None], pt, xr), np.where(t_e, f, fr))
            end_it |= m
        m = ph == P_OC
        if m.any():
            ok = m & (f <= fr)
            accept(ok, pt, f)
            end_it |= ok
            shrink |= m & ~ok
        m = ph == P_IC
        if m.any():
            ok = m & (f < fs[:, D])
            accept(ok, pt, f)
            end_it |= ok
            shrink |= m & ~ok
        if shrink.any():
            for kk in range(1, D + 1):
                v = clip(sim[:, 0] + 0.5 * (sim[:, kk] - sim[:, 0]))
                sim[:, kk] = np.where(shrink[:, None], v, sim[:, kk])
            sub = np.where(shrink, 1, sub)
            phase[shrink] = P_SHRINK
        if end_it.any():
            iters = np.where(end_it, iters + 1, iters)
            begin_iteration(end_it)
    return sim[:, 0].copy(), fs[:, 0].copy(), evals


def forecast(series, model, h, period=1):
    """(S, h) point forecasts, the per-series 'adjusted' flag and, for DynamicOptimizedTheta, the fitted (l0, alpha, theta) and
    evaluation counts.  Series of length 0 give NaN rows; lengths 1 and 2 are the host's INSUFFICIENT_DATA and are not used."""
    if model not in MODELS:
        raise ValueError(model)
    Y, lens = _as_block(series)
    S = len(series)
    X, idx, ok = _adjusted(Y, lens, period)
    if model == "DynamicTheta":
        par = np.stack([X[:, 0], np.full(S, DSTM_ALPHA), np.full(S, DSTM_THETA)], axis=1)
        evals = np.zeros(S, dtype=np.int64)
    else:
        par, _, evals = _nm_dotm(X, lens)
    _, fc = theta_pass(X, lens, par[:, 0], par[:, 1], par[:, 2], h)
    if period > 1:
        for i in range(h):
            ph = (lens + i) % period
            fc[:, i] = np.where(ok, fc[:, i] * idx[np.arange(S), ph], fc[:, i])
    fc[lens == 0] = np.nan
    return fc, ok, par, evals
