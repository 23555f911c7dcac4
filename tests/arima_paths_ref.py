"""Restatement of the sample paths simulated from fitted ARIMA models (anofox_hip_arima_innovations_device,
anofox_hip_arima_paths_device and what is built on them): THE definition of what those entries compute, bit for bit.

Method: the fitted recursion simulated forward and the differences integrated (Box & Jenkins; Hyndman & Athanasopoulos, Forecasting:
Principles and Practice, "Prediction intervals from simulated paths"), in the convention of AnofoxHipArimaFit and arima_ref,
    (1 - phi(B)) (1 - Phi(B^m)) (w_t - c) = (1 - theta(B)) (1 - Theta(B^m)) e_t,     w = (1 - B)^d (1 - B^m)^D y,
w the seasonal difference first, then the d ordinary ones, each a single subtraction; c = constant with has_constant, else 0.0.

Arithmetic: fp64, one rounding per operation, nothing fused, in this order.
  - The lag polynomials are not multiplied out.  A side is the sum over the terms (i, j), 0 <= i <= p, 0 <= j <= P, without (0, 0), of
    coefficient * value at lag i + j m, the coefficient phi_i, Phi_j or -(phi_i * Phi_j); terms on the same lag stay separate; they are
    added j-major, i-minor from acc = 0.0 (`terms`, `_side`).  A value before the differenced series is 0.0 and is multiplied and
    added like any other.  The MA side is the same with theta, Theta on e.
  - x_t = w_t - c.  In sample (the CSS recursion of arima_ref.css): e_t = 0.0 for t < La = p + m P, e_t = (x_t - ar) + ma for
    t = La .. n_diff - 1; css = their serial sum of squares from 0.0, nu = n_diff - La, sigma = sqrt(css / nu).
  - A path: for k = 0 .. h - 1, t = n_diff + k: x_t = (ar + e_t) - ma, v = x_t + c; d == 2: last_d1 = last_d1 + v, v = last_d1;
    d >= 1: last_d0 = last_d0 + v, v = last_d0; D == 1: v = v + y_(n + k - m), from the history for k < m, else the path's own value.
    With u the seasonally differenced series (u = y for D = 0): last_d0 = u[-1], last_d1 = u[-1] - u[-2].
  - Nothing is clamped.  A step whose value is not finite is NaN and so is every later step of the path.

Draws.  Gaussian: the rule of ets_paths_ref with the last counter word 3 (so the stream is not the ETS one): counter (p, s, k >> 2, 3),
words (w0, w1) serve steps 4j and 4j + 1, (w2, w3) steps 4j + 2 and 4j + 3 by ets_paths_ref.normal_pair, e = sigma z.  Bootstrap: the
index rule and the counters of paths_ref unchanged on the series' own nu residuals; joint: draw j < pool_rows takes residual row
nu - pool_rows + j of every series (the same date for series that end together).

Status per series: NO_MODEL (4) for orders outside p, q <= 5, P, Q <= 2, d <= 2, D <= 1, has_constant 0 / 1, a length < 1, an n_diff that
is not length - d - D m (a series without a fit has the zero orders and n_diff 0 of the fit block), nu < 1, or a resid_length that is
not nu; then RAGGED (3; joint: nu < pool_rows), EMPTY (1; joint: pool_rows 0), NAN (2): a NaN in a coefficient the orders read, in
sigma (Gaussian), in the last La + d + D m observations, in the last min(nu, q + m Q) residuals or (bootstrap) in the pool's rows.

The blocks: orders int32 [8, ld] rows p, d, q, P, D, Q, has_constant, n_diff; coef fp64 [16, ld] rows phi 1..5, theta 1..5, Phi 1..2,
Theta 1..2, constant, aicc; y fp64 [T, ld] time-major; resid fp64 [T, ld] compacted: row j of a column is e at index La + j.

Tolerances against arima_ref (80-bit), 16 x the worst deviation over the families of tests/arima_cases.py (measured by
tests/test_arima_paths_cpu.py, which prints every figure):
"""
from __future__ import annotations

import numpy as np

import ets_paths_ref as E
import paths_ref as P

FORECAST_REL = 1.6e-14            # zero-innovation paths against arima_ref.forecast, relative to max |y|      # measured 9.536e-16 (differencing)
CSS_REL = 1.5e-13                 # css and sigma^2 against arima_ref.css, relative                           # measured 9.010e-15 (box)
INNOVATION_REL = 2.7e-12          # the innovations against arima_ref.css, relative to their root mean square  # measured 1.687e-13 (box)

OK, EMPTY, NAN, RAGGED, NO_MODEL = 0, 1, 2, 3, 4
GAUSSIAN, BOOTSTRAP = 0, 1
MAX_PERIOD, MAX_LDS_ROWS = 2048, 128
F = np.float64


def lds_rows(m, horizon):
    """The LDS rows a wave of the device kernel needs: two rings of min(h, 2 m + 5) and the y ring of m when m < h."""
    m, h = int(m), int(horizon)
    return 2 * min(h, 2 * m + 5) + (m if m < h else 0)


# ---- fits and blocks ----
def blocks_of(fits, ld, lengths=None, m=None):
    """A list of arima_ref-style fit dicts (None: no fit) -> (orders int32 [8, ld], coef fp64 [16, ld]).  n_diff is the dict's, or
    lengths[s] - d - D m."""
    orders = np.zeros((8, ld), dtype=np.int32)
    coef = np.full((16, ld), np.nan)
    for s, f in enumerate(fits):
        if f is None:
            continue
        mm = int(f.get("m", m) if m is None else m)
        orders[:7, s] = [f["p"], f["d"], f["q"], f["P"], f["D"], f["Q"], 1 if f["has_constant"] else 0]
        orders[7, s] = f["n_diff"] if "n_diff" in f else int(lengths[s]) - f["d"] - f["D"] * mm
        coef[:15, s] = 0.0
        for row, key, k in ((0, "phi", 5), (5, "theta", 5), (10, "Phi", 2), (12, "Theta", 2)):
            v = list(f.get(key, []))[:k]
            coef[row:row + len(v), s] = v
        coef[14, s] = f.get("constant", 0.0) if f["has_constant"] else 0.0
        coef[15, s] = f.get("aicc", 0.0)
    return orders, coef


def fit_of(orders, coef, s, m):
    """Column s of the blocks as an arima_ref fit dict (the coefficients the orders read)."""
    p, d, q, Ps, D, Q, c, nd = (int(v) for v in orders[:8, s])
    return {"p": p, "d": d, "q": q, "P": Ps, "D": D, "Q": Q, "m": int(m), "has_constant": bool(c), "n_diff": nd,
            "phi": [F(v) for v in coef[0:p, s]], "theta": [F(v) for v in coef[5:5 + q, s]], "Phi": [F(v) for v in coef[10:10 + Ps, s]],
            "Theta": [F(v) for v in coef[12:12 + Q, s]], "constant": F(coef[14, s]) if c else F(0.0)}


def has_model(orders_col, length, m, t_rows, resid_length=None):
    """-> (n, n_diff, La) or None.  `length` is cut to [0, t_rows]."""
    p, d, q, Ps, D, Q, c, nd = (int(v) for v in orders_col[:8])
    if not (0 <= p <= 5 and 0 <= q <= 5 and 0 <= Ps <= 2 and 0 <= Q <= 2 and 0 <= d <= 2 and 0 <= D <= 1 and c in (0, 1)):
        return None
    n = min(max(int(length), 0), int(t_rows))
    n_diff, La = n - d - D * int(m), p + int(m) * Ps
    if int(length) < 1 or n < 1 or nd != n_diff or n_diff - La < 1:
        return None
    if resid_length is not None and int(resid_length) != n_diff - La:
        return None
    return n, n_diff, La


def terms(c1, c2, m):
    """[(lag, coefficient)] of one side, j-major and i-minor, without (0, 0)."""
    out = []
    for j in range(len(c2) + 1):
        for i in range(len(c1) + 1):
            if i == 0 and j == 0:
                continue
            if j == 0:
                c = F(c1[i - 1])
            elif i == 0:
                c = F(c2[j - 1])
            else:
                c = -(F(c1[i - 1]) * F(c2[j - 1]))
            out.append((i + j * int(m), c))
    return out


def _sides(fit, m):
    """The terms of the AR and of the MA side of a fit (the coefficients its orders read)."""
    return (terms(fit["phi"][:fit["p"]], fit["Phi"][:fit["P"]], m), terms(fit["theta"][:fit["q"]], fit["Theta"][:fit["Q"]], m))


def difference(y, d, D, m):
    """fp64: the seasonal difference first, then the ordinary ones."""
    w = np.asarray(y, dtype=F).copy()
    with np.errstate(all="ignore"):
        for _ in range(int(D)):
            w = w[m:] - w[:-m]
        for _ in range(int(d)):
            w = w[1:] - w[:-1]
    return w


def _side(tms, t, past, sim=None, origin=0):
    """The sum of a side at index t: `past` holds the values of indices < origin (0.0 before index 0), `sim` [paths, h] those from
    `origin` on.  Scalar fp64 without `sim`, else one value per path."""
    acc = F(0.0) if sim is None else np.zeros(sim.shape[0])
    for lag, c in tms:
        i = t - lag
        if sim is not None and i >= origin:
            v = sim[:, i - origin]
        else:
            v = F(past[i]) if i >= 0 else F(0.0)
        acc = acc + c * v
    return acc


def css_one(fit, y):
    """One series: -> (x, e, css, nu, sigma) with x [n_diff] the differenced series less the constant and e [n_diff] (0.0 below La)."""
    m = int(fit["m"])
    with np.errstate(all="ignore"):
        x = difference(y, fit["d"], fit["D"], m) - F(fit["constant"] if fit["has_constant"] else 0.0)
        ar_t, ma_t = _sides(fit, m)
        La, n = fit["p"] + m * fit["P"], len(x)
        e = np.zeros(n)
        css = F(0.0)
        for t in range(La, n):
            e[t] = (x[t] - _side(ar_t, t, x)) + _side(ma_t, t, e)
            css = css + e[t] * e[t]
        nu = n - La
        sigma = np.sqrt(css / F(nu))
    return x, e, css, nu, sigma


def simulate(fit, y, x, e_past, draws):
    """One series: draws fp64 [n_paths, h] -> paths [n_paths, h].  x, e_past: the differenced series less the constant and its
    innovations (index 0 .. n_diff - 1)."""
    y = np.asarray(y, dtype=F)
    m, d, D = int(fit["m"]), int(fit["d"]), int(fit["D"])
    n, nd = len(y), len(x)
    n_paths, h = draws.shape
    c = F(fit["constant"] if fit["has_constant"] else 0.0)
    ar_t, ma_t = _sides(fit, m)
    xs, out = np.zeros((n_paths, h)), np.full((n_paths, h), np.nan)
    broken = np.zeros(n_paths, dtype=bool)
    with np.errstate(all="ignore"):
        u = y[m:] - y[:-m] if D else y
        l0 = np.full(n_paths, u[-1]) if d >= 1 else None
        l1 = np.full(n_paths, u[-1] - u[-2]) if d == 2 else None
        for k in range(h):
            t = nd + k
            xk = (_side(ar_t, t, x, xs, nd) + draws[:, k]) - _side(ma_t, t, e_past, draws, nd)
            v = xk + c
            if d == 2:
                l1 = l1 + v
                v = l1
            if d >= 1:
                l0 = l0 + v
                v = l0
            if D:
                v = v + (y[n + k - m] if k < m else out[:, k - m])
            broken = broken | ~np.isfinite(v)
            out[:, k] = np.where(broken, np.nan, v)
            xs[:, k] = xk
    return out


# ---- draws ----
def normal_draws(seed, n_series, n_paths, horizon):
    """fp64 [n_paths, horizon, n_series]: z of every (path, step, series), counter (p, s, k >> 2, 3)."""
    p = np.arange(n_paths, dtype=np.uint64).reshape(-1, 1, 1)
    b = np.arange((horizon + 3) // 4, dtype=np.uint64).reshape(1, -1, 1)
    s = np.arange(n_series, dtype=np.uint64).reshape(1, 1, -1)
    w = P.philox_words(p, s, b, np.uint64(3), seed)
    blocks = w.shape[2]
    z = np.empty((n_paths, blocks, 4, n_series))
    z[:, :, 0], z[:, :, 1] = E.normal_pair(w[0], w[1])
    z[:, :, 2], z[:, :, 3] = E.normal_pair(w[2], w[3])
    return z.reshape(n_paths, blocks * 4, n_series)[:, :horizon, :]


# ---- the entries ----
def innovations(orders, coef, y, lengths, m, n_series=None):
    """-> (resid fp64 [T, n] compacted, NaN where nothing is written; resid_lengths int32 [n] = nu, 0 without a model; sigma fp64 [n],
    NaN without a model)."""
    y = np.asarray(y, dtype=F)
    T = y.shape[0]
    n = len(lengths) if n_series is None else int(n_series)
    resid, lens, sigma = np.full((T, n), np.nan), np.zeros(n, dtype=np.int32), np.full(n, np.nan)
    for s in range(n):
        hm = has_model(orders[:, s], lengths[s], m, T)
        if hm is None:
            continue
        _, e, _, nu, sg = css_one(fit_of(orders, coef, s, m), y[:hm[0], s])
        resid[:nu, s], lens[s], sigma[s] = e[hm[2]:], nu, sg
    return resid, lens, sigma


def series_status(orders_col, coef_col, y_col, length, resid_col, resid_length, sigma, m, innovations_mode, joint=False, pool_rows=0):
    hm = has_model(orders_col, length, m, len(y_col), resid_length)
    if hm is None:
        return NO_MODEL
    n, n_diff, La = hm
    p, d, q, Ps, D, Q, c, _ = (int(v) for v in orders_col[:8])
    nu, boot = n_diff - La, innovations_mode == BOOTSTRAP
    if boot and joint and nu < int(pool_rows):
        return RAGGED
    if boot and joint and int(pool_rows) == 0:
        return EMPTY
    read = list(coef_col[0:p]) + list(coef_col[5:5 + q]) + list(coef_col[10:10 + Ps]) + list(coef_col[12:12 + Q]) + ([coef_col[14]] if c else [])
    tail = min(n, La + d + D * int(m))
    read += list(y_col[n - tail:n])
    first = nu - min(nu, q + int(m) * Q)
    if boot:
        first = min(first, nu - int(pool_rows)) if joint else 0
    read += list(resid_col[first:nu])
    if not boot:
        read.append(sigma)
    return NAN if any(np.isnan(F(v)) for v in read) else OK


def paths(orders, coef, y, lengths, resid, resid_lengths, sigma, m, n_paths, horizon, innovations=GAUSSIAN, joint=False, pool_rows=0, seed=0,
          n_series=None, draws=None):
    """-> (block fp64 [n_paths * horizon, n], row p * horizon + k; status int32 [n]; n_broken int32 [n]: the paths that hold a NaN).
    `draws` fp64 [n_paths, horizon, n] replaces the drawn innovations (the CPU tests: zeros, hand-set values)."""
    y, resid = np.asarray(y, dtype=F), np.asarray(resid, dtype=F)
    m, h = int(m), int(horizon)
    n = len(lengths) if n_series is None else int(n_series)
    assert 1 <= m <= MAX_PERIOD and lds_rows(m, h) <= MAX_LDS_ROWS and not (joint and innovations == GAUSSIAN)
    pool_rows = int(pool_rows) if (joint and innovations == BOOTSTRAP) else 0
    status = np.array([series_status(orders[:, s], coef[:, s], y[:, s], lengths[s], resid[:, s], resid_lengths[s], sigma[s], m, innovations,
                                     joint, pool_rows) for s in range(n)], dtype=np.int32)
    if draws is None and innovations == GAUSSIAN:
        z = normal_draws(seed, n, n_paths, h)
    elif draws is None:
        u = P.draws(seed, n, n_paths, h, joint)
    block = np.full((n_paths, h, n), np.nan)
    for s in np.flatnonzero(status == OK):
        nn, n_diff, La = has_model(orders[:, s], lengths[s], m, y.shape[0])
        nu = n_diff - La
        fit = fit_of(orders, coef, s, m)
        with np.errstate(all="ignore"):
            x = difference(y[:nn, s], fit["d"], fit["D"], m) - fit["constant"]
            if draws is not None:
                e = np.asarray(draws[:, :, s], dtype=F)
            elif innovations == GAUSSIAN:
                e = F(sigma[s]) * z[:, :, s]
            else:
                cut = pool_rows if joint else nu
                j = ((u[:, :, s] * np.uint64(cut)) >> np.uint64(32)).astype(np.int64)
                e = resid[(nu - pool_rows if joint else 0) + j, s]
        e_past = np.concatenate([np.zeros(La), resid[:nu, s]])
        block[:, :, s] = simulate(fit, y[:nn, s], x, e_past, e)
    n_broken = np.isnan(block).any(axis=1).sum(axis=0).astype(np.int32)
    return block.reshape(n_paths * h, n), status, n_broken
