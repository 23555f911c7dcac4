"""Numpy checker of the ARIMAX path (csrc/fit_exog.hip), operation for operation.

The reference (forecast.rs forecast_with_exog -> forecast_arima_with_exog) regresses y on the regressors with an intercept, runs
its in-tree ARIMA (a fixed-0.5 AR(1) on the first differences; naive below 5 observations) on the residuals and adds
intercept + sum beta_j future_j.  Its least-squares solver is an external crate; ours is stated here and is what the kernel runs:

  * ybar = (sum_t y_t) / n, xbar_j = (sum_t x_jt) / n -- every sum sequential in time order, one accumulator each;
  * S_jk = sum_t (x_jt - xbar_j)(x_kt - xbar_k) for k <= j, g_j = sum_t (x_jt - xbar_j)(y_t - ybar);
  * Cholesky of S in column order without pivoting: v = S_jj - sum over the USED k < j of L_jk^2; regressor j is used iff
    v > 1e-10 S_jj (false for NaN); then L_jj = sqrt(v), L_ij = (S_ij - sum over the used k < j of L_ik L_jk) / L_jj for i > j.
    An unused regressor is skipped everywhere: it is never multiplied, so a NaN in it cannot reach a result;
  * forward and back substitution over the used regressors give beta_j; b0 = ybar - sum over the used j (ascending) of beta_j xbar_j;
  * r_t = y_t - (b0 + sum over the used j (ascending) of beta_j x_jt);
  * residual forecast: n < 5 -> r_{n-1}; else md = (sum_{t>=1} (r_t - r_{t-1})) / (n - 1), prev = r_{n-1} - r_{n-2}, cum = r_{n-1},
    per step nd = md + 0.5 (prev - md), cum += nd, prev = nd (forecast.rs:1391-1431);
  * point_i = residual forecast_i + (b0 + sum over the used j (ascending) of beta_j future_j[i]).

Every product and sum is a separate IEEE operation (the kernels are built with -ffp-contract=off), vectorised here over the SERIES
axis only, so a batch of ragged series is computed with exactly the per-series operations.  The intervals are the generic rule on y
(forecast.rs:2558-2591): point -/+ (z sd) sqrt(step) with the population sd of y.
"""
import numpy as np

MAX_REGRESSORS = 8
TOL = 1e-10


def z_for_confidence(c):
    return 2.576 if c >= 0.99 else 1.96 if c >= 0.95 else 1.645 if c >= 0.90 else 1.28 if c >= 0.80 else 1.0


def _blocks(series, xregs, futures):
    n = len(series)
    K = len(xregs[0]) if n else 0
    h = len(futures[0][0]) if n and K else 0
    lens = np.array([len(y) for y in series], dtype=np.int64)
    T = int(lens.max()) if n else 0
    Y = np.zeros((T, n))
    X = np.zeros((K, T, n))
    F = np.zeros((K, h, n))
    for s in range(n):
        Y[:lens[s], s] = series[s]
        for j in range(K):
            X[j, :lens[s], s] = xregs[s][j]
            F[j, :, s] = futures[s][j]
    return Y, lens, X, F


def fit_batch(series, xregs, futures):
    """series[s]: y of length n_s (no NULLs); xregs[s][j]: regressor j, length n_s; futures[s][j]: length h.
    Returns dict(point [n x h], b0 [n], beta [n x K] (0.0 where unused), used [n x K] bool).  Series shorter than 1 give NaN."""
    Y, lens, X, F = _blocks(series, xregs, futures)
    K, T, n = X.shape
    h = F.shape[1]
    assert 1 <= K <= MAX_REGRESSORS
    dn = lens.astype(np.float64)
    with np.errstate(all="ignore"):
        # sweep 1
        ybar = np.zeros(n)
        xbar = np.zeros((K, n))
        for t in range(T):
            m = t < lens
            ybar = np.where(m, ybar + Y[t], ybar)
            for j in range(K):
                xbar[j] = np.where(m, xbar[j] + X[j, t], xbar[j])
        ybar = ybar / dn
        for j in range(K):
            xbar[j] = xbar[j] / dn
        # sweep 2
        L = [[np.zeros(n) for k in range(j + 1)] for j in range(K)]
        g = [np.zeros(n) for j in range(K)]
        for t in range(T):
            m = t < lens
            dy = Y[t] - ybar
            d = [X[j, t] - xbar[j] for j in range(K)]
            for j in range(K):
                g[j] = np.where(m, g[j] + d[j] * dy, g[j])
                for k in range(j + 1):
                    L[j][k] = np.where(m, L[j][k] + d[j] * d[k], L[j][k])
        # Cholesky in place
        used = [np.zeros(n, dtype=bool) for j in range(K)]
        for j in range(K):
            sjj = L[j][j]
            v = sjj.copy()
            for k in range(j):
                v = np.where(used[k], v - L[j][k] * L[j][k], v)
            used[j] = v > TOL * sjj
            ljj = np.sqrt(np.where(used[j], v, 1.0))
            L[j][j] = np.where(used[j], ljj, L[j][j])
            for i in range(j + 1, K):
                w = L[i][j]
                for k in range(j):
                    w = np.where(used[k], w - L[i][k] * L[j][k], w)
                L[i][j] = np.where(used[j], w / ljj, L[i][j])
        # substitutions
        z = [None] * K
        for j in range(K):
            w = g[j]
            for k in range(j):
                w = np.where(used[k], w - L[j][k] * z[k], w)
            z[j] = np.where(used[j], w / np.where(used[j], L[j][j], 1.0), 0.0)
        beta = [np.zeros(n) for j in range(K)]
        for j in range(K - 1, -1, -1):
            w = z[j]
            for i in range(j + 1, K):
                w = np.where(used[i], w - L[i][j] * beta[i], w)
            beta[j] = np.where(used[j], w / np.where(used[j], L[j][j], 1.0), 0.0)
        b0 = ybar.copy()
        for j in range(K):
            b0 = np.where(used[j], b0 - beta[j] * xbar[j], b0)
        # sweep 3
        sum_diff = np.zeros(n)
        r_last = np.zeros(n)
        r_prev = np.zeros(n)
        for t in range(T):
            m = t < lens
            e = b0
            for j in range(K):
                e = np.where(used[j], e + beta[j] * X[j, t], e)
            r = Y[t] - e
            if t > 0:
                sum_diff = np.where(m, sum_diff + (r - r_last), sum_diff)
            r_prev = np.where(m, r_last, r_prev)
            r_last = np.where(m, r, r_last)
        mean_diff = sum_diff / (dn - 1.0)
        prev = r_last - r_prev
        cum = r_last.copy()
        point = np.zeros((n, h))
        long_enough = lens >= 5
        for i in range(h):
            nd = mean_diff + 0.5 * (prev - mean_diff)
            cum = cum + nd
            prev = nd
            rf = np.where(long_enough, cum, r_last)
            e = b0
            for j in range(K):
                e = np.where(used[j], e + beta[j] * F[j, i], e)
            point[:, i] = rf + e
    bad = lens < 1
    point[bad] = np.nan
    return {"point": point, "b0": np.where(bad, np.nan, b0), "beta": np.array(beta).T.copy() if K else np.zeros((n, 0)),
            "used": np.array(used).T.copy() if K else np.zeros((n, 0), bool)}


def fit(y, xreg, future):
    """One series: y [n], xreg [K][n], future [K][h] -> (point [h], b0, beta [K], used [K])."""
    r = fit_batch([np.asarray(y, dtype=np.float64)], [[np.asarray(c, dtype=np.float64) for c in xreg]],
                  [[np.asarray(c, dtype=np.float64) for c in future]])
    return r["point"][0], float(r["b0"][0]), r["beta"][0], r["used"][0]


def residuals(y, xreg, b0, beta, used):
    """r_t of one series, as sweep 3 forms them."""
    y = np.asarray(y, dtype=np.float64)
    e = np.full(len(y), b0)
    for j in range(len(beta)):
        if used[j]:
            e = e + beta[j] * np.asarray(xreg[j], dtype=np.float64)
    return y - e


def toy_arima(r, h):
    """forecast.rs:1391-1431 on one series."""
    n = len(r)
    if n < 5:
        return np.full(h, r[-1])
    sd = 0.0
    for i in range(1, n):
        sd = sd + (r[i] - r[i - 1])
    md = sd / float(n - 1)
    prev = r[-1] - r[-2]
    cum = r[-1]
    out = np.empty(h)
    for i in range(h):
        nd = md + 0.5 * (prev - md)
        cum = cum + nd
        out[i] = cum
        prev = nd
    return out


def intervals(y, point, confidence=0.95):
    """lower, upper of one series by the generic rule on y (prep_kernel's mean / sd, interval_kernel)."""
    y = np.asarray(y, dtype=np.float64)
    n = len(y)
    s = 0.0
    for v in y:
        s = s + v
    mean = s / float(n)
    var = 0.0
    for v in y:
        dv = v - mean
        var = var + dv * dv
    sd = np.sqrt(var / float(n))
    z = z_for_confidence(confidence)
    wd = (z * sd) * np.sqrt(np.arange(1, len(point) + 1, dtype=np.float64))
    return point - wd, point + wd
