"""A textbook restatement of what an AutoARIMA fit MEANS, in 80-bit arithmetic: differencing and its two decisions (KPSS, strength of
seasonality), the conditional sum of squares on the two expanded lag polynomials, the information criteria, the forecast of the
original series through the one multiplied-out operator phi(B) Phi(B^m) (1 - B)^d (1 - B^m)^D, the smallest root modulus and the
exact Gaussian likelihood by the Durbin-Levinson factorisation of the autocovariance matrix.  Nothing here comes from oracle/ or is
shaped like it: no cascaded filters, no integration loop, no step-down recursion, no Kalman filter, no det_log.

A fit is a dict: p, d, q, P, D, Q, m, has_constant, phi[<= 5], theta[<= 5], Phi[<= 2], Theta[<= 2], constant -- the coefficients as
the recursion reads them (inside the box), in the convention
    (1 - phi(B)) (1 - Phi(B^m)) (w_t - constant) = (1 - theta(B)) (1 - Theta(B^m)) e_t,     w = (1 - B)^d (1 - B^m)^D y.

tests/test_arima_cpu.py measures every constant below on the oracle (no GPU); tests/test_gpu_arima_replay.py holds the device to them.
"""
import numpy as np

LD = np.longdouble
KPSS_CRITICAL, STRENGTH_CRITICAL = LD("0.463"), LD("0.64")
DECISION_EDGE = 1.0e-9            # a decision may differ only when the 80-bit statistic is within this (relative) of its critical value
ROOT_MIN = 1.001                  # admissible models have every AR and MA root outside this radius
COEF_BOX = 0.99

# Tolerances: 16 x the worst deviation between the oracle and this restatement over the families of tests/arima_cases.py, with the
# CSS estimates and with the exact-likelihood refit's (the project's convention: stats, periods), measured by
# tests/test_arima_cpu.py, which prints every figure.  "BOX": the family whose selected coefficients sit on the +-0.99 box.  It was
# expected to need looser constants and does not: at n <= 260 a root at 1.005 has forgotten a rounding error long before it grows.
CSS_REL = 6.4e-14                 # css, sigma2: relative                                   # measured 3.983e-15 (ragged)
CSS_REL_BOX = 2.9e-14             # (and the start-up rows, coefficients across the box)    # measured 1.752e-15 (start-up rows; box family 1.371e-15)
AICC_ABS = 1.1e-11                # aicc, aic, bic: absolute (n log(sigma2), n <= 260)      # measured 6.738e-13 (ragged)
AICC_ABS_BOX = 1.4e-12            #                                                          # measured 8.748e-14
FORECAST_REL = 1.6e-14            # point forecasts, relative to max |y| of the series      # measured 9.536e-16 (differencing, h = 40)
FORECAST_REL_BOX = 1.3e-14        #                                                          # measured 7.787e-16 (after the refit)
LOGLIK_ABS = 2.7e-11              # exact_loglik against the Chandrasekhar filter: absolute # measured 1.664e-12 (lengths-m7, after the refit)
LOGLIK_ABS_BOX = 7.7e-12          #                                                          # measured 4.796e-13
STRENGTH_ABS = 5.0e-14            # strength of seasonality: absolute                        # measured 3.085e-15 (differencing)
ROOT_MARGIN = 1.0e-12             # numpy.roots against the step-down verdict at 1.001: never needed -- the smallest root of a selected
                                  # model measured 1.001 + 1.367e-04 (ragged); the margin is numpy.roots' own error on degree <= 5 polynomials


def _ld(a):
    return np.asarray(a, dtype=LD)


def difference(y, d, D, m):
    """(1 - B)^d (1 - B^m)^D y: the seasonal difference first, then the ordinary ones."""
    w = _ld(y).copy()
    for _ in range(int(D)):
        w = w[m:] - w[:-m]
    for _ in range(int(d)):
        w = w[1:] - w[:-1]
    return w


def kpss_lag(n):
    return int(3.0 * np.sqrt(float(n)) / 13.0)


def kpss_statistic(x):
    """Level-stationarity statistic eta / s^2(l) (Kwiatkowski et al. 1992): partial sums of the demeaned series over n^2, long-run
    variance with Bartlett weights up to lag trunc(3 sqrt(n) / 13).  None when the long-run variance is not positive (constant series)."""
    x = _ld(x)
    n = len(x)
    e = x - x.sum() / LD(n)
    eta = (np.cumsum(e) ** 2).sum() / LD(n) ** 2
    lag = kpss_lag(n)
    s2 = (e * e).sum() / LD(n)
    for k in range(1, lag + 1):
        s2 = s2 + 2 * (1 - LD(k) / LD(lag + 1)) * (e[k:] * e[:-k]).sum() / LD(n)
    return eta / s2 if s2 > 0 else None


def seasonal_strength(y, m):
    """1 - Var(remainder) / Var(detrended) of the classical additive decomposition, clamped to [0, 1]; 0 when n < 3 m."""
    y = _ld(y)
    n = len(y)
    if m < 2 or n < 3 * m:
        return LD(0)
    half = m // 2
    if m % 2 == 0:
        wts = np.full(m + 1, LD(1) / LD(m))
        wts[0] = wts[-1] = LD(1) / LD(2 * m)
    else:
        wts = np.full(m, LD(1) / LD(m))
    idx = np.arange(half, n - half)
    trend = np.array([(wts * y[i - half:i - half + len(wts)]).sum() for i in idx], dtype=LD)
    det = y[idx] - trend
    fig = np.array([det[idx % m == j].mean() for j in range(m)], dtype=LD)
    fig = fig - fig.mean()
    rem = det - fig[idx % m]
    vd, vr = ((det - det.mean()) ** 2).sum(), ((rem - rem.mean()) ** 2).sum()
    if not vd > 0:
        return LD(0)
    return min(max(1 - vr / vd, LD(0)), LD(1))


def decide_differences(y, m):
    """(d, D, statistics): D = 1 when the strength exceeds 0.64 (and n > m + 2); then up to two ordinary differences while the KPSS
    test rejects at 0.463 (series of fewer than 4 values are never tested).  `statistics` lists ("strength" | "kpss", value, critical)
    of every decision taken, for the edge rule."""
    y = _ld(y)
    n, D, d, stats = len(y), 0, 0, []
    if m > 1:
        f = seasonal_strength(y, m)
        stats.append(("strength", f, STRENGTH_CRITICAL))
        if f > STRENGTH_CRITICAL and n > m + 2:
            D = 1
    w = difference(y, 0, D, m)
    while d < 2 and len(w) > 3:
        k = kpss_statistic(w)
        if k is None:
            break
        stats.append(("kpss", k, KPSS_CRITICAL))
        if not k > KPSS_CRITICAL:
            break
        w = w[1:] - w[:-1]
        d += 1
    return d, D, stats


def on_decision_edge(stats):
    return any(abs(v - c) <= DECISION_EDGE * c for _, v, c in stats)


def _polymul(a, b):
    out = np.zeros(len(a) + len(b) - 1, dtype=LD)
    for i, ai in enumerate(a):
        out[i:i + len(b)] += ai * b
    return out


def _factor(c, step=1):
    """1 - sum_i c_i B^(i step) as a coefficient array in powers of B."""
    out = np.zeros(len(c) * step + 1, dtype=LD)
    out[0] = 1
    for i, ci in enumerate(c):
        out[(i + 1) * step] = -LD(ci)
    return out


def polynomials(fit):
    """(ar, ma): coefficient arrays in powers of B of (1 - phi(B))(1 - Phi(B^m)) and (1 - theta(B))(1 - Theta(B^m)), ar[0] = ma[0] = 1."""
    m = max(int(fit["m"]), 1)
    ar = _polymul(_factor(fit["phi"][:fit["p"]]), _factor(fit["Phi"][:fit["P"]], m))
    ma = _polymul(_factor(fit["theta"][:fit["q"]]), _factor(fit["Theta"][:fit["Q"]], m))
    return ar, ma


def css(fit, w, detail=False):
    """Conditional sum of squares of ar(B) (w - constant) = ma(B) e: e_t = 0 for t < La = p + m P, history before the series 0.
    Returns (css, n - La); with `detail` also the residuals and the sum of squares the same recursion has with every term taken by
    its absolute value -- what rounding errors scale with (degenerate())."""
    ar, ma = polynomials(fit)
    La = len(ar) - 1
    x = _ld(w) - LD(fit["constant"] if fit["has_constant"] else 0.0)
    n = len(x)
    e = np.zeros(n, dtype=LD)
    gross = LD(0)
    for t in range(La, n):
        k = min(t, len(ma) - 1)
        e[t] = (ar * x[t - La:t + 1][::-1]).sum() - (ma[1:k + 1] * e[t - k:t][::-1]).sum()
        gross = gross + ((np.abs(ar) * np.abs(x[t - La:t + 1][::-1])).sum() + (np.abs(ma[1:k + 1]) * np.abs(e[t - k:t][::-1])).sum()) ** 2
    out = ((e * e).sum(), n - La)
    return out + (e, gross) if detail else out


DEGENERATE = 1.0e-24              # css below this fraction of the gross sum of squares: residuals of 1e-12 of their terms


def degenerate(css_value, gross):
    """A fit that reproduces its series (n - La residuals from as many free values: an 8-point series under a seasonal AR term of m = 7):
    the residuals are what rounding left, css is noise squared and log(css) means nothing.  Such fits are compared on the absolute
    scale of `gross` and left out of the criteria; the forecasts are compared like any others."""
    return not css_value > DEGENERATE * gross


def n_parameters(fit):
    return fit["p"] + fit["q"] + fit["P"] + fit["Q"] + (1 if fit["has_constant"] else 0) + 1


def criteria(css_value, nu, n, k):
    """sigma2 = css / nu; aicc = n log(sigma2) + 2 k + 2 k (k + 1) / (n - k - 1); aic and bic as the inspection derives them from it:
    aic = aicc - 2 k (k + 1) / (n - k - 1), bic = aic - 2 k + k log(n)."""
    n, k = LD(n), LD(k)
    sigma2 = LD(css_value) / LD(nu)
    with np.errstate(divide="ignore"):
        aic = n * np.log(sigma2) + 2 * k
    return {"sigma2": sigma2, "aicc": aic + 2 * k * (k + 1) / (n - k - 1), "aic": aic, "bic": aic - 2 * k + k * np.log(n)}


def forecast(fit, y, h):
    """h forecasts of y itself from the multiplied-out operator: full(B) y_t = c + ma(B) e_t with full = ar(B) (1 - B)^d (1 - B^m)^D and
    c = constant ar(1) (the constant is the mean of the differenced series); future innovations 0, past ones from css()."""
    y = _ld(y)
    m, d, D = max(int(fit["m"]), 1), int(fit["d"]), int(fit["D"])
    ar, ma = polynomials(fit)
    full = ar
    for _ in range(d):
        full = _polymul(full, _ld([1, -1]))
    for _ in range(D):
        full = _polymul(full, _factor([1], m))
    _, _, e, _ = css(fit, difference(y, d, D, m), detail=True)
    shift = d + D * m                       # e[t] belongs to y[t + shift]
    c = LD(fit["constant"] if fit["has_constant"] else 0.0) * ar.sum()
    n = len(y)
    z = np.concatenate([y, np.zeros(h, dtype=LD)])
    for j in range(h):
        t = n + j
        acc = c
        for k in range(1, len(full)):
            acc = acc - full[k] * z[t - k]
        for k in range(j + 1, len(ma)):
            if 0 <= t - k - shift:
                acc = acc + ma[k] * e[t - k - shift]
        z[t] = acc
    return z[n:]


def roots_min_modulus(fit):
    """Smallest modulus over the roots of the four factor polynomials (numpy.roots); a seasonal factor is a polynomial in z = B^m and
    its roots are judged in B: |z|^(1/m).  inf for a model without coefficients."""
    m = max(int(fit["m"]), 1)
    best = np.inf
    for c, step in ((fit["phi"][:fit["p"]], 1), (fit["theta"][:fit["q"]], 1), (fit["Phi"][:fit["P"]], m), (fit["Theta"][:fit["Q"]], m)):
        c = np.asarray(c, dtype=np.float64)
        if len(c) == 0 or not np.any(c != 0.0):
            continue
        r = np.roots(np.concatenate([-c[::-1], [1.0]]))
        if len(r):
            best = min(best, float(np.min(np.abs(r))) ** (1.0 / step))
    return best


def _solve(A, b):
    """Gaussian elimination with partial pivoting in 80-bit arithmetic (numpy.linalg has no long double)."""
    A, b = A.copy(), b.copy()
    n = len(b)
    for i in range(n):
        piv = i + int(np.argmax(np.abs(A[i:, i])))
        if piv != i:
            A[[i, piv]] = A[[piv, i]]
            b[[i, piv]] = b[[piv, i]]
        f = A[i + 1:, i] / A[i, i]
        A[i + 1:] -= f[:, None] * A[i][None, :]
        b[i + 1:] -= f * b[i]
    x = np.zeros(n, dtype=LD)
    for i in range(n - 1, -1, -1):
        x[i] = (b[i] - (A[i, i + 1:] * x[i + 1:]).sum()) / A[i, i]
    return x


def autocovariances(fit, n):
    """gamma_0 .. gamma_(n-1) of the stationary ARMA process ar(B) x = ma(B) e with unit innovation variance: the linear system
    gamma_k - sum_i a_i gamma_|k-i| = sum_(j>=k) c_j psi_(j-k), k = 0 .. La, then the AR recursion."""
    ar, ma = polynomials(fit)
    a, c = -ar[1:], ma                      # x_t = sum a_i x_(t-i) + sum c_j e_(t-j), c_0 = 1
    p, q = len(a), len(c) - 1
    psi = np.zeros(q + 1, dtype=LD)
    for j in range(q + 1):
        psi[j] = c[j] + sum(a[i - 1] * psi[j - i] for i in range(1, min(j, p) + 1))
    rhs = lambda k: (c[k:] * psi[:q + 1 - k]).sum() if k <= q else LD(0)
    A = np.zeros((p + 1, p + 1), dtype=LD)
    b = np.zeros(p + 1, dtype=LD)
    for k in range(p + 1):
        A[k, k] += 1
        for i in range(1, p + 1):
            A[k, abs(k - i)] -= a[i - 1]
        b[k] = rhs(k)
    g = np.zeros(max(n, p + 1), dtype=LD)
    g[:p + 1] = _solve(A, b)
    for k in range(p + 1, n):
        g[k] = (a * g[k - p:k][::-1]).sum() + rhs(k)
    return g[:n]


def exact_loglik(fit, w):
    """Concentrated Gaussian objective 0.5 (log(x' S^-1 x / n) + log det S / n) of x = w - constant, S the n x n autocovariance
    matrix at unit innovation variance, factorised by the Durbin-Levinson recursion (the Cholesky factor of a Toeplitz matrix)."""
    x = _ld(w) - LD(fit["constant"] if fit["has_constant"] else 0.0)
    n = len(x)
    g = autocovariances(fit, n)
    v = g[0]
    phi = np.zeros(0, dtype=LD)
    ssq, sumlog = x[0] * x[0] / v, np.log(v)
    for t in range(1, n):
        k = (g[t] - (phi * g[1:t][::-1]).sum()) / v
        phi = np.concatenate([phi - k * phi[::-1], [k]])
        v = v * (1 - k * k)
        if not v > 0:
            return LD(np.inf)
        err = x[t] - (phi * x[:t][::-1]).sum()
        ssq = ssq + err * err / v
        sumlog = sumlog + np.log(v)
    return (np.log(ssq / LD(n)) + sumlog / LD(n)) / 2


def shape_class(p, q, P, Q):
    """The six pass variants of the device's CSS kernel (the coverage the cases claim is stated in these)."""
    if P == 0 and Q == 0:
        return 0 if (p <= 1 and q <= 1) else (1 if (p <= 2 and q <= 3) else 5)
    if p <= 1 and q <= 1 and P <= 1 and Q <= 1:
        return 2
    if p <= 1 and q <= 2 and P <= 1 and Q <= 2:
        return 3
    return 4 if (p <= 2 and q <= 3) else 5


def ring_class(m):
    """Where the device keeps the seasonal ring: none, registers (m = 7), LDS (m <= 24), HBM."""
    return "none" if m <= 1 else ("registers" if m == 7 else ("lds" if m <= 24 else "hbm"))


def model_name(fit):
    if fit["m"] > 1 and (fit["P"] or fit["D"] or fit["Q"]):
        return "AutoARIMA(%d,%d,%d)(%d,%d,%d)[%d]" % (fit["p"], fit["d"], fit["q"], fit["P"], fit["D"], fit["Q"], fit["m"])
    return "AutoARIMA(%d,%d,%d)" % (fit["p"], fit["d"], fit["q"])


def model_code(fit):
    return 1000000 + fit["p"] * 100000 + fit["d"] * 10000 + fit["q"] * 1000 + fit["P"] * 100 + fit["D"] * 10 + fit["Q"]
