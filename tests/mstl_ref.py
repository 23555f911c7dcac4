"""numpy checker of csrc/fit_mstl.hip: the reference's MSTL decomposition (decomposition.rs stl_decompose / mstl_decompose) and
SeasonalWindowAverage (forecast.rs:1234-1248), restated literally.  Every sum is a sequential left fold in the reference's order
(Rust's iter().sum() on f64), so the kernels, which perform the same IEEE operations, agree with it bit for bit."""
import math

import numpy as np

FAIL, TREND, NONE = 0, 1, 2          # InsufficientDataMode::from_int


def _seqsum(v):
    s = 0.0
    for x in v:
        s += float(x)
    return s


def _extend(trend):
    n = len(trend)
    valid = [i for i in range(n) if not math.isnan(trend[i])]
    fv = valid[0] if valid else 0
    lv = valid[-1] if valid else n - 1
    for i in range(fv):
        trend[i] = trend[fv]
    for i in range(lv + 1, n):
        trend[i] = trend[lv]
    return trend


def stl_decompose(values, period):
    """(trend, seasonal, remainder) of one period, or None where the reference returns its InsufficientData error."""
    n = len(values)
    if n < 2 * period:
        return None
    window = period + 1 if period % 2 == 0 else period
    hw = window // 2
    trend = [math.nan] * n
    for i in range(hw, n - hw):
        trend[i] = _seqsum(values[i - hw:i + hw + 1]) / float(window)
    trend = _extend(trend)
    detrended = [v - t for v, t in zip(values, trend)]
    seasonal = [0.0] * n
    num_cycles = n // period
    for s in range(period):
        acc, count = 0.0, 0
        for c in range(num_cycles + 1):
            idx = c * period + s
            if idx < n:
                acc += detrended[idx]
                count += 1
        avg = acc / float(count) if count > 0 else 0.0
        for c in range(num_cycles + 1):
            idx = c * period + s
            if idx < n:
                seasonal[idx] = avg
    mean = _seqsum(seasonal) / float(n)
    seasonal = [s - mean for s in seasonal]
    remainder = [v - t - s for v, t, s in zip(values, trend, seasonal)]
    return trend, seasonal, remainder


def mstl_decompose(values, periods, mode=FAIL):
    """dict(trend, seasonal, periods, remainder, applied) or dict(error=(needed, got)) -- mstl_decompose, op for op."""
    values = [float(v) for v in values]
    n = len(values)
    if n == 0:
        if mode == FAIL:
            return {"error": (1, 0)}
        return {"trend": None, "seasonal": [], "periods": [], "remainder": None, "applied": False}
    pos = [p for p in periods if p > 0]
    min_period = min(pos) if pos else 0
    insufficient = len(periods) > 0 and min_period > 0 and n < 2 * min_period
    if insufficient:
        if mode == FAIL:
            return {"error": (2 * min_period, n)}
        if mode == NONE:
            return {"trend": None, "seasonal": [], "periods": [], "remainder": None, "applied": False}
    if len(periods) == 0 or insufficient:
        window = min(max(n // 5, 3), n)
        hw = window // 2
        trend = [math.nan] * n
        for i in range(hw, n - hw):
            trend[i] = _seqsum(values[i - hw:i + hw + 1]) / float(window)
        trend = _extend(trend)
        return {"trend": np.array(trend), "seasonal": [], "periods": [], "applied": True,
                "remainder": np.array([v - t for v, t in zip(values, trend)])}
    current = list(values)
    comps, used = [], []
    for p in sorted(periods, reverse=True):
        if p < 2 or n < 2 * p:
            continue
        r = stl_decompose(current, p)
        if r is None:
            continue
        seasonal = r[1]
        comps.append(np.array(seasonal))
        used.append(int(p))
        current = [c - s for c, s in zip(current, seasonal)]
    window = min(max(n // 5, 3), n)
    hw = window // 2
    trend = [math.nan] * n
    for i in range(hw, max(n - hw, hw)):
        end = min(i + hw + 1, n)
        start = max(i - hw, 0)
        trend[i] = _seqsum(current[start:end]) / float(end - start)
    trend = _extend(trend)
    remainder = [c - t for c, t in zip(current, trend)]
    return {"trend": np.array(trend), "seasonal": comps, "periods": used, "remainder": np.array(remainder), "applied": True}


def swa_forecast(values, period, h):
    """SeasonalWindowAverage: p = period.max(2).min(n), the last n / p (>= 1) complete seasons, summed per phase oldest first."""
    y = [float(v) for v in values]
    n = len(y)
    p = min(max(period, 2), n)
    ns = max(n // p, 1)
    start = n - ns * p
    out = []
    for i in range(h):
        if i >= p:
            out.append(out[i - p])
            continue
        acc = 0.0
        for c in range(ns):
            acc += y[start + c * p + i]
        out.append(acc / float(ns))
    return np.array(out)


def swa_fitted(values, period):
    """forecast.rs:2608-2627: the running mean of the earlier values at the same phase (the value itself where there is none)."""
    y = [float(v) for v in values]
    n = len(y)
    p = min(max(period, 1), n)
    acc, cnt, f = [0.0] * p, [0] * p, []
    for i, v in enumerate(y):
        pos = i % p
        f.append(acc[pos] / float(cnt[pos]) if cnt[pos] > 0 else v)
        acc[pos] += v
        cnt[pos] += 1
    return np.array(f)


# ---------------------------------------------------------------------------------------------------------------------------
# Candidate (e): STL with LOESS smoothers in the published form (Cleveland et al. 1990, the Fortran `stl` of netlib: inner loop only,
# no robustness iterations), the trend window from statsmodels' rule and the low-pass window p (+ 1 when even).  Used only for the
# pin search below; nothing in the product computes it.
# ---------------------------------------------------------------------------------------------------------------------------
def _loess_at(y, n, window, degree, xs, nleft, nright):
    """Tricube-weighted local fit at position xs (1-based) over y[nleft..nright] (stl.f `est`); None when every weight is 0."""
    h = max(xs - nleft, nright - xs)
    if window > n:
        h += (window - n) // 2
    w = {}
    total = 0.0
    for j in range(nleft, nright + 1):
        r = abs(j - xs)
        if r <= 0.999 * h:
            w[j] = 1.0 if r <= 0.001 * h else (1.0 - (r / h) ** 3) ** 3
            total += w[j]
    if total <= 0.0:
        return None
    for j in w:
        w[j] /= total
    if h > 0 and degree > 0:
        a = sum(w[j] * j for j in w)
        c = sum(w[j] * (j - a) ** 2 for j in w)
        if math.sqrt(c) > 0.001 * (n - 1):
            b = (xs - a) / c
            for j in w:
                w[j] = w[j] * (b * (j - a) + 1.0)
    return sum(w[j] * y[j - 1] for j in w)


def _loess(y, window, degree):
    n = len(y)
    out = np.array(y, dtype=np.float64)
    if n < 2:
        return out
    nleft, nright, half = 1, min(window, n), (window + 1) // 2
    for i in range(1, n + 1):
        if window < n and i > half and nright != n:
            nleft += 1
            nright += 1
        v = _loess_at(y, n, window, degree, i, nleft, nright)
        if v is not None:
            out[i - 1] = v
    return out


def stl_loess(y, period, s_window, s_degree=1, inner=2):
    """(trend, seasonal) of the inner loop of STL: cycle-subseries LOESS (extended by one value at each end), the low-pass filter
    (moving averages p, p, 3, then LOESS), trend LOESS of the deseasonalised series."""
    y = np.asarray(y, dtype=np.float64)
    n, p = len(y), period
    nt = int(math.ceil(1.5 * p / (1.0 - 1.5 / s_window)))
    nt += nt % 2 == 0
    nl = p + 1 if p % 2 == 0 else p
    trend = np.zeros(n)
    for _ in range(inner):
        cyc = np.zeros(n + 2 * p)
        for j in range(p):
            sub = list(y[j::p] - trend[j::p])
            k = len(sub)
            v0 = _loess_at(sub, k, s_window, s_degree, 0, 1, min(s_window, k))
            v1 = _loess_at(sub, k, s_window, s_degree, k + 1, max(1, k - s_window + 1), k)
            full = [sub[0] if v0 is None else v0] + list(_loess(sub, s_window, s_degree)) + [sub[-1] if v1 is None else v1]
            for m, v in enumerate(full):
                cyc[m * p + j] = v
        low = cyc
        for length in (p, p, 3):
            low = np.array([low[i:i + length].mean() for i in range(len(low) - length + 1)])
        low = _loess(low, nl, 1)
        seasonal = cyc[p:p + n] - low
        trend = _loess(y - seasonal, nt, 1)
    return trend, seasonal


# ---------------------------------------------------------------------------------------------------------------------------
# MSTL point forecast: candidate trend extrapolations tried against the reference's only pin.  None of them
# meets it, so MSTL / AutoMSTL keep their error; the search is kept so that the outcome can be re-checked.
# ---------------------------------------------------------------------------------------------------------------------------
def _extrapolations(tr, des, seas, h, tag):
    n = len(des)
    x = np.arange(n, dtype=np.float64)
    steps = np.arange(1, h + 1, dtype=np.float64)

    def ols(v):
        b, a = np.polyfit(x, v, 1)
        return a + b * (n - 1 + steps)

    level = des[0]
    for t in range(1, n):
        level = 0.3 * des[t] + 0.7 * level
    return {
        f"{tag}: final trend held flat": tr[-1] + seas,
        f"{tag}: OLS line through the final trend": ols(tr) + seas,
        f"{tag}: OLS line through the deseasonalised series": ols(des) + seas,
        f"{tag}: drift of the final trend": tr[-1] + (tr[-1] - tr[0]) / (n - 1) * steps + seas,
        f"{tag}: drift of the deseasonalised series": des[-1] + (des[-1] - des[0]) / (n - 1) * steps + seas,
        f"{tag}: last slope of the final trend": tr[-1] + (tr[-1] - tr[-2]) * steps + seas,
        f"{tag}: SES(0.3) of the deseasonalised series": np.full(h, level) + seas,
    }


def mstl_candidates(y, periods, h):
    """{name: h forecasts} of the closed-form candidates (a)-(c) and (d) SES(0.3) on the reference's moving-average decomposition,
    and the same extrapolations on LOESS STL decompositions (e); plus {tag: (deseasonalised series, seasonal forecasts)} for the
    model-based trend forecasters the caller runs (the project's SESOptimized, Holt, AutoETS, ... in the oracle)."""
    y = np.asarray(y, dtype=np.float64)
    n = len(y)
    d = mstl_decompose(y, periods)
    seas = np.zeros(h)
    for comp, p in zip(d["seasonal"], d["periods"]):
        seas = seas + np.array([comp[(n + i) % p] for i in range(h)])
    des = y - sum(d["seasonal"]) if d["seasonal"] else y.copy()
    out = _extrapolations(d["trend"], des, seas, h, "moving average")
    bases = {"moving average": (des, seas)}
    p = max(periods)
    # (e): statsforecast's MSTL defaults (s_window 7 + 4 = 11 for the first period, statsmodels' degree 1; R's stl degree 0) and
    # the shortest window, 7
    for s_window in (7, 11):
        for s_degree in (0, 1):
            tr, sl = stl_loess(y, p, s_window, s_degree)
            sf = np.array([sl[n - p + (i % p)] for i in range(h)])         # seasonal naive of the component
            tag = f"LOESS STL s_window {s_window} degree {s_degree}"
            out.update(_extrapolations(tr, y - sl, sf, h, tag))
            bases[tag] = (y - sl, sf)
    return out, bases
