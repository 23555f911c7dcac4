"""A pure-Python restatement of the reference's detect_seasonality, analyze_seasonality and compute_trend_strength (seasonality.rs
323-461): plain float loops in the source's order, one accumulator per sum, from 0.0, multiply and add separate.  It is the
yardstick of tests/test_gpu_seasonality.py (equality of bits) and shares nothing with oracle/.

`analyze(values, max_period)` takes a list whose None elements are NULLs (dropped, as ts_seasonality.cpp:27-32 drops them) and returns
the figures of every entry of the library: status, detected_periods, strengths, acf (the raw values at the periods), primary_period,
seasonal_strength, trend_strength, is_seasonal.  `analyze_fast` is the same arithmetic with numpy's sequential cumsum for the lag
sums; tests/test_seasonality_cpu.py shows it equal to the loops on every short case before the GPU tests use it for long series."""
import math

import numpy as np

EPS = 2.220446049250313e-16          # f64::EPSILON
OK, SHORT = 0, 1
TOP = 5
THRESHOLD = 0.1


def compact(series):
    return [float(v) for v in series if v is not None]


def _div(a, b):
    """IEEE division (Python raises on a zero divisor)."""
    return float(np.float64(a) / np.float64(b)) if b == 0.0 else a / b


def mean_variance(v):
    s = 0.0
    for x in v:
        s += x
    mean = s / float(len(v))
    var = 0.0
    for x in v:
        d = x - mean
        var += d * d
    return mean, var


def max_lag_of(n, max_period):
    half = n // 2
    return min(max_period, half) if max_period > 0 else half


def acf_loops(v, mean, var, max_lag):
    n = len(v)
    out = []
    for lag in range(1, max_lag + 1):
        s = 0.0
        for i in range(n - lag):
            s += (v[i] - mean) * (v[i + lag] - mean)
        out.append(_div(s, var))
    return out


def acf_fast(v, mean, var, max_lag):
    """The same sums by np.cumsum, which adds in order; the leading 0.0 is the loops' starting value."""
    n = len(v)
    out = []
    with np.errstate(all="ignore"):
        c = np.asarray(v, dtype=np.float64) - np.float64(mean)
        for lag in range(1, max_lag + 1):
            s = np.cumsum(np.concatenate(([0.0], c[:n - lag] * c[lag:])))[-1]
            out.append(float(s / np.float64(var)))
    return out


def pick_periods(acf):
    """Peaks above the threshold, by ACF descending with a STABLE sort (equal values keep ascending lag), the first five."""
    peaks = [i + 1 for i in range(1, len(acf) - 1) if acf[i] > acf[i - 1] and acf[i] > acf[i + 1] and acf[i] > THRESHOLD]
    # Rust's sort_by(|a, b| acf_b.partial_cmp(acf_a)) is stable; no NaN passes the comparisons above, so the order is total
    peaks.sort(key=lambda p: -acf[p - 1])
    return peaks[:TOP]


def clamp01(x):
    """Rust's f64::clamp(0.0, 1.0): a NaN stays a NaN."""
    return 0.0 if x < 0.0 else 1.0 if x > 1.0 else x


def trend_strength(v, y_mean):
    n = float(len(v))
    x_mean = (n - 1.0) / 2.0
    ss_xy = ss_xx = ss_yy = 0.0
    for i, y in enumerate(v):
        x = float(i)
        ss_xy += (x - x_mean) * (y - y_mean)
        ss_xx += (x - x_mean) * (x - x_mean)
        ss_yy += (y - y_mean) * (y - y_mean)
    if abs(ss_xx) < EPS or abs(ss_yy) < EPS:
        return 0.0
    with np.errstate(all="ignore"):
        q = float(np.float64(ss_xy * ss_xy) / np.float64(ss_xx * ss_yy))
    return clamp01(math.sqrt(q) if q == q and q >= 0.0 else float("nan"))


def _analyze(series, max_period, acf_fn):
    v = compact(series)
    n = len(v)
    out = {"status": OK, "n": n, "detected_periods": [], "strengths": [], "acf": [], "primary_period": 0, "seasonal_strength": 0.0,
           "trend_strength": 0.0, "is_seasonal": False}
    if n < 4:
        out["status"] = SHORT
        return out
    mean, var = mean_variance(v)
    max_lag = max_lag_of(n, max_period)
    if max_lag >= 2 and not abs(var) < EPS:
        acf = acf_fn(v, mean, var, max_lag)
        periods = pick_periods(acf)
        out["detected_periods"] = periods
        out["acf"] = [acf[p - 1] for p in periods]
        # analyze_seasonality recomputes the sum with the same arithmetic; its own test of the variance is `> EPSILON`
        out["strengths"] = [clamp01(acf[p - 1]) if abs(var) > EPS else 0.0 for p in periods]
        if periods:
            out["primary_period"] = periods[0]
            out["seasonal_strength"] = out["strengths"][0]
    out["trend_strength"] = trend_strength(v, mean)
    out["is_seasonal"] = out["seasonal_strength"] > 0.1
    return out


def analyze(series, max_period=0):
    return _analyze(series, max_period, acf_loops)


def analyze_fast(series, max_period=0):
    return _analyze(series, max_period, acf_fast)


def full_acf(series, max_period=0):
    """The whole ACF of a series (loops), for the tests that classify ties."""
    v = compact(series)
    mean, var = mean_variance(v)
    return acf_loops(v, mean, var, max_lag_of(len(v), max_period))


def scalar_detect(values):
    """ts_detect_seasonality(values): None for a NULL list and for every failure."""
    if values is None:
        return None
    r = analyze(values)
    return None if r["status"] != OK else r["detected_periods"]


def scalar_analyze(values):
    if values is None:
        return None
    r = analyze(values)
    if r["status"] != OK:
        return None
    return {k: r[k] for k in ("detected_periods", "primary_period", "seasonal_strength", "trend_strength")}
