"""Plain restatement of the closed-form members of the classic family, in numpy.longdouble -- TEST INFRASTRUCTURE.

Written from the reference's text, not from the kernels or the oracle:
  forecast.rs:1026-1100  Naive, SeasonalNaive, SMA, RandomWalkDrift
  forecast.rs:1391-1431  the toy ARIMA (AR coefficient 0.5 on the differenced series, Naive below five observations)
  forecast.rs:1102-1109, 1206-1218  SES at alpha = 0.3 and SeasonalES at alpha = 0.1, period.max(2) (the smoothing itself is the
                         textbook form the crate documents: state <- alpha * y + (1 - alpha) * state, the level starting at the first
                         observation, the seasonal states at the first season, forecasts from the state of the phase that comes next)
  forecast.rs:2558-2591  the intervals: z by the ladder of confidence levels, population sd of the history, sqrt(step)
  forecast.rs:2593-2643  fitted values
  forecast.rs:516-525    fewer than three observations: InsufficientData

Every function takes one series (any sequence of floats) and returns longdouble arrays; sums run in the order the text gives.
"""
import numpy as np

LD = np.longdouble
INSUFFICIENT_DATA = 6
COMPUTATION_ERROR = 3
# the reference holds the smoothing constants as the doubles 0.3 / 0.1: the restatement takes the same numbers
FIXED_ALPHA_F64 = {"SES": LD(0.3), "SeasonalES": LD(0.1)}

MODELS = ("Naive", "SeasonalNaive", "SMA", "RandomWalkDrift", "ARIMA", "SES", "SeasonalES")


def _ld(y):
    return np.asarray(y, dtype=np.float64).astype(LD)


def naive(y, h):
    y = _ld(y)
    return np.full(h, y[-1], dtype=LD)


def seasonal_naive(y, h, period):
    y = _ld(y)
    p = min(max(int(period), 1), len(y))
    last_season = y[len(y) - p:]
    return np.array([last_season[i % p] for i in range(h)], dtype=LD)


def sma_window(window, period=1):
    """The window the binding hands to forecast_sma: the caller's, or max(period, 3) when none is given."""
    return int(window) if int(window) > 0 else max(int(period), 3)


def sma(y, h, window):
    y = _ld(y)
    w = min(int(window), len(y))
    s = LD(0)
    for v in y[::-1][:w]:
        s += v
    return np.full(h, s / LD(w), dtype=LD)


def drift(y, h):
    y = _ld(y)
    n = len(y)
    d = (y[-1] - y[0]) / LD(n - 1)
    return np.array([y[-1] + d * LD(i) for i in range(1, h + 1)], dtype=LD)


def toy_arima(y, h):
    y = _ld(y)
    if len(y) < 5:
        return naive(y, h)
    diff = y[1:] - y[:-1]
    s = LD(0)
    for v in diff:
        s += v
    mean_diff = s / LD(len(diff))
    prev, cum = diff[-1], y[-1]
    out = []
    for _ in range(h):
        nd = mean_diff + LD(0.5) * (prev - mean_diff)
        cum = cum + nd
        out.append(cum)
        prev = nd
    return np.array(out, dtype=LD)


def ses(y, h, alpha=FIXED_ALPHA_F64["SES"]):
    y = _ld(y)
    level = y[0]
    for v in y[1:]:
        level = alpha * v + (LD(1) - alpha) * level
    return np.full(h, level, dtype=LD)


def seasonal_es(y, h, period, alpha=FIXED_ALPHA_F64["SeasonalES"]):
    """None when the series is shorter than one season (the fit fails: ComputationError)."""
    y = _ld(y)
    m = max(int(period), 2)
    n = len(y)
    if n < m:
        return None
    s = [y[i] for i in range(m)]
    for t in range(m, n):
        s[t % m] = alpha * y[t] + (LD(1) - alpha) * s[t % m]
    return np.array([s[(n + i) % m] for i in range(h)], dtype=LD)


def point(model, y, h, period=1, window=0):
    """(code, forecasts): the error code the reference returns for this series (0: forecasts follow)."""
    if len(y) < 3:
        return INSUFFICIENT_DATA, None
    if model == "Naive":
        return 0, naive(y, h)
    if model == "SeasonalNaive":
        return 0, seasonal_naive(y, h, period)
    if model == "SMA":
        return 0, sma(y, h, sma_window(window, period))
    if model == "RandomWalkDrift":
        return 0, drift(y, h)
    if model == "ARIMA":
        return 0, toy_arima(y, h)
    if model == "SES":
        return 0, ses(y, h)
    if model == "SeasonalES":
        out = seasonal_es(y, h, period)
        return (COMPUTATION_ERROR, None) if out is None else (0, out)
    raise ValueError(model)


def z_value(confidence):
    """forecast.rs:2570-2576."""
    c = float(confidence)
    if c >= 0.99:
        return 2.576
    if c >= 0.95:
        return 1.96
    if c >= 0.90:
        return 1.645
    if c >= 0.80:
        return 1.28
    return 1.0


def intervals(forecasts, y, confidence):
    y = _ld(y)
    s = LD(0)
    for v in y:
        s += v
    mean = s / LD(len(y))
    q = LD(0)
    for v in y:
        q += (v - mean) * (v - mean)
    sd = np.sqrt(q / LD(len(y)))
    z = LD(z_value(confidence))
    f = np.asarray(forecasts, dtype=LD)
    w = np.array([z * sd * np.sqrt(LD(i + 1)) for i in range(len(f))], dtype=LD)
    return f - w, f + w


def fitted(model, y, period=1):
    y = _ld(y)
    n = len(y)
    if model == "Naive":
        return np.concatenate([y[:1], y[:-1]])
    if model == "SeasonalNaive":
        p = min(max(int(period), 1), n)
        return np.concatenate([np.full(p, y[0], dtype=LD), y[:n - p]])
    alpha = LD(0.3)
    out, level = [y[0]], y[0]
    for v in y[1:]:
        out.append(level)
        level = alpha * v + (LD(1) - alpha) * level
    return np.array(out, dtype=LD)


def rel(a, b):
    """max |a - b| / max(1, |b|), in long double (the scale of tests/test_gpu_parity.py _rel)."""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    if a.shape != b.shape:
        return float("inf")
    if a.size == 0:
        return 0.0
    return float(np.max(np.abs(a - b) / np.maximum(LD(1), np.abs(b))))


# --------------------------------------------------------------------------------------------
# the cases both the CPU test (oracle against this module) and the GPU test (kernels against this module) run
# --------------------------------------------------------------------------------------------
CASE_N0 = 37            # the length SMA's window and SeasonalNaive's period are set to (and one past)
CASE_HORIZONS = (1, 200)

# What the oracle achieves against this module over closed_form_cases() x CASE_HORIZONS, on the scale of rel(): measured by
# tests/test_classic_cpu.py::test_oracle_meets_the_restatement, which fails when the figure moves.  The GPU test allows the kernels
# four times this (the kernel and the oracle may differ from long double only by the fp64 rounding of the same sums).
ORACLE_VS_LONGDOUBLE = 1.5e-14           # measured 1.469e-14: the toy ARIMA's 200-step running sum on a series of 21 observations


def closed_form_cases():
    """[(model, options, series)]: options are keyword arguments of make_options (auto_detect is off throughout)."""
    rng = np.random.default_rng(20260105)
    lens = [CASE_N0] + [int(x) for x in rng.integers(3, 91, 64)]
    base = []
    for k, L in enumerate(lens):
        if k % 3 == 0:
            y = rng.poisson(3.0, L).astype(np.float64)                 # counts with zeros
        elif k % 3 == 1:
            y = rng.normal(0.0, 50.0, L)                               # signed
        else:
            y = 1000.0 + np.cumsum(rng.normal(0.5, 2.0, L))            # a trending level far from zero
        base.append(y)
    short = [rng.normal(10.0, 3.0, L) for L in (1, 2, 3, 4, 5, 6)] + [np.round(rng.normal(0.0, 9.0, L)) for L in (1, 2, 3, 4, 5, 6)]
    cases = [("Naive", {}, base + short), ("SES", {}, base + short),
             ("RandomWalkDrift", {}, short + base[:20]), ("ARIMA", {}, short + base[:20])]
    for w in (0, 1, 5, CASE_N0, CASE_N0 + 3):
        cases.append(("SMA", {"window": w}, base + short))
    for p in (1, 7, CASE_N0, CASE_N0 + 1):
        cases.append(("SeasonalNaive", {"seasonal_period": p}, base + short))
    for p in (2, 7, 12):
        cases.append(("SeasonalES", {"seasonal_period": p}, base + short))
    return cases
