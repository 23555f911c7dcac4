"""Pure-Python restatement of the reference's twelve accuracy metrics (crates/anofox-fcst-core/src/metrics.rs) and of the row
filter of its table functions (src/table_functions/ts_metrics_native.cpp).  Python floats are IEEE doubles and every expression
below is written in the source's order of operations, so the results are the source's bits: sums run sequentially from 0.0 in
row order (`iter().sum()`), `powi(2)` is `d * d`.  Two things are outside the contract: the sign of a zero
result (Rust's Sum started from 0.0 in older compilers, from -0.0 in newer ones) and NaN payloads."""
import math

EPS = 2.220446049250313e-16          # f64::EPSILON
NAN = float("nan")
FIGURES = ("mae", "mse", "rmse", "mape", "smape", "r2", "bias", "rmae", "mase", "quantile_loss", "mqloss", "coverage")
EMPTY_TEXT = "Insufficient data: need at least 1 observations, got 0"
QUANTILE_TEXT = "Invalid input: Quantile must be between 0 and 1"


class MetricError(Exception):
    """ForecastError as the FFI wrappers report it: COMPUTATION_ERROR with the Display text (error.rs:9-45, lib.rs:338-341)."""


def validate_inputs(actual, forecast):                              # metrics.rs:364-375
    if len(actual) != len(forecast):
        raise MetricError(f"Invalid input: Actual and forecast arrays must have the same length: {len(actual)} vs {len(forecast)}")
    if len(actual) == 0:
        raise MetricError(EMPTY_TEXT)


def _sum(terms):
    s = 0.0
    for v in terms:
        s = s + v
    return s


def mae(actual, forecast):                                         # metrics.rs:46-54
    validate_inputs(actual, forecast)
    return _sum(abs(a - f) for a, f in zip(actual, forecast)) / float(len(actual))


def mse(actual, forecast):                                         # metrics.rs:70-78
    validate_inputs(actual, forecast)
    return _sum((a - f) * (a - f) for a, f in zip(actual, forecast)) / float(len(actual))


def rmse(actual, forecast):                                        # metrics.rs:94-96
    v = mse(actual, forecast)
    return math.sqrt(v) if v >= 0.0 else NAN                       # (f64::sqrt of a negative or NaN value is NaN; -0.0 stays)


def mape(actual, forecast):                                        # metrics.rs:113-126
    validate_inputs(actual, forecast)
    s, count = 0.0, 0
    for a, f in zip(actual, forecast):
        if abs(a) > EPS:
            s = s + abs(_div(a - f, a))
            count += 1
    if count == 0:
        return NAN
    return s / float(count) * 100.0


def smape(actual, forecast):                                       # metrics.rs:142-159
    validate_inputs(actual, forecast)
    s, count = 0.0, 0
    for a, f in zip(actual, forecast):
        if abs(a) + abs(f) > EPS:
            s = s + _div(2.0 * abs(a - f), abs(a) + abs(f))
            count += 1
    if count == 0:
        return NAN
    return s / float(count) * 100.0


def _div(x, y):
    """IEEE division (Python raises on a zero divisor)."""
    if y == 0.0:
        if x != x or x == 0.0:
            return NAN
        return math.copysign(math.inf, x) * math.copysign(1.0, y)
    return x / y


def _ratio(actual, first, second, what):                           # metrics.rs:165-187, 235-257
    validate_inputs(actual, first)
    if len(actual) != len(second):
        raise MetricError(f"Invalid input: Actual and {what} arrays must have the same length: {len(actual)} vs {len(second)}")
    num = mae(actual, first)
    den = mae(actual, second)
    if abs(den) < EPS:
        return NAN
    return _div(num, den)


def mase(actual, forecast, baseline):
    return _ratio(actual, forecast, baseline, "baseline")


def rmae(actual, pred1, pred2):
    return _ratio(actual, pred1, pred2, "pred2")


def r2(actual, forecast):                                          # metrics.rs:190-208
    validate_inputs(actual, forecast)
    mean = _sum(actual) / float(len(actual))
    ss_res = _sum((a - f) * (a - f) for a, f in zip(actual, forecast))
    ss_tot = _sum((a - mean) * (a - mean) for a in actual)
    if abs(ss_tot) < EPS:
        return NAN
    return 1.0 - _div(ss_res, ss_tot)


def bias(actual, forecast):                                        # metrics.rs:225-229
    validate_inputs(actual, forecast)
    return _sum(f - a for a, f in zip(actual, forecast)) / float(len(actual))


def quantile_loss(actual, forecast, quantile):                     # metrics.rs:275-298
    validate_inputs(actual, forecast)
    if not (0.0 <= quantile <= 1.0):
        raise MetricError(QUANTILE_TEXT)
    s = 0.0
    for a, f in zip(actual, forecast):
        e = a - f
        s = s + (quantile * e if e >= 0.0 else (quantile - 1.0) * e)
    return s / float(len(actual))


def mqloss(actual, forecasts, quantiles):                          # metrics.rs:312-325
    if len(forecasts) != len(quantiles):
        raise MetricError("Invalid input: Number of forecasts must match number of quantiles")
    total = 0.0
    for f, q in zip(forecasts, quantiles):
        total += quantile_loss(actual, f, q)
    return _div(total, float(len(quantiles)))


def coverage(actual, lower, upper):                                # metrics.rs:343-362
    if len(actual) != len(lower) or len(actual) != len(upper):
        raise MetricError("Invalid input: All arrays must have the same length")
    if len(actual) == 0:
        return NAN
    covered = sum(1 for a, l, u in zip(actual, lower, upper) if a >= l and a <= u)
    return float(covered) / float(len(actual))


def filter_rows(*columns):
    """The row filter of the table functions (ts_metrics_native.cpp:454, 777, 1072, 1367, 1654): rows in which any of the
    statement's columns is NaN are dropped, the order of the others is kept."""
    keep = [i for i in range(len(columns[0])) if not any(c[i] != c[i] for c in columns)]
    return [[c[i] for i in keep] for c in columns]


def figure(name, actual, forecast=None, second=None, lower=None, upper=None, quantiles=None, levels=None, quantile=0.5):
    """One figure by name from the blocks the batch entries take (`second` is the baseline / pred2)."""
    if name in ("mae", "mse", "rmse", "mape", "smape", "r2", "bias"):
        return globals()[name](actual, forecast)
    if name == "mase":
        return mase(actual, forecast, second)
    if name == "rmae":
        return rmae(actual, forecast, second)
    if name == "quantile_loss":
        return quantile_loss(actual, forecast, quantile)
    if name == "mqloss":
        return mqloss(actual, quantiles, levels)
    if name == "coverage":
        return coverage(actual, lower, upper)
    raise KeyError(name)


def group_figures(names, actual, forecast=None, second=None, lower=None, upper=None, quantiles=None, levels=None, quantile=0.5,
                  drop_nan=False):
    """What anofox_hip_metrics_batch returns for one group: ({figure: value}, error text or None).  With drop_nan the rows are
    filtered on every supplied block first.  A figure that fails is NaN; the error is that of the first failing figure in the
    order of FIGURES (coverage of nothing is NaN and no error)."""
    cols = [actual] + [c for c in (forecast, second, lower, upper) if c is not None] + list(quantiles or [])
    cols = [[float(v) for v in c] for c in cols]
    if drop_nan:
        cols = filter_rows(*cols)
    it = iter(cols)
    a = next(it)
    f = next(it) if forecast is not None else None
    s = next(it) if second is not None else None
    lo = next(it) if lower is not None else None
    up = next(it) if upper is not None else None
    qs = [next(it) for _ in (quantiles or [])]
    out, err = {}, None
    for name in FIGURES:
        if name not in names:
            continue
        try:
            out[name] = figure(name, a, f, s, lo, up, qs, None if levels is None else [float(v) for v in levels], quantile)
        except MetricError as e:
            out[name] = NAN
            err = err or str(e)
    return out, err
