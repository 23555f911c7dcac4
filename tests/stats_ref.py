"""A numpy / Python restatement of the reference's per-series statistics (crates/anofox-fcst-core/src/stats.rs:
compute_ts_stats, compute_ts_stats_with_dates_and_type and their helpers) and of the FFI wrapper's `length == 0` default
(crates/anofox-fcst-ffi/src/types.rs).  Written anew from the source's formulas; it is the checker of tests/test_stats_cpu.py
and tests/test_gpu_stats.py.

Every sum of the source is a left-to-right accumulation.  `order="seq"` keeps that (np.add.accumulate is strictly
sequential); `order="fsum"` takes every sum with math.fsum (the correctly rounded sum) and `order="tree"` with the fixed
binary tree of `tree_sum` below.  The distance between the three is the data's own rounding noise, from which the tolerance of
the GPU comparison is derived.

`powi(k)` is repeated multiplication, `round` is half away from zero, a float -> usize cast saturates (NaN and negatives
give 0), integer division truncates, `i64 as usize` wraps.
"""
from __future__ import annotations

import math

import numpy as np

EPS = float(np.finfo(np.float64).eps)          # f64::EPSILON
NAN = float("nan")

INT_FIELDS = ("length", "n_nulls", "n_nan", "n_zeros", "n_positive", "n_negative", "n_unique_values", "is_constant",
              "n_zeros_start", "n_zeros_end", "plateau_size", "plateau_size_nonzero")
FP_FIELDS = ("mean", "median", "std_dev", "variance", "min", "max", "range", "sum", "skewness", "kurtosis", "tail_index",
             "bimodality_coef", "trimmed_mean", "coef_variation", "q1", "q3", "iqr", "autocorr_lag1", "trend_strength",
             "seasonality_strength", "entropy", "stability")
DATE_FIELDS = ("expected_length", "n_gaps")
FIELDS = INT_FIELDS + FP_FIELDS + DATE_FIELDS
EXACT_FP = ("min", "max", "range", "median", "q1", "q3", "iqr")
TOL_FP = tuple(f for f in FP_FIELDS if f not in EXACT_FP)
FREQUENCY_TYPES = {"FIXED": 0, "MONTHLY": 1, "QUARTERLY": 2, "YEARLY": 3}
ORDERS = ("seq", "fsum", "tree")


# ----------------------------------------------------------------------------------------------------------------------
# the three evaluation orders of a sum
# ----------------------------------------------------------------------------------------------------------------------
def tree_sum(x) -> float:
    """Fixed binary tree: neighbours are added pairwise, an odd last element is carried to the next level."""
    x = np.asarray(x, dtype=np.float64)
    if x.size == 0:
        return 0.0
    while x.size > 1:
        h = x.size // 2
        y = x[0:2 * h:2] + x[1:2 * h:2]
        x = np.concatenate([y, x[2 * h:]]) if x.size & 1 else y
    return float(x[0])


def _tree_rows(X):
    while X.shape[1] > 1:
        h = X.shape[1] // 2
        Y = X[:, 0:2 * h:2] + X[:, 1:2 * h:2]
        X = np.concatenate([Y, X[:, 2 * h:]], axis=1) if X.shape[1] & 1 else Y
    return X[:, 0]


def total(x, order="seq") -> float:
    x = np.asarray(x, dtype=np.float64)
    if x.size == 0:
        return 0.0
    with np.errstate(all="ignore"):
        if order == "seq":
            return float(np.add.accumulate(x)[-1])
        if order == "tree":
            return tree_sum(x)
    if order == "fsum":
        if not np.all(np.isfinite(x)):
            with np.errstate(all="ignore"):
                return float(np.add.accumulate(x)[-1])       # fsum raises on inf - inf; the value is the IEEE one
        return math.fsum(x.tolist())
    raise ValueError(order)


def window_sums(v, w, order="seq"):
    """Sum of v[j : j + w] for every j, each window summed afresh from its first element (stats.rs compute_stability)."""
    k = len(v) - w + 1
    out = np.empty(k)
    if order == "fsum" and np.all(np.isfinite(v)):
        lst = v.tolist()
        for j in range(k):
            out[j] = math.fsum(lst[j:j + w])
        return out
    win = np.lib.stride_tricks.sliding_window_view(v, w)
    step = max(1, (1 << 22) // w)
    with np.errstate(all="ignore"):
        for a in range(0, k, step):
            blk = win[a:a + step]
            out[a:a + step] = _tree_rows(np.array(blk)) if order == "tree" else np.add.accumulate(blk, axis=1)[:, -1]
    return out


# ----------------------------------------------------------------------------------------------------------------------
# helpers of stats.rs
# ----------------------------------------------------------------------------------------------------------------------
def _as_usize(x: float) -> int:
    """Rust's saturating `f64 as usize`."""
    if x != x or x <= 0.0:
        return 0
    if x >= 18446744073709551615.0:
        return (1 << 64) - 1
    return int(x)


def _rust_round(x: float) -> float:
    if x != x or math.isinf(x):
        return x
    return math.copysign(math.floor(abs(x) + 0.5), x) if abs(x) < 4503599627370496.0 else x


def percentile(s, p):
    n = len(s)
    if n == 0:
        return NAN
    if n == 1:
        return float(s[0])
    idx = p * (float(n) - 1.0)
    lo, hi = int(math.floor(idx)), int(math.ceil(idx))
    frac = idx - float(lo)
    if hi >= n:
        return float(s[n - 1])
    with np.errstate(all="ignore"):
        return float(np.float64(s[lo]) * np.float64(1.0 - frac) + np.float64(s[hi]) * np.float64(frac))


def autocorrelation(v, lag, order="seq", probe=None):
    n = len(v)
    if n <= lag:
        return NAN
    with np.errstate(all="ignore"):
        mean = total(v, order) / float(n)
        d = v - mean
        den = total(d * d, order)
        num = total(d[lag:] * d[:n - lag], order)
        if probe is not None:
            probe.append(("acf_denominator", abs(den)))
        if abs(den) < EPS:
            return 0.0
        return float(np.float64(num) / np.float64(den))


def strength_metrics(v, order="seq", probe=None):
    n = len(v)
    if n < 4:
        return 0.0, 0.0
    with np.errstate(all="ignore"):
        nf = float(n)
        x_mean = (nf - 1.0) / 2.0
        y_mean = total(v, order) / nf
        dx = np.arange(n, dtype=np.float64) - x_mean
        dy = v - y_mean
        ss_xy, ss_xx, ss_yy = total(dx * dy, order), total(dx * dx, order), total(dy * dy, order)
        if probe is not None:
            probe.append(("ss_xx", abs(ss_xx)))
            probe.append(("ss_yy", abs(ss_yy)))
        if abs(ss_xx) > EPS and abs(ss_yy) > EPS:
            r = float(np.sqrt(np.float64(ss_xy * ss_xy) / np.float64(ss_xx * ss_yy)))
            if probe is not None:
                probe.append(("trend_raw", r))
            trend = r if r != r else min(max(r, 0.0), 1.0)           # f64::clamp keeps NaN
        else:
            trend = 0.0
        best = 0.0
        for lag in (2, 4, 7, 12):
            a = abs(autocorrelation(v, lag, order))
            if math.isfinite(a):
                best = max(best, a)
        if probe is not None:
            probe.append(("season_raw", best))
        return trend, min(max(best, 0.0), 1.0)


def approximate_entropy(v):
    if len(v) < 10:
        return NAN
    with np.errstate(all="ignore"):
        lo, hi = float(np.min(v)), float(np.max(v))
        rng = hi - lo
        if abs(rng) < EPS:
            return 0.0
        bins = [0] * 10
        for x in ((v - lo) / rng * 9.0).tolist():
            bins[min(_as_usize(_rust_round(x)), 9)] += 1
    n = float(len(v))
    e = 0.0
    for c in bins:
        if c > 0:
            p = float(c) / n
            e -= p * math.log(p)
    return e


def entropy_bins(v):
    """The ten bin counts of approximate_entropy (None where it returns early)."""
    if len(v) < 10:
        return None
    with np.errstate(all="ignore"):
        lo, hi = float(np.min(v)), float(np.max(v))
        rng = hi - lo
        if abs(rng) < EPS:
            return None
        bins = [0] * 10
        for x in ((v - lo) / rng * 9.0).tolist():
            bins[min(_as_usize(_rust_round(x)), 9)] += 1
    return bins


def stability(v, order="seq", probe=None):
    n = len(v)
    if n < 10:
        return NAN
    w = max(n // 5, 3)
    with np.errstate(all="ignore"):
        rm = window_sums(v, w, order) / float(w)
        k = float(len(rm))
        rm_mean = total(rm, order) / k
        d = rm - rm_mean
        var = total(d * d, order) / k
        rm_std = math.sqrt(var) if var >= 0 else NAN
        if probe is not None:
            probe.append(("rm_mean", abs(rm_mean)))
        if abs(rm_mean) > EPS:
            return float(np.float64(1.0) / (np.float64(rm_std) / np.float64(abs(rm_mean)) + np.float64(0.01)))
        return NAN


def hill_estimator(v, order="seq", probe=None):
    if len(v) < 10:
        return NAN
    a = np.abs(v)
    a = a[a > EPS]
    if len(a) < 10:
        return NAN
    a = np.sort(a)[::-1]
    k = int(math.floor(math.sqrt(float(len(a)))))
    k = min(max(k, 2), len(a) - 1)
    thr = float(a[k])
    if thr <= EPS:
        return NAN
    with np.errstate(all="ignore"):
        logs = np.array([x if x != x or math.isinf(x) else math.log(x) for x in (a[:k] / thr).tolist()])      # x >= 1, inf or NaN
        h = total(logs, order) / float(k)
    if probe is not None:
        probe.append(("hill_h", abs(h)))
    if h <= EPS:
        return NAN
    return 1.0 / h


def trimmed_mean(s, order="seq"):
    n = len(s)
    if n == 0:
        return NAN
    trim = _as_usize(math.floor(float(n) * 0.1))
    if 2 * trim >= n:
        return total(s, order) / float(n)
    cut = s[trim:n - trim]
    with np.errstate(all="ignore"):
        return total(cut, order) / float(len(cut))


def plateau_size(bits):
    if len(bits) == 0:
        return 0
    best = run = 1
    for i in range(1, len(bits)):
        if bits[i] == bits[i - 1]:
            run += 1
            best = max(best, run)
        else:
            run = 1
    return best


def plateau_size_nonzero(v, bits):
    best = run = 0
    prev = None
    for x, b in zip(v, bits):
        if x == 0.0:
            best = max(best, run)
            run = 0
            prev = None
        else:
            if prev is not None and prev == b:
                run += 1
            else:
                best = max(best, run)
                run = 1
            prev = b
    return max(best, run)


# ----------------------------------------------------------------------------------------------------------------------
# dates
# ----------------------------------------------------------------------------------------------------------------------
def _wrap64(x: int) -> int:
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


def _trunc_div(a: int, b: int) -> int:
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def year_month(micros: int):
    """(year, month) of micros_to_datetime: seconds by truncating division; a non-zero negative remainder makes the nanosecond
    argument invalid and the conversion falls back to 1970-01-01, as does a date outside chrono's range."""
    micros = int(micros)
    secs = _trunc_div(micros, 1000000)
    rem = micros - secs * 1000000
    if rem < 0:
        return 1970, 1
    z = secs // 86400 + 719468                       # days-to-civil (era arithmetic on the proleptic Gregorian calendar)
    era = z // 146097
    doe = z - era * 146097
    yoe = (doe - doe // 1460 + doe // 36524 - doe // 146096) // 365
    doy = doe - (365 * yoe + yoe // 4 - yoe // 100)
    mp = (5 * doy + 2) // 153
    m = mp + 3 if mp < 10 else mp - 9
    y = yoe + era * 400 + (1 if m <= 2 else 0)
    if y < -262143 or y > 262142:
        return 1970, 1
    return y, m


def _period_index(micros, ftype):
    y, m = year_month(micros)
    if ftype == "MONTHLY":
        return y * 12 + m
    if ftype == "QUARTERLY":
        return y * 4 + (m - 1) // 3
    return y


def date_metrics(dates, frequency_micros=0, frequency_type="FIXED"):
    """(expected_length, n_gaps) or (None, None); usize values (a negative count wraps as `as usize` does)."""
    if dates is None or len(dates) == 0:
        return None, None
    d = sorted(int(x) for x in dates)
    if len(d) < 2:
        return len(d), 0
    first, last = d[0], d[-1]
    mask = (1 << 64) - 1
    if frequency_type in ("MONTHLY", "QUARTERLY", "YEARLY"):
        idx = [_period_index(x, frequency_type) for x in d]
        return (idx[-1] - idx[0] + 1) & mask, sum(1 for a, b in zip(idx, idx[1:]) if b - a > 1)
    f = int(frequency_micros)
    if f <= 0:
        return None, None
    duration = _wrap64(last - first)
    expected = _wrap64(_trunc_div(duration, f) + 1) & mask
    x = float(f) * 1.5
    thr = (1 << 63) - 1 if x >= 9223372036854775807.0 else int(x)
    return expected, sum(1 for a, b in zip(d, d[1:]) if _wrap64(b - a) > thr)


# ----------------------------------------------------------------------------------------------------------------------
# compute_ts_stats
# ----------------------------------------------------------------------------------------------------------------------
def ffi_default():
    """TsStatsResult::default(): what the wrapper returns for length == 0."""
    r = {f: 0 for f in INT_FIELDS}
    r["is_constant"] = False
    r.update({f: NAN for f in FP_FIELDS})
    r["expected_length"] = r["n_gaps"] = None
    return r


def compute(values, valid=None, dates=None, frequency_micros=0, frequency_type="FIXED", order="seq", probe=None):
    """The wrapper plus compute_ts_stats_with_dates_and_type.  `valid[i]` false = NULL.  `dates` None = the date-less entry.
    `probe`, a list, receives (name, magnitude) of every quantity the source compares with EPSILON."""
    x = np.asarray(values, dtype=np.float64)
    n = len(x)
    if n == 0:
        return ffi_default()
    ok = np.ones(n, dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
    isnan = ok & np.isnan(x)
    keep = ok & ~isnan
    v = x[keep]
    r = {f: 0 for f in INT_FIELDS}
    r["is_constant"] = False
    r.update({f: 0.0 for f in FP_FIELDS})
    r["length"], r["n_nulls"], r["n_nan"] = n, int(n - ok.sum()), int(isnan.sum())
    r["expected_length"], r["n_gaps"] = date_metrics(dates, frequency_micros, frequency_type)
    m = len(v)
    if m == 0:
        return r
    bits = v.view(np.uint64)
    r["n_zeros"], r["n_positive"], r["n_negative"] = int((v == 0.0).sum()), int((v > 0.0).sum()), int((v < 0.0).sum())
    r["n_unique_values"] = len(set(bits.tolist()))
    r["is_constant"] = r["n_unique_values"] == 1
    zero = keep & (x == 0.0)
    brk = np.nonzero(~zero)[0]
    r["n_zeros_start"] = int(brk[0]) if len(brk) else n
    r["n_zeros_end"] = int(n - 1 - brk[-1]) if len(brk) else n
    r["plateau_size"] = plateau_size(bits.tolist())
    r["plateau_size_nonzero"] = plateau_size_nonzero(v.tolist(), bits.tolist())
    with np.errstate(all="ignore"):
        nf = float(m)
        s = total(v, order)
        mean = s / nf
        lo, hi = float(np.min(v)), float(np.max(v))
        d = v - mean
        d2 = d * d
        variance = total(d2, order) / float(m - 1) if m > 1 else 0.0
        std = math.sqrt(variance) if variance >= 0 else NAN
        if variance == math.inf:
            std = math.inf
        if probe is not None:
            probe.append(("std_dev", abs(std)))
            probe.append(("mean", abs(mean)))
        r.update(sum=s, mean=mean, min=lo, max=hi, range=hi - lo, variance=variance, std_dev=std)
        r["coef_variation"] = float(np.float64(std) / np.float64(abs(mean))) if abs(mean) > EPS else NAN
        srt = np.sort(v, kind="stable")
        r["median"], r["q1"], r["q3"] = percentile(srt, 0.5), percentile(srt, 0.25), percentile(srt, 0.75)
        r["iqr"] = r["q3"] - r["q1"]
        if m > 2 and std > EPS:
            m3 = total(d2 * d, order) / nf
            g1 = np.float64(m3) / np.float64(std * std * std)
            r["skewness"] = float(g1 * np.sqrt(np.float64(nf * (nf - 1.0))) / np.float64(nf - 2.0))
        else:
            r["skewness"] = NAN
        if m > 3 and std > EPS:
            m4 = total(d2 * d2, order) / nf
            s2 = std * std
            g2 = np.float64(m4) / np.float64(s2 * s2) - 3.0
            r["kurtosis"] = float((nf - 1.0) / ((nf - 2.0) * (nf - 3.0)) * ((nf + 1.0) * g2 + 6.0))
        else:
            r["kurtosis"] = NAN
        r["tail_index"] = hill_estimator(v, order, probe)
        sk, ku = r["skewness"], r["kurtosis"]
        r["bimodality_coef"] = float(np.float64(sk * sk + 1.0) / np.float64(ku + 3.0)) if m > 3 and math.isfinite(ku) and math.isfinite(sk) else NAN
        r["trimmed_mean"] = trimmed_mean(srt, order)
        r["autocorr_lag1"] = autocorrelation(v, 1, order, probe)
        r["trend_strength"], r["seasonality_strength"] = strength_metrics(v, order, probe)
        r["entropy"] = approximate_entropy(v)
        r["stability"] = stability(v, order, probe)
    return r


def deviation(a, b) -> float:
    """The project's measure |a - b| / max(1, |b|); 0 where both are NaN or equal (infinities included), inf where only one is."""
    if a is None or b is None:
        return 0.0 if a is b else math.inf
    if (a != a) or (b != b):
        return 0.0 if (a != a) and (b != b) else math.inf
    if a == b:
        return 0.0
    if math.isinf(a) or math.isinf(b):
        return math.inf
    return abs(a - b) / max(1.0, abs(b))


def same(a, b) -> bool:
    """`==`, or both NaN, or both None."""
    if a is None or b is None:
        return a is b
    return a == b or (a != a and b != b)


def noise_table(families, floor=1e-12, factor=16.0):
    """{family: {figure: tol}} of the contract: tol = max(floor, factor x the largest deviation between the source order and the
    fsum / tree orders over the family's series).  `families`: {name: [dict(values=..., valid=...)]}."""
    out = {}
    for name, cases in families.items():
        worst = {f: 0.0 for f in TOL_FP}
        for c in cases:
            base = compute(c["values"], c.get("valid"))
            for order in ("fsum", "tree"):
                alt = compute(c["values"], c.get("valid"), order=order)
                for f in TOL_FP:
                    d = deviation(alt[f], base[f])
                    if d > worst[f]:
                        worst[f] = d
        out[name] = {f: max(floor, factor * worst[f]) for f in TOL_FP}
    return out
