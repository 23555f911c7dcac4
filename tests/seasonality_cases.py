"""The case list shared by tests/test_seasonality_cpu.py and tests/test_gpu_seasonality.py.  A series is a list of floats whose None
elements are NULLs.  Everything here is deterministic (seeded generators), so both suites see the same inputs."""
import json
import math
import os
import random
import struct

import numpy as np

import seasonality_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
LDS_ROWS = 5120                      # anofox_forecast_amd.lib.SEASONALITY_LDS_ROWS (test_seasonality_cpu.py checks the two agree)
FAST_FROM = 200                      # series of at least this many values use R.analyze_fast in the GPU suite


def load_kats():
    with open(os.path.join(HERE, "golden", "seasonality_kats.json")) as fh:
        return json.load(fh)


def golden_holds(st, detect, analyze):
    """One golden statement against an implementation of the two scalars."""
    got = (detect if st["function"] == "ts_detect_seasonality" else analyze)(st["input"])
    if st["check"] == "is_null":
        return got is None
    if got is None:
        return False
    if st["field"] is not None:
        got = got[st["field"]]
    return {"not_null": lambda: got is not None, "length_ge": lambda: len(got) >= st["value"], "ge": lambda: got >= st["value"],
            "eq": lambda: got == st["value"], "contains": lambda: st["value"] in got}[st["check"]]()


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def same_bits(a, b):
    """Equality of bit patterns; the only exemption is a NaN's payload."""
    a, b = float(a), float(b)
    return (a != a and b != b) or bits(a) == bits(b)


def split(series):
    """(values with 0.0 at the NULLs, validity list)"""
    return [0.0 if v is None else float(v) for v in series], [v is not None for v in series]


def expected(series, max_period=0):
    v = R.compact(series)
    return R.analyze_fast(v, max_period) if len(v) >= FAST_FROM else R.analyze(v, max_period)


def seasonal(n, period, seed, amp=3.0, noise=0.5, slope=0.01):
    rng = random.Random(seed)
    return [20.0 + slope * t + amp * math.sin(2.0 * math.pi * t / period) + rng.gauss(0.0, noise) for t in range(n)]


def noise(n, seed):
    rng = random.Random(seed)
    return [rng.gauss(0.0, 1.0) for _ in range(n)]


# ---- short lengths: 0, 1, 3 are too short; 4, 5 have max_lag 2 (no candidate); 6, 7 have exactly one candidate lag ----
def short_batch():
    base = [3.0, 9.0, 1.0, 8.0, 2.0, 9.5, 0.5, 7.0, 3.0, 9.0, 1.0, 8.0]
    out = [base[:k] for k in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12)]
    out += [[1.0, 5.0, 1.0, 5.0, 1.0, 5.0], [1.0, 5.0, 1.0, 5.0, 1.0, 5.0, 1.0], [1.0, 2.0, 9.0, 1.0, 2.0, 9.0, 1.0]]
    return out


# ---- max_period: 1, 2, 3, n / 2, above n / 2, and the value that cuts off the otherwise strongest peak ----
def two_period_series(n=240):
    """Two periodicities, 5 and 35; the stronger peak is the longer lag."""
    rng = random.Random(77)
    return [3.0 * math.sin(2 * math.pi * t / 5.0) + 4.0 * math.sin(2 * math.pi * t / 35.0) + rng.gauss(0.0, 0.3) for t in range(n)]


MAX_PERIODS = (1, 2, 3, 8, 35, 36, 120, 121, 10000)


def max_period_batch():
    return [two_period_series(), seasonal(96, 12, 5), noise(50, 6), [10.0, 20.0, 30.0, 40.0] * 4, seasonal(41, 5, 8)]


# ---- lag stride: max_lag 256, 257 and 515 (a lane group's second and third turn at every width of the lag loop) ----
def stride_batch():
    return [seasonal(512, 24, 11), seasonal(514, 128, 12, noise=1.0), noise(1030, 13), seasonal(1030, 365, 14), seasonal(2050, 7, 15),
            noise(2100, 16)]


# ---- storage boundary ----
def boundary_series():
    return [seasonal(LDS_ROWS, 168, 21, noise=1.0), seasonal(LDS_ROWS + 1, 52, 22, noise=1.0)]


# ---- ragged block: every length 0 .. t_rows ----
def ragged_batch(t_rows=70):
    rng = random.Random(31)
    out = []
    for n in range(t_rows + 1):
        p = 2 + n % 9
        out.append([round(5.0 + 2.0 * math.sin(2 * math.pi * t / p) + rng.gauss(0.0, 0.4), 3) for t in range(n)])
    return out


# ---- NULL masks ----
def null_batch():
    s = seasonal(90, 7, 41)
    rng = random.Random(42)
    interior = [None if rng.random() < 0.2 else v for v in s]
    out = [[None] * 9 + s, s + [None] * 11, interior, [None] * 30, [None] * 5 + s[:3] + [None] * 4, [None, 1.0, None, 5.0, 2.0, None, None, 7.0, None],
           [None] * 64 + s[:20] + [None] * 64 + s[20:] + [None] * 3, s]
    long = seasonal(700, 30, 43)
    out.append([None if rng.random() < 0.05 else v for v in long])
    out.append([None if (t // 64) % 2 else v for t, v in enumerate(long)])         # whole 64-row chunks NULL
    return out


# ---- ties: integer series with an integral mean, so that the ACF sums are exact and equal values really occur ----
def _tie_kind(series):
    """(has two peaks of exactly equal ACF, the kept periods are not in ascending order)"""
    acf = R.full_acf(series)
    peaks = [i for i in range(1, len(acf) - 1) if acf[i] > acf[i - 1] and acf[i] > acf[i + 1] and acf[i] > R.THRESHOLD]
    vals = [acf[i] for i in peaks]
    periods = R.analyze(series)["detected_periods"]
    return len(set(vals)) < len(vals), periods != sorted(periods)


def tie_cases(want=12, seed=2024, tries=60000):
    rng = random.Random(seed)
    equal, unordered = [], []
    for _ in range(tries):
        n = rng.randint(12, 40)
        s = [float(rng.randint(0, 3)) for _ in range(n)]
        if int(sum(s)) % n:
            continue
        eq, un = _tie_kind(s)
        if eq and len(equal) < want:
            equal.append(s)
        if un and len(unordered) < want:
            unordered.append(s)
        if len(equal) >= want and len(unordered) >= want:
            break
    return equal, unordered


# ---- more than five peaks; two periodicities; the variance edges; non-finite input ----
def many_peaks_series():
    rng = random.Random(51)
    return [math.sin(2 * math.pi * t / 6.0) + rng.gauss(0.0, 0.2) for t in range(200)]


def edge_batch():
    tiny = [1.0 + (1e-9 if t % 2 else 0.0) for t in range(40)]              # variance 1e-17 < EPSILON
    nan = seasonal(60, 7, 61)
    nan[17] = float("nan")
    inf = seasonal(60, 7, 62)
    inf[33] = float("inf")
    return {"constant": [5.0] * 50, "constant_zero": [0.0] * 13, "tiny_variance": tiny, "ramp": [float(t) for t in range(60)],
            "steep_ramp": [1e6 * t for t in range(33)], "nan": nan, "inf": inf, "neg_inf": [1.0, 2.0, float("-inf"), 4.0, 5.0, 6.0, 7.0, 8.0],
            "huge": [1e200 * x for x in noise(80, 63)], "overflowing_sum": [1.7e308] * 4 + [1.0, -1.7e308, 3.0, 1.7e308],
            "many_peaks": many_peaks_series(), "two_periods": two_period_series()}


def every_short_case():
    """All cases of fewer than FAST_FROM values, with the max_period each is checked at: the CPU suite shows R.analyze_fast equal to
    R.analyze on them."""
    out = [(s, 0) for s in short_batch() + ragged_batch() + null_batch()[:8] + list(edge_batch().values())]
    out += [(s, mp) for s in max_period_batch() for mp in MAX_PERIODS]
    eq, un = tie_cases()
    out += [(s, 0) for s in eq + un]
    return [(s, mp) for s, mp in out if len(R.compact(s)) < 300]


def block(series_list, t_rows=None, extra_cols=5, pad=12345.0):
    """(y [t_rows x ld], valid uint8 or None, lengths int32 [ld], ld) of a time-major block with ld > n_series."""
    n = len(series_list)
    T = max(1, max(len(s) for s in series_list)) if t_rows is None else t_rows
    ld = (n + extra_cols + 63) // 64 * 64
    y = np.full((T, ld), pad)
    v = np.ones((T, ld), dtype=np.uint8)
    any_null = False
    for i, s in enumerate(series_list):
        vals, ok = split(s)
        y[:len(s), i] = vals
        v[:len(s), i] = ok
        any_null = any_null or not all(ok)
    lens = np.zeros(ld, dtype=np.int32)
    lens[:n] = [len(s) for s in series_list]
    return y, (v if any_null else None), lens, ld
