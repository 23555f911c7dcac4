"""Pure-Python restatement of the data-preparation chain, following the source's loops: gaps.rs:78-259 (fill_gaps, the four
FrequencyTypes), the ts_drop_*_zeros_by macros (ts_macros.cpp:208-256) and imputation.rs.  A series is a list of dates (int
microseconds, or None when the call has none) and a list of values in which None is a NULL.  Every operation is integer logic
or a handful of fp64 operations on Python floats (IEEE doubles, no fused multiply-add), so the contract with the GPU is `==` on
bits."""
from __future__ import annotations

import math
import struct

from stats_ref import year_month

TRIMS = {"none": 0, "leading": 1, "trailing": 2, "edge": 3}
FILLS = {"none": 0, "const": 1, "forward": 2, "backward": 3, "mean": 4, "interpolate": 5}
MAX_ROWS = 1 << 24
NAN = float("nan")


def bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def _trunc_div(a: int, b: int) -> int:
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def _wrap(x: int) -> int:
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >= (1 << 63) else x


def month_start_micros(year: int, month: int) -> int:
    """datetime_to_micros of year-month-01 00:00:00 (days from the civil date, proleptic Gregorian)."""
    y = year - (1 if month <= 2 else 0)
    era = y // 400
    yoe = y - era * 400
    doy = (153 * (month - 3 if month > 2 else month + 9) + 2) // 5
    doe = yoe * 365 + yoe // 4 - yoe // 100 + doy
    return (era * 146097 + doe - 719468) * 86400 * 1000000


def _period(micros: int, ftype: str):
    """(period index, year, first month of the period) of micros_to_datetime(micros)."""
    y, m = year_month(micros)
    if ftype == "MONTHLY":
        return y * 12 + m, y, m
    if ftype == "QUARTERLY":
        return y * 4 + (m - 1) // 3, y, ((m - 1) // 3) * 3 + 1
    return y, y, 1


def fill_gaps(dates, values, frequency_micros, ftype="FIXED", sort=True):
    """gaps.rs fill_gaps.  sort=False is the device entry: the loop over the rows as they lie."""
    if ftype == "FIXED" and frequency_micros <= 0:
        raise ValueError("Frequency must be positive for fixed intervals")
    n = len(dates)
    if n <= 1:
        return list(dates), list(values)
    pairs = list(zip(dates, values))
    if sort:
        pairs.sort(key=lambda p: p[0])                  # sort_by_key: stable
    out_d, out_v = [pairs[0][0]], [pairs[0][1]]
    for i in range(1, n):
        pd, cd = pairs[i - 1][0], pairs[i][0]
        if ftype == "FIXED":
            steps = _trunc_div(_wrap(cd - pd), frequency_micros)
            for step in range(1, steps):
                out_d.append(_wrap(pd + step * frequency_micros))
                out_v.append(None)
        else:
            pp, py, pm0 = _period(pd, ftype)
            cp, _, _ = _period(cd, ftype)
            diff = cp - pp
            if diff > 1:
                k = {"MONTHLY": 1, "QUARTERLY": 3, "YEARLY": 12}[ftype]
                for step in range(1, diff):
                    idx = py * 12 + (pm0 - 1) + step * k     # start of the previous row's period plus `step` periods
                    out_d.append(month_start_micros(idx // 12, idx % 12 + 1))
                    out_v.append(None)
        out_d.append(cd)
        out_v.append(pairs[i][1])
    return out_d, out_v


def is_nonzero(v) -> bool:
    """value_col != 0 AND value_col IS NOT NULL: -0.0 is a zero, NaN is non-zero, a NULL is not non-zero."""
    return v is not None and not (v == 0.0)


def trim_bounds(values, mode):
    """(rows trimmed at the front, rows trimmed at the back)."""
    n = len(values)
    if mode == "none":
        return 0, 0
    nz = [i for i, v in enumerate(values) if is_nonzero(v)]
    if not nz:
        return (n, 0) if mode in ("leading", "edge") else (0, n)
    front = nz[0] if mode in ("leading", "edge") else 0
    back = n - 1 - nz[-1] if mode in ("trailing", "edge") else 0
    return front, back


def fill_nulls_const(values, c):
    return [c if v is None else v for v in values]


def fill_nulls_forward(values):
    out, last = [], None
    for v in values:
        if v is not None:
            last = v
        out.append(v if v is not None else last)
    return out


def fill_nulls_backward(values):
    out, nxt = [None] * len(values), None
    for i in range(len(values) - 1, -1, -1):
        if values[i] is not None:
            nxt = values[i]
        out[i] = values[i] if values[i] is not None else nxt
    return out


def fill_nulls_mean(values):
    non_null = [v for v in values if v is not None]
    if not non_null:
        return [NAN] * len(values)
    s = 0.0
    for v in non_null:
        s = s + v
    mean = s / float(len(non_null))
    return [mean if v is None else v for v in values]


def fill_nulls_interpolate(values):
    n = len(values)
    out = [NAN] * n
    idx = [i for i, v in enumerate(values) if v is not None]
    if not idx:
        return out
    first, last = idx[0], idx[-1]
    for i in range(first):
        out[i] = values[first]
    for i in range(last + 1, n):
        out[i] = values[last]
    prev, pv = first, values[first]
    out[first] = pv
    for i in range(first + 1, last + 1):
        v = values[i]
        if v is not None:
            gap = i - prev
            if gap > 1:
                slope = (v - pv) / float(gap)
                for j in range(1, gap):
                    out[prev + j] = pv + slope * float(j)
            out[i] = v
            prev, pv = i, v
    return out


def fill_nulls(values, fill, fill_value=0.0):
    if fill == "none":
        return list(values)
    if fill == "const":
        return fill_nulls_const(values, fill_value)
    return {"forward": fill_nulls_forward, "backward": fill_nulls_backward, "mean": fill_nulls_mean,
            "interpolate": fill_nulls_interpolate}[fill](values)


def min_max(values):
    """MIN and MAX of the valid values as DuckDB ranks them: NaN above every number; (NaN, NaN) without a valid value."""
    vs = [v for v in values if v is not None]
    nums = [v for v in vs if not math.isnan(v)]
    if not vs:
        return NAN, NAN
    lo = hi = None
    for v in nums:                                        # strict comparisons: of -0.0 and 0.0 the first seen stays
        if lo is None or v < lo:
            lo = v
        if hi is None or v > hi:
            hi = v
    vmin = lo if nums else NAN
    vmax = NAN if len(nums) < len(vs) else hi
    return vmin, vmax


def prepare(dates, values, gaps=False, frequency_micros=0, ftype="FIXED", trim="none", fill="none", fill_value=0.0, sort=False,
            t_out=None):
    """The chain of anofox_hip_prepare_device for one series: gaps, trim, fill, then the figures.  `dates` may be None unless
    gaps.  t_out: rows of the output block (None: count mode).  Returns a dict: dates (None without dates), values (None = NULL),
    figures (the eight int64 figures), min, max."""
    n = len(values)
    n_null_in = sum(1 for v in values if v is None)
    d, v = (list(dates) if dates is not None else None), list(values)
    if sort and d is not None:
        order = sorted(range(n), key=lambda i: d[i])
        d, v = [d[i] for i in order], [v[i] for i in order]
    if gaps:
        d, v = fill_gaps(d, v, frequency_micros, ftype, sort=False)
    inserted = len(v) - n
    front, back = trim_bounds(v, trim)
    v = v[front:len(v) - back]
    if d is not None:
        d = d[front:len(d) - back]
    status = 0
    if n + inserted > MAX_ROWS:
        status = 2
    elif t_out is not None and len(v) > t_out:
        status = 1
    if status:
        return {"dates": [] if d is not None else None, "values": [], "figures": [n, n_null_in, inserted, front, back, 0, 0, status],
                "min": NAN, "max": NAN}
    v = fill_nulls(v, fill, fill_value)
    vmin, vmax = min_max(v)
    figs = [n, n_null_in, inserted, front, back, sum(1 for x in v if x is None), sum(1 for x in v if is_nonzero(x)), 0]
    return {"dates": d, "values": v, "figures": figs, "min": vmin, "max": vmax}


def same_values(a, b) -> bool:
    """Two value lists are the same cells: NULL where NULL, else the same bits."""
    return len(a) == len(b) and all((x is None and y is None) or (x is not None and y is not None and bits(x) == bits(y))
                                    for x, y in zip(a, b))
