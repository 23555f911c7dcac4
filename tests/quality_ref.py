"""A pure-Python restatement of the reference's data quality figures (quality.rs compute_data_quality as its FFI entry calls it:
without dates) and of the SQL functions around it.  Python floats are IEEE doubles and every sum below is an explicit
left-to-right loop from 0.0 (never numpy.sum, which sums pairwise), so the figures carry the bits of the source's.  Shares nothing
with the library.

A series is a list whose None elements are NULLs.  A NaN among the values gives status 2 and five NaN scores: the source leaves
that answer to its sort's internals."""
import math
import struct

EPS = 2.220446049250313e-16            # f64::EPSILON
FP_FIELDS = ("structural_score", "temporal_score", "magnitude_score", "behavioral_score", "overall_score")
FIELDS = FP_FIELDS + ("n_gaps", "n_missing", "is_constant")
OK, NAN = 0, 2
NAN_TEXT = "Invalid input: a value is NaN"


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def same_bits(a, b):
    a, b = float(a), float(b)
    return (a != a and b != b) or bits(a) == bits(b)


def clamp01(x):                        # f64::clamp(0.0, 1.0)
    if x < 0.0:
        return 0.0
    if x > 1.0:
        return 1.0
    return x


def mean_of(x):
    s = 0.0
    for v in x:
        s += v
    return s / float(len(x))


def centred_sum(x, mean):
    s = 0.0
    for v in x:
        d = v - mean
        s += d * d
    return s


def is_constant(x):
    if len(x) < 2:
        return True
    first = x[0]
    return all(abs(v - first) < EPS for v in x)


def structural_score(k, n_missing):
    if k == 0 and n_missing > 0:
        return 0.0
    completeness = float(k) / float(k + n_missing)
    length_factor = min(float(k) / 30.0, 1.0)
    return clamp01(completeness * 0.7 + length_factor * 0.3)


def total_order_key(v):
    b = bits(v)
    return (~b) & 0xFFFFFFFFFFFFFFFF if b >> 63 else b | (1 << 63)


def quartiles(x):
    """sorted[(k * 0.25) as usize], sorted[(k * 0.75) as usize]; the sort puts -0.0 below +0.0 (no comparison sees the difference)."""
    k = len(x)
    srt = sorted(x, key=total_order_key)
    return srt[int(float(k) * 0.25)], srt[int(float(k) * 0.75)]


def magnitude_counts(x):
    q1, q3 = quartiles(x)
    iqr = q3 - q1
    lower = q1 - 1.5 * iqr
    upper = q3 + 1.5 * iqr
    outliers = sum(1 for v in x if v < lower or v > upper)
    mean = mean_of(x)
    std = math.sqrt(centred_sum(x, mean) / float(len(x)))          # (a NaN or inf passes through; the sum is never negative)
    extreme = sum(1 for v in x if abs(v - mean) > 4.0 * std)
    return outliers, extreme


def magnitude_score(x):
    if not x:
        return 0.0
    n = float(len(x))
    outliers, extreme = magnitude_counts(x)
    return clamp01(1.0 - (float(outliers) / n) * 2.0 - (float(extreme) / n) * 3.0)


def autocorrelation1(x):
    mean = mean_of(x)
    num = 0.0
    denom = 0.0
    for i, v in enumerate(x):
        denom += (v - mean) * (v - mean)
        if i >= 1:
            num += (v - mean) * (x[i - 1] - mean)
    if abs(denom) < EPS:
        return 0.0
    return num / denom


def behavioral_score(x):
    if len(x) < 3:
        return 0.5
    mean = mean_of(x)
    variance = centred_sum(x, mean) / float(len(x))
    if abs(variance) < EPS:
        return 0.0
    acf1 = autocorrelation1(x)
    penalty = 0.2 if abs(acf1) > 0.95 else 0.0
    return clamp01(1.0 - penalty)


def data_quality(series):
    """(dict keyed by FIELDS, status) of a list with None at the NULLs."""
    n = len(series)
    if n == 0:
        return {**{f: 0.0 for f in FP_FIELDS}, "n_gaps": 0, "n_missing": 0, "is_constant": False}, OK
    x = [float(v) for v in series if v is not None]
    k = len(x)
    out = {"n_gaps": 0, "n_missing": n - k, "is_constant": is_constant(x)}
    if any(v != v for v in x):
        out.update({f: math.nan for f in FP_FIELDS})
        return out, NAN
    s = structural_score(k, n - k)
    t = clamp01(1.0 - (0.0 / float(n)) * 5.0)
    m = magnitude_score(x)
    b = behavioral_score(x)
    out.update(structural_score=s, temporal_score=t, magnitude_score=m, behavioral_score=b, overall_score=(s + t + m + b) / 4.0)
    return out, OK


# ---- the SQL functions ----
def scalar(values):
    """_ts_data_quality: None for a NULL or an empty list and for a list with a NaN."""
    if values is None or len(values) == 0:
        return None
    d, status = data_quality(list(values))
    return d if status == OK else None


def _groups(group, date, value):
    order, rows = [], {}
    for i, g in enumerate(group):
        if g not in rows:
            rows[g] = []
            order.append(g)
        rows[g].append(i)
    lists = []
    for g in order:
        idx = sorted(rows[g], key=lambda i: (date[i] is None, 0 if date[i] is None else date[i]))      # stable, NULL dates last
        lists.append([value[i] for i in idx])
    return order, lists


def table(group, date, value):
    """ts_data_quality / ts_data_quality_by over integer dates (None = NULL)."""
    order, lists = _groups(group, date, value)
    res = [scalar(l) for l in lists]
    out = {"unique_id": order}
    for f in FIELDS:
        out[f] = [None if r is None else r[f] for r in res]
    return out


def summary(group, date, value):
    overall = table(group, date, value)["overall_score"]
    if not overall:
        return {"n_total": 0, "n_good": None, "n_fair": None, "n_poor": None, "avg_score": None}
    known = [x for x in overall if x is not None]
    total = 0.0
    for x in known:
        total += x
    return {"n_total": len(overall), "n_good": sum(1 for x in known if x >= 0.8), "n_fair": sum(1 for x in known if 0.5 <= x < 0.8),
            "n_poor": sum(1 for x in known if x < 0.5), "avg_score": total / len(known) if known else None}


def agg(ts, value):
    pairs = sorted((t, v) for t, v in zip(ts, value) if t is not None and v is not None)
    if not pairs:
        return None
    return scalar([v for _, v in pairs])
