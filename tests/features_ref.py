"""Pure-Python restatement of the reference's feature extraction (features.rs extract_features), the checker of
csrc/features.hip.  It shares nothing with oracle/ and adds every chain with Python floats (IEEE binary64, one rounding per
operation), in the source's order, from 0.0.  powi(2) is x*x, powi(3) is x*(x*x), powi(4) is (x*x)*(x*x).

Where the source has no single answer the order is DEFINED here: the two reoccurring sums run over the distinct
bit patterns in ascending total order (negatives by descending magnitude first, -0.0 below +0.0), the terms of
permutation_entropy over the six patterns in lexicographic order of the index vector.

`log`, `log2` and `sincos` are parameters so that the noise of the elementary functions can be measured: log_shifted(+-1) and
trig_shifted(+-1) move every result one ulp."""
from __future__ import annotations

import math
import struct

EPS = 2.220446049250313e-16
NAN = float("nan")
INF = float("inf")

OK, EMPTY, HAS_NAN = 0, 1, 2


def list_features():
    """features.rs list_features, in its order (117 names)."""
    names = ["length", "sum", "mean", "minimum", "maximum", "range", "variance", "standard_deviation", "variation_coefficient",
             "large_standard_deviation", "median", "quantile_0.1", "quantile_0.25", "quantile_0.75", "quantile_0.9", "skewness",
             "kurtosis", "count_above_mean", "count_below_mean", "percentage_above_mean", "zero_crossing_rate", "mean_change",
             "mean_abs_change", "first_value", "last_value", "first_location_of_maximum", "last_location_of_maximum",
             "first_location_of_minimum", "last_location_of_minimum", "abs_energy", "root_mean_square",
             "mean_second_derivative_central", "cid_ce", "absolute_sum_of_changes", "lempel_ziv_complexity",
             "longest_strike_above_mean", "longest_strike_below_mean", "number_peaks", "number_peaks_threshold_1",
             "number_peaks_threshold_2", "benford_correlation", "linear_trend_slope", "linear_trend_intercept",
             "linear_trend_r_squared", "binned_entropy", "sample_entropy", "approximate_entropy", "permutation_entropy",
             "count_unique", "ratio_value_number_to_length", "has_duplicate", "has_duplicate_max", "has_duplicate_min",
             "percentage_of_reoccurring_datapoints_to_all_datapoints", "percentage_of_reoccurring_values_to_all_values",
             "sum_of_reoccurring_values", "sum_of_reoccurring_datapoints", "spectral_centroid", "spectral_variance",
             "agg_linear_trend_slope", "agg_linear_trend_intercept", "agg_linear_trend_rvalue", "agg_linear_trend_stderr"]
    names += [f"autocorrelation_lag{i}" for i in range(1, 11)]
    names += [f"partial_autocorrelation_lag{i}" for i in range(1, 6)]
    names += [f"ratio_beyond_r_sigma_{i}" for i in range(1, 4)]
    names += [f"time_reversal_asymmetry_stat_{i}" for i in range(1, 4)]
    names += [f"c3_lag{i}" for i in range(1, 4)]
    for i in range(10):
        names += [f"fft_coefficient_{i}_real", f"fft_coefficient_{i}_imag", f"fft_coefficient_{i}_abs"]
    return names


SORTED_NAMES = sorted(list_features(), key=lambda s: s.encode())       # the order of the FFI entry and of out_features
LOG_FEATURES = ("binned_entropy", "sample_entropy", "approximate_entropy", "permutation_entropy", "lempel_ziv_complexity")
TRIG_FEATURES = tuple(f"fft_coefficient_{i}_{p}" for i in range(10) for p in ("real", "imag", "abs")) + ("spectral_centroid",
                                                                                                        "spectral_variance")


def validate_feature_params(keys):
    known = set(list_features())
    return [f"Unknown feature parameter key '{k}' - this parameter will be ignored" for k in keys if k not in known]


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def from_bits(u):
    return struct.unpack("<d", struct.pack("<Q", u))[0]


def same(a, b):
    """Equality of bits up to what the contract exempts: the sign of a zero and the payload of a NaN."""
    return a == b or (a != a and b != b)


def total_key(x):
    """wave_sort.hpp's key: unsigned order = total order of the values."""
    u = bits(x)
    return (~u) & 0xFFFFFFFFFFFFFFFF if u >> 63 else u | (1 << 63)


def _ulp_step(x, k):
    if k == 0 or x != x or math.isinf(x):
        return x
    for _ in range(abs(k)):
        x = math.nextafter(x, INF if k > 0 else -INF)
    return x


def log_shifted(k, fn=math.log, alternate=False):
    """fn with every result moved k ulps; with `alternate` the direction flips from call to call (errors that do not cancel in a
    ratio of logarithms)."""
    state = [k]

    def shifted(x):
        y = _ulp_step(fn(x), state[0])
        if alternate:
            state[0] = -state[0]
        return y
    return shifted


LOG_VARIANTS = ((1, False), (-1, False), (1, True), (-1, True))


def trig_shifted(k):
    return lambda a: (_ulp_step(math.sin(a), k), _ulp_step(math.cos(a), k))


def _sincos(a):
    return math.sin(a), math.cos(a)


# ---- helpers, one per helper of the source ----

def seq_sum(xs):
    s = 0.0
    for x in xs:
        s += x
    return s


def fmin(a, b):
    return b if (a != a or b < a) else a


def fmax(a, b):
    return b if (a != a or b > a) else a


def quantile(srt, q):
    idx = q * float(len(srt) - 1)
    lo, hi = math.floor(idx), math.ceil(idx)
    frac = idx - float(lo)
    if hi >= len(srt):
        return srt[-1]
    return srt[lo] * (1.0 - frac) + srt[hi] * frac


def autocorr(v, lag, mean):
    num = den = 0.0
    for i, x in enumerate(v):
        d = x - mean
        den += d * d
        if i >= lag:
            num += d * (v[i - lag] - mean)
    return 0.0 if abs(den) < EPS else num / den


def partial_autocorr(v, lag, mean):
    a1 = autocorr(v, 1, mean)
    if lag == 1:
        return a1
    a2 = autocorr(v, 2, mean)
    if abs(1.0 - a1 * a1) < EPS:
        return 0.0
    return (a2 - a1 * a1) / (1.0 - a1 * a1)


def longest_strike(v, thr, above):
    best = cur = 0
    for x in v:
        if (x > thr) if above else (x < thr):
            cur += 1
            best = max(best, cur)
        else:
            cur = 0
    return float(best)


def count_peaks(v, mean=None, thr=None):
    c = 0
    for i in range(1, len(v) - 1):
        if v[i] > v[i - 1] and v[i] > v[i + 1] and (thr is None or abs(v[i] - mean) > thr):
            c += 1
    return c


def first_digit(a):
    """First non-zero digit of Rust's to_string() of a finite a >= 1: the shortest round-trip digits, as repr gives them."""
    for ch in repr(a):
        if ch in "123456789":
            return int(ch)
        if ch not in "0.":
            break
    return None


BENFORD_EXPECTED = (0.301, 0.176, 0.125, 0.097, 0.079, 0.067, 0.058, 0.051, 0.046)


def benford_thresholds():
    """The 9 x 309 correctly rounded doubles dEk, ascending: the table the device searches."""
    return [float(f"{d}e{k}") for k in range(309) for d in range(1, 10)]


def first_digit_by_table(a, table=None):
    """The device's rule: the digit d with strtod(dEk) <= a < strtod((d+1)Ek), a finite and >= 1."""
    import bisect
    table = table or benford_thresholds()
    return (bisect.bisect_right(table, a) - 1) % 9 + 1


def benford_counts(v):
    counts = [0] * 9
    for x in v:
        a = abs(x)
        if a >= 1.0 and a != INF:
            counts[first_digit(a) - 1] += 1
    return counts


def benford_correlation(v):
    counts = benford_counts(v)
    total = sum(counts)
    if total == 0:
        return 0.0
    obs = [float(c) / float(total) for c in counts]
    me, mo = seq_sum(BENFORD_EXPECTED) / 9.0, seq_sum(obs) / 9.0
    num = de = do = 0.0
    for e, o in zip(BENFORD_EXPECTED, obs):
        num += (e - me) * (o - mo)
        de += (e - me) * (e - me)
        do += (o - mo) * (o - mo)
    den = math.sqrt(de * do)
    return 0.0 if abs(den) < EPS else num / den


def linear_trend(v):
    if len(v) < 2:
        return 0.0, (v[0] if v else 0.0), 0.0
    n = float(len(v))
    xm = (n - 1.0) / 2.0
    ym = seq_sum(v) / n
    sxy = sxx = syy = 0.0
    for i, y in enumerate(v):
        x = float(i)
        sxy += (x - xm) * (y - ym)
        sxx += (x - xm) * (x - xm)
        syy += (y - ym) * (y - ym)
    slope = sxy / sxx if abs(sxx) > EPS else 0.0
    intercept = ym - slope * xm
    if abs(sxx) > EPS and abs(syy) > EPS:
        r2 = (sxy * sxy) / (sxx * syy)
        r2 = 0.0 if r2 < 0.0 else 1.0 if r2 > 1.0 else r2
    else:
        r2 = 0.0
    return slope, intercept, r2


def _as_usize(x):
    if x != x or x < 0.0:
        return 0
    return int(min(x, 1e18))


def _round_half_away(x):
    if x != x or math.isinf(x):
        return x
    return math.copysign(math.floor(abs(x) + 0.5), x) if abs(x) < 4503599627370496.0 else x


def bin_counts(v, lo, hi, n_bins=10):
    rng = hi - lo
    counts = [0] * n_bins
    for x in v:
        b = _as_usize(_round_half_away(((x - lo) / rng) * float(n_bins - 1)))
        counts[min(b, n_bins - 1)] += 1
    return counts


def binned_entropy(v, lo, hi, log):
    if abs(hi - lo) < EPS:
        return 0.0
    n = float(len(v))
    e = 0.0
    for c in bin_counts(v, lo, hi):
        if c > 0:
            p = float(c) / n
            e -= p * log(p)
    return e


def template_matches(v, m, r):
    """count_template_matches: pairs i < j < n - m.  A NaN difference (inf - inf) is not > r and so matches."""
    n = len(v)
    c = 0
    for i in range(n - m):
        for j in range(i + 1, n - m):
            if all(not (abs(v[i + k] - v[j + k]) > r) for k in range(m)):
                c += 1
    return c


def sample_entropy(v, r, log, matches=template_matches):
    n, m = len(v), 2
    if n < m + 1 or r <= 0.0:
        return NAN
    cm, cm1 = matches(v, m, r), matches(v, m + 1, r)
    if cm == 0 or cm1 == 0:
        return NAN
    pm = float(cm) / float((n - m) * (n - m - 1) // 2)
    pm1 = float(cm1) / float((n - m - 1) * (n - m - 2) // 2)
    return -log(pm1 / pm)


def phi_counts(v, m, r):
    n = len(v)
    out = []
    for i in range(n - m + 1):
        c = 0
        for j in range(n - m + 1):
            if all(not (abs(v[i + k] - v[j + k]) > r) for k in range(m)):
                c += 1
        out.append(c)
    return out


def phi_from_counts(counts, log):
    tot = float(len(counts))
    s = 0.0
    for c in counts:
        if c > 0:
            s += log(float(c) / tot)
    return s / tot


def approximate_entropy(v, r, log, counts=phi_counts):
    if len(v) < 3 or r <= 0.0:
        return NAN, 0.0
    p2, p3 = phi_from_counts(counts(v, 2, r), log), phi_from_counts(counts(v, 3, r), log)
    return p2 - p3, abs(p2) + abs(p3)


PATTERNS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))


def pattern_counts(v):
    counts = [0] * 6
    for i in range(len(v) - 2):
        w = v[i:i + 3]
        idx = tuple(sorted(range(3), key=lambda a: w[a]))              # a stable sort, ties keep index order
        counts[PATTERNS.index(idx)] += 1
    return counts


def permutation_entropy(v, log):
    if len(v) < 3:
        return NAN
    total = float(len(v) - 2)
    e = 0.0
    for c in pattern_counts(v):
        p = float(c) / total
        if p > 0.0:
            e -= p * log(p)
    mx = 0.0
    for i in (1.0, 2.0, 3.0):
        mx += log(i)
    return e / mx if mx > 0.0 else e


def reoccurring(v):
    counts = {}
    for x in v:
        counts[bits(x)] = counts.get(bits(x), 0) + 1
    order = sorted(counts, key=lambda u: total_key(from_bits(u)))
    terms_v = [from_bits(u) for u in order if counts[u] > 1]
    terms_d = [from_bits(u) * float(counts[u]) for u in order if counts[u] > 1]
    n_dp = sum(c for c in counts.values() if c > 1)
    return (float(n_dp) / float(len(v)), float(len(terms_v)) / max(float(len(counts)), 1.0), seq_sum(terms_v), seq_sum(terms_d),
            len(counts), terms_v, terms_d)


def time_reversal_asymmetry(v, lag):
    s = 0.0
    for i in range(lag, len(v) - lag):
        s += (v[i + lag] * v[i + lag]) * v[i] - v[i - lag] * (v[i] * v[i])
    return s / float(len(v) - 2 * lag)


def c3(v, lag):
    s = 0.0
    for i in range(len(v) - 2 * lag):
        s += v[i] * v[i + lag] * v[i + 2 * lag]
    return s / float(len(v) - 2 * lag)


def lempel_ziv_count(v, thr):
    """The source's scan, literally: the inner range `0..l + k - k` is 0..l, so a match may overlap the substring itself.  (The
    substring occurs at l, so "some start below l matches" is "its first occurrence starts below l".)"""
    b = "".join("1" if x >= thr else "0" for x in v)
    n = len(b)
    complexity, l, k, k_max = 1, 1, 1, 1
    while l + k <= n:
        found = b.find(b[l:l + k]) < l
        if found:
            k += 1
            k_max = max(k_max, k)
        else:
            complexity += 1
            l += k_max
            k = k_max = 1
    return complexity


def lempel_ziv_complexity(v, thr, log2=math.log2):
    n = len(v)
    bb = log2(float(n))
    return float(lempel_ziv_count(v, thr)) * bb / float(n) if bb > 0.0 else 0.0


def simple_dft(v, sincos=_sincos):
    n = len(v)
    out = []
    for k in range(n):
        re = im = 0.0
        for t, x in enumerate(v):
            ang = -2.0 * math.pi * float(k) * float(t) / float(n)
            s, c = sincos(ang)
            re += x * c
            im += x * s
        out.append((re / float(n), im / float(n)))
    return out


def spectral_features(coeffs):
    power = [r * r + i * i for r, i in coeffs]
    total = seq_sum(power)
    if total <= EPS:
        return 0.0, 0.0
    cen = seq_sum(float(i) * p for i, p in enumerate(power)) / total
    var = seq_sum(((float(i) - cen) * (float(i) - cen)) * p for i, p in enumerate(power)) / total
    return cen, var


def aggregated_linear_trend(v):
    cl = max(len(v) // 10, 2)
    if len(v) < cl:
        return 0.0, 0.0, 0.0, 0.0
    means = [seq_sum(v[i:i + cl]) / float(len(v[i:i + cl])) for i in range(0, len(v), cl)]
    if len(means) < 2:
        return 0.0, means[0], 0.0, 0.0
    slope, intercept, r2 = linear_trend(means)
    n = float(len(means))
    xm = (n - 1.0) / 2.0
    sxx = seq_sum((float(i) - xm) * (float(i) - xm) for i in range(len(means)))
    rss = 0.0
    for i, y in enumerate(means):
        d = y - (intercept + slope * float(i))
        rss += d * d
    stderr = math.sqrt(rss / (n - 2.0) / sxx) if n > 2.0 and sxx > EPS else 0.0
    return slope, intercept, math.sqrt(r2), stderr


def extract_features(values, log=math.log, sincos=_sincos, matches=template_matches, counts=phi_counts, want=None, dft=None, log2=math.log2):
    """(status, {name: value}): the features the source inserts, for a non-empty list without a NaN.  A NaN among the values gives
    (HAS_NAN, {"length": n}); an empty list (EMPTY, {}).  `want`: restrict the O(n^2) families ("match", "dft", "lz") for speed; `matches`, `counts` and `dft` may replace the
    pure-Python template counters and DFT (tests/features_cases.py counts with numpy above 64 rows)."""
    v = [float(x) for x in values]
    if not v:
        return EMPTY, {}
    if any(x != x for x in v):
        return HAS_NAN, {"length": float(len(v))}
    want = {"match", "dft", "lz"} if want is None else set(want)
    f = {}
    ln = len(v)
    n = float(ln)
    total = seq_sum(v)
    mean = total / n
    f["length"], f["sum"], f["mean"] = n, total, mean
    lo, hi = INF, -INF
    for x in v:
        lo, hi = fmin(lo, x), fmax(hi, x)
    f["minimum"], f["maximum"], f["range"] = lo, hi, hi - lo
    var = seq_sum((x - mean) * (x - mean) for x in v) / n
    sd = math.sqrt(var)
    f["variance"], f["standard_deviation"] = var, sd
    f["variation_coefficient"] = sd / abs(mean) if abs(mean) > EPS else NAN
    f["large_standard_deviation"] = 1.0 if sd > 0.25 * (hi - lo) else 0.0
    srt = sorted(v)
    f["median"] = (srt[ln // 2 - 1] + srt[ln // 2]) / 2.0 if ln % 2 == 0 else srt[ln // 2]
    for q, name in ((0.1, "quantile_0.1"), (0.25, "quantile_0.25"), (0.75, "quantile_0.75"), (0.9, "quantile_0.9")):
        f[name] = quantile(srt, q)
    if sd > EPS:
        s3 = s4 = 0.0
        for x in v:
            z = (x - mean) / sd
            s3 += z * (z * z)
        for x in v:
            z = (x - mean) / sd
            s4 += (z * z) * (z * z)
        f["skewness"], f["kurtosis"] = s3 / n, s4 / n - 3.0
    above, below = sum(1 for x in v if x > mean), sum(1 for x in v if x < mean)
    f["count_above_mean"], f["count_below_mean"], f["percentage_above_mean"] = float(above), float(below), float(above) / n
    zc = sum(1 for a, b in zip(v, v[1:]) if a != 0.0 and b != 0.0 and (a < 0.0) != (b < 0.0))
    f["zero_crossing_rate"] = float(zc) / max(n - 1.0, 1.0)
    if ln > 1:
        ch = [b - a for a, b in zip(v, v[1:])]
        f["mean_change"] = seq_sum(ch) / float(len(ch))
        f["mean_abs_change"] = seq_sum(abs(c) for c in ch) / float(len(ch))
        f["cid_ce"] = math.sqrt(seq_sum(c * c for c in ch))
        f["absolute_sum_of_changes"] = seq_sum(abs(c) for c in ch)
    for lag in range(1, 11):
        if ln > lag:
            f[f"autocorrelation_lag{lag}"] = autocorr(v, lag, mean)
    for lag in range(1, 6):
        if ln > lag + 1:
            f[f"partial_autocorrelation_lag{lag}"] = partial_autocorr(v, lag, mean)
    f["first_value"], f["last_value"] = v[0], v[-1]
    for name, target in (("maximum", hi), ("minimum", lo)):
        hits = [i for i, x in enumerate(v) if abs(x - target) < EPS]
        f[f"first_location_of_{name}"] = float(hits[0] if hits else 0) / n
        f[f"last_location_of_{name}"] = float(hits[-1] if hits else 0) / n
        f[f"has_duplicate_{name[:3]}"] = 1.0 if len(hits) > 1 else 0.0
    energy = seq_sum(x * x for x in v)
    f["abs_energy"], f["root_mean_square"] = energy, math.sqrt(energy / n)
    if ln > 2:
        f["mean_second_derivative_central"] = seq_sum(v[i + 2] - 2.0 * v[i + 1] + v[i] for i in range(ln - 2)) / float(ln - 2)
    f["longest_strike_above_mean"] = longest_strike(v, mean, True)
    f["longest_strike_below_mean"] = longest_strike(v, mean, False)
    f["number_peaks"] = float(count_peaks(v))
    f["number_peaks_threshold_1"] = float(count_peaks(v, mean, 1.0 * sd))
    f["number_peaks_threshold_2"] = float(count_peaks(v, mean, 2.0 * sd))
    f["benford_correlation"] = benford_correlation(v)
    f["linear_trend_slope"], f["linear_trend_intercept"], f["linear_trend_r_squared"] = linear_trend(v)
    f["binned_entropy"] = binned_entropy(v, lo, hi, log)
    r = 0.2 * sd
    if "match" in want:
        f["sample_entropy"] = sample_entropy(v, r, log, matches)
        f["approximate_entropy"] = approximate_entropy(v, r, log, counts)[0]
    f["permutation_entropy"] = permutation_entropy(v, log)
    for k in (1, 2, 3):
        thr = float(k) * sd
        f[f"ratio_beyond_r_sigma_{k}"] = float(sum(1 for x in v if abs(x - mean) > thr)) / n
    pd, pv, sv, sdp, uniq, _, _ = reoccurring(v)
    f["count_unique"], f["ratio_value_number_to_length"] = float(uniq), float(uniq) / n
    f["has_duplicate"] = 1.0 if uniq < ln else 0.0
    f["percentage_of_reoccurring_datapoints_to_all_datapoints"] = pd
    f["percentage_of_reoccurring_values_to_all_values"] = pv
    f["sum_of_reoccurring_values"], f["sum_of_reoccurring_datapoints"] = sv, sdp
    for lag in (1, 2, 3):
        if ln > 2 * lag:
            f[f"time_reversal_asymmetry_stat_{lag}"] = time_reversal_asymmetry(v, lag)
            f[f"c3_lag{lag}"] = c3(v, lag)
    if "lz" in want:
        f["lempel_ziv_complexity"] = lempel_ziv_complexity(v, mean, log2)
    if "dft" in want:
        co = dft(v) if dft is not None else simple_dft(v, sincos)
        for i, (re, im) in enumerate(co[:10]):
            f[f"fft_coefficient_{i}_real"], f[f"fft_coefficient_{i}_imag"] = re, im
            f[f"fft_coefficient_{i}_abs"] = math.sqrt(re * re + im * im)
        f["spectral_centroid"], f["spectral_variance"] = spectral_features(co)
    (f["agg_linear_trend_slope"], f["agg_linear_trend_intercept"], f["agg_linear_trend_rvalue"],
     f["agg_linear_trend_stderr"]) = aggregated_linear_trend(v)
    return OK, f


DUMMY_COLUMNS = tuple(k for k in SORTED_NAMES if k in extract_features([float(i) for i in range(1, 11)])[1])   # the 116 columns


def noise(values, names, base, variants):
    """Per name the largest |variant - base| over the variants: the noise of the elementary function for this input."""
    out = {k: 0.0 for k in names}
    for var in variants:
        for k in names:
            if k in base and k in var and base[k] == base[k] and var[k] == var[k]:
                out[k] = max(out[k], abs(var[k] - base[k]))
    return out


def operator_series(group, ts, value):
    """The loop of _ts_features_native up to its FFI call: (ids, series) -- groups in first-arrival order, rows with a NULL
    timestamp dropped, a NULL value (None) is NaN, each group's pairs sorted by (timestamp, value)."""
    order, rows = [], {}
    for g, t, x in zip(group, ts, value):
        if t is None:
            continue
        key = "__NULL__" if g is None else str(g)
        if key not in rows:
            rows[key] = (g, [])
            order.append(key)
        rows[key][1].append((int(t), NAN if x is None else float(x)))
    ids, out = [], []
    for key in order:
        g, pairs = rows[key]
        ids.append(g)
        out.append([x for _, x in (pairs if any(x != x for _, x in pairs) else sorted(pairs))])
    return ids, out


def ts_features_by(group, ts, value):
    """_ts_features_native: per group of operator_series the 116 columns of the dummy series; NaN where the source inserts nothing,
    and for a group with a NaN everywhere but in `length`."""
    ids, groups = operator_series(group, ts, value)
    out = {"id": ids, **{c: [] for c in DUMMY_COLUMNS}}
    for vals in groups:
        _, f = extract_features(vals)
        for c in DUMMY_COLUMNS:
            out[c].append(f.get(c, NAN))
    return out
