"""Checker of csrc/period_search.hip: the reference's ssa_period (periods.rs:800-937) and stl_period (:952-1120), restated op for
op.  No fused multiply-add anywhere, powi(2) is x * x, every iter().sum() is a sequential sum from 0.0 in index order, so the
kernels, which perform the same IEEE operations, agree with it bit for bit.  Each method is written twice: *_plain on Python
floats, and a numpy form that keeps the serial order (covariance as C += outer(y[t:t+l], y[t:t+l]) for t ascending, the matvec as
a = a + C[:, j] * v[j] for j ascending, the deflation as C - outer(lambda * v, v)); tests/test_period_search_cpu.py holds the two
equal with ==.  Source quirks are restated, not repaired: variance_explained may exceed 1 by rounding, components beyond a
series' rank iterate on rounding residue, the period is NaN when no eigenvector qualifies."""
import math

import numpy as np

import mstl_ref as M

EPS = 2.220446049250313e-16          # f64::EPSILON
SSA_MAX_WINDOW, SSA_MAX_COMPONENTS, STL_MAX_CANDIDATES, MAX_ROWS = 2048, 32, 64, 65536       # the backend's limits


class InsufficientData(Exception):
    def __init__(self, needed, got):
        super().__init__(f"Insufficient data: need at least {needed} observations, got {got}")


class InvalidInput(Exception):
    def __init__(self, text):
        super().__init__(f"Invalid input: {text}")


def _seqsum(v):
    s = 0.0
    for x in v:
        s += x
    return s


def ssa_window(n, window_size=None):
    """l = window_size.unwrap_or(n / 3).min(n / 2).max(4); None or 0 is the default (the FFI's argument rule)."""
    return max(min(window_size if window_size else n // 3, n // 2), 4)


def _periods_of(eigenvectors, n):
    detected = []
    for vec in eigenvectors[:4]:
        crossings = 0
        for i in range(1, len(vec)):
            if (vec[i - 1] >= 0.0 and vec[i] < 0.0) or (vec[i - 1] < 0.0 and vec[i] >= 0.0):
                crossings += 1
        if crossings > 0:
            period = 2.0 * float(len(vec)) / float(crossings)
            if period > 2.0 and period < float(n) / 2.0:
                detected.append(period)
    return detected


def _ssa_result(eigenvalues, eigenvectors, iterations, n, l):
    detected = _periods_of(eigenvectors, n)
    total = _seqsum(eigenvalues)
    ve = _seqsum(eigenvalues[:2]) / total if eigenvalues and total > 0.0 else 0.0
    return {"period": detected[0] if detected else math.nan, "variance_explained": ve, "eigenvalues": eigenvalues,
            "n_eigenvalues": len(eigenvalues), "detected_periods": detected, "iterations": iterations, "window": l, "method": "ssa"}


def ssa_period_plain(values, window_size=None, n_components=None):
    y = [float(v) for v in values]
    n = len(y)
    if n < 16:
        raise InsufficientData(16, n)
    l = ssa_window(n, window_size)
    k = n - l + 1
    kd = float(k)
    C = [[0.0] * l for _ in range(l)]
    for i in range(l):
        for j in range(l):
            s = 0.0
            for t in range(k):
                s += y[i + t] * y[j + t]
            C[i][j] = s / kd
    n_comp = min(n_components if n_components else 10, l)
    eigenvalues, eigenvectors, iterations = [], [], []
    for _ in range(n_comp):
        v = [1.0 / float(i + 1) for i in range(l)]
        v_norm = math.sqrt(_seqsum(x * x for x in v))
        v = [x / v_norm for x in v]
        steps = 0
        for _ in range(100):
            steps += 1
            v_new = [0.0] * l
            for i in range(l):
                row, a = C[i], 0.0
                for j in range(l):
                    a += row[j] * v[j]
                v_new[i] = a
            norm = math.sqrt(_seqsum(x * x for x in v_new))
            if norm < EPS:
                break
            v_new = [x / norm for x in v_new]
            diff = _seqsum(abs(a - b) for a, b in zip(v, v_new))
            v = v_new
            if diff < 1e-10:
                break
        cv = [0.0] * l
        for i in range(l):
            row, a = C[i], 0.0
            for j in range(l):
                a += row[j] * v[j]
            cv[i] = a
        lam = _seqsum(a * b for a, b in zip(v, cv))
        if abs(lam) < EPS:
            break
        eigenvalues.append(lam)
        eigenvectors.append(list(v))
        iterations.append(steps)
        for i in range(l):
            lv = lam * v[i]
            row = C[i]
            for j in range(l):
                row[j] -= lv * v[j]
    return _ssa_result(eigenvalues, eigenvectors, iterations, n, l)


def ssa_period(values, window_size=None, n_components=None):
    """The numpy form: the same operations in the same order, fast enough for windows of a few hundred."""
    y = np.asarray(values, dtype=np.float64)
    n = len(y)
    if n < 16:
        raise InsufficientData(16, n)
    l = ssa_window(n, window_size)
    k = n - l + 1
    with np.errstate(all="ignore"):
        C = np.zeros((l, l))
        for t in range(k):
            seg = y[t:t + l]
            C += np.outer(seg, seg)
        C = C / float(k)
        n_comp = min(n_components if n_components else 10, l)
        eigenvalues, eigenvectors, iterations = [], [], []
        for _ in range(n_comp):
            v = 1.0 / (np.arange(l, dtype=np.float64) + 1.0)
            v = v / math.sqrt(_seqsum((v * v).tolist()))
            steps = 0
            for _ in range(100):
                steps += 1
                a = np.zeros(l)
                for j in range(l):
                    a = a + C[:, j] * v[j]
                norm = math.sqrt(_seqsum((a * a).tolist()))
                if norm < EPS:
                    break
                a = a / norm
                diff = _seqsum(np.abs(v - a).tolist())
                v = a
                if diff < 1e-10:
                    break
            cv = np.zeros(l)
            for j in range(l):
                cv = cv + C[:, j] * v[j]
            lam = _seqsum((v * cv).tolist())
            if abs(lam) < EPS:
                break
            eigenvalues.append(lam)
            eigenvectors.append(v.tolist())
            iterations.append(steps)
            C = C - np.outer(lam * v, v)
    return _ssa_result(eigenvalues, eigenvectors, iterations, n, l)


def _round_half_away(x):
    f = math.floor(x)
    return int(f) + (1 if x - f >= 0.5 else 0)


def stl_n_candidates(n_candidates=None):
    return max(n_candidates if n_candidates else 20, 5)


def stl_candidates(n, min_period=None, max_period=None, n_candidates=None):
    """The candidate list (ascending, deduplicated); raises the source's two InvalidInput errors."""
    min_p = max(min_period if min_period else 4, 2)
    max_p = min(max_period if max_period else n // 3, n // 2)
    n_cand = stl_n_candidates(n_candidates)
    if min_p >= max_p:
        raise InvalidInput("min_period must be less than max_period")
    step = max(float(max_p - min_p) / float(n_cand), 1.0)
    cands = {p for p in (_round_half_away(float(min_p) + float(i) * step) for i in range(n_cand))
             if p >= min_p and p <= max_p and p >= 2 and n >= 2 * p}
    if not cands:
        raise InvalidInput("No valid candidate periods found")
    return sorted(cands)


def _clamp0(x):
    """f64::max(0.0): the other operand for a NaN."""
    return 0.0 if (x != x or x < 0.0) else x


def strengths_plain(d):
    """(seasonal_strength, trend_strength) of one applied decomposition: the source's four variances, as it writes them."""
    seasonal, trend, remainder = [float(x) for x in d["seasonal"][0]], [float(x) for x in d["trend"]], [float(x) for x in d["remainder"]]
    n = len(remainder)

    def var(v):
        mean = _seqsum(v) / float(len(v))
        return _seqsum((x - mean) * (x - mean) for x in v) / float(len(v))
    var_detrended = var([s + r for s, r in zip(seasonal, remainder)])
    var_remainder = var(remainder)
    ss = _clamp0(1.0 - var_remainder / var_detrended) if var_detrended > EPS else 0.0
    var_with_trend = var([t + r for t, r in zip(trend, remainder)])
    var_remainder = var(remainder)
    ts = _clamp0(1.0 - var_remainder / var_with_trend) if var_with_trend > EPS else 0.0
    assert n == len(seasonal) == len(trend)
    return ss, ts


def strengths(d):
    """The numpy form of strengths_plain."""
    seasonal, trend, remainder = np.asarray(d["seasonal"][0], dtype=np.float64), np.asarray(d["trend"], dtype=np.float64), np.asarray(d["remainder"], dtype=np.float64)

    def var(v):
        nd = float(len(v))
        dev = v - _seqsum(v.tolist()) / nd
        return _seqsum((dev * dev).tolist()) / nd
    with np.errstate(all="ignore"):
        var_detrended, var_remainder, var_with_trend = var(seasonal + remainder), var(remainder), var(trend + remainder)
        ss = _clamp0(1.0 - var_remainder / var_detrended) if var_detrended > EPS else 0.0
        ts = _clamp0(1.0 - var_remainder / var_with_trend) if var_with_trend > EPS else 0.0
    return ss, ts


def _stl_period(values, min_period, max_period, n_candidates, strengths_of, plain):
    y = [float(v) for v in values]
    n = len(y)
    if n < 16:
        raise InsufficientData(16, n)
    cands = stl_candidates(n, min_period, max_period, n_candidates)
    if plain:
        mean = _seqsum(y) / float(n)
        total_var = _seqsum((v - mean) * (v - mean) for v in y) / float(n)
    else:
        a = np.asarray(y)
        dev = a - _seqsum(y) / float(n)
        total_var = _seqsum((dev * dev).tolist()) / float(n)
    if total_var < EPS:
        return {"period": math.nan, "seasonal_strength": 0.0, "trend_strength": 0.0, "candidates": cands,
                "candidate_strengths": [0.0] * len(cands), "index": -1, "method": "stl"}
    best, best_s, best_t, cs = 0, 0.0, 0.0, []
    for i, p in enumerate(cands):
        d = M.mstl_decompose(y, [p], M.TREND)
        if d.get("applied") and len(d["seasonal"]) > 0:
            ss, ts = strengths_of(d)
        else:
            ss, ts = 0.0, 0.0
        cs.append(ss)
        if ss > best_s:
            best, best_s, best_t = i, ss, ts
    return {"period": float(cands[best]), "seasonal_strength": best_s, "trend_strength": best_t, "candidates": cands,
            "candidate_strengths": cs, "index": best, "method": "stl"}


def stl_period_plain(values, min_period=None, max_period=None, n_candidates=None):
    return _stl_period(values, min_period, max_period, n_candidates, strengths_plain, True)


def stl_period(values, min_period=None, max_period=None, n_candidates=None):
    return _stl_period(values, min_period, max_period, n_candidates, strengths, False)


# ---------------------------------------------------------------------------------------------------------------------------
# where the kernels keep their data (csrc/host_period_search.hpp): the tests put shapes on both sides of each boundary
# ---------------------------------------------------------------------------------------------------------------------------
SSA_WAVE_WINDOW, TILE, LDS_DOUBLES = 64, 2048, 7936


def ssa_matrix_in_lds(n, l):
    return l * l + 3 * l + (n if n <= TILE else 0) <= LDS_DOUBLES


def stl_rows_in_lds(n):
    return 4 * (2 * n + n // 2) + (n if n <= TILE else 0) <= LDS_DOUBLES
