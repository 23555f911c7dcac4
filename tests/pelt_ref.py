"""The yardstick of the PELT entries: the reference's anofox_ts_detect_changepoints (lib.rs:2988-3049) over detect_changepoints with
the L2 cost (changepoint.rs:26-41, 102-175), restated twice.

`literal` is the loops as they are written there, one Python float operation per source operation (Python floats are IEEE doubles,
math.log is the C library's log, nothing is fused): every candidate pair pays a serial sum, one division and a serial sum of
squares.  The pruning sets of the source are never read and are left out.

`fast` is the same arithmetic vectorised over the (tau, t*) pairs for a fixed row j: row j enters the sum of every segment that
holds it, for j ascending, so every pair's chain of additions keeps the source's order, and numpy adds and multiplies element by
element without fusing.  It is used where `literal` is slow.  Its two switches exist only to show that the comparison
discriminates (tests/test_pelt_cpu.py): `rule="last"` takes the last minimum instead of the first, `cost="prefix"` computes a
segment's cost from prefix sums instead of the two passes.
"""
import math

import numpy as np

INF = float("inf")


def sizes(n, min_size, penalty):
    """(ms, pen) as the FFI wrapper and detect_changepoints fix them; pen is None where the series is too short."""
    ms = max(int(min_size), 1)
    if n < 2 * ms:
        return ms, None
    penalty = float(penalty)
    return ms, penalty if penalty > 0.0 else math.log(float(n)) * 2.0


def backtrack(cp, n):
    out, idx = [], n
    while idx > 0:
        tau = cp[idx]
        if tau > 0:
            out.append(tau)
        idx = tau
    out.reverse()
    return out


def literal(values, min_size=2, penalty=0.0):
    """(changepoints, cost) by the source's loops."""
    v = [float(x) for x in values]
    n = len(v)
    ms, pen = sizes(n, min_size, penalty)
    if pen is None:
        return [], 0.0
    f = [-INF] * (n + 1)
    cp = [0] * (n + 1)
    f[0] = -pen
    for t in range(ms, n + 1):
        best, best_tau = INF, 0
        for tau in range(0, t - ms + 1):
            if not (tau == 0 or tau >= ms):
                continue
            s = 0.0
            for j in range(tau, t):
                s = s + v[j]
            mean = s / float(t - tau)
            c = 0.0
            for j in range(tau, t):
                d = v[j] - mean
                c = c + d * d
            cand = f[tau] + c + pen
            if cand < best:
                best, best_tau = cand, tau
        f[t], cp[t] = best, best_tau
    return backtrack(cp, n), f[n]


def segment_costs(v, cost="serial"):
    """C[tau, t] = cost of [tau, t) for every tau < t <= n, every pair's chains in the source's order."""
    n = len(v)
    with np.errstate(all="ignore"):
        if cost == "prefix":      # NOT the source's arithmetic: sum of squares minus the squared sum over n, from prefix sums
            p1 = np.concatenate([[0.0], np.cumsum(v)])
            p2 = np.concatenate([[0.0], np.cumsum(v * v)])
            tau, t = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
            s1, s2 = p1[t] - p1[tau], p2[t] - p2[tau]
            return s2 - s1 * s1 / np.maximum(t - tau, 1)
        S = np.zeros((n + 1, n + 1))
        for j in range(n):        # row j joins every segment with tau <= j < t
            S[:j + 1, j + 1:] += v[j]
        tau, t = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
        mean = S / np.maximum(t - tau, 1).astype(np.float64)
        C = np.zeros((n + 1, n + 1))
        for j in range(n):
            d = v[j] - mean[:j + 1, j + 1:]
            C[:j + 1, j + 1:] += d * d
    return C


def fast(values, min_size=2, penalty=0.0, rule="first", cost="serial"):
    """(changepoints, cost): `literal` with the segment costs from segment_costs."""
    v = np.array([float(x) for x in values], dtype=np.float64)
    n = len(v)
    ms, pen = sizes(n, min_size, penalty)
    if pen is None:
        return [], 0.0
    C = segment_costs(v, cost).tolist()
    f = [-INF] * (n + 1)
    cp = [0] * (n + 1)
    f[0] = -pen
    for t in range(ms, n + 1):
        best, best_tau = INF, 0
        for tau in range(0, t - ms + 1):
            if not (tau == 0 or tau >= ms):
                continue
            cand = f[tau] + C[tau][t] + pen
            if cand < best or (rule == "last" and cand <= best):
                best, best_tau = cand, tau
        f[t], cp[t] = best, best_tau
    return backtrack(cp, n), f[n]


def bits(x):
    return np.float64(x).view(np.uint64).item()


def scalar(values, min_size=None, penalty=None, detect=fast):
    """The list scalar of ts_changepoints.cpp:53-213 over `detect`: None for a NULL list, NULL elements dropped, None for fewer than
    2 values, a NULL min_size is 2 and a NULL penalty 0.0."""
    if values is None:
        return None
    vals = [float(x) for x in values if x is not None]
    if len(vals) < 2:
        return None
    cps, c = detect(vals, 2 if min_size is None else int(min_size), 0.0 if penalty is None else float(penalty))
    return {"changepoints": cps, "n_changepoints": len(cps), "cost": c}
