"""A restatement of the ETS start states and of the ETS recursion that stands outside oracle/: what the kernels and oracle/ets.c call
"fitted values" and "final states" must BE the innovations recursion of the textbook, run from the start states DESIGN describes, at
the parameters the record itself reports.  Plain numpy; every function takes the number format as an argument and is run once in
np.float64 and once in np.longdouble (80-bit): the difference between the two evaluations is a series' own conditioning (`noise`).

Written from Hyndman, Koehler, Ord & Snyder 2008, tables 2.1 - 2.3 (state-space form: the recursions on y_t, mu_t and the states, with
alpha, beta, gamma, phi in MODEL terms) and from the description of the start states: classical decomposition, least squares of the
seasonally adjusted series on t = 1..n, the mean of the first max(10, 2 m) adjusted values.  Nothing of the operation order of the
kernels or of oracle/ets.c: no fused multiply-add, no shared reciprocal, no per-phase sums, no series for b^phi (a true `**`), the moving
average a convolution, the regression in centred form.

A spec is its notation ("AAdA", "MNM", ...; inspect_ref.parts).  Series of one family are replayed TOGETHER: the states are arrays over
the series, the time loop is shared, a series that has ended keeps its states.
"""
from __future__ import annotations

import numpy as np

import inspect_ref as R

LD = np.longdouble
FORMATS = (np.float64, np.longdouble)
FIGURE_FLOOR = 1.0e-2          # a multiplicative seasonal figure is at least this
NUDGE_BELOW = 1.0e-8           # additive trend: |l0 + b0| below this moves both by a thousandth
SMALL_STATE = 1.0e-8           # multiplicative trend: a level or growth rate below this takes the first two adjusted values instead
FALLBACK_FLOOR = 1.0e-3        # ... each floored at this
GROWTH_CAP = 1.0e10            # multiplicative trend: |b0| is at most this
Z_TABLE = ((0.99, 2.576), (0.95, 1.96), (0.90, 1.645), (0.80, 1.28))         # five steps: below 0.80 z = 1


def moving_average(y, m, dtype):
    """Centred moving average of order m as a convolution: m weights 1 / m for an odd period, m + 1 weights with half-weight ends
    (a 2 x m average) for an even one.  Returns the values at the interior centres m // 2 .. n - 1 - m // 2."""
    y = np.asarray(y, dtype=dtype)
    if m % 2:
        w = np.full(m, dtype(1)) / dtype(m)
    else:
        w = np.full(m + 1, dtype(1))
        w[0] = w[-1] = dtype(1) / dtype(2)
        w = w / dtype(m)
    return np.convolve(y, w, mode="valid")


def seasonal_figure(y, m, kind, dtype):
    """Classical decomposition: per-phase mean of y - trend ("A") or y / trend ("M") over the interior centres, normalised to mean 0 /
    mean 1.  Returns (figure [m] before the floor, figure [m])."""
    y = np.asarray(y, dtype=dtype)
    n, half = len(y), m // 2
    trend = moving_average(y, m, dtype)
    centre = np.arange(half, n - half)
    assert len(trend) == len(centre)
    detr = y[centre] - trend if kind == "A" else y[centre] / trend
    fig = np.array([np.mean(detr[centre % m == p]) for p in range(m)], dtype=dtype)
    raw = fig - np.mean(fig) if kind == "A" else fig / np.mean(fig)
    return raw, (raw if kind == "A" else np.maximum(raw, dtype(FIGURE_FLOOR)))


def _rel_gap(value, threshold):
    """(value - threshold) / threshold: how far a quantity is ABOVE the threshold of a clamp, relative to the threshold."""
    return float((value - threshold) / threshold)


def start_states(y, notation, m, dtype=np.float64):
    """Start states of spec `notation` on series y: {"level", "growth" (None without a trend), "seasonal" ([m], None without a season),
    "clamps"}.  clamps[name] is the relative distance of the deciding quantity from the threshold of clamp `name`, POSITIVE on the side
    where the clamp does not act:
        figure_floor      smallest multiplicative figure against 1e-2
        nudge             |l0 + b0| against 1e-8                                   (additive trend)
        level_guard       |intercept + slope| against 1e-8                         (multiplicative trend; below it the value is 1e-7)
        growth_cap        1e10 against |b0|                                        (multiplicative trend)
        fallback          min(l0, b0) against 1e-8                                 (multiplicative trend)
        fallback_level, fallback_growth   first adjusted value / ratio of the first two against 1e-3   (only inside the fallback)"""
    e, t, s = R.parts(notation)
    y = np.asarray(y, dtype=dtype)
    n = len(y)
    if s == "N":
        m = 1                      # a spec without a season has period 1 whatever the batch's period is
    clamps = {}
    fig = None
    adj = y
    if s != "N":
        assert m >= 2 and n >= 2 * m, (m, n)
        raw, fig = seasonal_figure(y, m, s, dtype)
        if s == "M":
            clamps["figure_floor"] = _rel_gap(np.min(raw), dtype(FIGURE_FLOOR))
        phase = np.arange(n) % m
        adj = y - fig[phase] if s == "A" else y / fig[phase]
    if t == "N":
        k = min(n, max(10, 2 * m))
        return {"level": np.mean(adj[:k]), "growth": None, "seasonal": fig, "clamps": clamps}
    time = np.arange(1, n + 1).astype(dtype)
    tc, ac = time - np.mean(time), adj - np.mean(adj)
    slope = np.sum(tc * ac) / np.sum(tc * tc)
    icpt = np.mean(adj) - slope * np.mean(time)
    if t in ("A", "Ad"):
        l0, b0 = icpt, slope
        clamps["nudge"] = _rel_gap(abs(l0 + b0), dtype(NUDGE_BELOW))
        if abs(l0 + b0) < dtype(NUDGE_BELOW):
            l0, b0 = l0 * (dtype(1) + dtype(1.0e-3)), b0 * (dtype(1) - dtype(1.0e-3))
    else:
        l0 = icpt + slope
        clamps["level_guard"] = _rel_gap(abs(l0), dtype(SMALL_STATE))
        if abs(l0) < dtype(SMALL_STATE):
            l0 = dtype(1.0e-7)
        b0 = (icpt + dtype(2) * slope) / l0
        l0 = l0 / b0
        clamps["growth_cap"] = float((dtype(GROWTH_CAP) - abs(b0)) / dtype(GROWTH_CAP))
        if abs(b0) > dtype(GROWTH_CAP):
            b0 = np.sign(b0) * dtype(GROWTH_CAP)
        clamps["fallback"] = _rel_gap(min(l0, b0), dtype(SMALL_STATE))
        if l0 < dtype(SMALL_STATE) or b0 < dtype(SMALL_STATE):
            l0, r = adj[0], adj[1] / adj[0]
            clamps["fallback_level"] = _rel_gap(l0, dtype(FALLBACK_FLOOR))
            clamps["fallback_growth"] = _rel_gap(r, dtype(FALLBACK_FLOOR))
            l0, b0 = max(l0, dtype(FALLBACK_FLOOR)), max(r, dtype(FALLBACK_FLOOR))
    return {"level": l0, "growth": b0, "seasonal": fig, "clamps": clamps}


def replay_many(series, notation, m, alpha, beta, gamma, phi, dtype=np.float64, starts=None):
    """The recursion of spec `notation` over a list of series at once, from start_states (or the given `starts`), with one (alpha, beta,
    gamma, phi) per series in model terms (a NaN where the spec has no such parameter is not read).  Returns a list of
    {"fitted" [n], "level", "trend" (NaN without), "seasonal" ([m], phase-indexed: state of phase t mod m; NaN [m] without),
     "far": the largest |b - 1| a damped multiplicative-trend step raised to phi, "start": the start states}.

    State-space form (tables 2.2 / 2.3): with q = l, l + b, l + phi b, l b, l b^phi and p the trend's part of it (b, phi b, b^phi),
        mu = q, q + s, q s
        additive error        e = y - mu :   l' = q + alpha e           [/ s  with a multiplicative season]
                                             b' = p + beta e            [/ s  with a multiplicative season; / l for a multiplicative trend]
                                             s' = s + gamma e           [/ q  with a multiplicative season]
        multiplicative error  eps = (y - mu) / mu :  l' = q (1 + alpha eps),  b' = p + beta q eps  or  p (1 + beta eps),  s' = s (1 + gamma eps)."""
    e, t, s = R.parts(notation)
    assert not (e == "M" and s == "A"), "not a spec of this project"
    S = len(series)
    one = dtype(1)
    if starts is None:
        starts = [start_states(y, notation, m, dtype) for y in series]
    lens = np.array([len(y) for y in series])
    T = int(lens.max())
    Y = np.ones((S, T), dtype=dtype)
    for i, y in enumerate(series):
        Y[i, : len(y)] = np.asarray(y, dtype=dtype)
    a = np.asarray(alpha, dtype=dtype)
    b_ = np.asarray(beta, dtype=dtype)
    g = np.asarray(gamma, dtype=dtype)
    ph = np.asarray(phi, dtype=dtype) if t in ("Ad", "Md") else np.ones(S, dtype=dtype)
    l = np.array([st["level"] for st in starts], dtype=dtype)
    b = np.array([st["growth"] for st in starts], dtype=dtype) if t != "N" else None
    ring = np.array([st["seasonal"] for st in starts], dtype=dtype) if s != "N" else None
    fitted = np.full((S, T), np.nan, dtype=dtype)
    far = np.zeros(S)
    with np.errstate(all="ignore"):
        for step in range(T):
            live = step < lens
            j = step % m if s != "N" else 0
            if t == "N":
                p, q = None, l
            elif t in ("A", "Ad"):
                p = ph * b
                q = l + p
            else:
                if t == "Md":
                    far = np.where(live, np.maximum(far, np.abs(np.asarray(b - one, dtype=np.float64))), far)
                p = b ** ph
                q = l * p
            sj = ring[:, j] if s != "N" else None
            mu = q if s == "N" else (q + sj if s == "A" else q * sj)
            fitted[:, step] = mu
            yt = Y[:, step]
            if e == "A":
                err = yt - mu
                l_new = q + a * (err if s != "M" else err / sj)
                if t in ("A", "Ad"):
                    b_new = p + b_ * (err if s != "M" else err / sj)
                elif t in ("M", "Md"):
                    b_new = p + b_ * (err / l if s != "M" else err / (sj * l))
                if s == "A":
                    s_new = sj + g * err
                elif s == "M":
                    s_new = sj + g * err / q
            else:
                eps = (yt - mu) / mu
                l_new = q * (one + a * eps)
                if t in ("A", "Ad"):
                    b_new = p + b_ * q * eps
                elif t in ("M", "Md"):
                    b_new = p * (one + b_ * eps)
                if s == "M":
                    s_new = sj * (one + g * eps)
            l = np.where(live, l_new, l)
            if t != "N":
                b = np.where(live, b_new, b)
            if s != "N":
                ring[:, j] = np.where(live, s_new, sj)
    out = []
    for i in range(S):
        out.append({"fitted": fitted[i, : lens[i]].copy(), "level": l[i], "trend": b[i] if t != "N" else dtype(np.nan),
                    "seasonal": ring[i].copy() if s != "N" else np.full(max(m, 1), np.nan, dtype=dtype), "far": float(far[i]),
                    "start": starts[i]})
    return out


def replay(y, notation, m, alpha, beta, gamma, phi, dtype=np.float64):
    """replay_many for one series."""
    return replay_many([y], notation, m, [alpha], [beta], [gamma], [phi], dtype)[0]


def point_forecasts(rep, n, notation, m, phi, h):
    """inspect_ref.forecast on a replay's final states (extended precision whatever format the replay ran in)."""
    rec = {"phi": phi, "level": rep["level"], "trend": rep["trend"], "seasonal_states": rep["seasonal"]}
    return R.forecast(rec, n, notation, m, h)


def intervals(point, y, conf, dtype=np.float64):
    """(lower, upper): point -/+ z sd sqrt(i), i = 1..h, sd the POPULATION standard deviation of the series, z from the five-step table."""
    y = np.asarray(y, dtype=dtype)
    point = np.asarray(point, dtype=dtype)
    sd = np.sqrt(np.mean((y - np.mean(y)) ** 2))
    z = next((dtype(v) for c, v in Z_TABLE if conf >= c), dtype(1))
    w = z * sd * np.sqrt(np.arange(1, len(point) + 1).astype(dtype))
    return point - w, point + w


QUANTITIES = ("fitted", "level", "trend", "seasonal", "point")


def quantities(rep, n, notation, m, phi, h):
    """What a record is compared on: fitted values, level, trend, the m seasonal states and the h point forecasts of a replay."""
    e, t, s = R.parts(notation)
    q = {"fitted": rep["fitted"], "level": rep["level"], "point": point_forecasts(rep, n, notation, m, phi, h)}
    if t != "N":
        q["trend"] = rep["trend"]
    if s != "N":
        q["seasonal"] = rep["seasonal"]
    return q


def noise(q64, q80):
    """The series' own conditioning: the largest deviation |a - b| / max(1, |b|) between the float64 and the longdouble evaluation of
    the same quantities."""
    return max(R.dev(q64[k], q80[k]) for k in q80)


def deviation(got, q80):
    """Largest deviation of a record's quantities (a dict with the keys of `quantities`) from the extended-precision replay's."""
    return max(R.dev(got[k], q80[k]) for k in q80)
