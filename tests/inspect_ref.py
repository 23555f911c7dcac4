"""High-precision identities of an ETS inspection record (anofox_hip_batch_inspect / oracle.ets_inspect), independent of
oracle/: what either side calls SSE, AIC / AICc / BIC and "final states" must BE those things.  Plain numpy in np.longdouble
(80-bit), textbook formulas (Hyndman, Koehler, Ord & Snyder 2008, tables 2.1 and 2.2), nothing of the operation order of the
kernels or of oracle/ets.c.

A record is a dict with alpha, beta, gamma, phi, aic, aicc, bic, sse, level, trend, seasonal_states and fitted_values; `y` is the
cleaned series (NULLs interpolated) and `notation` the spec ("AAdA", "MNM", ...).  Deviations are returned under the project's
measure |a - b| / max(1, |b|) with b the high-precision value.
"""
from __future__ import annotations

import numpy as np

LD = np.longdouble
TRENDS = ("N", "A", "Ad", "M", "Md")
SPECS = ("ANN", "AAN", "AAdN", "ANA", "AAA", "AAdA", "MNN", "MAN", "MAdN", "MMN", "MMdN", "AMN", "AMdN",
         "ANM", "AAM", "AAdM", "AMA", "AMdA", "AMM", "AMdM", "MNM", "MAM", "MAdM", "MMM", "MMdM")
SCALARS = ("alpha", "beta", "gamma", "phi", "aic", "aicc", "bic", "sse", "level", "trend")


def parts(notation):
    """("A" | "M", "N" | "A" | "Ad" | "M" | "Md", "N" | "A" | "M")"""
    return notation[0], notation[1:-1], notation[-1]


def spec_id(notation):
    """error * 15 + trend index * 3 + season (oracle/forecast.c spec_from_id; model_code of AutoETS = 100 + this)."""
    e, t, s = parts(notation)
    return "AM".index(e) * 15 + TRENDS.index(t) * 3 + "NAM".index(s)


def notation_of(sid):
    return "AM"[sid // 15] + TRENDS[(sid % 15) // 3] + "NAM"[sid % 3]


_LETTER = {"Additive": "A", "Multiplicative": "M", "None": "N", "AdditiveDamped": "Ad", "MultiplicativeDamped": "Md"}


def notation_of_name(name):
    """"AutoETS(Additive,AdditiveDamped,None)" -> "AAdN"; None for a name without a spec (the fallback chain)."""
    if "(" not in name or not name.endswith(")"):
        return None
    inner = name[name.find("(") + 1:-1].split(",")
    return "".join(_LETTER[p] for p in inner) if len(inner) == 3 and all(p in _LETTER for p in inner) else None


def dev(a, b):
    """|a - b| / max(1, |b|), the worst over the elements; a value that is not a number on either side is a mismatch."""
    a, b = np.atleast_1d(np.asarray(a, dtype=LD)), np.atleast_1d(np.asarray(b, dtype=LD))
    if a.shape != b.shape:
        return float("inf")
    if a.size == 0:
        return 0.0
    d = np.abs(a - b) / np.maximum(LD(1), np.abs(b))
    d[~np.isfinite(d)] = np.inf
    return float(np.max(d))


def n_param(notation, m):
    """k = 3 + 2 [trend] + m [season] + [damped]: the smoothing parameters, the start states (m - 1 free seasonal ones) and sigma."""
    e, t, s = parts(notation)
    return 3 + 2 * (t != "N") + (m if s != "N" else 0) + (t in ("Ad", "Md"))


def sse(rec, y, notation):
    """sum e_t^2, e = y - fitted for an additive error and (y - fitted) / fitted for a multiplicative one."""
    y = np.asarray(y, dtype=LD)
    f = np.asarray(rec["fitted_values"], dtype=LD)[: len(y)]
    e = y - f
    if notation[0] == "M":
        e = e / f
    return np.sum(e * e)


def criteria(rec, y, notation, m):
    """(aic, aicc, bic) from the record's own fitted values: lik = n log SSE (+ 2 sum log|fitted| for a multiplicative error)."""
    n = LD(len(y))
    k = LD(n_param(notation, m))
    lik = n * np.log(sse(rec, y, notation))
    if notation[0] == "M":
        lik = lik + LD(2) * np.sum(np.log(np.abs(np.asarray(rec["fitted_values"], dtype=LD)[: len(y)])))
    aic = lik + LD(2) * k
    return aic, aic + LD(2) * k * (k + LD(1)) / (n - k - LD(1)), lik + k * np.log(n)


def components(rec, n, notation, m, h):
    """The forecast function taken apart: (level [h], trend [h] or None, seasonal [h] or None) for steps 1..h from the final states.
    damp_i = phi + ... + phi^i (i when undamped); trend contribution damp_i b (A / Ad) or b^damp_i (M / Md); seasonal state of phase
    (n + i - 1) % m."""
    e, t, s = parts(notation)
    phi = LD(rec["phi"]) if t in ("Ad", "Md") else LD(1)
    damp = np.cumsum(phi ** np.arange(1, h + 1, dtype=LD))
    level = np.full(h, LD(rec["level"]))
    trend = None
    if t in ("A", "Ad"):
        trend = damp * LD(rec["trend"])
    elif t in ("M", "Md"):
        trend = LD(rec["trend"]) ** damp
    seasonal = None
    if s != "N":
        st = np.asarray(rec["seasonal_states"], dtype=LD)
        seasonal = np.array([st[(n + i - 1) % m] for i in range(1, h + 1)], dtype=LD)
    return level, trend, seasonal


def forecast(rec, n, notation, m, h):
    """Textbook point forecasts of steps 1..h from the record's final states."""
    e, t, s = parts(notation)
    level, trend, seasonal = components(rec, n, notation, m, h)
    f = level
    if t in ("A", "Ad"):
        f = level + trend
    elif t in ("M", "Md"):
        f = level * trend
    if s == "A":
        f = f + seasonal
    elif s == "M":
        f = f * seasonal
    return f


def component_rule(rec, notation, m):
    """beta, gamma, phi, trend and the seasonal states are NaN exactly where the spec has no such component; everything else is
    finite.  Returns the list of fields that break the rule (empty: the rule holds)."""
    e, t, s = parts(notation)
    want_nan = {"beta": t == "N", "trend": t == "N", "gamma": s == "N", "phi": t not in ("Ad", "Md")}
    bad = [k for k, nan in want_nan.items() if bool(np.isnan(rec[k])) != nan]
    bad += [k for k in SCALARS if k not in want_nan and not np.isfinite(rec[k])]
    st = np.asarray(rec["seasonal_states"], dtype=np.float64)
    if s == "N":
        if not np.all(np.isnan(st)):
            bad.append("seasonal_states")
    elif len(st) != m or not np.all(np.isfinite(st)):
        bad.append("seasonal_states")
    return bad


def identities(rec, y, notation, m, point):
    """The three identities of one record: deviations {"sse", "criteria", "forecast"} (`point`: the run's own forecasts)."""
    aic, aicc, bic = criteria(rec, y, notation, m)
    return {"sse": dev(rec["sse"], sse(rec, y, notation)),
            "criteria": max(dev(rec["aic"], aic), dev(rec["aicc"], aicc), dev(rec["bic"], bic)),
            "forecast": dev(point, forecast(rec, len(y), notation, m, len(point)))}


def parameter_rule(rec, notation):
    """The parameters are in MODEL terms: 0 < alpha < 1, 0 <= beta <= alpha (= alpha beta*), 0 <= gamma <= 1 - alpha
    (= gamma* (1 - alpha)), 0 < phi <= 1.  Returns the fields outside their region."""
    e, t, s = parts(notation)
    a = rec["alpha"]
    bad = [] if 0.0 < a < 1.0 else ["alpha"]
    if t != "N" and not 0.0 <= rec["beta"] <= a:
        bad.append("beta")
    if s != "N" and not 0.0 <= rec["gamma"] <= 1.0 - a:
        bad.append("gamma")
    if t in ("Ad", "Md") and not 0.0 < rec["phi"] <= 1.0:
        bad.append("phi")
    return bad


def arima_criteria(aicc, k, n):
    """(aic, bic) of an AutoARIMA fit from its AICc: aicc = aic + 2 k (k + 1) / (n - k - 1), bic = aic - 2 k + k log n, with
    k = p + q + P + Q + constant + 1 and n the observations the criterion was computed over."""
    k, n = LD(k), LD(n)
    aic = LD(aicc) - LD(2) * k * (k + LD(1)) / (n - k - LD(1))
    return aic, aic - LD(2) * k + k * np.log(n)
