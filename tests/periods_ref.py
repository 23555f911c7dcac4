"""numpy restatement of the reference's lomb_scargle, aic_comparison, sazed_period and detect_periods_with_validation
(crates/anofox-fcst-core/src/periods.rs:522-644, 660-786, 1259-1361, 1385-1520, 1651-1686, 1741-1758) -- the checker of the GPU
period detection.

Every sum keeps the source's order of additions: the code is vectorised ACROSS frequencies / candidates / bins and walks t in a
Python loop, so each frequency's sums grow element by element as in the source; the mean and the sums of squares are sequential
(np.cumsum), never numpy's pairwise np.sum.

Each function has two evaluations.  `exact=False` is the source in float64, its own argument arithmetic included.  `exact=True`
evaluates the same grid (the float64 frequencies, candidates and bins: the decisions are about the same points) in np.longdouble
with a longdouble pi, and SAZED's phase as the exact integer (k t) mod L.  The distance between the two is the trig noise of the
problem: how far two correct evaluations of the source's formulas may lie apart because sin / cos, their arguments and the sums
are rounded differently.  `contract()` turns it into the tolerance and the decision margins that tests/test_periods_cpu.py checks
and tests/test_gpu_periods.py applies."""
import math

import numpy as np

EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble
PI_LD = 4 * np.arctan(LD(1))
METHOD_ALIASES = {
    "fft": "fft", "periodogram": "fft", "acf": "acf", "autocorrelation": "acf", "regression": "regression", "fourier": "regression",
    "multi": "multi", "multiple": "multi", "auto": "auto", "autoperiod": "autoperiod", "ap": "autoperiod", "cfd": "cfd_autoperiod",
    "cfdautoperiod": "cfd_autoperiod", "cfd_autoperiod": "cfd_autoperiod", "lombscargle": "lomb_scargle", "lomb_scargle": "lomb_scargle",
    "lomb-scargle": "lomb_scargle", "ls": "lomb_scargle", "aic": "aic", "aic_comparison": "aic", "ssa": "ssa", "singular_spectrum": "ssa",
    "stl": "stl", "stl_period": "stl", "seasonal_trend": "stl", "matrix_profile": "matrix_profile", "matrixprofile": "matrix_profile",
    "mp": "matrix_profile", "sazed": "sazed", "zero_padded": "sazed", "enhanced_dft": "sazed"}
IMPLEMENTED = ("lomb_scargle", "aic", "sazed")
NEEDED = {"lomb_scargle": 4, "aic": 8, "sazed": 16}


class InsufficientData(Exception):
    def __init__(self, needed, got):
        super().__init__(f"Insufficient data: need at least {needed} observations, got {got}")
        self.needed, self.got = needed, got


def parse_method(s):
    """PeriodMethod::from_str: case-insensitive, aliases, an unknown string is fft."""
    return METHOD_ALIASES.get("fft" if s is None else str(s).lower(), "fft")


def _seq(x):
    return float(np.cumsum(np.asarray(x, dtype=np.float64))[-1])


def _div(a, b):
    """IEEE division of floats (x / 0 is inf or NaN, as in Rust)."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def lomb_scargle(values, min_period=None, max_period=None, n_frequencies=None, exact=False):
    v = np.asarray(values, dtype=np.float64)
    n = len(v)
    if n < 4:
        raise InsufficientData(4, n)
    mean = _seq(v) / n
    variance = _seq((v - mean) * (v - mean)) / n
    if abs(variance) < EPS:
        return {"period": math.nan, "frequency": math.nan, "power": 0.0, "false_alarm_prob": 1.0, "method": "lomb_scargle", "index": -1,
                "powers": np.zeros(0)}
    y = v - mean
    t_span = float(n - 1) - 0.0
    min_p = 2.0 if min_period is None else float(min_period)
    max_p = t_span / 2.0 if max_period is None else float(max_period)
    n_freq = 1000 if n_frequencies is None else int(n_frequencies)
    min_freq, max_freq = 1.0 / max_p, 1.0 / min_p
    step = _div(max_freq - min_freq, float(n_freq - 1))
    with np.errstate(all="ignore"):
        freq = min_freq + np.arange(n_freq, dtype=np.float64) * step
        F = LD if exact else np.float64
        omega = (2 * PI_LD * freq.astype(LD)) if exact else 2.0 * np.pi * freq
        s2 = np.zeros(n_freq, dtype=F)
        c2 = np.zeros(n_freq, dtype=F)
        for t in range(n):
            arg = 2.0 * omega * F(t)
            s2 += np.sin(arg)
            c2 += np.cos(arg)
        tau = np.arctan2(s2, c2) / (2.0 * omega)
        cs_sum = np.zeros(n_freq, dtype=F)
        sn_sum = np.zeros(n_freq, dtype=F)
        cs2 = np.zeros(n_freq, dtype=F)
        sn2 = np.zeros(n_freq, dtype=F)
        for t in range(n):
            arg = omega * (F(t) - tau)
            cv, sv = np.cos(arg), np.sin(arg)
            cs_sum += F(y[t]) * cv
            sn_sum += F(y[t]) * sv
            cs2 += cv * cv
            sn2 += sv * sv
        power = np.where((np.abs(cs2) > EPS) & (np.abs(sn2) > EPS), 0.5 * (cs_sum * cs_sum / cs2 + sn_sum * sn_sum / sn2) / F(variance), F(0.0))
    best_power, best_freq, best_i = 0.0, 0.0, -1
    for i in range(n_freq):
        if power[i] > best_power:
            best_power, best_freq, best_i = power[i], float(freq[i]), i
    if best_power > 0.0:
        prob_single = math.exp(-float(best_power))
        fap = 1.0 - (1.0 - prob_single) ** float(n_freq)
    else:
        fap = 1.0
    return {"period": 1.0 / best_freq if best_freq > 0.0 else math.nan, "frequency": best_freq, "power": best_power,
            "false_alarm_prob": 1.0 if fap != fap else min(fap, 1.0), "method": "lomb_scargle", "index": best_i, "powers": power}


def aic_comparison(values, min_period=None, max_period=None, n_candidates=None, exact=False):
    v = np.asarray(values, dtype=np.float64)
    n = len(v)
    if n < 8:
        raise InsufficientData(8, n)
    min_p = 2.0 if min_period is None else float(min_period)
    max_p = n / 2.0 if max_period is None else float(max_period)
    n_cand = 50 if n_candidates is None else int(n_candidates)
    step = _div(max_p - min_p, float(n_cand - 1))
    k = 3.0
    mean = _seq(v) / n
    ss_total = _seq((v - mean) * (v - mean))
    F = LD if exact else np.float64
    with np.errstate(all="ignore"):
        cand = min_p + np.arange(n_cand, dtype=np.float64) * step
        omega = (2 * PI_LD / cand.astype(LD)) if exact else 2.0 * np.pi / cand
        syc = np.zeros(n_cand, dtype=F)
        sys_ = np.zeros(n_cand, dtype=F)
        sc2 = np.zeros(n_cand, dtype=F)
        ss2 = np.zeros(n_cand, dtype=F)
        for t in range(n):
            ang = omega * F(t)
            cv, sv = np.cos(ang), np.sin(ang)
            syc += F(v[t] - mean) * cv
            sys_ += F(v[t] - mean) * sv
            sc2 += cv * cv
            ss2 += sv * sv
        a = np.where(np.abs(sc2) > EPS, syc / sc2, F(0.0))
        b = np.where(np.abs(ss2) > EPS, sys_ / ss2, F(0.0))
        rss = np.zeros(n_cand, dtype=F)
        for t in range(n):
            ang = omega * F(t)
            fitted = F(mean) + a * np.cos(ang) + b * np.sin(ang)
            d = F(v[t]) - fitted
            rss += d * d
        aic = np.where(rss > 0.0, F(n) * np.log(rss / F(n)) + F(2.0 * k), F(-np.inf))
    best_aic, best_i, best_rss = math.inf, 0, 0.0
    for i in range(n_cand):
        if aic[i] < best_aic:
            best_aic, best_i, best_rss = aic[i], i, rss[i]
    with np.errstate(all="ignore"):
        bic = F(n) * np.log(F(best_rss) / F(n)) + F(k) * np.log(F(n))
    r2 = 1.0 - best_rss / F(ss_total) if ss_total > 0.0 else 0.0
    return {"period": float(cand[best_i]), "aic": best_aic, "bic": bic, "rss": best_rss, "r_squared": r2, "method": "aic", "index": best_i,
            "aics": aic, "rsss": rss, "ss_total": ss_total}


def sazed_period(values, padding_factor=None, min_period=None, max_period=None, exact=False):
    v = np.asarray(values, dtype=np.float64)
    n = len(v)
    if n < 16:
        raise InsufficientData(16, n)
    pad = max(4 if padding_factor is None else int(padding_factor), 1)
    L = 1
    while L < n * pad:
        L *= 2
    mean = _seq(v) / n
    window = 0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(n, dtype=np.float64) / float(n - 1)))
    x = (v - mean) * window
    half = L // 2
    F = LD if exact else np.float64
    ks = np.arange(half, dtype=np.int64)
    re = np.zeros(half, dtype=F)
    im = np.zeros(half, dtype=F)
    for t in range(n):                                  # the padded tail adds exact zeros: the sum may stop at n
        if exact:
            ang = -2 * PI_LD * ((ks * t) % L).astype(LD) / LD(L)
        else:
            ang = -2.0 * np.pi * ks.astype(np.float64) * float(t) / float(L)
        re += F(x[t]) * np.cos(ang)
        im += F(x[t]) * np.sin(ang)
    spec = (re * re + im * im) / F(L)
    spec[0] = 0.0
    min_p = max(2 if min_period is None else int(min_period), 2)
    max_p = min(n // 2 if max_period is None else int(max_period), n // 2)
    k_min, k_max = L // max_p, L // min_p
    lo, hi = max(k_min, 1), min(k_max, half)
    peaks = []
    for k in range(lo, hi):
        p = spec[k]
        period = float(L) / float(k)
        is_peak = (k == 1 or p > spec[k - 1]) and (k + 1 >= half or p > spec[k + 1])
        if is_peak and min_p <= period <= max_p:
            peaks.append((k, p))
    peaks.sort(key=lambda kp: -kp[1])                   # stable: ties keep the ascending k
    in_range = np.sort(spec[lo:hi], kind="stable") if hi > lo else np.zeros(0, dtype=F)
    noise = in_range[len(in_range) // 2] if len(in_range) else F(1.0)
    if peaks:
        k, p = peaks[0]
        res = {"period": float(L) / float(k), "power": p, "snr": p / noise if noise > 0.0 else p, "index": k}
    else:
        res = {"period": math.nan, "power": 0.0, "snr": 0.0, "index": -1}
    res.update(method="sazed", spec=spec, peaks=peaks, noise=noise, lo=lo, hi=hi, padded_len=L)
    return res


def run(method, values, exact=False, **kw):
    if method == "lomb_scargle":
        return lomb_scargle(values, kw.get("min_period"), kw.get("max_period"), kw.get("n_frequencies"), exact)
    if method == "aic":
        return aic_comparison(values, kw.get("min_period"), kw.get("max_period"), kw.get("n_candidates"), exact)
    return sazed_period(values, kw.get("zero_pad_factor"), kw.get("min_period"), kw.get("max_period"), exact)


def confidence_strength(method, r):
    if method == "lomb_scargle":
        return 1.0 - float(r["false_alarm_prob"]), float(r["power"])
    if method == "aic":
        return float(r["r_squared"]), float(r["r_squared"])
    snr = float(r["snr"])
    return (1.0 if snr != snr else min(snr, 1.0)), float(r["power"])


def validate_period(detected, expected, tolerance):
    best = None
    for e in expected or []:
        if e <= 0.0:
            continue
        dev = abs(detected - e) / e
        if dev <= tolerance and (best is None or dev < best[1]):
            best = (e, dev)
    return (True, best[0], best[1]) if best else (False, None, None)


def detect_periods_with_validation(values, method, max_period=None, min_confidence=None, expected_periods=None, tolerance=None, exact=False):
    """For the three methods; `method` is a string as the FFI gets it.  max_period is accepted and not used (periods.rs:1651, 1669,
    1741 call the methods with their own defaults).  Returns periods (list of dicts), primary_period, method."""
    m = parse_method(method)
    if m not in IMPLEMENTED:
        raise NotImplementedError(m)
    r = run(m, values, exact)
    conf, strength = confidence_strength(m, r)
    one = {"period": float(r["period"]), "confidence": conf, "strength": strength, "amplitude": 0.0, "phase": 0.0, "iteration": 1,
           "matches_expected": False, "matched_expected_period": None, "match_deviation": None}
    periods, primary, name = [one], float(r["period"]), m
    threshold = 0.3 if min_confidence is None else min_confidence
    if threshold > 0.0:
        periods = [p for p in periods if p["confidence"] >= threshold]
        if not periods:
            return {"periods": [], "primary_period": 0.0, "method": f"{name} (no seasonality)", "raw": r}
        primary = periods[0]["period"]
    if expected_periods:
        tol = 0.1 if tolerance is None else tolerance
        for p in periods:
            p["matches_expected"], p["matched_expected_period"], p["match_deviation"] = validate_period(p["period"], expected_periods, tol)
    return {"periods": periods, "primary_period": primary, "method": name, "raw": r}


def contract(method, values, **kw):
    """The tolerance and the decision margins of one (method, series, parameters) problem.

    noise: the largest |float64 - longdouble| over the whole grid (powers; for AIC the RSS), relative to the peak power (the best
    RSS).  tol = max(1e-12, 16 noise), the factor and the floor of stats_ref.noise_table.  gap: the smallest relative distance of a
    decision from flipping -- best against runner-up power (AIC: best against runner-up AIC, as a change of RSS: an AIC moves by
    n d(rss) / rss); for SAZED also the top peak against its two neighbours.  The confidence must keep 1,000 times its own
    tolerance (figure_tolerances) away from the 0.3 threshold.  SAZED's median needs no margin of its own: an order statistic moves by no more than the largest change of any
    power, so a different element of (nearly) the same value changes the noise floor by no more than the tolerance allows.
    `ok` is gap > 1000 tol: a correct evaluation then cannot pick another point.  A problem without a decision (constant series,
    no peak, a NaN grid) has gap = inf."""
    a, b = run(method, values, False, **kw), run(method, values, True, **kw)
    out = {"ref": a, "exact": b, "noise": 0.0, "gap": math.inf}
    if a["index"] != b["index"]:
        out.update(noise=math.inf, tol=math.inf, gap=0.0, ok=False)
        return out
    if a["index"] < 0 or (method == "aic" and not math.isfinite(float(a["aic"]))):
        out.update(tol=1e-12, ok=True, scale=0.0)
        return out
    with np.errstate(all="ignore"):
        if method == "lomb_scargle":
            pa, pb = np.asarray(a["powers"], dtype=LD), np.asarray(b["powers"], dtype=LD)
            scale = float(b["power"])
            noise = float(np.nanmax(np.abs(pa - pb))) / scale
            others = np.delete(pa, a["index"])
            others = others[np.isfinite(others)]
            gap = (float(a["power"]) - float(others.max())) / scale if len(others) else math.inf
        elif method == "aic":
            ra, rb = np.asarray(a["rsss"], dtype=LD), np.asarray(b["rsss"], dtype=LD)
            scale = float(b["rss"])
            noise = float(np.nanmax(np.abs(ra - rb))) / scale
            aics = np.asarray(a["aics"], dtype=np.float64)
            others = np.delete(aics, a["index"])
            others = others[np.isfinite(others)]
            gap = (float(others.min()) - float(a["aic"])) / len(values) if len(others) else math.inf
        else:
            sa, sb = np.asarray(a["spec"], dtype=LD), np.asarray(b["spec"], dtype=LD)
            scale = float(b["power"])
            noise = float(np.max(np.abs(sa - sb))) / scale
            k = a["index"]
            near = [float(a["spec"][j]) for j in (k - 1, k + 1) if 1 <= j < len(sa)]
            rest = [float(p) for kk, p in a["peaks"][1:]]
            gap = min([(float(a["power"]) - q) / scale for q in near + rest] or [math.inf])
    tol = max(1e-12, 16.0 * noise)
    conf, _ = confidence_strength(method, a)
    conf_tol = confidence_tolerance(method, a, tol)
    conf_ok = abs(conf - 0.3) > 1000.0 * conf_tol
    if method == "sazed" and float(a["snr"]) > 1.0 + 1000.0 * conf_tol:
        conf_ok = True                                   # min(snr, 1) is 1.0 exactly on both sides
    out.update(noise=noise, tol=tol, gap=gap, scale=scale, conf_margin=abs(conf - 0.3), conf_tol=conf_tol,
               ok=gap > 1000.0 * tol and conf_ok)
    return out


def confidence_tolerance(method, r, tol):
    return figure_tolerances(method, r, tol)[{"lomb_scargle": "false_alarm_prob", "aic": "r_squared", "sazed": "snr"}[method]]


def figure_tolerances(method, r, tol, n=None):
    """Absolute tolerance of every float figure, from `tol` (relative to the peak power / the best RSS) by error propagation.
    Lomb-Scargle: fap = 1 - (1 - e^-z)^M has |d fap / dz| <= 1 / e for every z and M.  AIC: aic and bic move by n d(rss) / rss,
    r_squared by d(rss) / ss_total <= tol; a few ulps of the figure itself are added for ln.  SAZED: snr = power / noise with both
    off by tol * power at most."""
    ulps = 8 * EPS
    if method == "lomb_scargle":
        p = float(r["power"])
        return {"power": tol * p, "false_alarm_prob": tol * max(p, 1.0) + ulps}
    if method == "aic":
        n = float(n if n is not None else 1)
        rss = float(r["rss"])
        return {"rss": tol * rss, "aic": n * tol + ulps * abs(float(r["aic"])), "bic": n * tol + ulps * abs(float(r["bic"])),
                "r_squared": tol + ulps}
    p, noise = float(r["power"]), float(r.get("noise", 1.0))
    snr = float(r["snr"])
    rel = tol + (tol * p / noise if noise > 0.0 else 0.0)
    return {"power": tol * p, "snr": rel * abs(snr) + ulps * abs(snr)}
