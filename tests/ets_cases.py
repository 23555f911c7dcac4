"""Inputs and bookkeeping of the ETS replay tests, shared by tests/test_ets_cpu.py (the oracle's records against the restatement of
tests/ets_ref.py) and tests/test_gpu_ets_replay.py (the kernels' records against it).  Shapes are the smallest that still reach each
branch of prep.hip and of the recursion: see the docstring of each family.

Tolerance of ONE series: max(REL_TOL, F x noise), noise = the deviation between the float64 and the 80-bit evaluation of the
restatement on that series (ets_ref.noise) -- its own conditioning; a multiplicative trend whose level passes near zero loses digits in
ANY float64 evaluation.  F was measured on the oracle and the restatement, never on the kernels (test_ets_cpu.py prints the ratios).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import ets_ref as E
import inspect_cases as K
import inspect_ref as R
from anofox_forecast_amd import synth

REL_TOL = K.REL_TOL
# (oracle deviation from the 80-bit replay) / (the replay's own float64-to-80-bit noise), largest over every series of every case below
# whose noise exceeds 1e-15, times a margin of 4.  Measured: 35.40 (deviation 4.7e-14 over noise 1.3e-15: AMA at given parameters, series
# 61 of the m = 7 straight-line wave; next 24.5, MAM fitted; the series above the 1e-12 floor -- all of them multiplicative trends
# under an additive season, deviation up to 5.7e-8 -- have ratios of 0.8 to 5).  test_ets_cpu.py::test_the_factor_covers_every_case
# measures it again over all cases.
MEASURED_RATIO = 35.40
F = 4.0 * MEASURED_RATIO
QUIET_NOISE = 1.0e-13            # at least three quarters of a fitted family are at or below this: held at the REL_TOL floor
WORST_NOISE = 1.0e-6             # no series is above this
CLAMP_MARGIN = 1.0e-6            # every series keeps this relative distance from every start-state clamp, on its intended side
CONFIDENCES = (0.80, 0.90, 0.95, 0.99)

# parameters of the fixed-parameter prep and clamp cases: beta / alpha = 1/4 and gamma / (1 - alpha) = 1/2 are exact, so the entry's
# optimiser coordinates (alpha, beta / alpha, gamma / (1 - alpha)) give back exactly these numbers in model terms
PREP_PARAMS = (0.25, 0.0625, 0.375, 1.0)
PREP_SPECS = ("ANA", "AAA", "AMA", "MNM", "MAM", "MMM")      # additive / multiplicative figure x level-only / additive / multiplicative start
# anofox_hip_batch_set_fixed_params admits 0 < alpha < 1, 0 <= beta <= alpha, 0 <= gamma <= 1 - alpha, 0 < phi <= 1: both ends of alpha
# are open (2^-20 from each: far outside the optimiser's box [1e-4, 0.9999]), beta and gamma ON their upper bounds, phi at the smallest
# positive double and at 1
ALPHA_ENDS = (2.0 ** -20, 1.0 - 2.0 ** -20)
PHI_ENDS = (float.fromhex("0x1p-1074"), 1.0)
CORNER_SPECS = ("AAdA", "AAdM", "MMdM")                       # additive class, general class, damped multiplicative trend
POW_NEAR1_R = 1.0 / 16.0         # |b - 1| up to this: b^phi by the binomial series; beyond: the table-driven power


def positive_series(seed, count, T, m, sd=0.1):
    """`count` strictly positive real-valued series [count, T]: level 20..200, a seasonal profile of period m, a slow trend, lognormal noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(T)
    level = rng.uniform(20.0, 200.0, size=(count, 1))
    prof = 1.0 + 0.3 * np.sin(2.0 * np.pi * (t % max(m, 1))[None, :] / max(m, 1) + rng.uniform(0.0, 2.0 * np.pi, size=(count, 1)))
    trend = 1.0 + 0.4 * t[None, :] / T * rng.uniform(-0.5, 1.0, size=(count, 1))
    return level * prof * trend * np.exp(rng.normal(0.0, sd, size=(count, T)))


def _ragged(Y, lens):
    return [Y[s, :n].copy() for s, n in enumerate(lens)]


def _case(series, m, runs, clamp=None, h=None):
    return {"series": series, "m": m, "h": h if h is not None else min(2 * m + 3, 31), "runs": list(runs), "clamp": clamp}


def _prep(series, m, specs=PREP_SPECS, **kw):
    return _case(series, m, [(spec, PREP_PARAMS) for spec in specs], **kw)


def fixed_cases():
    """{name: case}: every batch that runs with GIVEN parameters (one pass: what the record holds is start states + recursion).
    case = {"series", "m", "h", "runs": [(spec, (alpha, beta, gamma, phi))], "clamp": None or the start-state clamp hit on purpose}."""
    if "fixed" in _REFS:
        return _REFS["fixed"]
    c = {}
    # ---- parameter corners no optimiser run reaches: 6 series of 40..45 observations, m = 7
    Y = positive_series(9100, 6, 45, 7, sd=0.2)
    for spec in CORNER_SPECS:
        c[f"corner-{spec}"] = _case(_ragged(Y, [45 - s for s in range(6)]), 7,
                                    [(spec, (a, a, 1.0 - a, phi)) for a in ALPHA_ENDS for phi in PHI_ENDS])
    # ---- m = 7, the register sweep: blocks of 21 rows, straight-line once every series of the wave covers the block, gated otherwise
    Y = positive_series(9200, 64, 101, 7)
    c["m7-straight"] = _prep(_ragged(Y, [63 + (5 * s + s // 9) % 39 for s in range(64)]), 7)      # shortest 63: blocks 2 and 3 straight-line
    c["m7-one-of-14"] = _prep(_ragged(Y[7:8], [14]), 7)                                            # every block gated
    c["m7-block-edges"] = _prep(_ragged(Y[8:16], [14, 15, 41, 42, 43, 62, 63, 64]), 7)
    c["m7-edge-wave"] = _prep(_ragged(Y[16:22], [62, 63, 64, 83, 84, 85]), 7)                      # block 2 straight-line, block 3 gated
    # a strictly positive series beside two with a zero (one in the first block, one in a straight-line block): the multiplicative
    # specs refuse those two, the wave goes on computing the multiplicative figure for the first
    Yz = Y[22:25, :70].copy()
    Yz[1, 5] = 0.0
    Yz[2, 30] = 0.0
    c["m7-with-zeros"] = _prep(_ragged(Yz, [70, 66, 63]), 7, ("AAA", "MAM", "MNM"))
    # ---- every other period: season_figures_kernel (series in LDS) + the generic sweep; n = 2 m and 2 m + 1; K = max(10, 2 m) against n
    for m in (2, 4, 12, 24, 3, 5):
        Y = positive_series(9300 + m, 5, 7 * m + 2, m)
        c[f"m{m}"] = _prep(_ragged(Y, [2 * m, 2 * m + 1, 5 * m + 3, 7 * m + 2, 7 * m + 1]), m)
    c["m2-short"] = _prep(_ragged(positive_series(9400, 3, 9, 2), [7, 8, 9]), 2, ("ANA", "MNM"))  # max(10, 2 m) = 10 exceeds n
    c["m3-short"] = _prep(_ragged(positive_series(9401, 2, 9, 3), [8, 9]), 3, ("ANA", "MNM"))
    c["m300"] = _prep(_ragged(positive_series(9500, 2, 640, 300), [640, 601]), 300, h=9)          # the phase loop strides past 256 threads
    c["scratch"] = _prep(_ragged(positive_series(9600, 4, 6200, 12, sd=0.05), [6200, 6199, 6150, 6001]), 12, ("AAA", "MAM"), h=9)
    # ---- the start-state clamps, each hit on purpose
    t = np.arange(56)
    Y = positive_series(9700, 3, 56, 7, sd=0.02)
    Y[:, t % 7 == 3] *= 1.0e-3                                                   # one weekday at a thousandth: its figure is floored at 1e-2
    c["clamp-figure-floor"] = _prep(_ragged(Y, [56, 50, 44]), 7, ("MNM", "MAM", "AAM"), clamp="figure_floor")
    # an exponentially RISING series: the least-squares line is negative at t = 1, so l0 / b0 < 1e-8 and the first two adjusted values
    # take over (a falling positive series cannot get there: its line is positive at t = 1 and t = 2)
    t = np.arange(24)
    prof = np.array([1.0, 1.2, 0.9, 0.9])[t % 4]
    Y = np.stack([np.exp(t / 3.0) * prof * (1.0 + 0.01 * np.cos(1.7 * t + k)) for k in range(2)])
    c["clamp-fallback"] = _prep(_ragged(Y, [24, 21]), 4, ("AMM", "MMM"), clamp="fallback")
    c["clamp-fallback-flat"] = _case(_ragged(Y / prof, [24, 21]), 1, [("AMN", PREP_PARAMS), ("MMN", PREP_PARAMS), ("AMdN", (0.25, 0.0625, 0.0, 0.9))],
                                     clamp="fallback")
    # y = t - 1 plus second differences (orthogonal to 1 and t): intercept + slope = 0 up to rounding, far inside |l0 + b0| < 1e-8
    y = np.arange(30.0)
    for k, a in ((3, 0.4), (11, -0.7), (20, 0.3)):
        y[k:k + 3] += a * np.array([1.0, -2.0, 1.0])
    c["clamp-nudge"] = _case([y, y[:23].copy()], 1, [("AAN", PREP_PARAMS), ("AAdN", (0.25, 0.0625, 0.0, 0.9))], clamp="nudge")
    for case in c.values():
        for y in case["series"]:
            y.setflags(write=False)
    _REFS["fixed"] = c
    return c


def auto_case():
    """AutoETS at m = 7 (multiplicative-season candidates in the batch, so the sweep may compute their figure): one wave whose 64 series
    all have a zero in their first block of 21 rows -- the multiplicative figure is switched off for the wave from the second block on --
    then a wave of 6 that mixes such series with strictly positive ones.  Lengths 63..92.  Returns (series, horizon)."""
    if "auto" not in _REFS:
        Yz = synth.gen_series(synth.SEED_M5, 9800, 70, 92, 7, positive=True)
        Yp = synth.gen_series(synth.SEED_M5, 9900, 70, 92, 7, positive=True)
        rows = []
        for s in range(70):
            positive = s >= 64 and s % 2 == 0
            y = (Yp if positive else Yz)[s].copy()
            if not positive:
                y[(3 * s) % 21] = 0.0
            rows.append(y[: 63 + (7 * s) % 30])
        for y in rows:
            y.setflags(write=False)
        _REFS["auto"] = (rows, 17)
    return _REFS["auto"]


# ---- the oracle's record at given parameters (oracle/ets.h through ctypes: ets_init_states, ets_fit_fixed, ets_lik + its fitted-value hook)

class EtsSpec(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("error", "trend", "damped", "season", "m")]


class EtsFit(C.Structure):
    _fields_ = [("status", C.c_int), ("dim", C.c_int), ("par", C.c_double * 4), ("alpha", C.c_double), ("beta_star", C.c_double),
                ("gamma_star", C.c_double), ("phi", C.c_double), ("l0", C.c_double), ("b0", C.c_double), ("lik", C.c_double),
                ("sse", C.c_double), ("aic", C.c_double), ("aicc", C.c_double), ("bic", C.c_double), ("n_param", C.c_int),
                ("iters", C.c_int), ("evals", C.c_int), ("l", C.c_double), ("b", C.c_double)]


ETS_MAX_PERIOD = 2048


def _spec(notation, m):
    e, t, s = R.parts(notation)
    return EtsSpec("AM".index(e) + 1, {"N": 0, "A": 1, "Ad": 1, "M": 2, "Md": 2}[t], int(t in ("Ad", "Md")), "NAM".index(s),
                   m if s != "N" else 1)


def oracle_start(O, y, notation, m):
    """oracle/ets.c ets_init_states: (l0, b0, s0 [m])."""
    L = O.lib()
    y = np.ascontiguousarray(y, dtype=np.float64)
    sp, l0, b0, s0 = _spec(notation, m), C.c_double(), C.c_double(), np.zeros(ETS_MAX_PERIOD)
    L.ets_init_states.restype = C.c_int
    L.ets_init_states.argtypes = [C.POINTER(EtsSpec), C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p]
    assert L.ets_init_states(C.byref(sp), y.ctypes.data, len(y), C.byref(l0), C.byref(b0), s0.ctypes.data) == 0
    return l0.value, b0.value, s0[: sp.m].copy()


def oracle_fixed_record(O, y, notation, m, params):
    """The oracle's record of ETS(notation) at given (alpha, beta, gamma, phi): oracle/ets.c ets_fit_fixed, then one more pass with the
    fitted-value hook set.  The fields of oracle.ets_inspect plus the start states; None when the series cannot be fitted."""
    L = O.lib()
    y = np.ascontiguousarray(y, dtype=np.float64)
    sp, fit, sfin = _spec(notation, m), EtsFit(), np.zeros(ETS_MAX_PERIOD)
    L.ets_fit_fixed.restype = C.c_int
    L.ets_fit_fixed.argtypes = [C.POINTER(EtsSpec), C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double,
                                C.POINTER(EtsFit), C.c_void_p]
    if len(y) < 3 or L.ets_fit_fixed(C.byref(sp), y.ctypes.data, len(y), *[float(p) for p in params], C.byref(fit), sfin.ctypes.data) != 0:
        return None
    l0, b0, s0 = oracle_start(O, y, notation, m)
    assert (l0, b0) == (fit.l0, fit.b0)
    fitted = np.full(len(y), np.nan)
    s0full = np.zeros(ETS_MAX_PERIOD)
    s0full[: sp.m] = s0
    sink = C.c_void_p.in_dll(L, "ets_fitted_sink")
    L.ets_lik.restype = C.c_double
    L.ets_lik.argtypes = [C.POINTER(EtsSpec), C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_void_p] + [C.c_void_p] * 4
    sink.value = fitted.ctypes.data
    try:
        L.ets_lik(C.byref(sp), y.ctypes.data, len(y), C.addressof(fit.par), l0, b0, s0full.ctypes.data, None, None, None, None)
    finally:
        sink.value = None
    e, t, s = R.parts(notation)
    nan = float("nan")
    return {"alpha": fit.alpha, "beta": fit.alpha * fit.beta_star if t != "N" else nan,
            "gamma": fit.gamma_star * (1.0 - fit.alpha) if s != "N" else nan, "phi": fit.phi if t in ("Ad", "Md") else nan,
            "level": fit.l, "trend": fit.b if t != "N" else nan,
            "seasonal_states": sfin[: sp.m].copy() if s != "N" else np.full(max(m, 1), nan), "fitted_values": fitted,
            "l0": l0, "b0": b0 if t != "N" else nan, "s0": s0 if s != "N" else None}


# ---- comparing records with the restatement

_REFS = {}


def replays(key, series, notation, m, h, recs):
    """The restatement's quantities (ets_ref.quantities) of every series of a batch in both formats, from each record's OWN parameters;
    computed once per `key` of a session.  recs[i] is None for a series without a fit.  Returns a list of None or
    {"q64", "q80": the quantities in float64 / 80-bit, "noise", "tol": the series' tolerance, "far": the largest |b - 1| raised to phi,
     "clamps": distances from the start-state clamps, "start64", "start80": the start states}."""
    key = ("replay",) + tuple(key)
    if key in _REFS:
        return _REFS[key]
    idx = [i for i, r in enumerate(recs) if r is not None]
    out = [None] * len(series)
    if idx:
        sub = [series[i] for i in idx]
        par = {k: [recs[i][k] for i in idx] for k in ("alpha", "beta", "gamma", "phi")}
        both = []
        for fmt in E.FORMATS:
            reps = E.replay_many(sub, notation, m, par["alpha"], par["beta"], par["gamma"], par["phi"], fmt)
            both.append([(rep, E.quantities(rep, len(y), notation, m, fmt(p), h)) for rep, y, p in zip(reps, sub, par["phi"])])
        for i, (r64, q64), (r80, q80) in zip(idx, *both):
            nz = E.noise(q64, q80)
            out[i] = {"q64": q64, "q80": q80, "noise": nz, "tol": max(REL_TOL, F * nz), "far": r80["far"], "clamps": r80["start"]["clamps"],
                      "start64": r64["start"], "start80": r80["start"]}
    _REFS[key] = out
    return out


def record_quantities(rec, point, notation):
    """The fields of an inspection record under the names of ets_ref.quantities."""
    e, t, s = R.parts(notation)
    q = {"fitted": rec["fitted_values"], "level": rec["level"], "point": point}
    if t != "N":
        q["trend"] = rec["trend"]
    if s != "N":
        q["seasonal"] = rec["seasonal_states"]
    return q


def check_clamps(clamps, want, where):
    """Every clamp of a series at least CLAMP_MARGIN (relative) on the side where it does not act -- except the one the case hits on
    purpose (`want`), which is at least as far on the side where it does; the fallback's own two floors stay unused."""
    for name, gap in clamps.items():
        if name == want:
            assert gap <= -CLAMP_MARGIN, (where, name, gap)
        else:
            assert gap >= CLAMP_MARGIN, (where, name, gap)
    if want is not None:
        assert want in clamps, (where, want, sorted(clamps))
