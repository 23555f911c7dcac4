"""Small AutoARIMA inputs that reach every path of csrc/arima.hip, shared by tests/test_arima_cpu.py (oracle against the restatement
of tests/arima_ref.py, where the tolerances are measured) and tests/test_gpu_arima_replay.py (device against the restatement).
A family is dict(name, m, h, series[, valids]); every family stays at or below 192 series x 260 observations, h <= 40.
Everything is seeded; the references are computed once per session and handed out read-only."""
import json
import os

import numpy as np

import arima_ref as A

HERE = os.path.dirname(os.path.abspath(__file__))


def _synth():
    from anofox_forecast_amd import synth
    return synth


def simulate(rng, n, phi=(), theta=(), Phi=(), Theta=(), m=1, d=0, D=0, sd=1.0, level=0.0, season=None):
    """n values of a SARIMA process in the project's sign convention, integrated d times and D times seasonally, plus `level` and an
    optional fixed seasonal figure (array of m) that makes the decomposition's strength large."""
    fit = dict(p=len(phi), q=len(theta), P=len(Phi), Q=len(Theta), m=m, phi=list(phi), theta=list(theta), Phi=list(Phi), Theta=list(Theta))
    ar, ma = [np.asarray(v, dtype=np.float64) for v in A.polynomials(fit)]
    burn = 4 * (len(ar) + len(ma)) + 50
    T = n + burn
    e = rng.normal(0.0, sd, T)
    x = np.zeros(T)
    for t in range(T):
        acc = 0.0
        for k in range(len(ma)):
            if t - k >= 0:
                acc += ma[k] * e[t - k]
        for k in range(1, len(ar)):
            if t - k >= 0:
                acc -= ar[k] * x[t - k]
        x[t] = acc
    x = x[burn:]
    for _ in range(D):
        for t in range(m, n):
            x[t] += x[t - m]
    for _ in range(d):
        x = np.cumsum(x)
    x = x + level
    if season is not None:
        x = x + np.asarray(season)[np.arange(n) % m]
    return x


def _figure(m, amp):
    return amp * np.sin(2.0 * np.pi * np.arange(m) / m) + 0.5 * amp * (np.arange(m) == m // 3)


def ring_family(m):
    """One period per home of the seasonal ring: none (m = 1), registers (7), LDS (12, and 24 = the last LDS period), HBM (30)."""
    rng = np.random.default_rng(1000 + m)
    syn = _synth()
    T = {1: 150, 7: 160, 12: 170, 24: 240, 30: 260}[m]
    Y = syn.gen_series(syn.SEED_M5, 7000 + 16 * m, 6, T, max(m, 2))
    series = [Y[s, : T - 5 * s] for s in range(6)]
    for k in range(10):
        n = T - 3 * k
        if m == 1:
            series.append(simulate(rng, n, phi=(0.5, -0.3)[: 1 + k % 2], theta=(0.4,), d=k % 2, level=20.0))
        else:
            series.append(simulate(rng, n, phi=(0.5,), theta=(0.3,)[: k % 2], Phi=(0.5,) if k % 3 else (), Theta=(0.4,) if k % 3 != 1 else (),
                                   m=m, D=1 if k >= 5 else 0, level=40.0, season=_figure(m, 6.0 if k >= 5 else 0.0)))
    if m > 1:                     # a model without seasonal terms in the second pass variant, whatever the home of the ring
        series += [simulate(rng, T - 1 - 2 * k, phi=(0.5, -0.4), theta=(0.5, 0.3), level=40.0, sd=2.0) for k in range(3)]
    return dict(name=f"ring-m{m}", m=m, h={1: 5, 7: 15, 12: 25, 24: 40, 30: 40}[m], series=series)


def shapes_family(m):
    """Processes whose selected model lands in every pass variant: classes 0, 1, 5 without seasonal terms (m = 1), 2 .. 5 with (m = 7)."""
    rng = np.random.default_rng(2000 + m)
    series = []
    if m == 1:
        specs = [dict(phi=(0.6,), theta=(0.4,)), dict(phi=(0.5, -0.4), theta=(0.5, 0.3)), dict(phi=(0.4, -0.3, 0.35)),
                 dict(theta=(0.5, -0.4, 0.45, 0.35)), dict(phi=(0.3, 0.2, -0.3, 0.3)), dict(theta=(0.6, 0.4, 0.3))]
    else:
        specs = [dict(phi=(0.5,), theta=(0.4,), Phi=(0.5,), Theta=(0.4,)), dict(phi=(0.5,), theta=(0.5, 0.35), Phi=(0.4,), Theta=(0.3, 0.3)),
                 dict(phi=(0.5, -0.4), theta=(0.4, 0.3), Phi=(0.4, 0.3)), dict(phi=(0.4, -0.3, 0.35), Phi=(0.5,)),
                 dict(theta=(0.5, 0.3), Theta=(0.5, 0.3)), dict(phi=(0.5, -0.35), Theta=(0.5,))]
    for k, sp in enumerate(specs):
        for r in range(4):
            series.append(simulate(rng, 250 - 7 * r, m=m, level=30.0, sd=2.0, **sp))
    return dict(name=f"shapes-m{m}", m=m, h=8, series=series)


def differencing_family():
    """All six (d, D) pairs at m = 7, h = 40 (the integration runs 40 steps on d = 2 and wraps the season five times on D = 1)."""
    rng = np.random.default_rng(3000)
    series = []
    for r in range(3):
        n = 180 + 9 * r
        fig = _figure(7, 12.0)
        series.append(simulate(rng, n, phi=(0.3,), m=7, level=50.0))
        series.append(simulate(rng, n, theta=(0.3,), m=7, d=1, level=50.0))
        series.append(simulate(rng, n, phi=(0.4,), m=7, d=2, sd=0.5, level=50.0))
        series.append(simulate(rng, n, phi=(0.3,), m=7, level=50.0, season=fig))
        series.append(simulate(rng, n, theta=(0.3,), m=7, d=1, level=50.0, season=fig))
        series.append(simulate(rng, n, phi=(0.4,), m=7, d=2, sd=0.5, level=50.0, season=fig))
    return dict(name="differencing", m=7, h=40, series=series)


def horizons_family(h):
    """h = 1, m - 1, m, m + 1 and 2 m + 1 on D = 1 series of m = 7: the seasonal wrap of the integration on both sides of j = m."""
    rng = np.random.default_rng(3500)
    fig = _figure(7, 10.0)
    series = [simulate(rng, 120 + 5 * k, phi=(0.4,), theta=(0.3,)[: k % 2], m=7, d=k % 3 == 2, level=30.0, season=fig) for k in range(8)]
    return dict(name=f"horizons-h{h}", m=7, h=h, series=series)


HORIZONS = (1, 6, 7, 8, 15)
EDGE_LENGTHS = (31, 32, 33, 64, 65, 96, 97)          # differenced lengths around the streamed block of 32 steps


def lengths_family(m):
    """Lengths at which the code takes another path: 3 .. 12 (candidates become impossible, some series fit nothing), 18 and 19 (the
    KPSS lag goes 0 -> 1), differenced lengths on the edges of the 32-step block; with m = 7 also 3 m - 1 and 3 m (the strength rule),
    m + 2 and m + 3 (the guard of the seasonal difference) and the block edges after a seasonal difference."""
    rng = np.random.default_rng(4000 + m)
    series = []
    for n in list(range(3, 13)) + [18, 19] + ([3 * m - 1, 3 * m, m + 2, m + 3] if m > 1 else []):
        series.append(simulate(rng, n, phi=(0.4,), level=10.0))
        series.append(simulate(rng, n, theta=(0.3,), d=1, level=10.0))
    for n in EDGE_LENGTHS:
        series.append(simulate(rng, n, phi=(0.5,), theta=(0.3,), level=10.0))
        if m > 1:
            series.append(simulate(rng, n + m, phi=(0.5,), Theta=(0.4,), m=m, level=10.0, season=_figure(m, 9.0)))
    return dict(name=f"lengths-m{m}", m=m, h=3, series=series)


def ragged_family():
    """130 series (two full waves and two lanes), m = 7, lengths from 3 to 200 in no order: a wave's longest series is longer than most
    of its lanes'.  Four series carry one NULL each (integer neighbours: the interpolated value is exact), one series is constant, one
    all zero."""
    syn = _synth()
    rng = np.random.default_rng(5000)
    Y = syn.gen_series(syn.SEED_M5, 8100, 130, 200, 7)
    lens = rng.integers(24, 201, size=130)
    lens[[5, 70, 129]] = [3, 8, 11]
    lens[[0, 64, 128]] = 200
    series = [Y[s, 200 - lens[s]:].copy() for s in range(130)]
    series[17] = np.full(60, 3.0)
    series[90] = np.zeros(75)
    valids = [np.ones(len(y), dtype=bool) for y in series]
    for s in (3, 40, 77, 120):
        i = len(series[s]) // 2
        valids[s][i] = False
        series[s][i] = -999.0              # (never read: the slot is NULL)
    return dict(name="ragged", m=7, h=9, series=series, valids=valids)


def ragged_second_run():
    """Shorter series for a second run on the handle of the ragged family: series 20 .. 39 are too short to fit anything."""
    fam = ragged_family()
    series = [clean(y, v)[-60:].copy() for y, v in zip(fam["series"], fam["valids"])]
    for s in range(20, 40):
        series[s] = series[s][: 2 + s % 2]
    return dict(name="ragged-second", m=7, h=9, series=series)


def box_family():
    """The reference's known-answer series (its CSS optimum is the corner phi = (-0.99, -0.99)) and MA(1) processes with a root near the
    unit circle: selected coefficients on the +-0.99 box."""
    with open(os.path.join(HERE, "golden", "theta_kats.json")) as f:
        kat = np.array(json.load(f)["distinctness_series"]["y"], dtype=np.float64)
    rng = np.random.default_rng(6000)
    series = [kat, kat[:21].copy(), kat * 3.0 + 5.0]
    for k in range(9):
        series.append(simulate(rng, 90 + 11 * k, theta=(0.995 if k % 2 else -0.995,), level=20.0))
    return dict(name="box", m=1, h=12, series=series)


def families():
    out = [ring_family(m) for m in (1, 7, 12, 24, 30)] + [shapes_family(1), shapes_family(7), differencing_family()]
    out += [horizons_family(h) for h in HORIZONS] + [lengths_family(1), lengths_family(7), ragged_family(), box_family()]
    return {f["name"]: f for f in out}


FAMILY_NAMES = ["ring-m1", "ring-m7", "ring-m12", "ring-m24", "ring-m30", "shapes-m1", "shapes-m7", "differencing"] + \
               [f"horizons-h{h}" for h in HORIZONS] + ["lengths-m1", "lengths-m7", "ragged", "box"]

# what the families are there to reach (asserted on the oracle's selections by tests/test_arima_cpu.py and on the device's by the
# GPU test): every pass variant, every home of the ring, every pair of differences
INTENDED_CLASSES = {(c, "none") for c in (0, 1, 5)} | {(c, r) for c in range(6) for r in ("registers", "lds", "hbm")}
INTENDED_DIFFERENCES = {(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (2, 1)}

_CACHE = {}


def family(name):
    """A family by name (built once per session, series read-only)."""
    if "families" not in _CACHE:
        fams = families()
        fams["ragged-second"] = ragged_second_run()
        for f in fams.values():
            for y in f["series"]:
                y.setflags(write=False)
        _CACHE["families"] = fams
    return _CACHE["families"][name]


def clean(y, valid):
    """The series the model sees: an interior NULL is the mean of its two neighbours (linear interpolation across one slot)."""
    y = np.array(y, dtype=np.float64)
    if valid is not None:
        for i in np.flatnonzero(~np.asarray(valid)):
            y[i] = y[i - 1] + (y[i + 1] - y[i - 1]) * 0.5
    return y


def cleaned(fam):
    v = fam.get("valids")
    return [clean(y, v[s]) if v is not None else y for s, y in enumerate(fam["series"])]


def fit_from_record(rec, m):
    """A read-back record (api.arima_fit_record) as a fit of arima_ref."""
    return dict(p=rec["p"], d=rec["d"], q=rec["q"], P=rec["P"], D=rec["D"], Q=rec["Q"], m=max(int(m), 1), has_constant=bool(rec["has_constant"]),
                phi=[float(v) for v in rec["phi"]], theta=[float(v) for v in rec["theta"]], Phi=[float(v) for v in rec["Phi"]],
                Theta=[float(v) for v in rec["Theta"]], constant=float(rec["constant"]))


def fit_from_coordinates(order, x, m):
    """Orders (p, d, q, P, D, Q, has_constant) and optimiser coordinates (phi, theta, Phi, Theta, constant) as a fit: the
    coefficients are read through the box."""
    p, d, q, P, D, Q, c = [int(v) for v in order]
    x = [float(v) for v in x]
    box = lambda v: [min(max(u, -A.COEF_BOX), A.COEF_BOX) for u in v]
    k = [0, p, p + q, p + q + P, p + q + P + Q]
    pad = lambda v, n: v + [0.0] * (n - len(v))
    return dict(p=p, d=d, q=q, P=P, D=D, Q=Q, m=max(int(m), 1), has_constant=bool(c), phi=pad(box(x[k[0]:k[1]]), 5), theta=pad(box(x[k[1]:k[2]]), 5),
                Phi=pad(box(x[k[2]:k[3]]), 2), Theta=pad(box(x[k[3]:k[4]]), 2), constant=x[k[4]] if c else 0.0)


def replay(key, fit, y, h):
    """The restatement at a fit, computed once per key: css, n - La, criteria, forecasts, smallest root modulus."""
    key = ("replay",) + tuple(key)
    if key not in _CACHE:
        w = A.difference(y, fit["d"], fit["D"], fit["m"])
        c, nu, _, gross = A.css(fit, w, detail=True)
        out = dict(css=c, nu=nu, n=len(w), gross=gross, degenerate=A.degenerate(c, gross), forecast=A.forecast(fit, y, h), root=A.roots_min_modulus(fit), w=w)
        out.update(A.criteria(c, nu, len(w), A.n_parameters(fit)))
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def decisions(key, y, m):
    key = ("decide",) + tuple(key)
    if key not in _CACHE:
        _CACHE[key] = A.decide_differences(y, m)
    return _CACHE[key]
