"""Inputs and the expected answers of the feature tests (tests/test_features_cpu.py, tests/test_gpu_features.py).

A series is a list of floats; None is a NULL (dropped by the entries that take a validity mask).  LENGTHS cover every presence rule
(1 .. 7, 10 .. 12, 20 / 21), the chunk_len = max(n / 10, 2) switch and its remainder chunk (19, 20, 21), the wave edge (63 .. 65),
more than one pass (255 .. 257), the tile edge and the workspace route (2,047 .. 2,049).  Every family runs at every length up to
257; each of the three longest lengths runs one or two families, so that the restatement stays quick.

expected(series) is computed once per series and kept: the restatement's features, presence and status, and per feature the
tolerance -- 0 (equality) except for what passes through ln or sin / cos, where it is 16 x the measured noise of the elementary
function for THIS series: ln moved one ulp each way (all up, all down, alternating); sin / cos moved one ulp each way and the float64 DFT against a longdouble one.
Above 64 rows the O(n^2) counts and the DFT come from numpy (integer counts; cumsum adds in order)."""
from __future__ import annotations

import math
import random

import numpy as np

import features_ref as R

LENGTHS = (1, 2, 3, 4, 5, 6, 7, 10, 11, 12, 19, 20, 21, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049)
SHORT_LENGTHS = tuple(n for n in LENGTHS if n <= 257)
LONG_LENGTHS = tuple(n for n in LENGTHS if n > 257)
NUMPY_ABOVE = 64
NOISE_FACTOR = 16.0


def _rng(name, n):
    return random.Random(f"{name}:{n}")


def ties(n):
    r = _rng("ties", n)
    pool = [0.0, -0.0, 1.0, 2.0, 2.0, 3.0, -1.0, 5.0, 0.0, -0.0]
    return [r.choice(pool) for _ in range(n)]


def constant(n):
    return [3.25] * n


def alternating(n):
    return [(1.0 if i % 2 == 0 else -1.0) * (1.0 + 0.5 * (i % 3)) for i in range(n)]


def monotone(n):
    return [0.75 * i - 3.0 for i in range(n)]


def decades(n):
    r = _rng("decades", n)
    return [r.choice((-1.0, 1.0)) * float(f"{r.randint(1, 9)}.{r.randint(0, 999):03d}e{r.randint(-150, 150)}") for _ in range(n)]


def sum_order(n):
    r = _rng("sum_order", n)
    pool = [1e16, -1e16, 1.0, 0.1, 3e-5, -0.1, 2.5]
    return [r.choice(pool) for _ in range(n)]


def walk(n):
    r = _rng("walk", n)
    x, out = 10.0, []
    for i in range(n):
        x += r.gauss(0.0, 1.0) + 0.8 * math.sin(i / 3.0)
        out.append(round(x, 2))
    return out


def with_inf(n):
    v = walk(n)
    v[n // 3] = math.inf
    if n >= 2:
        v[(2 * n) // 3 if (2 * n) // 3 != n // 3 else n - 1] = -math.inf
    return v


def one_nan(n):
    v = walk(n)
    v[n // 2] = math.nan
    return v


def nulls(n):
    r = _rng("nulls", n)
    return [None if r.random() < 0.2 else x for x in walk(n)]


FAMILIES = {"ties": ties, "constant": constant, "alternating": alternating, "monotone": monotone, "decades": decades,
            "sum_order": sum_order, "walk": walk, "inf": with_inf, "nan": one_nan, "nulls": nulls}
LONG_CASES = (("ties", 2047), ("walk", 2048), ("nulls", 2049), ("sum_order", 2049))     # (nulls: fewer than 2,049 values stay)

_series = {}


def series(family, n):
    """The same list object on every call, so that expected() can key on it."""
    if (family, n) not in _series:
        _series[(family, n)] = FAMILIES[family](n)
    return _series[(family, n)]


def short_cases():
    return [(f, n) for f in FAMILIES for n in SHORT_LENGTHS]


def long_cases():
    return list(LONG_CASES)


def split(s):
    """(values with 0.0 at the NULLs, validity)"""
    return [0.0 if x is None else float(x) for x in s], [x is not None for x in s]


def valid_values(s):
    return [float(x) for x in s if x is not None]


# ---- numpy counters: integers, so their order does not matter ----

def np_template_matches(v, m, r):
    a = np.asarray(v, dtype=np.float64)
    k = len(a) - m
    if k <= 1:
        return 0
    with np.errstate(invalid="ignore"):
        ok = np.ones((k, k), dtype=bool)
        for j in range(m):
            ok &= ~(np.abs(a[j:j + k, None] - a[None, j:j + k]) > r)
    return int(np.triu(ok, 1).sum())


def np_phi_counts(v, m, r):
    a = np.asarray(v, dtype=np.float64)
    k = len(a) - m + 1
    with np.errstate(invalid="ignore"):
        ok = np.ones((k, k), dtype=bool)
        for j in range(m):
            ok &= ~(np.abs(a[j:j + k, None] - a[None, j:j + k]) > r)
    return [int(c) for c in ok.sum(axis=1)]


def np_dft(v, shift=0, dtype=np.float64):
    """The source's DFT with numpy's sin / cos: the angle ((-2 pi k) t) / n rounded as the source rounds it, the sums in order
    (cumsum).  shift = +-1 moves every sin / cos one ulp; dtype=np.longdouble evaluates everything in extended precision."""
    x = np.asarray(v, dtype=dtype)
    n = len(x)
    k = np.arange(n, dtype=dtype)[:, None]
    t = np.arange(n, dtype=dtype)[None, :]
    pi = np.pi if dtype is np.float64 else np.longdouble("3.14159265358979323846264338327950288")
    with np.errstate(invalid="ignore", over="ignore"):
        ang = dtype(-2.0) * pi * k * t / dtype(n)
        c, s = np.cos(ang), np.sin(ang)
        if shift:
            way = dtype(np.inf if shift > 0 else -np.inf)
            c, s = np.nextafter(c, way), np.nextafter(s, way)
        re = np.cumsum(x[None, :] * c, axis=1)[:, -1] / dtype(n)
        im = np.cumsum(x[None, :] * s, axis=1)[:, -1] / dtype(n)
    return list(zip(re.tolist() if dtype is np.float64 else list(re), im.tolist() if dtype is np.float64 else list(im)))


def trig_figures(coeffs, to=float):
    """The 32 figures that pass through sin / cos, from the coefficients."""
    f = {}
    for i, (re, im) in enumerate(coeffs[:10]):
        f[f"fft_coefficient_{i}_real"], f[f"fft_coefficient_{i}_imag"] = to(re), to(im)
        f[f"fft_coefficient_{i}_abs"] = to(np.sqrt(re * re + im * im))
    power = [re * re + im * im for re, im in coeffs]
    total = type(power[0])(0)
    for p in power:
        total = total + p
    if total <= R.EPS:
        f["spectral_centroid"] = f["spectral_variance"] = 0.0
        return f
    sc = sv = type(power[0])(0)
    for i, p in enumerate(power):
        sc = sc + i * p
    cen = sc / total
    for i, p in enumerate(power):
        sv = sv + ((i - cen) * (i - cen)) * p
    f["spectral_centroid"], f["spectral_variance"] = to(cen), to(sv / total)
    return f


def log_figures(v, f, log, log2, cm, cm1, c2, c3):
    """The five figures that pass through ln, from the integer counts under them; also phi_2 and phi_3 of approximate_entropy."""
    n = len(v)
    r = 0.2 * f["standard_deviation"]
    out = {"binned_entropy": R.binned_entropy(v, f["minimum"], f["maximum"], log), "permutation_entropy": R.permutation_entropy(v, log),
           "lempel_ziv_complexity": R.lempel_ziv_complexity(v, f["mean"], log2)}
    out["sample_entropy"] = R.sample_entropy(v, r, log, lambda _v, m, _r: cm if m == 2 else cm1)
    if n < 3 or r <= 0.0:
        out["approximate_entropy"], out["phi_2"], out["phi_3"] = R.NAN, 0.0, 0.0
    else:
        out["phi_2"], out["phi_3"] = R.phi_from_counts(c2, log), R.phi_from_counts(c3, log)
        out["approximate_entropy"] = out["phi_2"] - out["phi_3"]
    return out


_expected = {}


def expected(s):
    """{"status", "features" (the inserted ones), "tol" {name: absolute tolerance, 0 = equality}, "noise" {name: measured noise}}"""
    key = id(s)
    if key in _expected:
        return _expected[key][1]
    v = valid_values(s)
    fast = len(v) > NUMPY_ABOVE
    counts = {}

    def matches(vv, m, r):
        counts[("m", m)] = np_template_matches(vv, m, r) if fast else R.template_matches(vv, m, r)
        return counts[("m", m)]

    def phis(vv, m, r):
        counts[("p", m)] = np_phi_counts(vv, m, r) if fast else R.phi_counts(vv, m, r)
        return counts[("p", m)]

    co = {}

    def dft(vv):
        co[0] = np_dft(vv) if fast else R.simple_dft(vv)
        return co[0]

    status, f = R.extract_features(v, matches=matches, counts=phis, dft=dft)
    out = {"status": status, "features": f, "tol": {k: 0.0 for k in f}, "noise": {}}
    if status == R.OK:
        # ln: every logarithm one ulp up, one ulp down, and alternately up and down
        base = log_figures(v, f, math.log, math.log2, counts.get(("m", 2), 0), counts.get(("m", 3), 0), counts.get(("p", 2), []), counts.get(("p", 3), []))
        noise = {k: 0.0 for k in base}
        for way, alt in R.LOG_VARIANTS:
            var = log_figures(v, f, R.log_shifted(way, math.log, alt), R.log_shifted(way, math.log2, alt), counts.get(("m", 2), 0), counts.get(("m", 3), 0), counts.get(("p", 2), []),
                              counts.get(("p", 3), []))
            for k in base:
                if base[k] == base[k] and var[k] == var[k]:
                    noise[k] = max(noise[k], abs(var[k] - base[k]))
        # a figure that went through ln is no better than its own last place: one ulp of the figure is the floor of its noise
        for k in base:
            if base[k] == base[k] and not math.isinf(base[k]):
                noise[k] = max(noise[k], math.ulp(base[k]))
        # a difference: the noise of its two terms, stated absolutely
        noise["approximate_entropy"] = max(noise["phi_2"] + noise["phi_3"], math.ulp(abs(base["phi_2"]) + abs(base["phi_3"])))
        for k in R.LOG_FEATURES:
            assert R.same(base[k], f[k]), (k, base[k], f[k])
            out["noise"][k] = noise[k]
            out["tol"][k] = NOISE_FACTOR * noise[k]
        # sin / cos: one ulp each way, and float64 against longdouble
        tb = trig_figures(co[0])
        tn = {k: 0.0 for k in tb}
        variants = [trig_figures(np_dft(v, way) if fast else R.simple_dft(v, R.trig_shifted(way))) for way in (+1, -1)]
        variants.append(trig_figures(np_dft(v, 0, np.longdouble)))
        for var in variants:
            for k in tb:
                if tb[k] == tb[k] and var[k] == var[k] and not math.isinf(tb[k]):
                    tn[k] = max(tn[k], abs(var[k] - tb[k]))
        coeff = max([tn[k] for k in tb if k.startswith("fft_")] or [0.0])     # one scale for the thirty coefficients
        for k in tb:
            assert R.same(tb[k], f[k]), (k, tb[k], f[k])
            out["noise"][k] = coeff if k.startswith("fft_") else tn[k]
            out["tol"][k] = NOISE_FACTOR * out["noise"][k]
    _expected[key] = (s, out)
    return out


def check(got, present, status, s, where=""):
    """Problems of one series: `got` {name: value} over all 117 names, `present` the set of names whose bit is set."""
    want = expected(s)
    bad = []
    if int(status) != want["status"]:
        return [(where, "status", int(status), want["status"])]
    if set(present) != set(want["features"]):
        return [(where, "present", sorted(set(present) ^ set(want["features"])))]
    for name in R.SORTED_NAMES:
        g = float(got[name])
        if name not in want["features"]:
            if g == g:
                bad.append((where, name, "absent but", g))
            continue
        w, tol = want["features"][name], want["tol"][name]
        if R.same(g, w):
            continue
        if tol > 0.0 and g == g and w == w and abs(g - w) <= tol:
            continue
        bad.append((where, name, g, w, tol))
    return bad
