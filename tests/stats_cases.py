"""Shared by tests/test_stats_cpu.py and tests/test_gpu_stats.py: the golden statements of tests/golden/stats_kats.json, the
parity input families of the statistics contract and the comparison rule."""
from __future__ import annotations

import json
import math
import os

import numpy as np

import stats_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
KATS = os.path.join(HERE, "golden", "stats_kats.json")
TOLERANCES = os.path.join(HERE, "golden", "stats_tolerances.json")
N_FAMILY = 32


def load_kats():
    with open(KATS) as f:
        return json.load(f)


def cells(values):
    """JSON cells to Python: null stays None, "NaN" becomes a NaN."""
    return None if values is None else [float("nan") if v == "NaN" else v for v in values]


def table_columns(t):
    return t["group"], np.array(t["date"], dtype="datetime64[us]"), np.array([None if v is None else float(v) for v in t["value"]], dtype=object)


def check(value, op, *args):
    if op == "abs_lt":
        return abs(value) < args[0]
    if op == "gt":
        return value > args[0]
    if op == "close":
        return abs(value - args[0]) <= args[1] * max(1.0, abs(args[0]))
    if op == "finite":
        return math.isfinite(value)
    if op == "round0_ge":
        return round(value, 0) >= args[0]
    if op == "round1_eq":
        return round(value, 1) == args[0]
    raise ValueError(op)


def ref_stats_batch(series, valids=None, dates=None, frequency_micros=0, frequency_type="FIXED"):
    """api.stats_batch answered by the restatement."""
    out = []
    for i, s in enumerate(series):
        v = None if valids is None else valids[i]
        d = None if dates is None else dates[i]
        out.append(R.compute(s, v, d, frequency_micros, frequency_type))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# parity input families: name -> list of dict(values=, valid=)
# ----------------------------------------------------------------------------------------------------------------------
LONG_LENGTHS = (2049, 2500, 3000, 4097, 5000)


def families():
    from anofox_forecast_amd import synth
    n = N_FAMILY
    fam = {}
    counts = synth.gen_series(synth.SEED_M5, 0, n, 1913, 7, positive=False)
    fam["m5_counts"] = [dict(values=np.array(y, dtype=np.float64), valid=None) for y in counts]
    fam["m5_positive"] = [dict(values=np.array(y, dtype=np.float64), valid=None)
                          for y in synth.gen_series(synth.SEED_M5, 0, n, 1913, 7, positive=True)]
    rng = np.random.default_rng(20261001)
    fam["m5_real"] = [dict(values=np.array(y, dtype=np.float64) + rng.normal(0.0, 0.5, 1913), valid=None) for y in counts]
    rng = np.random.default_rng(20261002)
    fam["poisson"] = [dict(values=rng.poisson(0.7, 1913).astype(np.float64), valid=None) for _ in range(n)]
    rng = np.random.default_rng(20261003)
    fam["level_1e6"] = [dict(values=1e6 + rng.normal(0.0, 1.0, 1913), valid=None) for _ in range(n)]
    rng = np.random.default_rng(20261004)
    fam["short"] = [dict(values=rng.normal(3.0, 2.0, 10 + (i % 31)), valid=None) for i in range(n)]
    rng = np.random.default_rng(20261005)
    ragged = []
    for i in range(n):
        T = int(rng.integers(300, 2501))
        y = rng.gamma(2.0, 3.0, T)
        ok = rng.random(T) >= 0.05
        y[rng.random(T) < 0.01] = np.nan
        ragged.append(dict(values=y, valid=ok))
    fam["ragged"] = ragged
    rng = np.random.default_rng(20261006)
    fam["long"] = [dict(values=rng.normal(10.0, 3.0, LONG_LENGTHS[i % len(LONG_LENGTHS)]) + 0.001 * np.arange(LONG_LENGTHS[i % len(LONG_LENGTHS)]),
                        valid=None) for i in range(n)]
    return fam


COUNT_FAMILIES = ("m5_counts", "m5_positive", "poisson")     # entropy is compared here although a bin argument can be exactly .5


def load_tolerances():
    with open(TOLERANCES) as f:
        return json.load(f)["tolerances"]


def compare(got, ref, tol=None, where=""):
    """The contract: integers, booleans, the date figures and EXACT_FP are `==` (or both NaN); the other floating figures are
    within tol[figure] (default 1e-12) by |a - b| / max(1, |b|), NaN exactly where the restatement has NaN."""
    bad = []
    for f in R.INT_FIELDS + R.DATE_FIELDS + R.EXACT_FP:
        if not R.same(got[f], ref[f]):
            bad.append((where, f, got[f], ref[f]))
    worst = {}
    for f in R.TOL_FP:
        d = R.deviation(got[f], ref[f])
        worst[f] = d
        if not d <= (1e-12 if tol is None else tol[f]):
            bad.append((where, f, got[f], ref[f], d))
    return bad, worst
