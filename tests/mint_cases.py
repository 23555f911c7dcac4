"""The shared cases of the MinT-shrink tests: the plans and base forecasts of reconcile_cases with a block of base-forecast
residuals each.  Plans: a series counted twice, empty columns, cancelling magnitudes, and n_agg on both sides of the factor's
64-wide panels (64, 65, 129, 197).  n_res, crossed with the plans: 2 (the minimum), 3, 63 / 64 / 65 (the edge of a Gram tile and
of every 64-row staging tile), one value below n_agg (the sample covariance is rank-deficient: M is positive definite only through
lambda > 0) and one above.  Residuals: the bottoms share a common factor (a strong one where n_res < 8), so the correlations are
real; an aggregate's residuals follow the sum of its members' but are NOT that sum -- base forecasts are incoherent -- and every column's scale lies within about
1.5 decades, which keeps cond(M) <= 1e6 (test_mint_cpu.py checks both conditions for every case, on the CPU).  Each case is built
once (seeded) and never changed; the long-double yardsticks of a case are computed once and shared."""
from __future__ import annotations

import functools
import zlib

import numpy as np

import mint_ref as MR
import reconcile_cases as RC

PLANS = ("leaf1_twice", "small", "prefix_cancel", "agg64", "agg65", "agg129", "agg197")     # "small" and "agg129" hold empty columns
EPS = float(np.finfo(np.float64).eps)


def n_res_values(plan):
    n_agg = len(RC.plan_parts(plan)["agg_cols"])
    vals = {2, 3, 63, 64, 65, n_agg + 3}
    if n_agg - 1 >= 2:
        vals.add(n_agg - 1)
    return sorted(vals)


def names():
    return [f"{plan}-{n_res}" for plan in PLANS for n_res in n_res_values(plan)]


def _residuals(p, n_res, rng):
    n, na = p["n_series"], len(p["agg_cols"])
    A = p["A"].astype(np.float64)
    common = rng.standard_normal((n_res, 1))
    load = 0.6 if n_res >= 8 else 2.0                         # (a handful of rows: a strong factor, or the estimate clamps at 1)
    xb = (load * common + rng.standard_normal((n_res, n))) * 10.0 ** rng.uniform(0.0, 1.0, size=n)
    sums = xb @ A.T
    rms = np.sqrt((sums ** 2).mean(0))
    rms[rms == 0.0] = 1.0
    xa = (0.8 * sums / rms + 0.6 * rng.standard_normal((n_res, na))) * 10.0 ** rng.uniform(0.5, 1.5, size=na)
    res = rng.standard_normal((p["n_out"], n_res))            # (the rows of empty columns hold values too: they are never read)
    res[p["bottom_col"]] = xb.T
    res[p["agg_cols"]] = xa.T
    return res


@functools.lru_cache(maxsize=None)
def case(name):
    plan, n_res = name.rsplit("-", 1)
    c, p = RC.all_cases()[plan], RC.plan_parts(plan)
    for attempt in range(64):
        res = _residuals(p, int(n_res), np.random.default_rng([zlib.crc32(name.encode()), attempt]))
        # a handful of rows estimate lambda poorly, often past 1, where it is clamped: such a draw is replaced by the next one
        if int(n_res) >= 8 or 0.02 < float(MR.shrinkage_dense(p, res)[1]) < 0.98:
            break
    return {"name": name, "plan": plan, "n_res": int(n_res), "column_of": c["column_of"], "n_out": c["n_out"], "n_series": c["n_series"],
            "yhat": c["yhat"], "rows": c["rows"], "residuals": res}


def parts(name):
    return RC.plan_parts(case(name)["plan"])


@functools.lru_cache(maxsize=None)
def shrinkage(name):
    """(lambda by the dense pairwise formula in long double, as a float; the fp64 Gram route's value; the allowance for a computed
    lambda: 16 x the larger of the Gram route's own relative deviation and eps, relative to the dense value)."""
    c, p = case(name), parts(name)
    dense = float(MR.shrinkage_dense(p, c["residuals"])[0])
    gram = MR.shrinkage_gram(p, c["residuals"])
    return dense, gram, 16.0 * max(abs(gram - dense) / dense, EPS) * dense


@functools.lru_cache(maxsize=None)
def yardstick(name):
    """(yard [n_out, rows] by the long-double projection with the dense W at the dense lambda; the allowance: 16 x the larger of the
    plain fp64 constraint form's deviation from it and eps * max|yhat|)."""
    c, p = case(name), parts(name)
    part = MR.participants(p)
    dense, gram, _tol = shrinkage(name)
    yard = MR.project_longdouble(p, MR.dense_w(p, c["residuals"], dense), c["yhat"])
    noise = float(np.max(np.abs(MR.constraint_fp64(p, c["residuals"], gram, c["yhat"])[part] - yard[part])))
    return yard, 16.0 * max(noise, EPS * float(np.max(np.abs(c["yhat"][part]))))


@functools.lru_cache(maxsize=None)
def variances(name):
    return MR.variance_chain(parts(name), case(name)["residuals"])


def empty_columns(name):
    return RC.empty_columns(case(name)["plan"])
