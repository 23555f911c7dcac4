"""The shared cases of the reconciliation tests: the smallest shapes at which the kernels can go wrong.  n_agg crosses the 64-wide
panels of the factor and of the substitution (0, 1, 2, 63, 64, 65, 129, 197: whole panels, one over, a ragged last panel), the
leaves go past one 64-lane tile of a member chain (1, 6, 70, 300), the rows past one 64-row tile and one 32-row chunk (1, 3, 65).
Plans: a series listed twice in an aggregate, two identical aggregates, an empty column, arbitrary (non-prefix) groupings, a prefix
plan whose total holds every leaf.  Forecasts: incoherent on purpose; one case with cancelling magnitudes (1e16, 1, -1e16), so that
a sum in another order fails the bit checks.  Each case is built once (seeded) and never changed; the yardsticks of a case are
computed once and shared."""
from __future__ import annotations

import functools

import numpy as np

import hierarchy_ref as HR
import reconcile_ref as R


def _table(n_leaf, agg_members, n_empty, rng, shuffle=True):
    """column_of [G, n_leaf] for bottoms + the given aggregates (lists of leaves, a leaf may repeat) + n_empty empty columns."""
    n_cols = n_leaf + len(agg_members) + n_empty
    ids = rng.permutation(n_cols) if shuffle else np.arange(n_cols)
    bottom_ids, agg_ids = ids[:n_leaf], ids[n_leaf:n_leaf + len(agg_members)]
    rows = [list(map(int, bottom_ids))]
    for i, ms in enumerate(agg_members):
        for k in range(max(ms.count(s) for s in set(ms))):       # one grouping row per occurrence: a leaf listed twice takes two
            rows.append([int(agg_ids[i]) if ms.count(s) > k else -1 for s in range(n_leaf)])
    return np.array(rows, dtype=np.int32)


def _random_aggs(n_leaf, n_agg, rng, total=False):
    aggs = []
    for i in range(n_agg):
        if total and i == 0:
            aggs.append(list(range(n_leaf)))
            continue
        size = int(rng.integers(2, max(3, min(n_leaf, 12) + 1))) if n_leaf > 1 else 2
        aggs.append(sorted(rng.choice(n_leaf, size=min(size, n_leaf), replace=False).tolist()) if n_leaf > 1 else [0, 0])
    return aggs


def _forecasts(co, rows, rng, scale=100.0):
    """Base forecasts [n_out, rows]: the leaves random, every aggregate its sum bent by a few percent, empty columns random."""
    n_out, offs, memb = HR.plan(co.tolist())
    p = R.parts(offs, memb, co.shape[1])
    y = rng.uniform(1.0, scale, size=(n_out, rows))
    for c in p["agg_cols"]:
        y[c] = sum(y[p["bottom_col"][s]] for s in p["cols"][c]) * rng.uniform(0.9, 1.1, size=rows)
    return y


def _case(name, n_leaf, aggs, rows, seed, n_empty=0, weights_decades=3.0):
    rng = np.random.default_rng(seed)
    co = _table(n_leaf, aggs, n_empty, rng)
    n_out, offs, memb = HR.plan(co.tolist())
    y = _forecasts(co, rows, rng)
    w = 10.0 ** rng.uniform(0.0, weights_decades, size=n_out)   # wls_var: within a ratio of 10^6
    return {"name": name, "column_of": co, "n_series": n_leaf, "n_out": n_out, "col_offsets": np.array(offs, dtype=np.int32),
            "members": np.array(memb, dtype=np.int32), "yhat": y, "weights": w, "rows": rows}


@functools.lru_cache(maxsize=None)
def all_cases():
    rng = np.random.default_rng(20241)
    cases = {}
    add = lambda c: cases.__setitem__(c["name"], c)
    add(_case("leaf1_agg0", 1, [], 1, 1))
    add(_case("leaf1_twice", 1, [[0, 0]], 3, 2))                                   # n_agg 1: the one leaf listed twice
    # 6 leaves: two identical aggregates, a leaf listed twice, an empty column, non-prefix groupings; n_out <= 40: the exact yardstick
    add(_case("small", 6, [[0, 1, 2], [0, 1, 2], [1, 3, 3, 5], [0, 2, 4, 5]], 3, 3, n_empty=2))
    add(_case("agg2", 6, [[0, 1, 2, 3, 4, 5], [4, 5]], 65, 4, n_empty=1))
    # the prefix plan of a 3-level key: stores 0-1 | 2-3 | 4-5, states, total -- with cancelling magnitudes in the leaves
    pre = _case("prefix_cancel", 6, [[0, 1, 2, 3, 4, 5], [0, 1, 2, 3], [4, 5], [0, 1], [2, 3]], 3, 5)
    p = R.parts(pre["col_offsets"].tolist(), pre["members"].tolist(), 6)
    for s, v in enumerate((1e16, 1.0, -1e16, 3.0, 0.25, 7.0)):
        pre["yhat"][p["bottom_col"][s], :] = v * np.array([1.0, 1.0, -1.0])
    add(pre)
    add(_case("agg63", 70, _random_aggs(70, 63, rng, total=True), 3, 6, n_empty=1))
    add(_case("agg64", 70, _random_aggs(70, 64, rng), 1, 7))
    add(_case("agg65", 70, _random_aggs(70, 65, rng, total=True), 65, 8))
    add(_case("agg129", 70, _random_aggs(70, 129, rng), 3, 9, n_empty=3))
    add(_case("agg197", 300, _random_aggs(300, 197, rng, total=True), 65, 10, n_empty=2, weights_decades=6.0))
    return cases


def names():
    return list(all_cases())


@functools.lru_cache(maxsize=None)
def plan_parts(name):
    c = all_cases()[name]
    return R.parts(c["col_offsets"].tolist(), c["members"].tolist(), c["n_series"])


@functools.lru_cache(maxsize=None)
def yardstick(name, method):
    """(yard [n_out, rows], allowance, weights) of a case under ols / wls_struct / wls_var; for bottom_up the chain itself, 0."""
    c, p = all_cases()[name], plan_parts(name)
    if method == "bottom_up":
        return R.bottom_up(p, c["yhat"]), 0.0, None
    w = R.method_weights(p, method, c["weights"])
    yard, tol = R.allowance(p, w, c["yhat"])
    return yard, tol, w


def participants(name):
    p = plan_parts(name)
    return list(p["bottom_col"]) + list(p["agg_cols"])


def empty_columns(name):
    p = plan_parts(name)
    return [c for c, ms in enumerate(p["cols"]) if not ms]


def with_nonfinite(name):
    """The case's block with a NaN in a bottom column (row 0), an inf in an aggregate column (last row) and a NaN in an empty column
    (row 1 if there is one, else row 0): (block, rows that must have status 2)."""
    c, p = all_cases()[name], plan_parts(name)
    y = c["yhat"].copy()
    bad = {0, y.shape[1] - 1}
    y[p["bottom_col"][0], 0] = np.nan
    y[p["agg_cols"][-1], y.shape[1] - 1] = np.inf
    for e in empty_columns(name):
        y[e, min(1, y.shape[1] - 1)] = np.nan
    return y, sorted(bad)


def time_major(block, pad=5, fill=-777.0):
    """[n_out, rows] -> a time-major block [rows, n_out + pad] whose padding columns hold `fill`."""
    t = np.full((block.shape[1], block.shape[0] + pad), fill)
    t[:, :block.shape[0]] = block.T
    return t
