"""Hand-set ARIMA fits for the model-path tests (tests/test_arima_paths_cpu.py, tests/test_gpu_arima_paths.py): fit blocks as
anofox_hip_batch_arima_fit_device lays them out, no fit needed.

COMBOS is every combination of p in {0, 2, 5}, q in {0, 1, 5}, P, Q in {0, 1, 2}, d in {0, 1, 2}, D in {0, 1}, with and without a
constant: 972 order sets, cut into 8 chunks (seven of 129 series, one of 70 that wraps around), each used at every period.  The
coefficients keep the sum of their absolute values below 1 per factor, so no path can overflow within the horizons the tests use;
the series are a level near 50 with a random walk and a seasonal figure on it.  Lengths are ragged: a series has La + d + D m + nu
observations with nu = 1 for every ninth series, nu = 0 (no residual: NO_MODEL) for every ninth, and 4 .. 29 otherwise.  The series
block is NaN beyond a series' length and in the padding columns, so that a read past a length shows.
"""
from __future__ import annotations

import itertools

import numpy as np

import arima_paths_ref as AP

COMBOS = tuple(itertools.product((0, 2, 5), (0, 1, 5), (0, 1, 2), (0, 1, 2), (0, 1, 2), (0, 1), (0, 1)))       # p, q, P, Q, d, D, constant
PERIODS = (1, 2, 4, 7, 12)
CHUNKS = 8
T_ROWS = 90
_CACHE = {}


def chunk_combos(c):
    """Chunk c of COMBOS: 129 order sets (the last chunk: 70, wrapping around)."""
    n = 129 if c < CHUNKS - 1 else 70
    return [COMBOS[(c * 129 + s) % len(COMBOS)] for s in range(n)]


def horizons(m):
    """1, m - 1, m and 2 m + 6: every AR and MA lag and the seasonal integration reach back into the simulated values."""
    return sorted({h for h in (1, m - 1, m, 2 * m + 6) if h >= 1})


def _coefs(rng, k, total):
    if k == 0:
        return []
    v = rng.uniform(-1.0, 1.0, k)
    return [float(x) for x in v / np.abs(v).sum() * total]


def batch(m, combos, seed=0, pad=5):
    """-> dict(m, n, ld, fits, orders int32 [8, ld], coef fp64 [16, ld], y fp64 [T_ROWS, ld], lengths int32 [ld]), built once."""
    key = (m, tuple(combos), seed, pad)
    if key in _CACHE:
        return _CACHE[key]
    n = len(combos)
    ld = n + pad
    rng = np.random.default_rng([seed, m, n])
    fits, lengths = [], np.zeros(ld, dtype=np.int32)
    y = np.full((T_ROWS, ld), np.nan)
    for s, (p, q, P, Q, d, D, c) in enumerate(combos):
        base = p + m * P + d + D * m
        nu = 1 if s % 9 == 3 else (0 if s % 9 == 7 else int(rng.integers(4, 30)))
        nlen = min(base + nu, T_ROWS)
        t = np.arange(nlen)
        y[:nlen, s] = 50.0 + np.cumsum(rng.normal(0.0, 1.0, nlen)) + 3.0 * np.sin(2.0 * np.pi * t / max(m, 2))
        lengths[s] = nlen
        fits.append(dict(p=p, d=d, q=q, P=P, D=D, Q=Q, m=m, has_constant=bool(c), phi=_coefs(rng, p, 0.8), theta=_coefs(rng, q, 0.8),
                         Phi=_coefs(rng, P, 0.6), Theta=_coefs(rng, Q, 0.6), constant=float(rng.normal(0.0, 0.5))))
    orders, coef = AP.blocks_of(fits, ld, lengths, m)
    out = dict(m=m, n=n, ld=ld, fits=fits, orders=orders, coef=coef, y=y, lengths=lengths)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CACHE[key] = out
    return out


def status_scenario():
    """70 series at m = 7 (every 14th order set), spoiled one by one -> dict(batch, orders, coef, y, resid, rl, sigma: the spoiled
    inputs; no_model: four series (p = 6, D = 2, a wrong n_diff, a wrong resid_length); nan_coef, nan_sigma, nan_y, nan_resid: one series
    each, all with p > 0 and q > 0 so that both tails are read; overflow: a series with d = 2 and no AR term whose constant is 1e308
    -- ordinary arithmetic that leaves the finite numbers at the second step; joint_rows = 9: a series with 0 < nu < 9 is RAGGED)."""
    b = batch(7, list(COMBOS[::14]), seed=70)
    resid, rl, sigma = [np.array(v) for v in innovations(b)]
    orders, coef, y = np.array(b["orders"]), np.array(b["coef"]), np.array(b["y"])
    good = [int(s) for s in np.flatnonzero(rl > 8)]
    plain = [s for s in good if orders[0, s] == 0 and orders[3, s] == 0]
    over = [s for s in plain if orders[1, s] == 2][0]
    no_model = [s for s in plain if s != over][:4]
    both = [s for s in good if orders[0, s] > 0 and orders[2, s] > 0][:4]
    assert len(no_model) == 4 and len(both) == 4
    orders[0, no_model[0]] = 6
    orders[4, no_model[1]] = 2
    orders[7, no_model[2]] += 1
    rl[no_model[3]] -= 1
    coef[0, both[0]] = np.nan                               # phi_1
    sigma[both[1]] = np.nan
    y[b["lengths"][both[2]] - 1, both[2]] = np.nan          # the last observation
    resid[rl[both[3]] - 1, both[3]] = np.nan                # the last residual: in the MA tail and in every pool
    orders[6, over], coef[14, over] = 1, 1.0e308
    return dict(batch=b, orders=orders, coef=coef, y=y, resid=resid, rl=rl, sigma=sigma, no_model=no_model, nan_coef=both[0], nan_sigma=both[1],
                nan_y=both[2], nan_resid=both[3], overflow=over, joint_rows=9)


def check_status_scenario(sc, mode, status, n_broken, block, n_paths):
    """What status_scenario() must give in `mode` ("gaussian", "own", "joint" with pool_rows = joint_rows); block [n_paths * h, n]."""
    assert all(status[s] == AP.NO_MODEL for s in sc["no_model"]), status
    assert status[sc["nan_coef"]] == AP.NAN and status[sc["nan_y"]] == AP.NAN and status[sc["nan_resid"]] == AP.NAN, status
    assert status[sc["nan_sigma"]] == (AP.NAN if mode == "gaussian" else AP.OK), status
    o = sc["overflow"]
    assert status[o] == AP.OK and n_broken[o] == n_paths and np.isfinite(block[0, o]) and np.isnan(block[-1, o])
    whole = [s for s in range(sc["batch"]["n"]) if status[s] == AP.OK and s != o]
    assert len(whole) >= 20 and all(n_broken[s] == 0 for s in whole) and np.isfinite(block[:, whole]).all()
    ragged = [s for s in range(sc["batch"]["n"]) if 0 < sc["rl"][s] < sc["joint_rows"] and s not in sc["no_model"]]
    assert ragged and all(status[s] == (AP.RAGGED if mode == "joint" else AP.OK) for s in ragged), status


def innovations(b):
    """The restatement's (resid [T_ROWS, n], resid_lengths, sigma) of a batch, computed once."""
    key = ("innovations", id(b))
    if key not in _CACHE:
        out = AP.innovations(b["orders"], b["coef"], b["y"], b["lengths"], b["m"], n_series=b["n"])
        for v in out:
            v.setflags(write=False)
        _CACHE[key] = (b, out)
    return _CACHE[key][1]
