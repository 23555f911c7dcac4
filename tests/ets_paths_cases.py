"""Hand-made fit records for the model-path tests (tests/test_ets_paths_cpu.py, tests/test_gpu_ets_paths.py): parameters and final
states of every one of the 25 specs as anofox_hip_batch_inspect_device lays them out, no fit needed.

The values are chosen so that no path can break or leave the positive numbers within the horizons the tests use: levels near 100,
additive growth below 1, growth rates within a percent of 1, seasonal figures within 10 % of neutral, innovations of about one unit
(additive error) or 2 % (multiplicative error), smoothing parameters inside the model's region.  Every test asserts n_broken == 0 on
the restatement alone, so that no comparison hides behind NaN == NaN.
"""
from __future__ import annotations

import numpy as np

import inspect_ref as R

SPEC_IDS = tuple(R.spec_id(s) for s in R.SPECS)


def records(n_series, m, seed=0, notation=None, ragged=True):
    """-> {"spec" int32 [n], "info" fp64 [8, n], "states" fp64 [2 + max(m, 1), n], "lengths" int32 [n]}.  Series s has spec
    R.SPECS[s % 25] (every wave mixes them) or `notation`; ragged lengths put different phases into one wave."""
    rng = np.random.default_rng([seed, n_series, m])
    n = int(n_series)
    spec = np.array([R.spec_id(notation) if notation else SPEC_IDS[s % 25] for s in range(n)], dtype=np.int32)
    lengths = (40 + rng.integers(0, 3 * max(m, 1) + 5, n) if ragged else np.full(n, 60)).astype(np.int32)
    info = np.full((8, n), np.nan)
    states = np.full((2 + max(m, 1), n), np.nan)
    for s in range(n):
        e, t, sn = R.parts(R.notation_of(int(spec[s])))
        alpha = rng.uniform(0.05, 0.4)
        info[0, s] = alpha
        states[0, s] = rng.uniform(80.0, 120.0)
        if t != "N":
            info[1, s] = rng.uniform(0.0, 0.5) * alpha
            states[1, s] = rng.uniform(-0.5, 0.8) if t in ("A", "Ad") else rng.uniform(0.995, 1.01)
        if sn != "N":
            info[2, s] = rng.uniform(0.0, 0.5) * (1.0 - alpha)
            states[2:2 + m, s] = rng.uniform(-6.0, 6.0, m) if sn == "A" else rng.uniform(0.9, 1.1, m)
        if t in ("Ad", "Md"):
            info[3, s] = rng.uniform(0.85, 0.98)
        sigma = rng.uniform(0.5, 1.5) if e == "A" else rng.uniform(0.01, 0.03)
        info[7, s] = sigma * sigma * float(lengths[s])
    return {"spec": spec, "info": info, "states": states, "lengths": lengths}


def pool(rec, rows, seed=0):
    """fp64 [rows, n] time-major: innovations in each series' own terms (about one unit, or 2 % for a multiplicative error)."""
    rng = np.random.default_rng([seed, rows, len(rec["spec"])])
    scale = np.where(rec["spec"] // 15 == 1, 0.02, 1.0)
    return rng.standard_normal((rows, len(rec["spec"]))) * scale[None, :]


def record_of(rec, s, m):
    """Series s as a record of inspect_ref.forecast."""
    return {"phi": rec["info"][3, s], "level": rec["states"][0, s], "trend": rec["states"][1, s], "seasonal_states": rec["states"][2:2 + m, s]}
