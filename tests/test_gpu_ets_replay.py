"""The kernels' ETS records against the restatement of tests/ets_ref.py: for every fitted series of every case of tests/ets_cases.py
the fitted values, final level, trend, ALL m seasonal states and the point forecasts the device reports equal the textbook recursion,
run in 80-bit arithmetic from the classical-decomposition / least-squares start states at the record's OWN parameters, within that
series' tolerance max(1e-12, F x its float64-to-80-bit noise) -- F, the conditioning of every family and the distance of every series
from the start-state clamps are fixed without a GPU by tests/test_ets_cpu.py, on the oracle.  No oracle value enters a comparison
here except the statuses of the series nothing can be fitted to.

Fitted cases go through api.inspect_batch; the fixed-parameter cases (parameter corners, every path of prep.hip, the start-state
clamps) through DeviceBatch + set_fixed_params + anofox_hip_batch_inspect, where the record must also report exactly the given
parameters in model terms.  lower / upper are point -/+ z sd sqrt(i) at 0.80, 0.90, 0.95 and 0.99, once where the batch's final pass
carries the sd (one spec) and once where the second prep sweep does (AutoETS).
"""
import ctypes as C

import numpy as np
import pytest

import ets_cases as X
import ets_ref as E
import inspect_cases as K
import inspect_ref as R
from test_gpu_inspect import _check_unfitted

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(hiplib, oracle):
    import torch
    assert torch.cuda.is_available()
    from anofox_forecast_amd import api
    return api, oracle, hiplib


def _compare(key, series, notation, m, h, recs, worst):
    """Records of one batch (None: no fit) against the restatement at their own parameters; `worst` keeps the largest deviation /
    tolerance seen with its deviation, tolerance and noise."""
    reps = X.replays(("gpu",) + key, series, notation, m, h, recs)
    for s, (rec, rep) in enumerate(zip(recs, reps)):
        if rec is None:
            continue
        assert len(rec["fitted_values"]) == len(series[s]) and len(rec["seasonal_states"]) == max(m, 1), (key, s)
        assert R.component_rule(rec, notation, m) == [], (key, s, R.component_rule(rec, notation, m))
        got = X.record_quantities(rec, rec["point"], notation)
        d = E.deviation(got, rep["q80"])
        if d / rep["tol"] >= worst.get("ratio", -1.0):
            worst.update(ratio=d / rep["tol"], deviation=d, tolerance=rep["tol"], noise=rep["noise"], where=key + (s,))
        assert d <= rep["tol"], (key, s, notation, d, rep["tol"], rep["noise"], {k: R.dev(got[k], rep["q80"][k]) for k in rep["q80"]})
    return reps


def _report(what, worst):
    print(f"{what}: worst deviation {worst.get('deviation', 0.0):.2e} at tolerance {worst.get('tolerance', X.REL_TOL):.2e} "
          f"(noise {worst.get('noise', 0.0):.2e}, {worst.get('where')})")


@pytest.mark.parametrize("spec", R.SPECS)
def test_every_spec_record_is_the_recursion(env, spec):
    """All 25 specs, fitted: 70 series of every length residue modulo 7 (tests/inspect_cases.py every_spec)."""
    api, O, lib = env
    series, m, h = K.every_spec(spec)
    res = api.inspect_batch(series, lib.make_options("ETS", h, ets_model=spec, seasonal_period=m))
    assert all(r["ok"] and r["status"] == 0 for r in res), spec
    worst = {}
    _compare(("spec", spec), series, spec, m, h, res, worst)
    _report(spec, worst)


@pytest.mark.parametrize("period", K.RING_PERIODS)
def test_ring_class_record_is_the_recursion(env, period):
    """Every home of the seasonal ring, fitted, for an additive, two general and a damped multiplicative-trend spec; the series a season
    short and the fits that end without a finite likelihood report what the forecast path reports."""
    api, O, lib = env
    series, h = K.ring_class(period)
    worst = {}
    for spec in K.RING_SPECS:
        res = api.inspect_batch(series, lib.make_options("ETS", h, ets_model=spec, seasonal_period=period))
        recs = []
        for s, r in enumerate(res):
            fc = K.oracle_forecast(O, ("ring", period, spec, s), series[s], None, "ETS", h, ets_model=spec, seasonal_period=period)
            if not fc["ok"]:
                _check_unfitted(r, fc, (period, spec, s))
            else:
                assert r["ok"] and r["status"] == 0, (period, spec, s, r["message"])
            recs.append(r if fc["ok"] else None)
        assert recs[24] is None and sum(r is not None for r in recs) >= 21, (period, spec)
        _compare(("ring", period, spec), series, spec, period, h, recs, worst)
    _report(f"m = {period}", worst)


def _fixed_run(lib, series, spec, m, h, params, conf=0.90):
    """ETS(spec) at given parameters over a resident block, then the readback.  Returns (records or None per series, statuses)."""
    import torch
    from anofox_forecast_amd.device import DeviceBatch
    n, T = len(series), max(len(y) for y in series)
    b = DeviceBatch(n, T, lib.make_options("ETS", h, ets_model=spec, seasonal_period=m, confidence_level=conf), "cuda:0")
    try:
        Y = np.zeros((T, b.ld))
        lens = np.zeros(b.ld, dtype=np.int32)
        for s, y in enumerate(series):
            Y[: len(y), s] = y
            lens[s] = len(y)
        b.set_block(torch.from_numpy(Y).to("cuda:0"), torch.from_numpy(lens).to("cuda:0"))
        b.set_fixed_params(*params)
        b.run()
        torch.cuda.synchronize()
        mm = max(m, 1)
        insp = (lib.AnofoxHipInspection * n)()
        fitted = np.full((n, T), 7.0)
        seas = np.full((n, mm), np.nan)
        err = lib.AnofoxError()
        assert b.L.anofox_hip_batch_inspect(b.handle, insp, fitted.ctypes.data, seas.ctypes.data, mm, C.byref(err)), err.message
        torch.cuda.synchronize()
        res = {k: v.cpu().numpy().copy() for k, v in b.results().items()}
    finally:
        b.close()
    recs = []
    for s in range(n):
        assert insp[s].status == res["status"][s] and insp[s].model_code == res["model_code"][s], (spec, s)
        assert np.all(np.isnan(fitted[s, len(series[s]):])), (spec, s)
        d = {k: getattr(insp[s], k) for k in R.SCALARS}
        d.update(fitted_values=fitted[s, : len(series[s])].copy(), seasonal_states=seas[s].copy(), point=res["yhat"][s],
                 lower=res["lower"][s], upper=res["upper"][s])
        if res["status"][s] != 0:
            assert all(np.isnan(d[k]) for k in R.SCALARS) and np.all(np.isnan(d["fitted_values"])) and np.all(np.isnan(seas[s])), (spec, s)
        recs.append(d if res["status"][s] == 0 else None)
    return recs, res["status"][:n]


def _check_intervals(rec, y, conf, where):
    lo, hi = E.intervals(rec["point"], y, conf, E.LD)
    d = max(R.dev(rec["lower"], lo), R.dev(rec["upper"], hi))
    assert d <= X.REL_TOL, (where, conf, d)
    return d


@pytest.mark.parametrize("name", sorted(X.fixed_cases()))
def test_fixed_parameter_record_is_the_recursion(env, name):
    """Given parameters, one pass: the parameter corners, every path of prep.hip (the m = 7 register sweep straight-line and gated,
    season_figures_kernel in LDS and in scratch, even and odd periods, n = 2 m, the level-only start on fewer than 10 observations)
    and the start-state clamps.  The record reports exactly the given parameters; statuses as the oracle's fixed-parameter entry."""
    api, O, lib = env
    case = X.fixed_cases()[name]
    series, m, h = case["series"], case["m"], case["h"]
    offs = np.concatenate([[0], np.cumsum([len(y) for y in series])])
    vals = np.concatenate(series)
    worst, fitted, far = {}, 0, []
    for r, (spec, params) in enumerate(case["runs"]):
        recs, status = _fixed_run(lib, series, spec, m, h, params)
        assert np.array_equal(status, O.ets_fixed_batch(vals, offs, spec, m, *params, h)["status"]), (name, spec, status)
        e, t, sn = R.parts(spec)
        want = (params[0], params[1] if t != "N" else None, params[2] if sn != "N" else None, params[3] if t in ("Ad", "Md") else None)
        for s, rec in enumerate(recs):
            if rec is None:
                continue
            for k, v in zip(("alpha", "beta", "gamma", "phi"), want):
                assert (np.isnan(rec[k]) if v is None else rec[k] == v), (name, spec, s, k, rec[k], v)
            _check_intervals(rec, series[s], 0.90, (name, spec, s))
            fitted += 1
        reps = _compare(("fixed", name, r), series, spec, m, h, recs, worst)
        far.append(max((rep["far"] for rep in reps if rep is not None), default=0.0))
    assert fitted >= len(case["runs"]), (name, fitted)
    if name == "corner-MMdM":             # (the same parameters as on the oracle: a run inside |b - 1| <= 1/16 and a run outside it)
        assert min(far) < X.POW_NEAR1_R * (1.0 - 1.0e-6) and max(far) > X.POW_NEAR1_R * (1.0 + 1.0e-6), far
    _report(name, worst)


def test_autoets_record_is_the_recursion(env):
    """AutoETS, m = 7: a wave whose every series has a zero in its first block (the sweep stops computing the multiplicative figure),
    then a wave that mixes such series with strictly positive ones.  The selected spec is the oracle's; its record is the recursion."""
    api, O, lib = env
    series, h = X.auto_case()
    res = api.inspect_batch(series, lib.make_options("AutoETS", h, seasonal_period=7))
    by_spec = {}
    for s, r in enumerate(res):
        fc = K.oracle_forecast(O, ("ets-auto", s), series[s], None, "AutoETS", h, seasonal_period=7)
        spec = R.notation_of_name(fc["model_name"]) if fc["ok"] else None
        if spec is None:
            _check_unfitted(r, fc, s)
            continue
        assert r["ok"] and r["model_name"] == fc["model_name"] and r["model_code"] == 100 + R.spec_id(spec), (s, r["model_name"], fc["model_name"])
        by_spec.setdefault(spec, []).append(s)
    worst = {}
    for spec, idx in sorted(by_spec.items()):
        _compare(("auto", spec), [series[s] for s in idx], spec, 7, h, [res[s] for s in idx], worst)
    assert sum(len(v) for v in by_spec.values()) >= 60, by_spec
    _report("AutoETS m = 7", worst)


@pytest.mark.parametrize("conf", X.CONFIDENCES)
def test_intervals_follow_the_table(env, conf):
    """lower / upper = point -/+ z sd sqrt(i), sd the population sd of the series, z from the five-step table: on a one-spec batch
    (the final pass carries the sd) and on an AutoETS batch (the second prep sweep carries it)."""
    api, O, lib = env
    case = X.fixed_cases()["m7-block-edges"]
    recs, _ = _fixed_run(lib, case["series"], "MAM", 7, case["h"], X.PREP_PARAMS, conf)
    worst = max(_check_intervals(rec, y, conf, "one spec") for rec, y in zip(recs, case["series"]))
    series, h = X.auto_case()
    sub = series[58:70]
    res = api.inspect_batch(sub, lib.make_options("AutoETS", h, seasonal_period=7, confidence_level=conf))
    checked = 0
    for r, y in zip(res, sub):
        if r["ok"]:
            worst = max(worst, _check_intervals(r, y, conf, "AutoETS"))
            checked += 1
    assert checked >= 10, checked
    print(f"confidence {conf}: worst interval deviation {worst:.2e} at tolerance {X.REL_TOL:.0e}")
