"""The fit-state readback (anofox_hip_batch_inspect; api.inspect_batch, ts_forecast_inspect_by, ts_forecast_explain_by) of every
ETS spec, ring class and schedule, against the CPU oracle AND against the high-precision identities of tests/inspect_ref.py.

The readback is a second launch of every spec's final kernel: it re-reads the parked optimum, the start states and the y block,
filters lanes by the selected model, writes the fitted values from inside the streamed loop and the seasonal ring once per ring
variant.  For every series: model code, the ten scalars, the fitted values and ALL m seasonal states equal oracle.ets_inspect at the
suite's 1e-12 (NaN meets NaN); the record's SSE, criteria and final states are what those names mean (inspect_ref.py; the oracle's
record meets the same identities on the same inputs: tests/test_inspect_cpu.py); fitted values are NaN past a series' length and
nowhere before it.  Inputs: tests/inspect_cases.py.
"""
import ctypes as C

import numpy as np
import pytest

import inspect_cases as K
import inspect_ref as R
from test_gpu_parity import REL_TOL, _rel

pytestmark = pytest.mark.gpu

_M7 = dict(seasonal_period=7)
NON_ETS = [("Naive", {}), ("SES", {}), ("SESOptimized", {}), ("Holt", {}), ("RandomWalkDrift", {}), ("ARIMA", {}), ("SMA", _M7),
           ("SeasonalNaive", _M7), ("HoltWinters", _M7), ("SeasonalES", _M7), ("SeasonalESOptimized", _M7), ("SeasonalWindowAverage", _M7),
           ("DynamicTheta", _M7), ("DynamicOptimizedTheta", _M7), ("CrostonClassic", {}), ("CrostonSBA", {}), ("TSB", {}), ("ADIDA", {}),
           ("IMAPA", {})]                            # (every forecast model of the batch entry but ETS and the two Auto searches)


@pytest.fixture(scope="module")
def env(hiplib, oracle):
    import torch
    assert torch.cuda.is_available()
    from anofox_forecast_amd import api
    return api, oracle, hiplib


def _report(what, worst):
    print(f"{what}: worst deviations " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(worst.items())))


def _all_nan(r):
    return (all(np.isnan(r[k]) for k in R.SCALARS) and bool(np.all(np.isnan(r["fitted_values"])))
            and bool(np.all(np.isnan(r["seasonal_states"]))))


def _check_record(r, ref, y, notation, m, worst, where):
    """One fitted series: the kernels' record against the oracle's, then against the identities."""
    for k in R.SCALARS:
        d = _rel(np.array([r[k]]), np.array([ref[k]]))
        worst["oracle"] = max(worst.get("oracle", 0.0), d)
        assert d <= REL_TOL, (where, notation, k, r[k], ref[k])
    assert len(r["fitted_values"]) == len(y) and not np.any(np.isnan(r["fitted_values"])), (where, notation)
    assert len(r["seasonal_states"]) == m == len(ref["seasonal_states"]), (where, notation)
    for k in ("fitted_values", "seasonal_states"):                      # every phase of the ring, NaN meeting NaN
        d = _rel(r[k], ref[k])
        worst["oracle"] = max(worst["oracle"], d)
        assert d <= REL_TOL, (where, notation, k, d)
    K.check_identities(r, y, notation, m, r["point"], worst, where)


def _check_unfitted(r, fc, where):
    """A series the forecast path rejects, or hands to the fallback chain: its status, error and model name, NaN fields."""
    assert r["ok"] == fc["ok"] and r["code"] == fc["code"] == r["status"], (where, r["code"], r["status"], fc)
    if fc["ok"]:
        assert r["model_name"] == fc["model_name"], (where, r["model_name"], fc["model_name"])
        assert _rel(r["point"], fc["point"]) <= REL_TOL, where
    else:
        assert r["message"] == fc["message"], (where, r["message"], fc["message"])
    assert _all_nan(r), (where, {k: r[k] for k in R.SCALARS})


@pytest.mark.parametrize("spec", R.SPECS)
def test_every_spec_readback(env, spec):
    """All 25 valid specs (m = 7; the nine without a season at seasonal_period = 1): one full wave plus a wave of 6, lengths of every
    residue modulo 7 that end inside streamed blocks, a horizon that wraps the phases twice.  NaN exactly where the spec has no
    such component, beta = alpha beta*, gamma = gamma* (1 - alpha), n_param of the spec, the multiplicative-error SSE."""
    api, O, lib = env
    series, m, h = K.every_spec(spec)
    res = api.inspect_batch(series, lib.make_options("ETS", h, ets_model=spec, seasonal_period=m))
    worst = {}
    for s, (y, r) in enumerate(zip(series, res)):
        ref = K.oracle_record(O, ("spec", spec, s), y, m, R.spec_id(spec))
        fc = K.oracle_forecast(O, ("spec", spec, s), y, None, "ETS", h, ets_model=spec, seasonal_period=m)
        assert r["ok"] and fc["ok"] and ref is not None, (spec, s, r["message"], fc)
        assert r["model_code"] == 0 and r["status"] == 0 and r["model_name"] == fc["model_name"], (spec, s, r["model_code"], r["model_name"])
        assert _rel(r["point"], fc["point"]) <= REL_TOL, (spec, s)
        _check_record(r, ref, y, spec, m, worst, s)
    _report(spec, worst)


@pytest.mark.parametrize("period", K.RING_PERIODS)
def test_ring_class_readback(env, period):
    """The seasonal ring of the readback in each of its homes: the compile-time m = 12 ring (additive class), the LDS ring (5, 24, 64),
    the HBM ring and its prefetched loop (65, 70; `2 + m` state rows), for an additive, a general and a damped multiplicative-trend
    spec; ragged lengths, one series a season short and one of exactly two seasons."""
    api, O, lib = env
    series, h = K.ring_class(period)
    worst = {}
    for spec in K.RING_SPECS:
        res = api.inspect_batch(series, lib.make_options("ETS", h, ets_model=spec, seasonal_period=period))
        fitted = 0
        for s, (y, r) in enumerate(zip(series, res)):
            ref = K.oracle_record(O, ("ring", period, spec, s), y, period, R.spec_id(spec))
            fc = K.oracle_forecast(O, ("ring", period, spec, s), y, None, "ETS", h, ets_model=spec, seasonal_period=period)
            if not fc["ok"]:
                assert ref is None
                _check_unfitted(r, fc, (period, spec, s))
                continue
            assert r["ok"] and ref is not None and r["model_code"] == 0 and r["model_name"] == fc["model_name"], (period, spec, s, r["message"])
            assert _rel(r["point"], fc["point"]) <= REL_TOL, (period, spec, s)
            _check_record(r, ref, y, spec, period, worst, (spec, s))
            fitted += 1
        assert fitted >= 21 and not res[24]["ok"], (period, spec, fitted)
    _report(f"m = {period}", worst)


def _check_auto(api, O, lib, period, idx, res, worst):
    series, valids, kind = K.auto_mixed()
    h = 2 * period + 3
    fitted = multiplicative = 0
    for s, r in zip(idx, res):
        yc = K.clean(O, series[s], valids[s])
        ref = K.oracle_record(O, ("auto", period, s), yc, period)
        fc = K.oracle_forecast(O, ("auto", period, s), series[s], valids[s], "AutoETS", h, seasonal_period=period)
        spec = R.notation_of_name(fc["model_name"]) if fc["ok"] else None
        if spec is None:
            assert ref is None
            _check_unfitted(r, fc, (period, s, kind[s]))
            continue
        assert r["ok"] and ref is not None and r["model_code"] == 100 + ref["spec_id"] and r["model_name"] == fc["model_name"], \
            (period, s, kind[s], r["model_code"], fc["model_name"])
        assert _rel(r["point"], fc["point"]) <= REL_TOL, (period, s)
        _check_record(r, ref, yc, spec, period, worst, (s, kind[s]))
        fitted += 1
        multiplicative += "M" in spec
    return fitted, multiplicative


@pytest.mark.parametrize("period", [7, 1])
def test_autoets_mixed_batch_readback(env, period):
    """A mixed batch: multiplicative specs run their first round on the gathered positive list, specs with nothing to fit are skipped by
    the run but launched by the readback; a constant, an all-zero, a five-point, a two-point and an empty series and ten series with
    NULLs (compared on the interpolated values).  Series on the fallback chain report NaN everywhere under the forecast path's name."""
    api, O, lib = env
    series, valids, kind = K.auto_mixed()
    res = api.inspect_batch(series, lib.make_options("AutoETS", 2 * period + 3, seasonal_period=period), valids)
    worst = {}
    fitted, multiplicative = _check_auto(api, O, lib, period, range(len(series)), res, worst)
    assert fitted >= 135 and multiplicative >= 10, (fitted, multiplicative)
    assert sum(1 for r in res if r["ok"] and _all_nan(r)) >= 2 and sum(1 for r in res if not r["ok"]) >= 2      # fallback chain; errors
    _report(f"AutoETS m = {period}", worst)


def _device_inspect(lib, series, opts, m):
    """The resident-block route: DeviceBatch, run, anofox_hip_batch_inspect on its handle.  Returns (batch, records, raw fitted rows)."""
    b, _ = _device_run_only(lib, series, opts)
    return b, *_read_back(lib, b, series, m)


def _results(b):
    import torch
    torch.cuda.synchronize()
    r = b.results()
    return {k: r[k].cpu().numpy().copy() for k in ("yhat", "lower", "upper", "model_code", "status")}


def _read_back(lib, b, series, m):
    n, T = b.n, max(b.t_max, 1)
    insp = (lib.AnofoxHipInspection * n)()
    fitted = np.full((n, T), 7.0)                    # (not NaN: the entry itself must write NaN past a length)
    seas = np.full((n, m), np.nan)
    err = lib.AnofoxError()
    assert b.L.anofox_hip_batch_inspect(b.handle, insp, fitted.ctypes.data, seas.ctypes.data, m, C.byref(err)), err.message
    res = _results(b)
    out = []
    for s in range(n):
        d = {k: getattr(insp[s], k) for k in ("model_code", "status") + R.SCALARS}
        d.update(fitted_values=fitted[s, : len(series[s])].copy(), seasonal_states=seas[s].copy(), point=res["yhat"][s], ok=insp[s].status == 0)
        out.append(d)
    return out, fitted


def _bits(records):
    """Every number of a list of records as one integer array (NaNs made one NaN): equal arrays are equal bits."""
    parts = []
    for r in records:
        parts += [np.array([r["model_code"], r["status"]], dtype=np.float64), np.array([r[k] for k in R.SCALARS]),
                  r["fitted_values"], r["seasonal_states"]]
        if r["ok"]:
            parts.append(np.asarray(r["point"], dtype=np.float64))
    a = np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in parts]) if parts else np.zeros(0)
    a[np.isnan(a)] = np.nan
    return a.view(np.uint64)


@pytest.mark.parametrize("period", [7, 1])
@pytest.mark.parametrize("tune", K.TUNES)
def test_autoets_readback_under_schedules(env, monkeypatch, tune, period):
    """The readback depends on where each schedule leaves the optimum: compaction and gather rounds, sequential rounds only, two-level
    speculation from the first round, four trial points per lane (raw counts), the float and the uint16 copy of the block
    (count-valued series; through the resident-block route, which also reports the storage).  Under every setting the record is
    the oracle's and meets the identities, and it does not move a bit against the default schedule."""
    api, O, lib = env
    series, valids, kind = K.auto_mixed()
    idx = K.tune_subset(tune, kind)
    sub, val = [series[s] for s in idx], [valids[s] for s in idx]
    opts = lib.make_options("AutoETS", 2 * period + 3, seasonal_period=period)
    compact = tune.startswith("compact")

    def run(setting):
        if setting is None:
            monkeypatch.delenv("ANOFOX_HIP_TUNE", raising=False)
        else:
            monkeypatch.setenv("ANOFOX_HIP_TUNE", setting)
        if not compact:
            return api.inspect_batch(sub, opts, val), None
        b, rec, _ = _device_inspect(lib, sub, opts, period)
        storage = b.stats()["y_storage"]
        b.close()
        return rec, storage

    base, base_storage = run("compact=0" if compact else None)
    got, storage = run(tune)
    if compact:
        assert (base_storage, storage) == (0, 1 if tune == "compact=1" else 2), (tune, base_storage, storage)
    assert np.array_equal(_bits(got), _bits(base)), tune
    worst = {}
    if compact:
        fitted = _check_device_auto(O, period, idx, got, worst)
    else:
        fitted, _ = _check_auto(api, O, lib, period, idx, got, worst)
    assert fitted >= len(idx) - 12, (tune, fitted, len(idx))
    _report(f"{tune} m = {period}", worst)


def _check_device_auto(O, period, idx, records, worst):
    """_check_auto for records of the resident-block route (codes instead of names and messages)."""
    series, valids, kind = K.auto_mixed()
    fitted = 0
    for s, r in zip(idx, records):
        ref = K.oracle_record(O, ("auto", period, s), series[s], period)
        fc = K.oracle_forecast(O, ("auto", period, s), series[s], valids[s], "AutoETS", 2 * period + 3, seasonal_period=period)
        spec = R.notation_of_name(fc["model_name"]) if fc["ok"] else None
        if spec is None:
            assert ref is None and r["status"] == fc["code"] and _all_nan(r), (period, s, r["status"], fc)
            continue
        assert r["ok"] and ref is not None and r["model_code"] == 100 + ref["spec_id"], (period, s, r["model_code"], fc["model_name"])
        assert _rel(r["point"], fc["point"]) <= REL_TOL, (period, s)
        _check_record(r, ref, series[s], spec, period, worst, (s, kind[s]))
        fitted += 1
    return fitted


def test_readback_does_not_disturb_the_run(env):
    """On a resident block: results() before and after the readback are the same bits, a second readback and a readback after a
    second run return the same bits, fitted values are NaN past a series' length and nowhere before it, and a readback before any
    run is INVALID_INPUT.  The default chain (ETS without a spec) and every model outside ETS report NaN fields beside the run's own
    model code and status.  A batch whose detected periods differ fails with the "one seasonal period" message and still forecasts."""
    import torch
    from anofox_forecast_amd.device import DeviceBatch
    api, O, lib = env
    series, valids, kind = K.auto_mixed()
    sub = [y for y, k in zip(series, kind) if k in ("positive", "counts")] + [series[130], series[132]]        # + constant, arange(5)
    opts = lib.make_options("AutoETS", 17, seasonal_period=7)
    fresh = DeviceBatch(len(sub), 120, opts, "cuda:0")
    insp = (lib.AnofoxHipInspection * len(sub))()
    err = lib.AnofoxError()
    assert not fresh.L.anofox_hip_batch_inspect(fresh.handle, insp, None, None, 7, C.byref(err))
    assert err.code == lib.INVALID_INPUT and b"has not been run" in err.message, (err.code, err.message)
    fresh.close()

    b, before = _device_run_only(lib, sub, opts)
    first, raw = _read_back(lib, b, sub, 7)
    after = _results(b)
    second, _ = _read_back(lib, b, sub, 7)
    b.run()
    torch.cuda.synchronize()
    rerun = _results(b)
    third, _ = _read_back(lib, b, sub, 7)
    final = _results(b)
    for k in before:
        assert np.array_equal(before[k], after[k], equal_nan=True) and np.array_equal(before[k], rerun[k], equal_nan=True), k
        assert np.array_equal(before[k], final[k], equal_nan=True), k
    assert np.array_equal(_bits(second), _bits(first)) and np.array_equal(_bits(third), _bits(first))
    fitted = 0
    for s, (y, r) in enumerate(zip(sub, first)):
        assert np.all(np.isnan(raw[s, len(y):])), s
        if r["ok"] and 100 <= r["model_code"] < 130:
            assert not np.any(np.isnan(raw[s, : len(y)])), s
            fitted += 1
        else:
            assert _all_nan(r), s
    assert fitted >= 120 and not np.isnan(first[0]["alpha"])
    b.close()

    few = sub[:20]
    for model, kw in [("ETS", dict(seasonal_period=7))] + NON_ETS:
        b, rec, raw = _device_inspect(lib, few, lib.make_options(model, 5, **kw), max(kw.get("seasonal_period", 1), 1))
        res = _results(b)
        b.close()
        assert np.all(np.isnan(raw)), model
        for s, r in enumerate(rec):
            assert _all_nan(r) and r["model_code"] == res["model_code"][s] and r["status"] == res["status"][s], (model, s, r["model_code"], r["status"])
        assert sum(1 for r in rec if r["status"] == 0) >= 10, (model, [r["status"] for r in rec])

    # detected periods that differ (params := MAP{}): no readback, the batch is unharmed
    rng = np.random.default_rng(31)
    t = np.arange(100)
    two = [50.0 + 0.02 * t + 8.0 * np.sin(2 * np.pi * t / p) + 3.0 * np.cos(4 * np.pi * t / p) + rng.normal(0, 0.6, 100) for p in (7, 12, 7, 12)]
    with pytest.raises(api.InvalidInputException, match="one seasonal period"):
        api.inspect_batch(two, lib.make_options("AutoETS", 6))
    auto = lib.make_options("AutoETS", 6)
    b, before = _device_run_only(lib, two, auto)
    assert sorted(set(b.periods().tolist())) == [7, 12], b.periods()
    insp = (lib.AnofoxHipInspection * 4)()
    err = lib.AnofoxError()
    assert not b.L.anofox_hip_batch_inspect(b.handle, insp, None, None, 12, C.byref(err))
    assert b"one seasonal period" in err.message, err.message
    b.run()
    again = _results(b)
    b.close()
    oo = O.make_options("AutoETS", 6)
    for k in before:
        assert np.array_equal(before[k], again[k], equal_nan=True), k
    for s, y in enumerate(two):
        ref = O.forecast(y, oo)
        assert ref["ok"] and again["status"][s] == 0 and _rel(again["yhat"][s], ref["point"]) <= REL_TOL, s


def _device_run_only(lib, series, opts):
    import torch
    from anofox_forecast_amd.device import DeviceBatch
    n, T = len(series), max(len(y) for y in series)
    b = DeviceBatch(n, T, opts, "cuda:0")
    Y = np.zeros((T, b.ld))
    lens = np.zeros(b.ld, dtype=np.int32)
    for s, y in enumerate(series):
        Y[: len(y), s] = y
        lens[s] = len(y)
    b.set_block(torch.from_numpy(Y).to("cuda:0"), torch.from_numpy(lens).to("cuda:0"))
    b.run()
    return b, _results(b)


@pytest.mark.parametrize("period", [7, 1])
def test_autoarima_readback(env, period):
    """AutoARIMA: aicc from the device equals the oracle fit's, the orders in model_code and has_constant are its orders, and aic / bic
    -- derived on the host from the orders and the length of the differenced series -- equal the extended-precision values from
    that aicc, k = p + q + P + Q + constant + 1 and the oracle's n_used (oracle/arima.c css_criterion)."""
    api, O, lib = env
    series = K.arima(period)
    res = api.inspect_batch(series, lib.make_options("AutoARIMA", 3, seasonal_period=period))
    worst, fitted = {"aicc": 0.0, "aic_bic": 0.0}, 0
    for s, (y, r) in enumerate(zip(series, res)):
        got = K.arima_detail(O, y, period, 3)
        if got is None:
            assert not (r["ok"] and r["model_code"] >= 1000000) and np.isnan(r["aicc"]), (period, s, r["model_code"])
            continue
        fit, point = got
        o = fit.ord
        assert r["ok"] and r["model_code"] >= 1000000, (period, s, r["code"], r["model_code"])
        c = r["model_code"] - 1000000
        assert (c // 100000, c // 10000 % 10, c // 1000 % 10, c // 100 % 10, c // 10 % 10, c % 10) == (o.p, o.d, o.q, o.P, o.D, o.Q), (period, s, c)
        assert r["has_constant"] == bool(o.with_constant), (period, s)
        assert _rel(r["point"], point) <= REL_TOL, (period, s)
        k = o.p + o.q + o.P + o.Q + o.with_constant + 1
        aic, bic = R.arima_criteria(fit.aicc, k, fit.n_used)
        worst["aicc"] = max(worst["aicc"], _rel(np.array([r["aicc"]]), np.array([fit.aicc])))
        worst["aic_bic"] = max(worst["aic_bic"], R.dev(r["aic"], aic), R.dev(r["bic"], bic))
        assert worst["aicc"] <= REL_TOL and worst["aic_bic"] <= REL_TOL, (period, s, worst, r["aic"], float(aic), r["bic"], float(bic), fit.n_used)
        assert all(np.isnan(r[k2]) for k2 in ("alpha", "beta", "gamma", "phi", "sse", "level", "trend")), (period, s)
        fitted += 1
    assert fitted >= len(series) - 2, fitted
    _report(f"AutoARIMA m = {period}", worst)


@pytest.mark.parametrize("m", [7, 5])
@pytest.mark.parametrize("spec", K.EXPLAIN_SPECS)
def test_explain_mirror_components(env, spec, m):
    """ts_forecast_explain_by: the level / trend / seasonal contribution of every step equals the forecast function's, taken apart in
    extended precision from the ORACLE's final states -- groups of every length residue modulo the period, a NULL target each, a
    horizon that wraps the phases twice; m = 7 (ring in registers) and m = 5 (ring in LDS).  (That the components recombine to yhat cannot tell a phase error in the mirror from one in the
    kernel: both would agree.)"""
    api, O, lib = env
    h = 17
    grp, ds, tgt = K.explain_groups(m)
    ex = api.ts_forecast_explain_by(grp, ds, tgt, "ETS", h, {"model": spec, "seasonal_period": m})
    assert sorted(ex) == [f"g{g}" for g in range(7)]
    worst = {"components": 0.0}
    for g in range(7):
        rows = np.flatnonzero(grp == f"g{g}")
        rows = rows[np.argsort(ds[rows], kind="stable")]
        valid = np.array([tgt[i] is not None for i in rows])
        y = np.array([0.0 if tgt[i] is None else tgt[i] for i in rows], dtype=np.float64)
        assert len(y) == 85 + g and int(np.sum(~valid)) == 1
        yc = K.clean(O, y, valid)
        ref = K.oracle_record(O, ("explain", m, spec, g), yc, m, R.spec_id(spec))
        fc = K.oracle_forecast(O, ("explain", m, spec, g), y, valid, "ETS", h, ets_model=spec, seasonal_period=m)
        assert ref is not None and fc["ok"]
        level, trend, seasonal = R.components(ref, len(y), spec, m, h)
        e = ex[f"g{g}"]
        assert e["horizon"] == h and e["model_name"] == fc["model_name"]
        for name, want in (("level", level), ("trend", trend), ("seasonal", seasonal)):
            assert want is not None and e[name] is not None and len(e[name]) == h, (spec, g, name)
            d = R.dev(e[name], want)
            worst["components"] = max(worst["components"], d)
            assert d <= REL_TOL, (spec, g, name, d)
        assert e["residual"] is None and _rel(e["yhat"], fc["point"]) <= REL_TOL, (spec, g)
    _report(f"explain {spec} m = {m}", worst)
