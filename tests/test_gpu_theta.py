"""GPU: the dynamic Theta models (DynamicTheta, DynamicOptimizedTheta; csrc/fit_theta.hip) through every layer above the kernels
-- the C-ABI single and batch entries, the device-resident batch and the operator mirrors -- against the numpy checker
tests/theta_ref.py (the same IEEE operations: equal bit for bit) and the reference's pins and SQL tests
(test/sql/ts_model_distinctness.test, test/sql/ts_forecast_theta.test).  Theta, OptimizedTheta and AutoTheta keep their error."""
import json
import os

import numpy as np
import pytest

import theta_ref as R

pytestmark = pytest.mark.gpu

MODELS = R.MODELS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "theta_kats.json")))
Y24 = np.array(KATS["distinctness_series"]["y"], dtype=np.float64)
SQL = KATS["sql_cases"]


@pytest.fixture(scope="module")
def env(hiplib, oracle):
    import torch
    assert torch.cuda.is_available()
    from anofox_forecast_amd import api, synth
    return api, oracle, hiplib, synth


def _interpolated(O, y, valid):
    """The wrapper's NULL interpolation (imputation.rs), as the oracle restates it: what the kernels see."""
    y = np.ascontiguousarray(y, dtype=np.float64)
    if valid is None or len(y) == 0:
        return y.copy()
    mask = O.validity_mask(valid)
    out = np.empty_like(y)
    O.lib().oracle_fill_nulls_interpolate(y.ctypes.data, mask.ctypes.data, len(y), out.ctypes.data)
    return out


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def test_pins_and_names_through_the_c_abi(env):
    """test/sql/ts_model_distinctness.test:69-91: DynamicTheta to 6 dp, DynamicOptimizedTheta at its labelled deviation."""
    api, O, lib, synth = env
    pins = KATS["pins"]["point_1"]
    got = {}
    for m in MODELS:
        r = api.forecast_series(Y24, lib.make_options(m, 3, seasonal_period=0, auto_detect=False))
        assert r["ok"], (m, r)
        assert r["model_name"] == m
        got[m] = r["point"]
        assert _same(r["point"], R.forecast([Y24], m, 3)[0][0]), m
        assert np.all(r["lower"] <= r["point"]) and np.all(r["point"] <= r["upper"])
    assert round(float(got["DynamicTheta"][0]), 6) == pins["DynamicTheta"]
    dev = KATS["deviations"]["DynamicOptimizedTheta"]
    assert round(float(got["DynamicOptimizedTheta"][0]), 6) == dev["point_1"]
    assert abs(float(got["DynamicOptimizedTheta"][0]) / pins["DynamicOptimizedTheta"] - 1.0) < dev["max_rel"]


def test_unshipped_theta_models_keep_their_error(env):
    api, O, lib, synth = env
    for name, canon in (("Theta", "Theta"), ("theta", "Theta"), ("OptimizedTheta", "OptimizedTheta"), ("otm", "OptimizedTheta"),
                        ("AutoTheta", "AutoTheta"), ("auto_theta", "AutoTheta")):
        r = api.forecast_series(Y24, lib.make_options(name, 3))
        assert not r["ok"] and r["code"] == lib.INTERNAL_ERROR
        assert r["message"] == f"Internal error: model '{canon}' is not implemented by the HIP backend"


def _parity_batch(synth, n=300, T=260, seed=5501):
    """Synthetic M5-shape series, shifted positive for two thirds (the seasonal path) and raw counts for the rest: ragged lengths,
    NULL masks, constant and short series, an empty one."""
    rng = np.random.default_rng(seed)
    Y = synth.gen_series(synth.SEED_M5, 20000, n, T, 7, positive=False)
    lens = rng.integers(3, T + 1, n)
    series = [Y[s, :lens[s]].copy() + (0.0 if s % 3 == 0 else 5.0) for s in range(n)]
    valids = [None if s % 4 else rng.random(lens[s]) > 0.05 for s in range(n)]
    for s in range(0, n, 61):
        series[s][:] = 7.0
    for s in range(2, n, 37):
        series[s] = series[s] * (1.0 + 0.5 * np.sin(2.0 * np.pi * np.arange(len(series[s])) / 7.0))   # strong weekly pattern
    series += [np.array([3.0, 1.0, 2.0]), np.array([1.0, 2.0]), np.array([])]
    valids += [None, None, None]
    return series, valids


@pytest.mark.parametrize("period", [0, 7, 12])
def test_parity_with_the_checker(env, period):
    api, O, lib, synth = env
    series, valids = _parity_batch(synth)
    clean = [_interpolated(O, y, v) for y, v in zip(series, valids)]
    h = 14
    naive, nerr = api.forecast_batch(series, lib.make_options("Naive", h), valids)
    assert nerr["ok"]
    adjusted = 0
    for m in MODELS:
        got, berr = api.forecast_batch(series, lib.make_options(m, h, seasonal_period=period, auto_detect=False), valids)
        assert berr["ok"], (m, berr)
        ref, ok, _, _ = R.forecast(clean, m, h, period=period)
        adjusted += int(ok.sum())
        for s in range(len(series)):
            assert got[s]["ok"] == naive[s]["ok"] and got[s]["code"] == naive[s]["code"], (m, s, got[s], naive[s])
            if not got[s]["ok"]:
                continue
            assert got[s]["model_name"] == m
            assert _same(got[s]["point"], ref[s]), (m, period, s, got[s]["point"], ref[s])
            assert np.all(got[s]["lower"] <= got[s]["point"]) and np.all(got[s]["point"] <= got[s]["upper"])
    if period > 1:
        assert adjusted > 0


def test_m5_sample_against_the_checker(env):
    """A seeded sample of the 30,490 x 1,913 synthetic M5 block, raw counts (non-seasonal) and shifted positive at m = 7."""
    api, O, lib, synth = env
    rng = np.random.default_rng(77)
    pick = np.sort(rng.choice(30490, 96, replace=False))
    Y = np.stack([synth.gen_series(synth.SEED_M5, int(s), 1, 1913, 7, positive=False)[0] for s in pick])
    for period, shift in ((0, 0.0), (7, 1.0)):
        series = list(Y + shift)
        for m in MODELS:
            got, berr = api.forecast_batch(series, lib.make_options(m, 28, seasonal_period=period, auto_detect=False))
            assert berr["ok"]
            ref = R.forecast(series, m, 28, period=period)[0]
            for s in range(len(series)):
                assert got[s]["ok"] and _same(got[s]["point"], ref[s]), (m, period, s)


def test_full_m5_block_properties(env):
    """All 30,490 x 1,913 series, h = 28: every series fits, forecasts are finite and inside their intervals."""
    api, O, lib, synth = env
    Y = synth.gen_series(synth.SEED_M5, 0, 30490, 1913, 7, positive=False)
    for period in (0, 7):
        for m in MODELS:
            got, berr = api.forecast_batch(list(Y), lib.make_options(m, 28, seasonal_period=period, auto_detect=False))
            assert berr["ok"], (m, berr)
            assert all(g["ok"] and np.all(np.isfinite(g["point"])) for g in got), m
            assert all(np.all(g["lower"] <= g["point"]) and np.all(g["point"] <= g["upper"]) for g in got), m


def test_batch_company_does_not_matter(env):
    api, O, lib, synth = env
    series, valids = _parity_batch(synth, n=200, seed=5502)
    sub = np.random.default_rng(9).permutation(len(series))[:71]
    for m in MODELS:
        for period in (0, 7):
            opts = lib.make_options(m, 9, seasonal_period=period, auto_detect=False)
            full, _ = api.forecast_batch(series, opts, valids)
            part, _ = api.forecast_batch([series[s] for s in sub], opts, [valids[s] for s in sub])
            for j, s in enumerate(sub):
                assert part[j]["ok"] == full[s]["ok"] and part[j]["code"] == full[s]["code"], (m, s)
                if full[s]["ok"]:
                    for k in ("point", "lower", "upper"):
                        assert np.array_equal(part[j][k], full[s][k]), (m, s, k)


def test_device_resident_batch_equals_the_host_entry(env):
    import torch
    from anofox_forecast_amd.device import DeviceBatch
    api, O, lib, synth = env
    n, T, h = 150, 300, 9
    rng = np.random.default_rng(12)
    Y = synth.gen_series(synth.SEED_M5, 3000, n, T, 7, positive=False) + 2.0
    lens = rng.integers(3, T + 1, n).astype(np.int32)
    series = [Y[s, :lens[s]] for s in range(n)]
    for m in MODELS:
        for period in (0, 7):
            opts = lib.make_options(m, h, seasonal_period=period, auto_detect=False)
            host, berr = api.forecast_batch(series, opts)
            assert berr["ok"]
            b = DeviceBatch(n, T, opts, "cuda:0")
            try:
                block = torch.zeros((T, b.ld), dtype=torch.float64, device="cuda:0")
                block[:, :n] = torch.from_numpy(np.ascontiguousarray(Y.T)).to("cuda:0")
                ln = torch.zeros(b.ld, dtype=torch.int32, device="cuda:0")
                ln[:n] = torch.from_numpy(lens).to("cuda:0")
                b.set_block(block, ln)
                b.run()
                torch.cuda.synchronize()
                r = b.results()
                out = {k: r[k].cpu().numpy().reshape(n, -1) if k in ("yhat", "lower", "upper") else r[k].cpu().numpy() for k in ("yhat", "lower", "upper", "status")}
            finally:
                b.close()
            for s in range(n):
                assert host[s]["ok"] and out["status"][s] == 0, (m, s)
                assert np.array_equal(out["yhat"][s], host[s]["point"]), (m, period, s)
                assert np.array_equal(out["lower"][s], host[s]["lower"]) and np.array_equal(out["upper"][s], host[s]["upper"]), (m, s)


def test_auto_detect_equals_explicit_periods(env):
    """params := MAP{}: every series gets its detected period (the oracle's detection), exactly as if it had been given."""
    api, O, lib, synth = env
    Y = synth.gen_series(synth.SEED_M5, 500, 240, 210, 7, positive=True)
    series = list(Y)
    per = [int(O.lib().oracle_detect_seasonality_first(np.ascontiguousarray(y).ctypes.data, len(y))) for y in series]
    assert len(set(per)) > 1
    for m in MODELS:
        a, ea = api.forecast_batch(series, lib.make_options(m, 14, seasonal_period=0, auto_detect=True))
        assert ea["ok"]
        for p in sorted(set(per)):
            idx = [s for s in range(len(series)) if per[s] == p]
            b, eb = api.forecast_batch([series[s] for s in idx], lib.make_options(m, 14, seasonal_period=p if p > 1 else 0, auto_detect=False))
            assert eb["ok"]
            for j, s in enumerate(idx):
                assert a[s]["ok"] and b[j]["ok"], (m, s)
                for k in ("point", "lower", "upper"):
                    assert np.array_equal(a[s][k], b[j][k]), (m, p, s, k)


def _dates(rows):
    return np.datetime64(SQL["tables"]["start"], "us") + np.arange(rows) * np.timedelta64(1, "D")


def test_sql_replay_theta(env):
    """test/sql/ts_forecast_theta.test:212-300 and the table cases, through the mirrors of _ts_forecast, ts_forecast_agg,
    ts_forecast_by and ts_cv_forecast_by."""
    api, O, lib, synth = env
    ramp = np.array(SQL["ramp10"])
    tabs = SQL["tables"]
    rows = tabs["rows"]
    i = np.arange(rows)
    for m in MODELS:
        for name in (m,) + tuple(SQL["aliases"][m]):
            assert api.forecast_series(ramp, lib.make_options(name, 3))["model_name"] == m, name
        r = api.forecast_series(ramp, lib.make_options(m, 5, include_fitted=True, include_residuals=True))
        assert r["ok"] and len(r["point"]) == 5 and len(r["fitted"]) == 10 and len(r["residuals"]) == 10
        r = api.forecast_series(ramp, lib.make_options(m, 3))
        assert r["point"][0] > SQL["ramp10_point_1_above"] and r["lower"][0] <= r["point"][0] <= r["upper"][0]
        for key, up in (("trend_data", True), ("decreasing_data", False)):
            vals = tabs[key]["intercept"] + i * tabs[key]["slope"]
            agg = api.ts_forecast_agg(np.array(["x"] * rows, dtype=object), _dates(rows), vals, m, 5, {})
            fc = np.asarray(agg["x"]["point_forecast"])
            assert agg["x"]["model_name"] == m and len(fc) == 5 and np.all(np.isfinite(fc))
            assert (fc[-1] > fc[0]) if up else (fc[-1] < fc[0]), (m, key)
        g = tabs["grouped_data"]
        grp = np.array(["A"] * rows + ["B"] * rows, dtype=object)
        ds = np.concatenate([_dates(rows)] * 2)
        ys = np.concatenate([g["A"]["intercept"] + i * g["A"]["slope"], g["B"]["intercept"] + i * g["B"]["slope"]])
        ga = api.ts_forecast_agg(grp, ds, ys, m, 3, {})
        assert sorted(ga) == ["A", "B"] and all(ga[k]["model_name"] == m and np.all(np.isfinite(ga[k]["point_forecast"])) for k in ga)
        out = api.ts_forecast_by(grp, ds, ys, m, 4, "1d", {})
        assert len(out["yhat"]) == 8 and list(out["model_name"]) == [m] * 8 and np.all(np.isfinite(out["yhat"]))
        assert np.all((out["yhat_lower"] <= out["yhat"]) & (out["yhat"] <= out["yhat_upper"]))
        # ts_cv_forecast_by: two folds of the grouped table
        fold = np.concatenate([np.zeros(2 * rows, dtype=np.int64), np.ones(2 * rows, dtype=np.int64)])
        split = np.array((["train"] * (rows - 3) + ["test"] * 3) * 2 + (["train"] * (rows - 5) + ["test"] * 5) * 2, dtype=object)
        cv = api.ts_cv_forecast_by(fold, split, np.concatenate([grp, grp]), np.concatenate([ds, ds]), np.concatenate([ys, ys]), m, {})
        yh = np.asarray(cv["yhat"], dtype=np.float64)
        assert len(yh) == 2 * 3 + 2 * 5 and np.all(np.isfinite(yh)), m
