"""GPU: forecasting with exogenous regressors (ARIMAX; csrc/fit_exog.hip) through every layer above the kernel -- the C-ABI single
entry anofox_ts_forecast_exog, the batch entry, the device-resident entry and the mirrors of _ts_forecast_exog / ts_forecast_exog_by
-- against the numpy checker tests/exog_ref.py.  Every numerical comparison is bit for bit (np.array_equal), no series is left
out of a comparison.  The golden inputs are those of the reference's test/sql/ts_forecast_exog.test (tests/golden/exog_cases.json)."""
import json
import os

import numpy as np
import pytest

import exog_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "exog_cases.json")))
Y6 = np.array([10.0, 20.0, 15.0, 25.0, 20.0, 30.0])
X6 = np.array([1.0, 2.0, 1.0, 2.0, 1.0, 2.0])
KS = (1, 2, 3, 5, 8)


@pytest.fixture(scope="module")
def env(hiplib, oracle):
    import torch
    assert torch.cuda.is_available()
    from anofox_forecast_amd import api, synth
    return api, oracle, hiplib, synth


def _interpolated(O, y, valid):
    y = np.ascontiguousarray(y, dtype=np.float64)
    if valid is None or len(y) == 0:
        return y.copy()
    mask = O.validity_mask(valid)
    out = np.empty_like(y)
    O.lib().oracle_fill_nulls_interpolate(y.ctypes.data, mask.ctypes.data, len(y), out.ctypes.data)
    return out


def _same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def _opts(lib, model, h, **kw):
    kw.setdefault("confidence_level", 0.95)
    kw.setdefault("auto_detect", False)
    return lib.make_options(model, h, **kw)


# ---------------------------------------------------------------------------------------------------------------------------
# single-series C ABI
# ---------------------------------------------------------------------------------------------------------------------------
def test_golden_cases_through_the_single_entry(env):
    api, O, lib, synth = env
    for c in GOLDEN["scalar_cases"]:
        y = np.array(c["values"])
        r = api.forecast_series_exog(y, c["xreg"], c["future_xreg"], _opts(lib, c["model"], c["horizon"], include_fitted=True, include_residuals=True))
        if c.get("expect_not_implemented"):
            assert not r["ok"] and r["code"] == lib.INTERNAL_ERROR and r["message"].endswith("is not implemented by the HIP backend"), (c["source"], r)
            assert c["reference_model"] in r["message"]
            assert api.ts_forecast_exog(c["values"], c["xreg"], c["future_xreg"], c["horizon"], c["model"]) is None
            continue
        assert r["ok"], (c["source"], r)
        h = c["expect_length"]
        assert len(r["point"]) == h and len(r["lower"]) == h and len(r["upper"]) == h
        assert np.all(r["lower"] <= r["point"]) and np.all(r["point"] <= r["upper"])
        assert len(r["fitted"]) == len(y) and len(r["residuals"]) == len(y) and r["n_fitted"] == len(y)
        assert np.isnan(r["aic"]) and np.isnan(r["bic"]) and np.isfinite(r["mse"])
        if "expect_model" in c:
            assert r["model_name"] == c["expect_model"]
            point, b0, beta, used = R.fit(y, c["xreg"], c["future_xreg"])
            lo, hi = R.intervals(y, point, 0.95)
            assert _same(r["point"], point) and _same(r["lower"], lo) and _same(r["upper"], hi), c["source"]
            # fitted values / residuals / mse: the SES(0.3) rule on y (forecast.rs:2593-2643), as anofox_ts_forecast reports them
            plain = api.forecast_series(y, _opts(lib, "ARIMA", h, include_fitted=True, include_residuals=True))
            assert _same(r["fitted"], plain["fitted"]) and _same(r["residuals"], plain["residuals"]) and r["mse"] == plain["mse"]
        else:
            assert r["model_name"].startswith(c["expect_model_prefix"])
        if "expect_point" in c:
            assert np.max(np.abs(r["point"] - np.array(c["expect_point"]))) <= 1e-12
        s = api.ts_forecast_exog(c["values"], c["xreg"], c["future_xreg"], c["horizon"], c["model"])
        assert s is not None and s["model"] == r["model_name"] and _same(s["point"], r["point"]) and _same(s["lower"], r["lower"])
        assert len(s["fitted"]) == len(y) and len(s["residuals"]) == len(y)


def test_error_contract(env):
    api, O, lib, synth = env
    o = lambda m, h=2: _opts(lib, m, h)
    r = api.forecast_series_exog(Y6, [X6[:5]], [[1.0, 2.0]], o("NoSuchModel"))
    assert r["code"] == lib.INVALID_MODEL and r["message"] == "Invalid model: Unknown model: 'NoSuchModel'"
    r = api.forecast_series_exog(Y6, [X6, X6[:5]], [[1.0, 2.0], [1.0, 2.0]], o("ARIMA"))
    assert r["code"] == lib.INVALID_INPUT and r["message"] == "Invalid input: Exogenous regressor 1 has 5 values but y has 6 values"
    r = api.forecast_series_exog(Y6, [X6], [[1.0, 2.0, 3.0]], o("AutoARIMA"))
    assert r["code"] == lib.INVALID_INPUT and r["message"] == "Invalid input: Exogenous regressor 0 has 3 future values but horizon is 2"
    # the regressor checks apply to models that ignore regressors too (lib.rs:3625-3668 runs before the model is looked at)
    r = api.forecast_series_exog(Y6, [X6], [[1.0, 2.0, 3.0]], o("Naive"))
    assert r["code"] == lib.INVALID_INPUT
    r = api.forecast_series_exog(Y6[:2], [X6[:2]], [[1.0, 2.0]], o("ARIMA"))
    assert r["code"] == lib.INSUFFICIENT_DATA and r["message"] == "Insufficient data: need at least 3 observations, got 2"
    r = api.forecast_series_exog([], [[]], [[1.0, 2.0]], o("ARIMA"))
    assert r["code"] == lib.INSUFFICIENT_DATA and r["message"] == "Insufficient data: need at least 1 observations, got 0"
    r = api.forecast_series_exog(Y6, [X6] * 9, [[1.0, 2.0]] * 9, o("ARIMA"))
    assert r["code"] == lib.COMPUTATION_ERROR and r["message"] == "Computation error: ARIMAX takes at most 8 exogenous regressors, got 9"


def test_thetax_and_mflesx_stay_not_implemented(env):
    api, O, lib, synth = env
    for m, x in (("OptimizedTheta", "ThetaX"), ("DynamicTheta", "ThetaX"), ("MFLES", "MFLESX"), ("AutoMFLES", "MFLESX")):
        r = api.forecast_series_exog(Y6, [X6], [[1.0, 2.0]], _opts(lib, m, 2))
        assert not r["ok"] and r["code"] == lib.INTERNAL_ERROR
        assert r["message"] == f"Internal error: model '{m}' with exogenous regressors ({x}) is not implemented by the HIP backend"
        res, berr = api.forecast_exog_batch([Y6, Y6[:2]], [[X6], [X6[:2]]], [[[1.0, 2.0]]] * 2, _opts(lib, m, 2))
        assert not berr["ok"] and berr["code"] == lib.INTERNAL_ERROR
        assert res[0]["code"] == lib.INTERNAL_ERROR and res[1]["code"] == lib.INSUFFICIENT_DATA
    # DynamicTheta without regressors runs as it does today
    y = np.arange(1.0, 41.0) + np.tile([0.0, 2.0, -1.0, 1.0], 10)
    a = api.forecast_series_exog(y, [], [], _opts(lib, "DynamicTheta", 4))
    b = api.forecast_series(y, _opts(lib, "DynamicTheta", 4))
    assert a["ok"] and b["ok"] and a["model_name"] == b["model_name"] == "DynamicTheta" and _same(a["point"], b["point"])


def test_models_outside_the_exog_set_ignore_the_regressors(env):
    api, O, lib, synth = env
    rng = np.random.default_rng(17)
    y = np.round(20 + rng.normal(0, 3, 60))
    x = rng.normal(0, 1, 60)
    fx = rng.normal(0, 1, 7)
    for m, kw in (("Naive", {}), ("SES", {}), ("Holt", {}), ("CrostonSBA", {}), ("SeasonalNaive", {"seasonal_period": 7}), ("AutoETS", {"seasonal_period": 7}),
                  ("DynamicOptimizedTheta", {}), ("AutoTheta", {})):
        o = _opts(lib, m, 7, include_fitted=True, **kw)
        a = api.forecast_series_exog(y, [x], [fx], o)
        b = api.forecast_series(y, o)
        assert a["ok"] == b["ok"] and a["code"] == b["code"] and a["message"] == b["message"], (m, a, b)
        if b["ok"]:
            assert a["model_name"] == b["model_name"] and _same(a["point"], b["point"]) and _same(a["lower"], b["lower"]) and _same(a["upper"], b["upper"])
            assert _same(a["fitted"], b["fitted"])
        res, berr = api.forecast_exog_batch([y, y[:30]], [[x], [x[:30]]], [[fx], [fx]], o)
        ref, rerr = api.forecast_batch([y, y[:30]], o)
        assert berr["ok"] == rerr["ok"]
        for p, q in zip(res, ref):
            assert p["ok"] == q["ok"] and p["code"] == q["code"]
            if q["ok"]:
                assert p["model_name"] == q["model_name"] and _same(p["point"], q["point"]) and "beta" not in p


def test_ordinary_path_keeps_the_checks_of_the_plain_entry(env):
    """under the exogenous entries the ordinary path is anofox_ts_forecast itself -- an explicit ETS spec is
    honoured and seasonal_period is validated against the model (the reference's forecast_with_model drops the one and skips the
    other); the ARIMAX path has no period, so ARIMA with a seasonal_period and regressors runs (as in the reference)."""
    api, O, lib, synth = env
    rng = np.random.default_rng(23)
    y = np.round(50 + rng.normal(0, 5, 80)) + 1.0
    x = rng.normal(0, 1, 80)
    fx = rng.normal(0, 1, 5)
    o = _opts(lib, "ETS", 5, ets_model="ANN")
    a, b = api.forecast_series_exog(y, [x], [fx], o), api.forecast_series(y, o)
    assert a["ok"] and a["model_name"] == b["model_name"] == "ETS(ANN)" and _same(a["point"], b["point"])
    o = _opts(lib, "Naive", 5, seasonal_period=7)
    a, b = api.forecast_series_exog(y, [x], [fx], o), api.forecast_series(y, o)
    assert not a["ok"] and a["code"] == b["code"] == lib.INVALID_INPUT and a["message"] == b["message"]
    a = api.forecast_series_exog(y, [x], [fx], _opts(lib, "ARIMA", 5, seasonal_period=7))
    assert a["ok"] and a["model_name"] == "ARIMAX" and _same(a["point"], R.fit(y, [x], [fx])[0])
    a = api.forecast_series_exog(y, [x], [fx], _opts(lib, "AutoARIMA", 5, seasonal_period=7))
    assert a["ok"] and a["model_name"] == "ARIMAX" and _same(a["point"], R.fit(y, [x], [fx])[0])


# ---------------------------------------------------------------------------------------------------------------------------
# batches
# ---------------------------------------------------------------------------------------------------------------------------
P_CONST, P_COPY, P_ZERO = 0.03, 0.03, 0.02      # injection rates of aliased regressors (per regressor)


def _parity_batch(synth, K, n=2000, T=400, h=14, seed=5501):
    """Seed 5501 + K.  Lengths 3-400 (every 97th series 3-8 long: n <= K and the naive branch), regressors of synth.gen_regressors,
    each replaced by a constant with probability 0.03, by a copy of regressor 0 with 0.03 (j >= 1) and by zeros with 0.02; y
    count-valued for even series, real-valued for odd ones; every third series carries ~5 % NULLs."""
    rng = np.random.default_rng(seed + K)
    XF = synth.gen_regressors(synth.SEED_EXOG, 7000 * K, n, T, h, K)
    for s in range(n):
        for j in range(K):
            u = rng.random()
            if u < P_CONST:
                XF[s, j, :] = XF[s, j, 0]
            elif u < P_CONST + P_COPY and j >= 1:
                XF[s, j, :] = XF[s, 0, :]
            elif u < P_CONST + P_COPY + P_ZERO:
                XF[s, j, :] = 0.0
    Yc = synth.gen_exog_target(synth.SEED_EXOG, 7000 * K, n, XF[:, :, :T], real_valued=False)
    Yr = synth.gen_exog_target(synth.SEED_EXOG, 7000 * K, n, XF[:, :, :T], real_valued=True)
    lens = rng.integers(3, T + 1, n)
    lens[::97] = 3 + (np.arange(len(lens[::97])) % 6)
    series = [(Yc if s % 2 == 0 else Yr)[s, :lens[s]].copy() for s in range(n)]
    xs = [[XF[s, j, :lens[s]].copy() for j in range(K)] for s in range(n)]
    fs = [[XF[s, j, T:].copy() for j in range(K)] for s in range(n)]
    valids = [None if s % 3 else rng.random(lens[s]) > 0.05 for s in range(n)]
    return series, xs, fs, valids


def _check_against_checker(lib, O, got, series, xs, fs, valids, conf=0.95):
    clean = [_interpolated(O, y, v) for y, v in zip(series, valids)]
    ref = R.fit_batch(clean, xs, fs)
    K = len(xs[0])
    for s in range(len(series)):
        g = got[s]
        assert g["ok"], (s, g)
        assert g["model_name"] == "ARIMAX"
        lo, hi = R.intervals(clean[s], ref["point"][s], conf)
        assert _same(g["point"], ref["point"][s]), (s, K, len(series[s]), g["point"], ref["point"][s])
        assert _same(g["lower"], lo) and _same(g["upper"], hi), (s, K)
        assert g["intercept"] == ref["b0"][s], (s, K, g["intercept"], ref["b0"][s])
        assert _same(g["beta"], ref["beta"][s]) and np.array_equal(g["used"], ref["used"][s]), (s, K, g["used"], ref["used"][s])
    return ref


def test_ragged_batches_match_the_checker(env):
    api, O, lib, synth = env
    total = 0
    for K in KS:
        series, xs, fs, valids = _parity_batch(synth, K)
        got, berr = api.forecast_exog_batch(series, xs, fs, _opts(lib, "AutoARIMA" if K % 2 else "ARIMA", 14), valids)
        assert berr["ok"], berr
        ref = _check_against_checker(lib, O, got, series, xs, fs, valids)
        used = ref["used"]
        none_used = float(np.mean(~used.any(axis=1)))
        pairs_unused = float(np.mean(~used))
        short = sum(len(y) < 5 for y in series)
        n_le_k = sum(len(y) <= K for y in series)
        print(f"K {K}: {len(series)} series, no regressor used {none_used:.4f}, pairs unused {pairs_unused:.4f}, shorter than 5: {short}, n <= K: {n_le_k}")
        assert none_used <= 0.10 and pairs_unused <= 0.20, (K, none_used, pairs_unused)
        assert short > 0 and (K < 3 or n_le_k > 0)
        assert np.isfinite(ref["b0"]).all()
        total += len(series)
    assert total >= 2000


def test_failing_series_do_not_disturb_the_batch(env):
    api, O, lib, synth = env
    series, xs, fs, valids = _parity_batch(synth, 2, n=200, T=120, h=5, seed=77)
    extra = [np.array([]), np.array([4.0]), np.array([1.0, 2.0])]
    series2 = series + extra
    xs2 = xs + [[np.zeros(len(e)), np.zeros(len(e))] for e in extra]
    fs2 = fs + [[np.zeros(5), np.zeros(5)] for e in extra]
    got, berr = api.forecast_exog_batch(series2, xs2, fs2, _opts(lib, "ARIMA", 5), valids + [None] * 3)
    assert berr["ok"], berr
    _check_against_checker(lib, O, got[:200], series, xs, fs, valids)
    msgs = ["Insufficient data: need at least 1 observations, got 0", "Insufficient data: need at least 3 observations, got 1",
            "Insufficient data: need at least 3 observations, got 2"]
    for g, m in zip(got[200:], msgs):
        assert not g["ok"] and g["code"] == lib.INSUFFICIENT_DATA and g["message"] == m


def test_batch_independence(env):
    """A shuffled sub-batch gives every series the bits it got in the full batch."""
    api, O, lib, synth = env
    series, xs, fs, valids = _parity_batch(synth, 5, n=600, T=300, h=9, seed=91)
    o = _opts(lib, "ARIMA", 9)
    full, berr = api.forecast_exog_batch(series, xs, fs, o, valids)
    assert berr["ok"]
    pick = np.random.default_rng(92).permutation(600)[:217]
    sub, berr = api.forecast_exog_batch([series[i] for i in pick], [xs[i] for i in pick], [fs[i] for i in pick], o, [valids[i] for i in pick])
    assert berr["ok"]
    for g, i in zip(sub, pick):
        f = full[i]
        assert g["ok"] and f["ok"]
        assert _same(g["point"], f["point"]) and _same(g["lower"], f["lower"]) and _same(g["upper"], f["upper"])
        assert g["intercept"] == f["intercept"] and _same(g["beta"], f["beta"]) and np.array_equal(g["used"], f["used"])
    one = api.forecast_series_exog(series[pick[0]], xs[pick[0]], fs[pick[0]], o, valids[pick[0]])
    assert one["ok"] and _same(one["point"], full[pick[0]]["point"]) and _same(one["upper"], full[pick[0]]["upper"])


def _device_blocks(series, xs, fs, T, h):
    import torch
    n, K = len(series), len(xs[0])
    ld = (n + 63) // 64 * 64
    y = np.zeros((T, ld))
    x = np.zeros((K, T, ld))
    f = np.zeros((K, h, ld))
    ln = np.zeros(ld, dtype=np.int32)
    for s in range(n):
        m = len(series[s])
        ln[s] = m
        y[:m, s] = series[s]
        for j in range(K):
            x[j, :m, s] = xs[s][j]
            f[j, :, s] = fs[s][j]
    return torch.from_numpy(y).cuda(), torch.from_numpy(ln).cuda(), torch.from_numpy(x).cuda(), torch.from_numpy(f).cuda()


@pytest.mark.parametrize("model,n", [("ARIMA", 700), ("AutoARIMA", 130)])
def test_device_resident_entry(env, model, n):
    """set_exog adopts the blocks: the run equals the host batch entry; set_exog(None) restores the ordinary model bit for bit."""
    import torch
    api, O, lib, synth = env
    from anofox_forecast_amd.device import DeviceBatch
    T, h, K = 200, 7, 3
    series, xs, fs, _ = _parity_batch(synth, K, n=n, T=T, h=h, seed=301)
    for s in range(0, n, 50):
        series[s] = series[s][:2]                     # too short: an error on both paths
        xs[s] = [c[:2] for c in xs[s]]
    o = _opts(lib, model, h)
    host, berr = api.forecast_exog_batch(series, xs, fs, o)
    assert berr["ok"]
    plain, perr = api.forecast_batch(series, o)
    assert perr["ok"]
    y, ln, x, f = _device_blocks(series, xs, fs, T, h)
    b = DeviceBatch(n, T, o, "cuda:0")
    b.set_block(y, ln)

    def fetch():
        torch.cuda.synchronize()
        r = b.results()
        return (r["yhat"].cpu().numpy().reshape(n, h), r["lower"].cpu().numpy().reshape(n, h), r["upper"].cpu().numpy().reshape(n, h),
                r["model_code"].cpu().numpy(), r["status"].cpu().numpy())
    b.set_exog(x, f)
    b.run()
    yh, lo, hi, code, status = fetch()
    coef = b.exog_coefficients()
    for s in range(n):
        assert (status[s] == 0) == host[s]["ok"], (s, status[s], host[s])
        if not host[s]["ok"]:
            assert status[s] == lib.INSUFFICIENT_DATA and np.isnan(yh[s]).all()
            continue
        assert code[s] == lib.MODEL_CODE_ARIMAX and b.model_name(int(code[s])) == "ARIMAX" and b.model_name(int(code[s]), s) == "ARIMAX"
        assert _same(yh[s], host[s]["point"]) and _same(lo[s], host[s]["lower"]) and _same(hi[s], host[s]["upper"])
        assert coef["intercept"][s] == host[s]["intercept"] and _same(coef["beta"][s], host[s]["beta"]) and np.array_equal(coef["used"][s], host[s]["used"])
    b.set_exog(None)
    b.run()
    yh, lo, hi, code, status = fetch()
    for s in range(n):
        assert (status[s] == 0) == plain[s]["ok"]
        if plain[s]["ok"]:
            assert b.model_name(int(code[s]), s) == plain[s]["model_name"] != "ARIMAX"
            assert _same(yh[s], plain[s]["point"]) and _same(lo[s], plain[s]["lower"]) and _same(hi[s], plain[s]["upper"])
    with pytest.raises(RuntimeError):
        b.exog_coefficients()
    b.close()


def test_other_models_ignore_adopted_blocks(env):
    import torch
    api, O, lib, synth = env
    from anofox_forecast_amd.device import DeviceBatch
    T, h, K, n = 120, 5, 2, 100
    series, xs, fs, _ = _parity_batch(synth, K, n=n, T=T, h=h, seed=401)
    o = _opts(lib, "Naive", h)
    plain, _ = api.forecast_batch(series, o)
    y, ln, x, f = _device_blocks(series, xs, fs, T, h)
    b = DeviceBatch(n, T, o, "cuda:0")
    b.set_block(y, ln)
    b.set_exog(x, f)
    b.run()
    torch.cuda.synchronize()
    yh = b.results()["yhat"].cpu().numpy().reshape(n, h)
    code = b.results()["model_code"].cpu().numpy()
    for s in range(n):
        assert _same(yh[s], plain[s]["point"]) and b.model_name(int(code[s])) == "Naive"
    err = lib.AnofoxError()
    import ctypes as C
    assert not b.L.anofox_hip_batch_set_exog_device(b.handle, x.data_ptr(), f.data_ptr(), 9, C.byref(err)) and err.code == lib.COMPUTATION_ERROR
    b.close()


def test_m5_shape_sample(env):
    """4,096 x 1,913 from synth, K = 3, h = 28: points, bounds, coefficients and masks equal the checker's."""
    api, O, lib, synth = env
    n, T, h, K = 4096, 1913, 28, 3
    XF = synth.gen_regressors(synth.SEED_EXOG, 0, n, T, h, K)
    Y = synth.gen_exog_target(synth.SEED_EXOG, 0, n, XF[:, :, :T])
    series = list(Y)
    xs = [list(XF[s, :, :T]) for s in range(n)]
    fs = [list(XF[s, :, T:]) for s in range(n)]
    got, berr = api.forecast_exog_batch(series, xs, fs, _opts(lib, "AutoARIMA", h))
    assert berr["ok"], berr
    ref = _check_against_checker(lib, O, got, series, xs, fs, [None] * n)
    assert ref["used"].all()


# ---------------------------------------------------------------------------------------------------------------------------
# the mirrors of the shipped callers
# ---------------------------------------------------------------------------------------------------------------------------
def test_scalar_mirror_null_cells_and_pair_truncation(env):
    api, O, lib, synth = env
    y = list(Y6) + [25.0, 35.0]
    x = [1.0, None, 1.0, 2.0, 1.0, 2.0, None, 2.0]
    x0 = [0.0 if v is None else v for v in x]
    a = api.ts_forecast_exog(y, [x, x0], [[1.0, None, 1.0]], 3, "AutoARIMA")     # two historical lists, one future list: one pair
    b = api.ts_forecast_exog(y, [x0], [[1.0, 0.0, 1.0]], 3, "AutoARIMA")
    assert a is not None and b is not None and a["model"] == "ARIMAX" and _same(a["point"], b["point"])
    assert _same(a["point"], R.fit(np.array(y), [x0], [[1.0, 0.0, 1.0]])[0])
    yn = list(y)
    yn[3] = None                                                                 # a NULL of the series is interpolated
    c = api.ts_forecast_exog(yn, [x0], [[1.0, 0.0, 1.0]], 3, "ARIMA")
    yi = np.array(y)
    yi[3] = (y[2] + y[4]) / 2.0
    assert c is not None and _same(c["point"], R.fit(yi, [x0], [[1.0, 0.0, 1.0]])[0])
    assert api.ts_forecast_exog(None, [x0], [[1.0, 0.0, 1.0]], 3, "ARIMA") is None
    assert api.ts_forecast_exog(y, [x0], [[1.0, 0.0]], 3, "ARIMA") is None        # future list shorter than the horizon
    assert api.ts_forecast_exog(y, [x0], [[1.0, 0.0, 1.0]], 3, "NoSuchModel") is None


def _by_tables():
    by = GOLDEN["by_case"]
    H, F = by["history"], by["future"]
    return (by, np.array(H["group_id"], dtype=object), np.array(H["date"], dtype="datetime64[us]"), np.array(H["target"]),
            np.array(H["xreg1"]), np.array(F["group_id"], dtype=object), np.array(F["date"], dtype="datetime64[us]"), np.array(F["xreg1"]))


def test_exog_by_replays_the_golden_case(env):
    api, O, lib, synth = env
    by, g, d, t, x, fg, fd, fx = _by_tables()
    out = api.ts_forecast_exog_by(g, d, t, {"xreg1": x}, fg, fd, {"xreg1": fx}, by["frequency"], by["method"], by["horizon"], {})
    assert list(out) == ["id", "forecast_step", "date", "yhat", "yhat_lower", "yhat_upper", "model_name"]
    assert len(set(out["id"])) == by["expect_groups"] and len(out["yhat"]) == by["expect_rows"]
    assert out["id"] == ["A"] * 7 + ["B"] * 7 and out["forecast_step"].tolist() == list(range(1, 8)) * 2
    assert set(out["model_name"]) == {"ARIMAX"}
    assert out["date"][0] == np.datetime64("2023-01-21T00:00:00") and out["date"][6] == np.datetime64("2023-01-27T00:00:00")
    for k, grp in enumerate(("A", "B")):
        sel = g == grp
        o = np.argsort(d[sel], kind="stable")
        fo = np.argsort(fd[fg == grp], kind="stable")
        point = R.fit(t[sel][o], [x[sel][o]], [fx[fg == grp][fo]])[0]
        lo, hi = R.intervals(t[sel][o], point, 0.95)
        assert _same(out["yhat"][7 * k:7 * k + 7], point) and _same(out["yhat_lower"][7 * k:7 * k + 7], lo) and _same(out["yhat_upper"][7 * k:7 * k + 7], hi)


def test_exog_by_group_without_future_rows_and_regressor_order(env):
    api, O, lib, synth = env
    by, g, d, t, x, fg, fd, fx = _by_tables()
    rng = np.random.default_rng(3)
    x2 = rng.normal(0, 1, len(x))
    fx2 = rng.normal(0, 1, len(fx))
    keep = fg == "A"                                            # group B is absent from the future table
    # rows shuffled: every list is built in date order; the dicts are given in different orders: lists are ordered by column name
    p = rng.permutation(len(g))
    out = api.ts_forecast_exog_by(g[p], d[p], t[p], {"b_promo": x2[p], "a_price": x[p]}, fg[keep], fd[keep],
                                  {"a_price": fx[keep], "b_promo": fx2[keep]}, "1 day", "ARIMA", 7)
    assert out["id"] == ["A"] * 7 + ["B"] * 7
    assert out["model_name"][:7] == ["ARIMAX"] * 7 and out["model_name"][7:] == ["ARIMA"] * 7
    sel = g == "A"
    point = R.fit(t[sel], [x[sel], x2[sel]], [fx[keep], fx2[keep]])[0]
    assert _same(out["yhat"][:7], point)
    plain = api.forecast_series(t[g == "B"], _opts(lib, "ARIMA", 7))
    assert _same(out["yhat"][7:], plain["point"]) and _same(out["yhat_upper"][7:], plain["upper"])
    # pairs are positional after the sort by name: a future table with fewer columns keeps the first pairs only
    out1 = api.ts_forecast_exog_by(g, d, t, {"b_promo": x2, "a_price": x}, fg, fd, {"zz": fx}, "1d", "ARIMA", 7)
    assert _same(out1["yhat"][:7], R.fit(t[sel], [x[sel]], [fx[fg == "A"]])[0])
    # a future list that is not `horizon` long: the scalar returns NULL, the group yields no rows
    out2 = api.ts_forecast_exog_by(g, d, t, {"a_price": x}, fg[:-1], fd[:-1], {"a_price": fx[:-1]}, "1d", "ARIMA", 7)
    assert out2["id"] == ["A"] * 7
    # dates: last date truncated to seconds, fixed-length steps; calendar frequencies are refused loudly
    d2 = d + np.timedelta64(123456, "us")
    out3 = api.ts_forecast_exog_by(g, d2, t, {"a_price": x}, fg, fd, {"a_price": fx}, "12h", "ARIMA", 7)
    assert out3["date"][0] == np.datetime64("2023-01-20T12:00:00") and out3["date"][1] == np.datetime64("2023-01-21T00:00:00")
    for freq in ("1mo", "1q", "1y"):
        with pytest.raises(api.InvalidInputException):
            api.ts_forecast_exog_by(g, d, t, {"a_price": x}, fg, fd, {"a_price": fx}, freq, "ARIMA", 7)
