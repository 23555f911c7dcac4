"""CPU: the ARIMAX definition (tests/exog_ref.py, the numpy checker the kernels of csrc/fit_exog.hip follow bit for bit) against a
hand-derived case, numpy.linalg.lstsq and the oracle's ARIMA; the layout of the three exogenous structs against the reference's
measured offsets; the exported symbols; and the entries' behaviour without a GPU (argument errors first, no CPU fallback)."""
import ctypes as C
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import exog_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "exog_cases.json")))

Y6 = np.array([10.0, 20.0, 15.0, 25.0, 20.0, 30.0])
X6 = np.array([1.0, 2.0, 1.0, 2.0, 1.0, 2.0])


def test_hand_derived_case():
    """y = [10,20,15,25,20,30] on x = [1,2,1,2,1,2]: means 20 and 1.5, S = 1.5, g = 15 -> beta = 10, b0 = 5; residuals
    [-5,-5,0,0,5,5], mean difference 10 / 5 = 2, last difference 0 -> differences 1, 1.5 -> residual forecasts 6, 7.5; effects
    5 + 10 * [1, 2] -> [21.0, 32.5]."""
    point, b0, beta, used = R.fit(Y6, [X6], [[1.0, 2.0]])
    assert used.tolist() == [True]
    assert abs(beta[0] - 10.0) <= 1e-12 and abs(b0 - 5.0) <= 1e-12
    assert np.max(np.abs(point - np.array([21.0, 32.5]))) <= 1e-12
    case = [c for c in GOLDEN["scalar_cases"] if "expect_point" in c][0]
    p2 = R.fit(case["values"], case["xreg"], case["future_xreg"])[0]
    assert np.max(np.abs(p2 - np.array(case["expect_point"]))) <= 1e-12


def test_short_series_take_the_naive_branch_and_the_error():
    """n < 5: the residual forecast is the last residual (forecast.rs:1391-1431); n < 3 is InsufficientData in the entries."""
    y = np.array([3.0, 5.0, 4.0, 8.0])
    x = np.array([1.0, 2.0, 1.5, 3.0])
    point, b0, beta, used = R.fit(y, [x], [[2.0, 2.5, 4.0]])
    r = R.residuals(y, [x], b0, beta, used)
    expect = r[-1] + (b0 + beta[0] * np.array([2.0, 2.5, 4.0]))
    assert np.array_equal(point, expect)
    assert np.array_equal(R.toy_arima(r, 3), np.full(3, r[-1]))


def _generator_case(rng, n, K, h):
    t = np.arange(n + h)
    cols = []
    for j in range(K):
        kind = j % 4
        if kind == 0:
            c = 5 + rng.normal(0, 0.5) + np.cumsum(rng.normal(0, 0.05, n + h))
        elif kind == 1:
            c = (rng.random(n + h) < 0.2).astype(float)
        elif kind == 2:
            c = 15 + 10 * np.sin(2 * np.pi * t / 365 + rng.uniform(0, 6)) + rng.normal(0, 2, n + h)
        else:
            c = (t % 7 == int(rng.integers(0, 7))).astype(float)
        cols.append(c)
    XF = np.array(cols)
    X, F = XF[:, :n], XF[:, n:]
    y = np.round(np.maximum(0, 20 + 0.02 * t[:n] - 2 * (X[0] - 5) + (4 * X[1] if K > 1 else 0) + rng.normal(0, 2, n)))
    return y, X, F


def _lstsq_forecast(y, X, F, h):
    n = len(y)
    A = np.column_stack([np.ones(n)] + [X[j] for j in range(X.shape[0])])
    c = np.linalg.lstsq(A, y, rcond=None)[0]
    r = y - A @ c
    eff = c[0] + (F.T @ c[1:] if X.shape[0] else 0.0)
    return R.toy_arima(r, h) + eff


def test_checker_against_lstsq():
    """300 cases of the M5-like generator (seed 20261016; n 12-400, K 1-8, h 14): every forecast point within 1e-9 of numpy's
    SVD least squares with an explicit intercept column, relative to max(1, |point|).  A column that is constant over the history is
    aliased with the intercept: lstsq is then given the design without it (every tenth case has an all-zero flag).  Nothing is
    skipped.  Measured: worst 5.2e-14."""
    rng = np.random.default_rng(20261016)
    worst, n_const = 0.0, 0
    for trial in range(300):
        n = int(rng.integers(12, 401))
        K = int(rng.integers(1, 9))
        h = 14
        y, X, F = _generator_case(rng, n, K, h)
        if trial % 10 == 0 and K > 1:
            X[1, :] = 0.0                  # a promotion flag that never fired in the history (its future values still vary)
        point, b0, beta, used = R.fit(y, X, F)
        const = np.array([np.ptp(X[j]) == 0 for j in range(K)])
        n_const += int(const.any())
        assert not used[const].any()
        ref = _lstsq_forecast(y, X[~const], F[~const], h)
        rel = float(np.max(np.abs(point - ref) / np.maximum(1.0, np.abs(ref))))
        print(f"trial {trial} n {n} K {K} const {int(const.sum())} rel {rel:.3e}")
        worst = max(worst, rel)
        assert rel <= 1e-9, (trial, n, K, rel)
    print("worst", worst, "cases with a constant column", n_const)


def test_aliased_regressors_are_left_out():
    rng = np.random.default_rng(7)
    n = 50
    x1 = rng.normal(0, 1, n)
    y = 3 + 2 * x1 + rng.normal(0, 0.1, n)
    fut = [[0.5, 1.0]] * 4
    point, b0, beta, used = R.fit(y, [x1, np.full(n, 4.0), x1.copy(), 2 * x1 + 1], fut)
    assert used.tolist() == [True, False, False, False]
    alone = R.fit(y, [x1], fut[:1])
    assert np.array_equal(point, alone[0]) and b0 == alone[1] and beta[0] == alone[2][0]
    assert beta[1:].tolist() == [0.0, 0.0, 0.0]
    # a non-finite historical value: the regressor is skipped everywhere, NaN never reaches the result
    bad = x1.copy()
    bad[3] = np.nan
    p2, b2, be2, u2 = R.fit(y, [bad, x1, np.full(n, np.inf)], [[9.0, 9.0], [0.5, 1.0], [1.0, 1.0]])
    assert u2.tolist() == [False, True, False]
    assert np.array_equal(p2, alone[0]) and b2 == alone[1]
    # all-zero regressor alone: the plain ARIMA forecast of y - mean, plus the mean
    p3, b3, be3, u3 = R.fit(y, [np.zeros(n)], [[1.0, 1.0]])
    assert u3.tolist() == [False] and np.isfinite(p3).all()
    # a non-finite FUTURE value of a used regressor propagates into that step only
    p4 = R.fit(y, [x1], [[np.nan, 1.0]])[0]
    assert np.isnan(p4[0]) and p4[1] == alone[0][1]


def test_eight_regressors_and_more_regressors_than_observations():
    rng = np.random.default_rng(11)
    y, X, F = _generator_case(rng, 200, 8, 14)
    point, b0, beta, used = R.fit(y, X, F)
    assert used.all() and np.isfinite(point).all()
    # n <= K: the Gram matrix has rank <= n - 1, the trailing columns are aliased; results stay finite
    for n in (3, 4, 5, 8):
        Xs = rng.normal(0, 1, (8, n))
        ys = rng.normal(10, 2, n)
        p, b, be, u = R.fit(ys, Xs, rng.normal(0, 1, (8, 3)))
        assert int(u.sum()) <= n - 1 and np.isfinite(p).all() and np.isfinite(b), (n, u)


def test_batch_form_equals_the_single_series_form():
    """fit_batch vectorises over the series axis only: a ragged batch gives every series the bits of its own fit."""
    rng = np.random.default_rng(5)
    series, xs, fs = [], [], []
    for s in range(40):
        n = int(rng.integers(1, 60))
        y, X, F = _generator_case(rng, n, 3, 5)
        series.append(y); xs.append(list(X)); fs.append(list(F))
    got = R.fit_batch(series, xs, fs)
    for s in range(40):
        p, b0, beta, used = R.fit(series[s], xs[s], fs[s])
        assert np.array_equal(got["point"][s], p, equal_nan=True)
        assert np.array_equal(got["beta"][s], beta) and np.array_equal(got["used"][s], used)


def test_residual_stage_equals_the_oracle_arima(oracle):
    """The checker's residual forecast is the oracle's `ARIMA` forecast of the same residual series, bit for bit."""
    O = oracle
    rng = np.random.default_rng(3)
    for n in (3, 4, 5, 6, 17, 120, 400):
        y, X, F = _generator_case(rng, n, 3, 9)
        point, b0, beta, used = R.fit(y, X, F)
        r = R.residuals(y, X, b0, beta, used)
        ref = O.forecast(r, O.make_options("ARIMA", 9))
        assert ref["ok"], ref
        assert np.array_equal(R.toy_arima(r, 9), ref["point"]), n


# sizes and offsets measured with gcc on the reference's src/include/anofox_fcst_ffi.h:1152-1249
EXOG_LAYOUT = "32 0 8 16 24\n16 0 8\n192 0 32 40 48 56 60 61 62 64 72 76 140 172 188"


def test_exog_struct_layout_matches_the_reference(hiplib):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "anofox_fcst_hip.h"
#define O(f) offsetof(ForecastOptionsExog, f)
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", sizeof(ExogenousRegressor), offsetof(ExogenousRegressor, values), offsetof(ExogenousRegressor, n_values),
         offsetof(ExogenousRegressor, future_values), offsetof(ExogenousRegressor, n_future));
  printf("%zu %zu %zu\n", sizeof(ExogenousData), offsetof(ExogenousData, regressors), offsetof(ExogenousData, n_regressors));
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(ForecastOptionsExog), O(model), O(ets_model), O(horizon),
         O(confidence_level), O(seasonal_period), O(auto_detect_seasonality), O(include_fitted), O(include_residuals), O(exog), O(window),
         O(seasonal_periods_str), O(model_pool), O(laplace_variant), O(laplace_seasonal_batch_init));
  return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = subprocess.check_output([os.path.join(d, "t")]).decode().strip()
    assert out == EXOG_LAYOUT
    E = hiplib.ForecastOptionsExog
    assert (C.sizeof(hiplib.ExogenousRegressor), C.sizeof(hiplib.ExogenousData), C.sizeof(E)) == (32, 16, 192)
    assert [getattr(E, f).offset for f, _ in E._fields_] == [0, 32, 40, 48, 56, 60, 61, 62, 64, 72, 76, 140, 172, 188]


def test_library_exports_the_exog_entries(hiplib):
    L = hiplib.load()
    for sym in ("anofox_ts_forecast_exog", "anofox_ts_forecast_exog_batch", "anofox_hip_batch_set_exog_device",
                "anofox_hip_batch_exog_coefficients"):
        assert sym in hiplib.EXPORTED_SYMBOLS and hasattr(L, sym), sym


def test_argument_errors_come_first(hiplib):
    """Model name, regressor lengths, series length -- in the reference's order -- and the cap of 8, GPU or not."""
    from anofox_forecast_amd import api
    o = lambda m, h=2: hiplib.make_options(m, h, auto_detect=False)
    r = api.forecast_series_exog(Y6, [X6], [[1.0, 2.0]], o("NoSuchModel"))
    assert r["code"] == hiplib.INVALID_MODEL and r["message"] == "Invalid model: Unknown model: 'NoSuchModel'"
    r = api.forecast_series_exog(Y6, [X6[:5]], [[1.0, 2.0]], o("NoSuchModel"))
    assert r["code"] == hiplib.INVALID_MODEL                     # the model name wins over a bad regressor
    r = api.forecast_series_exog(Y6, [X6, X6[:5]], [[1.0, 2.0], [1.0, 2.0]], o("ARIMA"))
    assert r["code"] == hiplib.INVALID_INPUT and r["message"] == "Invalid input: Exogenous regressor 1 has 5 values but y has 6 values"
    r = api.forecast_series_exog(Y6, [X6], [[1.0, 2.0, 3.0]], o("ARIMA"))
    assert r["code"] == hiplib.INVALID_INPUT and r["message"] == "Invalid input: Exogenous regressor 0 has 3 future values but horizon is 2"
    r = api.forecast_series_exog(Y6[:2], [X6[:2]], [[1.0, 2.0]], o("ARIMA"))
    assert r["code"] == hiplib.INSUFFICIENT_DATA and r["message"] == "Insufficient data: need at least 3 observations, got 2"
    r = api.forecast_series_exog([], [[]], [[1.0, 2.0]], o("ARIMA"))
    assert r["code"] == hiplib.INSUFFICIENT_DATA and r["message"] == "Insufficient data: need at least 1 observations, got 0"
    r = api.forecast_series_exog(Y6, [X6] * 9, [[1.0, 2.0]] * 9, o("AutoARIMA"))
    assert r["code"] == hiplib.COMPUTATION_ERROR and r["message"] == "Computation error: ARIMAX takes at most 8 exogenous regressors, got 9"
    for m, x in (("OptimizedTheta", "ThetaX"), ("DynamicTheta", "ThetaX"), ("MFLES", "MFLESX"), ("AutoMFLES", "MFLESX")):
        r = api.forecast_series_exog(Y6, [X6], [[1.0, 2.0]], o(m))
        assert r["code"] == hiplib.INTERNAL_ERROR, (m, r)
        assert r["message"] == f"Internal error: model '{m}' with exogenous regressors ({x}) is not implemented by the HIP backend"
    err = hiplib.AnofoxError()
    L = hiplib.load()
    assert not L.anofox_ts_forecast_exog(None, None, 0, None, None, C.byref(err)) and err.code == hiplib.NULL_POINTER
    assert err.message == b"Null pointer argument"
    assert not L.anofox_ts_forecast_exog_batch(None, None, None, 0, None, 0, None, None, None, None, C.byref(err), None, None)
    assert err.code == hiplib.NULL_POINTER
    assert not L.anofox_hip_batch_set_exog_device(None, None, None, 0, C.byref(err)) and err.code == hiplib.NULL_POINTER
    assert not L.anofox_hip_batch_exog_coefficients(None, None, None, None, C.byref(err)) and err.code == hiplib.NULL_POINTER


def test_no_gpu_fails_loudly(hiplib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from anofox_forecast_amd import api
    o = hiplib.make_options("ARIMA", 2, auto_detect=False)
    r = api.forecast_series_exog(Y6, [X6], [[1.0, 2.0]], o)
    assert not r["ok"] and r["code"] == hiplib.INTERNAL_ERROR and "no CPU fallback" in r["message"]
    res, berr = api.forecast_exog_batch([Y6, Y6[:2]], [[X6], [X6[:2]]], [[[1.0, 2.0]]] * 2, o)
    assert not berr["ok"] and berr["code"] == hiplib.INTERNAL_ERROR and "no CPU fallback" in berr["message"]
    assert res[0]["code"] == hiplib.INTERNAL_ERROR and res[1]["code"] == hiplib.INSUFFICIENT_DATA
    assert api.ts_forecast_exog(list(Y6), [list(X6)], [[1.0, 2.0]], 2, "ARIMA") is None
    # without regressors the entry is the ordinary one
    r = api.forecast_series_exog(Y6, [], [], hiplib.make_options("Naive", 2))
    assert not r["ok"] and r["code"] == hiplib.INTERNAL_ERROR and "no CPU fallback" in r["message"]


def test_golden_file_is_data_only():
    assert len(GOLDEN["scalar_cases"]) == 8
    by = GOLDEN["by_case"]
    assert len(by["history"]["target"]) == 40 and len(by["future"]["xreg1"]) == 14
    assert by["expect_groups"] == 2 and by["expect_rows"] == 14
    for c in GOLDEN["scalar_cases"]:
        assert c["source"].startswith("test/sql/ts_forecast_exog.test:")
        assert all(len(x) == len(c["values"]) for x in c["xreg"]) and all(len(f) == c["horizon"] for f in c["future_xreg"])


def test_regressor_generator_is_seeded_and_sliceable():
    """synth.gen_regressors / gen_exog_target: the same (seed, range) gives the same values, a sub-range is a slice of the range."""
    from anofox_forecast_amd import synth
    a = synth.gen_regressors(synth.SEED_EXOG, 1000, 60, 50, 7, 8)
    b = synth.gen_regressors(synth.SEED_EXOG, 1000, 60, 50, 7, 8)
    assert a.shape == (60, 8, 57) and np.array_equal(a, b)
    assert np.array_equal(synth.gen_regressors(synth.SEED_EXOG, 1020, 30, 50, 7, 8), a[20:50])      # (crosses a block of 1,024)
    assert set(np.unique(a[:, 1])) <= {0.0, 1.0} and set(np.unique(a[:, 3])) <= {0.0, 1.0} and set(np.unique(a[:, 7])) <= {0.0, 1.0}
    y = synth.gen_exog_target(synth.SEED_EXOG, 1000, 60, a[:, :, :50])
    assert y.shape == (60, 50) and np.array_equal(y, np.round(y)) and (y >= 0).all()
    assert np.array_equal(y, synth.gen_exog_target(synth.SEED_EXOG, 1000, 60, a[:, :, :50]))
    yr = synth.gen_exog_target(synth.SEED_EXOG, 1000, 60, a[:, :, :50], real_valued=True)
    assert not np.array_equal(yr, np.round(yr))
