"""The reference side of tests/test_gpu_inspect.py, pinned without a GPU: on exactly the inputs the GPU tests use, the oracle's
inspection record (oracle.ets_inspect) meets the high-precision identities of tests/inspect_ref.py -- its SSE is the sum of squared
one-step errors of its own fitted values, its criteria follow from that sum, and the textbook forecast function applied to its
final states gives the forecasts the oracle's forecast path returns.  So what the GPU assertions test is the kernels, not the
formulas.  Worst deviations measured when this was written: SSE 1.4e-15 (m = 70 with 387 observations, the longest sum of squares
here; 8.7e-16 at m = 7), criteria 4.6e-16, forecast from states 8.0e-16 (MAdM at h = 17: the power of a damped growth rate; 5.1e-16
elsewhere) -- rounding of fp64 sums and powers against their 80-bit values, three orders below the 1e-12 asserted."""
import numpy as np
import pytest

import inspect_cases as K
import inspect_ref as R


def _report(what, worst):
    print(f"{what}: worst identity deviations " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(worst.items())))


@pytest.mark.parametrize("spec", R.SPECS)
def test_every_spec_oracle_record_meets_the_identities(oracle, spec):
    O = oracle
    series, m, h = K.every_spec(spec)
    worst = {}
    for s, y in enumerate(series):
        ref = K.oracle_record(O, ("spec", spec, s), y, m, R.spec_id(spec))
        fc = K.oracle_forecast(O, ("spec", spec, s), y, None, "ETS", h, ets_model=spec, seasonal_period=m)
        assert ref is not None and fc["ok"] and ref["spec_id"] == R.spec_id(spec), (spec, s, fc)
        assert not np.any(np.isnan(ref["fitted_values"])) and len(ref["fitted_values"]) == len(y)
        K.check_identities(ref, y, spec, m, fc["point"], worst, s)
    _report(spec, worst)


@pytest.mark.parametrize("period", K.RING_PERIODS)
def test_ring_class_oracle_record_meets_the_identities(oracle, period):
    O = oracle
    series, h = K.ring_class(period)
    worst = {}
    for spec in K.RING_SPECS:
        fitted = 0
        for s, y in enumerate(series):
            ref = K.oracle_record(O, ("ring", period, spec, s), y, period, R.spec_id(spec))
            fc = K.oracle_forecast(O, ("ring", period, spec, s), y, None, "ETS", h, ets_model=spec, seasonal_period=period)
            if len(y) < 2 * period:
                assert ref is None and not fc["ok"], (period, spec, s, fc)         # one season short: the forecast path says so
                continue
            assert (ref is not None) == fc["ok"], (period, spec, s, fc)
            if ref is None:
                continue
            assert len(ref["seasonal_states"]) == period
            K.check_identities(ref, y, spec, period, fc["point"], worst, (spec, s))
            fitted += 1
        assert fitted >= 21, (period, spec, fitted)        # (a few AMdA fits end with a likelihood that is not finite: an error on both paths)
    _report(f"m = {period}", worst)


@pytest.mark.parametrize("period", [7, 1])
def test_autoets_oracle_record_meets_the_identities(oracle, period):
    O = oracle
    series, valids, kind = K.auto_mixed()
    worst, fitted, multiplicative = {}, 0, 0
    for s, (y, v) in enumerate(zip(series, valids)):
        yc = K.clean(O, y, v)
        ref = K.oracle_record(O, ("auto", period, s), yc, period)
        fc = K.oracle_forecast(O, ("auto", period, s), y, v, "AutoETS", 2 * period + 3, seasonal_period=period)
        spec = R.notation_of_name(fc["model_name"]) if fc["ok"] else None
        if spec is None:                                       # an error or the fallback chain: nothing to inspect
            assert ref is None, (period, s, kind[s], fc)
            continue
        assert ref is not None and R.notation_of(ref["spec_id"]) == spec, (period, s, kind[s], fc["model_name"], ref)
        K.check_identities(ref, yc, spec, period, fc["point"], worst, (s, kind[s]))
        fitted += 1
        multiplicative += "M" in spec
    assert fitted >= 135 and multiplicative >= 10, (fitted, multiplicative)
    _report(f"AutoETS m = {period}", worst)


def test_arima_criteria_of_the_oracle_fit(oracle):
    """aicc of oracle_auto_arima_detail is n log(sigma2) + 2 k + 2 k (k + 1) / (n - k - 1) of its own sigma2 and n_used
    (oracle/arima.c css_criterion): the aic / bic the GPU test derives from it in extended precision are the fit's."""
    O = oracle
    worst = 0.0
    for m in (7, 1):
        for s, y in enumerate(K.arima(m)):
            got = K.arima_detail(O, y, m, 3)
            assert got is not None, (m, s)
            fit = got[0]
            o = fit.ord
            k = o.p + o.q + o.P + o.Q + o.with_constant + 1
            n = fit.n_used
            assert 0 < n <= len(y) - o.d - o.D * o.s, (m, s, n)
            aic, bic = R.arima_criteria(fit.aicc, k, n)
            aic_direct = R.LD(n) * np.log(R.LD(fit.sigma2)) + R.LD(2) * R.LD(k)
            worst = max(worst, R.dev(aic, aic_direct))
            assert np.isfinite(float(bic))
    print(f"AutoARIMA: aic from aicc against n log(sigma2) + 2 k, worst {worst:.2e}")
    assert worst <= K.REL_TOL, worst
