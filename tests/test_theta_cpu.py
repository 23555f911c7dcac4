"""CPU: the dynamic Theta checker (tests/theta_ref.py) against the reference's pins, the textbook recursion, edge cases and the
seasonal path's conventions."""
import json
import os

import numpy as np

import theta_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "theta_kats.json")))
Y24 = np.array(KATS["distinctness_series"]["y"], dtype=np.float64)


def test_checker_meets_the_pins():
    pins = KATS["pins"]["point_1"]
    fc, ok, par, _ = R.forecast([Y24], "DynamicTheta", 3)
    assert round(float(fc[0, 0]), 6) == pins["DynamicTheta"]
    assert not ok[0] and list(par[0]) == [10.0, 0.1, 2.0]
    # DynamicOptimizedTheta: the project's Nelder-Mead stops at (6.5476, 0.2407, 2.0645); the reference's optimiser evidently
    # elsewhere on the same flat valley: 19.348989 against the pin 19.347803 (+6.1e-5 relative)
    fc, _, par, evals = R.forecast([Y24], "DynamicOptimizedTheta", 3)
    dev = KATS["deviations"]["DynamicOptimizedTheta"]
    assert round(float(fc[0, 0]), 6) == dev["point_1"]
    assert abs(float(fc[0, 0]) / pins["DynamicOptimizedTheta"] - 1.0) < dev["max_rel"]
    assert 0.1 <= par[0, 1] <= 0.99 and par[0, 2] >= 1.0 and 0 < evals[0] <= R.NM_MAX
    assert set(KATS["shipped"]) == set(R.MODELS) and set(KATS["not_shipped"]) == set(R.NOT_SHIPPED)


def test_dynamic_trend_is_the_ols_line_of_every_prefix():
    """B_t and A_t of the dynamic recursion are the OLS slope and intercept (time 1..t+1) of y[0..t]."""
    rng = np.random.default_rng(3)
    y = rng.normal(10.0, 3.0, 60) + 0.2 * np.arange(60)
    mean, A, B = y[0], y[0], 0.0
    for t in range(1, len(y)):
        B = ((t - 1) * B + 6.0 * (y[t] - mean) / (t + 1)) / (t + 2)
        mean = (t * mean + y[t]) / (t + 1)
        A = mean - B * (t + 2) / 2.0
        slope, icpt = np.polyfit(np.arange(1, t + 2, dtype=np.float64), y[:t + 1], 1)
        assert abs(B - slope) <= 1e-9 * max(1.0, abs(slope)), t
        assert abs(A - icpt) <= 1e-9 * max(1.0, abs(icpt)), t


def test_running_power_is_the_power():
    alpha = 0.2407
    p, q = 1.0, 1.0 - alpha
    for t in range(1, 200):
        p = p * q
        assert abs(p / q ** t - 1.0) < 1e-12


def test_edge_cases():
    for m in R.MODELS:
        # n = 3 (the shortest the host passes on), a constant series, a ragged pair, an empty series
        fc, _, _, _ = R.forecast([np.array([1.0, 2.0, 3.0]), np.full(17, 4.0), np.array([]), np.arange(1.0, 41.0)], m, 5)
        assert np.all(np.isfinite(fc[[0, 1, 3]])) and np.all(np.isnan(fc[2])), m
        assert np.all(np.diff(fc[3]) > 0), m                             # an increasing line keeps increasing
    # DynamicOptimizedTheta holds a constant series (theta = 1 removes the drift term)
    c = KATS["sql_cases"]["constant10"]
    fc, _, par, _ = R.forecast([np.full(c["n"], c["value"])], "DynamicOptimizedTheta", 3)
    assert np.all(np.abs(fc[0] - c["value"]) < c["within"])
    # a batch answers every series as alone
    many = [Y24, np.arange(1.0, 31.0), np.array([5.0, 1.0, 4.0, 2.0])]
    for m in R.MODELS:
        together = R.forecast(many, m, 4)[0]
        for s, y in enumerate(many):
            assert np.array_equal(R.forecast([y], m, 4)[0][0], together[s]), (m, s)


def test_seasonal_path_conventions():
    t = np.arange(84, dtype=np.float64)
    pattern = np.array([1.3, 0.8, 0.9, 1.1, 1.0, 0.7, 1.2])
    y = (50.0 + 0.3 * t) * pattern[np.arange(84) % 7]
    idx, ok = R.season_indices(*R._as_block([y]), 7)
    assert ok[0] and abs(idx[0].mean() - 1.0) < 1e-12
    assert np.max(np.abs(idx[0] / pattern * pattern.mean() - 1.0)) < 0.02
    # not adjusted: a non-positive value, fewer than 2m observations, no seasonality at lag m, m = 1
    y0 = y.copy(); y0[5] = 0.0
    assert not R.season_indices(*R._as_block([y0]), 7)[1][0]
    assert not R.season_indices(*R._as_block([y[:13]]), 7)[1][0]
    assert not R.season_indices(*R._as_block([np.random.default_rng(5).normal(50.0, 1.0, 84)]), 7)[1][0]
    for m in R.MODELS:
        fc, ok, _, _ = R.forecast([y, y0], m, 14, period=7)
        assert ok[0] and not ok[1]
        # the forecasts carry the pattern: their ratio one season apart is the index ratio of the trend, near 1
        assert np.max(np.abs(fc[0, 7:] / fc[0, :7] - 1.0)) < 0.1, m
        assert np.array_equal(fc[1], R.forecast([y0], m, 14)[0][0]), m        # unadjusted: the non-seasonal fit
