"""CPU: the MSTL decomposition / SeasonalWindowAverage checker (tests/mstl_ref.py) against the properties of the reference's Rust
unit tests (decomposition.rs:321-368) and its decomposition SQL tests, the MSTL pin outcome, hand-computed
SeasonalWindowAverage cases, and the MstlResult layout of the public header."""
import json
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import mstl_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "mstl_kats.json")))


def _sine_trend(n=120, p=12):
    i = np.arange(n, dtype=np.float64)
    return 0.1 * i + 5.0 * np.sin(2.0 * math.pi * i / p)


def test_rust_unit_test_properties():
    y = _sine_trend()
    d = R.mstl_decompose(y, [12], R.FAIL)
    assert d["applied"] and len(d["trend"]) == 120 and len(d["seasonal"]) == 1 and len(d["seasonal"][0]) == 120
    assert len(d["remainder"]) == 120 and d["periods"] == [12]
    assert "error" in R.mstl_decompose([1.0, 2.0, 3.0], [12], R.FAIL)
    d = R.mstl_decompose([1.0, 2.0, 3.0, 4.0, 5.0], [12], R.TREND)
    assert d["applied"] and d["trend"] is not None and d["seasonal"] == [] and d["remainder"] is not None
    d = R.mstl_decompose([1.0, 2.0], [12], R.NONE)
    assert not d["applied"] and d["trend"] is None and d["seasonal"] == [] and d["remainder"] is None


def test_decomposition_is_additive_and_the_seasonals_periodic():
    rng = np.random.default_rng(3)
    y = 50.0 + _sine_trend(400, 7) + 3.0 * np.sin(2.0 * math.pi * np.arange(400) / 30.0) + rng.normal(0, 0.5, 400)
    d = R.mstl_decompose(y, [7, 30])
    assert d["periods"] == [30, 7]                          # longest first
    recon = d["trend"] + d["seasonal"][0] + d["seasonal"][1] + d["remainder"]
    assert np.allclose(recon, y, rtol=0, atol=1e-9)
    for comp, p in zip(d["seasonal"], d["periods"]):
        assert np.array_equal(comp[p:], comp[:-p])          # exactly periodic
        assert abs(comp.mean()) < 1e-9                       # centred
    # a period without two seasons is skipped, a period below 2 is ignored
    d = R.mstl_decompose(y[:50], [1, 7, 30])
    assert d["periods"] == [7]


def test_insufficient_data_modes_and_edges():
    assert R.mstl_decompose([], [7], R.FAIL) == {"error": (1, 0)}
    assert not R.mstl_decompose([], [7], R.TREND)["applied"]
    assert R.mstl_decompose(np.arange(10.0), [7], R.FAIL) == {"error": (14, 10)}
    d = R.mstl_decompose(np.arange(10.0), [7], R.TREND)
    assert d["periods"] == [] and np.all(np.isfinite(d["trend"]))
    # the trend-only branch divides an even window's 2 hw + 1 values by the window (literal): n = 20 -> window 4
    y = np.arange(20.0) ** 2
    d = R.mstl_decompose(y, [])
    assert d["trend"][10] == R._seqsum(y[8:13]) / 4.0
    # ... the final-trend branch by the number of values summed
    d = R.mstl_decompose(y, [1])
    assert d["trend"][10] == R._seqsum(y[8:13]) / 5.0
    # no full window: the trend stays NaN, as in the reference
    d = R.mstl_decompose([1.0, 2.0], [])
    assert np.all(np.isnan(d["trend"]))


MODEL_FORECASTERS = ("SESOptimized", "Holt", "AutoETS", "Naive", "RandomWalkDrift", "AutoARIMA")


def test_mstl_pin_is_not_met_so_mstl_keeps_its_error(oracle):
    """no candidate -- (a)-(d) on the reference's decomposition, (e) on LOESS STL decompositions -- comes within
    1e-4 relative of the pin; MSTL and AutoMSTL stay errors."""
    O = oracle
    y = np.array(KATS["distinctness_series"]["y"])
    pin = KATS["pins"]["MSTL_point_1"]
    cands, bases = R.mstl_candidates(y, KATS["distinctness_series"]["default_periods"], 3)
    for tag, (des, seas) in bases.items():
        for m in MODEL_FORECASTERS:
            r = O.forecast(des, O.make_options(m, 3, seasonal_period=0, auto_detect=False))
            assert r["ok"], (tag, m)
            cands[f"{tag}: {m} of the deseasonalised series"] = r["point"] + seas
    rel = {k: abs(float(v[0]) / pin - 1.0) for k, v in cands.items()}
    best = min(rel, key=rel.get)
    assert rel[best] > 1e-4, (best, cands[best][0])
    # the figures DESIGN section 7 quotes
    assert round(float(bases["moving average"][1][0]), 6) == -2.538462
    assert round(float(cands["moving average: final trend held flat"][0]), 6) == 15.538462
    assert round(float(cands["moving average: AutoETS of the deseasonalised series"][0]), 6) == 16.214616
    assert round(float(cands["LOESS STL s_window 11 degree 1: AutoETS of the deseasonalised series"][0]), 6) == 18.0
    assert round(float(cands["LOESS STL s_window 11 degree 0: AutoETS of the deseasonalised series"][0]), 6) == 16.943779
    assert best == "LOESS STL s_window 7 degree 0: OLS line through the deseasonalised series"
    assert round(float(cands[best][0]), 6) == 17.370598 and 3e-4 < rel[best] < 4e-4


def test_loess_stl_recovers_a_clean_season():
    """The LOESS STL of candidate (e) on a noiseless sine plus a line: the seasonal part is the sine, the trend the line."""
    t = np.arange(96, dtype=np.float64)
    y = 0.2 * t + 3.0 * np.sin(2 * np.pi * t / 12)
    tr, sl = R.stl_loess(y, 12, 11, 1)
    assert np.max(np.abs(sl[12:-12] - 3.0 * np.sin(2 * np.pi * t[12:-12] / 12))) < 0.05
    assert np.max(np.abs(tr[12:-12] - 0.2 * t[12:-12])) < 0.05


def test_sql_decomposition_properties():
    """ts_decomposition.test: _ts_mstl_decomposition passes no periods (the trend-only branch)."""
    lin = np.arange(1.0, 13.0)
    d = R.mstl_decompose(lin, [])
    assert len(d["trend"]) == 12 and len(d["remainder"]) == 12 and not np.isnan(d["trend"][0])
    assert d["trend"][11] > d["trend"][0]
    assert abs(d["remainder"][5]) < 5.0
    assert abs(R.mstl_decompose(np.full(12, 5.0), [])["trend"][0] - 5.0) < 1.0
    assert len(R.mstl_decompose([10.0, 20.0, 30.0, 40.0] * 4, [])["trend"]) == 16


def test_periods_beyond_any_length():
    """usize arithmetic in the reference: a period of 2^30 or more is simply too long (error, skip or trend only)."""
    y = np.arange(30.0)
    assert R.mstl_decompose(y, [2 ** 30]) == {"error": (2 ** 31, 30)}
    assert R.mstl_decompose(y, [2 ** 31 - 1, 7])["periods"] == [7]
    assert R.mstl_decompose(y, [2 ** 30], R.TREND)["periods"] == []


def test_seasonal_window_average_by_hand():
    y = KATS["swa_series"]["y"]                              # ts_forecast_exp_smoothing.test:328-336
    assert list(R.swa_forecast(y, 3, 6)) == [10.0, 20.0, 30.0, 10.0, 20.0, 30.0]
    # no period: p = 2, 4 complete seasons of the last 8 values
    assert list(R.swa_forecast(y, 1, 3)) == [(20 + 10 + 30 + 20) / 4, (30 + 20 + 10 + 30) / 4, (20 + 10 + 30 + 20) / 4]
    # 10 values, p = 4: the last 2 complete seasons (values 2..9)
    v = np.arange(10.0)
    assert list(R.swa_forecast(v, 4, 5)) == [(2 + 6) / 2, (3 + 7) / 2, (4 + 8) / 2, (5 + 9) / 2, (2 + 6) / 2]
    # a period longer than the series: p = n, one season = the series itself
    assert list(R.swa_forecast([1.0, 2.0, 4.0], 12, 4)) == [1.0, 2.0, 4.0, 1.0]
    assert list(R.swa_fitted([1.0, 2.0, 3.0, 5.0, 7.0], 2)) == [1.0, 2.0, 1.0, 2.0, 2.0]


def test_mstl_result_layout_matches_the_reference_header():
    """anofox_fcst_ffi.h:939-968: MstlResult is byte-compatible (offsets as gcc lays them out)."""
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "anofox_fcst_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(MstlResult), offsetof(MstlResult, trend), offsetof(MstlResult, seasonal_components),
    offsetof(MstlResult, remainder), offsetof(MstlResult, n_observations), offsetof(MstlResult, n_seasonal),
    offsetof(MstlResult, seasonal_periods), offsetof(MstlResult, decomposition_applied));
  return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = subprocess.check_output([os.path.join(d, "t")]).decode().split()
    assert out == ["56", "0", "8", "16", "24", "32", "40", "48"]
    import ctypes as C
    from anofox_forecast_amd import lib
    assert C.sizeof(lib.MstlResult) == 56 and lib.MstlResult.decomposition_applied.offset == 48
