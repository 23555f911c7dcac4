"""CPU: the restatement tests/seasonality_ref.py of detect_seasonality / analyze_seasonality / compute_trend_strength against
hand-derived answers and the golden statements of tests/golden/seasonality_kats.json; the case list's own claims (ties, the fast form
of the lag sums); the SeasonalityResult layout; the NULL-pointer paths and the free functions of the C entries, none of which reaches
the GPU.  This restatement is the yardstick of tests/test_gpu_seasonality.py."""
import ctypes as C
import json
import os

import pytest

import seasonality_cases as SC
import seasonality_ref as R

KATS = SC.load_kats()


def test_golden_file_is_what_its_script_writes(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_seasonality_kats", os.path.join(SC.HERE, "golden", "make_seasonality_kats.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.HERE = str(tmp_path)
    mod.main()
    with open(tmp_path / "seasonality_kats.json") as fh:
        assert json.load(fh) == KATS


@pytest.mark.parametrize("st", KATS["statements"], ids=lambda st: f'{st["function"]}@{st["src"].split("/")[-1]}')
def test_golden_statements(st):
    assert SC.golden_holds(st, R.scalar_detect, R.scalar_analyze), st["src"]


def test_hand_derived():
    # [10, 20, 30, 40] x 4: mean 25, d = (-15, -5, 5, 15) repeated; lag 4 pairs every d with itself, 12 of the 16 squares: 0.75
    r = R.analyze([10.0, 20.0, 30.0, 40.0] * 4)
    assert r["detected_periods"] == [4] and r["primary_period"] == 4 and r["strengths"] == [0.75] and r["is_seasonal"]
    assert r["trend_strength"].hex() == "0x1.f0b6848d2af1cp-3"
    # [1, 2, 3, 4] x 3: 8 of the 12 squares
    r = R.analyze([1.0, 2.0, 3.0, 4.0] * 3)
    assert r["detected_periods"] == [4] and r["seasonal_strength"].hex() == "0x1.5555555555555p-1"
    assert r["trend_strength"].hex() == "0x1.4ba5ec939f6ffp-2"
    # a ramp: its ACF falls monotonically (no peak); the regression on the row number is exact
    r = R.analyze([float(t) for t in range(60)])
    assert r["detected_periods"] == [] and r["primary_period"] == 0 and r["seasonal_strength"] == 0.0 and r["trend_strength"] == 1.0
    assert not r["is_seasonal"]
    # a constant: variance 0 < EPSILON, ss_yy 0 < EPSILON
    r = R.analyze([5.0] * 50)
    assert r["status"] == R.OK and r["detected_periods"] == [] and r["trend_strength"] == 0.0


def test_short_and_max_lag():
    for n in (0, 1, 2, 3):
        assert R.analyze([1.0, 5.0, 2.0][:n])["status"] == R.SHORT
    assert R.scalar_detect([1.0, 2.0, 3.0]) is None and R.scalar_analyze([None, 1.0, 2.0, 3.0]) is None and R.scalar_detect(None) is None
    for s in SC.short_batch():
        r = R.analyze(s)
        if 4 <= len(s) <= 5:                              # max_lag 2: the peak loop is empty
            assert r["status"] == R.OK and r["detected_periods"] == []
        if 6 <= len(s) <= 7:                              # max_lag 3: lag 2 is the one candidate
            assert r["detected_periods"] in ([], [2])
    assert R.analyze([1.0, 5.0, 1.0, 5.0, 1.0, 5.0])["detected_periods"] == [2]
    assert R.max_lag_of(10, 0) == 5 and R.max_lag_of(10, 3) == 3 and R.max_lag_of(10, 9) == 5 and R.max_lag_of(10, -1) == 5


def test_max_period_cuts_the_strongest_peak():
    s = SC.two_period_series()
    assert R.analyze(s)["detected_periods"][:2] == [35, 5]               # the stronger peak is the longer lag
    assert R.analyze(s, 36)["primary_period"] == 35
    assert R.analyze(s, 35)["primary_period"] == 5                       # lag 35 is the last of the ACF: no right neighbour
    for mp in (1, 2, 3):
        assert R.analyze(s, mp)["detected_periods"] == []
    assert R.analyze(s, 120) == R.analyze(s, 121) == R.analyze(s, 10000) == R.analyze(s, 0)
    assert R.analyze(s, 36)["trend_strength"] == R.analyze(s)["trend_strength"]


def test_nulls_are_dropped():
    for s in SC.null_batch()[:8]:
        assert R.analyze(s) == R.analyze(R.compact(s))
    assert R.analyze(SC.null_batch()[4])["status"] == R.SHORT and R.analyze(SC.null_batch()[5])["status"] == R.OK


def test_more_than_five_peaks_and_edges():
    acf = R.full_acf(SC.many_peaks_series())
    peaks = [i + 1 for i in range(1, len(acf) - 1) if acf[i] > acf[i - 1] and acf[i] > acf[i + 1] and acf[i] > 0.1]
    assert len(peaks) > 5
    r = R.analyze(SC.many_peaks_series())
    assert len(r["detected_periods"]) == 5 and r["strengths"] == sorted(r["strengths"], reverse=True)
    e = SC.edge_batch()
    for name in ("constant", "constant_zero", "tiny_variance"):
        r = R.analyze(e[name])
        assert r["detected_periods"] == [] and r["trend_strength"] == 0.0, name
    for name in ("ramp", "steep_ramp"):
        r = R.analyze(e[name])
        assert r["detected_periods"] == [] and r["trend_strength"] > 0.999, name
    for name in ("nan", "inf", "neg_inf", "huge", "overflowing_sum"):
        r = R.analyze(e[name])
        assert r["status"] == R.OK and r["detected_periods"] == [] and (r["trend_strength"] != r["trend_strength"] or r["trend_strength"] == 0.0), name


def test_tie_cases_are_what_they_claim():
    equal, unordered = SC.tie_cases()
    assert len(equal) >= 10 and len(unordered) >= 10
    for s in equal + unordered:
        assert 12 <= len(s) <= 40 and all(v in (0.0, 1.0, 2.0, 3.0) for v in s) and sum(s) % len(s) == 0
    for s in equal:
        assert SC._tie_kind(s)[0]
        acf, periods = R.full_acf(s), R.analyze(s)["detected_periods"]
        for a, b in zip(periods, periods[1:]):                # the stable order: equal values keep ascending lag
            assert acf[a - 1] > acf[b - 1] or (acf[a - 1] == acf[b - 1] and a < b)
    for s in unordered:
        assert SC._tie_kind(s)[1]


def test_fast_form_equals_the_loops():
    cases = SC.every_short_case()
    assert len(cases) > 150
    for s, mp in cases:
        a, b = R.analyze(s, mp), R.analyze_fast(s, mp)
        for k in a:
            if k in ("strengths", "acf"):
                assert len(a[k]) == len(b[k]) and all(SC.same_bits(x, y) for x, y in zip(a[k], b[k])), (k, mp, len(s))
            elif k in ("seasonal_strength", "trend_strength"):
                assert SC.same_bits(a[k], b[k]), (k, mp, len(s))
            else:
                assert a[k] == b[k], (k, mp, len(s))


# ---- the C ABI without a GPU ----
def test_struct_layouts(hiplib):
    S = hiplib.SeasonalityResult                         # the reference's header: int *, size_t, int, double, double
    assert C.sizeof(S) == 40
    assert [getattr(S, f).offset for f, _ in S._fields_] == [0, 8, 16, 24, 32]
    assert [f for f, _ in S._fields_] == ["detected_periods", "n_periods", "primary_period", "seasonal_strength", "trend_strength"]
    B = hiplib.AnofoxHipSeasonality
    assert C.sizeof(B) == 128 and B.n_periods.offset == 20 and B.strengths.offset == 32 and B.acf.offset == 72 and B.trend_strength.offset == 120
    assert hiplib.SEASONALITY_LDS_ROWS == SC.LDS_ROWS
    assert len(hiplib.SEASONALITY_INT_FIELDS) == 8 and len(hiplib.SEASONALITY_FP_FIELDS) == 12


def test_null_pointer_paths(hiplib):
    L = hiplib.load()
    NULL_POINTER = 1
    v = (C.c_double * 8)(*[1.0, 5.0, 1.0, 5.0, 1.0, 5.0, 1.0, 5.0])
    periods, n = C.POINTER(C.c_int)(), C.c_size_t(99)
    res = hiplib.SeasonalityResult()
    for call in (lambda e: L.anofox_ts_detect_seasonality(None, 8, 0, C.byref(periods), C.byref(n), e),
                 lambda e: L.anofox_ts_detect_seasonality(v, 8, 0, None, C.byref(n), e),
                 lambda e: L.anofox_ts_detect_seasonality(v, 8, 0, C.byref(periods), None, e),
                 lambda e: L.anofox_ts_analyze_seasonality(None, 0, None, 8, 0, C.byref(res), e),
                 lambda e: L.anofox_ts_analyze_seasonality(None, 0, v, 8, 0, None, e),
                 lambda e: L.anofox_hip_seasonality_batch(None, None, None, 3, 0, None, None, e),
                 lambda e: L.anofox_hip_seasonality_device(None, None, 64, None, 3, 8, 0, None, None, None, e)):
        err = hiplib.AnofoxError()
        assert call(C.byref(err)) is False and err.code == NULL_POINTER and b"ull pointer" in err.message
        assert call(None) is False                        # the error pointer may itself be NULL
    assert not periods and n.value == 99 and not res.detected_periods
    err = hiplib.AnofoxError()
    assert L.anofox_hip_seasonality_batch(None, None, None, 0, 0, None, None, C.byref(err)) is True      # an empty batch is no failure


def test_free_functions(hiplib):
    L = hiplib.load()
    L.anofox_free_int_array(None)
    L.anofox_free_seasonality_result(None)
    z = hiplib.SeasonalityResult()
    L.anofox_free_seasonality_result(C.byref(z))
    L.anofox_free_seasonality_result(C.byref(z))
    assert not z.detected_periods and z.n_periods == 0


def test_mirrors_of_a_null_list(hiplib):
    from anofox_forecast_amd import api
    assert api.ts_detect_seasonality(None) is None and api.ts_analyze_seasonality(None) is None
    assert api.ts_analyze_seasonality([1, 2, 3], None) is None
    assert api.ts_detect_seasonality([]) is None and api.ts_analyze_seasonality([None, None]) is None     # data() of an empty vector is NULL
    assert api.anofox_fcst_ts_detect_seasonality is api.ts_detect_seasonality
    assert api.anofox_fcst_ts_analyze_seasonality is api.ts_analyze_seasonality
