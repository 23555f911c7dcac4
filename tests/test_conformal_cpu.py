"""No GPU: the restatement tests/conformal_ref.py against the golden statements (tests/golden/conformal_kats.json) and the
identities of conformal.rs, the ctypes mirrors of the reference's structs, and the argument errors of the host layer that are
answered before any device is touched."""
import ctypes as C
import math
import random

import numpy as np
import pytest

import conformal_cases as CC
import conformal_ref as R

KATS = CC.load_kats()
REF = CC.RefScalars()


@pytest.mark.parametrize("st", KATS["scalars"], ids=lambda st: f'{st["fn"]}@{st["src"].split("/")[-1]}')
def test_restatement_meets_the_golden_scalars(st):
    ok, value = CC.golden_scalar(REF, st)
    assert ok, (st["src"], value)


def test_restatement_meets_the_golden_pairs_and_tables():
    for st in KATS["pairs"]:
        ok, value = CC.golden_pair(REF, st)
        assert ok, (st["src"], value)
    for st in KATS["table_statements"]:
        for what, ok in CC.golden_table(REF, KATS, st):
            assert ok, (st["src"], what)


def _groups():
    rng = random.Random(1)
    return [CC.residuals(rng, n) for n in (1, 2, 3, 10, 64, 141)] + [g for _, g in CC.content_groups()]


def test_alpha_zero_gives_the_largest_magnitude():
    for g in _groups():
        assert CC.same_bits(R.conformal_quantile(g, 0.0)[0], max(abs(r) for r in g))


def test_single_residual_is_every_score():
    for r in (-4.25, 0.0, 3.5, math.inf):
        for a in CC.ALPHAS:
            assert CC.same_bits(R.conformal_quantile([r], a)[0], abs(r))
            p, _ = R.conformal_learn([r], [a], "asymmetric")
            assert p["scores_upper"][0] == (r if r > 0 else 0.0) and p["scores_lower"][0] == (-r if r < 0 else 0.0)


def test_empty_side_of_the_asymmetric_split_gives_zero():
    p, _ = R.conformal_learn([1.0, 2.0, 0.0, -0.0], [0.1, 0.5], "asymmetric")
    assert p["scores_lower"] == [0.0, 0.0] and all(v > 0 for v in p["scores_upper"])
    p, _ = R.conformal_learn([-1.0, -2.0], [0.1], "asymmetric")
    assert p["scores_upper"] == [0.0] and p["scores_lower"] == [2.0]
    p, _ = R.conformal_learn([0.0, -0.0], [0.1], "asymmetric")
    assert p["scores_upper"] == [0.0] and p["scores_lower"] == [0.0]


@pytest.mark.parametrize("method", R.METHODS)
@pytest.mark.parametrize("strategy", R.STRATEGIES)
def test_learn_apply_identities(method, strategy):
    rng = random.Random(7)
    alphas = list(CC.ALPHAS)
    for g in _groups():
        f = [rng.gauss(10.0, 3.0) for _ in range(5)]
        d_cal, d_pred = [1.0 + rng.random() for _ in g], [0.5 + rng.random() for _ in f]
        whole, e = R.conformalize(g, f, alphas, method, strategy, d_cal, d_pred)
        if strategy == "jackknife+" and method == "asymmetric":
            assert whole is None and e == R.JACKKNIFE_ASYM
            continue
        p, e = R.conformal_learn(g, alphas, method, strategy, d_cal)
        assert e is None
        parts, e = R.conformal_apply(f, p, d_pred)
        assert e is None and all(CC.same_bits(a, b) for k in range(len(alphas)) for a, b in zip(whole["lower"][k] + whole["upper"][k],
                                                                                                 parts["lower"][k] + parts["upper"][k]))
        if method != "asymmetric":                                   # symmetric: one value in both score rows
            assert all(CC.same_bits(a, b) for a, b in zip(p["scores_lower"], p["scores_upper"]))
            split, _ = R.conformal_learn(g, alphas, method, "split", d_cal)      # Jackknife+ scores equal split scores
            assert all(CC.same_bits(a, b) for a, b in zip(p["scores_lower"], split["scores_lower"]))
        assert p["state_vector"] == (R.sorted_abs(g) if strategy == "jackknife+" else p["scores_lower"] + p["scores_upper"])


def test_v1_equals_v2():
    rng = random.Random(3)
    for g in _groups():
        f = [rng.gauss(0.0, 1.0) for _ in range(4)]
        for a in CC.ALPHAS:
            v1, _ = R.conformal_predict(g, f, a)
            v2, _ = R.conformalize(g, f, [a])
            assert all(CC.same_bits(x, y) for x, y in zip(v1["lower"] + v1["upper"], v2["lower"][0] + v2["upper"][0]))
            a1, _ = R.conformal_predict_asymmetric(g, f, a)
            a2, _ = R.conformalize(g, f, [a], "asymmetric")
            assert all(CC.same_bits(x, y) for x, y in zip(a1["lower"] + a1["upper"], a2["lower"][0] + a2["upper"][0]))


def test_evaluation_identities():
    rng = random.Random(5)
    for n in (1, 2, 28, 333):
        a = [round(rng.gauss(10, 4), 1) for _ in range(n)]
        l = [x - abs(rng.gauss(0, 2)) if rng.random() < 0.8 else x + 1 for x in a]
        u = [x + abs(rng.gauss(0, 2)) if rng.random() < 0.8 else x - 1 for x in a]
        for alpha in (0.0, 0.1, 0.999999):
            ev, e = R.conformal_evaluate(a, l, u, alpha)
            assert e is None and ev["violation_rate"] + ev["coverage"] == 1.0 and ev["n_observations"] == n
            assert ev["coverage"] == R.conformal_coverage(a, l, u)[0] and CC.same_bits(ev["mean_width"], R.mean_interval_width(l, u))
    # a row ON a bound is covered and pays no penalty
    ev, _ = R.conformal_evaluate([1.0, 2.0], [1.0, 0.0], [3.0, 2.0], 0.1)
    assert ev["coverage"] == 1.0 and ev["winkler_score"] == 2.0


def test_errors_in_the_source_s_order():
    assert R.conformal_quantile([], 2.0) == (None, R.EMPTY)
    assert R.conformal_quantile([1.0], 1.0) == (None, R.ALPHA_V1)
    assert R.conformal_learn([], [], "symmetric") == (None, R.EMPTY)
    assert R.conformal_learn([1.0], [], "symmetric") == (None, R.NO_ALPHA)
    assert R.conformal_learn([1.0], [0.1, 1.5], "symmetric") == (None, "Invalid input: Alpha must be in (0, 1), got 1.5")
    assert R.conformal_learn([1.0], [1.0], "symmetric") == (None, "Invalid input: Alpha must be in (0, 1), got 1")
    assert R.conformal_learn([1.0], [0.1], "adaptive") == (None, R.NEED_DIFFICULTY)
    assert R.conformal_learn([1.0], [0.1], "adaptive", "split", [1.0, 2.0])[1] == "Invalid input: Difficulty length (2) must match residuals length (1)"
    assert R.conformal_learn([1.0], [0.1], "adaptive", "split", [0.0]) == (None, R.DIFFICULTY)
    p, _ = R.conformal_learn([1.0], [0.1], "adaptive", "split", [1.0])
    assert R.conformal_apply([], p, []) == (None, R.NO_FORECAST)
    assert R.conformal_apply([1.0], p, None) == (None, R.NEED_DIFFICULTY)
    assert R.conformal_apply([1.0], p, [-1.0]) == (None, R.DIFFICULTY)
    assert R.conformal_evaluate([], [], [], 0.1) == (None, R.EMPTY)
    assert R.conformal_evaluate([1.0], [0.0], [2.0], 1.0) == (None, "Invalid input: Alpha must be in (0, 1), got 1")
    assert R.conformal_coverage([1.0], [0.0, 1.0], [2.0])[1] == "Invalid input: Length mismatch: actuals=1, lower=2, upper=1"


# --------------------------------------------------------------------------------------------
# the library's host layer, no device
# --------------------------------------------------------------------------------------------
def test_struct_mirrors_have_the_reference_layout(hiplib):
    """types.rs:1427-1672 on a 64-bit target: #[repr(C)] sizes and field offsets."""
    want = {
        "ConformalResultFFI": (80, {"point": 0, "lower": 8, "upper": 16, "n_forecasts": 24, "coverage": 32, "conformity_score": 40, "method": 48}),
        "ConformalMultiResultFFI": (56, {"point": 0, "n_forecasts": 8, "coverage_levels": 16, "conformity_scores": 24, "n_levels": 32, "lower": 40,
                                         "upper": 48}),
        "CalibrationProfileFFI": (64, {"method": 0, "strategy": 4, "alphas": 8, "state_vector": 16, "state_vector_len": 24, "scores_lower": 32,
                                       "scores_upper": 40, "n_levels": 48, "n_residuals": 56}),
        "PredictionIntervalsFFI": (56, {"point": 0, "n_forecasts": 8, "coverage": 16, "n_levels": 24, "lower": 32, "upper": 40, "method": 48}),
        "ConformalEvaluationFFI": (40, {"coverage": 0, "violation_rate": 8, "mean_width": 16, "winkler_score": 24, "n_observations": 32}),
        "AnofoxHipConformal": (64, {"scores_lower": 0, "scores_upper": 8, "sorted": 16, "n_residuals": 24, "lower": 32, "upper": 40,
                                    "n_forecasts": 48, "n_levels": 56}),
    }
    for name, (size, offsets) in want.items():
        cls = getattr(hiplib, name)
        assert C.sizeof(cls) == size, name
        assert {f: getattr(cls, f).offset for f, _ in cls._fields_} == offsets, name


def test_symbols_are_exported(hiplib):
    L = hiplib.load()
    names = [s for s in hiplib.EXPORTED_SYMBOLS if "conformal" in s or s in ("anofox_ts_mean_interval_width", "anofox_free_calibration_profile",
                                                                             "anofox_free_prediction_intervals")]
    assert len(names) == 20
    for s in names:
        assert hasattr(L, s), s
    header = open(hiplib.LIB_PATH.replace("anofox-forecast_amd/libanofox_fcst_hip.so", "include/anofox_fcst_hip.h")).read()
    for s in names:
        assert s + "(" in header, s
    assert "anofox_ts_conformal_predict_per_step(" not in header and not hasattr(L, "anofox_ts_bootstrap_intervals")


def _arr(x):
    return np.ascontiguousarray(x, dtype=np.float64)


def test_argument_errors_need_no_device(hiplib):
    L = hiplib.load()
    err = hiplib.AnofoxError()
    msg = lambda: (err.code, err.message.decode())
    r, f, q = _arr([1.0, -2.0, 3.0]), _arr([10.0, 20.0]), C.c_double()
    none = np.zeros(1, dtype=np.uint64)                                            # every residual NULL
    # quantile
    assert not L.anofox_ts_conformal_quantile(None, None, 3, 0.1, C.byref(q), C.byref(err)) and msg() == (hiplib.NULL_POINTER, "Null pointer argument")
    assert not L.anofox_ts_conformal_quantile(r.ctypes.data, None, 3, 0.1, None, C.byref(err)) and msg() == (hiplib.NULL_POINTER, "Null output pointer")
    assert not L.anofox_ts_conformal_quantile(r.ctypes.data, None, 0, 7.0, C.byref(q), C.byref(err)) and msg() == (hiplib.COMPUTATION_ERROR, R.EMPTY)
    assert not L.anofox_ts_conformal_quantile(r.ctypes.data, none.ctypes.data, 3, 0.1, C.byref(q), C.byref(err)) and msg() == (hiplib.COMPUTATION_ERROR, R.EMPTY)
    for bad in (1.0, -0.1, math.nan):
        assert not L.anofox_ts_conformal_quantile(r.ctypes.data, None, 3, bad, C.byref(q), C.byref(err)) and msg() == (hiplib.COMPUTATION_ERROR, R.ALPHA_V1)
    # predict family
    res = hiplib.ConformalResultFFI()
    assert not L.anofox_ts_conformal_predict(r.ctypes.data, None, 3, None, 2, 0.1, C.byref(res), C.byref(err)) and msg()[0] == hiplib.NULL_POINTER
    assert not L.anofox_ts_conformal_predict(r.ctypes.data, None, 0, f.ctypes.data, 2, 0.1, C.byref(res), C.byref(err)) and msg()[1] == R.EMPTY
    assert not L.anofox_ts_conformal_predict_asymmetric(r.ctypes.data, None, 3, f.ctypes.data, 2, 1.0, C.byref(res), C.byref(err)) and msg()[1] == R.ALPHA_V1
    d = _arr([1.0, 0.0])
    assert not L.anofox_ts_conformal_predict_adaptive(r.ctypes.data, None, 0, f.ctypes.data, d.ctypes.data, 2, 5.0, C.byref(res), C.byref(err))
    assert msg() == (hiplib.COMPUTATION_ERROR, R.DIFFICULTY)                       # the difficulty is looked at first
    multi = hiplib.ConformalMultiResultFFI()
    al = _arr([0.1] * 17)
    assert not L.anofox_ts_conformal_predict_multi(r.ctypes.data, None, 3, f.ctypes.data, 2, al.ctypes.data, 17, C.byref(multi), C.byref(err))
    assert msg()[0] == hiplib.INVALID_INPUT and "at most 16" in msg()[1]
    assert not L.anofox_ts_conformal_predict_multi(r.ctypes.data, None, 3, f.ctypes.data, 2, al.ctypes.data, 0, C.byref(multi), C.byref(err))
    assert msg() == (hiplib.COMPUTATION_ERROR, R.NO_ALPHA)
    # learn: the source's order
    prof = hiplib.CalibrationProfileFFI()
    learn = lambda n, alphas, k, method, strategy, diff, validity=None: L.anofox_ts_conformal_learn(
        r.ctypes.data, validity, n, alphas.ctypes.data, k, method, strategy, diff, C.byref(prof), C.byref(err))
    a2 = _arr([0.1, 1.5])
    assert not learn(0, a2, 0, 0, 0, None) and msg()[1] == R.EMPTY
    assert not learn(3, a2, 0, 0, 0, None) and msg()[1] == R.NO_ALPHA
    assert not learn(3, a2, 2, 0, 0, None) and msg() == (hiplib.COMPUTATION_ERROR, "Invalid input: Alpha must be in (0, 1), got 1.5")
    assert not learn(3, a2, 1, 2, 0, None) and msg()[1] == R.NEED_DIFFICULTY
    two = np.array([0b011], dtype=np.uint64)
    d3 = _arr([1.0, 2.0, -1.0])
    assert not learn(3, a2, 1, 2, 0, d3.ctypes.data, two.ctypes.data) and msg()[1] == "Invalid input: Difficulty length (3) must match residuals length (2)"
    assert not learn(3, a2, 1, 2, 0, d3.ctypes.data) and msg()[1] == R.DIFFICULTY
    assert not learn(3, a2, 1, 1, 2, None) and msg()[1] == R.JACKKNIFE_ASYM
    assert not learn(3, al, 17, 0, 0, None) and msg()[0] == hiplib.INVALID_INPUT
    # apply
    iv = hiplib.PredictionIntervalsFFI()
    sc = _arr([1.0])
    prof = hiplib.CalibrationProfileFFI()
    ptr = lambda a: C.cast(a.ctypes.data, C.POINTER(C.c_double))
    prof.alphas, prof.scores_lower, prof.scores_upper, prof.n_levels, prof.method = ptr(sc), ptr(sc), ptr(sc), 1, 2
    assert not L.anofox_ts_conformal_apply(f.ctypes.data, 0, C.byref(prof), None, C.byref(iv), C.byref(err)) and msg()[1] == R.NO_FORECAST
    assert not L.anofox_ts_conformal_apply(f.ctypes.data, 2, C.byref(prof), None, C.byref(iv), C.byref(err)) and msg()[1] == R.NEED_DIFFICULTY
    assert not L.anofox_ts_conformal_apply(f.ctypes.data, 2, C.byref(prof), d.ctypes.data, C.byref(iv), C.byref(err)) and msg()[1] == R.DIFFICULTY
    # evaluation
    ev, cov = hiplib.ConformalEvaluationFFI(), C.c_double()
    assert not L.anofox_ts_conformal_coverage(f.ctypes.data, f.ctypes.data, f.ctypes.data, 0, C.byref(cov), C.byref(err)) and msg()[1] == R.EMPTY
    assert not L.anofox_ts_conformal_evaluate(f.ctypes.data, f.ctypes.data, f.ctypes.data, 0, 5.0, C.byref(ev), C.byref(err)) and msg()[1] == R.EMPTY
    assert not L.anofox_ts_conformal_evaluate(f.ctypes.data, f.ctypes.data, f.ctypes.data, 2, 1.0, C.byref(ev), C.byref(err))
    assert msg() == (hiplib.COMPUTATION_ERROR, "Invalid input: Alpha must be in (0, 1), got 1")
    assert L.anofox_ts_mean_interval_width(f.ctypes.data, f.ctypes.data, 0, C.byref(cov), C.byref(err)) and math.isnan(cov.value)
    # the device and batch entries
    assert not L.anofox_hip_conformal_learn_device(None, None, None, None, 1, 64, None, 1, 1, al.ctypes.data, 1, 0, None, None, 64, None, None, None,
                                                   None, C.byref(err)) and msg()[0] == hiplib.NULL_POINTER
    assert not L.anofox_hip_conformal_evaluate_device(1, 1, 1, 1, 64, 1, 1, 1, 1.0, 1, 64, 1, None, C.byref(err)) and msg()[0] == hiplib.INVALID_INPUT
    assert not L.anofox_hip_conformal_apply_device(1, None, 1, 64, None, 1, 1, 1, 1, 64, 1, 2, 1, 1, 64, 1, None, C.byref(err))
    assert msg() == (hiplib.INVALID_INPUT, R.NEED_DIFFICULTY)
    assert not L.anofox_hip_conformal_apply_device(1, None, 1, 64, None, 1, 1, 1, 1, 0, 1, 0, 1, 1, 64, 1, None, C.byref(err))
    assert msg() == (hiplib.INVALID_INPUT, "Invalid input: ld is smaller than n_groups")


def test_python_layer_answers_null_without_a_device(hiplib):
    from anofox_forecast_amd import api as A
    assert A.ts_conformal_quantile(None, 0.1) is None and A.ts_conformal_quantile([], 0.1) is None and A.ts_conformal_quantile([None], 0.1) is None
    assert A.ts_conformal_quantile([1.0, 2.0], 1.0) is None and A.ts_conformal_quantile([1.0], None) is None
    assert A.ts_conformal_predict([1.0], [], 0.1) is None and A.ts_conformal_predict_asymmetric([1.0], [2.0], -1.0) is None
    assert A.ts_conformal_learn([1.0], [0.1], "adaptive", "split") is None and A.ts_conformal_learn([1.0], [0.1], "asymmetric", "jackknife+") is None
    assert A.ts_conformal_coverage([1.0, 2.0], [0.0], [3.0, 4.0]) is None and A.ts_conformal_evaluate([1.0], [0.0], [2.0], 1.0) is None
    assert A.ts_mean_interval_width([1.0], [2.0, 3.0]) is None and A.ts_mean_interval_width([], []) is None
    assert A.anofox_fcst_ts_conformal_quantile is A.ts_conformal_quantile
    with pytest.raises(A.InvalidInputException, match="Unknown conformal method"):
        A.conformal_batch([[1.0]], None, [0.1], method="other")
    with pytest.raises(A.InvalidInputException, match="at most 16"):
        A.conformal_batch([_arr([1.0])], None, [0.1] * 17)
    with pytest.raises(A.InvalidInputException, match="JackknifePlus"):
        A.conformal_batch([_arr([1.0])], None, [0.1], method="asymmetric", strategy="jackknife+")
    # the macros' rows when every call fails: the groups stay, the structs are NULL
    r = A.ts_conformal_by({"g": ["a", "a", "b"]}, [1.0, 2.0, 3.0], [0.5, 2.5, 2.0], [10.0, 9.0, 8.0], {"alpha": 1.5})
    assert r["g"] == ["a", "b"] and r["lower"] == [None, None] and r["method"] == [None, None]
    assert A.ts_conformal_calibrate([None, 1.0], [1.0, None], {"alpha": "x"}) == {"conformity_score": None, "coverage": 0.9, "n_residuals": 0}
