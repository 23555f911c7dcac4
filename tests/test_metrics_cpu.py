"""CPU: the restatement of the reference's accuracy metrics (tests/metrics_ref.py) against every statement of
test/sql/ts_metrics.test and the metric statements of extension_comparison.test (inputs: tests/golden/metrics_kats.json); the new
symbols in the header and in lib.EXPORTED_SYMBOLS; the argument errors of the twelve single entries, which need no GPU; and the
host-only logic of the mirrors in api.py (NULL lists and cells, group keys, NULL dates, date order, the row filter) with the GPU
batch call replaced by the restatement."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import metrics_cases as MC
import metrics_ref as R

KATS = MC.load_kats()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SINGLE = ["anofox_ts_" + f for f in R.FIGURES]


@pytest.fixture()
def api(monkeypatch):
    from anofox_forecast_amd import api as A
    monkeypatch.setattr(A, "metrics_batch", MC.ref_metrics_batch)
    return A


# --------------------------------------------------------------------------------------------
# the restatement against the reference's own statements
# --------------------------------------------------------------------------------------------
def scalar_value(fn, args):
    name = fn.replace("anofox_fcst_", "")[3:]
    if name == "mqloss":
        return R.mqloss(args[0], args[1], args[2])
    return getattr(R, name)(*args)


def check_scalar(case, value_of):
    v = value_of(case["fn"], case["args"])
    if "expect" in case:
        assert v == case["expect"], (case["name"], v)
        return
    op, *args = case["check"]
    if op == "abs_diff_other_lt":
        assert abs(v - value_of(case["fn"], case["other_args"])) < args[0]
    else:
        assert MC.check(v, op, *args), (case["name"], v)


@pytest.mark.parametrize("case", KATS["scalar"], ids=lambda c: c["name"])
def test_restatement_meets_scalar_statements(case):
    check_scalar(case, scalar_value)


@pytest.mark.parametrize("st", KATS["statements"], ids=lambda s: s["name"])
def test_restatement_meets_table_statements(api, st):
    MC.check_statement(api, KATS, st)


def test_restatement_branches():
    nan = float("nan")
    assert math.isnan(R.mape([0.0, 0.0], [1.0, 2.0])) and math.isnan(R.smape([0.0, 0.0], [0.0, -0.0]))
    assert math.isnan(R.r2([3.0, 3.0, 3.0], [1.0, 2.0, 3.0])) and math.isnan(R.mase([1.0, 2.0], [2.0, 3.0], [1.0, 2.0]))
    assert R.mape([0.0, 10.0], [5.0, 5.0]) == 50.0                 # the zero actual does not count
    assert R.quantile_loss([1.0, 2.0], [2.0, 1.0], 0.0) == 0.5 and R.quantile_loss([1.0, 2.0], [2.0, 1.0], 1.0) == 0.5
    assert R.coverage([1.0, 2.0], [nan, 0.0], [5.0, nan]) == 0.0   # NaN bounds never cover
    assert math.isnan(R.coverage([], [], []))
    assert R.filter_rows([1.0, nan, 3.0, 4.0], [1.0, 2.0, nan, 5.0]) == [[1.0, 4.0], [1.0, 5.0]]
    assert R.mqloss([1.0, 3.0], [[0.0, 4.0], [2.0, 2.0]], [0.1, 0.9]) == (R.quantile_loss([1.0, 3.0], [0.0, 4.0], 0.1)
                                                                         + R.quantile_loss([1.0, 3.0], [2.0, 2.0], 0.9)) / 2.0


# --------------------------------------------------------------------------------------------
# the C ABI: symbols, and the argument errors that are checked before anything touches the GPU
# --------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported(hiplib):
    header = open(os.path.join(ROOT, "include", "anofox_fcst_hip.h")).read()
    declared = set(re.findall(r"\b(anofox_[a-z_0-9]+)\s*\(", header))
    L = hiplib.load()
    for sym in SINGLE + ["anofox_hip_metrics_batch", "anofox_hip_metrics_device"]:
        assert sym in declared and sym in hiplib.EXPORTED_SYMBOLS and hasattr(L, sym), sym
    assert hiplib.METRIC_FIGURES == R.FIGURES and hiplib.METRICS_MAX_LEVELS == 16


def _arr(v):
    return np.ascontiguousarray(v, dtype=np.float64)


def _call(lib, name, *args):
    out, err = C.c_double(-7.0), lib.AnofoxError()
    ok = getattr(lib.load(), name)(*args, C.byref(out), C.byref(err))
    return ok, out.value, err.code, err.message.decode()


def test_null_pointers_are_code_1(hiplib):
    a = _arr([1.0, 2.0, 3.0])
    p = a.ctypes.data
    for f in MC.TWO_INPUT:
        for args in ((None, 3, p, 3), (p, 3, None, 3)):
            assert _call(hiplib, "anofox_ts_" + f, *args)[2:] == (hiplib.NULL_POINTER, "Null pointer argument"), f
        err = hiplib.AnofoxError()
        assert not getattr(hiplib.load(), "anofox_ts_" + f)(p, 3, p, 3, None, C.byref(err)) and err.code == hiplib.NULL_POINTER
    for f in ("rmae", "mase"):
        for args in ((None, 3, p, 3, p, 3), (p, 3, None, 3, p, 3), (p, 3, p, 3, None, 3)):
            assert _call(hiplib, "anofox_ts_" + f, *args)[2:] == (hiplib.NULL_POINTER, "Null pointer argument"), f
    assert _call(hiplib, "anofox_ts_quantile_loss", None, 3, p, 3, 0.5)[2] == hiplib.NULL_POINTER
    assert _call(hiplib, "anofox_ts_coverage", p, 3, None, p)[2] == hiplib.NULL_POINTER
    assert _call(hiplib, "anofox_ts_coverage", p, 3, p, None)[2] == hiplib.NULL_POINTER
    lv = _arr([0.5])
    qs = (C.c_void_p * 1)(p)
    assert _call(hiplib, "anofox_ts_mqloss", None, 3, qs, 1, lv.ctypes.data)[2] == hiplib.NULL_POINTER
    assert _call(hiplib, "anofox_ts_mqloss", p, 3, None, 1, lv.ctypes.data)[2] == hiplib.NULL_POINTER
    assert _call(hiplib, "anofox_ts_mqloss", p, 3, qs, 1, None)[2] == hiplib.NULL_POINTER


def test_argument_errors_carry_the_source_text(hiplib):
    a, b = _arr([1.0, 2.0, 3.0]), _arr([1.0, 2.0])
    pa, pb = a.ctypes.data, b.ctypes.data
    ce = hiplib.COMPUTATION_ERROR
    for f in MC.TWO_INPUT:
        with pytest.raises(R.MetricError) as e:
            getattr(R, f)(a.tolist(), b.tolist())
        assert _call(hiplib, "anofox_ts_" + f, pa, 3, pb, 2)[2:] == (ce, str(e.value)), f
        assert str(e.value) == "Invalid input: Actual and forecast arrays must have the same length: 3 vs 2"
        assert _call(hiplib, "anofox_ts_" + f, pa, 0, pb, 0)[2:] == (ce, "Insufficient data: need at least 1 observations, got 0"), f
    assert _call(hiplib, "anofox_ts_mase", pa, 3, pa, 3, pb, 2)[2:] == (ce, "Invalid input: Actual and baseline arrays must have the same length: 3 vs 2")
    assert _call(hiplib, "anofox_ts_rmae", pa, 3, pa, 3, pb, 2)[2:] == (ce, "Invalid input: Actual and pred2 arrays must have the same length: 3 vs 2")
    assert _call(hiplib, "anofox_ts_mase", pa, 3, pb, 2, pb, 2)[2:] == (ce, "Invalid input: Actual and forecast arrays must have the same length: 3 vs 2")
    assert _call(hiplib, "anofox_ts_rmae", pa, 0, pa, 0, pa, 0)[2:] == (ce, R.EMPTY_TEXT)
    for q in (1.5, -0.1, float("nan")):
        assert _call(hiplib, "anofox_ts_quantile_loss", pa, 3, pa, 3, q)[2:] == (ce, "Invalid input: Quantile must be between 0 and 1")
    assert _call(hiplib, "anofox_ts_quantile_loss", pa, 3, pb, 2, 1.5)[2:] == (ce, "Invalid input: Actual and forecast arrays must have the same length: 3 vs 2")
    assert _call(hiplib, "anofox_ts_quantile_loss", pa, 0, pa, 0, 1.5)[2:] == (ce, R.EMPTY_TEXT)      # validate_inputs comes first
    lv = _arr([0.5, 1.5])
    qs = (C.c_void_p * 2)(pa, pa)
    assert _call(hiplib, "anofox_ts_mqloss", pa, 3, qs, 0, lv.ctypes.data)[2:] == (hiplib.INVALID_INPUT, "Must have at least one quantile level")
    assert _call(hiplib, "anofox_ts_mqloss", pa, 3, qs, 2, lv.ctypes.data)[2:] == (ce, R.QUANTILE_TEXT)
    assert _call(hiplib, "anofox_ts_mqloss", pa, 0, qs, 2, lv.ctypes.data)[2:] == (ce, R.EMPTY_TEXT)
    hole = (C.c_void_p * 2)(pa, None)
    assert _call(hiplib, "anofox_ts_mqloss", pa, 3, hole, 2, lv.ctypes.data)[2:] == (ce, "Invalid input: Null pointer at quantile index 1")
    many = (C.c_void_p * 17)(*[pa] * 17)
    ok, _, code, msg = _call(hiplib, "anofox_ts_mqloss", pa, 3, many, 17, _arr([0.5] * 17).ctypes.data)
    assert not ok and code == hiplib.INVALID_INPUT and "at most 16 quantile levels" in msg and "17" in msg
    ok, v, code, _ = _call(hiplib, "anofox_ts_coverage", pa, 0, pa, pa)          # coverage of nothing: true and NaN
    assert ok and math.isnan(v) and code == hiplib.SUCCESS


def test_batch_request_errors_need_no_gpu(hiplib):
    """A requested figure whose input is missing, an empty mask, and more than 16 levels fail the batch call before the device."""
    L = hiplib.load()
    a = _arr([1.0, 2.0])
    cols = (C.c_void_p * 1)(a.ctypes.data)
    lens = np.array([2], dtype=np.uint64)
    fig = np.zeros(12)

    def batch(mask, forecast=None, second=None, lower=None, upper=None, quantiles=None, levels=None, n_levels=0):
        err = hiplib.AnofoxError()
        ok = L.anofox_hip_metrics_batch(cols, forecast, second, lower, upper, quantiles, levels, n_levels, lens.ctypes.data, 1, mask, 0.5, False,
                                        fig.ctypes.data, None, C.byref(err))
        return ok, err.code, err.message.decode()

    bit = lambda f: 1 << R.FIGURES.index(f)
    assert batch(0)[:2] == (False, hiplib.INVALID_INPUT) and batch(1 << 12, cols)[:2] == (False, hiplib.INVALID_INPUT)
    ok, code, msg = batch(bit("mae"))
    assert (ok, code) == (False, hiplib.INVALID_INPUT) and "'mae' needs forecast" in msg
    assert "'mase' needs second" in batch(bit("mae") | bit("mase"), cols)[2]
    assert "'coverage' needs lower and upper" in batch(bit("coverage"), cols, None, cols)[2]
    assert batch(bit("mqloss"))[1:] == (hiplib.INVALID_INPUT, "Must have at least one quantile level")
    lv = _arr([0.5] * 17)
    qq = (C.c_void_p * 17)(*[C.addressof(cols)] * 17)
    ok, code, msg = batch(bit("mqloss"), quantiles=qq, levels=lv.ctypes.data, n_levels=17)
    assert (ok, code) == (False, hiplib.INVALID_INPUT) and "at most 16 quantile levels" in msg
    err = hiplib.AnofoxError()
    assert not L.anofox_hip_metrics_batch(None, cols, None, None, None, None, None, 0, lens.ctypes.data, 1, 1, 0.5, False, fig.ctypes.data, None,
                                          C.byref(err)) and err.code == hiplib.NULL_POINTER


# --------------------------------------------------------------------------------------------
# the mirrors, the GPU call answered by the restatement
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", KATS["scalar"], ids=lambda c: c["name"])
def test_scalar_mirrors(api, case):
    check_scalar(case, lambda fn, args: getattr(api, fn)(*args))


def test_scalar_mirrors_null_handling(api):
    assert api.ts_mae(None, [1.0]) is None and api.ts_mae([1.0], None) is None
    assert api.ts_mase([1.0], [1.0], None) is None and api.ts_quantile_loss([1.0], [1.0], None) is None
    assert api.ts_coverage([1.0], None, [2.0]) is None and api.ts_mqloss([1.0], None, [0.5]) is None
    # NULL cells are dropped from each list on its own: equal lengths afterwards compute, different ones are NULL
    assert api.ts_mae([1.0, None, 3.0], [2.0, 5.0, None]) == R.mae([1.0, 3.0], [2.0, 5.0])
    assert api.ts_mae([1.0, None, 3.0], [2.0, 5.0, 7.0]) is None
    assert api.ts_mae([], []) is None and api.ts_coverage([], [], []) is None
    assert api.ts_quantile_loss([1.0, 2.0], [2.0, 1.0], 1.5) is None
    assert api.ts_mqloss([1.0, 2.0], [[1.0, 2.0]], [0.1, 0.9]) is None and api.ts_mqloss([1.0, 2.0], [], []) is None
    assert api.ts_mqloss([1.0, 2.0], [[1.0, 2.0], None], [0.1, 0.9]) is None
    assert api.ts_mqloss([1.0, 3.0], [[0.0, 4.0], [2.0, 2.0]], [0.1, 0.9]) == R.mqloss([1.0, 3.0], [[0.0, 4.0], [2.0, 2.0]], [0.1, 0.9])
    from anofox_forecast_amd.api import InvalidInputException
    with pytest.raises(InvalidInputException, match="at most 16 quantile levels"):
        api.ts_mqloss([1.0], [[1.0]] * 17, [0.5] * 17)
    for f in R.FIGURES:
        assert getattr(api, "anofox_fcst_ts_" + f) is getattr(api, "ts_" + f)


def _messy_table():
    """Two group columns, shuffled dates, NULL dates, NULL cells, and a group ('z', 9) whose every row is filtered."""
    rng = np.random.default_rng(5)
    rows = []
    for g, k in (("b", 1), ("a", 1), ("b", 2), ("z", 9), (None, 1)):
        for t in range(12):
            a = round(float(rng.normal(0, 2)), 1)
            rows.append([g, k, t, a, round(a + float(rng.normal()), 1), round(a + float(rng.normal()), 1), a - 1.0, a + 1.0])
    rows = [rows[i] for i in rng.permutation(len(rows))]
    for i, r in enumerate(rows):
        if r[0] == "z":
            r[3] = None                                            # the actual is NULL in every row (and the forecast in some)
            if i % 2:
                r[4] = None
        elif i % 11 == 0:
            r[2] = None                                            # NULL date: the row never reaches its group
        elif i % 7 == 0:
            r[3 + i % 5] = None
    return rows


def _expected(rows, n_keys, cols, figure, quantile=0.5):
    order, members = [], {}
    for r in rows:
        if r[2] is None:
            continue
        key = tuple(r[:n_keys])
        if key not in members:
            members[key] = []
            order.append(key)
        members[key].append(r)
    out = []
    for key in order:
        rs = sorted(members[key], key=lambda r: r[2])
        data = [[float("nan") if r[c] is None else r[c] for r in rs] for c in cols]
        data = R.filter_rows(*data)
        names = {2: ("forecast",), 3: ("forecast", "second")}[len(cols)] if figure != "coverage" else ("lower", "upper")
        try:
            v = R.figure(figure, data[0], quantile=quantile, **dict(zip(names, data[1:])))
        except R.MetricError:
            v = float("nan")
        out.append((key, v))
    return out


MIRRORS = [("ts_mae_by", "mae", (3, 4)), ("ts_mse_by", "mse", (3, 4)), ("ts_rmse_by", "rmse", (3, 4)), ("ts_mape_by", "mape", (3, 4)),
           ("ts_smape_by", "smape", (3, 4)), ("ts_r2_by", "r2", (3, 4)), ("ts_bias_by", "bias", (3, 4)), ("ts_mase_by", "mase", (3, 4, 5)),
           ("ts_rmae_by", "rmae", (3, 4, 5)), ("ts_coverage_by", "coverage", (3, 6, 7)), ("ts_quantile_loss_by", "quantile_loss", (3, 4))]


@pytest.mark.parametrize("fn,figure,cols", MIRRORS, ids=[m[0] for m in MIRRORS])
@pytest.mark.parametrize("n_keys", [2, 1, 0])
def test_table_mirrors(api, fn, figure, cols, n_keys):
    rows = _messy_table()
    col = lambda j: np.array([r[j] for r in rows], dtype=object)
    groups = {name: [r[j] for r in rows] for j, name in list(enumerate(("g", "k")))[:n_keys]} or None
    extra = (0.9,) if figure == "quantile_loss" else ()
    t = getattr(api, fn)(groups, col(2), *[col(c) for c in cols], *extra)
    want = _expected(rows, n_keys, cols, figure, 0.9)
    assert list(t) == list(("g", "k")[:n_keys]) + [figure]
    assert len(t[figure]) == len(want)
    for i, (key, v) in enumerate(want):
        assert tuple(t[g][i] for g in ("g", "k")[:n_keys]) == key      # first-appearance order
        assert MC.same_bits(t[figure][i], v), (fn, key, t[figure][i], v)
    if n_keys == 2:
        assert math.isnan(t[figure][[k[0] for k, _ in want].index("z")])      # every row filtered: a NaN row, not a missing one


def test_table_mirror_details(api):
    from anofox_forecast_amd.api import InvalidInputException
    with pytest.raises(InvalidInputException, match=r"^Unknown metric type: mase\. Supported: mae, mse, rmse, mape, smape, r2, bias$"):
        api._ts_metrics_native(None, [1, 2], [1.0, 2.0], [1.0, 2.0], "mase")
    assert api._ts_metrics_native(None, [2, 1], [1.0, 2.0], [2.0, 4.0], "MAE") == {"mae": [1.5]}
    assert api.ts_mae_by({"id": []}, [], [], []) == {"id": [], "mae": []}
    d = np.array(["2024-01-02", "NaT", "2024-01-01"], dtype="datetime64[D]")
    assert api.ts_bias_by({"id": ["x", "y", "x"]}, d, [1.0, 5.0, 2.0], [2.0, 9.0, 2.0]) == {"id": ["x"], "bias": [0.5]}
    t = api.ts_quantile_loss_by({"id": ["x", "x"]}, [1, 2], [1.0, 2.0], [2.0, 1.0], 1.5)
    assert t["id"] == ["x"] and math.isnan(t["quantile_loss"][0])   # the failed FFI call of every group is a NaN row
