"""CPU: the numpy restatement of the reference's BOCPD (tests/changepoint_ref.py) against every value-bearing statement of
test/sql/ts_changepoints.test that concerns it (the scalar cases :15-158, the step and multi-step cases :397-514) and the BOCPD
unit tests of changepoint.rs; the host-only logic of the operator mirrors (ParseHazardLambda, row order, NULL-date and short-group
rows) with the GPU batch call replaced by the restatement; the layout of BocpdResult; and the condition the GPU parity test relies
on: no probability of the parity inputs lies within 1e-9 of the 0.5 threshold.  Inputs: tests/golden/changepoint_kats.json."""
import ctypes as C
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import changepoint_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "changepoint_kats.json")))
S = KATS["scalar"]


def _dates(strings, unit="D"):
    return np.array([np.datetime64("NaT") if s is None else np.datetime64(s) for s in strings], dtype=f"datetime64[{unit}]")


def _days(start, n, unit="us"):
    return (np.datetime64(start, "D") + np.arange(n)).astype(f"datetime64[{unit}]")


# --------------------------------------------------------------------------------------------
# the restatement against the reference's own statements
# --------------------------------------------------------------------------------------------
def test_scalar_struct_cases():
    """ts_changepoints.test:15-41."""
    r = R.scalar_bocpd(S["two_level_8"], 250.0, False)
    assert r["is_changepoint"] is not None and r["changepoint_probability"] is not None and r["changepoint_indices"] is not None
    assert len(r["is_changepoint"]) == 8 and len(r["changepoint_probability"]) == 8
    assert r["changepoint_probability"] == [0.0] * 8          # include_probabilities = false: allocated, all zeros


def test_constant_and_boundary_cases():
    """ts_changepoints.test:49-108."""
    assert len(R.scalar_bocpd(S["constant_8"], 250.0, False)["changepoint_indices"]) == 0
    for key in ("constant_8", "noisy_8"):
        r = R.scalar_bocpd(S[key], 250.0, True)
        assert r["is_changepoint"][0] is False and r["is_changepoint"][7] is False
    r = R.scalar_bocpd(S["constant_8"], 250.0, True)
    assert r["changepoint_probability"][4] < 0.1 and r["changepoint_probability"][7] < 0.1
    assert 0 not in r["changepoint_indices"] and 7 not in r["changepoint_indices"]
    # the figures the issue records for this series
    assert abs(r["changepoint_probability"][4] - 0.0010657930) < 1e-10 and abs(r["changepoint_probability"][7] - 0.0010652626) < 1e-10


def test_null_and_small_inputs():
    """ts_changepoints.test:116-158."""
    assert R.scalar_bocpd(None, 250.0, False) is None
    for key in ("empty", "one", "two"):
        assert R.scalar_bocpd(S[key], 250.0, False) is None
    r = R.scalar_bocpd(S["three"], 250.0, False)
    assert r is not None and len(r["changepoint_indices"]) == 0 and len(r["is_changepoint"]) == 3


def test_step_change_cases():
    """ts_changepoints.test:397-479 (issue #71) and the group-A statement :359-364."""
    k = KATS["step_change_test"]
    r = R.scalar_bocpd(k["val"], k["hazard_lambda"], True)
    p = np.array(r["changepoint_probability"])
    assert p.max() > p.min() * 10
    assert p[12] > 0.5
    assert p[5:11].mean() < 0.1
    assert 12 in r["changepoint_indices"]
    assert r["changepoint_indices"] == [12]                   # ts_detect_changepoints: COUNT(*) = 1, at day 12
    assert abs(p[12] - 0.8977909026) < 1e-9 and abs(p[5:11].mean() - 0.0013042688) < 1e-9
    # the aggregate ignores its params MAP and runs at 250: still exactly one flag (:469-479)
    assert R.scalar_bocpd(k["val"], 250.0, True)["changepoint_indices"] == [12]
    a = KATS["changepoints_by_test"]["A"]
    assert R.scalar_bocpd(a, 10.0, True)["changepoint_indices"] == [5]


def test_multi_step_cases():
    """ts_changepoints.test:485-511."""
    k = KATS["multi_step_test"]
    idx = R.scalar_bocpd(k["val"], k["hazard_lambda"], False)["changepoint_indices"]
    assert len(idx) >= 2 and 9 <= idx[0] <= 11
    assert idx == [10, 20]


def test_rust_unit_tests():
    """changepoint.rs:411-483."""
    u = KATS["rust_unit_tests"]
    k = u["test_detect_changepoints_bocpd"]
    flags, prob, _ = R.bocpd(k["values"], k["hazard_lambda"], True)
    assert len(flags) == 100 and len(prob) == 100 and np.all((prob >= 0.0) & (prob <= 1.0)) and prob.max() >= 0.0
    k = u["test_detect_changepoints_bocpd_step_change"]
    flags, prob, _ = R.bocpd(k["values"], k["hazard_lambda"], True)
    assert not np.all(np.abs(prob - prob[0]) < 1e-10)
    assert prob[12] > prob[5:11].sum() / 6.0 * 10.0 and prob[12] > 0.5
    k = u["test_detect_changepoints_bocpd_insufficient_data"]
    with pytest.raises(R.InsufficientData, match="need at least 3 observations, got 2"):
        R.bocpd(k["values"], k["hazard_lambda"], False)


def test_the_two_power_routes_agree_far_inside_the_tolerance():
    """The tolerance argument of DESIGN.md section 3: pow(b, e) against exp(e log b), both libm, differ by a few 1e-15."""
    rng = np.random.default_rng(5)
    y = rng.poisson(1.2, 700).astype(np.float64)
    y[350] = 4000.0                                           # an outlier step: every predictive weight is tiny
    for lam in (250.0, 10.0):
        f0, p0, _ = R.bocpd(y, lam)
        f1, p1, _ = R.bocpd(y, lam, power=R.pow_exp_log)
        assert np.array_equal(f0, f1)
        assert R.rel(p1, p0) <= 1e-13, R.rel(p1, p0)


def test_wrapper_and_clamp():
    y = KATS["step_change_test"]["val"]
    assert np.array_equal(R.ffi_bocpd(y, -1.0)[1], R.ffi_bocpd(y, 250.0)[1])
    assert np.array_equal(R.ffi_bocpd(y, 0.0)[1], R.ffi_bocpd(y, 250.0)[1])
    assert np.array_equal(R.ffi_bocpd(y, 0.5)[1], R.ffi_bocpd(y, 1.0)[1])
    assert R.ffi_bocpd([1.0, 2.0], 250.0) is None


# --------------------------------------------------------------------------------------------
# host-only logic of the mirrors
# --------------------------------------------------------------------------------------------
def test_parse_hazard_lambda():
    """ParseHazardLambda (ts_changepoints.cpp:451-473)."""
    from anofox_forecast_amd import api
    P = api.parse_hazard_lambda
    assert P("250.0") == 250.0 and P("  10.0\t") == 10.0 and P("1e2") == 100.0 and P("-3") == -3.0
    assert P("12abc") == 12.0                                 # std::stod takes the numeric prefix
    assert P("{'hazard_lambda': '42.5'}") == 42.5 and P('{"HAZARD_LAMBDA"="7"}') == 7.0 and P("hazard_lambda:3") == 3.0
    assert P("abc") == 250.0 and P("") == 250.0 and P("{}") == 250.0
    assert P("inf") == float("inf") and np.isnan(P("nan"))
    assert P("1e999") == 250.0                                # out of range: stod throws, no regex match, the default


def _fake_batch(series, hazard_lambda=250.0, valids=None):
    """api.changepoints_batch with the restatement in place of the GPU."""
    assert valids is None
    _fake_batch.calls.append((len(series), hazard_lambda))
    out = []
    for y in series:
        r = R.ffi_bocpd(y, hazard_lambda, True)
        if r is None:
            out.append({"ok": False, "code": 3, "message": f"Insufficient data: need at least 3 observations, got {len(y)}",
                        "probability": None, "is_changepoint": None, "n_changepoints": -1})
        else:
            out.append({"ok": True, "code": 0, "message": "", "probability": r[1], "is_changepoint": r[0], "n_changepoints": len(r[2])})
    return out


@pytest.fixture
def mirrors(monkeypatch):
    from anofox_forecast_amd import api
    _fake_batch.calls = []
    monkeypatch.setattr(api, "changepoints_batch", _fake_batch)
    return api


def _as_rows(out, group_name, date_name):
    d = out[date_name]
    us = [None if np.isnat(x) else int(x.astype("datetime64[us]").astype(np.int64)) for x in d]
    p = out["changepoint_probability"]
    pm = np.ma.getmaskarray(p)
    return [(g, t, bool(f), None if m else float(v)) for g, t, f, v, m in zip(out[group_name], us, out["is_changepoint"], np.ma.getdata(p), pm)]


def _us(dates):
    return [None if np.isnat(x) else int(x.astype("datetime64[us]").astype(np.int64)) for x in dates]


def test_by_mirror_rows_order_and_one_batch_call(mirrors):
    """Groups in first-appearance order, rows sorted by (timestamp, value), NULL value = 0.0, short and failing groups keep their
    rows, NULL dates last -- against the restated table function; every group goes out in ONE batch call."""
    api = mirrors
    rng = np.random.default_rng(3)
    grp, dts, val = [], [], []
    for g, n in (("z", 12), ("a", 1), ("m", 2), (None, 9), ("b", 30)):
        for i in rng.permutation(n):
            grp.append(g)
            dts.append(None if (g == "b" and i % 7 == 3) else f"2024-02-{1 + i // 2:02d}")      # duplicate dates: the value breaks the tie
            val.append(None if (g == "z" and i == 4) else float(rng.integers(0, 5) + (40 if i > n // 2 else 0)))
    o = rng.permutation(len(grp))                                                              # interleave the groups
    grp, dts, val = [grp[i] for i in o], [dts[i] for i in o], [val[i] for i in o]
    dates = _dates(dts)
    out = api.ts_detect_changepoints_by(grp, dates, np.array(val, dtype=object), {"hazard_lambda": "10.0"}, group_name="k", date_name="d")
    assert list(out.keys()) == ["k", "d", "is_changepoint", "changepoint_probability"]
    assert out["d"].dtype == np.dtype("datetime64[D]")
    want = R.by_rows(grp, _us(dates), val, 10.0)
    assert _as_rows(out, "k", "d") == want
    assert len(want) == len(grp)
    assert _fake_batch.calls == [(4, 10.0)]                                                    # z, m (2 rows: it fails there), NULL, b

def test_by_mirror_sql_row_preservation_blocks(mirrors):
    """ts_changepoints.test:521-622.  cp_combined: the file expects 2 rows with a NULL probability; group A there has 2 dated rows,
    for which the call fails (changepoint.rs:205-207) and ts_changepoints.cpp:707-719 writes NULL for both, so the source gives 4."""
    api = mirrors
    for name, n_null_date, n_null_prob in (("cp_null_dates", 1, 1), ("cp_singleton", 0, 1), ("cp_combined", 1, 4)):
        k = KATS[name]
        out = api.ts_detect_changepoints_by(k["grp"], _dates(k["dt"]), k["val"], {}, group_name="grp", date_name="dt")
        assert len(out["grp"]) == 4
        nd = np.isnat(out["dt"])
        pm = np.ma.getmaskarray(out["changepoint_probability"])
        assert nd.sum() == n_null_date and not out["is_changepoint"][nd].any() and pm[nd].all()
        assert (pm & ~out["is_changepoint"]).sum() == n_null_prob
        if n_null_date:
            assert nd[-1]                                                                      # NULL-date rows come last
    out = api.ts_detect_changepoints_by(KATS["cp_singleton"]["grp"], _dates(KATS["cp_singleton"]["dt"]), KATS["cp_singleton"]["val"], None,
                                        group_name="grp", date_name="dt")
    b = [i for i, g in enumerate(out["grp"]) if g == "B"]
    assert len(b) == 1 and not out["is_changepoint"][b[0]] and np.ma.getmaskarray(out["changepoint_probability"])[b[0]]
    i = np.arange(100)
    dt = np.where(i % 10 == 5, np.datetime64("NaT"), np.datetime64("2024-01-01") + i % 10).astype("datetime64[D]")
    out = api.ts_detect_changepoints_by([f"grp_{j // 10}" for j in i], dt, 100.0 + i, {}, group_name="grp", date_name="dt")
    assert len(out["grp"]) == 100 and np.isnat(out["dt"]).sum() == 10 and np.isnat(out["dt"][-10:]).all()


def test_by_mirror_date_type_and_lambda(mirrors):
    api = mirrors
    with pytest.raises(api.InvalidInputException, match="Date column must be DATE or TIMESTAMP, got: INTEGER"):
        api.ts_detect_changepoints_by(["a"] * 3, np.arange(3, dtype=np.int32), [1.0, 2.0, 3.0])
    k = KATS["changepoints_by_test"]
    ts = _days(k["start"], 10)
    grp, dates, val = ["A"] * 10 + ["B"] * 10, np.concatenate((ts, ts)), k["A"] + k["B"]
    out = api.ts_detect_changepoints_by(grp, dates, val, {}, group_name="grp", date_name="ts")
    assert len(out["grp"]) == 20 and set(out["grp"]) == {"A", "B"} and out["ts"].dtype == np.dtype("datetime64[us]")
    assert _fake_batch.calls[-1] == (2, 250.0)
    out = api.ts_detect_changepoints_by(grp, dates, val, {"hazard_lambda": "10.0"}, group_name="grp", date_name="ts")
    assert int(out["is_changepoint"][:10].sum()) == 1 and _fake_batch.calls[-1] == (2, 10.0)
    assert api.anofox_fcst_ts_detect_changepoints_by is api.ts_detect_changepoints_by


def test_agg_mirror_ignores_params_and_skips_nulls(mirrors):
    api = mirrors
    k = KATS["step_change_test"]
    ts = _days(k["start"], 24)
    rows = api.ts_detect_changepoints_agg(ts[::-1], k["val"][::-1], {"hazard_lambda": "10.0"})
    assert _fake_batch.calls[-1] == (1, 250.0)
    assert [r["timestamp"] for r in rows] == list(ts) and [r["value"] for r in rows] == k["val"]
    assert sum(r["is_changepoint"] for r in rows) == 1 and rows[12]["is_changepoint"]
    assert set(rows[0]) == {"timestamp", "value", "is_changepoint", "changepoint_probability"}
    val = np.array(k["val"], dtype=object)
    val[3] = None
    assert len(api.ts_detect_changepoints_agg(ts, val, None)) == 23
    assert api.ts_detect_changepoints_agg(ts[:2], k["val"][:2], None) is None
    assert api.ts_detect_changepoints_agg(ts[:0], [], None) is None


# --------------------------------------------------------------------------------------------
# ABI
# --------------------------------------------------------------------------------------------
def test_bocpd_result_layout(hiplib):
    """BocpdResult as the reference's cbindgen header declares it (anofox_fcst_ffi.h:992-1013): five 8-byte members at 0, 8, 16,
    24, 32, size 40 -- as gcc lays out include/anofox_fcst_hip.h and as lib.py mirrors it; the four new symbols are exported."""
    src = r"""
#include <stdio.h>
#include <stddef.h>
#include "anofox_fcst_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(BocpdResult), offsetof(BocpdResult, is_changepoint), offsetof(BocpdResult, changepoint_probability),
         offsetof(BocpdResult, n_points), offsetof(BocpdResult, changepoint_indices), offsetof(BocpdResult, n_changepoints));
  return 0; }"""
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = subprocess.check_output([os.path.join(d, "t")]).decode().split("\n")
    assert out[0] == "40 0 8 16 24 32"
    B = hiplib.BocpdResult
    assert out[0] == (f"{C.sizeof(B)} {B.is_changepoint.offset} {B.changepoint_probability.offset} {B.n_points.offset} "
                      f"{B.changepoint_indices.offset} {B.n_changepoints.offset}")
    L = hiplib.load()
    for sym in ("anofox_ts_detect_changepoints_bocpd", "anofox_free_bocpd_result", "anofox_hip_changepoints_batch",
                "anofox_hip_changepoints_device"):
        assert hasattr(L, sym), sym
    # argument errors come before any device work
    err = hiplib.AnofoxError()
    assert not L.anofox_ts_detect_changepoints_bocpd(None, 0, 250.0, False, None, C.byref(err)) and err.code == hiplib.NULL_POINTER
    L.anofox_free_bocpd_result(None)


# --------------------------------------------------------------------------------------------
# the parity inputs of the GPU test
# --------------------------------------------------------------------------------------------
def test_parity_inputs_keep_clear_of_the_threshold():
    """The GPU test compares flags exactly and may exclude no point.  That is legitimate only if no probability of the restatement
    lies within 1e-9 of 0.5 on the committed inputs; the batch must also hold what the issue lists, and flags must be frequent."""
    series, valids = R.parity_batch()
    lens = [len(y) for y in series]
    assert 200 <= len(series) <= 400 and max(lens) == 700 and min(lens) == 0
    assert all(n in lens for n in R.EDGE_LENGTHS)
    assert any(v is not None for v in valids)
    assert any(len(y) > 3 and np.all(y == y[0]) and y[0] != 0 for y in series) and any(len(y) > 3 and not y.any() for y in series)
    ref = R.parity_reference(series, valids)
    nearest, n_flags, n_points = 1.0, 0, 0
    for lam in R.PARITY_LAMBDAS:
        for y, r in zip(series, ref[lam]):
            assert (r is None) == (len(y) < 3)
            if r is None:
                continue
            flags, prob = r
            assert np.all(np.isfinite(prob))
            nearest = min(nearest, float(np.min(np.abs(prob - 0.5))))
            n_flags += int(flags.sum())
            n_points += len(flags)
    print(f"nearest probability to 0.5: {nearest:.3e}; {n_flags} flags over {n_points} points")
    assert nearest > 1e-9, nearest
    assert n_flags > 500
