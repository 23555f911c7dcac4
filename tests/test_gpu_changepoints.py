"""GPU: Bayesian online changepoint detection (csrc/changepoint.hip) through every layer above the kernel -- the C-ABI single, batch
and device-resident entries and the operator mirrors -- against the numpy restatement tests/changepoint_ref.py and the statements
of the reference's test/sql/ts_changepoints.test (inputs: tests/golden/changepoint_kats.json).

The contract is a tolerance, not bit-identity: the kernel differs from the restatement in the power function
(det_math, not libm) and in the association order of the two per-step sums.  Every probability agrees to REL_TOL = 1e-12 with the
deviation measure of tests/test_gpu_intermittent.py (|a - b| / max(1, |b|): absolute, as probabilities are <= 1); every flag
agrees exactly -- the parity inputs hold no probability within 1e-9 of 0.5 (asserted in tests/test_changepoint_cpu.py), so no
point is excluded from the flag comparison."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import changepoint_ref as R

pytestmark = pytest.mark.gpu

REL_TOL = 1e-12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "changepoint_kats.json")))
S = KATS["scalar"]


@pytest.fixture(scope="module")
def env(hiplib):
    import torch
    assert torch.cuda.is_available()
    from anofox_forecast_amd import api
    return api, hiplib, torch


def _dates(strings, unit="D"):
    return np.array([np.datetime64("NaT") if s is None else np.datetime64(s) for s in strings], dtype=f"datetime64[{unit}]")


def _days(start, n, unit="us"):
    return (np.datetime64(start, "D") + np.arange(n)).astype(f"datetime64[{unit}]")


def _single(lib, y, lam, include=True):
    """anofox_ts_detect_changepoints_bocpd: (ok, error code, message, flags, probabilities, indices)."""
    L = lib.load()
    y = np.ascontiguousarray(y, dtype=np.float64)
    res = lib.BocpdResult()
    C.memset(C.byref(res), 0, C.sizeof(res))
    err = lib.AnofoxError()
    dummy = np.zeros(1)
    ok = L.anofox_ts_detect_changepoints_bocpd(y.ctypes.data if len(y) else dummy.ctypes.data, len(y), float(lam), bool(include),
                                               C.byref(res), C.byref(err))
    if not ok:
        return False, int(err.code), err.message.decode(), None, None, None
    n, k = res.n_points, res.n_changepoints
    flags = np.array([res.is_changepoint[i] for i in range(n)], dtype=bool)
    prob = np.array([res.changepoint_probability[i] for i in range(n)], dtype=np.float64)
    assert bool(res.changepoint_indices) == (k > 0)                 # NULL when there are none
    idx = [int(res.changepoint_indices[i]) for i in range(k)]
    L.anofox_free_bocpd_result(C.byref(res))
    assert not res.is_changepoint and not res.changepoint_probability and not res.changepoint_indices
    return True, 0, "", flags, prob, idx


def _device(lib, torch, series, lam, sentinel=-7.0):
    """anofox_hip_changepoints_device on a time-major block prefilled with sentinels: (prob [T x ld], flags, counts) as numpy."""
    n = len(series)
    ld = (n + 63) // 64 * 64
    T = max(1, max(len(y) for y in series))
    yb = np.zeros((T, ld))
    for s, y in enumerate(series):
        yb[:len(y), s] = y
    dev = torch.device("cuda:0")
    y = torch.from_numpy(yb).to(dev)
    lens = torch.tensor([len(s) for s in series] + [0] * (ld - n), dtype=torch.int32, device=dev)
    prob = torch.full((T, ld), sentinel, dtype=torch.float64, device=dev)
    flags = torch.full((T, ld), 9, dtype=torch.uint8, device=dev)
    counts = torch.full((ld,), -99, dtype=torch.int32, device=dev)
    err = lib.AnofoxError()
    torch.cuda.synchronize()
    assert lib.load().anofox_hip_changepoints_device(y.data_ptr(), ld, lens.data_ptr(), n, T, float(lam), prob.data_ptr(), flags.data_ptr(),
                                                     counts.data_ptr(), None, C.byref(err)), err.message
    return prob.cpu().numpy(), flags.cpu().numpy(), counts.cpu().numpy()


# --------------------------------------------------------------------------------------------
# the reference's SQL statements through the C ABI and the mirrors
# --------------------------------------------------------------------------------------------
def test_scalar_statements_through_the_c_abi_and_the_scalar_mirror(env):
    """ts_changepoints.test:15-158."""
    api, lib, torch = env
    ok, _, _, flags, prob, idx = _single(lib, S["two_level_8"], 250.0, False)
    assert ok and len(flags) == 8 and len(prob) == 8 and np.all(prob == 0.0)       # not asked for: allocated, all zeros
    r = api._ts_detect_changepoints_bocpd(S["two_level_8"], 250.0, False)
    assert r["is_changepoint"] is not None and r["changepoint_probability"] is not None and r["changepoint_indices"] is not None
    assert len(r["is_changepoint"]) == 8 and len(r["changepoint_probability"]) == 8
    assert len(api._ts_detect_changepoints_bocpd(S["constant_8"], 250.0, False)["changepoint_indices"]) == 0
    for key in ("constant_8", "noisy_8"):
        r = api._ts_detect_changepoints_bocpd(S[key], 250.0, True)
        assert r["is_changepoint"][0] is False and r["is_changepoint"][7] is False
    r = api._ts_detect_changepoints_bocpd(S["constant_8"], 250.0, True)
    assert r["changepoint_probability"][4] < 0.1 and r["changepoint_probability"][7] < 0.1
    assert 0 not in r["changepoint_indices"] and 7 not in r["changepoint_indices"]
    want = R.scalar_bocpd(S["constant_8"], 250.0, True)
    assert R.rel(r["changepoint_probability"], want["changepoint_probability"]) <= REL_TOL
    # NULL, n = 0, 1, 2 give NULL; n = 3 works
    assert api._ts_detect_changepoints_bocpd(None, 250.0, False) is None
    for key in ("empty", "one", "two"):
        assert api._ts_detect_changepoints_bocpd(S[key], 250.0, False) is None
    r = api._ts_detect_changepoints_bocpd(S["three"], 250.0, False)
    assert r is not None and len(r["changepoint_indices"]) == 0 and len(r["is_changepoint"]) == 3
    assert api._ts_detect_changepoints_bocpd(S["three"], None, None) == r          # NULL lambda = 250, NULL flag = false
    assert api._ts_detect_changepoints_bocpd([5.0, None, 5.0], 250.0, False) is None   # NULL elements are dropped: 2 values left


def test_c_abi_error_behaviour(env):
    """lib.rs:3056-3130."""
    api, lib, torch = env
    L = lib.load()
    err = lib.AnofoxError()
    res = lib.BocpdResult()
    y = np.array([1.0, 2.0, 3.0])
    assert not L.anofox_ts_detect_changepoints_bocpd(None, 3, 250.0, True, C.byref(res), C.byref(err)) and err.code == lib.NULL_POINTER
    assert err.message == b"Null pointer argument"
    assert not L.anofox_ts_detect_changepoints_bocpd(y.ctypes.data, 3, 250.0, True, None, C.byref(err)) and err.code == lib.NULL_POINTER
    for n in (0, 1, 2):
        ok, code, msg, *_ = _single(lib, y[:n], 250.0)
        assert not ok and code == lib.COMPUTATION_ERROR and msg == f"Insufficient data: need at least 3 observations, got {n}"
    assert L.anofox_ts_detect_changepoints_bocpd(y.ctypes.data, 3, 250.0, True, C.byref(res), None)      # out_error may be NULL
    L.anofox_free_bocpd_result(C.byref(res))
    L.anofox_free_bocpd_result(C.byref(res))                        # idempotent
    # hazard_lambda <= 0 and NaN mean 250
    step = KATS["step_change_test"]["val"]
    base = _single(lib, step, 250.0)[4]
    for lam in (0.0, -1.0, float("nan")):
        assert np.array_equal(_single(lib, step, lam)[4], base)
    assert not np.array_equal(_single(lib, step, 10.0)[4], base)
    # the max(lambda, 1) clamp
    assert np.array_equal(_single(lib, step, 0.5)[4], _single(lib, step, 1.0)[4])


def test_table_macro_mirror(env):
    """ts_changepoints.test:164-174, 453-466, 485-511: ts_detect_changepoints."""
    api, lib, torch = env
    k = KATS["changepoint_test"]
    out = api.ts_detect_changepoints(_days(k["start"], 10), k["val"], {"hazard_lambda": "250.0"})
    assert list(out.keys()) == ["date_col", "value_col", "is_changepoint", "changepoint_probability"]
    assert len(out["date_col"]) == 10
    assert out["changepoint_probability"] == [0.0] * 10            # include_probabilities defaults to FALSE in this macro
    k = KATS["step_change_test"]
    ts = _days(k["start"], 24)
    o = np.random.default_rng(1).permutation(24)
    out = api.ts_detect_changepoints(ts[o], np.array(k["val"])[o], {"hazard_lambda": "10.0"})
    hit = [i for i, f in enumerate(out["is_changepoint"]) if f]
    assert len(hit) == 1
    assert int((out["date_col"][hit[0]] - np.datetime64("2023-01-01")) / np.timedelta64(1, "D")) == 12
    assert out["value_col"] == k["val"]
    out = api.ts_detect_changepoints(ts, k["val"], {"hazard_lambda": "10.0", "include_probabilities": "true"})
    p = np.array(out["changepoint_probability"])
    assert p[12] > 0.5 and p[5:11].mean() < 0.1 and p.max() > p.min() * 10
    k = KATS["multi_step_test"]
    out = api.ts_detect_changepoints(_days(k["start"], 30), k["val"], {"hazard_lambda": "10.0"})
    hit = [i for i, f in enumerate(out["is_changepoint"]) if f]
    assert len(hit) >= 2 and 9 <= hit[0] <= 11
    # a params value that is no number falls back to 250; two rows give NULLs
    a = api.ts_detect_changepoints(ts, KATS["step_change_test"]["val"], {"hazard_lambda": "abc"})
    b = api.ts_detect_changepoints(ts, KATS["step_change_test"]["val"], None)
    assert a == b
    out = api.ts_detect_changepoints(ts[:2], [1.0, 2.0], None)
    assert out["is_changepoint"] == [None, None] and out["changepoint_probability"] == [None, None]
    assert api.anofox_fcst_ts_detect_changepoints is api.ts_detect_changepoints


def test_step_statements_through_the_scalar(env):
    """ts_changepoints.test:404-451 (issue #71) and changepoint.rs:411-483."""
    api, lib, torch = env
    k = KATS["step_change_test"]
    r = api._ts_detect_changepoints_bocpd(k["val"], 10.0, True)
    p = np.array(r["changepoint_probability"])
    assert p.max() > p.min() * 10 and p[12] > 0.5 and p[5:11].mean() < 0.1 and 12 in r["changepoint_indices"]
    assert r["changepoint_indices"] == [12]
    want = R.scalar_bocpd(k["val"], 10.0, True)
    assert R.rel(p, want["changepoint_probability"]) <= REL_TOL and r["is_changepoint"] == want["is_changepoint"]
    u = KATS["rust_unit_tests"]["test_detect_changepoints_bocpd"]
    ok, _, _, flags, prob, idx = _single(lib, u["values"], u["hazard_lambda"])
    assert ok and len(flags) == 100 and len(prob) == 100 and np.all((prob >= 0.0) & (prob <= 1.0))
    u = KATS["rust_unit_tests"]["test_detect_changepoints_bocpd_insufficient_data"]
    assert not _single(lib, u["values"], u["hazard_lambda"], False)[0]


def test_aggregate_mirror(env):
    """ts_changepoints.test:184-297, 469-479: ts_detect_changepoints_agg."""
    api, lib, torch = env
    k = KATS["changepoints_by_test"]
    ts = _days(k["start"], 10)
    rows = api.ts_detect_changepoints_agg(ts, k["A"], {})
    assert rows is not None and len(rows) == 10
    for f in ("timestamp", "value", "is_changepoint", "changepoint_probability"):
        assert rows[0][f] is not None
    rows = api.ts_detect_changepoints_agg(ts, [5.0] * 10, {})
    assert sum(1 if r["is_changepoint"] else 0 for r in rows) == 0
    assert len(api.ts_detect_changepoints_agg(ts, k["A"], {"hazard_lambda": "100.0"})) == 10
    per_group = {g: api.ts_detect_changepoints_agg(ts, k[g], {}) for g in ("A", "B")}       # GROUP BY grp
    assert len(per_group) == 2 and all(len(v) == 10 for v in per_group.values())
    s = KATS["step_change_test"]
    rows = api.ts_detect_changepoints_agg(_days(s["start"], 24), s["val"], {"hazard_lambda": "10.0"})
    assert sum(1 if r["is_changepoint"] else 0 for r in rows) == 1
    want = R.ffi_bocpd(s["val"], 250.0)                              # the aggregate never reads its params: lambda stays 250
    assert R.rel([r["changepoint_probability"] for r in rows], want[1]) <= REL_TOL
    assert api.anofox_fcst_ts_detect_changepoints_agg is api.ts_detect_changepoints_agg


def test_by_mirror_statements(env):
    """ts_changepoints.test:306-390: ts_detect_changepoints_by."""
    api, lib, torch = env
    k = KATS["changepoints_by_test"]
    ts = _days(k["start"], 10)
    grp, dates, val = ["A"] * 10 + ["B"] * 10, np.concatenate((ts, ts)), k["A"] + k["B"]
    out = api.ts_detect_changepoints_by(grp, dates, val, {}, group_name="grp", date_name="ts")
    assert list(out.keys()) == ["grp", "ts", "is_changepoint", "changepoint_probability"]
    assert len(out["grp"]) == 20 and len(set(out["grp"])) == 2
    assert not np.isnat(out["ts"][0]) and out["is_changepoint"][0] is not None
    assert not np.ma.getmaskarray(out["changepoint_probability"])[0]
    assert len(api.ts_detect_changepoints_by(grp, dates, val, {"hazard_lambda": "100.0"}, group_name="grp", date_name="ts")["grp"]) == 20
    out = api.ts_detect_changepoints_by(grp, dates, val, {"hazard_lambda": "10.0"}, group_name="grp", date_name="ts")
    a = np.array([g == "A" for g in out["grp"]])
    assert int(out["is_changepoint"][a].sum()) == 1                  # exactly one flag for group A at lambda = 10
    assert int(np.nonzero(out["is_changepoint"][a])[0][0]) == 5
    for g, lam_rows in (("A", k["A"]), ("B", k["B"])):
        sel = np.array([x == g for x in out["grp"]])
        want = R.ffi_bocpd(lam_rows, 10.0)
        assert R.rel(np.ma.getdata(out["changepoint_probability"])[sel], want[1]) <= REL_TOL
        assert np.array_equal(out["is_changepoint"][sel], want[0])
    # cp_custom_cols: twenty groups of one row each keep their rows and their column names
    i = np.arange(1, 21)
    names = [f"product_{j}" for j in i]
    sale = (np.datetime64("2023-01-01") + i % 10).astype("datetime64[us]")
    out = api.ts_detect_changepoints_by(names, sale, np.where(i % 10 < 5, 100.0, 200.0), {}, group_name="my_product_id",
                                        date_name="sale_date")
    assert list(out.keys())[:2] == ["my_product_id", "sale_date"] and len(out["my_product_id"]) == 20
    assert sorted(out["my_product_id"])[0] == "product_1" and not np.isnat(out["sale_date"]).any()
    with pytest.raises(api.InvalidInputException, match="Date column must be DATE or TIMESTAMP, got: BIGINT"):
        api.ts_detect_changepoints_by(grp, np.arange(20, dtype=np.int64), val)


def test_by_mirror_row_preservation_blocks(env):
    """ts_changepoints.test:521-622.  ONE statement deviates: cp_combined expects 2 rows with a NULL probability (:598-602).  Group A
    there has 2 dated rows; by ts_changepoints.cpp:667-719 with changepoint.rs:205-207 the call fails for it and both rows get
    NULL, so the source gives 4 (A's two rows, the NULL-date row, B's single row).  The mirror follows the source."""
    api, lib, torch = env
    for name, n_null_date, n_null_prob in (("cp_null_dates", 1, 1), ("cp_singleton", 0, 1), ("cp_combined", 1, 4)):
        k = KATS[name]
        out = api.ts_detect_changepoints_by(k["grp"], _dates(k["dt"]), k["val"], {}, group_name="grp", date_name="dt")
        assert len(out["grp"]) == 4
        nd = np.isnat(out["dt"])
        pm = np.ma.getmaskarray(out["changepoint_probability"])
        assert int((nd & ~out["is_changepoint"]).sum()) == n_null_date and int((nd & pm).sum()) == n_null_date
        assert int((~out["is_changepoint"] & pm).sum()) == n_null_prob
        if name == "cp_singleton":
            b = np.array([g == "B" for g in out["grp"]])
            assert int((b & ~out["is_changepoint"]).sum()) == 1 and int((b & pm).sum()) == 1
        if name != "cp_combined":
            a = np.array([g == "A" for g in out["grp"]]) & ~nd
            want = R.ffi_bocpd(k["val"][:3], 250.0)
            assert R.rel(np.ma.getdata(out["changepoint_probability"])[a], want[1]) <= REL_TOL
    i = np.arange(100)
    dt = np.where(i % 10 == 5, np.datetime64("NaT"), np.datetime64("2024-01-01") + i % 10).astype("datetime64[D]")
    out = api.ts_detect_changepoints_by([f"grp_{j // 10}" for j in i], dt, 100.0 + i, {}, group_name="grp", date_name="dt")
    assert len(out["grp"]) == 100 and int(np.isnat(out["dt"]).sum()) == 10


# --------------------------------------------------------------------------------------------
# parity with the restatement, determinism, errors
# --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def parity():
    series, valids = R.parity_batch()
    return series, valids, R.parity_reference(series, valids)


def test_parity_with_the_restatement_through_all_three_entries(env, parity):
    """A few hundred ragged series (lengths 0..700: the growing phase and the cut at 500), NULL masks, constant, all-zero, spike and
    real-valued series, lambda in {250, 10, 1, 0.5, -1}: every probability to REL_TOL, every flag exactly, and the single, batch
    and device entries bit-equal to one another."""
    api, lib, torch = env
    series, valids, ref = parity
    clean = [R.masked(y, v) for y, v in zip(series, valids)]
    worst, n_flags, n_points, nearest = 0.0, 0, 0, 1.0
    for lam in R.PARITY_LAMBDAS:
        got = api.changepoints_batch(series, lam, valids)
        dprob, dflag, dcnt = _device(lib, torch, clean, lam)
        for s, (y, want) in enumerate(zip(clean, ref[lam])):
            g = got[s]
            one = _single(lib, y, lam)
            n = len(y)
            assert np.all(dprob[n:, s] == -7.0) and np.all(dflag[n:, s] == 9)                 # rows past the series: untouched
            if want is None:
                assert n < 3 and not g["ok"] and g["code"] == lib.COMPUTATION_ERROR and g["n_changepoints"] == -1
                assert g["message"] == f"Insufficient data: need at least 3 observations, got {n}"
                assert not one[0] and one[2] == g["message"]
                assert dcnt[s] == -1 and np.all(dprob[:, s] == -7.0) and np.all(dflag[:, s] == 9)
                continue
            flags, prob = want
            assert g["ok"], (lam, s, g)
            d = R.rel(g["probability"], prob)
            print(f"lambda {lam:6.1f} series {s:3d} n {n:3d} rel {d:.3e}") if d > 1e-14 else None
            worst = max(worst, d)
            assert d <= REL_TOL, (lam, s, d)
            assert np.array_equal(g["is_changepoint"], flags), (lam, s)                       # no point excluded
            assert g["n_changepoints"] == int(flags.sum()) == dcnt[s]
            # the three entries: the same bits
            assert one[0] and np.array_equal(one[4], g["probability"], equal_nan=True) and np.array_equal(one[3], g["is_changepoint"])
            assert one[5] == [int(i) for i in np.nonzero(flags)[0]]
            assert np.array_equal(dprob[:n, s], g["probability"], equal_nan=True)
            assert np.array_equal(dflag[:n, s].astype(bool), g["is_changepoint"]) and set(np.unique(dflag[:n, s])) <= {0, 1}
            n_flags += int(flags.sum())
            n_points += n
            nearest = min(nearest, float(np.min(np.abs(prob - 0.5))))
    print(f"max GPU-vs-restatement difference {worst:.3e} over {n_points} points, {n_flags} flags, nearest probability to 0.5 {nearest:.3e}")
    assert n_flags > 500 and nearest > 1e-9


def test_device_entry_is_deterministic(env, parity):
    api, lib, torch = env
    series, valids, _ = parity
    clean = [R.masked(y, v) for y, v in zip(series, valids)]
    a = _device(lib, torch, clean, 250.0)
    b = _device(lib, torch, clean, 250.0)
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)
    # the company does not matter: a series alone gives the bits it gives inside the batch
    for s in (16, 17, 40):
        alone = _device(lib, torch, [clean[s]], 250.0)
        n = len(clean[s])
        assert np.array_equal(alone[0][:n, 0], a[0][:n, s], equal_nan=True) and alone[2][0] == a[2][s]


def test_one_short_series_fails_alone(env):
    api, lib, torch = env
    rng = np.random.default_rng(8)
    series = [rng.poisson(2.0, 50).astype(np.float64), np.array([1.0, 2.0]), 10.0 * rng.standard_normal(77)]
    got = api.changepoints_batch(series, 10.0)
    assert [g["ok"] for g in got] == [True, False, True]
    assert got[1]["code"] == lib.COMPUTATION_ERROR and got[1]["message"] == "Insufficient data: need at least 3 observations, got 2"
    assert got[1]["probability"] is None and got[1]["n_changepoints"] == -1
    for s in (0, 2):
        want = R.ffi_bocpd(series[s], 10.0)
        assert R.rel(got[s]["probability"], want[1]) <= REL_TOL and np.array_equal(got[s]["is_changepoint"], want[0])
    dprob, dflag, dcnt = _device(lib, torch, series, 10.0)
    assert dcnt[1] == -1 and np.all(dprob[:, 1] == -7.0) and np.all(dflag[:, 1] == 9)
    assert np.all(dprob[50:, 0] == -7.0) and np.all(dprob[:, 3:] == -7.0) and np.all(dcnt[3:] == -99)
    assert np.array_equal(dprob[:50, 0], got[0]["probability"]) and np.array_equal(dprob[:77, 2], got[2]["probability"])
    # batch-level failures and the empty batch
    L = lib.load()
    berr = lib.AnofoxError()
    assert not L.anofox_hip_changepoints_batch(None, None, None, 1, 250.0, None, None, None, None, C.byref(berr)) and berr.code == lib.NULL_POINTER
    assert L.anofox_hip_changepoints_batch(None, None, None, 0, 250.0, None, None, None, None, C.byref(berr))
    assert api.changepoints_batch([]) == []
    err = lib.AnofoxError()
    assert not L.anofox_hip_changepoints_device(None, 64, None, 1, 1, 250.0, None, None, None, None, C.byref(err)) and err.code == lib.NULL_POINTER


def test_non_finite_values_follow_the_arithmetic(env):
    """No special casing: a NaN reaches the sums, the `> 1e-300` test fails, the probabilities from there on are NaN and never
    flagged -- as the restatement (the same arithmetic) gives."""
    api, lib, torch = env
    rng = np.random.default_rng(12)
    y = rng.standard_normal(40)
    y[20] = np.nan
    z = rng.standard_normal(40)
    z[10] = np.inf
    got = api.changepoints_batch([y, z], 10.0)
    for g, v in zip(got, (y, z)):
        want = R.ffi_bocpd(v, 10.0)
        assert g["ok"] and R.rel(g["probability"], want[1]) <= REL_TOL and np.array_equal(g["is_changepoint"], want[0])
    assert np.all(np.isnan(got[0]["probability"][20:])) and not got[0]["is_changepoint"][20:].any()
