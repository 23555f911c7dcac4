"""MinT-shrink without a GPU: the two routes of the yardstick against each other on every case, the conditions the cases promise
(the estimated intensity strictly inside (0, 1), cond(M) <= 1e6), anofox_hip_reconcile_mint_sizes, every refusal that needs no
device through the C entries and the mirrors, the loud failure without a device, and the host-only checks under sanitizers."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mint_cases as MC  # noqa: E402
import mint_ref as MR  # noqa: E402
import reconcile_cases as RC  # noqa: E402
import reconcile_ref as R  # noqa: E402

from anofox_forecast_amd import api, lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL_POINTER, INVALID_INPUT, INTERNAL_ERROR = 1, 2, 10
NAN = float("nan")


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:  # noqa: BLE001
        return False


# ---- the yardsticks and the cases ----
def test_cases_cover_the_shapes_the_kernels_switch_on():
    names = MC.names()
    assert len(names) == len(set(names))
    for plan in MC.PLANS:
        n_agg = len(RC.plan_parts(plan)["agg_cols"])
        vals = MC.n_res_values(plan)
        assert {2, 3, 63, 64, 65} <= set(vals) and any(v > n_agg for v in vals)
        assert n_agg < 4 or any(2 <= v < n_agg for v in vals)                      # a rank-deficient sample covariance
    assert {len(RC.plan_parts(plan)["agg_cols"]) for plan in MC.PLANS} >= {1, 64, 65, 129, 197}
    assert RC.empty_columns("small") and RC.empty_columns("agg129")
    twice = RC.plan_parts("leaf1_twice")
    assert twice["cols"][twice["agg_cols"][0]] == [0, 0]                           # a series counted twice


@pytest.mark.parametrize("name", MC.names())
def test_yardstick_routes_agree_and_the_case_keeps_its_conditions(name):
    c, p = MC.case(name), MC.parts(name)
    part = MR.participants(p)
    dense, gram, lam_tol = MC.shrinkage(name)
    raw = float(MR.shrinkage_dense(p, c["residuals"])[1])
    assert 0.0 < raw < 1.0 and dense == raw, "the estimated intensity is clamped"
    assert abs(gram - dense) <= 1e-12 * dense and lam_tol >= 16 * MC.EPS * dense    # the Gram route against the dense pairwise formula
    v = MC.variances(name)
    X = c["residuals"][part]
    assert np.allclose(v[part], (X ** 2).sum(1) / c["n_res"], rtol=1e-13, atol=0.0) and (v[MC.empty_columns(name)] == 0.0).all()
    M = MR.system_matrix(p, c["residuals"], gram, v)
    assert np.linalg.cond(M) <= 1e6
    if c["n_res"] < len(p["agg_cols"]):                                             # M is positive definite only through lambda > 0
        E = MR.incoherence(p, c["residuals"])
        assert np.linalg.matrix_rank(E.T @ E) < len(p["agg_cols"])
    assert (c["residuals"][p["agg_cols"]] != (p["A"] @ c["residuals"][p["bottom_col"]])).all()      # the residuals are incoherent
    yard, tol = MC.yardstick(name)
    plain = MR.constraint_fp64(p, c["residuals"], gram, c["yhat"])
    scale = float(np.max(np.abs(c["yhat"][part])))
    assert np.isfinite(yard).all() and tol >= 16 * MC.EPS * scale
    assert float(np.max(np.abs(plain[part] - yard[part]))) <= 64 * MC.EPS * scale * 1e6      # the two routes: within cond(M) roundings
    assert R.coherent_to_the_bit(p, c["yhat"]).sum() < R.coherent_to_the_bit(p, c["yhat"]).size or not p["agg_cols"]
    for e in MC.empty_columns(name):
        assert (plain[e] == c["yhat"][e]).all() and (yard[e] == c["yhat"][e]).all()


def test_intensity_one_is_wls_var_with_the_variances():
    name = "agg65-64"
    c, p = MC.case(name), MC.parts(name)
    part = MR.participants(p)
    v = MC.variances(name)
    a = MR.constraint_fp64(p, c["residuals"], 1.0, c["yhat"])
    b = R.constraint_fp64(p, np.where(v > 0, v, 1.0), c["yhat"])
    assert np.allclose(a[part], b[part], rtol=1e-9, atol=0.0)
    w1 = MR.dense_w(p, c["residuals"], 1.0)
    assert (w1 == np.diag(np.diag(w1))).all()


# ---- anofox_hip_reconcile_mint_sizes ----
def test_sizes_entry():
    s = lib.reconcile_mint_sizes(140, 14, 28)
    assert s == {"gram": 64 * 140 * 140 + 2 * 6, "e": 140 * 14, "factor": 14 * 14, "work": 28 * (14 + 140)}
    s = lib.reconcile_mint_sizes(1913, 12350, 28)
    assert s["gram"] == 5 * 1913 * 1913 + 2 * 465 and s["e"] == 1913 * 12350 and s["work"] == 28 * (12350 + 1913)
    assert lib.reconcile_mint_sizes(lib.RECONCILE_MAX_RESIDUAL_ROWS, 0, 0)["gram"] * 8 < 2 ** 30
    for n_res, text in ((1, "n_res is 1"), (lib.RECONCILE_MAX_RESIDUAL_ROWS + 1, "n_res 8193 exceeds the limit of 8192 residual rows")):
        with pytest.raises(ValueError, match=text):
            lib.reconcile_mint_sizes(n_res, 3, 3)
    with pytest.raises(ValueError, match="n_agg 16385 exceeds the limit of 16384"):
        lib.reconcile_mint_sizes(10, lib.RECONCILE_MAX_AGG + 1, 3)
    L, err = lib.load(), lib.AnofoxError()
    one = C.c_size_t(5)
    assert not L.anofox_hip_reconcile_mint_sizes(10, 3, 3, None, C.byref(one), C.byref(one), C.byref(one), C.byref(err)) and err.code == NULL_POINTER
    header = open(os.path.join(ROOT, "include", "anofox_fcst_hip.h")).read()
    assert "#define ANOFOX_HIP_RECONCILE_MAX_RESIDUAL_ROWS 8192" in header


def test_host_checks_under_sanitizers():
    """csrc/host_reconcile_mint.hpp compiled on its own (no HIP) and run as a program under ASan + UBSan
    (tests/c_abi/reconcile_mint_san.cpp): the sizes for every n_res, every refusal and its text."""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "reconcile_mint_san")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               os.path.join(ROOT, "tests", "c_abi", "reconcile_mint_san.cpp"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("reconcile_mint_san: ok"), (r.stdout, r.stderr[-3000:])


# ---- the entries without a device: argument errors first, then the loud failure ----
def _factor(L, err, **k):
    p = np.zeros(64).ctypes.data                                                   # never dereferenced: every call below is refused first
    lam = C.c_double(-5.0)
    ok = L.anofox_hip_reconcile_mint_factor_device(k.get("res", p), 5, 1, k.get("n_res", 5), p, p, k.get("n_out", 4), 6, k.get("n_series", 2), p, p,
                                                   k.get("n_agg", 2), p, p, 4, k.get("shrinkage", NAN), k.get("variances", p), k.get("e", p),
                                                   k.get("ld_e", 2), k.get("factor", p), k.get("ld_a", 2), k.get("gram", p),
                                                   C.byref(lam) if k.get("out", True) else None, None, C.byref(err))
    assert lam.value == -5.0 or ok
    return ok


def _apply(L, err, **k):
    p = np.zeros(64).ctypes.data
    return L.anofox_hip_reconcile_mint_apply_device(k.get("base", p), 3, 1, k.get("n_rows", 3), k.get("res", p), 5, 1, k.get("n_res", 5), p, p,
                                                    k.get("n_out", 4), 6, 2, p, p, k.get("n_agg", 2), p, p, 4, k.get("variances", p), p,
                                                    k.get("ld_e", 2), k.get("shrinkage", 0.5), k.get("factor", p), k.get("ld_a", 2), k.get("work", p),
                                                    p, p, None, C.byref(err))


def test_device_entries_refuse_bad_arguments_on_the_host():
    L, err = lib.load(), lib.AnofoxError()
    for entry in (_factor, _apply):
        assert not entry(L, err, n_res=1) and err.code == INVALID_INPUT and b"n_res is 1" in err.message
        assert not entry(L, err, n_res=lib.RECONCILE_MAX_RESIDUAL_ROWS + 1) and err.code == INVALID_INPUT and b"exceeds the limit of 8192 residual rows" in err.message
        for bad in (-0.25, 1.5, float("inf")):
            assert not entry(L, err, shrinkage=bad) and err.code == INVALID_INPUT and b"lies outside [0, 1]" in err.message
        assert not entry(L, err, n_agg=lib.RECONCILE_MAX_AGG + 1) and err.code == INVALID_INPUT and b"exceeds the limit of 16384" in err.message
        assert not entry(L, err, ld_e=1) and err.code == INVALID_INPUT and b"ld_e is smaller than n_agg" in err.message
        assert not entry(L, err, ld_a=1) and err.code == INVALID_INPUT and b"ld_a is smaller than n_agg" in err.message
        assert not entry(L, err, n_out=2 ** 31) and err.code == INVALID_INPUT and b"limited to 2^31 - 1" in err.message
        assert not entry(L, err, res=None) and err.code == NULL_POINTER
        assert not entry(L, err, variances=None) and err.code == NULL_POINTER
    assert not _factor(L, err, n_series=2 ** 31 - 1) and err.code == INVALID_INPUT and b"participating columns" in err.message
    assert not _factor(L, err, gram=None) and err.code == NULL_POINTER              # an estimate needs its workspace
    assert not _factor(L, err, factor=None) and err.code == NULL_POINTER
    assert not _factor(L, err, out=False) and err.code == NULL_POINTER
    assert not _apply(L, err, shrinkage=NAN) and err.code == INVALID_INPUT and b"the shrinkage intensity is NaN" in err.message
    assert not _apply(L, err, factor=None) and err.code == INVALID_INPUT and b"needs the factor of anofox_hip_reconcile_mint_factor_device" in err.message
    assert not _apply(L, err, work=None) and err.code == NULL_POINTER
    assert not _apply(L, err, base=None) and err.code == NULL_POINTER
    assert _apply(L, err, n_rows=0), err.message                                   # nothing to do needs no device


def test_batch_and_mirror_refusals_need_no_device():
    co = [[0, 0], [1, 2]]
    f, r = np.zeros((3, 2)), np.ones((3, 5))
    for bad, text in ((np.ones((3, 1)), "n_res is 1"), (np.ones((3, lib.RECONCILE_MAX_RESIDUAL_ROWS + 1)), "exceeds the limit of 8192 residual rows")):
        out, e = api.reconcile_mint_batch(co, f, bad)
        assert not e["ok"] and e["code"] == INVALID_INPUT and text in e["message"]
    for bad in (-0.5, 2.0):
        out, e = api.reconcile_mint_batch(co, f, r, shrinkage=bad)
        assert not e["ok"] and e["code"] == INVALID_INPUT and "lies outside [0, 1]" in e["message"] and np.isnan(out["y"]).all()
    out, e = api.reconcile_mint_batch([[0, 0], [1, -1]], np.zeros((2, 2)), np.ones((2, 5)))      # the planner's refusal
    assert not e["ok"] and e["code"] == INVALID_INPUT and "series 1 has no bottom column" in e["message"]
    with pytest.raises(ValueError, match="3 output columns"):
        api.reconcile_mint_batch(co, np.zeros((4, 2)), r)
    with pytest.raises(ValueError, match="the residual block has 2 rows"):
        api.reconcile_mint_batch(co, f, np.ones((2, 5)))
    assert lib.RECONCILE_METHODS == {"bottom_up": 0, "ols": 1, "wls_struct": 2, "wls_var": 3}
    # the mirror
    uid = ["A|AGGREGATED", "A|AGGREGATED", "A|x", "A|x", "A|y", "A|y"]
    days = np.array(["2024-01-01", "2024-01-02"] * 3, dtype="datetime64[D]")
    fc = np.arange(6, dtype=np.float64)
    with pytest.raises(api.InvalidInputException, match="mint_shrink needs residuals"):
        api.ts_reconcile_hierarchy(uid, days, fc, {"method": "mint_shrink"})
    with pytest.raises(api.InvalidInputException, match=r"mint_shrink needs residuals for the ids \['A\|y'\]"):
        api.ts_reconcile_hierarchy(uid, days, fc, {"method": "mint_shrink", "residuals": (uid[:4], days[:4], fc[:4])})
    with pytest.raises(api.InvalidInputException, match=r"the residual dates of the ids \['A\|y'\] differ"):
        api.ts_reconcile_hierarchy(uid, days, fc, {"method": "mint_shrink", "residuals": (uid[:5], days[:5], fc[:5])})
    with pytest.raises(api.InvalidInputException, match="n_res is 1"):
        api.ts_reconcile_hierarchy(uid, days, fc, {"method": "mint_shrink", "residuals": (uid[::2], days[::2], fc[::2])})
    with pytest.raises(api.InvalidInputException, match=r"lies outside \[0, 1\]"):
        api.ts_reconcile_hierarchy(uid, days, fc, {"method": "mint_shrink", "residuals": (uid, days, fc), "shrinkage": 1.5})
    with pytest.raises(api.InvalidInputException, match="unknown method 'top_down'"):
        api.ts_reconcile_hierarchy(uid, days, fc, {"method": "top_down"})


@pytest.mark.skipif(_has_gpu(), reason="GPU present: the entries run (tests/test_gpu_mint.py)")
def test_entries_without_a_device_have_no_cpu_fallback():
    L, err = lib.load(), lib.AnofoxError()
    assert not _factor(L, err) and err.code == INTERNAL_ERROR and b"no CPU fallback" in err.message
    assert not _factor(L, err, shrinkage=0.5, gram=None) and err.code == INTERNAL_ERROR and b"no CPU fallback" in err.message
    assert not _apply(L, err) and err.code == INTERNAL_ERROR and b"no CPU fallback" in err.message
    c = MC.case("small-7")
    out, e = api.reconcile_mint_batch(c["column_of"], c["yhat"], c["residuals"])
    assert not e["ok"] and e["code"] == INTERNAL_ERROR and "no CPU fallback" in e["message"]
