"""Reconciliation of hierarchy forecasts without a GPU: the three yardsticks against each other on every case, the host-only planner
against a Python transpose with every limit and its message, the mirror's key parsing against BuildUniqueId, the entries' argument
errors (which come before the device is looked for) and their loud failure without a device, and the planner under sanitizers."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hierarchy_ref as HR  # noqa: E402
import reconcile_cases as RC  # noqa: E402
import reconcile_ref as R  # noqa: E402

from anofox_forecast_amd import api, lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL_POINTER, INVALID_INPUT, INTERNAL_ERROR = 1, 2, 10
SOLVED = ("ols", "wls_struct", "wls_var")


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:  # noqa: BLE001
        return False


# ---- the yardsticks ----
def test_cases_cover_the_shapes_the_kernels_switch_on():
    cases = RC.all_cases()
    n_agg = {len(RC.plan_parts(n)["agg_cols"]) for n in cases}
    assert {0, 1, 2, 63, 64, 65, 129, 197} <= n_agg
    assert {c["n_series"] for c in cases.values()} >= {1, 6, 70, 300} and {c["rows"] for c in cases.values()} >= {1, 3, 65}
    small = RC.plan_parts("small")
    lists = [tuple(small["cols"][c]) for c in small["agg_cols"]]
    assert len(set(lists)) < len(lists)                                          # two identical aggregates
    assert any(len(set(ms)) < len(ms) for ms in lists) and RC.empty_columns("small")      # a series listed twice; an empty column
    assert max(len(RC.plan_parts("agg197")["cols"][c]) for c in RC.plan_parts("agg197")["agg_cols"]) == 300
    for c in cases.values():                                                     # wls_var weights within a ratio of 10^6
        assert c["weights"].max() / c["weights"].min() <= 1e6
    pre = cases["prefix_cancel"]
    p = RC.plan_parts("prefix_cancel")
    total = [c for c in p["agg_cols"] if len(p["cols"][c]) == 6][0]
    chain = R.bottom_up(p, pre["yhat"])[total]
    assert chain[0] != float(np.sum(np.sort(pre["yhat"][p["bottom_col"], 0])))   # an order-agnostic sum fails the bit check


@pytest.mark.parametrize("name", RC.names())
def test_plain_fp64_against_the_exact_and_the_long_double_projection(name):
    c, p = RC.all_cases()[name], RC.plan_parts(name)
    part = RC.participants(name)
    eps = np.finfo(np.float64).eps
    for method in SOLVED:
        w = R.method_weights(p, method, c["weights"])
        plain = R.constraint_fp64(p, w, c["yhat"])
        ext = R.project_longdouble(p, w, c["yhat"])
        scale = float(np.max(np.abs(c["yhat"][part])))
        spread = float(w[part].max() / w[part].min())
        # (c) against (b): the noise of the problem grows with the spread of the weights, never past 1e-9 here
        assert float(np.max(np.abs(plain[part] - ext[part]))) <= 64 * eps * scale * max(spread, 1.0) * max(len(p["agg_cols"]), 1)
        if c["n_out"] <= 40:
            exact = R.project_exact(p, w, c["yhat"])
            assert float(np.max(np.abs(ext[part] - exact[part]))) <= 4 * eps * scale      # (b) against (a): long double has 11 bits to spare
        yard, tol, _w = RC.yardstick(name, method)
        assert tol >= 16 * eps * scale and np.isfinite(yard).all()
        for e in RC.empty_columns(name):
            assert HR.same_bits(plain[e], c["yhat"][e]).all()


def test_bottom_up_restatement_is_the_aggregation_chain():
    c, p = RC.all_cases()["prefix_cancel"], RC.plan_parts("prefix_cancel")
    y = R.bottom_up(p, c["yhat"])
    assert R.coherent_to_the_bit(p, y).all() and HR.same_bits(y[p["bottom_col"]], c["yhat"][p["bottom_col"]]).all()
    series = [c["yhat"][p["bottom_col"][s]] for s in range(6)]
    cols = HR.aggregate_block(series, [0] * 6, c["col_offsets"].tolist(), c["members"].tolist())
    for col in p["agg_cols"]:
        assert HR.same_bits(y[col], np.array(cols[col][2])).all()
    assert not R.coherent_to_the_bit(p, c["yhat"]).all()                         # the base forecasts are incoherent on purpose


# ---- anofox_hip_reconcile_plan ----
@pytest.mark.parametrize("name", RC.names())
def test_planner_against_the_python_transpose(name):
    c, p = RC.all_cases()[name], RC.plan_parts(name)
    n_out, offs, memb = lib.hierarchy_plan(c["column_of"])
    assert n_out == c["n_out"] and offs.tolist() == c["col_offsets"].tolist() and memb.tolist() == c["members"].tolist()
    got = lib.reconcile_plan(offs, memb, c["n_series"])
    assert got["bottom_col"].tolist() == p["bottom_col"] and got["agg_cols"].tolist() == p["agg_cols"]
    assert got["leaf_aggs"].tolist() == [i for held in p["leaf"] for i in held]
    assert got["leaf_offsets"].tolist() == np.concatenate([[0], np.cumsum([len(h) for h in p["leaf"]])]).tolist()
    assert got["struct_weights"].tolist() == p["struct_weights"]
    assert (got["n_agg"], got["n_leaf"]) == (len(p["agg_cols"]), sum(len(h) for h in p["leaf"]))


def _plan_raw(offs, memb, n_series, arrays=True):
    L = lib.load()
    offs, memb = np.ascontiguousarray(offs, dtype=np.int32), np.ascontiguousarray(memb, dtype=np.int32)
    n_agg, n_leaf, err = C.c_size_t(77), C.c_size_t(77), lib.AnofoxError()
    bufs = [np.full(64, -7, dtype=np.int32) for _ in range(4)] + [np.full(64, -7.0)]
    ptrs = [b.ctypes.data for b in bufs] if arrays else [None] * 5
    ok = L.anofox_hip_reconcile_plan(offs.ctypes.data, memb.ctypes.data, len(offs) - 1, n_series, C.byref(n_agg), C.byref(n_leaf), *ptrs, C.byref(err))
    return ok, n_agg.value, n_leaf.value, err, bufs


def test_planner_sizing_call_and_limits():
    ok, n_agg, n_leaf, err, _ = _plan_raw([0, 1, 3, 3, 4], [0, 0, 1, 1], 2, arrays=False)
    assert ok and (n_agg, n_leaf) == (1, 2), err.message
    refusals = [([0, 1, 3], [0, 0, 2], 2, b"plan entry 2 names series 2, outside [0, 2)"),
                ([0, 1, 3], [0, 0, 1], 2, b"series 1 has no bottom column"),
                ([0, 1, 2, 3], [0, 1, 0], 2, b"series 0 has two bottom columns, 0 and 2"),
                ([0, 2, 1, 3], [0, 1, 0], 2, b"col_offsets descends at column 1")]
    for offs, memb, n, text in refusals:
        ok, _a, _l, err, bufs = _plan_raw(offs, memb, n)
        assert not ok and err.code == INVALID_INPUT and text in err.message, err.message
        assert all((b == -7).all() for b in bufs)                                # a refusal writes no array
    # n_agg above ANOFOX_HIP_RECONCILE_MAX_AGG: 16,385 aggregates of the same two leaves
    n_agg = lib.RECONCILE_MAX_AGG + 1
    offs = np.concatenate([[0, 1, 2], 2 + 2 * np.arange(1, n_agg + 1)])
    memb = np.concatenate([[0, 1], np.tile([0, 1], n_agg)])
    ok, a, _l, err, _ = _plan_raw(offs, memb, 2, arrays=False)
    assert not ok and err.code == INVALID_INPUT and b"n_agg 16385 exceeds the limit of 16384 aggregate columns" in err.message and a == n_agg
    ok, a, _l, err, _ = _plan_raw(offs[:-1], memb[:-2], 2, arrays=False)
    assert ok and a == lib.RECONCILE_MAX_AGG
    header = open(os.path.join(ROOT, "include", "anofox_fcst_hip.h")).read()
    assert "#define ANOFOX_HIP_RECONCILE_MAX_AGG 16384" in header
    L = lib.load()
    err = lib.AnofoxError()
    one = np.zeros(4, dtype=np.int32)
    assert not L.anofox_hip_reconcile_plan(one.ctypes.data, one.ctypes.data, 1, 1, None, None, None, one.ctypes.data, None, None, None, C.byref(err))
    assert err.code == NULL_POINTER
    with pytest.raises(ValueError, match="has no bottom column"):
        lib.reconcile_plan([0, 2], [0, 1], 2)


def test_planner_under_sanitizers():
    """csrc/host_reconcile_plan.hpp compiled on its own (no HIP) with exactly sized arrays and run as a program under ASan + UBSan
    (tests/c_abi/reconcile_san.cpp): the plan against a brute-force restatement, every refusal, null arrays."""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "reconcile_san")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               os.path.join(ROOT, "tests", "c_abi", "reconcile_san.cpp"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("reconcile_san: ok"), (r.stdout, r.stderr[-3000:])


# ---- the entries without a device: argument errors first, then the loud failure ----
def _apply(L, err, **k):
    p = np.zeros(64).ctypes.data                                                 # never dereferenced: every call below is refused first
    return L.anofox_hip_reconcile_apply_device(k.get("base", p), 3, 1, k.get("n_rows", 3), p, p, k.get("n_out", 4), 6, 2, p, p, k.get("n_agg", 2), p, p,
                                               4, k.get("method", 1), k.get("weights", None), k.get("factor", p), k.get("ld_a", 2),
                                               k.get("work", p), p, p, None, C.byref(err))


def _factor(L, err, **k):
    p = np.zeros(64).ctypes.data
    return L.anofox_hip_reconcile_factor_device(p, p, 4, 6, 2, p, p, k.get("n_agg", 2), p, p, 4, k.get("method", 1), k.get("weights", None),
                                                k.get("factor", p), k.get("ld_a", 2), None, C.byref(err))


def test_device_entries_refuse_bad_arguments_on_the_host():
    L, err = lib.load(), lib.AnofoxError()
    assert not _factor(L, err, method=0) and err.code == INVALID_INPUT and b"a factor exists for method 1" in err.message
    assert not _factor(L, err, method=4) and err.code == INVALID_INPUT
    assert not _factor(L, err, n_agg=lib.RECONCILE_MAX_AGG + 1) and err.code == INVALID_INPUT and b"exceeds the limit of 16384" in err.message
    assert not _factor(L, err, ld_a=1) and err.code == INVALID_INPUT and b"ld_a is smaller than n_agg" in err.message
    assert not _factor(L, err, method=3) and err.code == NULL_POINTER            # wls_var without weights
    assert not _factor(L, err, factor=None) and err.code == NULL_POINTER
    assert not _apply(L, err, method=7) and err.code == INVALID_INPUT and b"method must be 0 (bottom_up)" in err.message
    assert not _apply(L, err, factor=None) and err.code == INVALID_INPUT and b"need the factor" in err.message
    assert not _apply(L, err, ld_a=1) and err.code == INVALID_INPUT and b"ld_a is smaller than n_agg" in err.message
    assert not _apply(L, err, work=None) and err.code == NULL_POINTER
    assert not _apply(L, err, base=None) and err.code == NULL_POINTER
    assert not _apply(L, err, n_out=2**31) and err.code == INVALID_INPUT and b"limited to 2^31 - 1" in err.message
    assert _apply(L, err, n_rows=0), err.message                                 # nothing to do needs no device
    with pytest.raises(ValueError, match="unknown reconciliation method"):
        api.reconcile_batch([[0, 0], [1, 2]], np.zeros((3, 2)), "top_down")
    with pytest.raises(ValueError, match="3 output columns"):
        api.reconcile_batch([[0, 0], [1, 2]], np.zeros((4, 2)), "ols")
    out, e = api.reconcile_batch([[0, 1]], np.zeros((2, 2)), "wls_var")            # wls_var without weights
    assert not e["ok"] and e["code"] == NULL_POINTER
    out, e = api.reconcile_batch([[0, 0], [1, -1]], np.zeros((2, 2)), "ols")       # the planner's refusal needs no device
    assert not e["ok"] and e["code"] == INVALID_INPUT and "series 1 has no bottom column" in e["message"]
    assert lib.RECONCILE_METHODS == {"bottom_up": 0, "ols": 1, "wls_struct": 2, "wls_var": 3}


@pytest.mark.skipif(_has_gpu(), reason="GPU present: the entries run (tests/test_gpu_reconcile.py)")
def test_entries_without_a_device_have_no_cpu_fallback():
    L, err = lib.load(), lib.AnofoxError()
    assert not _factor(L, err) and err.code == INTERNAL_ERROR and b"no CPU fallback" in err.message
    assert not _apply(L, err) and err.code == INTERNAL_ERROR and b"no CPU fallback" in err.message
    c = RC.all_cases()["small"]
    out, e = api.reconcile_batch(c["column_of"], c["yhat"], "ols")
    assert not e["ok"] and e["code"] == INTERNAL_ERROR and "no CPU fallback" in e["message"]


# ---- the mirror's key parsing ----
def _keys(leaves, sep="|", keyword="AGGREGATED"):
    return sorted({HR.build_unique_id(list(l), lv, sep, keyword) for l in leaves for lv in range(len(leaves[0]) + 1)}, key=lambda u: u.encode())


@pytest.mark.parametrize("sep,keyword", [("|", "AGGREGATED"), ("::", "ALL"), ("", "AGGREGATED")])
def test_mirror_key_parsing_against_build_unique_id(sep, keyword):
    leaves = [("EU", "S1", "a"), ("EU", "S1", "b"), ("EU", "S2", "c"), ("EU", "S2", "d"), ("US", "S3", "e"), ("US", "S3", "f"), ("US", "S4", "g"),
              ("US", "S4", "h")]
    if not sep:
        leaves = [(l[2],) for l in leaves]                                       # a separator inside no id: one part, total and leaves
    keys = _keys(leaves, sep, keyword)
    names, leaf_ids, column_of = api._reconcile_columns(keys + keys[:3], sep, keyword)
    assert names == keys
    assert leaf_ids == sorted((HR.build_unique_id(list(l), len(l), sep, keyword) for l in leaves), key=lambda u: u.encode())
    N = len(leaves[0])
    assert column_of.shape == (N + 1, len(leaves))
    by_id = {HR.build_unique_id(list(l), N, sep, keyword): l for l in leaves}
    for s, u in enumerate(leaf_ids):
        for level in range(N + 1):                                               # the keyword at every level
            assert names[column_of[level, s]] == api._hierarchy_unique_id(list(by_id[u]), level, sep, keyword) == \
                HR.build_unique_id(list(by_id[u]), level, sep, keyword)
    _n, offs, memb = HR.plan(column_of.tolist())
    p = R.parts(offs, memb, len(leaves))
    assert len(p["agg_cols"]) == len(keys) - len(leaves)


def test_mirror_errors_name_the_ids():
    leaves = [("EU", "S1"), ("EU", "S2"), ("US", "S3"), ("US", "S4")]
    keys = _keys(leaves)
    days = np.array(["2024-01-01", "2024-01-02"], dtype="datetime64[D]")
    uid = [u for u in keys for _ in days]
    date = np.array([d for _ in keys for d in days])
    fc = np.arange(len(uid), dtype=np.float64)
    with pytest.raises(api.InvalidInputException, match=r"no leaf lies beneath the aggregate ids \['ZZ\|AGGREGATED'\]"):
        api.ts_reconcile_hierarchy(uid + ["ZZ|AGGREGATED"] * 2, np.concatenate([date, days]), np.concatenate([fc, [1.0, 2.0]]))
    with pytest.raises(api.InvalidInputException, match=r"the dates of the ids \['US\|S4'\] differ"):
        api.ts_reconcile_hierarchy(uid[:-1], date[:-1], fc[:-1])
    holes = fc.astype(object)
    holes[uid.index("EU|S2")] = None
    with pytest.raises(api.InvalidInputException, match=r"the leaf ids \['EU\|S2'\] have no forecast"):
        api.ts_reconcile_hierarchy(uid, date, holes)
    with pytest.raises(api.InvalidInputException, match="unknown method 'top_down'"):
        api.ts_reconcile_hierarchy(uid, date, fc, {"method": "top_down"})
    with pytest.raises(api.InvalidInputException, match="same number of parts"):
        api.ts_reconcile_hierarchy(uid + ["EU"], np.concatenate([date, days[:1]]), np.concatenate([fc, [1.0]]))
    with pytest.raises(api.InvalidInputException, match=r"wls_var needs a weight for the ids"):
        api.ts_reconcile_hierarchy(uid, date, fc, {"method": "wls_var", "weights": {"EU|S1": 1.0}})
    # a region with ONE store: the store's leaf and the region hold the same single series -- two bottom columns, refused by name
    lone = _keys([("EU", "S1"), ("EU", "S2"), ("US", "S3")])
    with pytest.raises(api.InvalidInputException, match="has two bottom columns"):
        api.ts_reconcile_hierarchy(lone, np.repeat(days[:1], len(lone)), np.ones(len(lone)))
