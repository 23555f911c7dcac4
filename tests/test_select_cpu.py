"""CPU: the selection entries without a device -- the restatement tests/select_ref.py against brute force, math.fsum and
statistics.median; the seeded inputs of tests/select_cases.py have the properties the GPU tests rely on; the new symbols in the
header and in lib.EXPORTED_SYMBOLS; every argument error and its text (they come before the device is touched); the host-only logic
csrc/host_select_plan.hpp under ASan + UBSan as a stand-alone program; and the product never imports the restatement."""
import ctypes as C
import math
import os
import re
import statistics
import subprocess
import tempfile

import numpy as np
import pytest

import select_cases as K
import select_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "anofox_fcst_hip.h")
NEW_SYMBOLS = ("anofox_hip_select_winner_device", "anofox_hip_select_gather_device", "anofox_hip_select_scatter_device",
               "anofox_hip_select_combine_device", "anofox_hip_select_batch")
EPS = 2.0 ** -52


# --------------------------------------------------------------------------------------------
# the restatement
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 3, 16])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("fallback", [-1, 0])
def test_choice_against_brute_force(N, M, fallback):
    scores, status = K.score_table(N, M, 1000 * N + M)
    winner, best, ff, offsets, members = R.choose(scores[:, :N].tolist(), status.tolist(), fallback)
    for s in range(N):
        tuples = [(scores[m, s], m) for m in range(M) if status[m, s] == 0 and not math.isnan(scores[m, s])]
        if tuples:
            sc, m = min(tuples)                               # the smallest score, the lowest m among equals (-0.0 == 0.0 in a tuple too)
            assert winner[s] == m and R.same_bits(best[s], scores[m, s]) and ff[s] == 0 and best[s] == sc
        else:
            assert winner[s] == fallback and math.isnan(best[s]) and ff[s] == (1 if fallback >= 0 else 0)
    want = sorted((winner[s], s) for s in range(N) if winner[s] >= 0)
    assert members == [s for _, s in want]
    assert offsets == [sum(1 for w, _ in want if w < m) for m in range(M + 1)]


@pytest.mark.parametrize("M", [1, 3, 16])
@pytest.mark.parametrize("N", [63, 64, 65, 1000])
def test_score_tables_have_their_properties(N, M):
    scores, status = K.score_table(N, M, 1000 * N + M)
    p = K.table_properties(scores, status, N, M, -1)
    lose = K.loser_of(M)
    assert all(p["wins"][m] >= 1 for m in range(M) if m != lose), p["wins"]
    assert lose < 0 or p["wins"][lose] == 0
    assert p["n_nan"] > 0 and p["n_inf"] > 0 and p["n_status"] > 0 and p["n_none"] > 0
    if M >= 3:
        assert 20 * p["ties"] >= N and p["three_way"] >= 1 and p["zero_tie"] >= 1, p
    q = K.table_properties(scores, status, N, M, 0)
    assert sum(q["from_fallback"]) == p["n_none"] and q["offsets"][M] == N and p["offsets"][M] == N - p["n_none"]


def test_order_key_is_the_total_order():
    values = [-math.inf, -3.5, -1e-300, -0.0, 0.0, 5e-324, 1.0, math.inf]
    keys = [R.order_key(v) for v in values]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)


@pytest.mark.parametrize("R_rows,h,group_div", [(1, 1, 1), (65, 3, 2), (300, 3, 1)])
def test_combine_against_fsum_and_median(R_rows, h, group_div):
    M = 16
    blocks, status, scores, winner = K.combine_case(R_rows, h, M, group_div, 7 * R_rows + h)
    bl, st, sc, wl = blocks.tolist(), status.tolist(), scores.tolist(), winner.tolist()
    mean, _ = R.combine(bl, st, "mean")
    med, med_status = R.combine(bl, st, "median")
    inv, _ = R.combine(bl, st, "inverse_score", scores=sc, group_div=group_div)
    pick, _ = R.combine(bl, st, "pick", winner=wl, group_div=group_div)
    counts = set()
    for r in range(R_rows):
        g = r // group_div
        for i in range(h):
            live = [m for m in range(M) if status[m, r] == 0 and not math.isnan(blocks[m, r, i])]
            counts.add(len(live))
            vals = [blocks[m, r, i] for m in live]
            assert R.same_bits(pick[r][i], blocks[winner[g], r, i] if winner[g] >= 0 else math.nan)
            if not live:
                assert math.isnan(mean[r][i]) and math.isnan(med[r][i]) and math.isnan(inv[r][i])
                continue
            bound = (len(vals) - 1) * EPS * math.fsum(abs(v) for v in vals)
            assert abs(mean[r][i] * len(vals) - math.fsum(vals)) <= bound + len(vals) * EPS * abs(mean[r][i])
            assert med[r][i] == statistics.median(vals)
            part = [m for m in live if not math.isnan(scores[m, g])]
            zero = [m for m in part if scores[m, g] == 0.0]
            if not part:
                assert math.isnan(inv[r][i])
            elif zero:
                zs = [blocks[m, r, i] for m in zero]
                assert abs(inv[r][i] * len(zs) - math.fsum(zs)) <= (len(zs) - 1) * EPS * math.fsum(abs(v) for v in zs) + len(zs) * EPS * abs(inv[r][i])
            else:
                w = [1.0 / scores[m, g] for m in part]
                terms = [wi * blocks[m, r, i] for wi, m in zip(w, part)]
                sw = math.fsum(w)
                if sw > 0.0:
                    exact = math.fsum(terms) / sw
                    k = len(part)
                    # every product, both sums and the quotient are rounded once each: (2 k + 1) roundings of terms bounded by the sum of
                    # their magnitudes
                    assert abs(inv[r][i] - exact) <= (2 * k + 1) * EPS * math.fsum(abs(t) for t in terms) / sw
                else:
                    assert math.isnan(inv[r][i])              # every weight 0 (all scores +inf): 0 / 0
        assert med_status[r] == (0 if any(not math.isnan(v) for v in med[r]) else 1)
    if R_rows >= 8:
        assert {0, 1, 2, 16} <= counts
        assert any(scores[m, g] == 0.0 for m in range(M) for g in range(scores.shape[1]))
    else:
        assert counts == {0} and med_status == [1]


def test_median_uses_the_total_order_of_zeros():
    assert R.same_bits(R.combine_cell([0.0, -0.0, 5.0], [0, 0, 0], "median"), 0.0)
    assert R.same_bits(R.combine_cell([0.0, -0.0, -5.0], [0, 0, 0], "median"), -0.0)
    assert R.combine_cell([1.0, 4.0], [0, 0], "median") == 2.5 and R.combine_cell([1.0, 4.0], [0, 1], "median") == 1.0


# --------------------------------------------------------------------------------------------
# the ABI
# --------------------------------------------------------------------------------------------
def test_symbols_declared_and_exported(hiplib):
    text = open(HEADER).read()
    L = hiplib.load()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % s, text), s
        assert s in hiplib.EXPORTED_SYMBOLS and hasattr(L, s)
    assert "#define ANOFOX_HIP_SELECT_MAX_METHODS 16" in text and hiplib.SELECT_MAX_METHODS == 16
    assert hiplib.SELECT_MODES == {"pick": 0, "mean": 1, "median": 2, "inverse_score": 3} and list(hiplib.SELECT_MODES) == list(R.MODES)
    assert hiplib.SELECT_CRITERIA == ("mae", "mse", "rmse", "mape", "smape")


def _no_device(hiplib):
    return hiplib.load().anofox_hip_device_count() <= 0


def _winner(L, err, **k):
    p = np.zeros(64).ctypes.data                             # never dereferenced: every call below is refused first
    return L.anofox_hip_select_winner_device(k.get("scores", p), k.get("ld", 64), p, k.get("M", 3), k.get("N", 10), k.get("fallback", -1), p, p, p,
                                             k.get("offsets", p), p, None, C.byref(err))


def _combine(L, err, **k):
    p = np.zeros(64).ctypes.data
    tab = (C.c_void_p * 17)(*([p] * 17))
    return L.anofox_hip_select_combine_device(k.get("blocks", tab), k.get("M", 3), k.get("R", 4), k.get("h", 2), p, k.get("mode", 1),
                                              k.get("winner", p), k.get("weights", p), k.get("ld_w", 4), k.get("group_div", 1), k.get("out", p), p,
                                              None, C.byref(err))


def test_device_entries_refuse_bad_arguments_without_a_device(hiplib):
    L = hiplib.load()
    err = hiplib.AnofoxError()
    for call, kw, text in (
            (_winner, {"M": 0}, "n_methods is 0"),
            (_winner, {"M": 17}, "n_methods 17 exceeds the limit of 16 methods"),
            (_winner, {"fallback": 3}, "fallback 3 is outside [-1, 3)"),
            (_winner, {"fallback": -2}, "fallback -2 is outside [-1, 3)"),
            (_winner, {"ld": 9}, "ld is smaller than n_series"),
            (_combine, {"M": 0}, "n_methods is 0"),
            (_combine, {"M": 17}, "n_methods 17 exceeds the limit of 16 methods"),
            (_combine, {"mode": 4}, "mode must be 0 (pick), 1 (mean), 2 (median) or 3 (inverse_score)"),
            (_combine, {"h": 0}, "horizon must be at least 1"),
            (_combine, {"group_div": 0}, "group_div must be at least 1"),
            (_combine, {"mode": 3, "ld_w": 3}, "ld_w is smaller than the number of groups")):
        assert not call(L, err, **kw)
        assert err.code == hiplib.INVALID_INPUT and text in err.message.decode(), (kw, err.message)
    for call, kw in ((_winner, {"offsets": None}), (_winner, {"scores": None}), (_combine, {"blocks": None}), (_combine, {"out": None}),
                     (_combine, {"mode": 0, "winner": None}), (_combine, {"mode": 3, "weights": None})):
        assert not call(L, err, **kw)
        assert err.code == hiplib.NULL_POINTER and err.message == b"Null pointer argument", kw
    p = np.zeros(64).ctypes.data
    assert not L.anofox_hip_select_gather_device(p, 64, p, 10, 5, p, 8, 3, p, 64, p, None, C.byref(err))
    assert err.code == hiplib.INVALID_INPUT and b"lies outside the n_series entries" in err.message
    assert not L.anofox_hip_select_gather_device(p, 64, p, 10, 5, p, 0, 3, p, 2, p, None, C.byref(err))
    assert err.code == hiplib.INVALID_INPUT and b"ld_m is smaller than n_m" in err.message
    assert not L.anofox_hip_select_gather_device(p, 64, p, 10, 5, None, 0, 3, p, 64, p, None, C.byref(err)) and err.code == hiplib.NULL_POINTER
    assert not L.anofox_hip_select_scatter_device(p, p, p, p, p, p, 0, 3, 0, None, 10, p, p, p, p, p, None, C.byref(err))
    assert err.code == hiplib.INVALID_INPUT and b"horizon must be at least 1" in err.message
    assert not L.anofox_hip_select_scatter_device(None, p, p, p, p, p, 0, 3, 2, None, 10, p, p, p, p, p, None, C.byref(err))
    assert err.code == hiplib.NULL_POINTER
    if _no_device(hiplib):                                   # with valid arguments: the loud failure, never a CPU answer
        for call in (_winner, _combine):
            assert not call(L, err)
            assert err.code == hiplib.INTERNAL_ERROR and b"no CPU fallback" in err.message


def _batch(api, hiplib, methods, metric="rmse", mode="pick", fallback=-1, folds=None, series=None):
    series = [np.arange(30.0), np.arange(30.0) * 2.0] if series is None else series
    folds = api.backtest_fold_bounds(30, 3, 2) if folds is None else folds
    return api.select_batch(series, methods, folds, metric, mode, fallback)


def test_select_batch_refuses_bad_requests_without_a_device(hiplib):
    from anofox_forecast_amd import api
    o = lambda m="Naive", h=3: hiplib.make_options(m, h, auto_detect=False)
    for kw, text in (
            ({"methods": []}, "n_methods is 0"),
            ({"methods": [o()] * 17}, "n_methods 17 exceeds the limit of 16 methods"),
            ({"methods": [o(), o("SES"), o("Naive", 4)]}, "all methods share one horizon, method 2 has 4 and method 0 has 3"),
            ({"methods": [o("Naive", 0)]}, "horizon must be at least 1"),
            ({"methods": [o()], "metric": "mase"}, "unknown criterion 'mase'"),
            ({"methods": [o()], "metric": "no_such_metric"}, "unknown criterion 'no_such_metric'"),
            ({"methods": [o()], "mode": "best"}, "unknown mode 'best'"),
            ({"methods": [o(), o("SES")], "fallback": 2}, "fallback 2 is outside [-1, 2)"),
            ({"methods": [o(), o("SES")], "fallback": -2}, "fallback -2 is outside [-1, 2)")):
        res, err = _batch(api, hiplib, **kw)
        assert not err["ok"] and err["code"] == hiplib.INVALID_INPUT and text in err["message"], (kw, err)
        assert (res["status"] == hiplib.INTERNAL_ERROR).all() and np.isnan(res["yhat"]).all()
    # an option block anofox_hip_batch_create refuses fails the whole call with that error
    res, err = _batch(api, hiplib, methods=[o(), o("NoSuchModel")])
    assert not err["ok"] and err["code"] == hiplib.INVALID_MODEL, err
    L = hiplib.load()
    e = hiplib.AnofoxError()
    tab = hiplib.make_options_table([o()])
    folds = hiplib.make_folds(api.backtest_fold_bounds(30, 3, 2))
    assert not L.anofox_hip_select_batch(None, None, 2, tab, 1, folds, 2, b"rmse", b"pick", -1, *([None] * 11), C.byref(e))
    assert e.code == hiplib.NULL_POINTER
    assert not L.anofox_hip_select_batch(None, None, 0, None, 1, folds, 2, b"rmse", b"pick", -1, *([None] * 11), C.byref(e))
    assert e.code == hiplib.NULL_POINTER
    assert not L.anofox_hip_select_batch(None, None, 0, tab, 1, folds, 2, None, b"pick", -1, *([None] * 11), C.byref(e))
    assert e.code == hiplib.NULL_POINTER
    if _no_device(hiplib):
        res, err = _batch(api, hiplib, methods=[o(), o("SES")])
        assert not err["ok"] and err["code"] == hiplib.INTERNAL_ERROR and "no CPU fallback" in err["message"]


def test_python_entries_refuse_the_limit_and_mixed_horizons(hiplib):
    from anofox_forecast_amd import api, device
    o = lambda m="Naive", h=3: hiplib.make_options(m, h, auto_detect=False)
    folds = api.backtest_fold_bounds(30, 3, 2)
    with pytest.raises(ValueError, match="n_methods 17 exceeds the limit of 16 methods"):
        device.select_block(None, None, [o()] * 17, folds)
    with pytest.raises(ValueError, match="all methods share one horizon, method 1 has 4"):
        device.select_block(None, None, [o(), o("SES", 4)], folds)
    with pytest.raises(ValueError, match="n_methods is 0"):
        device.select_block(None, None, [], folds)
    with pytest.raises(ValueError, match="limit of 16 methods"):
        device.combine_block([None] * 17, "mean")
    with pytest.raises(ValueError, match="unknown selection mode"):
        device.combine_block([None], "best")
    n = 24
    days = np.datetime64("2024-01-01") + np.arange(n)
    table = {"group": ["a"] * n + ["b"] * n, "date": np.concatenate([days, days]), "target": np.arange(2.0 * n)}
    with pytest.raises(api.InvalidInputException, match="n_methods 17 exceeds the limit of 16 methods"):
        api.ts_forecast_best_by(table["group"], table["date"], table["target"], ["Naive"] * 17, 3, "1d", folds=2)
    with pytest.raises(api.InvalidInputException, match="unknown criterion 'mase'"):
        api.ts_compare_models_by(table["group"], table["date"], table["target"], ["Naive", ("SES", None)], 3, "1d", folds=2, metric="mase")
    with pytest.raises(api.InvalidInputException, match="unknown mode"):
        api.ts_forecast_best_by(table["group"], table["date"], table["target"], ["Naive"], 3, "1d", folds=2, mode="best")
    with pytest.raises(api.InvalidInputException, match="none of the methods"):
        api.ts_forecast_best_by(table["group"], table["date"], table["target"], ["Naive"], 3, "1d", folds=2, fallback="SES")
    with pytest.raises(api.InvalidInputException, match="holds NULLs"):
        api.ts_forecast_best_by(table["group"], table["date"], np.where(np.arange(2 * n) == 5, np.nan, table["target"]), ["Naive"], 3, "1d", folds=2)


# --------------------------------------------------------------------------------------------
# the host-only logic under sanitizers, and the independence of the restatement
# --------------------------------------------------------------------------------------------
def test_host_select_plan_under_sanitizers():
    """csrc/host_select_plan.hpp -- the request checks, the criterion and mode names, the sub-batch shapes -- compiled on its own (no
    HIP) and run under ASan + UBSan (tests/c_abi/select_san.cpp)."""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "select_san")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               os.path.join(ROOT, "tests", "c_abi", "select_san.cpp"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("select_san: ok"), (r.stdout, r.stderr[-3000:])


def test_the_product_never_imports_the_restatement():
    pkg = os.path.join(ROOT, "anofox-forecast_amd")
    for base, _dirs, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                assert "select_ref" not in open(os.path.join(base, f), errors="replace").read(), f
    for f in ("__graft_entry__.py", "bench.py", "anofox_forecast_amd.py"):
        assert "select_ref" not in open(os.path.join(ROOT, f)).read(), f
