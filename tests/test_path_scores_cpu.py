"""No GPU: the restatement tests/path_scores_ref.py against the definitional double sum in exact rationals and against its own
properties, its tolerance against the exact scores, the ABI of the path-score entries (symbols, every argument error and its text
through every entry -- all of them come before the device is touched --, the sizing calls), the host-only checks under sanitizers,
and the independence of the restatement."""
import ctypes as C
import decimal
import math
import os
import re
import subprocess
import tempfile
from fractions import Fraction

import numpy as np
import pytest

import metrics_ref as M
import path_scores_cases as K
import path_scores_ref as R
import paths_cases
import paths_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "anofox_fcst_hip.h")
NEW_SYMBOLS = ("anofox_hip_path_scores_device", "anofox_hip_path_scores_sizes", "anofox_hip_path_energy_device",
               "anofox_hip_path_scores_batch")
EPS = 2.0 ** -52


def _finite(n, h, P, seed):
    return K.make_block(n, h, P, seed, special=False)


# --------------------------------------------------------------------------------------------
# the restatement: its two forms, and the identity behind the sorted form
# --------------------------------------------------------------------------------------------
def test_wave_sum_is_the_stated_order():
    t = [1e16, 1.0, -1e16, 3.0] * 40 + [1e-3]                             # 161 terms: the order of the additions shows in the bits
    a = [0.0] * 64
    for i, v in enumerate(t):
        a[i % 64] = a[i % 64] + v
    w = a[0]
    for l in range(1, 64):
        w = w + a[l]
    assert R.wave_sum(t) == w and R.wave_sum(t) != math.fsum(t)
    assert R.wave_sum([]) == 0.0 and R.wave_sum([-0.0]) == 0.0 and math.copysign(1.0, R.wave_sum([-0.0])) == 1.0
    for n in (0, 1, 63, 64, 65, 161):
        assert float(R.wave_sum_axis0(np.array(t[:n]).reshape(n, 1))[0]) == R.wave_sum(t[:n])


@pytest.mark.parametrize("case", [(5, 3, 1, "nine"), (9, 3, 2, "nine"), (9, 2, 65, "sixteen"), (12, 3, 100, "none")], ids=K.case_id)
def test_block_form_equals_the_scalar_statement(case):
    n, h, P, lv = case
    levels = K.LEVEL_SETS[lv]
    block, actual = K.make_block(n, h, P, 1)
    got = R.scores(block, actual, h, P, levels)
    cube = block.reshape(P, h, n)
    for c in range(n):
        want = R.column_scores([[cube[p, k, c] for k in range(h)] for p in range(P)], list(actual[c]), levels)
        assert int(got["status"][c]) == want["status"]
        assert R.same_bits(got["crps"][c], want["crps"]).all(), c
        assert got["below"][c].tolist() == want["below"] and got["equal"][c].tolist() == want["equal"]
        assert R.same_bits(got["column"][:, c], [want["crps_mean"], want["n_steps"]] + want["pinball"]).all(), c
        if levels:
            assert R.same_bits(got["quantiles"][:, c, :], want["quantiles"]).all(), c
    statuses = set(got["status"].tolist())
    assert statuses == ({R.OK, R.NO_ACTUAL, R.NAN} if n > 5 else {R.OK, R.NO_ACTUAL})
    for cb, ce in ((0, n), (1, 4), (3, 4)):
        e = R.energy(block, actual, h, P, cb, ce)
        for k in range(h):
            want = R.energy_one([[cube[p, k, c] for c in range(cb, ce)] for p in range(P)], [actual[c, k] for c in range(cb, ce)])
            assert R.same_bits([e["es"][k]], [want]).all(), (cb, ce, k)


def _exact_double_sum(x, y):
    """mean|x - y| - 1/2 mean|x_i - x_j| in exact rationals."""
    fx, fy, P = [Fraction(float(v)) for v in x], Fraction(float(y)), len(x)
    return sum(abs(v - fy) for v in fx) / P - sum(abs(a - b) for a in fx for b in fx) / (2 * P * P)


def _exact_sorted(x, y):
    """The sorted form in exact rationals: sum|d_i| / P - sum (2i - P + 1) d_i / P^2."""
    s, fy, P = sorted(Fraction(float(v)) for v in x), Fraction(float(y)), len(x)
    return sum(abs(v - fy) for v in s) / P - sum((2 * i - P + 1) * (v - fy) for i, v in enumerate(s)) / (P * P)


def test_sorted_form_is_the_double_sum():
    for P in (1, 2, 3, 7, 40):
        block, actual = _finite(6, 2, P, P)
        cube = block.reshape(P, 2, 6)
        for c in range(6):
            for k in range(2):
                assert _exact_sorted(cube[:, k, c], actual[c, k]) == _exact_double_sum(cube[:, k, c], actual[c, k])


def _plain_crps(x, y):
    x = np.asarray(x, dtype=np.float64)
    return float(np.abs(x - y).mean() - 0.5 * np.abs(x[:, None] - x[None, :]).mean())


def test_crps_tolerance_against_the_exact_rational_crps():
    """The restatement lies within 16 x max(|plain - exact|, eps * max|x_i - y|) of the exact CRPS: 16 x the plain fp64 route's own
    deviation, with a floor at the data's rounding.  Worst ratio measured on these cases: see DESIGN.md."""
    worst = 0.0
    for P in (1, 2, 63, 64, 65, 100, 257, 1000, 2048):
        n = 6 if P <= 257 else 3
        block, actual = _finite(n, 2, P, 40 + P)
        got = R.scores(block, actual, 2, P)["crps"]
        cube = block.reshape(P, 2, n)
        for c in range(n):
            for k in range(2):
                x, y = cube[:, k, c], actual[c, k]
                exact = _exact_sorted(x, y)
                bound = 16 * max(abs(Fraction(_plain_crps(x, y)) - exact), Fraction(EPS * float(np.abs(x - y).max())))
                dev = abs(Fraction(float(got[c, k])) - exact)
                assert dev <= bound, (P, c, k, float(dev), float(bound))
                if bound:
                    worst = max(worst, float(dev / bound) * 16)
    print(f"crps: worst ratio to max(plain deviation, floor) {worst:.3g}")
    assert worst <= 16.0


def _exact_energy(X, y):
    """Sums in exact rationals, roots at 60 decimal digits -> Fraction."""
    decimal.getcontext().prec = 60
    root = lambda f: Fraction((decimal.Decimal(f.numerator) / decimal.Decimal(f.denominator)).sqrt())
    FX = [[Fraction(float(v)) for v in row] for row in X]
    fy = [Fraction(float(v)) for v in y]
    P = len(FX)
    s1 = sum(root(sum((a - b) ** 2 for a, b in zip(row, fy))) for row in FX)
    if P == 1:
        return s1
    s2 = sum(root(sum((a - b) ** 2 for a, b in zip(FX[p], FX[p + 1]))) for p in range(P - 1))
    return s1 / P - s2 / (2 * (P - 1))


def _plain_energy(X, y):
    X = np.asarray(X, dtype=np.float64)
    d1 = np.sqrt(((X - y) ** 2).sum(1))
    if len(X) == 1:
        return float(d1.sum()), float(d1.max())
    d2 = np.sqrt(((X[:-1] - X[1:]) ** 2).sum(1))
    return float(d1.mean() - d2.sum() / (2.0 * (len(X) - 1))), float(max(d1.max(), d2.max()))


def test_energy_tolerance_against_the_exact_energy_score():
    """The same rule: within 16 x max(|plain - exact|, eps * the largest distance) of the score whose sums are exact rationals and
    whose roots carry 60 decimal digits; plain is numpy's sqrt(((X - y) ** 2).sum(1))."""
    worst = 0.0
    for n, h, P, cb, ce in ((20, 2, 1, 0, 20), (70, 2, 2, 0, 70), (70, 1, 65, 3, 68), (130, 1, 100, 64, 130), (9, 2, 300, 4, 5)):
        block, actual = _finite(n, h, P, 70 + P)
        e = R.energy(block, actual, h, P, cb, ce)
        cube = block.reshape(P, h, n)
        for k in range(h):
            X, y = cube[:, k, cb:ce], actual[cb:ce, k]
            exact = _exact_energy(X, y)
            plain, largest = _plain_energy(X, y)
            bound = 16 * max(abs(Fraction(plain) - exact), Fraction(EPS * largest))
            dev = abs(Fraction(float(e["es"][k])) - exact)
            assert dev <= bound, (n, P, cb, ce, k, float(dev), float(bound))
            if bound:
                worst = max(worst, float(dev / bound) * 16)
    print(f"energy: worst ratio to max(plain deviation, floor) {worst:.3g}")
    assert worst <= 16.0


# --------------------------------------------------------------------------------------------
# exact properties
# --------------------------------------------------------------------------------------------
def test_one_path_gives_the_distance():
    block, actual = K.make_block(9, 3, 1, 2)
    s = R.scores(block, actual, 3, 1, K.LEVELS)
    ok = np.isfinite(block).all(axis=0)                                  # (an infinite path: 0 * inf, the arithmetic falls as it falls)
    want = np.abs(block.reshape(3, 9).T - actual)
    assert ok.sum() == 7 and R.same_bits(s["crps"][ok], want[ok]).all()  # NaN where there is no actual, |x - y| to the bit elsewhere
    fb, fa = _finite(9, 3, 1, 3)
    e = R.energy(fb, fa, 3, 1, 2, 7)
    for k in range(3):
        assert float(e["es"][k]) == R.distance(fb.reshape(3, 9)[k, 2:7], fa[2:7, k])
    assert e["es_steps"] == 3 and e["d2"].shape == (0, 3)


def test_doubling_doubles_every_score_and_keeps_the_ranks():
    n, h, P = 12, 3, 100
    block, actual = K.make_block(n, h, P, 4)
    a, b = R.scores(block, actual, h, P, K.LEVELS), R.scores(2.0 * block, 2.0 * actual, h, P, K.LEVELS)
    assert R.same_bits(b["crps"], 2.0 * a["crps"]).all() and R.same_bits(b["quantiles"], 2.0 * a["quantiles"]).all()
    assert R.same_bits(b["column"][0], 2.0 * a["column"][0]).all() and R.same_bits(b["column"][2:], 2.0 * a["column"][2:]).all()
    assert R.same_bits(b["column"][1], a["column"][1]).all()
    assert (a["below"] == b["below"]).all() and (a["equal"] == b["equal"]).all() and (a["status"] == b["status"]).all()
    fb, fa = _finite(n, h, P, 5)
    e1, e2 = R.energy(fb, fa, h, P, 1, 9), R.energy(2.0 * fb, 2.0 * fa, h, P, 1, 9)
    assert R.same_bits(e2["es"], 2.0 * e1["es"]).all() and e2["es_mean"] == 2.0 * e1["es_mean"]


def test_ranks():
    n, h, P = 20, 3, 65
    block, actual = K.make_block(n, h, P, 6)
    s = R.scores(block, actual, h, P)
    live = (s["status"][:, None] != R.NAN) & ~np.isnan(actual)
    assert (s["below"][live] >= 0).all() and (s["equal"][live] >= 0).all() and (s["below"][live] + s["equal"][live] <= P).all()
    assert (s["below"][~live] == -1).all() and (s["equal"][~live] == -1).all()
    assert (s["equal"][live] > 0).any() and (s["below"][live] == 0).any() and (s["below"][live] == P).any()      # ties, below all, above all
    assert s["status"][2] == R.NO_ACTUAL and np.isnan(s["column"][0, 2]) and s["column"][1, 2] == 0.0
    assert s["status"][5] == R.NAN and np.isnan(s["column"][:, 5]).all() and np.isnan(s["crps"][5]).all()      # NaN takes precedence
    assert s["quantiles"].shape == (0, n, h)


def test_pinball_is_quantile_loss_of_the_quantile_entrys_quantiles():
    assert K.LEVELS == paths_cases.LEVELS and K.LEVELS_16 == paths_cases.LEVELS_16
    n, h, P = 12, 5, 100
    block, actual = K.make_block(n, h, P, 7)
    s = R.scores(block, actual, h, P, K.LEVELS)
    q, qs = paths_ref.quantiles(block, h, P, K.LEVELS)
    assert R.same_bits(s["quantiles"], q).all() and ((s["status"] == R.NAN) == (qs == paths_ref.NAN)).all()
    for c in range(n):
        keep = [k for k in range(h) if not math.isnan(actual[c, k])]
        if s["status"][c] != R.OK:
            continue
        for l, tau in enumerate(K.LEVELS):
            want = M.quantile_loss([float(actual[c, k]) for k in keep], [float(q[l, c, k]) for k in keep], tau)
            assert R.same_bits([s["column"][2 + l, c]], [want]).all(), (c, l)
        assert s["column"][1, c] == float(len(keep))


# --------------------------------------------------------------------------------------------
# the ABI
# --------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported(hiplib):
    L = hiplib.load()
    text = open(HEADER).read()
    for name in NEW_SYMBOLS:
        assert name in hiplib.EXPORTED_SYMBOLS and hasattr(L, name), name
        assert re.search(r"\bbool\s+" + name + r"\s*\(", text), name
    assert "Block 10" in text
    assert (hiplib.PATH_SCORES_OK, hiplib.PATH_SCORES_NO_ACTUAL, hiplib.PATH_SCORES_NAN) == (R.OK, R.NO_ACTUAL, R.NAN) == (0, 1, 2)
    for name, value in (("ANOFOX_PATH_SCORES_OK", 0), ("ANOFOX_PATH_SCORES_NO_ACTUAL", 1), ("ANOFOX_PATH_SCORES_NAN", 2)):
        assert re.search(name + r"\s*=\s*%d" % value, text), name


def _no_device(hiplib):
    return hiplib.load().anofox_hip_device_count() <= 0


_P = np.zeros(64)                                            # never dereferenced: every call below is refused first
_LEVELS = np.array([0.1, 0.5, 0.9])


def _scores(hiplib, L, err, **k):
    p = _P.ctypes.data
    lv = np.ascontiguousarray(k.get("levels", _LEVELS), dtype=np.float64)
    return L.anofox_hip_path_scores_device(k.get("paths", p), k.get("ld", 64), k.get("n", 10), k.get("h", 1), k.get("P", 4), k.get("actual", p), 1, 64,
                                           lv.ctypes.data if k.get("have_levels", True) else None, k.get("n_levels", len(lv)), p, p, p, p,
                                           p if k.get("column", True) else None, k.get("ld_out", 64), k.get("status", p), None, C.byref(err))


def _energy(hiplib, L, err, **k):
    p = _P.ctypes.data
    return L.anofox_hip_path_energy_device(k.get("paths", p), k.get("ld", 64), k.get("cb", 0), k.get("ce", 10), k.get("h", 1), k.get("P", 4),
                                           k.get("actual", p), 1, 64, k.get("workspace", p), k.get("es", p), k.get("summary", p), None, C.byref(err))


def _sizes(hiplib, L, err, **k):
    words = C.c_size_t(77)
    ok = L.anofox_hip_path_scores_sizes(k.get("h", 1), k.get("P", 4), C.byref(words) if k.get("out", True) else None, C.byref(err))
    return ok if not k.get("value") else (ok, words.value)


def _batch(hiplib, L, err, **k):
    n, h = k.get("n", 2), k.get("h", 2)
    pts = np.zeros((max(n, 1), min(max(h, 1), 4)))          # (read only by a call that passes every check: h = 2)
    act = np.zeros((max(n, 1), min(max(h, 1), 4)))
    pools = [np.arange(3.0)] * n
    ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in pools])
    lens = (C.c_size_t * max(n, 1))(*k.get("lengths", [3] * n))
    lv = np.ascontiguousarray(k.get("levels", _LEVELS), dtype=np.float64)
    o = hiplib.make_paths_options(k.get("mode", 0), k.get("joint", 0), 1, k.get("route", 0))
    co = k.get("column_of")
    co = None if co is None else np.ascontiguousarray(co, dtype=np.int32)
    n_out, ld = C.c_size_t(), C.c_size_t()
    st = np.zeros(128, dtype=np.int32)
    ok = L.anofox_hip_path_scores_batch(pts.ctypes.data if k.get("points", True) else None, ptrs, lens, n, h, k.get("P", 4),
                                        C.byref(o) if k.get("options", True) else None, k.get("struct_size", C.sizeof(o)), lv.ctypes.data,
                                        k.get("n_levels", len(lv)), None if co is None else co.ctypes.data, 0 if co is None else co.shape[0],
                                        act.ctypes.data if k.get("actuals", True) else None, k.get("ld", 64), None, None, None, None, None,
                                        None if k.get("sizing", False) else st.ctypes.data, None, None, None, C.byref(n_out), C.byref(ld),
                                        C.byref(err))
    return ok, n_out.value, ld.value


SHARED_ERRORS = (                                             # the texts of the quantile entry, refused alike by every entry
    ({"P": 0}, "n_paths is 0"),
    ({"P": 2049}, "n_paths 2049 exceeds the limit of 2048 paths per call"),
    ({"h": 0}, "horizon must be at least 1"),
    ({"P": 2048, "h": (1 << 19) + 1}, "exceeds the limit of 2^30 rows"),
)
LEVEL_ERRORS = (
    ({"levels": [0.5] * 17}, "n_levels 17 exceeds the limit of 16 levels per call"),
    ({"levels": [0.1, 1.25]}, "level 1 is 1.25, outside [0, 1]"),
    ({"levels": [-0.5, 0.5]}, "level 0 is -0.5, outside [0, 1]"),
    ({"levels": [0.1, 0.2, float("nan")]}, "level 2 is"),
)
OPTION_ERRORS = (
    ({"struct_size": 16}, "struct_size is not sizeof(AnofoxHipPathsOptions)"),
    ({"mode": 2}, "mode 2 is unknown: 0 (cumulative) or 1 (independent)"),
    ({"joint": 2}, "joint 2 is neither 0 nor 1"),
)


def test_device_entries_refuse_bad_arguments_without_a_device(hiplib):
    L = hiplib.load()
    err = hiplib.AnofoxError()
    for kw, text in SHARED_ERRORS + LEVEL_ERRORS + (({"ld": 9}, "ld is smaller than n_cols"), ({"ld_out": 9}, "ld_out is smaller than n_cols")):
        assert not _scores(hiplib, L, err, **kw)
        assert err.code == hiplib.INVALID_INPUT and text in err.message.decode(), (kw, err.message)
    for kw, text in SHARED_ERRORS + (({"cb": 5, "ce": 5}, "the column range [5, 5) is empty or reversed"),
                                     ({"cb": 7, "ce": 3}, "the column range [7, 3) is empty or reversed"),
                                     ({"cb": 3, "ce": 65}, "the column range [3, 65) ends beyond ld = 64")):
        assert not _energy(hiplib, L, err, **kw)
        assert err.code == hiplib.INVALID_INPUT and text in err.message.decode(), (kw, err.message)
    for kw, text in SHARED_ERRORS:
        assert not _sizes(hiplib, L, err, **kw)
        assert err.code == hiplib.INVALID_INPUT and text in err.message.decode(), (kw, err.message)
    for call, kw in ((_scores, {"paths": None}), (_scores, {"actual": None}), (_scores, {"status": None}), (_scores, {"have_levels": False}),
                     (_energy, {"paths": None}), (_energy, {"actual": None}), (_energy, {"workspace": None}), (_energy, {"es": None}),
                     (_energy, {"summary": None}), (_sizes, {"out": False})):
        assert not call(hiplib, L, err, **kw)
        assert err.code == hiplib.NULL_POINTER and err.message == b"Null pointer argument", kw
    # the sizing call needs no device
    assert _sizes(hiplib, L, err, h=28, P=1000, value=True) == (True, 2 * 28 * 1000)
    assert _sizes(hiplib, L, err, h=1, P=1, value=True) == (True, 2)
    if _no_device(hiplib):                                   # with valid arguments: the loud failure, never a CPU answer
        for call, kw in ((_scores, {}), (_scores, {"n_levels": 0, "have_levels": False}), (_scores, {"column": False, "ld_out": 0}), (_energy, {})):
            assert not call(hiplib, L, err, **kw)
            assert err.code == hiplib.INTERNAL_ERROR and b"no CPU fallback" in err.message, kw


def test_batch_entry_refuses_bad_requests_and_sizes_without_a_device(hiplib):
    L = hiplib.load()
    err = hiplib.AnofoxError()
    for kw, text in SHARED_ERRORS + OPTION_ERRORS + LEVEL_ERRORS + (
            ({"lengths": [3, (1 << 20) + 1]}, "pool_rows 1048577 exceeds the limit of 2^20"),
            ({"column_of": [[0, -2]]}, "a column_of entry is below -1"),
            ({"ld": 128}, "ld is not what the sizing call returns")):
        ok, _, _ = _batch(hiplib, L, err, **kw)
        assert not ok and err.code == hiplib.INVALID_INPUT and text in err.message.decode(), (kw, err.message)
    for kw in ({"options": False}, {"points": False}, {"actuals": False}):
        ok, _, _ = _batch(hiplib, L, err, **kw)
        assert not ok and err.code == hiplib.NULL_POINTER, kw
    assert _batch(hiplib, L, err, n=2, sizing=True) == (True, 2, 64)
    assert _batch(hiplib, L, err, n=2, sizing=True, n_levels=0) == (True, 2, 64)
    assert _batch(hiplib, L, err, n=2, sizing=True, column_of=[[0, 0], [1, 2]]) == (True, 3, 64)
    co = np.stack([np.zeros(70, dtype=np.int32), 1 + np.arange(70, dtype=np.int32)])
    assert _batch(hiplib, L, err, n=70, sizing=True, column_of=co) == (True, 71, 128)
    if _no_device(hiplib):
        ok, _, _ = _batch(hiplib, L, err)
        assert not ok and err.code == hiplib.INTERNAL_ERROR and b"no CPU fallback" in err.message


def test_python_entry_refuses_the_limits(hiplib):
    from anofox_forecast_amd import api
    pts, pools, act = np.zeros((2, 3)), [np.arange(4.0), np.arange(4.0)], np.zeros((2, 3))
    for kw, text in (({"n_paths": 0}, "n_paths is 0"), ({"n_paths": 2049}, "exceeds the limit of 2048 paths"),
                     ({"levels": [0.5] * 17}, "exceeds the limit of 16 levels"), ({"levels": [2.0]}, "outside [0, 1]")):
        args = {"levels": [0.1, 0.9], "n_paths": 8}
        args.update(kw)
        res, err = api.path_scores_batch(pts, pools, act, **args)
        assert not err["ok"] and err["code"] == hiplib.INVALID_INPUT and text in err["message"], (kw, err)
    if _no_device(hiplib):
        res, err = api.path_scores_batch(pts, pools, act, [0.1, 0.9], n_paths=8)
        assert not err["ok"] and err["code"] == hiplib.INTERNAL_ERROR and "no CPU fallback" in err["message"]
        assert np.isnan(res["crps"]).all() and res["crps"].shape == (2, 3) and res["ranges"].tolist() == [[0, 2]]


# --------------------------------------------------------------------------------------------
# the host-only logic under sanitizers, and the independence of the restatement
# --------------------------------------------------------------------------------------------
def test_host_path_scores_plan_under_sanitizers():
    """csrc/host_path_scores_plan.hpp -- the level and range checks, the workspace size and the column ranges of a plan's groupings --
    compiled on its own (no HIP) as a stand-alone program and run under ASan + UBSan (tests/c_abi/path_scores_san.cpp)."""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "path_scores_san")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               os.path.join(ROOT, "tests", "c_abi", "path_scores_san.cpp"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("path_scores_san: ok"), (r.stdout, r.stderr[-3000:])


def test_the_restatement_is_independent():
    pkg = os.path.join(ROOT, "anofox-forecast_amd")
    for base, _dirs, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                assert "path_scores_ref" not in open(os.path.join(base, f), errors="replace").read(), f
    for f in ("__graft_entry__.py", "bench.py", "anofox_forecast_amd.py"):
        assert "path_scores_ref" not in open(os.path.join(ROOT, f)).read(), f
    for f in ("path_scores_ref.py", "path_scores_cases.py"):
        text = open(os.path.join(ROOT, "tests", f)).read()
        assert "anofox_forecast_amd" not in text and "oracle" not in text, f
        assert not re.search(r"^\s*(import|from)\s+(paths_ref|metrics_ref|hierarchy_ref)", text, re.M), f
