"""CPU: the restatement of the reference's ssa_period and stl_period (tests/period_search_ref.py): its two forms equal with ==, the
STL strengths recomputed from mstl_ref.mstl_decompose, candidate lists and the window rule against hand-written values, the known
shapes; the struct layouts and symbols against the header; the host-only logic of the operator mirrors with the GPU batch calls
replaced by the restatement; the host header under ASan + UBSan as a stand-alone program; and the boundary that must not move: the
method dispatch by name still raises for 'ssa' and 'stl'."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import mstl_ref as M
import period_search_cases as PC
import period_search_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(a, b):
    """== on every figure, NaN equal to NaN."""
    if isinstance(a, dict):
        return set(a) == set(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and a != a:
        return b != b
    return a == b


# --------------------------------------------------------------------------------------------
# the restatement
# --------------------------------------------------------------------------------------------
SSA_CASES = [("seasonal", 16, None, None), ("seasonal", 48, None, 4), ("demand", 61, 9, 3), ("noise", 40, None, 10), ("sine", 24, None, None),
             ("zeros", 20, None, None), ("constant", 30, None, None), ("nan", 36, None, 2), ("inf", 36, None, 2), ("seasonal", 33, 1, 5)]


@pytest.mark.parametrize("fam,n,window,comps", SSA_CASES, ids=lambda x: str(x))
def test_ssa_two_forms_agree(fam, n, window, comps):
    v = PC.family(fam, n, 6)
    assert same(R.ssa_period_plain(v, window, comps), R.ssa_period(v, window, comps))


@pytest.mark.parametrize("fam,n,args", [("seasonal", 16, ()), ("seasonal", 48, ()), ("demand", 96, (2, 12, 5)), ("sine", 60, (3, 30, 64)),
                                        ("constant", 30, ()), ("noise", 45, (0, 0, 1))], ids=lambda x: str(x))
def test_stl_two_forms_agree(fam, n, args):
    v = PC.family(fam, n, 7)
    assert same(R.stl_period_plain(v, *args), R.stl_period(v, *args))


def test_stl_strengths_from_the_decomposition():
    v = PC.family("seasonal", 96, 12)
    r = R.stl_period(v)
    assert len(r["candidates"]) == 20 and r["candidates"][:7] == [4, 5, 7, 8, 10, 11, 12] and r["candidates"][-1] == 31
    for p, got in zip(r["candidates"], r["candidate_strengths"]):
        d = M.mstl_decompose(v, [p], M.TREND)
        s, rem = d["seasonal"][0], d["remainder"]
        det = s + rem
        var_d = R._seqsum(((det - R._seqsum(det.tolist()) / 96.0) ** 2).tolist()) / 96.0
        var_r = R._seqsum(((rem - R._seqsum(rem.tolist()) / 96.0) ** 2).tolist()) / 96.0
        assert got == max(1.0 - var_r / var_d, 0.0)
    best = max(range(len(r["candidates"])), key=lambda i: (r["candidate_strengths"][i], -i))      # the first of the largest: strict >
    assert r["index"] == best and r["period"] == float(r["candidates"][best]) and r["seasonal_strength"] == r["candidate_strengths"][best]
    assert 0.0 < r["trend_strength"] <= 1.0


def test_candidate_lists():
    assert R.stl_candidates(16) == [4, 5]
    assert R.stl_candidates(100, 2, 12, 5) == [2, 4, 6, 8, 10]
    assert R.stl_n_candidates(1) == 5 and R.stl_candidates(100, 2, 12, 1) == [2, 4, 6, 8, 10]
    assert R.stl_candidates(48) == list(range(4, 17))
    assert R.stl_candidates(40, None, 10 ** 9)[-1] == 20           # n = 2 p exactly
    assert R.stl_candidates(200, 4, 100, 20) == [4, 9, 14, 18, 23, 28, 33, 38, 42, 47, 52, 57, 62, 66, 71, 76, 81, 86, 90, 95]
    for lo, hi in ((10, 10), (12, 9), (None, 4), (2 ** 40, None)):
        with pytest.raises(R.InvalidInput, match="Invalid input: min_period must be less than max_period"):
            R.stl_candidates(40, lo, hi)
    # "No valid candidate periods found" cannot be reached: max_p <= n / 2 and the first candidate is min_p < max_p itself, so it always
    # passes the filter n >= 2 p.  The text is kept for status 4 of the device entry all the same.
    for n in range(16, 400):
        for lo, hi in ((None, None), (2, 3), (7, None), (None, n)):
            try:
                assert R.stl_candidates(n, lo, hi)[0] == max(lo or 4, 2)
            except R.InvalidInput as e:
                assert "min_period" in str(e)
    assert str(R.InvalidInput("No valid candidate periods found")) == "Invalid input: No valid candidate periods found"


def test_window_rule_and_errors():
    assert R.ssa_window(16) == 5 and R.ssa_window(16, 1) == 4 and R.ssa_window(16, 100) == 8 and R.ssa_window(1913) == 637
    assert R.ssa_period(PC.family("seasonal", 16))["window"] == 5 and R.ssa_period(PC.family("seasonal", 40), 30)["window"] == 20
    for f in (R.ssa_period, R.ssa_period_plain, R.stl_period, R.stl_period_plain):
        with pytest.raises(R.InsufficientData) as e:
            f(np.arange(15.0))
        assert str(e.value) == "Insufficient data: need at least 16 observations, got 15"
    assert R.ssa_matrix_in_lds(260, 86) and not R.ssa_matrix_in_lds(261, 87) and R.stl_rows_in_lds(721) and not R.stl_rows_in_lds(722)


def test_known_shapes():
    r = R.ssa_period(np.zeros(20))
    assert r["eigenvalues"] == [] and math.isnan(r["period"]) and r["variance_explained"] == 0.0
    r = R.ssa_period(np.full(30, 5.0))
    assert math.isnan(r["period"]) and r["n_eigenvalues"] >= 1 and abs(r["eigenvalues"][0] - 250.0) < 1e-9     # rank one: l * 25
    t = np.arange(24)
    r = R.ssa_period(np.sin(2.0 * math.pi * t / 4.0))
    # (the zero-crossing estimate 2 l / crossings of a window of 8 is coarse: 3 crossings give 16 / 3, 4 would give 4)
    assert r["window"] == 8 and r["period"] in (4.0, 16.0 / 3.0) and abs(r["variance_explained"] - 1.0) < 1e-9 and r["n_eigenvalues"] >= 2
    r = R.ssa_period(PC.family("seasonal", 96, 12))
    assert 10.0 < r["period"] < 14.0
    r = R.stl_period(np.full(30, 5.0))
    assert math.isnan(r["period"]) and r["index"] == -1 and r["candidate_strengths"] == [0.0] * len(r["candidates"])
    r = R.stl_period(PC.family("seasonal", 96, 12))
    assert r["period"] in (12.0, 24.0) and r["seasonal_strength"] > 0.5


def test_the_contract_is_not_vacuous():
    """Another summation order of the covariance (np.dot) changes bits of the eigenvalues: == does distinguish the orders."""
    changed = 0
    for seed in range(6):
        v = PC.family("seasonal", 60, 7, seed=seed)
        l = R.ssa_window(60)
        X = np.array([v[i:i + 60 - l + 1] for i in range(l)])
        C = X @ X.T / float(60 - l + 1)
        want = R.ssa_period(v, None, 1)["eigenvalues"][0]
        vec = 1.0 / (np.arange(l) + 1.0)
        vec /= np.linalg.norm(vec)
        for _ in range(100):
            vec = C @ vec
            vec /= np.linalg.norm(vec)
        changed += float(vec @ C @ vec) != want
    assert changed >= 1


# --------------------------------------------------------------------------------------------
# the Python layer against a restatement-backed stand-in
# --------------------------------------------------------------------------------------------
def _arg(v):
    return None if v is None or v == 0 else int(v) & 0xFFFFFFFFFFFFFFFF        # static_cast<size_t> of the BIGINT, as api._size_t


def ref_ssa_period_batch(series, window_size=None, n_components=None):
    """api.ssa_period_batch by the restatement: the same dicts."""
    out = []
    for s in series:
        try:
            n = len(s)
            if n >= 16 and R.ssa_window(n, _arg(window_size)) > R.SSA_MAX_WINDOW:
                raise R.InvalidInput("window")
            r = R.ssa_period(s, _arg(window_size), _arg(n_components))
            out.append({"ok": True, "code": 0, "message": "", "method": "ssa", "period": r["period"], "variance_explained": r["variance_explained"],
                        "n_eigenvalues": r["n_eigenvalues"], "eigenvalues": r["eigenvalues"], "detected_periods": r["detected_periods"]})
        except (R.InsufficientData, R.InvalidInput) as e:
            out.append({"ok": False, "code": 3, "message": str(e), "method": "ssa", "period": math.nan, "variance_explained": math.nan,
                        "n_eigenvalues": 0, "eigenvalues": [], "detected_periods": []})
    return out


def ref_stl_period_batch(series, min_period=None, max_period=None, n_candidates=None):
    """api.stl_period_batch by the restatement: the same dicts."""
    out = []
    for s in series:
        try:
            r = R.stl_period(s, _arg(min_period), _arg(max_period), _arg(n_candidates))
            out.append({"ok": True, "code": 0, "message": "", "method": "stl", "period": r["period"], "seasonal_strength": r["seasonal_strength"],
                        "trend_strength": r["trend_strength"], "index": r["index"], "candidates": r["candidates"],
                        "candidate_strengths": r["candidate_strengths"]})
        except (R.InsufficientData, R.InvalidInput) as e:
            out.append({"ok": False, "code": 3, "message": str(e), "method": "stl", "period": math.nan, "seasonal_strength": math.nan,
                        "trend_strength": math.nan, "index": -1, "candidates": [], "candidate_strengths": []})
    return out


@pytest.fixture()
def api(monkeypatch):
    from anofox_forecast_amd import api as A
    monkeypatch.setattr(A, "ssa_period_batch", ref_ssa_period_batch)
    monkeypatch.setattr(A, "stl_period_batch", ref_stl_period_batch)
    return A


def test_scalar_mirrors_null_rules(api):
    v = PC.family("seasonal", 48, 6)
    r = R.ssa_period(v)
    assert same(api.ts_ssa_period(list(v)), {"period": r["period"], "variance_explained": r["variance_explained"],
                                            "n_eigenvalues": r["n_eigenvalues"], "method": "ssa"})
    q = R.stl_period(v, 2, 12, 5)
    assert same(api.ts_stl_period(list(v), 2, 12, 5), {"period": q["period"], "seasonal_strength": q["seasonal_strength"],
                                                      "trend_strength": q["trend_strength"], "method": "stl"})
    assert list(api.ts_ssa_period(list(v))) == ["period", "variance_explained", "n_eigenvalues", "method"]
    assert list(api.ts_stl_period(list(v))) == ["period", "seasonal_strength", "trend_strength", "method"]
    # a NULL list, fewer than 16 non-NULL values, a failed call
    assert api.ts_ssa_period(None) is None and api.ts_stl_period(None) is None
    assert api.ts_ssa_period([1.0] * 15) is None and api.ts_stl_period([1.0, None] * 15) is None
    assert api.ts_stl_period(list(v), 10, 10) is None and api.ts_stl_period(list(v), 30, 5) is None
    # NULL elements are dropped
    with_nulls = [None if i % 7 == 3 else float(x) for i, x in enumerate(np.resize(v, 60))]
    dense = [x for x in with_nulls if x is not None]
    assert same(api.ts_ssa_period(with_nulls, 6, 3), api.ts_ssa_period(dense, 6, 3))
    assert same(api.ts_stl_period(with_nulls), api.ts_stl_period(dense))
    # zero and None are the defaults; a negative BIGINT wraps to a huge size_t
    assert same(api.ts_ssa_period(list(v), 0, 0), api.ts_ssa_period(list(v))) and same(api.ts_stl_period(list(v), 0, 0, 0), api.ts_stl_period(list(v)))
    assert api._size_t(-1) == 2 ** 64 - 1
    assert same(api.ts_ssa_period(list(v), -1), api.ts_ssa_period(list(v), 24))       # any window above n / 2 is n / 2
    assert api.ts_stl_period(list(v), -1) is None                                    # min_period beyond max_period


def test_by_mirrors_pack_one_batch(api, monkeypatch):
    calls = []

    def counting_ssa(series, *a):
        calls.append(("ssa", len(series), a))
        return ref_ssa_period_batch(series, *a)

    def counting_stl(series, *a):
        calls.append(("stl", len(series), a))
        return ref_stl_period_batch(series, *a)
    monkeypatch.setattr(api, "ssa_period_batch", counting_ssa)
    monkeypatch.setattr(api, "stl_period_batch", counting_stl)
    n = 40
    d = np.concatenate([np.arange(n)[::-1], np.arange(n), np.arange(5)]).astype("datetime64[D]")       # group a arrives in reverse date order
    va, vb = PC.family("seasonal", n, 6), PC.family("demand", n, 7, seed=3)
    g = ["a"] * n + ["b"] * n + ["c"] * 5
    val = np.concatenate([va[::-1], vb, np.ones(5)])
    out = api.ts_ssa_period_by(g, d, val, 8, 2, group_name="key")
    assert calls == [("ssa", 2, (8, 2))]                           # group c has 5 rows: a NULL row, never sent
    assert out["key"] == ["a", "b", "c"] and list(out) == ["key", "period", "variance_explained", "n_eigenvalues", "method"]
    ra, rb = R.ssa_period(va, 8, 2), R.ssa_period(vb, 8, 2)
    assert same(out["period"][:2], [ra["period"], rb["period"]]) and out["variance_explained"][:2] == [ra["variance_explained"], rb["variance_explained"]]
    assert out["period"][2] is None and out["method"] == ["ssa", "ssa", None]
    calls.clear()
    out = api.ts_stl_period_by(g, d, val, 2, 10)
    assert calls == [("stl", 2, (2, 10, None))] and out["id"] == ["a", "b", "c"]
    assert list(out) == ["id", "period", "seasonal_strength", "trend_strength", "method"]
    qa = R.stl_period(va, 2, 10)
    assert out["period"][0] == qa["period"] and out["seasonal_strength"][0] == qa["seasonal_strength"] and out["trend_strength"][2] is None


# --------------------------------------------------------------------------------------------
# the C ABI's layout, the argument errors that need no device, the host header under sanitizers
# --------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("anofox_ts_ssa_period", "anofox_ts_stl_period", "anofox_hip_ssa_period_batch", "anofox_hip_stl_period_batch",
               "anofox_hip_ssa_period_device", "anofox_hip_stl_period_device")


def test_struct_layout_and_symbols(hiplib):
    L = hiplib.load()
    header = open(os.path.join(ROOT, "include", "anofox_fcst_hip.h")).read()
    ctype = {"double": C.c_double, "size_t": C.c_size_t}
    for T in (hiplib.SsaPeriodResultFFI, hiplib.StlPeriodResultFFI):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (T.__name__, T.__name__), header, re.S).group(1)
        fields = []
        for line in body.split("\n"):
            m = re.match(r"\s*(double|size_t|char)\s*(\w+)(\[32\])?;", line)
            if m:
                fields.append((m.group(2), C.c_char * 32 if m.group(1) == "char" else ctype[m.group(1)]))
        assert [(n, t) for n, t in T._fields_] == fields, T.__name__
        assert C.sizeof(T) == 56 and T.method.offset == 24
    for s in NEW_SYMBOLS:
        assert s in hiplib.EXPORTED_SYMBOLS and hasattr(L, s) and re.search(r"\b%s\(" % s, header)
    assert hiplib.SSA_FIGURES == ("period", "variance_explained", "n_eigenvalues") and hiplib.STL_FIGURES == ("period", "seasonal_strength", "trend_strength")
    assert (hiplib.ssa_components(None), hiplib.ssa_components(0), hiplib.ssa_components(4)) == (10, 10, 4)
    assert (hiplib.stl_candidate_count(None), hiplib.stl_candidate_count(1), hiplib.stl_candidate_count(64)) == (20, 5, 64)


def test_argument_errors_come_before_the_device(hiplib):
    from anofox_forecast_amd import api as A
    L = hiplib.load()
    err = hiplib.AnofoxError()
    v = np.arange(20.0)
    res_a, res_b = hiplib.SsaPeriodResultFFI(), hiplib.StlPeriodResultFFI()
    assert not L.anofox_ts_ssa_period(None, 20, 0, 0, C.byref(res_a), C.byref(err)) and err.code == hiplib.NULL_POINTER
    assert err.message == b"Null pointer argument"
    assert not L.anofox_ts_stl_period(v.ctypes.data, 20, 0, 0, 0, None, C.byref(err)) and err.message == b"Null pointer argument"
    assert not L.anofox_ts_ssa_period(v.ctypes.data, 20, 0, 33, C.byref(res_a), C.byref(err)) and err.code == hiplib.INVALID_INPUT
    assert b"n_components 33 exceeds the limit of 32" in err.message
    assert not L.anofox_ts_stl_period(v.ctypes.data, 20, 0, 0, 65, C.byref(res_b), C.byref(err)) and err.code == hiplib.INVALID_INPUT
    assert b"n_candidates 65 exceeds the limit of 64" in err.message
    with pytest.raises(A.InvalidInputException, match="exceeds the limit of 65536 rows per series"):
        A.ssa_period_batch([np.zeros(65537)])
    with pytest.raises(A.InvalidInputException, match="exceeds the limit of 65536 rows per series"):
        A.stl_period_batch([np.zeros(20), np.zeros(65537)])
    with pytest.raises(A.InvalidInputException, match="n_candidates 65"):
        A.stl_period_batch([np.zeros(20)], n_candidates=65)
    for call in ("anofox_hip_ssa_period_device", "anofox_hip_stl_period_device"):
        args = [None if t is C.c_void_p else 0 for t in getattr(L, call).argtypes[:-1]] + [C.byref(err)]
        assert not getattr(L, call)(*args) and err.code == hiplib.NULL_POINTER
    assert A.ssa_period_batch([]) == [] and A.stl_period_batch([]) == []


def test_host_period_search_under_sanitizers():
    """csrc/host_period_search.hpp -- the window rule, the candidate list, where the data lives, every argument check and error
    text -- compiled on its own (no HIP) and run under ASan + UBSan (tests/c_abi/period_search_san.cpp), as a stand-alone program."""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "period_search_san")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               os.path.join(ROOT, "tests", "c_abi", "period_search_san.cpp"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("period_search_san: ok"), (r.stdout, r.stderr[-3000:])


# --------------------------------------------------------------------------------------------
# the boundary: the dispatch by method name keeps its error
# --------------------------------------------------------------------------------------------
def test_method_dispatch_still_raises():
    from anofox_forecast_amd import api as A
    v = list(PC.family("seasonal", 48, 6))
    for name, aliases in (("ssa", ("ssa", "singular_spectrum", "SSA")), ("stl", ("stl", "stl_period", "seasonal_trend"))):
        for a in aliases:
            for call in (lambda: A.period_method(a), lambda: A._ts_detect_periods(v, a), lambda: A.periods_batch([v], a),
                         lambda: A.ts_detect_periods_by(["g"] * 48, np.arange(48).astype("datetime64[D]"), v, {"method": a})):
                with pytest.raises(A.InvalidInputException, match=f"'{name}' is not implemented by the HIP backend"):
                    call()
    src = open(os.path.join(ROOT, "anofox-forecast_amd", "csrc", "host_api.hip")).read()
    assert '{"ssa", "ssa", -1}' in src and '{"stl", "stl", -1}' in src and '{"singular_spectrum", "ssa", -1}' in src
