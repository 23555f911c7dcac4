"""GPU: the SSA and STL period entries (anofox_ts_ssa_period, anofox_ts_stl_period, anofox_hip_ssa_period_batch / _device,
anofox_hip_stl_period_batch / _device), device.ssa_period_block / stl_period_block, api.ssa_period_batch / stl_period_batch and the
operator mirrors against the restatement tests/period_search_ref.py.  The contract is equality of bits: every
figure, optional vector, index and status is compared with ==, NaN exactly where the restatement has NaN, through every entry, on
every route and twice in a row.  Only the sign of a zero and NaN payloads are exempt (== does not see them).

Boundaries of the kernels, with a shape on each side: one wavefront per series up to a window of 64; the matrix in LDS while
l * l + 3 l + n <= 7,936 (default windows: l = 86 at n = 260, l = 87 at n = 261 goes to the workspace); 256 lanes per workgroup
(windows 255 / 256 / 257); the series in LDS up to 2,048 rows; the STL rows in LDS up to 721 rows."""
import ctypes as C
import math

import numpy as np
import pytest

import period_search_cases as PC
import period_search_ref as R

pytestmark = pytest.mark.gpu

COMPUTATION_ERROR, INVALID_INPUT = 3, 2
_CACHE = {}


@pytest.fixture(scope="module")
def api(hiplib):
    import torch
    assert torch.cuda.is_available()
    hiplib.load()
    from anofox_forecast_amd import api as A
    return A


def eq(a, b):
    """== with NaN equal to NaN, over floats, ints and lists."""
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(eq(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and a != a:
        return b != b
    return a == b


def ssa_ref(key, series, window=None, comps=None):
    """The restatement of one series, computed once per module: the batch-entry dict."""
    k = ("ssa", key, window, comps)
    if k not in _CACHE:
        try:
            if len(series) >= 16 and R.ssa_window(len(series), window) > R.SSA_MAX_WINDOW:
                raise R.InvalidInput("window")
            r = R.ssa_period(series, window, comps)
            _CACHE[k] = {"ok": True, "period": r["period"], "variance_explained": r["variance_explained"], "n_eigenvalues": r["n_eigenvalues"],
                         "eigenvalues": r["eigenvalues"], "detected_periods": r["detected_periods"], "message": ""}
        except R.InsufficientData as e:
            _CACHE[k] = {"ok": False, "message": str(e)}
        except R.InvalidInput:
            _CACHE[k] = {"ok": False, "message": "exceeds the limit of 2048"}
    return _CACHE[k]


def stl_ref(key, series, lo=None, hi=None, cands=None):
    k = ("stl", key, lo, hi, cands)
    if k not in _CACHE:
        try:
            r = R.stl_period(series, lo, hi, cands)
            _CACHE[k] = {"ok": True, "message": "", **{f: r[f] for f in ("period", "seasonal_strength", "trend_strength", "index", "candidates",
                                                                             "candidate_strengths")}}
        except (R.InsufficientData, R.InvalidInput) as e:
            _CACHE[k] = {"ok": False, "message": str(e)}
    return _CACHE[k]


def check_ssa(got, want, where):
    assert got["ok"] == want["ok"], (where, got, want)
    if not want["ok"]:
        assert got["code"] == COMPUTATION_ERROR and want["message"] in got["message"], (where, got["message"])
        assert math.isnan(got["period"]) and math.isnan(got["variance_explained"]) and got["eigenvalues"] == [] and got["detected_periods"] == []
        return
    for f in ("period", "variance_explained", "n_eigenvalues", "eigenvalues", "detected_periods"):
        assert eq(got[f], want[f]), (where, f, got[f], want[f])


def check_stl(got, want, where):
    assert got["ok"] == want["ok"], (where, got, want)
    if not want["ok"]:
        assert got["code"] == COMPUTATION_ERROR and got["message"] == want["message"], (where, got["message"])
        assert math.isnan(got["period"]) and got["index"] == -1 and got["candidates"] == [] and got["candidate_strengths"] == []
        return
    for f in ("period", "seasonal_strength", "trend_strength", "index", "candidates", "candidate_strengths"):
        assert eq(got[f], want[f]), (where, f, got[f], want[f])


def block(series, extra_cols=3, t_rows=None):
    import torch
    n = len(series)
    ld = (n + extra_cols + 63) // 64 * 64
    T = t_rows or max(1, max(len(s) for s in series))
    y = np.zeros((T, ld))
    ln = np.zeros(ld, dtype=np.int32)
    for i, s in enumerate(series):
        ln[i] = len(s)
        y[:len(s), i] = s
    return torch.from_numpy(y).to("cuda:0"), torch.from_numpy(ln).to("cuda:0"), n, ld


def ssa_block_dicts(out, n, comps):
    """device.ssa_period_block's tensors as the batch entry's dicts."""
    fig, eig, det, st = (out[k].cpu().numpy() for k in ("figures", "eigenvalues", "detected_periods", "status"))
    res = []
    for i in range(n):
        ok = st[i] == 0
        ne = int(fig[2, i]) if ok else 0
        res.append({"ok": bool(ok), "status": int(st[i]), "period": float(fig[0, i]), "variance_explained": float(fig[1, i]), "n_eigenvalues": ne,
                    "eigenvalues": [float(x) for x in eig[:ne, i]], "detected_periods": [float(x) for x in det[:, i] if x == x]})
        assert np.isnan(eig[ne:, i]).all() and eig.shape[0] == comps
    return res


def stl_block_dicts(out, n):
    fig, idx, cand, strength, st = (out[k].cpu().numpy() for k in ("figures", "index", "candidates", "candidate_strengths", "status"))
    res = []
    for i in range(n):
        m = int((cand[:, i] >= 0).sum())
        assert (cand[m:, i] == -1).all() and np.isnan(strength[m:, i]).all()
        res.append({"ok": bool(st[i] == 0), "status": int(st[i]), "period": float(fig[0, i]), "seasonal_strength": float(fig[1, i]),
                    "trend_strength": float(fig[2, i]), "index": int(idx[i]), "candidates": [int(x) for x in cand[:m, i]],
                    "candidate_strengths": [float(x) for x in strength[:m, i]]})
    return res


# --------------------------------------------------------------------------------------------
# SSA
# --------------------------------------------------------------------------------------------
# (name, family, n, period, window_size, n_components)
SSA_CASES = [
    ("n16", "seasonal", 16, 5, None, None),
    ("l4_forced_more_components_than_l", "seasonal", 40, 6, 1, 10),
    ("one_component", "demand", 61, 7, None, 1),
    ("four_components", "seasonal", 90, 12, None, 4),
    ("zeros_break_on_first_norm", "zeros", 40, 6, None, None),
    ("constant_rank_one", "constant", 40, 6, None, None),
    ("sine_rank_two", "sine", 48, 12, None, None),
    ("nan", "nan", 50, 6, None, 3),
    ("inf", "inf", 50, 6, None, 3),
    ("wave_limit_minus_one_l63", "seasonal", 200, 12, 63, 2),
    ("wave_limit_l64", "seasonal", 200, 12, 64, 2),
    ("wave_limit_plus_one_l65", "seasonal", 200, 12, 65, 2),
    ("lds_matrix_limit_l86", "seasonal", 260, 12, None, 2),
    ("lds_matrix_limit_plus_one_l87", "seasonal", 261, 12, None, 2),
    ("lanes_minus_one_l255", "demand", 520, 7, 255, 2),
    ("lanes_l256", "demand", 520, 7, 256, 2),
    ("lanes_plus_one_l257", "demand", 520, 7, 257, 2),
    ("workspace_l130", "seasonal", 390, 12, None, 2),
    ("workspace_l260", "seasonal", 780, 24, None, 2),
    ("series_above_the_lds_tile_window8", "seasonal", 2100, 12, 8, 3),
]


def ssa_case(c):
    name, fam, n, period, window, comps = c
    return PC.family(fam, n, period, seed=len(name)), window, comps


@pytest.mark.parametrize("case", SSA_CASES, ids=lambda c: c[0])
def test_ssa_batch_entry(api, case):
    v, window, comps = ssa_case(case)
    want = ssa_ref(case[0], v, window, comps)
    first = api.ssa_period_batch([v], window, comps)[0]
    check_ssa(first, want, case[0])
    again = api.ssa_period_batch([v], window, comps)[0]                 # run-to-run bits
    assert eq([first[f] for f in ("period", "variance_explained", "eigenvalues", "detected_periods")],
              [again[f] for f in ("period", "variance_explained", "eigenvalues", "detected_periods")])


def test_ssa_single_entry(hiplib):
    L = hiplib.load()
    for case in (SSA_CASES[0], SSA_CASES[1], SSA_CASES[3], SSA_CASES[10], SSA_CASES[13]):
        v, window, comps = ssa_case(case)
        want = ssa_ref(case[0], v, window, comps)
        res, err = hiplib.SsaPeriodResultFFI(), hiplib.AnofoxError()
        assert L.anofox_ts_ssa_period(v.ctypes.data, len(v), window or 0, comps or 0, C.byref(res), C.byref(err)), err.message
        assert eq(float(res.period), want["period"]) and res.variance_explained == want["variance_explained"]
        assert res.n_eigenvalues == want["n_eigenvalues"] and res.method == b"ssa"
    v = np.arange(15.0)
    res, err = hiplib.SsaPeriodResultFFI(), hiplib.AnofoxError()
    assert not L.anofox_ts_ssa_period(v.ctypes.data, 15, 0, 0, C.byref(res), C.byref(err))
    assert err.code == COMPUTATION_ERROR and err.message == b"Insufficient data: need at least 16 observations, got 15"
    v = np.sin(np.arange(4100.0))
    assert not L.anofox_ts_ssa_period(v.ctypes.data, 4100, 2049, 2, C.byref(res), C.byref(err))
    assert err.code == COMPUTATION_ERROR and b"window of 2049 rows" in err.message and b"exceeds the limit of 2048" in err.message


def test_ssa_device_entry_and_routes(hiplib):
    """Windows up to 64 through the one-wavefront route and through the 256-lane route: the same bits; padding columns untouched."""
    from anofox_forecast_amd import device
    for window, comps, names in ((None, None, ("n16", "zeros_break_on_first_norm", "constant_rank_one", "sine_rank_two")),
                                 (64, 2, ("wave_limit_l64",)), (63, 2, ("wave_limit_minus_one_l63",)), (65, 2, ("wave_limit_plus_one_l65",))):
        cases = [c for c in SSA_CASES if c[0] in names]
        series = [ssa_case(c)[0] for c in cases]
        y, ln, n, ld = block(series)
        for route in ("auto", "group"):
            out = device.ssa_period_block(y, ln, window or 0, comps or 0, route=route, n_series=n)
            for got, c in zip(ssa_block_dicts(out, n, comps or 10), cases):
                want = ssa_ref(c[0], ssa_case(c)[0], window, comps)
                assert got["status"] == 0
                for f in ("period", "variance_explained", "n_eigenvalues", "eigenvalues", "detected_periods"):
                    assert eq(got[f], want[f]), (c[0], route, f)
            assert (out["status"][n:] == -1).all() and out["figures"][:, n:].isnan().all()
    with pytest.raises(RuntimeError, match="n_components 33 exceeds the limit of 32"):
        device.ssa_period_block(y, ln, 0, 33)


def test_ssa_window_above_the_limit_fails_alone(api):
    long = PC.family("seasonal", 4100, 12)
    good = PC.family("seasonal", 60, 6)
    res = api.ssa_period_batch([good, long, PC.family("noise", 9)], 2049, 1)
    check_ssa(res[0], ssa_ref("good_w2049", good, 2049, 1), "good")       # its own window is n / 2 = 30
    assert not res[1]["ok"] and res[1]["code"] == COMPUTATION_ERROR and "window of 2049 rows" in res[1]["message"] and "limit of 2048" in res[1]["message"]
    assert not res[2]["ok"] and res[2]["message"] == "Insufficient data: need at least 16 observations, got 9"
    with pytest.raises(api.InvalidInputException, match="n_components 33 exceeds the limit of 32"):
        api.ssa_period_batch([good], None, 33)


def test_ssa_ragged_batch(api):
    """About 130 series in one launch: short and failed ones, every family, windows on both routes and in the workspace.  The tall
    block of the second call shrinks the workspace to 32 slices, so persistent workgroups walk the batch."""
    from anofox_forecast_amd import device
    batch = PC.ssa_ragged_batch()
    assert 120 <= len(batch) <= 140
    want = [ssa_ref(("ragged", i), s, None, 3) for i, s in enumerate(batch)]
    res = api.ssa_period_batch(batch, None, 3)
    for i, (g, w) in enumerate(zip(res, want)):
        check_ssa(g, w, i)
    y, ln, n, ld = block(batch, t_rows=R.MAX_ROWS)
    for _ in range(2):
        out = ssa_block_dicts(device.ssa_period_block(y, ln, 0, 3, n_series=n), n, 3)
        for i, (g, w) in enumerate(zip(out, want)):
            assert g["ok"] == w["ok"] and g["status"] == (0 if w["ok"] else 1), i
            if w["ok"]:
                for f in ("period", "variance_explained", "n_eigenvalues", "eigenvalues", "detected_periods"):
                    assert eq(g[f], w[f]), (i, f)


def test_ssa_mirrors(api):
    v = PC.family("seasonal", 90, 12, seed=len("four_components"))
    want = ssa_ref("four_components", v, None, 4)
    got = api.ts_ssa_period([None] + list(v), None, 4)
    assert got == {"period": want["period"], "variance_explained": want["variance_explained"], "n_eigenvalues": want["n_eigenvalues"], "method": "ssa"}
    assert api.ts_ssa_period(list(v[:15])) is None and api.ts_ssa_period(None) is None
    d = np.arange(90).astype("datetime64[D]")
    out = api.ts_ssa_period_by(["a"] * 90 + ["b"] * 5, np.concatenate([d, d[:5]]), np.concatenate([v, np.ones(5)]), None, 4)
    assert out["period"] == [want["period"], None] and out["variance_explained"][0] == want["variance_explained"] and out["method"] == ["ssa", None]


# --------------------------------------------------------------------------------------------
# STL
# --------------------------------------------------------------------------------------------
# (name, family, n, period, min_period, max_period, n_candidates)
STL_CASES = [
    ("n16", "seasonal", 16, 4, None, None, None),
    ("defaults_n48", "seasonal", 48, 6, None, None, None),
    ("defaults_n96_even_winner", "seasonal", 96, 12, None, None, None),
    ("defaults_n200", "demand", 200, 7, None, None, None),
    ("odd_winner", "sine", 90, 7, None, None, None),
    ("n_equals_2p", "seasonal", 40, 10, None, 1000, None),
    ("five_candidates", "seasonal", 100, 8, 2, 12, 5),
    ("sixty_four_candidates", "seasonal", 150, 12, 2, 70, 64),
    ("one_candidate_means_five", "noise", 60, 5, None, None, 1),
    ("constant", "constant", 50, 5, None, None, None),
    ("zeros", "zeros", 50, 5, None, None, None),
    ("rows_in_lds_n721", "seasonal", 721, 7, 2, 12, 5),
    ("rows_in_workspace_n722", "seasonal", 722, 7, 2, 12, 5),
    ("series_above_the_lds_tile", "seasonal", 2050, 7, 2, 12, 5),
]


def stl_case(c):
    name, fam, n, period, lo, hi, cands = c
    return PC.family(fam, n, period, seed=len(name)), lo, hi, cands


@pytest.mark.parametrize("case", STL_CASES, ids=lambda c: c[0])
def test_stl_batch_entry(api, case):
    v, lo, hi, cands = stl_case(case)
    want = stl_ref(case[0], v, lo, hi, cands)
    first = api.stl_period_batch([v], lo, hi, cands)[0]
    check_stl(first, want, case[0])
    again = api.stl_period_batch([v], lo, hi, cands)[0]
    assert eq([first[f] for f in ("period", "seasonal_strength", "trend_strength", "candidate_strengths")],
              [again[f] for f in ("period", "seasonal_strength", "trend_strength", "candidate_strengths")])


def test_stl_winners_and_lists(api):
    """The cases are what their names say: an even and an odd winner, a candidate with n = 2 p, 5 and 64 candidates."""
    w = {c[0]: stl_ref(c[0], *stl_case(c)) for c in STL_CASES[:9]}
    assert w["defaults_n96_even_winner"]["period"] % 2 == 0 and w["odd_winner"]["period"] % 2 == 1
    assert w["n_equals_2p"]["candidates"][-1] == 20 and len(w["five_candidates"]["candidates"]) == 5
    assert len(w["sixty_four_candidates"]["candidates"]) == 64 and len(w["one_candidate_means_five"]["candidates"]) == 5
    with pytest.raises(api.InvalidInputException, match="n_candidates 65 exceeds the limit of 64"):
        api.stl_period_batch([PC.family("seasonal", 150)], 2, 70, 65)


def test_stl_single_entry(hiplib):
    L = hiplib.load()
    for case in (STL_CASES[0], STL_CASES[2], STL_CASES[6], STL_CASES[9]):
        v, lo, hi, cands = stl_case(case)
        want = stl_ref(case[0], v, lo, hi, cands)
        res, err = hiplib.StlPeriodResultFFI(), hiplib.AnofoxError()
        assert L.anofox_ts_stl_period(v.ctypes.data, len(v), lo or 0, hi or 0, cands or 0, C.byref(res), C.byref(err)), err.message
        assert eq(float(res.period), want["period"]) and res.seasonal_strength == want["seasonal_strength"]
        assert res.trend_strength == want["trend_strength"] and res.method == b"stl"
    v = PC.family("seasonal", 48, 6)
    res, err = hiplib.StlPeriodResultFFI(), hiplib.AnofoxError()
    assert not L.anofox_ts_stl_period(v.ctypes.data, 15, 0, 0, 0, C.byref(res), C.byref(err))
    assert err.code == COMPUTATION_ERROR and err.message == b"Insufficient data: need at least 16 observations, got 15"
    for lo, hi in ((10, 10), (12, 9), (0, 4)):
        assert not L.anofox_ts_stl_period(v.ctypes.data, 48, lo, hi, 0, C.byref(res), C.byref(err))
        assert err.code == COMPUTATION_ERROR and err.message == b"Invalid input: min_period must be less than max_period"


def test_stl_ragged_batch_and_device_entry(api):
    """About 130 series with different candidate lists per series, failures included, through the batch entry and twice through the
    device entry on a tall block (its workspace has fewer slices than the batch has series: persistent workgroups)."""
    from anofox_forecast_amd import device
    batch = PC.stl_ragged_batch()
    assert 110 <= len(batch) <= 140
    want = [stl_ref(("ragged", i), s) for i, s in enumerate(batch)]
    assert len({tuple(w["candidates"]) for w in want if w["ok"]}) > 20
    res = api.stl_period_batch(batch)
    for i, (g, w) in enumerate(zip(res, want)):
        check_stl(g, w, i)
    y, ln, n, ld = block(batch, t_rows=R.MAX_ROWS)
    for _ in range(2):
        blk = device.stl_period_block(y, ln, n_series=n)
        for i, (g, w) in enumerate(zip(stl_block_dicts(blk, n), want)):
            assert g["ok"] == w["ok"] and g["status"] == (0 if w["ok"] else 1), i
            if w["ok"]:
                for f in ("period", "seasonal_strength", "trend_strength", "index", "candidates", "candidate_strengths"):
                    assert eq(g[f], w[f]), (i, f)
        assert (blk["status"][n:] == -1).all() and blk["figures"][:, n:].isnan().all() and (blk["index"][n:] == -1).all()
    # the two input errors, per series: min_period 20 is not below the max_period n / 3 of the shorter series
    mixed = [PC.family("seasonal", 48, 6), PC.family("seasonal", 120, 12), PC.family("noise", 10)]
    res = api.stl_period_batch(mixed, 20)
    assert not res[0]["ok"] and res[0]["message"] == "Invalid input: min_period must be less than max_period"
    check_stl(res[1], stl_ref("mixed1", mixed[1], 20), "mixed1")
    assert not res[2]["ok"] and res[2]["message"] == "Insufficient data: need at least 16 observations, got 10"
    y, ln, n, ld = block(mixed)
    st = device.stl_period_block(y, ln, 20, n_series=n)["status"].cpu().numpy()
    assert list(st[:3]) == [3, 0, 1]


def test_stl_strengths_from_the_mstl_entry(api):
    """Per candidate of two series: the strengths recomputed from the existing MSTL decomposition entry equal the kernel's."""
    for case in (STL_CASES[1], STL_CASES[6]):
        v, lo, hi, cands = stl_case(case)
        got = api.stl_period_batch([v], lo, hi, cands)[0]
        assert got["ok"] and len(got["candidates"]) >= 5
        for p, s in zip(got["candidates"], got["candidate_strengths"]):
            d = api.mstl_decompose_batch([v], [p], 1)[0]
            assert d["ok"] and d["applied"] and d["periods"] == [p]
            assert R.strengths(d)[0] == s, (case[0], p)
        best = got["index"]
        d = api.mstl_decompose_batch([v], [got["candidates"][best]], 1)[0]
        assert R.strengths(d) == (got["seasonal_strength"], got["trend_strength"])


def test_stl_mirrors(api):
    v = PC.family("seasonal", 100, 8, seed=len("five_candidates"))
    want = stl_ref("five_candidates", v, 2, 12, 5)
    got = api.ts_stl_period(list(v) + [None], 2, 12, 5)
    assert got == {"period": want["period"], "seasonal_strength": want["seasonal_strength"], "trend_strength": want["trend_strength"], "method": "stl"}
    assert api.ts_stl_period(list(v[:15])) is None and api.ts_stl_period(None) is None and api.ts_stl_period(list(v), 12, 12) is None
    d = np.arange(100).astype("datetime64[D]")
    out = api.ts_stl_period_by(["a"] * 100 + ["b"] * 5, np.concatenate([d, d[:5]]), np.concatenate([v, np.ones(5)]), 2, 12, 5)
    assert out["period"] == [want["period"], None] and out["seasonal_strength"][0] == want["seasonal_strength"] and out["method"] == ["stl", None]
