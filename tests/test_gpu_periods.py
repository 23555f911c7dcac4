"""GPU: the period-detection entries (anofox_ts_lomb_scargle, anofox_ts_aic_period, anofox_ts_sazed_period,
anofox_ts_detect_periods_flat, anofox_hip_periods_batch, anofox_hip_periods_device) and the operator mirrors against the
restatement tests/periods_ref.py, under the contract of DESIGN.md section 3: the selected grid index -- hence period and frequency
-- n_periods, method strings and flags are EQUAL; every other float figure lies within the tolerance of its input family
(periods_ref.contract: 16 x the measured trig noise, at least 1e-12, relative to the peak power or the best RSS, carried to each
figure by periods_ref.figure_tolerances); NaN exactly where the restatement has NaN; the same bits on two runs and through every
entry.  tests/test_periods_cpu.py checks that every family used here keeps 1,000 tolerances between each decision and its flip."""
import ctypes as C
import math

import numpy as np
import pytest

import periods_cases as PC
import periods_ref as R

pytestmark = pytest.mark.gpu

GRID = {"lomb_scargle": "n_frequencies", "aic": "n_candidates", "sazed": "zero_pad_factor"}
COMPUTATION_ERROR, INTERNAL_ERROR, NULL_POINTER = 3, 10, 1


@pytest.fixture(scope="module")
def api(hiplib):
    import torch
    assert torch.cuda.is_available()
    hiplib.load()
    from anofox_forecast_amd import api as A
    return A


def _single(lib, method, values, min_period=0, max_period=0, grid=0):
    """Through the single-series C entry: (dict or None, code, message)."""
    L = lib.load()
    v = np.ascontiguousarray(values, dtype=np.float64)
    vp = v.ctypes.data if len(v) else np.zeros(1).ctypes.data
    err = lib.AnofoxError()
    if method == "lomb_scargle":
        res = lib.LombScargleResultFFI()
        ok = L.anofox_ts_lomb_scargle(vp, len(v), float(min_period), float(max_period), int(grid), C.byref(res), C.byref(err))
    elif method == "aic":
        res = lib.AicPeriodResultFFI()
        ok = L.anofox_ts_aic_period(vp, len(v), float(min_period), float(max_period), int(grid), C.byref(res), C.byref(err))
    else:
        res = lib.SazedPeriodResultFFI()
        ok = L.anofox_ts_sazed_period(vp, len(v), int(min_period), int(max_period), int(grid), C.byref(res), C.byref(err))
    if not ok:
        return None, int(err.code), err.message.decode()
    out = {f: float(getattr(res, f)) for f in lib.PERIOD_FIGURES[method]}
    out["method"] = res.method.decode()
    return out, 0, ""


def _flat(lib, values, method, max_period=0, min_confidence=-1.0, expected=None, tolerance=-1.0):
    L = lib.load()
    v = np.ascontiguousarray(values, dtype=np.float64)
    res = lib.FlatMultiPeriodResult()
    err = lib.AnofoxError()
    e = np.ascontiguousarray(expected if expected is not None else [], dtype=np.float64)
    ok = L.anofox_ts_detect_periods_flat(v.ctypes.data, len(v), None if method is None else method.encode(), max_period, float(min_confidence),
                                         e.ctypes.data if len(e) else None, len(e), float(tolerance), C.byref(res), C.byref(err))
    if not ok:
        return None, int(err.code), err.message.decode()
    names = ("period", "confidence", "strength", "amplitude", "phase", "iteration", "matches_expected", "matched_expected", "match_deviation")
    periods = [{n: getattr(res, n + "_values")[i] for n in names} for i in range(res.n_periods)]
    if res.n_periods == 0:
        assert not res.period_values and not res.iteration_values
    out = {"periods": periods, "n_periods": int(res.n_periods), "primary_period": float(res.primary_period), "method": res.method.decode()}
    L.anofox_free_flat_multi_period_result(C.byref(res))
    assert not res.period_values and res.n_periods == 0
    return out, 0, ""


def _device(lib, series, method, min_period=0, max_period=0, grid=0, extra_cols=3):
    """Through anofox_hip_periods_device on torch tensors: (list of dicts or None, figures, index, status)."""
    import torch
    L = lib.load()
    n = len(series)
    ld = (n + extra_cols + 63) // 64 * 64
    T = max(1, max(len(s) for s in series))
    y = np.zeros((T, ld))
    ln = np.zeros(ld, dtype=np.int32)
    for i, s in enumerate(series):
        ln[i] = len(s)
        y[:len(s), i] = s
    dev = "cuda:0"
    ty, tln = torch.from_numpy(y).to(dev), torch.from_numpy(ln).to(dev)
    fig = torch.full((lib.PERIODS_N_FP, ld), -777.0, dtype=torch.float64, device=dev)
    idx = torch.full((ld,), -777, dtype=torch.int32, device=dev)
    st = torch.full((ld,), -777, dtype=torch.int32, device=dev)
    err = lib.AnofoxError()
    torch.cuda.synchronize()
    good = L.anofox_hip_periods_device(ty.data_ptr(), ld, tln.data_ptr(), n, T, lib.PERIOD_METHODS[method], float(min_period), float(max_period),
                                       int(grid), fig.data_ptr(), idx.data_ptr(), st.data_ptr(), None, C.byref(err))
    assert good, err.message
    hf, hi, hs = fig.cpu().numpy(), idx.cpu().numpy(), st.cpu().numpy()
    assert (hs[n:] == -777).all() and (hi[n:] == -777).all() and (hf[:, n:] == -777.0).all()       # columns past n_series stay untouched
    used = len(lib.PERIOD_FIGURES[method])
    out = []
    for i in range(n):
        if hs[i] != 0:
            assert hi[i] == -777 and (hf[:, i] == -777.0).all()                                     # nothing else written for a failed series
            out.append(None)
            continue
        assert (hf[used:, i] == -777.0).all()
        r = {f: float(hf[k, i]) for k, f in enumerate(lib.PERIOD_FIGURES[method])}
        r["index"] = int(hi[i])
        out.append(r)
    return out, hs


def _bits(lib, method, r):
    return tuple(np.float64(r[f]).tobytes() for f in lib.PERIOD_FIGURES[method])


def _same(a, b):
    return (a != a and b != b) or a == b


def compare(method, values, got, **kw):
    """`got` (the method's figures, optionally index) against the restatement under the family's contract; returns the list of misses."""
    kw = {k: v for k, v in kw.items() if v}
    c = PC.contract(method, values, **kw)
    assert c["ok"], ("the family fails the precondition of the contract", method, kw)
    ref = c["ref"]
    bad = []
    if "index" in got and got["index"] != ref["index"]:
        bad.append(("index", got["index"], ref["index"]))
    exact = ("period", "frequency") if method == "lomb_scargle" else ("period",)
    for f in exact:
        if not _same(got[f], float(ref[f])):
            bad.append((f, got[f], float(ref[f])))
    tols = R.figure_tolerances(method, ref, c["tol"], len(values))
    for f, t in tols.items():
        want = float(ref[f])
        if math.isnan(want) or math.isinf(want):
            if not _same(got[f], want):
                bad.append((f, got[f], want))
        elif not abs(got[f] - want) <= t:
            bad.append((f, got[f], want, t))
    return bad


def all_entries(api, lib, method, values, min_period=0, max_period=0, grid=0):
    """One problem through the single, batch and device entries, twice: the figures (checked equal bit for bit) with the index."""
    runs = []
    for _ in range(2):
        s, code, msg = _single(lib, method, values, min_period, max_period, grid)
        assert s is not None, (code, msg)
        assert s["method"] == method
        b = api.periods_batch([values], method, min_period, max_period, **{GRID[method]: grid})[0]
        assert b["ok"] and b["method"] == method
        d, st = _device(lib, [values], method, min_period, max_period, grid)
        assert st[0] == 0
        runs += [_bits(lib, method, s), _bits(lib, method, b), _bits(lib, method, d[0])]
        assert b["index"] == d[0]["index"]
    assert len(set(runs)) == 1, runs
    return b


# --------------------------------------------------------------------------------------------
# every length of the list, default parameters, every entry
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,n", PC.LENGTHS, ids=lambda x: str(x))
def test_lengths_all_entries(api, hiplib, fam, n):
    v = PC.family(fam, n)
    for m in R.IMPLEMENTED:
        if n < R.NEEDED[m]:
            text = f"Insufficient data: need at least {R.NEEDED[m]} observations, got {n}"
            assert _single(hiplib, m, v) == (None, COMPUTATION_ERROR, text)
            assert _flat(hiplib, v, m) == (None, COMPUTATION_ERROR, text)
            b = api.periods_batch([v], m)[0]
            assert not b["ok"] and b["code"] == COMPUTATION_ERROR and b["message"] == text and b["index"] == -1 and math.isnan(b["period"])
            d, st = _device(hiplib, [v], m)
            assert d == [None] and st[0] == 1
            continue
        got = all_entries(api, hiplib, m, v)
        assert not compare(m, v, got), (m, compare(m, v, got))
        # the flat entry: the same figures mapped to one DetectedPeriod, filtered at 0.3
        want = R.detect_periods_with_validation(v, m)
        f, code, msg = _flat(hiplib, v, m)
        assert f is not None, msg
        assert f["n_periods"] == len(want["periods"]) and f["method"] == want["method"]
        conf, strength = R.confidence_strength(m, got)
        if f["n_periods"]:
            p = f["periods"][0]
            assert p["period"] == got["period"] == f["primary_period"] and p["confidence"] == conf and p["strength"] == strength
            assert (p["amplitude"], p["phase"], p["iteration"], p["matches_expected"]) == (0.0, 0.0, 1, False)
            assert math.isnan(p["matched_expected"]) and math.isnan(p["match_deviation"])
        else:
            assert f["primary_period"] == 0.0 and f["method"] == m + " (no seasonality)"


# --------------------------------------------------------------------------------------------
# grids, pad factors, explicit ranges
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [1, 2, 63, 64, 65, 1000])
def test_grid_sizes(api, hiplib, grid):
    v = PC.family("sine12", 96)
    for m in ("lomb_scargle", "aic"):
        got = all_entries(api, hiplib, m, v, grid=grid)
        assert not compare(m, v, got, **{GRID[m]: grid}), (m, grid)
    if grid == 1:       # what the source's formula gives for a one-point grid: a NaN grid point
        ls = api.periods_batch([v], "ls", n_frequencies=1)[0]
        assert math.isnan(ls["period"]) and (ls["frequency"], ls["power"], ls["false_alarm_prob"], ls["index"]) == (0.0, 0.0, 1.0, -1)
        a = api.periods_batch([v], "aic", n_candidates=1)[0]
        assert math.isnan(a["period"]) and a["aic"] == -math.inf and a["index"] == 0 and math.isnan(a["rss"]) and math.isnan(a["bic"])


@pytest.mark.parametrize("pad", [1, 2, 4])
def test_sazed_pad_factors(api, hiplib, pad):
    for fam, n in (("sine12", 96), ("poisson7", 120), ("noise", 17)):
        v = PC.family(fam, n)
        got = all_entries(api, hiplib, "sazed", v, grid=pad)
        assert not compare("sazed", v, got, zero_pad_factor=pad), (fam, n, pad)


def test_explicit_period_range(api, hiplib):
    v = PC.family("sine12", 96)
    for m in R.IMPLEMENTED:
        got = all_entries(api, hiplib, m, v, 5, 20)
        assert not compare(m, v, got, min_period=5, max_period=20), m
        assert 5.0 <= got["period"] <= 20.0
    w = PC.family("poisson7", 120)
    got = all_entries(api, hiplib, "lomb_scargle", w, 2.5, 0)
    assert not compare("lomb_scargle", w, got, min_period=2.5)
    # SAZED: a range without a bin gives NaN / 0 / 0, as the source's empty peak list does
    r = api.periods_batch([v], "sazed", min_period=1000)[0]
    assert r["ok"] and math.isnan(r["period"]) and (r["power"], r["snr"], r["index"]) == (0.0, 0.0, -1)


# --------------------------------------------------------------------------------------------
# more than one LDS tile, the spectrum in LDS up to its limit and in the global workspace
# --------------------------------------------------------------------------------------------
def test_series_longer_than_one_tile(api, hiplib):
    v = PC.family("sine12", 2100)                    # 2,048 rows per tile: two tiles
    for m, grid in (("lomb_scargle", 65), ("aic", 20), ("sazed", 1)):
        got = all_entries(api, hiplib, m, v, grid=grid)
        assert not compare(m, v, got, **{GRID[m]: grid}), (m, compare(m, v, got, **{GRID[m]: grid}))


def test_sazed_spectrum_in_workspace(api, hiplib):
    v = PC.family("sine12", 600)                     # padded to 16,384: 8,192 bins, more than the 4,096 of LDS
    got = all_entries(api, hiplib, "sazed", v, grid=16)
    assert not compare("sazed", v, got, zero_pad_factor=16)
    # LDS and workspace spectra side by side in one batch; a workgroup's slice serves one series after another
    mixed = [v, PC.family("sine12", 96), PC.family("sine12", 600, seed=1)]
    res = api.periods_batch(mixed, "sazed", zero_pad_factor=16)
    assert np.float64(res[0]["power"]).tobytes() == np.float64(got["power"]).tobytes()
    for s, r in zip(mixed, res):
        assert r["ok"] and not compare("sazed", s, r, zero_pad_factor=16)


def test_sazed_padding_limit(api, hiplib):
    v = PC.family("sine12", 32)
    text = "SAZED: the zero-padded length of a series of 32 observations exceeds the limit of 16777216 of the HIP backend"
    assert _single(hiplib, "sazed", v, 0, 0, 1 << 20) == (None, COMPUTATION_ERROR, text)
    res = api.periods_batch([v, v], "sazed", zero_pad_factor=1 << 62)
    assert [r["message"] for r in res] == [text, text]


# --------------------------------------------------------------------------------------------
# a ragged batch: more than one wave and more than one workgroup under any mapping
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,grid", [("lomb_scargle", 64), ("aic", 20), ("sazed", 2)])
def test_ragged_batch(api, hiplib, method, grid):
    series = PC.ragged_batch(130)
    runs = []
    for _ in range(2):
        b = api.periods_batch(series, method, **{GRID[method]: grid})
        d, st = _device(hiplib, series, method, grid=grid)
        runs.append([_bits(hiplib, method, r) for r in b])
        for r, q, s in zip(b, d, st):
            assert r["ok"] == (s == 0)
            if r["ok"]:
                assert _bits(hiplib, method, r) == _bits(hiplib, method, q) and r["index"] == q["index"]
    assert runs[0] == runs[1]
    bad, failed = [], 0
    for i, (s, r) in enumerate(zip(series, b)):
        if len(s) < R.NEEDED[method]:
            failed += 1
            assert not r["ok"] and r["message"] == f"Insufficient data: need at least {R.NEEDED[method]} observations, got {len(s)}"
            continue
        bad += [(i,) + x for x in compare(method, s, r, **{GRID[method]: grid})]
    assert failed > 0 and not bad, bad[:8]


# --------------------------------------------------------------------------------------------
# filter, validation, NULLs, mirrors
# --------------------------------------------------------------------------------------------
def test_constant_series(api, hiplib):
    c = np.full(20, 5.0)
    ls = all_entries(api, hiplib, "lomb_scargle", c)
    assert math.isnan(ls["period"]) and math.isnan(ls["frequency"]) and (ls["power"], ls["false_alarm_prob"], ls["index"]) == (0.0, 1.0, -1)
    sz = all_entries(api, hiplib, "sazed", c)
    assert math.isnan(sz["period"]) and (sz["power"], sz["snr"], sz["index"]) == (0.0, 0.0, -1)
    a = all_entries(api, hiplib, "aic", c)           # rss = 0 at the first candidate: aic = -inf there, and the first one wins
    assert (a["period"], a["aic"], a["bic"], a["rss"], a["r_squared"], a["index"]) == (2.0, -math.inf, -math.inf, 0.0, 0.0, 0)
    for m in ("ls", "sazed"):
        f, _, _ = _flat(hiplib, c, m)
        assert f == {"periods": [], "n_periods": 0, "primary_period": 0.0, "method": R.parse_method(m) + " (no seasonality)"}
        k, _, _ = _flat(hiplib, c, m, 0, 0.0)
        assert k["n_periods"] == 1 and math.isnan(k["primary_period"]) and math.isnan(k["periods"][0]["period"])
        assert k["periods"][0]["confidence"] == 0.0 and k["method"] == R.parse_method(m)
        assert api._ts_detect_periods(list(c), m)["method"] == f["method"] and api._ts_detect_periods(list(c), m, 0, 0.0)["n_periods"] == 1


def test_expected_periods_and_nulls(api, hiplib):
    v = PC.family("sine12", 96)
    with_nulls = []
    for i, x in enumerate(v):                        # a NULL before every eighth value
        with_nulls += ([None] if i % 8 == 4 else []) + [float(x)]
    assert len(with_nulls) == 108
    for m in R.IMPLEMENTED:
        want = R.detect_periods_with_validation(v, m, expected_periods=[7.0, 12.0], tolerance=0.1)
        f, code, msg = _flat(hiplib, v, m.upper(), 365, -1.0, [7.0, 12.0], 0.1)
        assert f is not None and f["method"] == m and f["n_periods"] == 1
        p, q = f["periods"][0], want["periods"][0]
        assert p["period"] == q["period"] and p["matches_expected"] and p["matched_expected"] == 12.0 and p["match_deviation"] == q["match_deviation"]
        miss, _, _ = _flat(hiplib, v, m, 0, -1.0, [30.0, 0.0, -12.0], -1.0)
        assert not miss["periods"][0]["matches_expected"] and math.isnan(miss["periods"][0]["matched_expected"])
        # the scalar mirror drops NULL elements and agrees with the flat entry bit for bit
        s = api._ts_detect_periods(with_nulls, m, 0, -1.0, [7.0, 12.0], 0.1)
        sp = s["periods"][0]
        assert (s["n_periods"], s["primary_period"], s["method"]) == (1, f["primary_period"], m)
        assert (sp["period"], sp["confidence"], sp["strength"], sp["matched_expected_period"], sp["match_deviation"]) == \
            (p["period"], p["confidence"], p["strength"], p["matched_expected"], p["match_deviation"])
    assert api._ts_detect_periods(None, "aic") is None and api._ts_detect_periods([1.0, None, 2.0, 3.0], "ls") is None
    ls = api.ts_lomb_scargle(with_nulls, 5.0, 20.0, 64)
    assert ls["method"] == "lomb_scargle" and not compare("lomb_scargle", v, ls, min_period=5.0, max_period=20.0, n_frequencies=64)
    ai = api.ts_aic_period(with_nulls, None, None, 20)
    assert ai["method"] == "aic" and not compare("aic", v, ai, n_candidates=20)
    sz = api.ts_sazed_period(with_nulls, 5, 20, 2)
    assert sz["method"] == "sazed" and not compare("sazed", v, sz, min_period=5, max_period=20, zero_pad_factor=2)
    assert api.ts_sazed_period(list(v[:15])) is None and api.ts_aic_period(list(v[:7])) is None and api.ts_lomb_scargle([1.0, 2.0, 3.0]) is None


def test_by_mirror(api, hiplib):
    fams = [("sine12", 96), ("poisson7", 120), ("noise", 64), ("seasonal_7", 28), ("noise", 5)]
    g, d, val = [], [], []
    for k, (fam, n) in enumerate(fams):
        s = PC.family(fam, n)
        order = np.arange(n)[::-1] if k % 2 else np.arange(n)        # every other group arrives in reverse date order
        g += [f"g{k}"] * n
        d += list(order)
        val += list(s[order])
    d = np.array(d).astype("datetime64[D]")
    for m in R.IMPLEMENTED:
        out = api.ts_detect_periods_by(g, d, np.array(val), {"method": m, "expected_periods": [7.0, 12.0]})
        assert out["id"] == [f"g{k}" for k in range(len(fams))]
        for k, (fam, n) in enumerate(fams):
            s = PC.family(fam, n)
            f, code, msg = _flat(hiplib, s, m, 0, -1.0, [7.0, 12.0], -1.0)
            if f is None:
                assert n < R.NEEDED[m] and out["periods"][k] is None and out["method"][k] is None and out["n_periods"][k] is None
                continue
            assert (out["n_periods"][k], out["primary_period"][k], out["method"][k]) == (f["n_periods"], f["primary_period"], f["method"])
            want = R.detect_periods_with_validation(s, m, expected_periods=[7.0, 12.0])
            assert out["n_periods"][k] == len(want["periods"]) and out["method"][k] == want["method"]
            for p, q, w in zip(out["periods"][k], f["periods"], want["periods"]):
                assert (p["period"], p["confidence"], p["strength"], p["matches_expected"]) == (q["period"], q["confidence"], q["strength"], q["matches_expected"])
                assert p["period"] == w["period"] and p["matches_expected"] == w["matches_expected"]
                assert _same(p["matched_expected_period"], q["matched_expected"]) and _same(p["match_deviation"], q["match_deviation"])
    one = api.ts_detect_periods(d[:96], np.array(val[:96]), {"method": "sazed"})
    assert one["method"] == ["sazed"] and one["n_periods"] == [1]


def test_other_methods_are_errors(api, hiplib):
    v = PC.family("sine12", 96)
    for name in ("fft", "acf", "regression", "multi", "auto", "autoperiod", "cfd_autoperiod", "ssa", "stl", "matrix_profile"):
        text = f"Internal error: period detection method '{name}' is not implemented by the HIP backend"
        assert _flat(hiplib, v, name) == (None, INTERNAL_ERROR, text)
        with pytest.raises(api.InvalidInputException, match="not implemented by the HIP backend"):
            api._ts_detect_periods(list(v), name)
    fft = "Internal error: period detection method 'fft' is not implemented by the HIP backend"
    assert _flat(hiplib, v, "no_such_method") == (None, INTERNAL_ERROR, fft) and _flat(hiplib, v, None) == (None, INTERNAL_ERROR, fft)
    assert _flat(hiplib, v[:3], "periodogram") == (None, INTERNAL_ERROR, fft)       # whatever the length
    L = hiplib.load()
    err = hiplib.AnofoxError()
    res = hiplib.LombScargleResultFFI()
    assert not L.anofox_ts_lomb_scargle(None, 10, 0.0, 0.0, 0, C.byref(res), C.byref(err)) and err.code == NULL_POINTER
    assert not L.anofox_ts_aic_period(v.ctypes.data, len(v), 0.0, 0.0, 0, None, C.byref(err)) and err.code == NULL_POINTER
    assert not L.anofox_ts_sazed_period(None, 10, 0, 0, 0, None, None)
    assert not L.anofox_ts_detect_periods_flat(None, 10, b"ls", 0, -1.0, None, 0, -1.0, None, C.byref(err)) and err.code == NULL_POINTER
    assert err.message == b"Null pointer argument"
    assert not L.anofox_hip_periods_batch(None, None, 1, 7, 0.0, 0.0, 0, None, None, None, C.byref(err)) and err.code == NULL_POINTER
