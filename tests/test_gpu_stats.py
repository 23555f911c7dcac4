"""GPU: the per-series statistics entries (anofox_ts_stats*, anofox_hip_stats_batch, anofox_hip_stats_device) and the operator
mirrors against the restatement tests/stats_ref.py, under the contract of DESIGN.md section 3: counts, booleans, date figures,
min, max, range, median, q1, q3, iqr exact; the figures that are sums within the tolerance measured per input family
(tests/golden/stats_tolerances.json), NaN exactly where the restatement has NaN."""
import ctypes as C
import math

import numpy as np
import pytest

import stats_cases as SC
import stats_ref as R
from test_stats_cpu import check_statement

pytestmark = pytest.mark.gpu

KATS = SC.load_kats()
DAY = 86400 * 10**6


@pytest.fixture(scope="module")
def api(hiplib):
    import torch
    assert torch.cuda.is_available()
    hiplib.load()
    from anofox_forecast_amd import api as A
    return A


def _assert_ok(bad):
    assert not bad, bad[:8]


def _single(lib, values, valid=None, dates=None, freq=0, ftype="FIXED"):
    """Through the single-series C entries."""
    L = lib.load()
    v = np.ascontiguousarray(values, dtype=np.float64)
    res = lib.TsStatsResult()
    err = lib.AnofoxError()
    mask = None
    if valid is not None:
        from anofox_forecast_amd.api import validity_mask
        mask = validity_mask(valid)
    vp = v.ctypes.data if len(v) else np.zeros(1).ctypes.data
    mp = mask.ctypes.data if mask is not None and len(mask) else None
    if dates is None:
        ok = L.anofox_ts_stats(vp, mp, len(v), C.byref(res), C.byref(err))
    else:
        d = np.ascontiguousarray(dates, dtype=np.int64)
        dp = d.ctypes.data if len(d) else np.zeros(1, dtype=np.int64).ctypes.data
        if ftype == "FIXED":
            ok = L.anofox_ts_stats_with_dates(vp, mp, dp, len(v), int(freq), C.byref(res), C.byref(err))
        else:
            ok = L.anofox_ts_stats_with_dates_and_type(vp, mp, dp, len(v), int(freq), lib.FREQUENCY_TYPES[ftype], C.byref(res), C.byref(err))
    assert ok, err.message
    from anofox_forecast_amd.api import _stats_dict
    out = _stats_dict(res)
    L.anofox_free_ts_stats_result(C.byref(res))
    return out


def _device(lib, series, valids=None, dates=None, freq=0, ftype="FIXED", extra_cols=0, sentinel=None):
    """Through anofox_hip_stats_device on torch tensors.  Returns (list of dicts, out_int, out_fp)."""
    import torch
    L = lib.load()
    n = len(series)
    ld = (n + extra_cols + 63) // 64 * 64
    T = max(1, max(len(s) for s in series))
    y = np.zeros((T, ld)); ok = np.ones((T, ld), dtype=np.uint8); dt = np.zeros((T, ld), dtype=np.int64)
    ln = np.zeros(ld, dtype=np.int32)
    for i, s in enumerate(series):
        ln[i] = len(s)
        y[:len(s), i] = s
        if valids is not None and valids[i] is not None:
            ok[:len(s), i] = np.asarray(valids[i], dtype=np.uint8)
        if dates is not None:
            dt[:len(s), i] = dates[i]
    dev = "cuda:0"
    ty, tok, tdt, tln = (torch.from_numpy(a).to(dev) for a in (y, ok, dt, ln))
    oi = torch.full((14, ld), -777 if sentinel is None else sentinel, dtype=torch.int64, device=dev)
    of = torch.full((22, ld), -777.0 if sentinel is None else float(sentinel), dtype=torch.float64, device=dev)
    err = lib.AnofoxError()
    torch.cuda.synchronize()
    good = L.anofox_hip_stats_device(ty.data_ptr(), tok.data_ptr() if valids is not None else None, tdt.data_ptr() if dates is not None else None,
                                     ld, tln.data_ptr(), n, T, int(freq), lib.FREQUENCY_TYPES[ftype], oi.data_ptr(), of.data_ptr(), None,
                                     C.byref(err))
    assert good, err.message
    hi, hf = oi.cpu().numpy(), of.cpu().numpy()
    out = []
    for i in range(n):
        r = {f: int(hi[k, i]) for k, f in enumerate(R.INT_FIELDS)}
        r["is_constant"] = bool(hi[7, i])
        r.update({f: float(hf[k, i]) for k, f in enumerate(R.FP_FIELDS)})
        r["expected_length"] = None if hi[12, i] < 0 else int(hi[12, i])
        r["n_gaps"] = None if hi[13, i] < 0 else int(hi[13, i])
        out.append(r)
    return out, hi, hf


def _bits(r):
    return [np.float64(r[f]).tobytes() if f in R.FP_FIELDS else r[f] for f in R.FIELDS]


# --------------------------------------------------------------------------------------------
# the reference's own statements
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in KATS["scalar"] if not c.get("expect_null") and not c.get("core")], ids=lambda c: c["name"])
def test_scalar_statements(api, hiplib, case):
    vals = SC.cells(case["values"])
    r = api._ts_stats(vals)
    ref = R.compute([0.0 if v is None else v for v in vals], [v is not None for v in vals])
    _assert_ok(SC.compare(r, ref, where=case["name"])[0])
    for f, v in case.get("expect", {}).items():
        assert r[f] == v, (f, r[f], v)
    for f, op, *args in case.get("checks", []):
        assert SC.check(r[f], op, *args), (f, r[f], op, args)
    s = _single(hiplib, [0.0 if v is None else v for v in vals], [v is not None for v in vals])
    assert _bits(s) == _bits(r)


@pytest.mark.parametrize("st", KATS["statements"], ids=lambda s: s["name"])
def test_table_statements(api, st):
    check_statement(api, st)


def test_mirrors_against_restatement(api, monkeypatch):
    """Every mirror gives what it gives with the batch call answered by the restatement."""
    from anofox_forecast_amd import api as A
    rng = np.random.default_rng(7)
    n = 90
    g = [f"g{int(x)}" for x in rng.integers(0, 4, n)]
    d = (np.datetime64("2022-11-01", "us") + rng.permutation(n).astype("timedelta64[D]")).astype("datetime64[us]")
    d[5] = np.datetime64("NaT")
    v = np.array([None if i % 17 == 3 else float("nan") if i % 23 == 5 else float(x) for i, x in enumerate(rng.normal(5, 2, n))], dtype=object)
    calls = [lambda X: X.ts_stats(g, d, v, "1d"), lambda X: X.ts_stats_by(g, d, v, "1d", group_name="gg"),
             lambda X: X.ts_stats_by(g, d, v, "1mo"), lambda X: X.ts_stats_by(g, d, v, "1q"), lambda X: X.ts_stats_by(g, d, v, "1y"),
             lambda X: X.ts_stats(g, d, v, "1mo"), lambda X: {"r": [X.ts_stats_agg(d, v)]},
             lambda X: {"r": [X._ts_stats_with_dates(list(v), d, "2d")]}, lambda X: {"r": [X._ts_stats(list(v))]}]
    got = [c(A) for c in calls]
    monkeypatch.setattr(A, "stats_batch", SC.ref_stats_batch)
    want = [c(A) for c in calls]
    for a, b in zip(got, want):
        assert list(a) == list(b)
        if "r" in a:
            _assert_ok(SC.compare(a["r"][0], b["r"][0])[0])
            continue
        name = list(a)[0]
        assert a[name] == b[name]
        for i in range(len(a[name])):
            _assert_ok(SC.compare({f: a[f][i] for f in R.FIELDS}, {f: b[f][i] for f in R.FIELDS}, where=(name, i))[0])
    assert A._ts_stats(None) is None and A._ts_stats([]) is None


# --------------------------------------------------------------------------------------------
# parity families
# --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fams():
    return SC.families()


@pytest.mark.parametrize("name", ["m5_counts", "m5_positive", "m5_real", "poisson", "level_1e6", "short", "ragged", "long"])
def test_parity_family(api, hiplib, fams, name):
    tol = SC.load_tolerances()[name]
    cases = fams[name]
    series = [c["values"] for c in cases]
    valids = [c["valid"] for c in cases] if any(c["valid"] is not None for c in cases) else None
    got = api.stats_batch(series, valids)
    worst = {f: 0.0 for f in R.TOL_FP}
    bad = []
    for i, c in enumerate(cases):
        ref = R.compute(c["values"], c["valid"])
        b, w = SC.compare(got[i], ref, tol, where=(name, i))
        bad += b
        for f in w:
            worst[f] = max(worst[f], w[f])
    print(f"stats parity {name}: " + " ".join(f"{f}={worst[f]:.2e}" for f in R.TOL_FP))
    _assert_ok(bad)
    if name in SC.COUNT_FAMILIES:                                # the bin counts must be EQUAL even where an argument is exactly .5
        assert all(got[i]["entropy"] == got[i]["entropy"] for i in range(len(cases)))
    again = api.stats_batch(series, valids)                      # two runs, the same bits
    assert [_bits(r) for r in again] == [_bits(r) for r in got]
    dev, _, _ = _device(hiplib, series, valids)
    assert [_bits(r) for r in dev] == [_bits(r) for r in got]
    for i in (0, len(cases) - 1):                                # the single entry, the same bits
        assert _bits(_single(hiplib, series[i], None if valids is None else valids[i])) == _bits(got[i])


# --------------------------------------------------------------------------------------------
# lengths across both paths, special values, dates
# --------------------------------------------------------------------------------------------
def test_mixed_lengths_both_paths(api, hiplib):
    rng = np.random.default_rng(11)
    lens = [0, 1, 2, 3, 9, 10, 64, 65, 2047, 2048, 2049, 5000, 20000]
    series = [np.round(rng.normal(0.0, 4.0, n), 1) for n in lens]
    valids = [rng.random(n) >= 0.03 for n in lens]
    dates = [rng.permutation(n).astype(np.int64) * DAY for n in lens]
    got = api.stats_batch(series, valids, dates, DAY, "FIXED")
    # the rule of the contract on these very inputs: max(1e-12, 16 x the deviation between the source order and the other two)
    tol = R.noise_table({"mixed": [dict(values=s, valid=v) for s, v in zip(series, valids)]})["mixed"]
    for i, n in enumerate(lens):
        ref = R.compute(series[i], valids[i], dates[i], DAY, "FIXED")
        _assert_ok(SC.compare(got[i], ref, tol, where=n)[0])
    assert got[0]["length"] == 0 and math.isnan(got[0]["mean"]) and got[0]["expected_length"] is None
    dev, hi, hf = _device(hiplib, series, valids, dates, DAY, "FIXED", extra_cols=3)
    assert [_bits(r) for r in dev] == [_bits(r) for r in got]
    assert (hi[:, len(lens):] == -777).all() and (hf[:, len(lens):] == -777.0).all()      # columns beyond n_series stay untouched


def test_special_values(api, hiplib):
    nan, inf = float("nan"), float("inf")
    series = [[0.0, -0.0, 0.0, -0.0, 1.0, 1.0, -0.0, 0.0, 0.0, 2.0, 2.0, 2.0, 0.0],
              [1.0, inf, 2.0, -3.0] * 4,
              [1.0, inf, -inf, 2.0] * 3,
              [nan] * 6,
              [3.25] * 40,
              [1.0, -1.0] * 8,
              [0.0] * 5 + [1.0, 2.0, 3.0, 4.0, 5.0, 6.0],
              [0.0, 0.0, 5.0, nan, 5.0, 5.0, 0.0, 7.0, 7.0, 0.0, 0.0],
              list(np.arange(30.0) % 3),
              [1e-300, 2e-300, -1e-300] * 5]
    valids = [None, None, None, None, None, None, None, [True, False] + [True] * 9, None, None]
    valids[3] = [True, False, True, True, False, True]
    got = api.stats_batch([np.array(s) for s in series], [None if v is None else np.array(v) for v in valids])
    tol = R.noise_table({"special": [dict(values=np.array(s), valid=v) for s, v in zip(series, valids)]})["special"]
    for i, s in enumerate(series):
        ref = R.compute(s, valids[i])
        _assert_ok(SC.compare(got[i], ref, tol, where=i)[0])
    assert got[0]["n_unique_values"] == 4 and got[3]["n_nan"] == 4 and got[3]["mean"] == 0.0 and got[4]["is_constant"]
    assert math.isnan(got[5]["coef_variation"]) and math.isnan(got[6]["tail_index"]) and got[7]["n_zeros_start"] == 1
    dev, _, _ = _device(hiplib, [np.array(s) for s in series], [None if v is None else np.array(v) for v in valids])
    assert [_bits(r) for r in dev] == [_bits(r) for r in got]


def test_dates(api, hiplib):
    us = lambda s: int(np.datetime64(s, "us").astype(np.int64))           # noqa: E731
    rng = np.random.default_rng(5)
    monthly = [us(f"20{10 + k // 12:02d}-{k % 12 + 1:02d}-{1 + int(rng.integers(0, 28)):02d}") for k in rng.permutation(70)[:50]]
    old = [us("1969-12-31T23:59:59"), us("1960-02-29"), us("1955-05-05") + 1, us("1969-11-30"), us("1971-03-01"), us("1969-12-31T23:59:59") + 500000]
    cases = [(monthly, 0), (monthly + monthly[:7], 0), (old, 0), ([us("2024-02-29")], 0), (sorted(monthly), 30 * DAY),
             ([0, DAY + DAY // 2, 3 * DAY + 1, 3 * DAY + 1], DAY), ([5 * DAY, 0], 0), (list(rng.permutation(3000).astype(np.int64) * DAY), DAY)]
    for ftype in ("FIXED", "MONTHLY", "QUARTERLY", "YEARLY"):
        series = [np.arange(float(len(d))) for d, _ in cases]
        for f in sorted({f for _, f in cases}):
            idx = [i for i, (_, ff) in enumerate(cases) if ff == f]
            got = api.stats_batch([series[i] for i in idx], None, [np.array(cases[i][0], dtype=np.int64) for i in idx], f, ftype)
            for k, i in enumerate(idx):
                ref = R.compute(series[i], None, cases[i][0], f, ftype)
                assert (got[k]["expected_length"], got[k]["n_gaps"]) == (ref["expected_length"], ref["n_gaps"]), (ftype, i, got[k], ref)
                s = _single(hiplib, series[i], None, cases[i][0], f, ftype)
                assert (s["expected_length"], s["n_gaps"]) == (ref["expected_length"], ref["n_gaps"])
    mixed = api.stats_batch([np.arange(4.0), np.arange(3.0)], None, [np.array([0, DAY, 2 * DAY, 5 * DAY]), None], DAY)
    assert (mixed[0]["expected_length"], mixed[0]["n_gaps"], mixed[1]["expected_length"], mixed[1]["n_gaps"]) == (6, 1, None, None)


def test_null_pointers_and_empty(hiplib):
    L = hiplib.load()
    res, err = hiplib.TsStatsResult(), hiplib.AnofoxError()
    v = np.arange(4.0)
    assert not L.anofox_ts_stats(None, None, 4, C.byref(res), C.byref(err)) and err.code == 1
    assert not L.anofox_ts_stats(v.ctypes.data, None, 4, None, C.byref(err)) and err.code == 1
    assert not L.anofox_ts_stats_with_dates(v.ctypes.data, None, None, 4, DAY, C.byref(res), C.byref(err)) and err.code == 1
    assert not L.anofox_ts_stats_with_dates_and_type(v.ctypes.data, None, None, 4, DAY, 1, C.byref(res), C.byref(err)) and err.code == 1
    assert L.anofox_ts_stats(v.ctypes.data, None, 0, C.byref(res), C.byref(err))
    assert res.length == 0 and math.isnan(res.mean) and math.isnan(res.stability) and not res.has_date_metrics
    d = np.arange(4, dtype=np.int64)
    assert L.anofox_ts_stats_with_dates(v.ctypes.data, None, d.ctypes.data, 0, DAY, C.byref(res), C.byref(err))
    assert res.length == 0 and math.isnan(res.sum) and not res.has_date_metrics
