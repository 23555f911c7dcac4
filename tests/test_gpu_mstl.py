"""GPU: the MSTL decomposition entries and SeasonalWindowAverage (csrc/fit_mstl.hip) through the C-ABI single, batch and
device-resident entries and the operator mirrors, against the numpy checker tests/mstl_ref.py (the same IEEE operations: equal bit
for bit) and the shapes of the reference's SQL tests.  MSTL / AutoMSTL keep their error."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import mstl_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "mstl_kats.json")))


@pytest.fixture(scope="module")
def env(hiplib, oracle):
    import torch
    assert torch.cuda.is_available()
    from anofox_forecast_amd import api
    return api, oracle, hiplib


def _same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def _interpolated(O, y, valid):
    y = np.ascontiguousarray(y, dtype=np.float64)
    if valid is None or len(y) == 0:
        return y.copy()
    mask = O.validity_mask(valid)
    out = np.empty_like(y)
    O.lib().oracle_fill_nulls_interpolate(y.ctypes.data, mask.ctypes.data, len(y), out.ctypes.data)
    return out


def _ragged(rng, n, lo, hi, periods, null_rate=0.05):
    series, valids = [], []
    for i in range(n):
        m = int(rng.integers(lo, hi + 1))
        t = np.arange(m, dtype=np.float64)
        y = 20.0 + 0.05 * t + rng.normal(0, 1.0, m)
        for p in periods:
            y = y + rng.uniform(1, 5) * np.sin(2 * np.pi * t / p + rng.uniform(0, 6))
        if i % 5 == 0:
            y = np.round(np.abs(y))                          # count-like series too
        v = rng.random(m) >= null_rate
        series.append(y)
        valids.append(v)
    return series, valids


def _check_decomposition(got, y, periods, mode):
    want = R.mstl_decompose(y, periods, mode)
    if "error" in want:
        assert not got["ok"] and got["message"] == "Insufficient data: need at least %d observations, got %d" % want["error"], got
        return
    assert got["ok"] and got["applied"] == want["applied"]
    if not want["applied"]:
        return
    assert got["periods"] == want["periods"]
    assert _same(got["trend"], want["trend"]) and _same(got["remainder"], want["remainder"])
    for a, b in zip(got["seasonal"], want["seasonal"]):
        assert _same(a, b)


@pytest.mark.parametrize("periods,lo,hi", [([7], 3, 120), ([12], 3, 150), ([7, 14], 10, 200), ([24, 168], 100, 800),
                                           ([7, 365], 600, 1913)])
def test_decomposition_parity_with_the_checker(env, periods, lo, hi):
    api = env[0]
    rng = np.random.default_rng(sum(periods) + lo)
    n = 97 if hi <= 200 else 70
    series, valids = _ragged(rng, n, lo, hi, periods)
    zeroed = [np.where(v, y, 0.0) for y, v in zip(series, valids)]       # a NULL counts as 0.0 (the reference's table function)
    for mode in (R.FAIL, R.TREND, R.NONE):
        res = api.mstl_decompose_batch(series, periods, mode, valids)
        for got, y in zip(res, zeroed):
            _check_decomposition(got, y, periods, mode)


def test_decomposition_of_an_m5_sample(env):
    """Series of the bench's M5-shape generator (synth.gen_series), ragged, periods given and auto-detected ones."""
    from anofox_forecast_amd import synth
    api, O, lib = env
    rng = np.random.default_rng(11)
    y = np.asarray(synth.gen_series(5, 0, 128, 1913, m=7), dtype=np.float64)
    lens = rng.integers(200, 1914, len(y))
    series = [y[i, :lens[i]] for i in range(len(y))]
    for periods in ([7], [7, 28], [7, 365]):
        for got, s in zip(api.mstl_decompose_batch(series, periods, R.TREND), series):
            _check_decomposition(got, s, periods, R.TREND)
    # SeasonalWindowAverage on the device-resident block with the periods the batch detects (params := MAP{}), each series
    # against the checker at the period the batch reports for it; the host batch entry detects the same periods
    periods, got = _swa_device(lib, series, 7)
    assert len(set(periods.tolist())) > 1
    for i, s in enumerate(series):
        assert _same(got[i], R.swa_forecast(s, int(periods[i]), 7)), (i, periods[i])
    res, be = api.forecast_batch(series, lib.make_options("SeasonalWindowAverage", 7))
    assert be["ok"]
    for r, g in zip(res, got):
        assert r["ok"] and _same(r["point"], g)


def _swa_device(lib, series, h):
    """SeasonalWindowAverage with detected periods through the device-resident batch: (periods, forecasts [n x h])."""
    import torch
    from anofox_forecast_amd.device import DeviceBatch
    n, T = len(series), max(len(s) for s in series)
    b = DeviceBatch(n, T, lib.make_options("SeasonalWindowAverage", h), "cuda:0")
    yb = np.zeros((T, b.ld))
    for i, s in enumerate(series):
        yb[:len(s), i] = s
    ln = torch.zeros(b.ld, dtype=torch.int32)
    ln[:n] = torch.tensor([len(s) for s in series], dtype=torch.int32)
    b.set_block(torch.from_numpy(yb).cuda(), ln.cuda())
    b.run()
    torch.cuda.synchronize()
    periods = b.periods().copy()
    got = b.results()["yhat"].cpu().numpy().reshape(n, h).copy()
    b.close()
    return periods, got


def test_single_series_entry_and_errors(env):
    api, O, lib = env
    L = lib.load()

    def call(y, periods, mode):
        y = np.ascontiguousarray(y, dtype=np.float64)
        per = (C.c_int * max(len(periods), 1))(*periods)
        res = lib.MstlResult()
        err = lib.AnofoxError()
        ok = L.anofox_ts_mstl_decomposition(y.ctypes.data if len(y) else np.zeros(1).ctypes.data, len(y), per if periods else None,
                                            len(periods), mode, C.byref(res), C.byref(err))
        out = {"ok": bool(ok), "code": err.code, "message": err.message.decode()}
        if ok:
            n = res.n_observations
            out["applied"] = bool(res.decomposition_applied)
            out["trend"] = np.array(res.trend[:n]) if res.trend else None
            out["remainder"] = np.array(res.remainder[:n]) if res.remainder else None
            out["periods"] = [res.seasonal_periods[j] for j in range(res.n_seasonal)]
            out["seasonal"] = [np.array(res.seasonal_components[j][:n]) for j in range(res.n_seasonal)]
            L.anofox_free_mstl_result(C.byref(res))
        return out

    y = 0.1 * np.arange(120) + 5.0 * np.sin(2 * np.pi * np.arange(120) / 12.0)   # decomposition.rs:326-333
    for periods in ([12], [12, 4], [4, 12, 1], []):
        _check_decomposition(call(y, periods, 0), y, periods, 0)
    r = call([1.0, 2.0, 3.0], [12], 0)
    assert not r["ok"] and r["code"] == lib.COMPUTATION_ERROR and r["message"] == "Insufficient data: need at least 24 observations, got 3"
    r = call([1.0, 2.0, 3.0, 4.0, 5.0], [12], 1)
    assert r["ok"] and r["applied"] and r["trend"] is not None and r["seasonal"] == []
    r = call([1.0, 2.0], [12], 2)
    assert r["ok"] and not r["applied"] and r["trend"] is None and r["remainder"] is None
    r = call([], [12], 0)
    assert not r["ok"] and r["message"] == "Insufficient data: need at least 1 observations, got 0"
    # periods beyond any length (the reference compares in usize): the error, a skipped period, or the trend only
    r = call(y, [2 ** 30], 0)
    assert not r["ok"] and r["message"] == "Insufficient data: need at least 2147483648 observations, got 120"
    _check_decomposition(call(y, [2 ** 31 - 1, 12], 0), y, [2 ** 31 - 1, 12], 0)
    r = call(y, [2 ** 30, 2 ** 31 - 1], 1)
    assert r["ok"] and r["applied"] and r["periods"] == [] and _same(r["trend"], R.mstl_decompose(y, [2 ** 30], R.TREND)["trend"])
    batch = [y, y[:7], np.sin(np.arange(3000.0))]
    for got, s in zip(api.mstl_decompose_batch(batch, [2 ** 30, 7, 1500], R.TREND), batch):
        _check_decomposition(got, s, [2 ** 30, 7, 1500], R.TREND)
    # ts_decomposition.test: _ts_mstl_decomposition passes no periods
    lin = np.arange(1.0, 13.0)
    r = call(lin, [], 0)
    assert r["ok"] and r["trend"][11] > r["trend"][0] and abs(r["remainder"][5]) < 5.0 and _same(r["trend"], R.mstl_decompose(lin, [])["trend"])
    assert abs(call(np.full(12, 5.0), [], 0)["trend"][0] - 5.0) < 1.0
    r = call(y, list(range(2, 11)), 0)
    assert not r["ok"] and r["code"] == lib.COMPUTATION_ERROR and "at most 8" in r["message"]
    with pytest.raises(api.InvalidInputException, match="at most 8"):
        api.mstl_decompose_batch([y], list(range(2, 11)))


def test_device_entry_and_batch_independence(env):
    import torch
    api, O, lib = env
    L = lib.load()
    rng = np.random.default_rng(4)
    series, _ = _ragged(rng, 130, 5, 400, [7, 30])
    periods = [7, 30]
    n, T = len(series), max(len(s) for s in series)
    ld = (n + 63) // 64 * 64
    yb = np.zeros((T, ld))
    for i, s in enumerate(series):
        yb[:len(s), i] = s
    dev = torch.device("cuda:0")
    y = torch.from_numpy(yb).to(dev)
    lens = torch.tensor([len(s) for s in series] + [0] * (ld - n), dtype=torch.int32, device=dev)
    tr = torch.full((T, ld), 7.0, dtype=torch.float64, device=dev)
    rm = torch.full((T, ld), 7.0, dtype=torch.float64, device=dev)
    se = torch.full((2, T, ld), 7.0, dtype=torch.float64, device=dev)
    info = torch.zeros(ld, dtype=torch.int32, device=dev)
    per = (C.c_int * 2)(*periods)
    err = lib.AnofoxError()
    torch.cuda.synchronize()
    assert L.anofox_hip_mstl_decompose_device(y.data_ptr(), ld, lens.data_ptr(), n, T, per, 2, 1, tr.data_ptr(), se.data_ptr(),
                                              rm.data_ptr(), info.data_ptr(), None, C.byref(err)), err.message
    tr, rm, se, info = tr.cpu().numpy(), rm.cpu().numpy(), se.cpu().numpy(), info.cpu().numpy()
    whole = api.mstl_decompose_batch(series, periods, R.TREND)
    for i, s in enumerate(series):
        m = len(s)
        w = whole[i]
        assert _same(tr[:m, i], w["trend"]) and _same(rm[:m, i], w["remainder"])
        assert np.all(tr[m:, i] == 7.0)                      # rows past the length are untouched
        used = info[i] & 0xff
        got = [se[k, :m, i] for k in range(2) if (used >> k) & 1]
        assert [p for k, p in enumerate(sorted(periods, reverse=True)) if (used >> k) & 1] == w["periods"]
        assert all(_same(a, b) for a, b in zip(got, w["seasonal"]))
        # batch independence: the series alone gives the same bits
        if i % 13 == 0:
            alone = api.mstl_decompose_batch([s], periods, R.TREND)[0]
            assert _same(alone["trend"], w["trend"]) and _same(alone["remainder"], w["remainder"])


def test_operator_mirror(env):
    api = env[0]
    rows = 60
    grp = np.array(["A"] * rows + ["B"] * rows + ["C"] * 5, dtype=object)
    ds = np.concatenate([np.arange(rows)[::-1], np.arange(rows), np.arange(5)]).astype("datetime64[D]")
    t = np.arange(rows, dtype=np.float64)
    ya = 10 + np.sin(2 * np.pi * t[::-1] / 7)
    yb = 5 + 0.2 * t + np.cos(2 * np.pi * t / 7)
    yc = np.arange(5, dtype=np.float64)
    ys = np.concatenate([ya, yb, yc]).astype(object)
    ys[rows + 3] = None
    out = api.ts_mstl_decomposition_by(grp, ds, ys, [7])
    assert sorted(out) == ["A", "B"]                        # 'fail': the too-short group yields no row
    b = yb.copy(); b[3] = 0.0
    want = R.mstl_decompose(b, [7])
    assert _same(out["B"]["trend"], want["trend"]) and out["B"]["periods"] == [7]
    want = R.mstl_decompose(ya[::-1], [7])                  # rows sorted by date
    assert _same(out["A"]["seasonal"][0], want["seasonal"][0])
    out = api.ts_mstl_decomposition_by(grp, ds, ys, [7], "none")
    assert out["C"] == {"trend": [], "seasonal": [], "remainder": [], "periods": []}
    out = api.ts_mstl_decomposition_by(grp, ds, ys, [7], "trend")
    assert out["C"]["periods"] == [] and len(out["C"]["trend"]) == 5


@pytest.mark.parametrize("period", [0, 7, 12])
def test_seasonal_window_average_parity(env, period):
    api, O, lib = env
    rng = np.random.default_rng(period + 1)
    series, valids = _ragged(rng, 131, 3, 300, [7])
    h = 17
    res, be = api.forecast_batch(series, lib.make_options("SeasonalWindowAverage", h, seasonal_period=period, auto_detect=False,
                                                          include_fitted=True), valids)
    assert be["ok"], be
    for r, y, v in zip(res, series, valids):
        yi = _interpolated(O, y, v)
        assert r["ok"] and r["model_name"] == "SeasonalWindowAverage"
        assert _same(r["point"], R.swa_forecast(yi, max(period, 1), h))
        assert _same(r["fitted"], R.swa_fitted(yi, max(period, 1)))
        assert np.all(r["lower"] <= r["point"]) and np.all(r["point"] <= r["upper"])
    # a series alone gives the same bits
    alone = api.forecast_series(series[5], lib.make_options("SeasonalWindowAverage", h, seasonal_period=period, auto_detect=False),
                                valids[5])
    assert _same(alone["point"], res[5]["point"])


def test_seasonal_window_average_detected_periods_and_sharding(env):
    api, O, lib = env
    rng = np.random.default_rng(8)
    series, _ = _ragged(rng, 300, 40, 200, [7])
    res, be = api.forecast_batch(series, lib.make_options("SeasonalWindowAverage", 9))          # params := MAP{}: detection
    assert be["ok"]
    lib.set_devices([0, 0])
    try:
        lib.load().anofox_hip_set_min_series_per_device(1)
        res2, _ = api.forecast_batch(series, lib.make_options("SeasonalWindowAverage", 9))
    finally:
        lib.set_devices([])
        lib.load().anofox_hip_set_min_series_per_device(2048)
    periods, _ = _swa_device(lib, series, 9)
    for a, b, y, p in zip(res, res2, series, periods):
        assert a["ok"] and _same(a["point"], b["point"])
        assert _same(a["point"], R.swa_forecast(y, int(p), 9)), p


def test_sql_shapes_and_the_models_that_keep_their_error(env):
    api, O, lib = env
    y = KATS["swa_series"]["y"]                              # ts_forecast_exp_smoothing.test:326-336
    r = api.forecast_series(y, lib.make_options("SeasonalWindowAverage", 6))
    assert r["ok"] and r["model_name"] == "SeasonalWindowAverage" and len(r["point"]) == 6
    # ts_forecast_by.test:214-223: two groups, h = 7, params := MAP{}
    rows = 28
    t = np.arange(rows)
    grp = np.array(["a"] * rows + ["b"] * rows, dtype=object)
    ds = np.concatenate([t, t]).astype("datetime64[D]")
    ys = np.concatenate([10 + 5 * np.sin(2 * np.pi * t / 7), 50 + 3 * np.cos(2 * np.pi * t / 7)])
    out = api.ts_forecast_by(grp, ds, ys, "SeasonalWindowAverage", 7, "1d", {})
    assert len(out["yhat"]) == 14 and list(out["model_name"])[0] == "SeasonalWindowAverage"
    y24 = KATS["distinctness_series"]["y"]
    for m in ("MSTL", "AutoMSTL"):
        r = api.forecast_series(y24, lib.make_options(m, 3))
        assert not r["ok"] and r["code"] == lib.INTERNAL_ERROR and "not implemented by the HIP backend" in r["message"]
