"""GPU: the seasonality entries (anofox_ts_detect_seasonality, anofox_ts_analyze_seasonality, anofox_hip_seasonality_batch,
anofox_hip_seasonality_device), device.seasonality_block and the SQL mirrors of api.py against the restatement
tests/seasonality_ref.py.  The contract is equality of bits through every entry and on every run; the only
exemption is a NaN's payload."""
import ctypes as C

import numpy as np
import pytest

import seasonality_cases as SC
import seasonality_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
ISENT = -555


@pytest.fixture(scope="module")
def api(hiplib):
    import torch
    assert torch.cuda.is_available()
    hiplib.load()
    from anofox_forecast_amd import api as A
    return A


_MEMO = {}


def want(series, max_period=0):
    """The restatement's answer, computed once per (series, max_period) and left unchanged."""
    key = (id(series), max_period)
    if key not in _MEMO:
        _MEMO[key] = (series, SC.expected(series, max_period))
    return _MEMO[key][1]


def _device(lib, batch, max_period=0, t_rows=None, extra_cols=5):
    """anofox_hip_seasonality_device on torch tensors; the outputs start as a sentinel.  Returns (out_int [8 x ld], out_fp [12 x ld])."""
    import torch
    L = lib.load()
    dev = "cuda:0"
    y, v, lens, ld = SC.block(batch, t_rows, extra_cols)
    yd, ld_, lensd = torch.from_numpy(y).to(dev), ld, torch.from_numpy(lens).to(dev)
    vd = torch.from_numpy(v).to(dev) if v is not None else None
    oi = torch.full((8, ld), ISENT, dtype=torch.int32, device=dev)
    of = torch.full((12, ld), SENTINEL, dtype=torch.float64, device=dev)
    err = lib.AnofoxError()
    torch.cuda.synchronize()
    ok = L.anofox_hip_seasonality_device(yd.data_ptr(), None if vd is None else vd.data_ptr(), ld_, lensd.data_ptr(), len(batch), y.shape[0],
                                         max_period, oi.data_ptr(), of.data_ptr(), None, C.byref(err))
    assert ok, err.message
    return oi.cpu().numpy(), of.cpu().numpy()


def _column(oi, of, i):
    """Column i of the device outputs in the shape of the restatement's dict (all five slots kept)."""
    return {"periods": [int(x) for x in oi[:5, i]], "n_periods": int(oi[5, i]), "primary_period": int(oi[6, i]), "status": int(oi[7, i]),
            "strengths": [float(x) for x in of[:5, i]], "acf": [float(x) for x in of[5:10, i]], "seasonal_strength": float(of[10, i]),
            "trend_strength": float(of[11, i])}


def _column_ok(col, w):
    k = len(w["detected_periods"])
    pad = 5 - k
    return (col["status"] == w["status"] and col["n_periods"] == k and col["periods"] == w["detected_periods"] + [0] * pad
            and col["primary_period"] == w["primary_period"]
            and all(SC.same_bits(a, b) for a, b in zip(col["strengths"], w["strengths"] + [0.0] * pad))
            and all(SC.same_bits(a, b) for a, b in zip(col["acf"], w["acf"] + [0.0] * pad))
            and SC.same_bits(col["seasonal_strength"], w["seasonal_strength"]) and SC.same_bits(col["trend_strength"], w["trend_strength"]))


def _check_device(got, batch, max_period=0, where=""):
    oi, of = got
    n = len(batch)
    bad = [(where, i, len(s), _column(oi, of, i), want(s, max_period)) for i, s in enumerate(batch)
           if not _column_ok(_column(oi, of, i), want(s, max_period))]
    assert not bad, bad[:3]
    assert (oi[:, n:] == ISENT).all() and (of[:, n:] == SENTINEL).all()          # ld > n_series: the other columns are untouched


def _dict_ok(g, w):
    return (g["status"] == w["status"] and g["detected_periods"] == w["detected_periods"] and g["primary_period"] == w["primary_period"]
            and len(g["strengths"]) == len(w["strengths"]) and all(SC.same_bits(a, b) for a, b in zip(g["strengths"], w["strengths"]))
            and len(g["acf"]) == len(w["acf"]) and all(SC.same_bits(a, b) for a, b in zip(g["acf"], w["acf"]))
            and SC.same_bits(g["seasonal_strength"], w["seasonal_strength"]) and SC.same_bits(g["trend_strength"], w["trend_strength"])
            and g["is_seasonal"] == w["is_seasonal"])


def _check_batch(api, batch, max_period=0, where=""):
    got = api.seasonality_batch([np.array(SC.split(s)[0], dtype=np.float64) for s in batch], [SC.split(s)[1] for s in batch], max_period)
    bad = [(where, i, len(s), g, want(s, max_period)) for i, (g, s) in enumerate(zip(got, batch)) if not _dict_ok(g, want(s, max_period))]
    assert not bad, bad[:3]


def _check_singles(lib, series, max_period=0):
    """The two C singles on a series without NULLs."""
    L = lib.load()
    w = want(series, max_period)
    v = np.array(series, dtype=np.float64)
    ptr = v.ctypes.data if len(v) else np.zeros(1).ctypes.data
    periods, n, err = C.POINTER(C.c_int)(), C.c_size_t(77), lib.AnofoxError()
    ok = L.anofox_ts_detect_seasonality(ptr, len(v), max_period, C.byref(periods), C.byref(n), C.byref(err))
    res, err2 = lib.SeasonalityResult(), lib.AnofoxError()
    ok2 = L.anofox_ts_analyze_seasonality(None, 0, ptr, len(v), max_period, C.byref(res), C.byref(err2))
    if w["status"] == R.SHORT:
        text = f"Insufficient data: need at least 4 observations, got {len(v)}".encode()
        assert not ok and not ok2 and err.code == 3 and err2.code == 3 and err.message == text and err2.message == text
        return
    assert ok and ok2, (err.message, err2.message)
    assert [periods[i] for i in range(n.value)] == w["detected_periods"] and bool(periods) == (n.value > 0)
    assert [res.detected_periods[i] for i in range(res.n_periods)] == w["detected_periods"] and bool(res.detected_periods) == (res.n_periods > 0)
    assert res.primary_period == w["primary_period"]
    assert SC.same_bits(res.seasonal_strength, w["seasonal_strength"]) and SC.same_bits(res.trend_strength, w["trend_strength"])
    L.anofox_free_int_array(periods)
    L.anofox_free_seasonality_result(C.byref(res))
    assert not res.detected_periods


def _check_mirrors(api, series):
    w = want(series)
    d, a = api.ts_detect_seasonality(series), api.anofox_fcst_ts_analyze_seasonality(list(range(len(series))), series)
    if w["status"] == R.SHORT:
        assert d is None and a is None
        return
    assert d == w["detected_periods"] and a["detected_periods"] == w["detected_periods"] and a["primary_period"] == w["primary_period"]
    assert SC.same_bits(a["seasonal_strength"], w["seasonal_strength"]) and SC.same_bits(a["trend_strength"], w["trend_strength"])
    assert list(a) == ["detected_periods", "primary_period", "seasonal_strength", "trend_strength"]


def _check_all(hiplib, api, batch, max_period=0, singles=None):
    _check_device(_device(hiplib, batch, max_period), batch, max_period, "device")
    _check_batch(api, batch, max_period, "batch")
    for s in (batch if singles is None else singles):
        if None not in s:
            _check_singles(hiplib, s, max_period)
        if max_period == 0:
            _check_mirrors(api, s)


SHORT = SC.short_batch()
MAXP = SC.max_period_batch()
STRIDE = SC.stride_batch()
BOUNDARY = SC.boundary_series()
RAGGED = SC.ragged_batch()
NULLS = SC.null_batch()
TIES_EQUAL, TIES_UNORDERED = SC.tie_cases()
EDGES = SC.edge_batch()


def test_short_lengths(hiplib, api):
    assert [want(s)["status"] for s in SHORT[:6]] == [1, 1, 1, 1, 0, 0]
    assert all(want(s)["detected_periods"] == [] for s in SHORT[:6])             # n = 4, 5: max_lag 2, the peak loop is empty
    assert want(SHORT[11])["detected_periods"] == [2] and want(SHORT[12])["detected_periods"] == [2]        # n = 6, 7: one candidate lag
    _check_all(hiplib, api, SHORT)


def test_max_period(hiplib, api):
    two = MAXP[0]
    assert want(two, 36)["primary_period"] == 35 and want(two, 35)["primary_period"] == 5       # 35 cuts off the strongest peak
    for mp in SC.MAX_PERIODS + (0, -3):
        _check_all(hiplib, api, MAXP, mp, singles=MAXP[:2])


def test_lag_stride(hiplib, api):
    assert [len(s) // 2 for s in STRIDE[:3]] == [256, 257, 515]
    _check_all(hiplib, api, STRIDE, singles=STRIDE[:3])
    _check_device(_device(hiplib, STRIDE, 257), STRIDE, 257)
    _check_device(_device(hiplib, STRIDE[:2], 0, t_rows=600), STRIDE[:2], 0)      # t_rows above every length


def test_storage_boundary(hiplib, api):
    """One series at the LDS limit and one a row above it; the series at the limit in blocks of both heights gives equal bits."""
    a, b = BOUNDARY
    assert len(a) == hiplib.SEASONALITY_LDS_ROWS and len(b) == len(a) + 1
    in_lds = _device(hiplib, [a])
    in_global = _device(hiplib, [a, b])
    _check_device(in_lds, [a], where="lds")
    _check_device(in_global, [a, b], where="global")
    assert _column(*in_lds, 0) == _column(*in_global, 0) and want(a)["detected_periods"]
    _check_batch(api, [b])
    _check_singles(hiplib, b)


def test_ragged_block(hiplib, api):
    assert [len(s) for s in RAGGED] == list(range(71))
    _check_device(_device(hiplib, RAGGED, extra_cols=30), RAGGED)
    _check_device(_device(hiplib, RAGGED, 4, t_rows=75), RAGGED, 4)
    _check_batch(api, RAGGED)
    for s in RAGGED[::7]:
        _check_singles(hiplib, s)
        _check_mirrors(api, s)


def test_null_masks(hiplib, api):
    assert [want(s)["status"] for s in NULLS[3:6]] == [1, 1, 0] and [want(s)["n"] for s in NULLS[3:6]] == [0, 3, 4]
    _check_device(_device(hiplib, NULLS), NULLS)
    _check_batch(api, NULLS)
    compacted = [R.compact(s) for s in NULLS]
    got_masked, got_compact = _device(hiplib, NULLS), _device(hiplib, compacted)
    for i in range(len(NULLS)):
        assert _column(*got_masked, i) == _column(*got_compact, i), i
    for s in NULLS[:8]:
        _check_mirrors(api, s)


def test_ties_keep_the_stable_order(hiplib, api):
    assert len(TIES_EQUAL) >= 10 and len(TIES_UNORDERED) >= 10
    assert all(SC._tie_kind(s)[0] for s in TIES_EQUAL) and all(SC._tie_kind(s)[1] for s in TIES_UNORDERED)
    _check_all(hiplib, api, TIES_EQUAL + TIES_UNORDERED, singles=TIES_EQUAL[:4] + TIES_UNORDERED[:2])


def test_many_peaks_two_periods_edges_and_non_finite(hiplib, api):
    assert len(want(EDGES["many_peaks"])["detected_periods"]) == 5
    two = want(EDGES["two_periods"])["detected_periods"]
    assert two[0] > two[1]                                                        # the stronger peak is the longer lag
    for name in ("constant", "constant_zero", "tiny_variance", "ramp", "steep_ramp", "nan", "inf", "neg_inf", "huge", "overflowing_sum"):
        assert want(EDGES[name])["detected_periods"] == [], name
    assert want(EDGES["ramp"])["trend_strength"] == 1.0 and want(EDGES["nan"])["trend_strength"] != want(EDGES["nan"])["trend_strength"]
    _check_all(hiplib, api, list(EDGES.values()))


def test_primary_period_agrees_with_the_forecast_path(hiplib, api):
    """For a block without NULLs and lengths >= 4, primary_period is what the forecast batch's auto-detection adopts (0 -> 1)."""
    import torch
    from anofox_forecast_amd.device import DeviceBatch
    series = [s for s in STRIDE[:4] + MAXP + RAGGED[4:] + TIES_EQUAL + TIES_UNORDERED + [EDGES["many_peaks"], EDGES["constant"], EDGES["ramp"]]]
    n, T = len(series), max(len(s) for s in series)
    opts = hiplib.make_options("AutoETS", 6)
    assert opts.auto_detect_seasonality and opts.seasonal_period == 0
    b = DeviceBatch(n, T, opts, "cuda:0")
    y = np.zeros((T, b.ld))
    ln = np.zeros(b.ld, dtype=np.int32)
    for s, v in enumerate(series):
        y[:len(v), s] = v
        ln[s] = len(v)
    yd, lnd = torch.from_numpy(y).cuda(), torch.from_numpy(ln).cuda()
    b.set_block(yd, lnd)
    adopted = b.periods()
    b.close()
    from anofox_forecast_amd import device
    r = device.seasonality_block(yd, lnd, n_series=n)
    primary = r["primary_period"][:n].cpu().numpy()
    assert np.array_equal(np.where(primary == 0, 1, primary), adopted[:n])
    assert len(set(primary.tolist())) > 8


def test_device_wrapper_and_determinism(hiplib, api):
    """device.seasonality_block keeps everything on the device; two runs give identical bits."""
    import torch
    from anofox_forecast_amd import device
    batch = NULLS + STRIDE[:2] + TIES_EQUAL[:3]
    y, v, lens, ld = SC.block(batch)
    yd, vd, ld_ = torch.from_numpy(y).cuda(), torch.from_numpy(v).cuda(), torch.from_numpy(lens).cuda()
    r1 = device.seasonality_block(yd, ld_, vd.bool(), n_series=len(batch))
    r2 = device.seasonality_block(yd, ld_, vd, 0, n_series=len(batch))
    for k in ("figures", "values", "periods", "strengths", "is_seasonal"):
        assert r1[k].is_cuda
    assert torch.equal(r1["figures"], r2["figures"]) and torch.equal(r1["values"].view(torch.int64), r2["values"].view(torch.int64))
    oi, of = r1["figures"].cpu().numpy(), r1["values"].cpu().numpy()
    for i, s in enumerate(batch):
        assert _column_ok(_column(oi, of, i), want(s)), i
        assert bool(r1["is_seasonal"][i]) == want(s)["is_seasonal"]
    assert (oi[:, len(batch):] == -1).all() and np.isnan(of[:, len(batch):]).all()
    a, b = _device(hiplib, STRIDE), _device(hiplib, STRIDE)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int64), b[1].view(np.int64))


def test_golden_statements_through_the_mirrors(api):
    for st in SC.load_kats()["statements"]:
        assert SC.golden_holds(st, api.ts_detect_seasonality, api.ts_analyze_seasonality), st["src"]
