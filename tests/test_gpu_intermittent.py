"""GPU: the intermittent-demand models (CrostonClassic, CrostonSBA, TSB, ADIDA, IMAPA; csrc/fit_intermittent.hip) through every
layer above the kernels -- the C-ABI single and batch entries, the device-resident batch, multi-device sharding and the operator
mirrors -- against the numpy checker tests/intermittent_ref.py (the same IEEE operations: equal to REL_TOL = 1e-12 relative) and
the reference's pins and SQL tests (test/sql/ts_model_distinctness.test, test/sql/ts_forecast_intermittent.test)."""
import json
import multiprocessing as mp
import os
import sys

import numpy as np
import pytest

import intermittent_ref as R

pytestmark = pytest.mark.gpu

REL_TOL = 1e-12
MODELS = R.MODELS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "intermittent_kats.json")))
Y30 = np.array(KATS["distinctness_series"]["y"])
Y12 = np.array(KATS["short_series"]["y"])


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return np.inf
    same = (np.isnan(a) & np.isnan(b)) | (a == b)
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b) / np.maximum(1.0, np.abs(b))
    d[same] = 0.0
    d[np.isnan(d)] = np.inf
    return float(np.max(d)) if d.size else 0.0


@pytest.fixture(scope="module")
def env(hiplib, oracle):
    import torch
    assert torch.cuda.is_available()
    from anofox_forecast_amd import api, synth
    return api, oracle, hiplib, synth


def _interpolated(O, y, valid):
    """The wrapper's NULL interpolation (imputation.rs), as the oracle restates it: what the kernels see."""
    y = np.ascontiguousarray(y, dtype=np.float64)
    if valid is None or len(y) == 0:
        return y.copy()
    mask = O.validity_mask(valid)
    out = np.empty_like(y)
    O.lib().oracle_fill_nulls_interpolate(y.ctypes.data, mask.ctypes.data, len(y), out.ctypes.data)
    return out


def _table(spec, i):
    if "intercept" in spec:
        return spec["intercept"] + i * spec["slope"]
    if "at_index" in spec:
        return np.array([spec["at_index"].get(str(k), spec["otherwise"]) for k in i])
    v = np.full(len(i), spec["otherwise"])
    done = np.zeros(len(i), bool)
    for mod, val in spec["first_matching_modulus"]:
        hit = (i % mod == 0) & ~done
        v[hit] = val
        done |= hit
    return v


def test_pins_and_names_through_the_c_abi(env):
    """test/sql/ts_model_distinctness.test:45-66 through anofox_ts_forecast: four pins to 6 dp, IMAPA at its labelled deviation."""
    api, O, lib, synth = env
    pins = KATS["pins"]["point_1"]
    got = {}
    for m in MODELS:
        r = api.forecast_series(Y30, lib.make_options(m, 3))
        assert r["ok"], (m, r)
        assert r["model_name"] == m
        assert np.all(r["point"] == r["point"][0])
        got[m] = float(r["point"][0])
        assert got[m] == R.point_forecasts([Y30], m)[0], m
    for m in ("CrostonClassic", "CrostonSBA", "TSB", "ADIDA"):
        assert round(got[m], 6) == pins[m], m
    assert round(got["IMAPA"], 6) == 1.226437 and abs(got["IMAPA"] / pins["IMAPA"] - 1.0) < 5e-5
    assert len(set(got.values())) == len(got)


def test_croston_optimized_keeps_its_error(env):
    api, O, lib, synth = env
    for name in ("CrostonOptimized", "croston_optimized"):
        r = api.forecast_series(Y30, lib.make_options(name, 3))
        assert not r["ok"] and r["code"] == lib.INTERNAL_ERROR
        assert r["message"] == "Internal error: model 'CrostonOptimized' is not implemented by the HIP backend"


def _parity_batch(synth, n=700, T=400, seed=4401):
    """Synthetic M5 series (raw counts): ragged lengths, NULL masks, all-zero series, single demands (one at the last row: K = n),
    series without zeros, too-short and empty series."""
    rng = np.random.default_rng(seed)
    Y = synth.gen_series(synth.SEED_M5, 12000, n, T, 7, positive=False)
    lens = rng.integers(3, T + 1, n)
    series = [Y[s, :lens[s]].copy() for s in range(n)]
    valids = [None if s % 3 else rng.random(lens[s]) > 0.05 for s in range(n)]
    for s in range(0, n, 97):
        valids[s] = None
        series[s][:] = 0.0                                  # no demand
    for s in range(5, n, 89):
        series[s][:] = 0.0
        series[s][rng.integers(0, len(series[s]))] = 3.0    # a single demand
    for s in range(7, n, 83):
        series[s][:] = 0.0
        series[s][-1] = 6.0                                 # a single demand at the last row
        valids[s] = None
    for s in range(11, n, 79):
        series[s] = series[s] + 1.0                         # no zeros (K = 1)
    series += [np.array([0.0, 5.0, 0.0]), np.array([1.0, 2.0]), np.array([]), np.zeros(50)]
    valids += [None, None, None, None]
    return series, valids


def test_parity_with_the_checker(env):
    api, O, lib, synth = env
    series, valids = _parity_batch(synth)
    clean = [_interpolated(O, y, v) for y, v in zip(series, valids)]
    worst = 0.0
    for h in (1, 28, 50):
        naive, nerr = api.forecast_batch(series, lib.make_options("Naive", h), valids)
        assert nerr["ok"]
        for m in MODELS:
            got, berr = api.forecast_batch(series, lib.make_options(m, h), valids)
            assert berr["ok"], (m, berr)
            ref = R.point_forecasts(clean, m)
            for s in range(len(series)):
                assert got[s]["ok"] == naive[s]["ok"] and got[s]["code"] == naive[s]["code"], (m, h, s, got[s], naive[s])
                if not got[s]["ok"]:
                    continue
                assert got[s]["model_name"] == m
                pt = got[s]["point"]
                assert len(pt) == h
                worst = max(worst, _rel(pt, np.full(h, ref[s])))
                width, nwidth = got[s]["upper"] - got[s]["lower"], naive[s]["upper"] - naive[s]["lower"]
                assert _rel(width, nwidth) <= REL_TOL, (m, h, s)
                assert _rel((got[s]["upper"] + got[s]["lower"]) * 0.5, pt) <= REL_TOL, (m, h, s)
    assert worst <= REL_TOL, worst


def _check_chunk(args):
    """Worker of the full-size comparison (a fresh interpreter: it never touches the GPU)."""
    tests_dir, Y, model = args
    if tests_dir not in sys.path:
        sys.path.insert(0, tests_dir)
    import intermittent_ref as Rw
    return Rw.point_forecasts(list(Y), model)


def test_full_m5_block_against_the_checker(env):
    """All 30,490 x 1,913 synthetic M5 series (raw counts) for every model; the checker runs on up to 15 worker processes."""
    api, O, lib, synth = env
    n, T = 30490, 1913
    Y = synth.gen_series(synth.SEED_M5, 0, n, T, 7, positive=False)
    chunks = [Y[a:a + 1024] for a in range(0, n, 1024)]
    tests_dir = os.path.dirname(os.path.abspath(__file__))
    workers = max(1, min(15, (os.cpu_count() or 2) - 1))
    with mp.get_context("spawn").Pool(workers) as pool:
        for m in MODELS:
            got, berr = api.forecast_batch(list(Y), lib.make_options(m, 1))
            assert berr["ok"], (m, berr)
            ref = np.concatenate(pool.map(_check_chunk, [(tests_dir, c, m) for c in chunks]))
            pts = np.array([g["point"][0] if g["ok"] else np.nan for g in got])
            assert all(g["ok"] for g in got), m
            assert _rel(pts, ref) <= REL_TOL, (m, _rel(pts, ref))


def test_batch_company_does_not_matter(env):
    """The full batch equals a shuffled sub-batch bit for bit; sharding over listed devices changes nothing."""
    api, O, lib, synth = env
    series, valids = _parity_batch(synth, n=300, seed=4402)
    rng = np.random.default_rng(9)
    sub = rng.permutation(len(series))[:113]
    L = lib.load()
    for m in MODELS:
        opts = lib.make_options(m, 7)
        full, _ = api.forecast_batch(series, opts, valids)
        part, _ = api.forecast_batch([series[s] for s in sub], opts, [valids[s] for s in sub])
        for j, s in enumerate(sub):
            assert part[j]["ok"] == full[s]["ok"] and part[j]["code"] == full[s]["code"], (m, s)
            if full[s]["ok"]:
                for k in ("point", "lower", "upper"):
                    assert np.array_equal(part[j][k], full[s][k]), (m, s, k)
        L.anofox_hip_set_min_series_per_device(16)
        try:
            lib.set_devices([0, 0, 0])
            shard, berr = api.forecast_batch(series, opts, valids)
            assert berr["ok"]
        finally:
            lib.set_devices([])
            L.anofox_hip_set_min_series_per_device(2048)
        for s in range(len(series)):
            assert shard[s]["ok"] == full[s]["ok"] and shard[s]["code"] == full[s]["code"], (m, s)
            if full[s]["ok"]:
                for k in ("point", "lower", "upper"):
                    assert np.array_equal(shard[s][k], full[s][k]), (m, s, k)


def test_device_resident_batch_equals_the_host_entry(env):
    import torch
    from anofox_forecast_amd.device import DeviceBatch
    api, O, lib, synth = env
    n, T, h = 200, 300, 9
    rng = np.random.default_rng(12)
    Y = synth.gen_series(synth.SEED_M5, 3000, n, T, 7, positive=False)
    lens = rng.integers(3, T + 1, n).astype(np.int32)
    Y[::17] = 0.0
    series = [Y[s, :lens[s]] for s in range(n)]
    for m in MODELS:
        opts = lib.make_options(m, h)
        host, berr = api.forecast_batch(series, opts)
        assert berr["ok"]
        b = DeviceBatch(n, T, opts, "cuda:0")
        try:
            block = torch.zeros((T, b.ld), dtype=torch.float64, device="cuda:0")
            block[:, :n] = torch.from_numpy(np.ascontiguousarray(Y.T)).to("cuda:0")
            ln = torch.zeros(b.ld, dtype=torch.int32, device="cuda:0")
            ln[:n] = torch.from_numpy(lens).to("cuda:0")
            b.set_block(block, ln)
            b.run()
            torch.cuda.synchronize()
            r = b.results()
            out = {k: r[k].cpu().numpy().reshape(n, -1) if k in ("yhat", "lower", "upper") else r[k].cpu().numpy() for k in ("yhat", "lower", "upper", "status")}
            assert b.stats()
        finally:
            b.close()
        for s in range(n):
            assert host[s]["ok"] and out["status"][s] == 0, (m, s)
            assert np.array_equal(out["yhat"][s], host[s]["point"]), (m, s)
            assert np.array_equal(out["lower"][s], host[s]["lower"]) and np.array_equal(out["upper"][s], host[s]["upper"]), (m, s)


def test_auto_detect_equals_the_non_seasonal_call(env):
    """params := MAP{} (seasonal period 0, detection on) runs the models as one group: the same results as detection off; an
    explicit period > 1 is InvalidInput (the models are non-seasonal)."""
    api, O, lib, synth = env
    Y = synth.gen_series(synth.SEED_M5, 500, 400, 210, 7, positive=False)
    series = list(Y)
    for m in MODELS:
        a, ea = api.forecast_batch(series, lib.make_options(m, 14, seasonal_period=0, auto_detect=True))
        b, eb = api.forecast_batch(series, lib.make_options(m, 14, seasonal_period=0, auto_detect=False))
        assert ea["ok"] and eb["ok"]
        for s in range(len(series)):
            assert a[s]["ok"] and b[s]["ok"]
            for k in ("point", "lower", "upper"):
                assert np.array_equal(a[s][k], b[s][k]), (m, s, k)
        r = api.forecast_series(Y30, lib.make_options(m, 3, seasonal_period=7, auto_detect=False))
        assert not r["ok"] and r["code"] == lib.INVALID_INPUT and f"Model '{m}' does not use seasonal_period" in r["message"]
        r = api.forecast_series([1.0, 0.0], lib.make_options(m, 3))
        assert not r["ok"] and r["code"] == lib.INSUFFICIENT_DATA


ALIASES = {"CrostonClassic": ("crostonclassic", "croston_classic", "croston"), "CrostonSBA": ("crostonsba", "croston_sba", "sba"),
           "ADIDA": ("adida",), "IMAPA": ("imapa",), "TSB": ("tsb",)}


def test_sql_replay_intermittent(env):
    """test/sql/ts_forecast_intermittent.test for the five models, through the mirrors of _ts_forecast, ts_forecast_agg,
    _ts_forecast_scalar and ts_forecast_by."""
    api, O, lib, synth = env
    for m in MODELS:
        for name in (m,) + ALIASES[m]:
            assert api.forecast_series(Y12, lib.make_options(name, 3))["model_name"] == m, name
        for h in (3, 5, 50):
            r = api.forecast_series(Y12, lib.make_options(m, h))
            assert r["ok"] and len(r["point"]) == h and np.all(r["point"] == r["point"][0])
            assert r["point"][0] > 0 and np.all(r["lower"] <= r["point"]) and np.all(r["point"] <= r["upper"])
        r = api.forecast_series(Y12, lib.make_options(m, 3, include_fitted=True, include_residuals=True))
        assert len(r["fitted"]) == 12 and len(r["residuals"]) == 12 and r["mse"] >= 0
    tabs = KATS["tables"]
    day = np.timedelta64(1, "D")
    start = np.datetime64(tabs["start"], "us")

    def dates(rows):
        return start + np.arange(rows) * day
    sparse = _table(tabs["sparse_demand"], np.arange(tabs["sparse_demand"]["rows"]))
    for m in MODELS:
        r = api.forecast_series(sparse, lib.make_options(m, 5, include_fitted=True, include_residuals=True))
        assert r["ok"] and len(r["fitted"]) == 40 and len(r["residuals"]) == 40
    # ts_forecast_agg on intermittent_data and grouped_intermittent
    idata = tabs["intermittent_data"]
    iv = _table(idata, np.arange(idata["rows"]))
    g = tabs["grouped_intermittent"]
    gi = np.arange(g["rows"])
    g_grp = np.array(["P1"] * g["rows"] + ["P2"] * g["rows"], dtype=object)
    g_ds = np.concatenate([dates(g["rows"])] * 2)
    g_y = np.concatenate([_table(g["groups"]["P1"], gi), _table(g["groups"]["P2"], gi)])
    for m in MODELS:
        agg = api.ts_forecast_agg(np.array(["x"] * idata["rows"], dtype=object), dates(idata["rows"]), iv, m, 5, {})
        assert agg["x"]["model_name"] == m and len(agg["x"]["point_forecast"]) == 5 and np.isfinite(agg["x"]["point_forecast"][0])
        ga = api.ts_forecast_agg(g_grp, g_ds, g_y, m, 5, {})
        assert sorted(ga) == ["P1", "P2"] and all(len(ga[k]["point_forecast"]) == 5 and ga[k]["model_name"] == m for k in ga)
        assert ga["P1"]["point_forecast"][0] != ga["P2"]["point_forecast"][0], m
        # the scalar route (one chunk, one batch) and the table operator on the sparse and regular tables
        sc = api.ts_forecast_scalar([dates(40), dates(12)], [sparse, Y12], 4, "1d", m, {})
        assert all(row is not None and len(row["yhat"]) == 4 and list(row["model_name"]) == [m] * 4 for row in sc)
        assert sc[1]["yhat"][0] == api.forecast_series(Y12, lib.make_options(m, 4))["point"][0]
        reg = _table(tabs["regular_data"], np.arange(tabs["regular_data"]["rows"]))
        for vals in (sparse, reg):
            rows = len(vals)
            out = api.ts_forecast_by(np.array(["s"] * rows, dtype=object), dates(rows), vals, m, 6, "1d", {})
            assert len(out["yhat"]) == 6 and list(out["model_name"]) == [m] * 6 and np.all(np.isfinite(out["yhat"]))
            assert np.all((out["yhat_lower"] <= out["yhat"]) & (out["yhat"] <= out["yhat_upper"]))
