"""GPU: sample paths simulated from fitted AutoARIMA models -- anofox_hip_batch_arima_fit_device,
anofox_hip_arima_innovations_device, anofox_hip_arima_paths_device, anofox_hip_batch_arima_paths, their device.py / api.py mirrors --
against the pure-Python restatement tests/arima_paths_ref.py.  The contract (DESIGN.md section 3 "ARIMA paths") is equality of bits:
the draws are counter-based, log, sin and cos are the library's own deterministic ones, every step is plain fp64 in a fixed order, so
every comparison is == on the bit patterns unless a test says otherwise; only the payload of a NaN is exempt.  Fits:
tests/arima_paths_cases.py (hand-set, no fit needed), and real AutoARIMA batches."""
import ctypes as C
import os

import numpy as np
import pytest

import arima_cases as X
import arima_paths_cases as K
import arima_paths_ref as AP
import arima_ref as A
import paths_ref as P

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
MODES = {"gaussian": (AP.GAUSSIAN, False), "own": (AP.BOOTSTRAP, False), "joint": (AP.BOOTSTRAP, True)}
N_PATHS = (1, 3, 17)                    # below, inside and beyond the four waves of a workgroup


@pytest.fixture(scope="module")
def env(hiplib, oracle):
    import torch
    assert torch.cuda.is_available()
    L = hiplib.load()
    from anofox_forecast_amd import api, device, synth
    return {"torch": torch, "L": L, "lib": hiplib, "api": api, "device": device, "synth": synth, "dev": torch.device("cuda:0")}


def _assert_bits(got, want, what):
    same = P.same_bits(got, want)
    assert same.all(), f"{what}: {int((~same).sum())} cells differ, first at {np.argwhere(~same)[0].tolist()}"


def _dev(env, a):
    return env["torch"].from_numpy(np.array(a, order="C")).to(env["dev"])           # (a copy: the cases' arrays are read-only)


def _inn(env, b):
    """device.arima_innovations_block on a hand-set batch -> tensors."""
    return env["device"].arima_innovations_block(_dev(env, b["orders"]), _dev(env, b["coef"]), _dev(env, b["y"]), _dev(env, b["lengths"]), b["m"],
                                                 n_series=b["n"])


def _paths(env, b, h, n_paths, mode, seed, resid=None, rl=None, sigma=None, pool_rows=0, pad=3, orders=None, coef=None, y=None):
    """device.arima_paths_block on a hand-set batch into a sentinel-filled block of n + pad columns, and the restatement, both on the
    restatement's residuals (or the given ones) -> (got paths, status, n_broken, want paths, status, n_broken)."""
    torch = env["torch"]
    innovations, joint = MODES[mode]
    wres, wrl, wsig = K.innovations(b)
    resid = wres if resid is None else resid
    rl, sigma = wrl if rl is None else rl, wsig if sigma is None else sigma
    orders, coef, y = (b["orders"] if orders is None else orders), (b["coef"] if coef is None else coef), (b["y"] if y is None else y)
    n, ld = b["n"], b["ld"]
    rblock = np.full((K.T_ROWS, ld), np.nan)
    rblock[:, :n] = resid
    out = torch.full((n_paths * h, n + pad), SENTINEL, dtype=torch.float64, device=env["dev"])
    g = env["device"].arima_paths_block(orders=_dev(env, orders), coef=_dev(env, coef), y=_dev(env, y), lengths=_dev(env, b["lengths"]),
                                        resid=_dev(env, rblock), resid_lengths=_dev(env, rl), sigma=_dev(env, sigma), m=b["m"], horizon=h,
                                        n_paths=n_paths, innovations="gaussian" if innovations == AP.GAUSSIAN else "bootstrap", joint=joint,
                                        pool_rows=pool_rows, seed=seed, n_series=n, out=out)
    torch.cuda.synchronize()
    want = AP.paths(orders, coef, y, b["lengths"], resid, rl, sigma, b["m"], n_paths, h, innovations, joint=joint, pool_rows=pool_rows, seed=seed,
                    n_series=n)
    got = g["paths"].cpu().numpy()
    assert (got[:, n:] == SENTINEL).all(), "columns beyond n_series were touched"
    return (got[:, :n], g["status"].cpu().numpy(), g["n_broken"].cpu().numpy()) + want


def _seed(m, h, n):
    return (m * 1000003 + h * 10007 + n) | (0xBADC0DE << 32)            # both key words in use


def _joint_rows(b):
    """The smallest nu among the series that have a model."""
    rl = K.innovations(b)[1]
    return int(rl[rl > 0].min())


# --------------------------------------------------------------------------------------------
# the innovations and the paths of hand-set fits
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", range(K.CHUNKS))
@pytest.mark.parametrize("m", K.PERIODS)
def test_innovations_equal_the_restatement(env, m, c):
    """Every combination of orders (972 over the eight chunks) at every period; at m = 2 and 4 seasonal and ordinary lags collide.
    Ragged lengths with nu = 1 and nu = 0 (no model) in every chunk."""
    b = K.batch(m, K.chunk_combos(c), seed=c)
    want, wrl, wsig = K.innovations(b)
    assert (wrl == 0).any() and (wrl == 1).any() and (wrl > 1).any() and np.isfinite(wsig[wrl > 0]).all()
    g = _inn(env, b)
    env["torch"].cuda.synchronize()
    n = b["n"]
    assert g["resid_lengths"].cpu().numpy().tolist() == wrl.tolist()
    _assert_bits(g["sigma"].cpu().numpy(), wsig, f"sigma m={m} chunk {c}")
    got = g["resid"].cpu().numpy()
    _assert_bits(got[:, :n], want, f"resid m={m} chunk {c}")
    assert np.isnan(got[:, n:]).all()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("m", K.PERIODS)
def test_paths_of_every_order_combination_equal_the_restatement(env, m, mode):
    """The eight chunks of a period in one mode.  EVERY chunk -- every order combination -- runs the long horizon 2 m + 6, at which
    every AR and MA lag and the seasonal integration read simulated values back from the rings; the shorter horizons 1, m - 1 and m
    walk from chunk to chunk beside it.  The number of paths (1, 3, 17) walks on its own index, so it does not move with the horizon.
    Series without a model (nu = 0) have NaN paths on both sides; every other path is whole."""
    hs = K.horizons(m)
    long, short = hs[-1], hs[:-1]
    assert long == 2 * m + 6
    for c in range(K.CHUNKS):
        b = K.batch(m, K.chunk_combos(c), seed=c)
        pool_rows = _joint_rows(b) if mode == "joint" else 0
        for h, n_paths in ((long, N_PATHS[c % 3]), (short[c % len(short)], N_PATHS[(c // len(short) + 1) % 3])):
            got, st, nb, want, wst, wnb = _paths(env, b, h, n_paths, mode, _seed(m, h, c), pool_rows=pool_rows)
            what = f"m={m} chunk {c} h={h} paths={n_paths} {mode}"
            assert set(wst.tolist()) == {AP.OK, AP.NO_MODEL} and not np.isnan(want[:, wst == AP.OK]).any(), what
            assert st.tolist() == wst.tolist() and nb.tolist() == wnb.tolist(), what
            _assert_bits(got, want, what)


@pytest.mark.parametrize("mode", list(MODES))
def test_period_beyond_the_horizon_and_one_series(env, mode):
    """m = 12, h = 5: no lag reaches a simulated value and no ring wraps; and a batch of one series."""
    b = K.batch(12, K.chunk_combos(3), seed=40)
    got, st, nb, want, wst, wnb = _paths(env, b, 5, 3, mode, _seed(12, 5, 0), pool_rows=_joint_rows(b) if mode == "joint" else 0)
    assert st.tolist() == wst.tolist() and nb.tolist() == wnb.tolist()
    _assert_bits(got, want, f"m=12 h=5 {mode}")
    one = K.batch(7, [(2, 1, 1, 1, 1, 1, 1)], seed=41)
    assert K.innovations(one)[1][0] > 1
    got, st, nb, want, wst, wnb = _paths(env, one, 20, 17, mode, _seed(7, 20, 1), pool_rows=_joint_rows(one) if mode == "joint" else 0)
    assert st.tolist() == wst.tolist() == [AP.OK] and nb.tolist() == wnb.tolist() == [0]
    _assert_bits(got, want, f"one series {mode}")


def test_two_runs_and_every_launch_shape_give_the_same_bits(env):
    """The developer knob arima_paths_waves of ANOFOX_HIP_TUNE forces the waves per workgroup; the bits do not depend on it."""
    b = K.batch(4, K.chunk_combos(5), seed=50)
    runs = []
    old = os.environ.get("ANOFOX_HIP_TUNE")
    try:
        for waves in (0, 0, 1, 2, 3, 4):
            os.environ["ANOFOX_HIP_TUNE"] = f"arima_paths_waves={waves}"
            runs.append(_paths(env, b, 14, 17, "gaussian", 99))
    finally:
        if old is None:
            os.environ.pop("ANOFOX_HIP_TUNE", None)
        else:
            os.environ["ANOFOX_HIP_TUNE"] = old
    _assert_bits(runs[0][0], runs[0][3], "the restatement")
    for r in runs[1:]:
        assert np.array_equal(r[0].view(np.uint64), runs[0][0].view(np.uint64)) and r[1].tolist() == runs[0][1].tolist()


@pytest.mark.parametrize("m,h", [(7, 28), (12, 24), (24, 48), (52, 26), (168, 48), (1, 64)])
def test_accepted_period_and_horizon_pairs_run(env, m, h):
    """The (m, h) pairs the ring limit must admit, on a seasonal model that reads every lag it has: T_ROWS observations do not
    hold two seasonal lags of the long periods, so those take P = Q = 0 and D = 0 where they must."""
    long = 2 * m + 10 > K.T_ROWS
    combo = (2, 1, 0, 0, 1, 0 if m + 10 > K.T_ROWS else 1, 1) if long else (2, 1, 2, 2, 1, 1, 1)
    b = K.batch(m, [combo], seed=60)
    got, st, nb, want, wst, wnb = _paths(env, b, h, 3, "own", _seed(m, h, 2))
    assert st.tolist() == wst.tolist() == [AP.OK] and nb.tolist() == wnb.tolist() == [0]
    _assert_bits(got, want, f"m={m} h={h}")


@pytest.mark.parametrize("m,h,combo", [(168, 64, (2, 1, 0, 0, 1, 0, 1)), (8, 12, (2, 1, 2, 2, 1, 1, 1))])
def test_launch_at_the_lds_limit(env, m, h, combo):
    """Exactly 65,536 bytes of dynamic LDS: one wave of 128 rows (m = 168, h = 64, the ring limit itself) and four waves of 32 rows
    (m = 8, h = 12), 17 paths."""
    rows = AP.lds_rows(m, h)
    assert rows in (128, 32) and (AP.MAX_LDS_ROWS // rows) * rows * 512 == 65536
    b = K.batch(m, [combo] * 3, seed=61)
    got, st, nb, want, wst, wnb = _paths(env, b, h, 17, "gaussian", _seed(m, h, 3))
    assert st.tolist() == wst.tolist() and AP.OK in wst.tolist() and nb.tolist() == wnb.tolist()
    assert not np.isnan(want[:, wst == AP.OK]).any()
    _assert_bits(got, want, f"m={m} h={h}: {rows} LDS rows")


# --------------------------------------------------------------------------------------------
# statuses and broken paths
# --------------------------------------------------------------------------------------------
def test_statuses_precedence_and_broken_paths(env):
    """tests/arima_paths_cases.py status_scenario: bad orders, NaN in a coefficient, in sigma, in the tails of y and of the residuals,
    a joint pool that is too short, a path that overflows; all of it ordinary arithmetic."""
    h, n_paths = 9, 3
    sc = K.status_scenario()
    b, spoiled = sc["batch"], {k: sc[k] for k in ("orders", "coef", "y", "resid", "rl", "sigma")}
    for mode in MODES:
        got, st, nb, want, wst, wnb = _paths(env, b, h, n_paths, mode, 7, pool_rows=sc["joint_rows"] if mode == "joint" else 0, **spoiled)
        K.check_status_scenario(sc, mode, wst, wnb, want, n_paths)
        assert st.tolist() == wst.tolist() and nb.tolist() == wnb.tolist(), mode
        _assert_bits(got, want, mode)
    # precedence: NO_MODEL before RAGGED before NAN; and a pool of no rows
    got, st, nb, want, wst, wnb = _paths(env, b, h, n_paths, "joint", 7, pool_rows=int(sc["rl"].max()) + 1, **spoiled)
    assert st.tolist() == wst.tolist() and set(wst.tolist()) == {AP.NO_MODEL, AP.RAGGED}
    got, st, nb, want, wst, wnb = _paths(env, b, h, n_paths, "joint", 7, pool_rows=0)
    assert st.tolist() == wst.tolist() and set(wst.tolist()) == {AP.NO_MODEL, AP.EMPTY} and np.isnan(got).all()


# --------------------------------------------------------------------------------------------
# a real AutoARIMA batch: fit state, chain, downstream entries
# --------------------------------------------------------------------------------------------
def _real_series(env, m, n=70, T=84):
    syn = env["synth"]
    Y = syn.gen_series(syn.SEED_M5, 9100 + m, n, T, max(m, 2))
    series = [Y[s, : T - (s % 9)].copy() for s in range(n)]
    series[3], series[11], series[20], series[33] = series[3][:0], series[11][:1], series[20][:2], series[33][:3]
    series[40] = np.full(50, 3.0)
    return series


@pytest.fixture(scope="module", params=[1, 7])
def real(env, request):
    """One AutoARIMA DeviceBatch per period, run once: handle, host readback, forecasts."""
    from anofox_forecast_amd.device import DeviceBatch
    lib, api, torch = env["lib"], env["api"], env["torch"]
    m, h = request.param, 10
    series = _real_series(env, m)
    n, T = len(series), max(len(y) for y in series)
    opts = lib.make_options("AutoARIMA", h, seasonal_period=m)
    b = DeviceBatch(n, T, opts, "cuda:0")
    Y = np.zeros((T, b.ld))
    lens = np.zeros(b.ld, dtype=np.int32)
    for s, y in enumerate(series):
        Y[: len(y), s], lens[s] = y, len(y)
    b.set_block(_dev(env, Y), _dev(env, lens))
    b.run()
    torch.cuda.synchronize()
    fits = (lib.AnofoxHipArimaFit * n)()
    err = lib.AnofoxError()
    assert b.L.anofox_hip_batch_arima_fit(b.handle, fits, C.byref(err)), err.message
    recs = [api.arima_fit_record(f) for f in fits]
    res = {k: v.cpu().numpy().copy() for k, v in b.results().items()}
    yield dict(batch=b, m=max(m, 1), h=h, n=n, T=T, Y=Y, lens=lens, series=series, recs=recs, res=res, opts=opts)
    b.close()


def test_device_fit_state_equals_the_host_readback(env, real):
    """Field for field, with series whose fit failed (no observation, one, two and three of them).  The other way to have no fit,
    status 0 with a model_code below 1000000, is test_a_batch_on_the_fallback_chain_has_no_fit_state_and_no_paths."""
    recs, n = real["recs"], real["n"]
    assert sum(r["status"] != 0 for r in recs) >= 3, "no series whose fit failed"
    assert sum(r["status"] == 0 and r["model_code"] >= 1000000 for r in recs) >= n - 8
    d = real["batch"].arima_fit_device()
    assert d["m"] == real["m"]
    orders, coef = d["orders"].cpu().numpy(), d["coef"].cpu().numpy()
    for s, r in enumerate(recs):
        assert orders[:, s].tolist() == [r[k] for k in env["lib"].ARIMA_FIT_ORDER_ROWS], (s, orders[:, s], r)
        want = np.concatenate([r["phi"], r["theta"], r["Phi"], r["Theta"], [r["constant"], r["aicc"]]])
        _assert_bits(coef[:, s], want, f"coef of series {s}")


def test_a_batch_on_the_fallback_chain_has_no_fit_state_and_no_paths(env):
    """An AutoARIMA batch is run, then given regressors and run again on the same handle: the ARIMAX route forecasts every series with
    status 0 and a model_code below 1000000 and leaves the search state of the first run where it was.  Nothing of that state may
    come back: the device blocks equal the host readback (zero orders, NaN in every double), and the chain gives NO_MODEL and NaN
    paths for every series."""
    from anofox_forecast_amd.device import DeviceBatch
    lib, api, torch, device, L = env["lib"], env["api"], env["torch"], env["device"], env["L"]
    n, T, h, m = 20, 60, 6, 7
    syn = env["synth"]
    series = syn.gen_series(syn.SEED_M5, 9300, n, T, m, positive=True)
    b = DeviceBatch(n, T, lib.make_options("AutoARIMA", h, seasonal_period=m), "cuda:0")
    try:
        Y, lens = np.zeros((T, b.ld)), np.zeros(b.ld, dtype=np.int32)
        Y[:, :n], lens[:n] = series.T, T
        b.set_block(_dev(env, Y), _dev(env, lens))
        b.run()
        torch.cuda.synchronize()
        first = b.arima_fit_device()
        assert int((first["orders"][7, :n] > 0).sum()) >= n - 2             # the first run leaves real fits in the search state
        rng = np.random.default_rng(93)
        b.set_exog(_dev(env, rng.standard_normal((1, T, b.ld))), _dev(env, rng.standard_normal((1, h, b.ld))))
        b.run()
        torch.cuda.synchronize()
        fits = (lib.AnofoxHipArimaFit * n)()
        err = lib.AnofoxError()
        assert b.L.anofox_hip_batch_arima_fit(b.handle, fits, C.byref(err)), err.message
        recs = [api.arima_fit_record(f) for f in fits]
        assert all(r["status"] == 0 and r["model_code"] < 1000000 for r in recs), [(r["status"], r["model_code"]) for r in recs]
        d = b.arima_fit_device()
        orders, coef = d["orders"].cpu().numpy(), d["coef"].cpu().numpy()
        for s, r in enumerate(recs):
            assert orders[:, s].tolist() == [r[k] for k in lib.ARIMA_FIT_ORDER_ROWS] == [0] * 8, (s, orders[:, s], r)
            want = np.concatenate([r["phi"], r["theta"], r["Phi"], r["Theta"], [r["constant"], r["aicc"]]])
            assert np.isnan(want).all() and np.isnan(coef[:, s]).all(), (s, coef[:, s], want)
        for mode, (innovations, joint) in MODES.items():
            name = "gaussian" if innovations == AP.GAUSSIAN else "bootstrap"
            g = device.arima_paths_block(b, n_paths=3, innovations=name, joint=joint, seed=4)
            torch.cuda.synchronize()
            assert g["status"].cpu().numpy().tolist() == [AP.NO_MODEL] * n and g["n_broken"].cpu().numpy().tolist() == [3] * n, mode
            assert np.isnan(g["paths"].cpu().numpy()[:, :n]).all(), mode
            o = lib.make_arima_paths_options(name, joint, 4)
            al = np.array([0.5])
            q, qs, ss, nb = np.zeros((1, n, h)), np.full(n, -1, dtype=np.int32), np.full(n, -1, dtype=np.int32), np.full(n, -1, dtype=np.int32)
            paths = np.zeros((3 * h, b.ld))
            ld = C.c_size_t()
            assert L.anofox_hip_batch_arima_paths(b.handle, C.byref(o), C.sizeof(o), 3, al.ctypes.data, 1, b.ld, q.ctypes.data, qs.ctypes.data,
                                                  ss.ctypes.data, nb.ctypes.data, paths.ctypes.data, C.byref(ld), C.byref(err)), err.message
            assert ss.tolist() == [AP.NO_MODEL] * n and nb.tolist() == [3] * n and qs.tolist() == [P.NAN] * n, mode
            assert np.isnan(paths[:, :n]).all() and np.isnan(q).all(), mode
    finally:
        b.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_every_entry_gives_the_restatement_of_the_real_fit(env, real, mode):
    """The three single entries, anofox_hip_batch_arima_paths, device.arima_paths_block(batch) and api.arima_paths_batch give the same
    bits; the quantiles are paths_ref.quantiles of the reference paths."""
    torch, device, api, lib, L = env["torch"], env["device"], env["api"], env["lib"], env["L"]
    innovations, joint = MODES[mode]
    b, n, h, m, T, n_paths, levels = real["batch"], real["n"], real["h"], real["m"], real["T"], 17, [0.1, 0.5, 0.9]
    d = b.arima_fit_device()
    orders, coef = d["orders"].cpu().numpy(), d["coef"].cpu().numpy()
    Y, lens = real["Y"], real["lens"]
    wres, wrl, wsig = AP.innovations(orders, coef, Y, lens, m, n_series=n)
    inn = device.arima_innovations_block(d["orders"], d["coef"], _dev(env, Y), _dev(env, lens), m, n_series=n)
    torch.cuda.synchronize()
    assert inn["resid_lengths"].cpu().numpy().tolist() == wrl.tolist()
    _assert_bits(inn["resid"].cpu().numpy()[:, :n], wres, "resid of the real fit")
    _assert_bits(inn["sigma"].cpu().numpy(), wsig, "sigma of the real fit")
    fitted = np.array([r["status"] == 0 and r["model_code"] >= 1000000 for r in real["recs"]])
    assert ((wrl > 0) == fitted).all()
    pool_rows = int(wrl[wrl > 0].min()) if joint else 0
    want, wst, wnb = AP.paths(orders, coef, Y, lens, wres, wrl, wsig, m, n_paths, h, innovations, joint=joint, pool_rows=pool_rows, seed=2027, n_series=n)
    assert ((wst == AP.OK) == fitted).all() and (wst[~fitted] == AP.NO_MODEL).all() and (wnb[fitted] == 0).all()
    wq, wqs = P.quantiles(want, h, n_paths, levels)
    name = "gaussian" if innovations == AP.GAUSSIAN else "bootstrap"
    for run in range(2):
        g = device.arima_paths_block(b, n_paths=n_paths, innovations=name, joint=joint, seed=2027)
        torch.cuda.synchronize()
        assert g["status"].cpu().numpy().tolist() == wst.tolist() and g["n_broken"].cpu().numpy().tolist() == wnb.tolist() and g["pool_rows"] == pool_rows
        _assert_bits(g["paths"].cpu().numpy()[:, :n], want, f"arima_paths_block(batch) {mode} run {run}")
    o = lib.make_arima_paths_options(name, joint, 2027)
    al = np.array(levels)
    ld, err = C.c_size_t(), lib.AnofoxError()
    assert L.anofox_hip_batch_arima_paths(b.handle, C.byref(o), C.sizeof(o), n_paths, al.ctypes.data, 3, 0, None, None, None, None, None,
                                          C.byref(ld), C.byref(err)) and ld.value == b.ld
    q, qs, ss, nb = np.full((3, n, h), np.nan), np.full(n, -1, dtype=np.int32), np.full(n, -1, dtype=np.int32), np.full(n, -1, dtype=np.int32)
    paths = np.full((n_paths * h, b.ld), np.nan)
    assert L.anofox_hip_batch_arima_paths(b.handle, C.byref(o), C.sizeof(o), n_paths, al.ctypes.data, 3, b.ld, q.ctypes.data, qs.ctypes.data,
                                          ss.ctypes.data, nb.ctypes.data, paths.ctypes.data, C.byref(ld), C.byref(err)), err.message
    _assert_bits(paths[:, :n], want, f"anofox_hip_batch_arima_paths {mode}")
    _assert_bits(q, wq, f"anofox_hip_batch_arima_paths quantiles {mode}")
    assert qs.tolist() == wqs.tolist() and ss.tolist() == wst.tolist() and nb.tolist() == wnb.tolist()
    res, rerr = api.arima_paths_batch(real["series"], real["opts"], levels, n_paths=n_paths, innovations=name, joint=joint, seed=2027, want_paths=True)
    assert rerr["ok"], rerr
    _assert_bits(res["paths"][:, :n], want, f"api.arima_paths_batch {mode}")
    _assert_bits(res["quantiles"], wq, f"api.arima_paths_batch quantiles {mode}")
    assert res["status"].tolist() == wqs.tolist() and res["series_status"].tolist() == wst.tolist() and res["n_broken"].tolist() == wnb.tolist()


def test_zero_residuals_give_the_batch_forecast(env, real):
    """Zero innovations: every path is the point forecast.  The residual block is also the MA history of the model, so it cannot be
    zeroed without changing the forecast of a model with q + Q > 0; the drawn innovations are made zero through sigma = 0 in the
    Gaussian mode instead, and the history stays the fit's own.  The batch's yhat comes from arima_forecast_kernel, whose arithmetic
    is fused, so this is a tolerance: arima_ref.FORECAST_REL + arima_paths_ref.FORECAST_REL relative to max |y|, both taken against
    the same 80-bit yardstick."""
    torch, device = env["torch"], env["device"]
    b, n, h, m = real["batch"], real["n"], real["h"], real["m"]
    d = b.arima_fit_device()
    inn = device.arima_innovations_block(d["orders"], d["coef"], _dev(env, real["Y"]), _dev(env, real["lens"]), m, n_series=n)
    rl = inn["resid_lengths"].cpu().numpy()
    g = device.arima_paths_block(orders=d["orders"], coef=d["coef"], y=_dev(env, real["Y"]), lengths=_dev(env, real["lens"]),
                                 resid=inn["resid"], resid_lengths=inn["resid_lengths"], sigma=torch.zeros_like(inn["sigma"]), m=m, horizon=h,
                                 n_paths=3, innovations="gaussian", seed=1, n_series=n)
    torch.cuda.synchronize()
    got, st = g["paths"].cpu().numpy()[:, :n].reshape(3, h, n), g["status"].cpu().numpy()
    tol = A.FORECAST_REL + AP.FORECAST_REL
    worst, checked = 0.0, 0
    for s in range(n):
        if rl[s] == 0:
            assert st[s] == AP.NO_MODEL
            continue
        assert st[s] == AP.OK
        scale = float(np.max(np.abs(real["series"][s]))) or 1.0
        dev =float(np.max(np.abs(got[:, :, s] - real["res"]["yhat"][s][None, :]))) / scale
        worst, checked = max(worst, dev), checked + 1
    print(f"m={m}: {checked} series, worst deviation of a zero-innovation path from yhat {worst:.3e} (rel. max |y|), tolerance {tol:.3e}")
    assert checked >= n - 8 and worst <= tol, (worst, tol)


def test_quantile_and_hierarchy_entries_take_the_block_as_it_lies(env, real):
    torch, device = env["torch"], env["device"]
    b, n, h, n_paths, levels = real["batch"], real["n"], real["h"], 9, [0.05, 0.5, 0.95]
    g = device.arima_paths_block(b, n_paths=n_paths, innovations="gaussian", seed=5)
    q = device.path_quantiles_block(g["paths"], levels, horizon=h, n_paths=n_paths, n_cols=n)
    torch.cuda.synchronize()
    block = g["paths"].cpu().numpy()[:, :n]
    wq, wqs = P.quantiles(block, h, n_paths, levels)
    _assert_bits(q["quantiles"].cpu().numpy(), wq, "quantiles of the block")
    assert q["status"].cpu().numpy().tolist() == wqs.tolist()
    rows = torch.full((g["paths"].shape[1],), n_paths * h, dtype=torch.int32, device=env["dev"])
    a = device.aggregate_block(g["paths"], rows, _dev(env, np.zeros((1, n), dtype=np.int32)), n_series=n, t_out=n_paths * h)
    total = np.zeros(n_paths * h)
    for s in range(n):                                                  # the serial sum in plan order
        total = total + block[:, s]
    _assert_bits(a["y"].cpu().numpy()[:, 0], total, "the total of the paths")


def test_ts_forecast_quantiles_by_with_arima_model_paths(env):
    api, synth, lib = env["api"], env["synth"], env["lib"]
    n, T, h, m, n_paths = 5, 70, 6, 7, 50
    Y = synth.gen_series(synth.SEED_M5, 0, n, T, m, positive=True)
    days = np.datetime64("2024-01-01") + np.arange(T)
    group = [f"g{s}" for t in range(T) for s in range(n)]
    date = np.array([days[t] for t in range(T) for s in range(n)])
    target = np.array([Y[s, t] for t in range(T) for s in range(n)])
    levels = [0.1, 0.5, 0.9]
    params = {"seasonal_period": m}
    base = api.ts_forecast_quantiles_by(group, date, target, "AutoARIMA", h, "1d", levels, residual_folds=4, n_paths=n_paths, seed=3, params=params)
    info = {}
    out = api.ts_forecast_quantiles_by(group, date, target, "AutoARIMA", h, "1d", levels, n_paths=n_paths, seed=3, params=params,
                                       paths="model_gaussian", info=info)
    assert list(out) == list(base)
    for c in ("forecast_step", "yhat", "yhat_lower", "yhat_upper"):
        assert np.asarray(out[c]).tobytes() == np.asarray(base[c]).tobytes(), c
    assert list(out["model_name"]) == list(base["model_name"]) and list(out["id"]) == list(base["id"])
    opts = api.options_from_bind(api.bind("AutoARIMA", h, "1d", params))
    recs = api.arima_fit_batch(list(Y), opts)
    assert all(r["ok"] and r["model_code"] >= 1000000 for r in recs)
    orders, coef = AP.blocks_of([X.fit_from_record(r, m) for r in recs], n, np.full(n, T), m)
    resid, rl, sigma = AP.innovations(orders, coef, Y.T, np.full(n, T), m)
    want, wst, wnb = AP.paths(orders, coef, Y.T, np.full(n, T), resid, rl, sigma, m, n_paths, h, AP.GAUSSIAN, seed=3)
    assert (wst == AP.OK).all() and (wnb == 0).all()
    wq, _ = P.quantiles(want, h, n_paths, levels)
    for l, c in enumerate(("q0.1", "q0.5", "q0.9")):
        _assert_bits(np.asarray(out[c]).reshape(n, h), wq[l], c)
    assert (np.asarray(out["paths_status"]) == 0).all() and info["n_broken"].tolist() == [0] * n
    with pytest.raises(api.InvalidInputException, match="must be ETS or AutoETS"):
        api.ts_forecast_quantiles_by(group, date, target, "Naive", h, "1d", levels, paths="model_bootstrap")
