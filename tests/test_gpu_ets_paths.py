"""GPU: sample paths simulated from fitted ETS models -- anofox_hip_batch_inspect_device, anofox_hip_ets_innovations_device,
anofox_hip_ets_paths_device, anofox_hip_batch_ets_paths, their device.py / api.py mirrors -- against the pure-Python restatement
tests/ets_paths_ref.py.  The contract (DESIGN.md section 3 "Model paths") is equality of bits: the draws are counter-based, log, sin,
cos and pow are the library's own deterministic ones, every step is plain fp64 in a fixed order, so every comparison is == on the bit
patterns; only the payload of a NaN is exempt.  Records: tests/ets_paths_cases.py (no fit needed), and one real AutoETS fit."""
import ctypes as C

import numpy as np
import pytest

import ets_paths_cases as K
import ets_paths_ref as E
import inspect_ref as R
import paths_ref as P

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
MODES = {"gaussian": (E.GAUSSIAN, False), "own": (E.BOOTSTRAP, False), "joint": (E.BOOTSTRAP, True)}
# csrc/ets_paths.hip ets_paths_waves: 64 KiB / (64 lanes x R x 8 bytes), at most 4 waves per workgroup --
# 4 waves up to R = 32, 3 up to 42, 2 up to 64, 1 up to 128
WAVE_EDGES = (32, 33, 42, 43, 64, 65, 128)


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


def _block(env, a, ld, fill=np.nan):
    """A [rows, n] array as a device block of ld columns; the padding columns hold `fill`, which nothing may read into a result."""
    a = np.asarray(a, dtype=np.float64)
    out = np.full((a.shape[0], ld), fill)
    out[:, : a.shape[1]] = a
    return env["torch"].from_numpy(out).to(env["dev"])


def _ints(env, a, ld):
    out = np.zeros(ld, dtype=np.int32)
    out[: len(a)] = a
    return env["torch"].from_numpy(out).to(env["dev"])


def _run(env, rec, m, h, n_paths, mode, pool=None, pool_lengths=None, seed=0, pad=0, pool_series_major=False):
    """device.ets_paths_block on hand-made records into a sentinel-filled block with `pad` extra columns, and the restatement.
    -> (got paths [P * h, ld_out], got status, got n_broken, want paths, want status, want n_broken)."""
    torch, device = env["torch"], env["device"]
    innovations, joint = MODES[mode]
    n = len(rec["spec"])
    ld = (n + 63) // 64 * 64
    t_pool = t_len = None
    if innovations == E.BOOTSTRAP:
        t_pool = torch.from_numpy(np.ascontiguousarray(pool.T)).to(env["dev"]) if pool_series_major else _block(env, pool, ld)
        t_len = None if pool_lengths is None else _ints(env, pool_lengths, ld)
    out = torch.full((n_paths * h, ld + pad), SENTINEL, dtype=torch.float64, device=env["dev"])
    g = device.ets_paths_block(spec=_ints(env, rec["spec"], ld), info=_block(env, rec["info"], ld), states=_block(env, rec["states"], ld),
                               lengths=_ints(env, rec["lengths"], ld), m=m, horizon=h, n_paths=n_paths,
                               innovations="gaussian" if innovations == E.GAUSSIAN else "bootstrap", pool=t_pool, pool_lengths=t_len,
                               pool_series_major=pool_series_major, joint=joint, seed=seed, n_series=n, out=out)
    torch.cuda.synchronize()
    want = E.paths(rec["spec"], rec["info"], rec["states"], m, rec["lengths"], n_paths, h, innovations,
                   pool=pool if innovations == E.BOOTSTRAP else None, pool_lengths=pool_lengths, joint=joint, seed=seed)
    return (g["paths"].cpu().numpy(), g["status"].cpu().numpy(), g["n_broken"].cpu().numpy()) + want


def _check(env, rec, m, h, n_paths, mode, what, whole=True, **kw):
    got, status, broken, want, wstatus, wbroken = _run(env, rec, m, h, n_paths, mode, **kw)
    n = len(rec["spec"])
    if whole:
        assert (wstatus == E.OK).all() and (wbroken == 0).all() and not np.isnan(want).any(), what      # nothing hides behind NaN == NaN
    assert status.tolist() == wstatus.tolist(), what
    assert broken.tolist() == wbroken.tolist(), what
    _assert_bits(got[:, :n], want, what)
    assert (got[:, n:] == SENTINEL).all(), f"{what}: columns beyond n_series were touched"
    return got, want


def _seed(m, h, n):
    return (m * 1000003 + h * 10007 + n) | (0xBADC0DE << 32)            # both key words in use


# --------------------------------------------------------------------------------------------
# the kernels against the restatement
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("h", [1, 3, 6, 9])
@pytest.mark.parametrize("m", [1, 4, 7])
def test_all_specs_equal_the_restatement(env, m, h, mode):
    """130 series (two full tiles and a tile of 2), every spec five times and mixed within each wave, ragged lengths (different phases
    in one wave), 5 paths (more than the four waves of a workgroup), a block wider than the series; h below, equal to and above the
    period, ending inside a Philox block and inside a word pair."""
    n, n_paths = 130, 5
    rec = K.records(n, m, seed=m * 16 + h)
    assert set(rec["spec"].tolist()) == set(K.SPEC_IDS) and len(set((rec["lengths"] % max(m, 2)).tolist())) > 1
    pool = K.pool(rec, 11, seed=h)
    _check(env, rec, m, h, n_paths, mode, f"m={m} h={h} {mode}", pool=pool, seed=_seed(m, h, n), pad=64)


@pytest.mark.parametrize("mode", list(MODES))
def test_tile_edges_and_path_counts(env, mode):
    m, h = 4, 6
    for n, n_paths in ((2, 1), (63, 3), (64, 1), (65, 3), (64, 5)):
        rec = K.records(n, m, seed=n)
        _check(env, rec, m, h, n_paths, mode, f"n={n} P={n_paths} {mode}", pool=K.pool(rec, 9, seed=n), seed=_seed(m, h, n), pad=3)


def test_pool_layouts_lengths_and_statuses(env):
    m, h, n_paths, n, rows = 4, 6, 3, 70, 12
    rec = K.records(n, m, seed=21)
    pool = K.pool(rec, rows, seed=4)
    lens = (3 + np.arange(n) % (rows - 2)).astype(np.int32)              # every pool shorter than pool_rows
    lens[7] = rows + 5                                                   # cut to pool_rows
    for sm in (False, True):                                             # both pool layouts give the restatement's bits
        _check(env, rec, m, h, n_paths, "own", f"pool_series_major={sm}", pool=pool, pool_lengths=lens, seed=8, pool_series_major=sm)
    # statuses and their precedence
    rec = K.records(n, m, seed=22, notation="MAdM")
    pool = K.pool(rec, rows, seed=5)
    lens = np.full(n, rows, dtype=np.int32)
    rec["spec"][0] = R.spec_id("MAN") + 1                                # "MAA": none of the 25
    rec["spec"][1] = -1
    rec["lengths"][2] = 0                                                # no observation
    lens[0] = 0                                                          # NO_MODEL comes before EMPTY
    lens[3] = 0                                                          # EMPTY
    lens[4], pool[2, 4] = 5, np.nan                                      # a NaN among the first `length` rows: NAN
    lens[5], pool[9, 5] = 5, np.nan                                      # ... beyond them: fine
    rec["info"][2, 6] = np.nan                                           # gamma, read by MAdM: NAN
    rec["info"][5, 8] = np.nan                                           # aicc: not read
    rec["states"][1, 9] = np.nan                                         # growth: NAN
    got, status, broken, want, wstatus, wbroken = _run(env, rec, m, h, n_paths, "own", pool=pool, pool_lengths=lens, seed=9)
    assert wstatus[:10].tolist() == [E.NO_MODEL, E.NO_MODEL, E.NO_MODEL, E.EMPTY, E.NAN, E.OK, E.NAN, E.OK, E.OK, E.NAN]
    assert status.tolist() == wstatus.tolist() and broken.tolist() == wbroken.tolist()
    assert (wbroken[wstatus != E.OK] == n_paths).all() and (wbroken[wstatus == E.OK] == 0).all()
    _assert_bits(got[:, :n], want, "statuses (own rows)")
    # joint: a length other than pool_rows is RAGGED, before EMPTY and NAN; after NO_MODEL
    got, status, broken, want, wstatus, wbroken = _run(env, rec, m, h, n_paths, "joint", pool=pool, pool_lengths=lens, seed=9)
    assert wstatus[:10].tolist() == [E.NO_MODEL, E.NO_MODEL, E.NO_MODEL, E.RAGGED, E.RAGGED, E.RAGGED, E.NAN, E.OK, E.OK, E.NAN]
    assert status.tolist() == wstatus.tolist() and broken.tolist() == wbroken.tolist()
    _assert_bits(got[:, :n], want, "statuses (joint)")
    # Gaussian: a NaN sse is a NaN sigma
    rec["info"][7, 10] = np.nan
    got, status, broken, want, wstatus, wbroken = _run(env, rec, m, h, n_paths, "gaussian", seed=9)
    assert wstatus[:11].tolist() == [E.NO_MODEL, E.NO_MODEL, E.NO_MODEL, E.OK, E.OK, E.OK, E.NAN, E.OK, E.OK, E.NAN, E.NAN]
    assert status.tolist() == wstatus.tolist() and broken.tolist() == wbroken.tolist()
    _assert_bits(got[:, :n], want, "statuses (Gaussian)")


def test_broken_paths(env):
    """The hand-made AMdN record of the CPU test: NaN from the step on whose growth is not positive, counted in n_broken."""
    info = np.full((8, 2), np.nan)
    states = np.full((3, 2), np.nan)
    info[0], info[1], info[3], info[7] = 0.3, 0.3, 0.9, 40.0
    states[0], states[1] = 10.0, 1.0
    rec = {"spec": np.array([R.spec_id("AMdN")] * 2, dtype=np.int32), "info": info, "states": states, "lengths": np.array([40, 41], dtype=np.int32)}
    pool = np.stack([np.full(6, -50.0), np.full(6, 0.25)], axis=1)
    got, want = _check(env, rec, 1, 6, 5, "own", "broken paths", whole=False, pool=pool, seed=1)
    cube = got[:, :2].reshape(5, 6, 2)
    assert (cube[:, 0, 0] == -40.0).all() and np.isnan(cube[:, 1:, 0]).all() and np.isfinite(cube[:, :, 1]).all()


@pytest.mark.parametrize("ring", WAVE_EDGES)
def test_lds_edges(env, ring):
    """R = min(m, h) on either side of every change in the waves of a workgroup, and the largest one; h = R + 1 wraps the ring once."""
    n, n_paths = 65, 5
    rec = K.records(n, ring, seed=ring)
    for mode in ("gaussian", "own"):
        _check(env, rec, ring, ring + 1, n_paths, mode, f"R={ring} {mode}", pool=K.pool(rec, 7, seed=ring), seed=_seed(ring, ring + 1, n))
    if ring == 128:                                                     # a longer period with the horizon as R
        rec = K.records(n, 300, seed=3)
        _check(env, rec, 300, 128, 2, "own", "m=300 h=128", pool=K.pool(rec, 7, seed=1), seed=5)


def test_ring_above_the_limit_is_the_named_error(env):
    rec = K.records(3, 129, seed=1)
    with pytest.raises(ValueError, match=r"R = min\(m, horizon\) = 129 exceeds the limit of 128"):
        _run(env, rec, 129, 129, 2, "gaussian")


# --------------------------------------------------------------------------------------------
# through a real fit
# --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fit(env):
    """A 64-series synthetic batch, AutoETS at m = 7: the batch, its host inspection and the restatement's inputs from it."""
    torch, device, lib, synth = env["torch"], env["device"], env["lib"], env["synth"]
    n, T, h, m = 64, 98, 9, 7
    Y = synth.gen_series(synth.SEED_M5, 0, n, T, m, positive=True)
    opts = lib.make_options("AutoETS", h, seasonal_period=m)
    y = torch.from_numpy(device.pack_time_major(Y)).to(env["dev"])
    lens = torch.full((y.shape[1],), T, dtype=torch.int32, device=env["dev"])
    b = device.DeviceBatch(n, T, opts, env["dev"])
    b.set_block(y, lens)
    b.run()
    torch.cuda.synchronize()
    insp = (lib.AnofoxHipInspection * n)()
    fitted = np.full((n, T), 7.0)
    seas = np.full((n, m), np.nan)
    err = lib.AnofoxError()
    assert b.L.anofox_hip_batch_inspect(b.handle, insp, fitted.ctypes.data, seas.ctypes.data, m, C.byref(err)), err.message
    res = b.results()
    code, status = res["model_code"].cpu().numpy(), res["status"].cpu().numpy()
    info = np.array([[getattr(insp[s], k) for s in range(n)] for k in ("alpha", "beta", "gamma", "phi", "aic", "aicc", "bic", "sse")])
    states = np.vstack([np.array([[insp[s].level for s in range(n)], [insp[s].trend for s in range(n)]]), seas.T])
    spec = np.where(status == 0, code - 100, -1).astype(np.int32)
    assert (status == 0).all() and all(E.spec_ok(v) for v in spec) and len(set(spec.tolist())) >= 2
    return {"batch": b, "Y": Y, "y": y, "lens": lens, "opts": opts, "n": n, "T": T, "h": h, "m": m, "info": info, "states": states,
            "fitted": fitted, "spec": spec, "lengths": np.full(n, T, dtype=np.int32)}


def test_inspect_device_equals_the_host_inspection(env, fit):
    b, n = fit["batch"], fit["n"]
    for want_fitted in (True, False):
        d = b.inspect_device(fitted=want_fitted)
        _assert_bits(d["info"].cpu().numpy()[:, :n], fit["info"], "info")
        _assert_bits(d["states"].cpu().numpy()[:, :n], fit["states"], "states")
        assert np.isnan(d["info"].cpu().numpy()[:, n:]).all() and d["m"] == fit["m"]
        assert d["spec"].cpu().numpy().tolist() == fit["spec"].tolist()
        if want_fitted:
            _assert_bits(d["fitted"].cpu().numpy()[:, :n], fit["fitted"].T, "fitted")
        else:
            assert d["fitted"] is None


def test_innovations_block_equals_the_subtraction(env, fit):
    device, n = env["device"], fit["n"]
    d = fit["batch"].inspect_device()
    inn = device.ets_innovations_block(fit["y"], d["fitted"], fit["lens"], d["spec"], n_series=n)
    env["torch"].cuda.synchronize()
    want, wlen = E.innovations(fit["Y"].T, fit["fitted"].T, fit["lengths"], fit["spec"])
    assert inn["pool_lengths"].cpu().numpy().tolist() == wlen.tolist() == [fit["T"]] * n
    _assert_bits(inn["pool"].cpu().numpy()[:, :n], want, "innovations")
    mul = fit["spec"] // 15 == 1
    y, f = fit["Y"].T, fit["fitted"].T
    _assert_bits(inn["pool"].cpu().numpy()[:, :n], np.where(mul[None, :], (y - f) / f, y - f), "innovations against the plain formula")


@pytest.mark.parametrize("mode", list(MODES))
def test_every_entry_gives_the_restatement_of_the_fit(env, fit, mode):
    torch, device, api, lib = env["torch"], env["device"], env["api"], env["lib"]
    innovations, joint = MODES[mode]
    n, h, m, n_paths, levels = fit["n"], fit["h"], fit["m"], 40, [0.1, 0.5, 0.9]
    pool = E.innovations(fit["Y"].T, fit["fitted"].T, fit["lengths"], fit["spec"])[0] if innovations == E.BOOTSTRAP else None
    want, wstatus, wbroken = E.paths(fit["spec"], fit["info"], fit["states"], m, fit["lengths"], n_paths, h, innovations, pool=pool,
                                     pool_lengths=None if pool is None else fit["lengths"], joint=joint, seed=2027)
    assert (wstatus == E.OK).all() and (wbroken == 0).all() and not np.isnan(want).any()
    wq, wqs = P.quantiles(want, h, n_paths, levels)
    name = "gaussian" if innovations == E.GAUSSIAN else "bootstrap"
    for run in range(2):                                                # ... and so does a second run
        g = device.ets_paths_block(fit["batch"], n_paths=n_paths, innovations=name, joint=joint, seed=2027)
        torch.cuda.synchronize()
        assert g["status"].cpu().numpy().tolist() == wstatus.tolist() and g["n_broken"].cpu().numpy().tolist() == wbroken.tolist()
        _assert_bits(g["paths"].cpu().numpy()[:, :n], want, f"ets_paths_block(batch) {mode} run {run}")
    # the C entry on the batch's handle
    L, b = env["L"], fit["batch"]
    o = lib.make_ets_paths_options(name, joint, 2027)
    al = np.array(levels)
    ld, err = C.c_size_t(), lib.AnofoxError()
    assert L.anofox_hip_batch_ets_paths(b.handle, C.byref(o), C.sizeof(o), n_paths, al.ctypes.data, 3, 0, None, None, None, None, None,
                                        C.byref(ld), C.byref(err)) and ld.value == b.ld
    q, qs, ss, nb = np.full((3, n, h), np.nan), np.full(n, -1, dtype=np.int32), np.full(n, -1, dtype=np.int32), np.full(n, -1, dtype=np.int32)
    paths = np.full((n_paths * h, b.ld), np.nan)
    assert L.anofox_hip_batch_ets_paths(b.handle, C.byref(o), C.sizeof(o), n_paths, al.ctypes.data, 3, b.ld, q.ctypes.data, qs.ctypes.data,
                                        ss.ctypes.data, nb.ctypes.data, paths.ctypes.data, C.byref(ld), C.byref(err)), err.message
    _assert_bits(paths[:, :n], want, f"anofox_hip_batch_ets_paths {mode}")
    _assert_bits(q, wq, f"anofox_hip_batch_ets_paths quantiles {mode}")
    assert qs.tolist() == wqs.tolist() and ss.tolist() == wstatus.tolist() and nb.tolist() == wbroken.tolist()
    # the host-buffer mirror fits the same series itself
    res, rerr = api.ets_paths_batch(list(fit["Y"]), fit["opts"], levels, n_paths=n_paths, innovations=name, joint=joint, seed=2027, want_paths=True)
    assert rerr["ok"], rerr
    _assert_bits(res["paths"][:, :n], want, f"api.ets_paths_batch {mode}")
    _assert_bits(res["quantiles"], wq, f"api.ets_paths_batch quantiles {mode}")
    assert res["status"].tolist() == wqs.tolist() and res["series_status"].tolist() == wstatus.tolist() and res["n_broken"].tolist() == wbroken.tolist()


# --------------------------------------------------------------------------------------------
# downstream as it lies
# --------------------------------------------------------------------------------------------
def test_quantile_and_hierarchy_entries_take_the_block_as_it_lies(env, fit):
    torch, device = env["torch"], env["device"]
    n, h, m, n_paths, levels = fit["n"], fit["h"], fit["m"], 33, [0.05, 0.5, 0.95]
    want, _, _ = E.paths(fit["spec"], fit["info"], fit["states"], m, fit["lengths"], n_paths, h, E.GAUSSIAN, seed=5)
    g = device.ets_paths_block(fit["batch"], n_paths=n_paths, innovations="gaussian", seed=5)
    q = device.path_quantiles_block(g["paths"], levels, horizon=h, n_paths=n_paths, n_cols=n)
    wq, wqs = P.quantiles(want, h, n_paths, levels)
    _assert_bits(q["quantiles"].cpu().numpy(), wq, "quantiles of the block")
    assert q["status"].cpu().numpy().tolist() == wqs.tolist()
    column_of = np.zeros((1, n), dtype=np.int32)                        # one total above the leaves
    rows = torch.full((g["paths"].shape[1],), n_paths * h, dtype=torch.int32, device=env["dev"])
    a = device.aggregate_block(g["paths"], rows, torch.from_numpy(column_of).to(env["dev"]), n_series=n, t_out=n_paths * h)
    total = np.zeros(n_paths * h)
    for s in range(n):                                                  # the serial sum in plan order
        total = total + want[:, s]
    _assert_bits(a["y"].cpu().numpy()[:, 0], total, "the total of the paths")


def test_ts_forecast_quantiles_by_with_model_paths(env):
    api, synth = env["api"], env["synth"]
    n, T, h, m, n_paths = 5, 70, 6, 7, 200
    Y = synth.gen_series(synth.SEED_M5, 0, n, T, m, positive=True)
    days = np.datetime64("2024-01-01") + np.arange(T)
    group = [f"g{s}" for t in range(T) for s in range(n)]
    date = np.array([days[t] for t in range(T) for s in range(n)])
    target = np.array([Y[s, t] for t in range(T) for s in range(n)])
    levels = [0.1, 0.5, 0.9]
    params = {"seasonal_period": m}
    base = api.ts_forecast_quantiles_by(group, date, target, "AutoETS", h, "1d", levels, residual_folds=4, n_paths=n_paths, seed=3, params=params)
    same = api.ts_forecast_quantiles_by(group, date, target, "AutoETS", h, "1d", levels, residual_folds=4, n_paths=n_paths, seed=3, params=params,
                                        paths="bootstrap")
    assert list(base) == list(same)
    for c in base:                                                      # without paths= nothing changes: the same bytes
        assert np.asarray(base[c]).tobytes() == np.asarray(same[c]).tobytes() if isinstance(base[c], np.ndarray) else list(base[c]) == list(same[c]), c
    info = {}
    out = api.ts_forecast_quantiles_by(group, date, target, "AutoETS", h, "1d", levels, n_paths=n_paths, seed=3, params=params,
                                       paths="model_gaussian", info=info)
    assert list(out) == list(base)
    for c in ("forecast_step", "yhat", "yhat_lower", "yhat_upper"):
        assert np.asarray(out[c]).tobytes() == np.asarray(base[c]).tobytes(), c
    assert list(out["model_name"]) == list(base["model_name"]) and list(out["id"]) == list(base["id"])
    # the quantile columns: the quantile restatement on the reference paths of the same fit
    opts = api.options_from_bind(api.bind("AutoETS", h, "1d", params))
    recs = api.inspect_batch(list(Y), opts)
    spec = np.array([r["model_code"] - 100 for r in recs], dtype=np.int32)
    info_rows = np.array([[r[k] for r in recs] for k in ("alpha", "beta", "gamma", "phi", "aic", "aicc", "bic", "sse")])
    states = np.vstack([np.array([[r["level"] for r in recs], [r["trend"] for r in recs]]), np.array([r["seasonal_states"] for r in recs]).T])
    want, wstatus, wbroken = E.paths(spec, info_rows, states, m, np.full(n, T), n_paths, h, E.GAUSSIAN, seed=3)
    assert (wstatus == E.OK).all() and (wbroken == 0).all()
    wq, _ = P.quantiles(want, h, n_paths, levels)
    for l, c in enumerate(("q0.1", "q0.5", "q0.9")):
        _assert_bits(np.asarray(out[c]).reshape(n, h), wq[l], c)
    assert (np.asarray(out["paths_status"]) == 0).all() and info["n_broken"].tolist() == [0] * n
    with pytest.raises(api.InvalidInputException, match="must be ETS or AutoETS"):
        api.ts_forecast_quantiles_by(group, date, target, "Naive", h, "1d", levels, paths="model_bootstrap")
