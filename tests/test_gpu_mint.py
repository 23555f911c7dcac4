"""GPU: MinT with the shrinkage covariance -- anofox_hip_reconcile_mint_factor_device, anofox_hip_reconcile_mint_apply_device,
anofox_hip_reconcile_mint_batch, device.reconcile_mint_block and api.ts_reconcile_hierarchy(method="mint_shrink") -- against the
yardsticks of tests/mint_ref.py.  The contract (DESIGN.md section 3 "MinT-shrink"): the variances equal the serial chain bit for
bit; the intensity lies within 16 x the larger of the fp64 Gram route's own relative deviation from the dense pairwise formula in
long double and eps; the forecasts lie within 16 x the larger of the plain fp64 constraint form's deviation from the long-double
projection with the dense W and eps * max|yhat| (bounds computed on the CPU when the test runs); the output is coherent to the bit;
every entry, both layouts of the forecast block and both layouts of the residual block give the same bits."""
import ctypes as C

import numpy as np
import pytest

import hierarchy_ref as HR
import mint_cases as MC
import mint_ref as MR
import reconcile_cases as RC
import reconcile_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
WORST = {}                                                # "lambda" / "y" -> the worst deviation / allowance seen (printed by the last test)


@pytest.fixture(scope="module")
def env(hiplib):
    import torch
    assert torch.cuda.is_available()
    L = hiplib.load()
    from anofox_forecast_amd import api, device
    return {"torch": torch, "L": L, "lib": hiplib, "api": api, "device": device, "dev": torch.device("cuda:0")}


def _up(env, a):
    return env["torch"].from_numpy(np.ascontiguousarray(a)).to(env["dev"])


def _plan(env, name):
    return env["device"].reconcile_plan_device(MC.case(name)["column_of"], device=env["dev"])


def _same(a, b):
    return bool(HR.same_bits(np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)).all())


def _block(env, name, block=None, residuals=None, series_major=True, res_series_major=True, shrinkage=None, factor=None, plan=None):
    """device.reconcile_mint_block on a sentinel-filled output; returns (y [n_out, rows] on the host, status, result dict)."""
    torch = env["torch"]
    c = MC.case(name)
    yhat = c["yhat"] if block is None else block
    res = c["residuals"] if residuals is None else residuals
    src = yhat if series_major else RC.time_major(yhat, fill=SENTINEL)
    rsrc = res if res_series_major else RC.time_major(res, pad=3, fill=float("nan"))      # (a padding column that was read would poison the sums)
    out = torch.full(src.shape, SENTINEL, dtype=torch.float64, device=env["dev"])
    r = env["device"].reconcile_mint_block(_up(env, src), _up(env, rsrc), _plan(env, name) if plan is None else plan, shrinkage=shrinkage,
                                           series_major=series_major, residuals_series_major=res_series_major, factor=factor, out=out)
    torch.cuda.synchronize()
    y = r["y"].cpu().numpy()
    if not series_major:
        assert (y[:, c["n_out"]:] == SENTINEL).all(), "the padding columns were written"
        y = y[:, :c["n_out"]].T
    return np.ascontiguousarray(y), r["row_status"].cpu().numpy(), r


@pytest.mark.parametrize("name", MC.names())
def test_case_against_the_yardsticks(env, name):
    c, p = MC.case(name), MC.parts(name)
    part = MR.participants(p)
    y, status, r = _block(env, name)
    assert (status == 0).all()
    # the variances: equality of bits with the serial chain
    v = r["variances"].cpu().numpy()
    assert (v[part] == MC.variances(name)[part]).all() and _same(v[part], MC.variances(name)[part])
    # the intensity
    dense, gram, lam_tol = MC.shrinkage(name)
    lam = r["shrinkage"]
    print(f"{name}: lambda {lam!r} dense {dense!r} deviation {abs(lam - dense):.3e} allowance {lam_tol:.3e}")
    WORST["lambda"] = max(WORST.get("lambda", 0.0), abs(lam - dense) / lam_tol)
    # the forecasts
    yard, tol = MC.yardstick(name)
    dev = float(np.max(np.abs(y[part] - yard[part])))
    print(f"{name}: deviation {dev:.3e} allowance {tol:.3e} ratio {dev / tol:.3f}")
    WORST["y"] = max(WORST.get("y", 0.0), dev / tol)
    assert R.coherent_to_the_bit(p, y).all(), "an aggregate is not the chain over the output's bottoms"
    for e in MC.empty_columns(name):
        assert _same(y[e], c["yhat"][e])
    assert abs(lam - dense) <= lam_tol, (name, lam, dense, lam_tol)
    assert dev <= tol, (name, dev, tol)
    # the same bits: the four layout combinations, a second run, the passed-in estimate, the batch entry
    for series_major in (True, False):
        for res_series_major in (True, False):
            y2, s2, r2 = _block(env, name, series_major=series_major, res_series_major=res_series_major)
            assert _same(y2, y) and (s2 == 0).all() and r2["shrinkage"] == lam and _same(r2["variances"].cpu().numpy()[part], v[part])
    y3, _s, r3 = _block(env, name, shrinkage=lam)
    assert _same(y3, y) and r3["shrinkage"] == lam
    out, err = env["api"].reconcile_mint_batch(c["column_of"], c["yhat"], c["residuals"])
    assert err["ok"], err
    assert _same(out["y"], y) and (out["row_status"] == 0).all() and out["shrinkage"] == lam and _same(out["variances"][part], v[part])
    # one factor bundle applied to a second block == a factor of that block's own
    other = c["yhat"] * 1.5 + 2.0
    a, _s, _r = _block(env, name, block=other, factor=r["factor"], plan=r["plan"])
    b, _s, _r = _block(env, name, block=other)
    assert _same(a, b)


@pytest.mark.parametrize("name", ["leaf1_twice-3", "small-7", "agg65-64", "agg129-128", "agg197-200"])
def test_factor_against_the_exact_matrix(env, name):
    """L L^T against M assembled in long double from the returned variances and intensity; E against the residuals' incoherence; the
    strict upper part and the padding of ld_a and ld_e keep their sentinels; two runs give the same bits."""
    torch, L, lib = env["torch"], env["L"], env["lib"]
    c, p = MC.case(name), MC.parts(name)
    na, n_res = len(p["agg_cols"]), c["n_res"]
    plan = _plan(env, name)
    ld_a, ld_e = na + 3, na + 2
    res = _up(env, c["residuals"])
    sizes = lib.reconcile_mint_sizes(n_res, na, 1)
    got = []
    for _ in range(2):
        f = torch.full((na, ld_a), SENTINEL, dtype=torch.float64, device=env["dev"])
        e = torch.full((n_res, ld_e), SENTINEL, dtype=torch.float64, device=env["dev"])
        v = torch.full((c["n_out"],), SENTINEL, dtype=torch.float64, device=env["dev"])
        gram = torch.empty(sizes["gram"], dtype=torch.float64, device=env["dev"])
        lam, err = C.c_double(-1.0), lib.AnofoxError()
        ok = L.anofox_hip_reconcile_mint_factor_device(res.data_ptr(), n_res, 1, n_res, plan["col_offsets"].data_ptr(), plan["members"].data_ptr(),
                                                       plan["n_out"], plan["nnz"], plan["n_series"], plan["bottom_col"].data_ptr(),
                                                       plan["agg_cols"].data_ptr(), na, plan["leaf_offsets"].data_ptr(), plan["leaf_aggs"].data_ptr(),
                                                       plan["n_leaf"], float("nan"), v.data_ptr(), e.data_ptr(), ld_e, f.data_ptr(), ld_a,
                                                       gram.data_ptr(), C.byref(lam), None, C.byref(err))
        assert ok, err.message
        got.append((f.cpu().numpy(), e.cpu().numpy(), v.cpu().numpy(), lam.value))
    for k in range(3):
        assert _same(got[0][k], got[1][k])
    F, E, v, lam = got[0]
    assert lam == got[1][3] and (v[MC.empty_columns(name)] == 0.0).all()
    upper = np.triu_indices(na, 1)
    assert (F[:, :na][upper] == SENTINEL).all() and (F[:, na:] == SENTINEL).all() and (E[:, na:] == SENTINEL).all()
    want_e = MR.incoherence(p, c["residuals"])
    assert np.allclose(E[:, :na], want_e, rtol=0.0, atol=64 * MC.EPS * float(np.max(np.abs(c["residuals"]))) * max(len(m) for m in p["cols"]))
    Lf = np.tril(F[:, :na]).astype(np.longdouble)
    M = MR.system_matrix(p, c["residuals"], lam, v, np.longdouble)
    plain = np.linalg.cholesky(M.astype(np.float64)).astype(np.longdouble)
    noise = float(np.max(np.abs(plain @ plain.T - M)))
    tol = 16.0 * max(noise, MC.EPS * float(np.max(np.abs(M))))
    dev = float(np.max(np.abs(Lf @ Lf.T - M)))
    print(f"{name}: factor deviation {dev:.3e} allowance {tol:.3e}")
    assert dev <= tol


def test_update_variants_agree(env, monkeypatch):
    """The plain-FMA tile and the MFMA tile of the E^T E update (the developer knob reconcile_mint_ete of ANOFOX_HIP_TUNE, read at
    every factor call): both results lie within the allowance, each the same bits on a second run -- what
    test_trailing_update_variants_agree asks of the trailing update."""
    name = "agg197-200"
    yard, tol = MC.yardstick(name)
    part = MR.participants(MC.parts(name))
    for variant in ("0", "1"):
        monkeypatch.setenv("ANOFOX_HIP_TUNE", f"reconcile_mint_ete={variant}")
        y, _s, _r = _block(env, name)
        y2, _s, _r = _block(env, name)
        dev = float(np.max(np.abs(y[part] - yard[part])))
        print(f"E^T E variant {variant}: deviation {dev:.3e} allowance {tol:.3e}")
        assert dev <= tol and _same(y, y2)


@pytest.mark.parametrize("name", ["small-7", "agg65-64", "agg197-196"])
def test_intensity_one_is_wls_var_with_the_variances(env, name):
    c, p = MC.case(name), MC.parts(name)
    part = MR.participants(p)
    y, status, r = _block(env, name, shrinkage=1.0)
    assert r["shrinkage"] == 1.0 and (status == 0).all()
    v = r["variances"].cpu().numpy()
    w = np.where(v > 0.0, v, 1.0)
    out = env["torch"].full(c["yhat"].shape, SENTINEL, dtype=env["torch"].float64, device=env["dev"])
    ref = env["device"].reconcile_block(_up(env, c["yhat"]), _plan(env, name), "wls_var", weights=_up(env, w), out=out)
    env["torch"].cuda.synchronize()
    _yard, tol = R.allowance(p, w, c["yhat"])
    dev = float(np.max(np.abs(y[part] - ref["y"].cpu().numpy()[part])))
    print(f"{name}: lambda 1 against wls_var: deviation {dev:.3e} allowance {tol:.3e}")
    assert dev <= tol and R.coherent_to_the_bit(p, y).all()


@pytest.mark.parametrize("name", ["small-7", "agg65-64"])
def test_bad_residuals_are_refused_by_column_and_bad_forecast_rows_marked(env, name):
    torch = env["torch"]
    c, p = MC.case(name), MC.parts(name)
    part = MR.participants(p)
    agg, bottom = p["agg_cols"][-1], p["bottom_col"][1]
    for res_series_major in (True, False):
        for col, value, text in ((agg, np.nan, f"a residual of column {agg} is not finite"), (bottom, np.inf, f"a residual of column {bottom} is not finite"),
                                 (bottom, 0.0, f"the residual variance of column {bottom} is not finite and positive")):
            res = c["residuals"].copy()
            if value == 0.0:
                res[col, :] = 0.0
            else:
                res[col, c["n_res"] - 1] = value
            rsrc = res if res_series_major else RC.time_major(res, pad=3, fill=float("nan"))
            out = torch.full(c["yhat"].shape, SENTINEL, dtype=torch.float64, device=env["dev"])
            with pytest.raises(RuntimeError, match=text):
                env["device"].reconcile_mint_block(_up(env, c["yhat"]), _up(env, rsrc), _plan(env, name), residuals_series_major=res_series_major, out=out)
            torch.cuda.synchronize()
            assert (out.cpu().numpy() == SENTINEL).all(), "a refused call wrote to out"
    both = c["residuals"].copy()                                  # two bad columns: the smallest is named
    both[agg, 0], both[bottom, 1] = np.nan, np.nan
    with pytest.raises(RuntimeError, match=f"a residual of column {min(agg, bottom)} is not finite"):
        env["device"].reconcile_mint_block(_up(env, c["yhat"]), _up(env, both), _plan(env, name))
    res = c["residuals"].copy()                                   # an empty column is never read: NaN there changes nothing
    for e in MC.empty_columns(name):
        res[e, :] = np.nan
    clean, _s, _r = _block(env, name)
    y, status, _r = _block(env, name, residuals=res)
    assert _same(y, clean) and (status == 0).all()
    out, err = env["api"].reconcile_mint_batch(c["column_of"], c["yhat"], both)
    assert not err["ok"] and err["code"] == 3 and f"column {min(agg, bottom)}" in err["message"] and np.isnan(out["y"]).all()
    # a forecast row that is not finite: status 2 for that row alone
    block, bad = RC.with_nonfinite(c["plan"])
    good = [t for t in range(c["rows"]) if t not in bad]
    for series_major in (True, False):
        y, status, _r = _block(env, name, block=block, series_major=series_major)
        assert status.tolist() == [2 if t in bad else 0 for t in range(c["rows"])]
        assert np.isnan(y[part][:, bad]).all() and _same(y[part][:, good], clean[part][:, good])
        for e in MC.empty_columns(name):
            assert _same(y[e], block[e])


def test_chain_aggregate_forecast_backtest_reconcile_score(env):
    """aggregate_block -> DeviceBatch forecasts -> backtest_block over the aggregated block -> reconcile_mint_block on `yhat` and
    `error` as they lie -> score_block: no copy to the host in between; the result against mint_ref."""
    torch, device, lib, api, dev = env["torch"], env["device"], env["lib"], env["api"], env["dev"]
    n, T, h, n_folds = 24, 40, 3, 3                              # 24 leaves, 6 stores of 4, total: 31 columns, 7 aggregates, 9 residual rows
    s = np.arange(n)
    column_of = np.array([np.zeros(n), 1 + s // 4, 7 + s], dtype=np.int32)
    rng = np.random.default_rng(23)
    y = np.zeros((T, 64))
    y[:, :n] = rng.uniform(1.0, 30.0, size=(T, n)) + 4.0 * rng.standard_normal((T, 1)) + np.linspace(0.0, 5.0, T)[:, None]
    lengths = np.zeros(64, dtype=np.int32)
    lengths[:n] = T
    agg = device.aggregate_block(torch.from_numpy(y).to(dev), torch.from_numpy(lengths).to(dev), torch.from_numpy(column_of).to(dev), n_series=n)
    n_out, t_out = agg["n_out"], agg["t_out"]
    assert (n_out, t_out) == (31, T)
    plan = device.reconcile_plan_device(column_of, device=dev)
    _n, offs, memb = HR.plan(column_of.tolist())
    p = R.parts(offs, memb, n)
    part = MR.participants(p)
    folds = api.backtest_fold_bounds(T, h, n_folds)
    F = len(folds)
    for model in ("Naive", "SES"):
        opts = lib.make_options(model, h)
        b = device.DeviceBatch(n_out, t_out, opts, dev)
        b.set_block(agg["y"], agg["lengths"])
        b.run()
        res = b.results()
        bt = device.backtest_block(agg["y"], agg["lengths"], opts, folds, n_series=n_out)
        error = bt["error"][:n_out * F].view(n_out, F * h)       # series-major [n_out, n_res] as it lies
        rec = device.reconcile_mint_block(res["yhat"], error, plan)
        score, status = device.score_block(res["yhat"], rec["y"], "mae", n_groups=n_out)
        torch.cuda.synchronize()
        yr, base, resid = rec["y"].cpu().numpy()[:n_out], res["yhat"].cpu().numpy()[:n_out], error.cpu().numpy()
        mae = score.cpu().numpy()[:n_out]
        assert (rec["row_status"].cpu().numpy() == 0).all() and (status.cpu().numpy()[:n_out] == 0).all()
        b.close()
        bt["batch"].close()
        assert np.isfinite(resid).all() and R.coherent_to_the_bit(p, yr).all()
        assert _same(rec["variances"].cpu().numpy()[part], MR.variance_chain(p, resid)[part])
        dense = float(MR.shrinkage_dense(p, resid)[0])
        gram = MR.shrinkage_gram(p, resid)
        assert abs(rec["shrinkage"] - dense) <= 16.0 * max(abs(gram - dense), MC.EPS * max(dense, MC.EPS))
        yard = MR.project_longdouble(p, MR.dense_w(p, resid, dense), base) if dense > 0 else None
        if yard is not None:
            noise = float(np.max(np.abs(MR.constraint_fp64(p, resid, gram, base)[part] - yard[part])))
            tol = 16.0 * max(noise, MC.EPS * float(np.max(np.abs(base[part]))))
            assert float(np.max(np.abs(yr[part] - yard[part]))) <= tol
        want = np.array([np.mean(np.abs(base[c, :h] - yr[c, :h])) for c in range(n_out)])
        assert np.allclose(mae, want, rtol=1e-12, atol=1e-300)


def test_mirror_end_to_end(env):
    """ts_reconcile_hierarchy(method="mint_shrink") on a three-level table of a dozen leaves with a residual table, against mint_ref."""
    api = env["api"]
    rng = np.random.default_rng(5)
    leaves = [(f"R{k // 6}", f"S{k // 3}", f"i{k}") for k in range(12)]
    keys = sorted({HR.build_unique_id(list(l), lv) for l in leaves for lv in range(4)}, key=lambda u: u.encode())
    days = np.array(["2024-03-01", "2024-03-02", "2024-03-03"], dtype="datetime64[D]")
    past = np.array(["2024-02-01"], dtype="datetime64[D]") + np.arange(20)
    uid = [u for u in keys for _ in days]
    date = np.array([d for _ in keys for d in days])
    fc = rng.uniform(5.0, 50.0, size=len(uid))
    common = rng.standard_normal(len(past))
    resid = np.array([(0.7 * common + rng.standard_normal(len(past))) * (1.0 + 3.0 * rng.uniform()) for _ in keys])
    r_uid = [u for u in keys for _ in past]
    r_date = np.array([d for _ in keys for d in past])
    order, r_order = rng.permutation(len(uid)), rng.permutation(len(r_uid))          # the rows may arrive in any order
    info = {}
    got = api.ts_reconcile_hierarchy([uid[i] for i in order], date[order], fc[order],
                                     {"method": "mint_shrink", "residuals": ([r_uid[i] for i in r_order], r_date[r_order], resid.reshape(-1)[r_order])},
                                     info=info)
    assert list(got["unique_id"]) == uid and (got["date"] == date).all() and (info["row_status"] == 0).all()
    co = info["column_of"]
    _n, offs, memb = HR.plan(co.tolist())
    p = R.parts(offs, memb, 12)
    part = MR.participants(p)
    block = fc.reshape(len(keys), 3)
    dense = float(MR.shrinkage_dense(p, resid)[0])
    gram = MR.shrinkage_gram(p, resid)
    assert 0.0 < dense < 1.0 and abs(info["shrinkage"] - dense) <= 16.0 * max(abs(gram - dense), MC.EPS * dense)
    assert _same(info["variances"][part], MR.variance_chain(p, resid)[part])
    yard = MR.project_longdouble(p, MR.dense_w(p, resid, dense), block)
    tol = 16.0 * max(float(np.max(np.abs(MR.constraint_fp64(p, resid, gram, block) - yard))), MC.EPS * float(np.max(np.abs(block))))
    y = got["forecast"].reshape(len(keys), 3)
    assert R.coherent_to_the_bit(p, y).all() and float(np.max(np.abs(y - yard))) <= tol
    direct, err = api.reconcile_mint_batch(co, block, resid)
    assert err["ok"] and _same(direct["y"], y) and direct["shrinkage"] == info["shrinkage"]
    fixed = api.ts_reconcile_hierarchy(uid, date, fc, {"method": "mint_shrink", "residuals": (r_uid, r_date, resid.reshape(-1)), "shrinkage": 0.25}, info=info)
    assert info["shrinkage"] == 0.25
    yard = MR.project_longdouble(p, MR.dense_w(p, resid, 0.25), block)
    tol = 16.0 * max(float(np.max(np.abs(MR.constraint_fp64(p, resid, 0.25, block) - yard))), MC.EPS * float(np.max(np.abs(block))))
    assert float(np.max(np.abs(fixed["forecast"].reshape(len(keys), 3) - yard))) <= tol
    ols = api.ts_reconcile_hierarchy(uid, date, fc, {"method": "ols"})           # every other method as before
    assert R.coherent_to_the_bit(p, ols["forecast"].reshape(len(keys), 3)).all()


def test_worst_ratio_is_reported():
    print("worst deviation / allowance:", {k: round(v, 4) for k, v in WORST.items()})
    assert all(v <= 1.0 for v in WORST.values())
