"""GPU: the reconciliation of hierarchy forecasts -- anofox_hip_reconcile_factor_device, anofox_hip_reconcile_apply_device,
anofox_hip_reconcile_batch, device.reconcile_block and api.ts_reconcile_hierarchy -- against the yardsticks of tests/reconcile_ref.py.
The contract (DESIGN.md section 3 "Reconciliation"): bottom_up is equality of bits with the serial chain; every method's output is
coherent to the bit (an aggregate == the chain over the output's own bottoms); ols / wls_struct / wls_var lie within 16 x the larger
of the plain fp64 evaluation's own deviation from the exact (or long-double) projection and eps * max|yhat|, a bound computed on the
CPU when the test runs; every entry and both layouts give the same bits."""
import ctypes as C

import numpy as np
import pytest

import hierarchy_ref as HR
import reconcile_cases as RC
import reconcile_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
SOLVED = ("ols", "wls_struct", "wls_var")
WORST = {}                                                # method -> the worst deviation / allowance seen (printed by the last test)


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
    c = RC.all_cases()[name]
    return env["device"].reconcile_plan_device(c["column_of"], device=env["dev"])


def _block(env, name, method, block=None, series_major=True, factor=None, plan=None):
    """device.reconcile_block on a sentinel-filled output; returns (y [n_out, rows] on the host, status, result dict)."""
    torch = env["torch"]
    c = RC.all_cases()[name]
    yhat = c["yhat"] if block is None else block
    src = yhat if series_major else RC.time_major(yhat, fill=SENTINEL)
    out = torch.full(src.shape, SENTINEL, dtype=torch.float64, device=env["dev"])
    r = env["device"].reconcile_block(_up(env, src), _plan(env, name) if plan is None else plan, method,
                                      weights=_up(env, c["weights"]) if method == "wls_var" else None, series_major=series_major,
                                      factor=factor, out=out)
    torch.cuda.synchronize()
    y = r["y"].cpu().numpy()
    if not series_major:
        assert (y[:, c["n_out"]:] == SENTINEL).all(), "the padding columns were written"
        y = y[:, :c["n_out"]].T
    return np.ascontiguousarray(y), r["row_status"].cpu().numpy(), r


def _same(a, b):
    return bool(HR.same_bits(np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)).all())


@pytest.mark.parametrize("name", RC.names())
def test_bottom_up_is_the_serial_chain_to_the_bit(env, name):
    c, p = RC.all_cases()[name], RC.plan_parts(name)
    want, _tol, _w = RC.yardstick(name, "bottom_up")
    for series_major in (True, False):
        y, status, r = _block(env, name, "bottom_up", series_major=series_major)
        assert r["factor"] is None and (status == 0).all()
        assert _same(y, want), (name, series_major)
        assert _same(y[p["bottom_col"]], c["yhat"][p["bottom_col"]])
    out, err = env["api"].reconcile_batch(c["column_of"], c["yhat"], "bottom_up")
    assert err["ok"], err
    assert _same(out["y"], want) and (out["row_status"] == 0).all()


@pytest.mark.parametrize("method", SOLVED)
@pytest.mark.parametrize("name", RC.names())
def test_solved_methods_against_the_yardstick(env, name, method):
    c, p = RC.all_cases()[name], RC.plan_parts(name)
    yard, tol, _w = RC.yardstick(name, method)
    part = RC.participants(name)
    y, status, r = _block(env, name, method)
    assert (status == 0).all()
    dev = float(np.max(np.abs(y[part] - yard[part])))
    print(f"{name} {method}: deviation {dev:.3e} allowance {tol:.3e} ratio {dev / tol:.3f}")
    WORST[method] = max(WORST.get(method, 0.0), dev / tol)
    assert R.coherent_to_the_bit(p, y).all(), "an aggregate is not the chain over the output's bottoms"
    for e in RC.empty_columns(name):
        assert _same(y[e], c["yhat"][e])
    assert dev <= tol, (name, method, dev, tol)
    # the same bits: the time-major layout, a second run, the batch entry, and one factor applied again
    y_tm, status_tm, _ = _block(env, name, method, series_major=False)
    assert _same(y_tm, y) and (status_tm == 0).all()
    y2, _s, _r = _block(env, name, method, factor=r["factor"], plan=r["plan"])
    assert _same(y2, y)
    out, err = env["api"].reconcile_batch(c["column_of"], c["yhat"], method, c["weights"] if method == "wls_var" else None)
    assert err["ok"], err
    assert _same(out["y"], y) and (out["row_status"] == 0).all()


@pytest.mark.parametrize("method", SOLVED)
@pytest.mark.parametrize("name", ["leaf1_twice", "small", "agg65", "agg129", "agg197"])
def test_factor_against_the_exact_matrix(env, name, method):
    """L L^T against M assembled exactly (in long double above 40 columns); the strict upper part and the padding of ld_a keep
    their sentinels; two runs give the same bits."""
    torch, L, lib = env["torch"], env["L"], env["lib"]
    c, p = RC.all_cases()[name], RC.plan_parts(name)
    w = R.method_weights(p, method, c["weights"])
    na = len(p["agg_cols"])
    plan = _plan(env, name)
    ld_a = na + 3
    got = []
    for _ in range(2):
        f = torch.full((na, ld_a), SENTINEL, dtype=torch.float64, device=env["dev"])
        wt = _up(env, w)
        err = lib.AnofoxError()
        ok = L.anofox_hip_reconcile_factor_device(plan["col_offsets"].data_ptr(), plan["members"].data_ptr(), plan["n_out"], plan["nnz"],
                                                  plan["n_series"], plan["bottom_col"].data_ptr(), plan["agg_cols"].data_ptr(), na,
                                                  plan["leaf_offsets"].data_ptr(), plan["leaf_aggs"].data_ptr(), plan["n_leaf"],
                                                  lib.RECONCILE_METHODS[method], None if method == "ols" else wt.data_ptr(), f.data_ptr(), ld_a,
                                                  None, C.byref(err))
        assert ok, err.message
        got.append(f.cpu().numpy())
    assert _same(got[0], got[1])
    F = got[0]
    upper = np.triu_indices(na, 1)
    assert (F[:, :na][upper] == SENTINEL).all() and (F[:, na:] == SENTINEL).all()
    Lf = np.tril(F[:, :na]).astype(np.longdouble)
    if c["n_out"] <= 40:
        M = np.array([[float(v) for v in row] for row in R.system_matrix_exact(p, w)], dtype=np.longdouble)
    else:
        M = R.system_matrix(p, w, np.longdouble)
    plain = np.linalg.cholesky(R.system_matrix(p, w)).astype(np.longdouble)
    noise = float(np.max(np.abs(plain @ plain.T - M)))
    tol = 16.0 * max(noise, np.finfo(np.float64).eps * float(np.max(np.abs(M))))
    dev = float(np.max(np.abs(Lf @ Lf.T - M)))
    print(f"{name} {method}: factor deviation {dev:.3e} allowance {tol:.3e}")
    assert dev <= tol


@pytest.mark.parametrize("name", ["small", "agg65", "agg197"])
def test_nonfinite_rows_are_marked_and_the_others_untouched(env, name):
    c, p = RC.all_cases()[name], RC.plan_parts(name)
    block, bad = RC.with_nonfinite(name)
    part = RC.participants(name)
    good = [t for t in range(c["rows"]) if t not in bad]
    for method in ("bottom_up", "ols"):
        clean, _s, _r = _block(env, name, method)
        for series_major in (True, False):
            y, status, _ = _block(env, name, method, block=block, series_major=series_major)
            assert status.tolist() == [2 if t in bad else 0 for t in range(c["rows"])]
            assert np.isnan(y[part][:, bad]).all()
            assert _same(y[part][:, good], clean[part][:, good])
            for e in RC.empty_columns(name):                    # an empty column passes through, NaN included
                assert _same(y[e], block[e])


def test_idempotence_and_one_factor_for_two_blocks(env):
    name = "agg129"
    c = RC.all_cases()[name]
    part = RC.participants(name)
    for method in SOLVED:
        _yard, tol, _w = RC.yardstick(name, method)
        y, _s, r = _block(env, name, method)
        again, status, _ = _block(env, name, method, block=y, factor=r["factor"], plan=r["plan"])
        assert (status == 0).all() and float(np.max(np.abs(again[part] - y[part]))) <= tol
        other = c["yhat"] * 1.5 + 2.0                            # a second block through the same factor == through a factor of its own
        a, _s, _r = _block(env, name, method, block=other, factor=r["factor"], plan=r["plan"])
        b, _s, _r = _block(env, name, method, block=other)
        assert _same(a, b)


def test_bad_weights_are_refused_by_column(env):
    c = RC.all_cases()["small"]
    p = RC.plan_parts("small")
    for bad in (0.0, -1.0, np.nan, np.inf):
        w = c["weights"].copy()
        w[p["agg_cols"][1]] = bad
        with pytest.raises(ValueError, match=f"the weight of column {p['agg_cols'][1]} is not finite and positive"):
            env["device"].reconcile_block(_up(env, c["yhat"]), _plan(env, "small"), "wls_var", weights=_up(env, w))
    w = c["weights"].copy()
    w[RC.empty_columns("small")[0]] = -1.0                       # an empty column takes no part: its weight is not read
    env["device"].reconcile_block(_up(env, c["yhat"]), _plan(env, "small"), "wls_var", weights=_up(env, w))
    out, err = env["api"].reconcile_batch(c["column_of"], c["yhat"], "wls_var", np.where(np.arange(c["n_out"]) == p["bottom_col"][2], 0.0, 1.0))
    assert not err["ok"] and err["code"] == 2 and f"column {p['bottom_col'][2]}" in err["message"]


def test_trailing_update_variants_agree(env, monkeypatch):
    """The plain-FMA tile and the MFMA tile of the trailing update (the developer knob reconcile_trailing of ANOFOX_HIP_TUNE, read
    at every factor call): both results lie within the allowance, each the same bits on a second run."""
    yard, tol, _w = RC.yardstick("agg197", "wls_struct")
    part = RC.participants("agg197")
    for variant in ("0", "1"):
        monkeypatch.setenv("ANOFOX_HIP_TUNE", f"reconcile_trailing={variant}")
        y, _s, _r = _block(env, "agg197", "wls_struct")
        y2, _s, _r = _block(env, "agg197", "wls_struct")
        dev = float(np.max(np.abs(y[part] - yard[part])))
        print(f"trailing variant {variant}: deviation {dev:.3e} allowance {tol:.3e}")
        assert dev <= tol and _same(y, y2)


def test_chain_aggregate_forecast_reconcile_score(env):
    """aggregate_block -> DeviceBatch (Naive, SES) -> reconcile_block on yhat where it lies -> anofox_hip_metrics_device on the result:
    no copy to the host in between.  The reconciled block is coherent to the bit and scores as the host's arithmetic says."""
    torch, device, lib, L, dev = env["torch"], env["device"], env["lib"], env["L"], env["dev"]
    n, T, h = 240, 40, 3                                         # 240 leaves, 48 stores of 5, 8 states of 6 stores, total: 297 columns
    s = np.arange(n)
    column_of = np.array([np.zeros(n), 1 + s // 30, 9 + s // 5, 57 + s], dtype=np.int32)
    rng = np.random.default_rng(11)
    y = np.zeros((T, 256))
    y[:, :n] = rng.uniform(1.0, 30.0, size=(T, n)) + np.linspace(0.0, 5.0, T)[:, None]
    lengths = np.zeros(256, dtype=np.int32)
    lengths[:n] = T
    agg = device.aggregate_block(torch.from_numpy(y).to(dev), torch.from_numpy(lengths).to(dev), torch.from_numpy(column_of).to(dev), n_series=n)
    n_out, t_out = agg["n_out"], agg["t_out"]
    assert (n_out, t_out) == (297, T)
    plan = device.reconcile_plan_device(column_of, device=dev)
    _n, offs, memb = HR.plan(column_of.tolist())
    p = R.parts(offs, memb, n)
    assert len(p["agg_cols"]) == 57
    for model in ("Naive", "SES"):
        b = device.DeviceBatch(n_out, t_out, lib.make_options(model, h), dev)
        b.set_block(agg["y"], agg["lengths"])
        b.run()
        res = b.results()
        rec = device.reconcile_block(res["yhat"], plan, "wls_struct")
        actual = res["yhat"]                                      # score the reconciled block against the base forecasts
        ld = 320
        fig = torch.full((12, ld), SENTINEL, dtype=torch.float64, device=dev)
        status = torch.full((n_out,), -5, dtype=torch.int32, device=dev)
        hl = torch.full((n_out,), h, dtype=torch.int32, device=dev)
        err = lib.AnofoxError()
        ok = L.anofox_hip_metrics_device(actual.data_ptr(), rec["y"].data_ptr(), None, None, None, None, 0, None, 0, int(actual.shape[1]), 1,
                                         hl.data_ptr(), n_out, h, 1 << lib.METRIC_FIGURES.index("mae"), 0.5, False, fig.data_ptr(), ld,
                                         status.data_ptr(), None, C.byref(err))
        assert ok, err.message
        torch.cuda.synchronize()
        yr, base = rec["y"].cpu().numpy()[:n_out], res["yhat"].cpu().numpy()[:n_out]
        b.close()
        assert (rec["row_status"].cpu().numpy() == 0).all() and (status.cpu().numpy() == 0).all()
        assert R.coherent_to_the_bit(p, yr).all()
        w = R.method_weights(p, "wls_struct")
        yard, tol = R.allowance(p, w, base, exact_limit=0)
        part = list(p["bottom_col"]) + list(p["agg_cols"])
        assert float(np.max(np.abs(yr[part] - yard[part]))) <= tol
        mae = fig.cpu().numpy()[0, :n_out]
        want = np.array([np.mean(np.abs(base[c, :h] - yr[c, :h])) for c in range(n_out)])
        assert np.allclose(mae, want, rtol=1e-12, atol=1e-300)


def test_mirror_end_to_end(env):
    """ts_reconcile_hierarchy on a three-level table of a dozen leaves, keyed as ts_aggregate_hierarchy keys its output."""
    api = env["api"]
    rng = np.random.default_rng(5)
    leaves = [(f"R{k // 6}", f"S{k // 3}", f"i{k}") for k in range(12)]
    keys = sorted({HR.build_unique_id(list(l), lv) for l in leaves for lv in range(4)}, key=lambda u: u.encode())
    days = np.array(["2024-03-01", "2024-03-02", "2024-03-03"], dtype="datetime64[D]")
    uid = [u for u in keys for _ in days]
    date = np.array([d for _ in keys for d in days])
    fc = rng.uniform(5.0, 50.0, size=len(uid))
    order = rng.permutation(len(uid))                            # the rows may arrive in any order
    info = {}
    got = api.ts_reconcile_hierarchy([uid[i] for i in order], date[order], fc[order], {"method": "ols"}, info=info)
    assert list(got["unique_id"]) == uid and (got["date"] == date).all() and (info["row_status"] == 0).all()
    co = info["column_of"]
    _n, offs, memb = HR.plan(co.tolist())
    p = R.parts(offs, memb, 12)
    block = fc.reshape(len(keys), 3)
    yard, tol = R.allowance(p, np.ones(len(keys)), block)
    y = got["forecast"].reshape(len(keys), 3)
    assert R.coherent_to_the_bit(p, y).all() and float(np.max(np.abs(y - yard))) <= tol
    direct, err = api.reconcile_batch(co, block, "ols")
    assert err["ok"] and _same(direct["y"], y)
    bu = api.ts_reconcile_hierarchy(uid, date, fc, {"method": "bottom_up"})
    assert _same(bu["forecast"].reshape(len(keys), 3), R.bottom_up(p, block))


def test_worst_ratio_is_reported():
    print("worst deviation / allowance per method:", {k: round(v, 4) for k, v in WORST.items()})
    assert all(v <= 1.0 for v in WORST.values())
