"""GPU: bootstrap sample paths and their quantiles -- anofox_hip_paths_device, anofox_hip_path_quantiles_device, anofox_hip_paths_batch,
device.paths_block / path_quantiles_block and the api mirrors -- against the pure-Python restatement tests/paths_ref.py, and against
tests/hierarchy_ref.py for the sums.  The contract (DESIGN.md section 3 "Sample paths") is equality of bits: the draws are
counter-based, the additions are serial, the quantiles are two-point interpolations of a total-order sort, so every comparison is ==
on the bit patterns; only the payload of a NaN is exempt (the sign of a zero is not).  Shapes: tests/paths_cases.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import hierarchy_ref as H
import paths_cases as K
import paths_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -777.25


@pytest.fixture(scope="module")
def env(hiplib):
    import torch
    assert torch.cuda.is_available()
    L = hiplib.load()
    from anofox_forecast_amd import api, device
    return {"torch": torch, "L": L, "lib": hiplib, "api": api, "device": device, "dev": torch.device("cuda:0")}


def _seed(n, h, P):
    return (n * 1000003 + h * 10007 + P) | (0xC0FFEE << 32)           # both key words in use


@functools.lru_cache(maxsize=None)
def _case(n, h, P, mode, joint):
    """The inputs and the restatement's answer of one case, computed once and shared (read-only) by the tests that need it."""
    pts = K.make_points(n, h, n + h)
    pools, rows = K.make_pools(n, n + P, joint)
    block, status = R.paths(pts, pools, P, mode, joint, seed=_seed(n, h, P), pool_rows=rows)
    q, qstatus = R.quantiles(block, h, P, K.LEVELS)
    for a in (pts, block, status, q, qstatus):
        a.setflags(write=False)
    return {"points": pts, "pools": pools, "pool_rows": rows, "paths": block, "status": status, "quantiles": q, "qstatus": qstatus,
            "seed": _seed(n, h, P)}


def _up(env, a):
    return env["torch"].from_numpy(np.array(a, order="C")).to(env["dev"])       # (a copy: the shared reference arrays are read-only)


def _tensors(env, pts, pools, pool_rows, point_sm=False, pool_sm=False, lengths=None):
    """Device tensors of a case: the point block and the pool in the asked layouts (time-major blocks have ld = n rounded up to 64 and
    hold a NaN in the padding columns, which nothing may read into a result), the lengths."""
    n, h = pts.shape
    ld = (n + 63) // 64 * 64
    pb = K.pool_block(pools, pool_rows)
    if point_sm:
        tp = _up(env, pts)
    else:
        a = np.full((h, ld), np.nan)
        a[:, :n] = pts.T
        tp = _up(env, a)
    if pool_sm:
        te = _up(env, pb)
    else:
        a = np.full((max(pool_rows, 1), ld), np.nan)
        a[:pool_rows, :n] = pb.T
        te = _up(env, a[:pool_rows] if pool_rows else a[:0])
    lens = [len(e) for e in pools] if lengths is None else lengths
    return tp, te, _up(env, np.array(lens, dtype=np.int32))


def _generate(env, pts, pools, pool_rows, P, mode, joint, seed, point_sm=False, pool_sm=False, lengths=None, pad=0, use_lengths=True):
    """device.paths_block into a sentinel-filled block with `pad` extra columns -> (paths [P * h, ld_out] numpy, status numpy, tensor)."""
    torch, device = env["torch"], env["device"]
    n, h = pts.shape
    tp, te, tl = _tensors(env, pts, pools, pool_rows, point_sm, pool_sm, lengths)
    ld_out = (n + 63) // 64 * 64 + pad
    out = torch.full((P * h, ld_out), SENTINEL, dtype=torch.float64, device=env["dev"])
    g = device.paths_block(tp, te, pool_lengths=tl if use_lengths else None, n_paths=P, mode=mode, joint=joint, seed=seed,
                           series_major=point_sm, pool_series_major=pool_sm, n_series=n, out=out)
    torch.cuda.synchronize()
    return g["paths"].cpu().numpy(), g["status"].cpu().numpy(), g["paths"]


def _assert_bits(got, want, what):
    same = R.same_bits(got, want)
    assert same.all(), f"{what}: {int((~same).sum())} cells differ, first at {np.argwhere(~same)[0].tolist()}"


# --------------------------------------------------------------------------------------------
# the two kernels against the restatement
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_paths_and_quantiles_equal_the_restatement(env, case):
    n, h, P, mode, joint = case
    ref = _case(*case)
    got, status, block = _generate(env, ref["points"], ref["pools"], ref["pool_rows"], P, mode, joint, ref["seed"], pad=3)
    assert status.tolist() == ref["status"].tolist() and (status == R.OK).all()
    _assert_bits(got[:, :n], ref["paths"], "paths")
    assert (got[:, n:] == SENTINEL).all()                               # the padding columns are not touched
    q = env["device"].path_quantiles_block(block, K.LEVELS, horizon=h, n_paths=P, n_cols=n)
    env["torch"].cuda.synchronize()
    assert q["status"].cpu().numpy().tolist() == ref["qstatus"].tolist()
    assert tuple(q["quantiles"].shape) == (len(K.LEVELS), n, h)
    _assert_bits(q["quantiles"].cpu().numpy(), ref["quantiles"], "quantiles")


@pytest.mark.parametrize("case", [c for c in K.CASES if c[2] <= 100], ids=K.case_id)
def test_both_layouts_of_point_and_pool_give_the_same_bits(env, case):
    n, h, P, mode, joint = case
    ref = _case(*case)
    for point_sm in (False, True):
        for pool_sm in (False, True):
            got, status, _ = _generate(env, ref["points"], ref["pools"], ref["pool_rows"], P, mode, joint, ref["seed"], point_sm, pool_sm)
            assert status.tolist() == ref["status"].tolist()
            _assert_bits(got[:, :n], ref["paths"], f"paths (point_sm={point_sm}, pool_sm={pool_sm})")


def test_sixteen_levels(env):
    n, h, P = 65, 5, 64
    ref = _case(n, h, P, "cumulative", True)
    want, wstatus = R.quantiles(ref["paths"], h, P, K.LEVELS_16)
    q = env["device"].path_quantiles_block(_up(env, ref["paths"]), K.LEVELS_16, horizon=h, n_paths=P)
    assert q["status"].cpu().numpy().tolist() == wstatus.tolist()
    _assert_bits(q["quantiles"].cpu().numpy(), want, "16 levels")
    with pytest.raises(ValueError, match="n_levels 17 exceeds the limit of 16 levels"):
        env["device"].path_quantiles_block(_up(env, ref["paths"]), [0.5] * 17, horizon=h, n_paths=P)


def test_seeds(env):
    n, h, P = 65, 9, 100
    pts, (pools, rows) = K.make_points(n, h, 1), K.make_pools(n, 1, False)
    a1, _, _ = _generate(env, pts, pools, rows, P, "cumulative", False, 12345)
    a2, _, _ = _generate(env, pts, pools, rows, P, "cumulative", False, 12345)
    b, _, _ = _generate(env, pts, pools, rows, P, "cumulative", False, 12346)
    hi, _, _ = _generate(env, pts, pools, rows, P, "cumulative", False, 12345 | (1 << 32))    # the high key word counts
    assert R.same_bits(a1, a2).all()                                    # the same seed twice: the same bits
    assert not R.same_bits(a1, b).all() and not R.same_bits(a1, hi).all()
    for seed, got in ((12345, a1), (12346, b), (12345 | (1 << 32), hi)):
        want, _ = R.paths(pts, pools, P, "cumulative", False, seed=seed, pool_rows=rows)
        _assert_bits(got[:, :n], want, f"seed {seed}")


# --------------------------------------------------------------------------------------------
# every entry gives the same bits
# --------------------------------------------------------------------------------------------
def _raw_device_entries(env, pts, pools, pool_rows, P, mode, joint, seed, levels):
    """The two C device entries called directly, on a side stream, into padded blocks."""
    torch, L, lib = env["torch"], env["L"], env["lib"]
    n, h = pts.shape
    tp, te, tl = _tensors(env, pts, pools, pool_rows)
    ld, ld_out = int(tp.shape[1]), (n + 63) // 64 * 64 + 5
    out = torch.full((P * h, ld_out), SENTINEL, dtype=torch.float64, device=env["dev"])
    status = torch.full((n + 2,), -9, dtype=torch.int32, device=env["dev"])
    q = torch.full((len(levels), n, h), SENTINEL, dtype=torch.float64, device=env["dev"])
    qstatus = torch.full((n + 2,), -9, dtype=torch.int32, device=env["dev"])
    opts = lib.make_paths_options(mode, joint, seed, "lane")
    lv = np.ascontiguousarray(levels, dtype=np.float64)
    err = lib.AnofoxError()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=env["dev"])
    st = C.c_void_p(side.cuda_stream)
    assert L.anofox_hip_paths_device(tp.data_ptr(), 1, ld, te.data_ptr(), 1, ld, tl.data_ptr(), pool_rows, n, h, P, C.byref(opts), C.sizeof(opts),
                                     out.data_ptr(), ld_out, status.data_ptr(), st, C.byref(err)), err.message
    assert L.anofox_hip_path_quantiles_device(out.data_ptr(), ld_out, n, h, P, lv.ctypes.data, len(lv), q.data_ptr(), qstatus.data_ptr(), st,
                                              C.byref(err)), err.message
    side.synchronize()
    return out.cpu().numpy(), status.cpu().numpy(), q.cpu().numpy(), qstatus.cpu().numpy()


@pytest.mark.parametrize("case", [(65, 5, 64, "cumulative", True), (65, 5, 64, "independent", False), (130, 8, 65, "cumulative", False)],
                         ids=K.case_id)
def test_every_entry_gives_the_same_bits(env, case):
    n, h, P, mode, joint = case
    ref = _case(*case)
    out, status, q, qstatus = _raw_device_entries(env, ref["points"], ref["pools"], ref["pool_rows"], P, mode, joint, ref["seed"], K.LEVELS)
    _assert_bits(out[:, :n], ref["paths"], "device entry: paths")
    assert (out[:, n:] == SENTINEL).all() and status[:n].tolist() == ref["status"].tolist() and (status[n:] == -9).all()
    _assert_bits(q, ref["quantiles"], "device entry: quantiles")
    assert qstatus[:n].tolist() == ref["qstatus"].tolist() and (qstatus[n:] == -9).all()
    # the batch entry packs the pools itself: pool_rows is the longest pool there, which changes no draw (n is the pool's own length)
    res, err = env["api"].paths_batch(ref["points"], ref["pools"], K.LEVELS, n_paths=P, mode=mode, joint=joint, seed=ref["seed"], want_paths=True)
    assert err["ok"], err
    assert res["n_out"] == n and res["ld"] == (n + 63) // 64 * 64
    _assert_bits(res["paths"][:, :n], ref["paths"], "batch entry: paths")
    assert (res["paths"][:, n:] == 0.0).all()
    _assert_bits(res["quantiles"], ref["quantiles"], "batch entry: quantiles")
    assert res["status"].tolist() == ref["qstatus"].tolist() and res["series_status"].tolist() == ref["status"].tolist()


# --------------------------------------------------------------------------------------------
# statuses
# --------------------------------------------------------------------------------------------
def test_statuses(env):
    nan, inf = float("nan"), float("inf")
    n, h, P = 8, 5, 64
    pts = K.make_points(n, h, 9)
    pts[4, 2] = nan                                                     # a NaN point
    pools = [np.array([1.0, 2.0]), np.zeros(0), np.array([1.0, nan, 3.0]), np.array([1.0, 2.0, nan]), np.array([1.0]),
             np.array([inf, -inf, 1.0]), np.array([0.5, -0.5, 0.25, 4.0]), np.array([inf, 2.0])]
    lengths = [2, 0, 3, 2, 1, 3, 4, 2]                                  # series 3: the NaN lies beyond the length and is ignored
    want, wstatus = R.paths(pts, pools, P, "cumulative", False, seed=77, lengths=lengths, pool_rows=4)
    assert wstatus.tolist() == [R.OK, R.EMPTY, R.NAN, R.OK, R.NAN, R.OK, R.OK, R.OK]
    got, status, block = _generate(env, pts, pools, 4, P, "cumulative", False, 77, lengths=lengths)
    assert status.tolist() == wstatus.tolist()
    _assert_bits(got[:, :n], want, "paths with statuses")               # the series with other statuses in the same call are untouched
    assert np.isnan(got[:, [1, 2, 4]]).all() and not np.isnan(got[:, [0, 3, 6]]).any() and np.isinf(got[:, 7]).any()
    # the quantile entry: a column with a NaN among its paths (also one that inf - inf made) has status 2 and NaN everywhere
    wq, wqs = R.quantiles(want, h, P, K.LEVELS)
    assert wqs.tolist() == [0, 2, 2, 0, 2, 2, 0, 0]
    q = env["device"].path_quantiles_block(block, K.LEVELS, horizon=h, n_paths=P, n_cols=n)
    assert q["status"].cpu().numpy().tolist() == wqs.tolist()
    _assert_bits(q["quantiles"].cpu().numpy(), wq, "quantiles with statuses")
    # a NaN in ONE cell of a column, with either sign bit: NaN in every quantile of every step of that column alone
    for bits in (0x7FF8000000000000, 0xFFF8000000000000):
        one = want[:, [0, 3, 6]].copy()
        one[(P // 2) * h + 1, 1] = np.array([bits], dtype=np.uint64).view(np.float64)[0]
        wq1, wqs1 = R.quantiles(one, h, P, K.LEVELS)
        q1 = env["device"].path_quantiles_block(_up(env, np.pad(one, ((0, 0), (0, 61)))), K.LEVELS, horizon=h, n_paths=P, n_cols=3)
        assert q1["status"].cpu().numpy().tolist() == wqs1.tolist() == [0, 2, 0]
        _assert_bits(q1["quantiles"].cpu().numpy(), wq1, "one NaN cell")
    # joint mode: a ragged series has status 3, the others are untouched; without lengths every pool has pool_rows rows
    jl = [4, 4, 3, 4, 0, 4, 4, 5]
    jpools = [np.arange(1.0, 5.0) * (s + 1) for s in range(n)]
    jpts = K.make_points(n, h, 10)
    jw, jws = R.paths(jpts, jpools, P, "independent", True, seed=78, lengths=jl, pool_rows=4)
    assert jws.tolist() == [0, 0, R.RAGGED, 0, R.RAGGED, 0, 0, R.RAGGED]
    jg, js, _ = _generate(env, jpts, jpools, 4, P, "independent", True, 78, lengths=jl)
    assert js.tolist() == jws.tolist()
    _assert_bits(jg[:, :n], jw, "joint paths with a ragged series")
    fw, fws = R.paths(jpts, jpools, P, "independent", True, seed=78, pool_rows=4)
    fg, fs, _ = _generate(env, jpts, jpools, 4, P, "independent", True, 78, use_lengths=False)
    assert fs.tolist() == fws.tolist() == [0] * n
    _assert_bits(fg[:, :n], fw, "joint paths without lengths")


# --------------------------------------------------------------------------------------------
# the chain: paths -> sums up a hierarchy -> quantiles
# --------------------------------------------------------------------------------------------
def _aggregate_ref(block, column_of):
    """hierarchy_ref on the columns of a path block: [rows, n_out], every cell the serial chain over its members' paths."""
    n_out, offs, memb = H.plan(column_of)
    series = [block[:, s] for s in range(block.shape[1])]
    cols = H.aggregate_block(series, [0] * len(series), offs, memb)
    out = np.zeros((block.shape[0], n_out))
    for c, (_lo, length, y, _p) in enumerate(cols):
        out[:length, c] = y
    return out


def test_chain_on_a_three_level_plan(env):
    torch, device = env["torch"], env["device"]
    n, h, P = 12, 5, 100
    column_of = K.three_level_plan()
    pts = K.make_points(n, h, 12)
    pools, rows = K.make_pools(n, 12, True, rows=7)
    pools[3] = np.array([1e16, 1.0, -1e16, 3.0, 1e-3, -1e16, 1e16])      # sums whose bits show the order of the additions
    pools[9] = pools[3][::-1].copy()
    for mode, joint in (("cumulative", True), ("independent", False)):
        want, _ = R.paths(pts, pools, P, mode, joint, seed=4242, pool_rows=rows)
        wagg = _aggregate_ref(want, column_of.tolist())
        wq, wqs = R.quantiles(wagg, h, P, K.LEVELS)
        _, _, block = _generate(env, pts, pools, rows, P, mode, joint, 4242)
        full = torch.full((block.shape[1],), P * h, dtype=torch.int32, device=env["dev"])
        a = device.aggregate_block(block, full, torch.from_numpy(column_of).to(env["dev"]), n_series=n, t_out=P * h)
        assert a["n_out"] == 16
        _assert_bits(a["y"].cpu().numpy()[:, :16], wagg, f"aggregated paths ({mode})")
        q = device.path_quantiles_block(a["y"], K.LEVELS, horizon=h, n_paths=P, n_cols=16)
        assert q["status"].cpu().numpy().tolist() == wqs.tolist() == [0] * 16
        _assert_bits(q["quantiles"].cpu().numpy(), wq, f"quantiles of the aggregates ({mode})")
        res, err = env["api"].paths_batch(pts, pools, K.LEVELS, n_paths=P, mode=mode, joint=joint, seed=4242, column_of=column_of, want_paths=True)
        assert err["ok"], err
        assert res["n_out"] == 16 and res["ld"] == 64
        _assert_bits(res["paths"][:, :16], wagg, f"batch entry: aggregated paths ({mode})")
        _assert_bits(res["quantiles"], wq, f"batch entry: quantiles of the aggregates ({mode})")
        assert res["status"].tolist() == [0] * 16 and res["series_status"].tolist() == [0] * n
    # a wrong order of the members would show: the reversed chain differs in bits somewhere
    want, _ = R.paths(pts, pools, P, "cumulative", True, seed=4242, pool_rows=rows)
    n_out, offs, memb = H.plan(column_of.tolist())
    rev = H.aggregate_block([want[:, s] for s in range(n)], [0] * n, offs, memb, reverse=True)
    assert not R.same_bits(rev[0][2], _aggregate_ref(want, column_of.tolist())[:, 0]).all()


def test_joint_band_of_two_dependent_leaves_is_wider(env):
    """Two leaves with the same pool are perfectly dependent under a joint draw (the same row for both at every step) and independent
    otherwise: the 5 % .. 95 % band of their sum is wider in joint mode.  The restatement decides the direction; the device gives
    its bits."""
    h, P = 8, 1000
    pts = np.zeros((2, h))
    pool = np.random.default_rng(5).normal(0.0, 1.0, size=40)
    column_of = np.zeros((1, 2), dtype=np.int32)
    width = {}
    for joint in (True, False):
        want, _ = R.paths(pts, [pool, pool], P, "cumulative", joint, seed=31, pool_rows=40)
        wq, _ = R.quantiles(_aggregate_ref(want, column_of.tolist()), h, P, [0.05, 0.95])
        res, err = env["api"].paths_batch(pts, [pool, pool], [0.05, 0.95], n_paths=P, mode="cumulative", joint=joint, seed=31, column_of=column_of)
        assert err["ok"], err
        _assert_bits(res["quantiles"], wq, f"sum of two leaves (joint={joint})")
        width[joint] = (wq[1, 0, :] - wq[0, 0, :], res["quantiles"][1, 0, :] - res["quantiles"][0, 0, :])
    assert (width[True][0] > width[False][0]).all()                     # the restatement: wider at every step
    assert (width[True][1] > width[False][1]).all()                     # the device: the same direction


# --------------------------------------------------------------------------------------------
# the blocks of a backtest and of a batch, as they lie
# --------------------------------------------------------------------------------------------
def test_backtest_error_block_and_batch_yhat_as_they_lie(env):
    torch, device, lib, api = env["torch"], env["device"], env["lib"], env["api"]
    N, T, h, F, P = 8, 40, 4, 3, 65
    rng = np.random.default_rng(8)
    Y = np.cumsum(rng.normal(0.0, 1.0, size=(N, T)), axis=1) + 20.0
    y = _up(env, device.pack_time_major(Y))
    lens = torch.zeros(y.shape[1], dtype=torch.int32, device=env["dev"])
    lens[:N] = T
    opts = lib.make_options("Naive", h, auto_detect=False)
    folds = api.backtest_fold_bounds(T, h, F)
    bt = device.backtest_block(y, lens, opts, folds, n_series=N)
    batch = device.DeviceBatch(N, T, opts, env["dev"])
    batch.set_block(y, lens)
    batch.run()
    yhat = batch.results()["yhat"]                                      # [N, h] series-major
    error = bt["error"].view(N, len(folds) * h)                         # [N, F * h] series-major: the pool of every series
    torch.cuda.synchronize()
    pts, pool = yhat.cpu().numpy(), error.cpu().numpy()
    assert not np.isnan(pool).any() and pool.shape == (N, len(folds) * h)
    for mode, joint in (("cumulative", True), ("independent", False)):
        want, wstatus = R.paths(pts, list(pool), P, mode, joint, seed=2026)
        g = device.paths_block(yhat, error, n_paths=P, mode=mode, joint=joint, seed=2026, series_major=True, pool_series_major=True)
        torch.cuda.synchronize()
        assert g["status"].cpu().numpy().tolist() == wstatus.tolist() == [0] * N
        _assert_bits(g["paths"].cpu().numpy()[:, :N], want, f"paths from a backtest's blocks ({mode})")


# --------------------------------------------------------------------------------------------
# the end-to-end mirror
# --------------------------------------------------------------------------------------------
def test_ts_forecast_quantiles_by(env):
    api = env["api"]
    n, T, h, F, P = 6, 36, 5, 8, 1000
    rng = np.random.default_rng(6)
    days = np.datetime64("2024-01-01") + np.arange(T)
    group, date, target = [], [], []
    for t in range(T):                                                  # interleaved rows: the groups' first-appearance order is g3, g0, ...
        for s in (3, 0, 5, 1, 4, 2):
            if s == 4 and t >= T - 3:
                continue                                                # g4 ends three days early: it has no residual in the last folds
            group.append(f"g{s}")
            date.append(days[t])
            target.append(10.0 * (s + 1) + 0.3 * t + float(rng.normal()))
    date, target = np.array(date), np.array(target)
    levels = [0.05, 0.25, 0.5, 0.75, 0.95]
    info = {}
    out = api.ts_forecast_quantiles_by(group, date, target, "Naive", h, "1d", levels, residual_folds=F, n_paths=P, mode="cumulative", joint=True,
                                       seed=99, info=info)
    base = api.ts_forecast_by(group, date, target, "Naive", h, "1d")
    names = ["q0.05", "q0.25", "q0.5", "q0.75", "q0.95"]
    assert list(out) == list(base) + names + ["paths_status"]
    for c in base:                                                      # the columns and the row order of ts_forecast_by, the same points
        assert len(out[c]) == len(base[c]) == n * h
        if np.asarray(base[c]).dtype == np.float64:
            _assert_bits(out[c], base[c], c)
        else:
            assert list(out[c]) == list(base[c]), c
    assert info["groups"] == ["g3", "g0", "g5", "g1", "g4", "g2"] and info["errors"].shape == (n, F)
    # the quantile columns equal the restatement fed with the same backtest errors and the same points
    pts = np.asarray(out["yhat"]).reshape(n, h)
    block, wstatus = R.paths(pts, list(info["errors"]), P, "cumulative", True, seed=99)
    wq, wqs = R.quantiles(block, h, P, levels)
    assert wstatus.tolist() == [0, 0, 0, 0, R.NAN, 0] and info["series_status"].tolist() == wstatus.tolist()
    for l, c in enumerate(names):
        _assert_bits(np.asarray(out[c]).reshape(n, h), wq[l], c)
    status = np.asarray(out["paths_status"]).reshape(n, h)
    assert (status == np.array(wstatus)[:, None]).all()                 # g4 says why its quantiles are NaN
    assert np.isnan(np.asarray(out["q0.5"]).reshape(n, h)[4]).all()
    ok = [s for s in range(n) if s != 4]
    q = np.stack([np.asarray(out[c]).reshape(n, h)[ok] for c in names])
    assert (np.diff(q, axis=0) >= 0.0).all()                            # the levels are monotone
    with pytest.raises(api.InvalidInputException, match="exceeds the limit of 16 levels"):
        api.ts_forecast_quantiles_by(group, date, target, "Naive", h, "1d", [0.5] * 17, residual_folds=F, n_paths=8)
