"""GPU: the scores of sample paths -- anofox_hip_path_scores_device, anofox_hip_path_energy_device, anofox_hip_path_scores_batch,
device.path_scores_block / path_energy_block and the api mirrors -- against the pure-Python restatement tests/path_scores_ref.py,
against the existing quantile and metrics entries, and against tests/hierarchy_ref.py for the sums.  The contract (DESIGN.md section 3
"Path scores") is equality of bits: the sort is a total order, every sum over paths or columns is the wave sum, every other sum is
serial, so every comparison is == on the bit patterns; only the payload of a NaN is exempt (the sign of a zero is not).  Shapes:
tests/path_scores_cases.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import hierarchy_ref as H
import path_scores_cases as K
import path_scores_ref as R
import paths_cases
import paths_ref

pytestmark = pytest.mark.gpu

SENTINEL = -777.25


@pytest.fixture(scope="module")
def env(hiplib):
    import torch
    assert torch.cuda.is_available()
    L = hiplib.load()
    from anofox_forecast_amd import api, device
    return {"torch": torch, "L": L, "lib": hiplib, "api": api, "device": device, "dev": torch.device("cuda:0")}


@functools.lru_cache(maxsize=None)
def _case(n, h, P, lv, special=True):
    """The inputs and the restatement's answer of one case, computed once and shared (read-only) by the tests that need it."""
    block, actual = K.make_block(n, h, P, n + 7 * h + P, special)
    ref = R.scores(block, actual, h, P, K.LEVEL_SETS[lv])
    for a in (block, actual) + tuple(ref.values()):
        a.setflags(write=False)
    return {"block": block, "actual": actual, "ref": ref}


def _up(env, a):
    return env["torch"].from_numpy(np.array(a, order="C")).to(env["dev"])       # (a copy: the shared reference arrays are read-only)


def _bits(got, want, what):
    same = R.same_bits(got, want)
    assert same.all(), f"{what}: {int((~same).sum())} cells differ, first at {np.argwhere(~same)[0].tolist()}"


def _assert_scores(got, ref, n, what):
    """Every output of path_scores_block against the restatement."""
    assert got["status"].cpu().numpy().tolist() == ref["status"].tolist(), what
    _bits(got["crps"].cpu().numpy(), ref["crps"], what + ": crps")
    assert (got["below"].cpu().numpy() == ref["below"]).all() and (got["equal"].cpu().numpy() == ref["equal"]).all(), what + ": ranks"
    if ref["quantiles"].shape[0]:
        _bits(got["quantiles"].cpu().numpy(), ref["quantiles"], what + ": quantiles")
    else:
        assert got["quantiles"] is None
    _bits(got["column"].cpu().numpy()[:, :n], ref["column"], what + ": column")
    _bits(got["crps_mean"].cpu().numpy(), ref["column"][0], what + ": crps_mean")
    _bits(got["n_steps"].cpu().numpy(), ref["column"][1], what + ": n_steps")
    _bits(got["pinball"].cpu().numpy(), ref["column"][2:], what + ": pinball")


# --------------------------------------------------------------------------------------------
# the score kernel against the restatement, the quantile entry and the metrics entry
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_scores_equal_the_restatement(env, case):
    n, h, P, lv = case
    c = _case(*case)
    levels = K.LEVEL_SETS[lv]
    paths = _up(env, K.pad_columns(c["block"]))                        # NaN in the padding columns: nothing may read them into a result
    tm, sm = _up(env, K.time_major(c["actual"])), _up(env, c["actual"])
    got = env["device"].path_scores_block(paths, tm, levels, horizon=h, n_paths=P, n_cols=n)
    _assert_scores(got, c["ref"], n, "time-major actual")
    # both layouts of the actual, and a second run: the same bits
    again = env["device"].path_scores_block(paths, sm, levels, horizon=h, n_paths=P, n_cols=n, actual_series_major=True)
    _assert_scores(again, c["ref"], n, "series-major actual")
    # the quantiles are those of the quantile entry
    if levels:
        q = env["device"].path_quantiles_block(paths, levels, horizon=h, n_paths=P, n_cols=n)
        _bits(got["quantiles"].cpu().numpy(), q["quantiles"].cpu().numpy(), "quantiles against the quantile entry")
        assert ((got["status"].cpu().numpy() == R.NAN) == (q["status"].cpu().numpy() == paths_ref.NAN)).all()


@pytest.mark.parametrize("case", [(65, 3, 65, "nine"), (130, 28, 1000, "nine")], ids=K.case_id)
def test_pinball_has_the_bits_of_the_metrics_entry(env, case):
    """The pinball rows against anofox_hip_metrics_device's quantile_loss on the quantiles output, the steps without an actual dropped."""
    torch, L, lib = env["torch"], env["L"], env["lib"]
    n, h, P, lv = case
    c = _case(*case)
    levels = K.LEVEL_SETS[lv]
    sm = _up(env, c["actual"])
    got = env["device"].path_scores_block(_up(env, K.pad_columns(c["block"])), sm, levels, horizon=h, n_paths=P, n_cols=n, actual_series_major=True)
    lens = torch.full((n,), h, dtype=torch.int32, device=env["dev"])
    ld = (n + 63) // 64 * 64
    pin = got["pinball"].cpu().numpy()
    for l, tau in enumerate(levels):
        fig = torch.full((12, ld), SENTINEL, dtype=torch.float64, device=env["dev"])
        status = torch.full((n,), -5, dtype=torch.int32, device=env["dev"])
        err = lib.AnofoxError()
        ok = L.anofox_hip_metrics_device(sm.data_ptr(), got["quantiles"][l].data_ptr(), None, None, None, None, 0, None, 0, h, 1, lens.data_ptr(), n, h,
                                         1 << 9, float(tau), True, fig.data_ptr(), ld, status.data_ptr(), None, C.byref(err))
        assert ok, err.message
        _bits(pin[l], fig.cpu().numpy()[9, :n], f"pinball of level {tau}")


def test_padding_and_optional_outputs(env):
    """The raw entry on a side stream: a block with columns beyond n_cols gives the bits of the block cut to n_cols, cells beyond
    n_cols are not touched, and every output but the status can be left out."""
    torch, L, lib = env["torch"], env["L"], env["lib"]
    n, h, P, lv = 65, 3, 65, "nine"
    c = _case(n, h, P, lv)
    ref, levels = c["ref"], np.ascontiguousarray(K.LEVELS, dtype=np.float64)
    k = len(levels)
    wide = np.full((P * h, 192), 4e300)                                 # 127 columns beyond n_cols hold values that would show
    wide[:, :n] = c["block"]
    paths, actual = _up(env, wide), _up(env, K.time_major(c["actual"], 128, fill=4e300))
    ld_out = 70
    new = lambda shape, dt, fill: torch.full(shape, fill, dtype=dt, device=env["dev"])
    crps, below, equal = new((n + 2, h), torch.float64, SENTINEL), new((n + 2, h), torch.int32, -9), new((n + 2, h), torch.int32, -9)
    q, column, status = new((k, n, h), torch.float64, SENTINEL), new((2 + k, ld_out), torch.float64, SENTINEL), new((n + 2,), torch.int32, -9)
    err = lib.AnofoxError()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=env["dev"])
    st = C.c_void_p(side.cuda_stream)
    args = (paths.data_ptr(), 192, n, h, P, actual.data_ptr(), 1, 128, levels.ctypes.data, k)
    assert L.anofox_hip_path_scores_device(*args, crps.data_ptr(), below.data_ptr(), equal.data_ptr(), q.data_ptr(), column.data_ptr(), ld_out,
                                           status.data_ptr(), st, C.byref(err)), err.message
    only = new((n,), torch.int32, -9)
    assert L.anofox_hip_path_scores_device(*args, None, None, None, None, None, 0, only.data_ptr(), st, C.byref(err)), err.message
    crps2, col0 = new((n, h), torch.float64, SENTINEL), new((2, ld_out), torch.float64, SENTINEL)
    assert L.anofox_hip_path_scores_device(*args[:8], None, 0, crps2.data_ptr(), None, None, None, col0.data_ptr(), ld_out, only.data_ptr(), st,
                                           C.byref(err)), err.message
    side.synchronize()
    _bits(crps.cpu().numpy()[:n], ref["crps"], "crps")
    assert (crps.cpu().numpy()[n:] == SENTINEL).all() and (below.cpu().numpy()[n:] == -9).all() and (equal.cpu().numpy()[n:] == -9).all()
    assert (below.cpu().numpy()[:n] == ref["below"]).all() and (equal.cpu().numpy()[:n] == ref["equal"]).all()
    _bits(q.cpu().numpy(), ref["quantiles"], "quantiles")
    _bits(column.cpu().numpy()[:, :n], ref["column"], "column")
    assert (column.cpu().numpy()[:, n:] == SENTINEL).all()
    assert status.cpu().numpy()[:n].tolist() == ref["status"].tolist() == only.cpu().numpy().tolist() and (status.cpu().numpy()[n:] == -9).all()
    _bits(crps2.cpu().numpy(), ref["crps"], "crps without levels")
    _bits(col0.cpu().numpy()[:, :n], ref["column"][:2], "column without levels")
    with pytest.raises(ValueError, match="n_levels 17 exceeds the limit of 16 levels"):
        env["device"].path_scores_block(paths, actual, [0.5] * 17, horizon=h, n_paths=P, n_cols=n)
    with pytest.raises(ValueError, match="unknown outputs"):
        env["device"].path_scores_block(paths, actual, horizon=h, n_paths=P, n_cols=n, want=("crps", "variogram"))
    part = env["device"].path_scores_block(paths, actual, K.LEVELS, horizon=h, n_paths=P, n_cols=n, want=("column",))
    assert part["crps"] is None and part["below"] is None and part["quantiles"] is None
    _bits(part["column"].cpu().numpy()[:, :n], ref["column"], "column alone")


def test_statuses(env):
    nan = float("nan")
    n, h, P = 8, 3, 64
    block, actual = K.make_block(n, h, P, 99, special=False)
    block, actual = block.copy(), actual.copy()
    actual[1, :] = nan                                                  # no actual: 1
    actual[2, 1] = nan                                                  # one step dropped: 0
    block[5 * h + 2, 3] = nan                                           # a NaN path: 2
    block[7 * h + 0, 4] = np.array([0xFFF8000000000000], dtype=np.uint64).view(np.float64)[0]       # a NaN with the sign bit, and no
    actual[4, :] = nan                                                  # actual either: 2 takes precedence
    ref = R.scores(block, actual, h, P, K.LEVELS)
    assert ref["status"].tolist() == [0, 1, 0, 2, 2, 0, 0, 0] and ref["column"][1].tolist()[:3] == [3.0, 0.0, 2.0]
    got = env["device"].path_scores_block(_up(env, K.pad_columns(block)), _up(env, actual), K.LEVELS, horizon=h, n_paths=P, n_cols=n,
                                          actual_series_major=True)
    _assert_scores(got, ref, n, "statuses")
    col = got["column"].cpu().numpy()
    assert np.isnan(col[:, 3]).all() and np.isnan(col[:, 4]).all() and np.isnan(col[0, 1]) and col[1, 1] == 0.0
    assert not np.isnan(got["quantiles"].cpu().numpy()[:, 1]).any()      # the quantiles of a column without an actual are computed


# --------------------------------------------------------------------------------------------
# the energy score
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("special", (False, True), ids=("finite", "special"))
@pytest.mark.parametrize("case", K.ENERGY_CASES, ids=K.energy_id)
def test_energy_equals_the_restatement(env, case, special):
    n, h, P, cb, ce = case
    c = _case(n, h, P, "none", special)
    ref = R.energy(c["block"], c["actual"], h, P, cb, ce)
    paths = _up(env, K.pad_columns(c["block"]))
    for sm in (False, True):
        actual = _up(env, c["actual"] if sm else K.time_major(c["actual"]))
        got = env["device"].path_energy_block(paths, actual, horizon=h, n_paths=P, col_begin=cb, col_end=ce, actual_series_major=sm)
        _bits(got["es"].cpu().numpy(), ref["es"], f"es (series-major {sm})")
        summary = got["summary"].cpu().numpy()
        _bits(summary, [ref["es_mean"], float(ref["es_steps"])], f"summary (series-major {sm})")
        work = got["workspace"].cpu().numpy()
        _bits(work[0], ref["d1"], "D1")
        _bits(work[1, :P - 1], ref["d2"], "D2")
    if special and ce - cb > 60:
        assert ref["es_steps"] < h or np.isnan(ref["es_mean"])          # a NaN of the range reached the score
    with pytest.raises(ValueError, match="is empty or reversed"):
        env["device"].path_energy_block(paths, actual, horizon=h, n_paths=P, col_begin=ce, col_end=cb, actual_series_major=True)
    with pytest.raises(ValueError, match="ends beyond ld"):
        env["device"].path_energy_block(paths, actual, horizon=h, n_paths=P, col_begin=0, col_end=int(paths.shape[1]) + 1, actual_series_major=True)


# --------------------------------------------------------------------------------------------
# the chain: paths -> sums of paths and of actuals up a hierarchy -> scores per column, energy score per level
# --------------------------------------------------------------------------------------------
def _aggregate_ref(block, column_of):
    """hierarchy_ref on the columns of a block: [rows, n_out], every cell the serial chain over its members."""
    n_out, offs, memb = H.plan(column_of)
    series = [block[:, s] for s in range(block.shape[1])]
    cols = H.aggregate_block(series, [0] * len(series), offs, memb)
    out = np.zeros((block.shape[0], n_out))
    for c, (_lo, length, y, _p) in enumerate(cols):
        out[:length, c] = y
    return out


def _chain_inputs(n, h, seed):
    pts = paths_cases.make_points(n, h, seed)
    pools, rows = paths_cases.make_pools(n, seed, True, rows=7)
    pools[3] = np.array([1e16, 1.0, -1e16, 3.0, 1e-3, -1e16, 1e16])      # sums whose bits show the order of the additions
    pools[9] = pools[3][::-1].copy()
    actuals = pts + np.random.default_rng(seed).normal(0.0, 3.0, size=(n, h))
    actuals[5, 1] = np.nan                                              # a leaf without a row at step 1: its group and the total drop it
    actuals[0, 0] = pts[0, 0]
    return pts, pools, rows, actuals


def test_chain_on_a_three_level_plan(env):
    torch, device, api = env["torch"], env["device"], env["api"]
    n, h, P = 12, 5, 100
    column_of = paths_cases.three_level_plan()
    pts, pools, rows, actuals = _chain_inputs(n, h, 12)
    levels = K.LEVELS
    ranges = [(0, 1), (1, 4), (4, 16), (0, 16)]
    for mode, joint in (("cumulative", True), ("independent", False)):
        want, _ = paths_ref.paths(pts, pools, P, mode, joint, seed=4242, pool_rows=rows)
        wagg = _aggregate_ref(want, column_of.tolist())                   # [P * h, 16]
        wact = _aggregate_ref(actuals.T.copy(), column_of.tolist()).T     # [16, h]: the serial sums of the members' actuals
        assert np.isnan(wact[0, 1]) and np.isnan(wact[2, 1]) and np.isnan(wact[4 + 5, 1]) and np.isnan(wact).sum() == 3
        ref = R.scores(wagg, wact, h, P, levels)
        eref = [R.energy(wagg, wact, h, P, cb, ce) for cb, ce in ranges]
        # on the device, entry by entry
        g = device.paths_block(_up(env, pts), _up(env, paths_cases.pool_block(pools, rows)), n_paths=P, mode=mode, joint=joint, seed=4242,
                               series_major=True, pool_series_major=True, n_series=n)
        co = torch.from_numpy(column_of).to(env["dev"])
        full = torch.full((g["paths"].shape[1],), P * h, dtype=torch.int32, device=env["dev"])
        a = device.aggregate_block(g["paths"], full, co, n_series=n, t_out=P * h)
        steps = torch.full((64,), h, dtype=torch.int32, device=env["dev"])
        b = device.aggregate_block(_up(env, K.time_major(actuals, fill=0.0)), steps, co, n_series=n, t_out=h)
        assert a["n_out"] == b["n_out"] == 16
        _bits(b["y"].cpu().numpy()[:, :16].T, wact, f"aggregated actuals ({mode})")
        got = device.path_scores_block(a["y"], b["y"], levels, horizon=h, n_paths=P, n_cols=16)
        _assert_scores(got, ref, 16, f"scores of the aggregates ({mode})")
        for (cb, ce), e in zip(ranges, eref):
            ge = device.path_energy_block(a["y"], b["y"], horizon=h, n_paths=P, col_begin=cb, col_end=ce)
            _bits(ge["es"].cpu().numpy(), e["es"], f"energy score of [{cb}, {ce}) ({mode})")
            _bits(ge["summary"].cpu().numpy(), [e["es_mean"], float(e["es_steps"])], f"energy summary of [{cb}, {ce}) ({mode})")
        # the batch entry: the same bits from host buffers
        res, err = api.path_scores_batch(pts, pools, actuals, levels, n_paths=P, mode=mode, joint=joint, seed=4242, column_of=column_of)
        assert err["ok"], err
        assert res["n_out"] == 16 and res["ld"] == 64 and res["ranges"].tolist() == [list(r) for r in ranges]
        _bits(res["crps"], ref["crps"], f"batch entry: crps ({mode})")
        assert (res["below"] == ref["below"]).all() and (res["equal"] == ref["equal"]).all()
        _bits(res["quantiles"], ref["quantiles"], f"batch entry: quantiles ({mode})")
        _bits(np.vstack([res["crps_mean"], res["n_steps"], res["pinball"]]), ref["column"], f"batch entry: column ({mode})")
        assert res["status"].tolist() == ref["status"].tolist() == [0] * 16 and res["series_status"].tolist() == [0] * n
        _bits(res["energy"], np.stack([e["es"] for e in eref]), f"batch entry: energy ({mode})")
        _bits(res["energy_mean"], [e["es_mean"] for e in eref], f"batch entry: energy mean ({mode})")
        assert res["energy_steps"].tolist() == [float(e["es_steps"]) for e in eref] == [4.0, 4.0, 4.0, 4.0]


def test_batch_entry_without_a_plan(env):
    n, h, P = 65, 3, 64
    pts = paths_cases.make_points(n, h, 3)
    pools, rows = paths_cases.make_pools(n, 3, False)
    actuals = pts + np.random.default_rng(3).normal(0.0, 2.0, size=(n, h))
    actuals[2, :] = np.nan
    actuals[9, 2] = np.nan
    want, wstatus = paths_ref.paths(pts, pools, P, "cumulative", False, seed=17)
    ref, e = R.scores(want, actuals, h, P, K.LEVELS), R.energy(want, actuals, h, P, 0, n)
    res, err = env["api"].path_scores_batch(pts, pools, actuals, K.LEVELS, n_paths=P, seed=17)
    assert err["ok"], err
    assert res["n_out"] == n and res["ld"] == 128 and res["ranges"].tolist() == [[0, n]]
    _bits(res["crps"], ref["crps"], "crps")
    assert (res["below"] == ref["below"]).all() and (res["equal"] == ref["equal"]).all()
    _bits(res["quantiles"], ref["quantiles"], "quantiles")
    _bits(np.vstack([res["crps_mean"], res["n_steps"], res["pinball"]]), ref["column"], "column")
    assert res["status"].tolist() == ref["status"].tolist() and res["status"][2] == R.NO_ACTUAL
    assert res["series_status"].tolist() == wstatus.tolist()
    _bits(res["energy"][0], e["es"], "energy")
    assert np.isnan(res["energy"]).all() and res["energy_steps"].tolist() == [0.0] and np.isnan(res["energy_mean"][0])      # column 2 has no actual
    none, err = env["api"].path_scores_batch(pts, pools, actuals, (), n_paths=P, seed=17)
    assert err["ok"], err
    _bits(none["crps"], ref["crps"], "crps without levels")
    assert none["quantiles"].shape == (0, n, h) and none["pinball"].shape == (0, n)


# --------------------------------------------------------------------------------------------
# a backtest's blocks as they lie
# --------------------------------------------------------------------------------------------
def test_backtest_actual_block_as_it_lies(env):
    """The pairs of a backtest as columns: the paths around the backtest's forecasts, scored against its `actual` block -- series-major
    [n_pairs, h], NaN where a row does not exist -- without a copy."""
    torch, device, lib, api = env["torch"], env["device"], env["lib"], env["api"]
    N, T, h, F, P = 8, 40, 4, 3, 65
    rng = np.random.default_rng(8)
    Y = np.cumsum(rng.normal(0.0, 1.0, size=(N, T)), axis=1) + 20.0
    y = _up(env, device.pack_time_major(Y))
    lens = torch.zeros(y.shape[1], dtype=torch.int32, device=env["dev"])
    lens[:N] = T
    lens[3] = T - 2                                                     # series 3 ends two rows early: its last fold lacks two rows
    opts = lib.make_options("Naive", h, auto_detect=False)
    folds = api.backtest_fold_bounds(T, h, F)
    bt = device.backtest_block(y, lens, opts, folds, n_series=N)
    n_pairs = N * len(folds)
    pool = torch.from_numpy(rng.normal(0.0, 1.0, size=(n_pairs, 9))).to(env["dev"])
    g = device.paths_block(bt["yhat"], pool, n_paths=P, mode="cumulative", joint=False, seed=5, series_major=True, pool_series_major=True,
                           n_series=n_pairs)
    got = device.path_scores_block(g["paths"], bt["actual"], K.LEVELS, horizon=h, n_paths=P, n_cols=n_pairs, actual_series_major=True)
    torch.cuda.synchronize()
    actual = bt["actual"].cpu().numpy()
    assert actual.shape == (n_pairs, h) and 0 < np.isnan(actual).sum() < actual.size
    ref = R.scores(g["paths"].cpu().numpy(), actual, h, P, K.LEVELS, n_cols=n_pairs)
    _assert_scores(got, ref, n_pairs, "a backtest's actual block")
    assert (ref["column"][1] < h).any() and (ref["status"] != R.NAN).all()


# --------------------------------------------------------------------------------------------
# the end-to-end mirror
# --------------------------------------------------------------------------------------------
def test_ts_evaluate_quantiles_by(env):
    api = env["api"]
    n, T, h, F, P = 12, 36, 5, 8, 1000
    rng = np.random.default_rng(6)
    days = np.datetime64("2024-01-01") + np.arange(T)
    group, date, target = [], [], []
    order = (3, 0, 5, 1, 4, 2, 11, 7, 6, 10, 9, 8)
    for t in range(T):                                                  # interleaved rows
        for s in order:
            group.append(f"g{s}")
            date.append(days[t])
            target.append(10.0 * (s + 1) + 0.3 * t + float(rng.normal()))
    date, target = np.array(date), np.array(target)
    levels = [0.05, 0.25, 0.5, 0.75, 0.95]
    info = {}
    out = api.ts_evaluate_quantiles_by(group, date, target, "Naive", h, "1d", levels, residual_folds=F, n_paths=P, mode="cumulative", joint=True,
                                       seed=99, info=info)
    names = ["pinball_q0.05", "pinball_q0.25", "pinball_q0.5", "pinball_q0.75", "pinball_q0.95"]
    assert list(out) == ["id", "model_name", "crps"] + names + ["n_steps", "paths_status"]
    assert list(out["id"]) == [f"g{s}" for s in order] == info["groups"] and set(out["model_name"]) == {"Naive"}
    # the held-out rows are the last h of every series; the forecasts are those of the table without them
    per = {k: np.array([v for g_, v in zip(group, target) if g_ == k]) for k in info["groups"]}
    held = np.stack([per[k][-h:] for k in info["groups"]])
    _bits(info["actual"], held, "held-out rows")
    keep = np.array([d < days[T - h] for d in date])
    base = api.ts_forecast_by([g_ for g_, m in zip(group, keep) if m], date[keep], target[keep], "Naive", h, "1d")
    _bits(info["yhat"], np.asarray(base["yhat"]).reshape(n, h), "point forecasts")
    # the scores equal the restatement fed with the same paths
    block, wstatus = paths_ref.paths(info["yhat"], list(info["errors"]), P, "cumulative", True, seed=99)
    ref, e = R.scores(block, held, h, P, levels), R.energy(block, held, h, P, 0, n)
    assert wstatus.tolist() == [0] * n == info["series_status"].tolist() == list(out["paths_status"])
    _bits(out["crps"], ref["column"][0], "crps")
    for l, c in enumerate(names):
        _bits(out[c], ref["column"][2 + l], c)
    assert list(out["n_steps"]) == [h] * n and info["status"].tolist() == [0] * n
    _bits(info["crps"], ref["crps"], "crps per step")
    assert (info["below"] == ref["below"]).all() and (info["equal"] == ref["equal"]).all()
    _bits(info["quantiles"], ref["quantiles"], "quantiles")
    _bits(info["energy"], e["es"], "energy score of the leaves")
    assert info["energy_mean"] == e["es_mean"] and info["energy_steps"] == e["es_steps"] == h
    assert (out["crps"] > 0.0).all()
    with pytest.raises(api.InvalidInputException, match="exceeds the limit of 16 levels"):
        api.ts_evaluate_quantiles_by(group, date, target, "Naive", h, "1d", [0.5] * 17, residual_folds=F, n_paths=8)
    with pytest.raises(api.InvalidInputException, match="holds out 40 and needs at least one more"):
        api.ts_evaluate_quantiles_by(group, date, target, "Naive", 40, "1d", levels, n_paths=8)
