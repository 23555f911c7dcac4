"""GPU: the device backtest -- anofox_hip_backtest_expand_device / _collect_device (with the fold scores), anofox_hip_backtest_batch
behind api.ts_backtest_native_gpu, and device.backtest_block -- against the numpy restatement tests/backtest_ref.py,
backtest_metrics.backtest_metric and the host route api.ts_backtest_native.  The contract is equality of bits
with the host route: every comparison is == on the bits, NaN == NaN; no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import backtest_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
METRICS = ("mae", "mse", "mape", "smape", "bias", "r2", "coverage", "rmse", "no_such_metric")


@pytest.fixture(scope="module")
def env(hiplib):
    import torch
    assert torch.cuda.is_available()
    L = hiplib.load()
    from anofox_forecast_amd import api, device
    from anofox_forecast_amd.backtest_metrics import backtest_metric
    return {"torch": torch, "L": L, "lib": hiplib, "api": api, "device": device, "metric": backtest_metric, "dev": torch.device("cuda:0")}


def _edge_lengths(folds, T, n):
    """Lengths that hit every edge of every fold: len = train_end (dead), train_end + 1 (test_start >= len: dead), test_start + 1 (one
    test row), inside the test window, test_end + 1 (full), under 3 rows, the whole block."""
    cands = [0, 1, 2, T]
    for (_, tr0, tr1, te0, te1) in folds:
        cands += [tr1, tr1 + 1, te0, te0 + 1, te0 + 2, te1, te1 + 1, tr0 + 1]
    cands = [min(max(c, 0), T) for c in cands]
    return np.array([cands[i % len(cands)] for i in range(n)], dtype=np.int32)


def _expand_device(env, y, lengths, folds, n):
    torch, L, lib, dev = env["torch"], env["L"], env["lib"], env["dev"]
    tab = lib.make_folds(folds)
    t_train, n_pairs, ld_pairs = lib.backtest_sizes(tab, len(folds), n)
    yt = torch.from_numpy(y).to(dev)
    lt = torch.from_numpy(lengths).to(dev)
    out = torch.full((t_train, ld_pairs), SENTINEL, dtype=torch.float64, device=dev)
    len_pairs = torch.full((ld_pairs,), -5, dtype=torch.int32, device=dev)
    n_test = torch.full((ld_pairs,), -5, dtype=torch.int32, device=dev)
    err = lib.AnofoxError()
    torch.cuda.synchronize()
    ok = L.anofox_hip_backtest_expand_device(yt.data_ptr(), y.shape[1], lt.data_ptr(), n, y.shape[0], tab, len(folds), t_train, out.data_ptr(),
                                             ld_pairs, len_pairs.data_ptr(), n_test.data_ptr(), None, C.byref(err))
    assert ok, err.message
    return out.cpu().numpy(), len_pairs.cpu().numpy(), n_test.cpu().numpy()


@pytest.mark.parametrize("window", ["expanding", "fixed", "sliding"])
@pytest.mark.parametrize("n,n_folds", [(67, 3), (10, 7), (1, 1)])
def test_expand_against_reference(env, n, n_folds, window):
    T, h = 48, 4
    folds = env["api"].backtest_fold_bounds(T, h, n_folds, window, 5, 1, 2, -1, -1, True)
    assert len(folds) == n_folds
    rng = np.random.default_rng(100 * n + n_folds)
    ld = (n + 63) // 64 * 64
    y = rng.normal(size=(T, ld))
    lengths = _edge_lengths(folds, T, n) if n > 1 else np.array([T], dtype=np.int32)
    want_block, want_len, want_test = R.expand(y, lengths, folds, n)
    block, len_pairs, n_test = _expand_device(env, y, lengths, folds, n)
    assert np.array_equal(len_pairs, want_len) and np.array_equal(n_test, want_test)
    assert R.same_bits(block, want_block)
    # the zero fill: rows past the window, dead pairs, padding columns -- nothing of the sentinel is left
    assert not (block == SENTINEL).any() and not block[:, n * n_folds:].any()
    for p in range(n * n_folds):
        assert not block[want_len[p]:, p].any()
    if n > 1:
        live = want_len[:n * n_folds] > 0
        assert live.any() and (~live).any() and (want_test[:n * n_folds][live] < h).any() and (want_test[:n * n_folds][live] == h).any()


def _collect_device(env, y, folds, n, n_test, status, yhat, lower, upper, metric):
    torch, L, lib, dev = env["torch"], env["L"], env["lib"], env["dev"]
    tab = lib.make_folds(folds)
    F, h = len(folds), yhat.shape[1]
    n_pairs = n * F
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in
         {"y": y, "n_test": n_test, "status": status, "yhat": yhat, "lower": lower, "upper": upper}.items() if v is not None}
    outs = {k: torch.full((n_pairs, h), SENTINEL, dtype=torch.float64, device=dev) for k in ("actual", "error", "abs_error")}
    valid = torch.full((n_pairs, h), 9, dtype=torch.uint8, device=dev)
    n_rows = torch.full((n_pairs,), -5, dtype=torch.int32, device=dev)
    scores = torch.full((F,), SENTINEL, dtype=torch.float64, device=dev)
    err = lib.AnofoxError()
    ptr = lambda k: t[k].data_ptr() if k in t else None
    torch.cuda.synchronize()
    ok = L.anofox_hip_backtest_collect_device(ptr("y"), y.shape[1], n, y.shape[0], tab, F, ptr("n_test"), ptr("status"), ptr("yhat"), ptr("lower"),
                                              ptr("upper"), h, metric.encode(), outs["actual"].data_ptr(), outs["error"].data_ptr(),
                                              outs["abs_error"].data_ptr(), valid.data_ptr(), n_rows.data_ptr(), scores.data_ptr(), None,
                                              C.byref(err))
    assert ok, err.message
    return {**{k: v.cpu().numpy() for k, v in outs.items()}, "valid": valid.cpu().numpy(), "n_rows": n_rows.cpu().numpy(),
            "scores": scores.cpu().numpy()}


@pytest.fixture(scope="module")
def collect_case(env):
    """Hand-made yhat, status and n_test, no fit: six folds whose existing rows number 1, 63, 64, 65, 64 * h + 1 and 0 -- every tile
    edge of the score kernel -- with failing pairs in the middle of every fold, zeros in actual (mape's filter) and rows with
    |a| + |f| = 0 (smape's)."""
    T, h, n = 40, 4, 80
    folds = env["api"].backtest_fold_bounds(T, h, 6)
    assert len(folds) == 6 and folds[-1][4] < T
    F = len(folds)
    targets = [1, 63, 64, 65, 64 * h + 1, 0]
    rng = np.random.default_rng(77)
    ld = 128
    y = np.round(rng.normal(10.0, 4.0, size=(T, ld)), 3)
    y[rng.random((T, ld)) < 0.12] = 0.0
    n_test = np.zeros(n * F, dtype=np.int32)
    status = np.zeros(n * F, dtype=np.int32)
    for f, target in enumerate(targets):
        left = target
        for s in range(n):
            p = s * F + f
            if target and s % 7 == 3:                      # a failing pair between the others: its rows do not exist
                n_test[p], status[p] = h, 3 + s % 4
                continue
            if left > 0 and (target > 200 or s % 3 != 1):
                n_test[p] = min(h, left)
                left -= n_test[p]
        assert left == 0
    yhat = np.zeros((n * F, h))
    for s in range(n):
        for f, fold in enumerate(folds):
            yhat[s * F + f] = y[fold[3]:fold[3] + h, s] + np.round(rng.normal(0.0, 1.5, size=h), 3)
    zero = (yhat != 0) & (np.arange(n * F)[:, None] % 5 == 2)
    for s in range(n):                                       # rows with actual == 0 and a forecast of -0.0
        for f, fold in enumerate(folds):
            a = y[fold[3]:fold[3] + h, s]
            yhat[s * F + f][(a == 0) & zero[s * F + f]] = -0.0
    lower, upper = yhat - 1.0, yhat + 1.0
    return {"T": T, "h": h, "n": n, "F": F, "folds": folds, "targets": targets, "y": y, "n_test": n_test, "status": status, "yhat": yhat,
            "lower": lower, "upper": upper}


@pytest.mark.parametrize("metric", METRICS)
def test_collect_and_score_against_reference(env, collect_case, metric):
    c = collect_case
    n, F, h = c["n"], c["F"], c["h"]
    got = _collect_device(env, c["y"], c["folds"], n, c["n_test"], c["status"], c["yhat"], c["lower"], c["upper"], metric)
    actual, error, abs_error, valid, n_rows = R.collect(c["y"], c["folds"], n, c["n_test"], c["status"], c["yhat"])
    assert np.array_equal(got["n_rows"], n_rows) and np.array_equal(got["valid"], valid)
    assert R.same_bits(got["actual"], actual) and R.same_bits(got["error"], error) and R.same_bits(got["abs_error"], abs_error)
    assert [int(n_rows.reshape(n, F)[:, f].sum()) for f in range(F)] == c["targets"]
    saw_zero_actual = saw_zero_both = False
    for f in range(F):
        a, fc, lo, hi = R.fold_rows(f, F, n, n_rows, actual, c["yhat"], c["lower"], c["upper"])
        saw_zero_actual |= bool((a == 0).any())
        saw_zero_both |= bool(((np.abs(a) + np.abs(fc)) == 0).any())
        want = R.score(metric, a, fc, lo, hi)
        mirror = env["metric"](metric, a, fc, lo, hi)
        print(f"{metric} fold {f}: {len(a)} rows, device {got['scores'][f]!r}, reference {want!r}, backtest_metric {mirror!r}")
        assert R.same_bits(got["scores"][f:f + 1], np.array([want])) and R.same_bits(got["scores"][f:f + 1], np.array([mirror]))
    assert saw_zero_actual and saw_zero_both and np.isnan(got["scores"][F - 1])


def test_score_of_a_constant_actual_and_without_intervals(env, collect_case):
    c = collect_case
    n, F = c["n"], c["F"]
    y = np.full_like(c["y"], 3.5)
    got = _collect_device(env, y, c["folds"], n, c["n_test"], c["status"], c["yhat"], None, None, "r2")
    assert np.isnan(got["scores"]).all()                     # tot == 0 in every fold
    got = _collect_device(env, y, c["folds"], n, c["n_test"], c["status"], c["yhat"], None, None, "coverage")
    assert np.isnan(got["scores"]).all()                     # no lower / upper
    got = _collect_device(env, y, c["folds"], n, c["n_test"], c["status"], c["yhat"], c["lower"], c["upper"], "mae")
    actual, _, _, _, n_rows = R.collect(y, c["folds"], n, c["n_test"], c["status"], c["yhat"])
    for f in range(F):
        a, fc = R.fold_rows(f, F, n, n_rows, actual, c["yhat"])
        assert R.same_bits(got["scores"][f:f + 1], np.array([env["metric"]("mae", a, fc, None, None)]))


# ---------------------------------------------------------------------------------------------------------------------------
# the operator: api.ts_backtest_native_gpu against api.ts_backtest_native
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table():
    """40 groups of 20 .. 60 rows (one of them under the NULL group key), shuffled, with a few NULL values and one NULL-free copy of
    the dates per group: the short groups fall out of the later folds."""
    rng = np.random.default_rng(2024)
    group, date, value = [], [], []
    for g in range(40):
        n = 20 + (g * 7) % 41
        level = 20.0 + 3.0 * g
        v = level + np.cumsum(rng.normal(0.0, 1.0, size=n)) + 4.0 * np.sin(np.arange(n) * 2 * np.pi / 7)
        for t in range(n):
            group.append(None if g == 5 else f"g{g:02d}")
            date.append(t)
            value.append(None if (g == 9 and t == 11) else float(np.round(v[t], 4)))
    order = rng.permutation(len(group))
    return ([group[i] for i in order], np.array([date[i] for i in order], dtype=np.int64), [value[i] for i in order])


def _same_columns(a, b):
    assert list(a.keys()) == list(b.keys())
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, np.ndarray) and x.dtype == np.float64:
            assert R.same_bits(x, y), k
        elif isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and np.array_equal(x, y), k
        else:
            assert list(x) == list(y), k


@pytest.mark.parametrize("metric", ["rmse", "mape", "coverage"])
@pytest.mark.parametrize("window", ["expanding", "fixed", "sliding"])
@pytest.mark.parametrize("method", ["Naive", "SES", "AutoETS"])
def test_operator_equals_the_host_route(env, table, method, window, metric):
    group, date, value = table
    params = {"method": method, "window_type": window, "min_train_size": "12", "initial_train_size": "16", "skip_length": "9", "gap": "1"}
    want = env["api"].ts_backtest_native(group, date, value, horizon=4, folds=3, params=params, metric=metric)
    got = env["api"].ts_backtest_native_gpu(group, date, value, horizon=4, folds=3, params=params, metric=metric)
    _same_columns(got, want)
    assert len(want["yhat"]) > 100 and set(want["fold_id"]) == {1, 2, 3} and None in want["id"]
    per_fold = [int((want["fold_id"] == f).sum()) for f in (1, 2, 3)]
    assert per_fold[0] > per_fold[1] > per_fold[2]          # groups too short for the later folds


def test_operator_defaults_and_the_model_parameter(env, table):
    group, date, value = table
    api = env["api"]
    want = api.ts_backtest_native(group, date, value, horizon=4, folds=3, params={"method": "Naive"})
    got = api.ts_backtest_native_gpu(group, date, value, horizon=4, folds=3, params={"method": "Naive"})
    _same_columns(got, want)
    assert len(want["yhat"]) > 0
    params = {"method": "ETS", "model": "AAA"}               # "ETS:AAA": INVALID_MODEL on both routes, no rows
    want = api.ts_backtest_native(group, date, value, horizon=4, folds=3, params=params)
    got = api.ts_backtest_native_gpu(group, date, value, horizon=4, folds=3, params=params)
    _same_columns(got, want)
    assert len(got["yhat"]) == 0
    folds = api.backtest_fold_bounds(60, 4, 3)
    opts = env["lib"].make_options("ETS:AAA", 4, confidence_level=0.0, auto_detect=False)
    res, berr = api.backtest_batch([np.arange(60.0)], opts, folds)
    assert not berr["ok"] and berr["code"] == env["lib"].INVALID_MODEL and (res["n_rows"] == 0).all()


def _series_block(env, series):
    """Series of different lengths -> (time-major tensor [T, ld], lengths tensor)."""
    torch, dev = env["torch"], env["dev"]
    n, T = len(series), max(len(s) for s in series)
    ld = (n + 63) // 64 * 64
    y = np.zeros((T, ld))
    for s, v in enumerate(series):
        y[:len(v), s] = v
    return torch.from_numpy(y).to(dev), torch.from_numpy(np.array([len(s) for s in series], dtype=np.int32)).to(dev)


def test_backtest_block_with_a_seasonal_period(env):
    """Any option block is allowed on the device route: AutoETS with seasonal_period = 7 equals api.forecast_batch of the same windows
    cut on the host."""
    from anofox_forecast_amd import synth
    api, lib, device = env["api"], env["lib"], env["device"]
    n, T, h = 30, 70, 7
    Y = synth.gen_series(synth.SEED_M5, 0, n, T, 7, positive=False)
    folds = api.backtest_fold_bounds(T, h, 3)
    F = len(folds)
    assert F == 3
    opts = lib.make_options("AutoETS", h, seasonal_period=7)
    y, lens = _series_block(env, list(Y))
    r = device.backtest_block(y, lens, opts, folds, n_series=n, metric="mae")
    env["torch"].cuda.synchronize()
    windows = [Y[s, fold[1]:fold[2] + 1] for s in range(n) for fold in folds]
    want, berr = api.forecast_batch(windows, opts)
    assert berr["ok"], berr
    yhat, lower, upper, code, status = (r[k].cpu().numpy() for k in ("yhat", "lower", "upper", "model_code", "status"))
    assert (status == 0).all() and all(w["ok"] for w in want) and (r["n_rows"].cpu().numpy() == h).all()
    for p, w in enumerate(want):
        assert R.same_bits(yhat[p], w["point"]) and R.same_bits(lower[p], w["lower"]) and R.same_bits(upper[p], w["upper"]), p
        assert r["batch"].model_name(int(code[p]), p) == w["model_name"], p
    actual = r["actual"].cpu().numpy()
    for s in range(n):
        for f, fold in enumerate(folds):
            assert R.same_bits(actual[s * F + f], Y[s, fold[3]:fold[4] + 1])
    for f in range(F):
        a, fc = R.fold_rows(f, F, n, np.full(n * F, h), actual, yhat)
        assert R.same_bits(r["scores"].cpu().numpy()[f:f + 1], np.array([env["metric"]("mae", a, fc, None, None)]))


def _group_rows(cols, order, names):
    """Per group (in `order`) the rows of the host route's columns `names`, in the route's order (fold, then position)."""
    out = {k: [[] for _ in order] for k in names}
    at = {g: i for i, g in enumerate(order)}
    for r in range(len(cols["yhat"])):
        for k in names:
            out[k][at[cols["id"][r]]].append(cols[k][r])
    return {k: [np.array(v, dtype=np.float64) for v in out[k]] for k in names}


def test_chain_into_calibration_and_metrics(env):
    """actual, yhat and valid of a backtest_block result go, as [N, F * h] views and without a copy, into conformal_block and
    anofox_hip_metrics_device (drop_nan); both equal api.conformal_batch / api.metrics_batch on the rows api.ts_backtest_native
    returns for the same input."""
    torch, api, lib, device, L = env["torch"], env["api"], env["lib"], env["device"], env["L"]
    rng = np.random.default_rng(31)
    n, h, n_folds = 24, 4, 3
    lens = [10 if g % 8 == 7 else 20 + (g * 11) % 41 for g in range(n)]      # every eighth series is too short for any fold
    series = [np.round(30.0 + np.cumsum(rng.normal(0.0, 1.0, size=k)), 4) for k in lens]
    order = [f"s{g:02d}" for g in range(n)]
    group = [order[g] for g in range(n) for _ in range(lens[g])]
    date = np.array([t for g in range(n) for t in range(lens[g])], dtype=np.int64)
    value = [float(v) for s in series for v in s]
    params = {"method": "SES", "initial_train_size": "16", "skip_length": "9"}
    host = api.ts_backtest_native(group, date, value, horizon=h, folds=n_folds, params=params)
    folds = api.backtest_fold_bounds(max(lens), h, n_folds, "expanding", 1, 0, 0, 16, 9, False)
    F = len(folds)
    assert F == n_folds
    opts = lib.make_options("SES", h, confidence_level=0.0, auto_detect=False)
    y, lt = _series_block(env, series)
    r = device.backtest_block(y, lt, opts, folds, n_series=n)
    view = lambda t: t.view(n, F * h)
    actual, yhat, valid = view(r["actual"]), view(r["yhat"]), view(r["valid"])
    assert actual.data_ptr() == r["actual"].data_ptr() and yhat.data_ptr() == r["yhat"].data_ptr() and valid.is_contiguous()
    rows = _group_rows(host, order, ("actual", "yhat"))
    has_rows = np.array([len(a) > 0 for a in rows["actual"]])
    assert has_rows.any() and (~has_rows).any()
    assert np.array_equal(view(r["valid"]).cpu().numpy().sum(axis=1), [len(a) for a in rows["actual"]])

    # calibration: the residual is formed on the device as actual - forecast
    alphas = (0.1, 0.3)
    c = device.conformal_block(yhat, alphas, actual=actual, calibration_forecast=yhat, valid=valid, series_major=True)
    torch.cuda.synchronize()
    keep = np.nonzero(has_rows)[0]
    want = api.conformal_batch([rows["actual"][g] - rows["yhat"][g] for g in keep], [rows["yhat"][g] for g in keep], alphas)
    status, lower, upper = c["status"].cpu().numpy(), c["lower"].cpu().numpy(), c["upper"].cpu().numpy()
    mask = valid.cpu().numpy().astype(bool)
    assert (status[has_rows] == lib.CONFORMAL_OK).all() and (status[~has_rows] == lib.CONFORMAL_EMPTY).all()
    for j, g in enumerate(keep):
        assert want["code"][j] == 0
        assert R.same_bits(c["scores_lower"].cpu().numpy()[:, g], want["scores_lower"][j])
        for k in range(len(alphas)):
            assert R.same_bits(lower[k, g][mask[g]], want["lower"][j][k]) and R.same_bits(upper[k, g][mask[g]], want["upper"][j][k]), (g, k)

    # metrics: NaN marks the rows that do not exist, drop_nan skips them
    figures = ("mae", "rmse", "mape", "bias")
    bits = 0
    for f in figures:
        bits |= 1 << lib.METRIC_FIGURES.index(f)
    ld = 64
    fig = torch.full((len(lib.METRIC_FIGURES), ld), SENTINEL, dtype=torch.float64, device=env["dev"])
    mstatus = torch.full((n,), -5, dtype=torch.int32, device=env["dev"])
    full = torch.full((n,), F * h, dtype=torch.int32, device=env["dev"])
    err = lib.AnofoxError()
    ok = L.anofox_hip_metrics_device(actual.data_ptr(), yhat.data_ptr(), None, None, None, None, 0, None, 0, F * h, 1, full.data_ptr(), n, F * h,
                                     bits, 0.5, True, fig.data_ptr(), ld, mstatus.data_ptr(), None, C.byref(err))
    assert ok, err.message
    mwant = api.metrics_batch([rows["actual"][g] for g in keep], [rows["yhat"][g] for g in keep], figures=figures)
    got = fig.cpu().numpy()
    assert (mstatus.cpu().numpy()[has_rows] == 0).all() and (mstatus.cpu().numpy()[~has_rows] == 1).all()
    for f in figures:
        assert R.same_bits(got[lib.METRIC_FIGURES.index(f), keep], mwant[f]), f


def test_two_runs_give_the_same_bits(env, table):
    group, date, value = table
    api = env["api"]
    params = {"method": "AutoETS", "initial_train_size": "16", "skip_length": "9"}
    a = api.ts_backtest_native_gpu(group, date, value, horizon=4, folds=3, params=params, metric="smape")
    b = api.ts_backtest_native_gpu(group, date, value, horizon=4, folds=3, params=params, metric="smape")
    _same_columns(a, b)
    assert len(a["yhat"]) > 100
    rng = np.random.default_rng(8)
    series = [np.round(50.0 + np.cumsum(rng.normal(size=k)), 3) for k in (60, 44, 31, 60, 23, 52)]
    folds = api.backtest_fold_bounds(60, 4, 3, "fixed", 20, 1, 2, 24, 8, True)
    opts = env["lib"].make_options("AutoETS", 4, seasonal_period=4)
    runs = []
    for _ in range(2):
        y, lt = _series_block(env, series)
        r = env["device"].backtest_block(y, lt, opts, folds, n_series=len(series), metric="r2")
        env["torch"].cuda.synchronize()
        runs.append({k: r[k].cpu().numpy() for k in ("yhat", "lower", "upper", "actual", "error", "abs_error", "valid", "n_rows", "status",
                                                     "model_code", "scores", "len_pairs", "n_test", "train")})
    for k, x in runs[0].items():
        y = runs[1][k]
        assert R.same_bits(x, y) if x.dtype == np.float64 else np.array_equal(x, y), k
    assert (runs[0]["n_rows"] > 0).any()
