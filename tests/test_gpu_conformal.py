"""GPU: the conformal entries (anofox_hip_conformal_learn_device / _apply_device / _evaluate_device, anofox_hip_conformal_batch, the
reference's anofox_ts_conformal_* singles) and device.conformal_block against the restatement tests/conformal_ref.py.  The contract
 is equality of bits through every entry and both layouts; NaN compares by NaN-ness."""
import ctypes as C
import math
import random

import numpy as np
import pytest

import conformal_cases as CC
import conformal_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
PAD = 12345.0
METHODS = {"symmetric": 0, "asymmetric": 1, "adaptive": 2}


@pytest.fixture(scope="module")
def api(hiplib):
    import torch
    assert torch.cuda.is_available()
    hiplib.load()
    from anofox_forecast_amd import api as A
    return A


def _place(cols, layout, T, ld, n, t_pad, fill=PAD, dtype=np.float64):
    """Time-major ('tm': element (s, t) at t * ld + s) or series-major ('sm': at s * t_pad + t)."""
    if layout == "tm":
        m = np.full((T, ld), fill, dtype=dtype)
        for i, c in enumerate(cols):
            m[:len(c), i] = c
    else:
        m = np.full((n, t_pad), fill, dtype=dtype)
        for i, c in enumerate(cols):
            m[i, :len(c)] = c
    return m


def _take(block, layout, i, n):
    return block[:n, i] if layout == "tm" else block[i, :n]


def _learn(lib, layout, groups, alphas, method="symmetric", valids=None, actual_forecast=None, want_sorted=True, extra_cols=37, expect_ok=True):
    """anofox_hip_conformal_learn_device on torch tensors.  Returns (scores_lower, scores_upper [K x ld], sorted block, n_kept, status);
    the outputs start as a sentinel."""
    import torch
    L = lib.load()
    dev = "cuda:0"
    n = len(groups)
    T = max(1, max(len(g) for g in groups))
    ld = (n + extra_cols + 63) // 64 * 64
    t_pad = T + 3
    stride_s, stride_t = (1, ld) if layout == "tm" else (t_pad, 1)
    up = lambda cols, **kw: torch.from_numpy(_place(cols, layout, T, ld, n, t_pad, **kw)).to(dev)
    res = act = fc = None
    if actual_forecast is None:
        res = up(groups)
    else:
        act, fc = up(actual_forecast[0]), up(actual_forecast[1])
    val = None if valids is None else up([np.asarray(v, dtype=np.uint8) for v in valids], fill=1, dtype=np.uint8)
    lens = torch.from_numpy(np.array([len(g) for g in groups], dtype=np.int32)).to(dev)
    al = np.ascontiguousarray(alphas, dtype=np.float64)
    K = len(al)
    sl = torch.full((max(K, 1), ld), SENTINEL, dtype=torch.float64, device=dev)
    su = torch.full((max(K, 1), ld), SENTINEL, dtype=torch.float64, device=dev)
    srt = torch.full((T, ld) if layout == "tm" else (n, t_pad), SENTINEL, dtype=torch.float64, device=dev) if want_sorted else None
    kept = torch.full((n,), -5, dtype=torch.int32, device=dev)
    status = torch.full((n,), -5, dtype=torch.int32, device=dev)
    err = lib.AnofoxError()
    ptr = lambda t: None if t is None else t.data_ptr()
    torch.cuda.synchronize()
    ok = L.anofox_hip_conformal_learn_device(ptr(res), ptr(act), ptr(fc), ptr(val), stride_s, stride_t, lens.data_ptr(), n, T, al.ctypes.data, K,
                                             METHODS[method], sl.data_ptr(), su.data_ptr(), ld, ptr(srt), kept.data_ptr(), status.data_ptr(),
                                             None, C.byref(err))
    if not expect_ok:
        return ok, err.code, err.message.decode()
    assert ok, err.message
    return (sl.cpu().numpy(), su.cpu().numpy(), None if srt is None else srt.cpu().numpy(), kept.cpu().numpy(), status.cpu().numpy())


def _check_learn(got, layout, groups, alphas, method, valids=None, where=""):
    sl, su, srt, kept, status = got
    n, K = len(groups), len(alphas)
    bad = []
    for i, g in enumerate(groups):
        st, want_sorted, wl, wu, nk = CC.expect_learn(list(g), alphas, method, None if valids is None else valids[i])
        if status[i] != st or kept[i] != nk:
            bad.append((where, i, "status", int(status[i]), st, int(kept[i]), nk))
            continue
        for k in range(K):
            if not CC.same_bits(sl[k, i], wl[k]) or not CC.same_bits(su[k, i], wu[k]):
                bad.append((where, i, len(g), alphas[k], float(sl[k, i]), wl[k], float(su[k, i]), wu[k]))
        if srt is not None:
            row = _take(srt, layout, i, len(g))
            if want_sorted is None:
                want_sorted = []
            if any(not CC.same_bits(a, b) for a, b in zip(row[:len(want_sorted)], want_sorted)) or (row[len(want_sorted):] != SENTINEL).any():
                bad.append((where, i, len(g), "sorted"))
    assert not bad, bad[:6]
    # padding columns and cells beyond a group's rows keep their sentinel
    assert (sl[:, n:] == SENTINEL).all() and (su[:, n:] == SENTINEL).all()
    if srt is not None and layout == "tm":
        assert (srt[:, n:] == SENTINEL).all()


# --------------------------------------------------------------------------------------------
# learn: sorted output and scores, every tile boundary, both layouts
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("small", [False, True], ids=["to_4097", "to_140"])
@pytest.mark.parametrize("layout", ["tm", "sm"])
def test_learn_shapes(hiplib, layout, small):
    groups = CC.shape_batch(small)
    for method in ("symmetric", "asymmetric"):
        got = _learn(hiplib, layout, groups, CC.ALPHAS, method)
        _check_learn(got, layout, groups, CC.ALPHAS, method, where=(layout, small, method))


def test_learn_sixteen_levels_and_the_limit(hiplib):
    groups = CC.shape_batch(True)
    for method in ("symmetric", "asymmetric"):
        got = _learn(hiplib, "tm", groups, CC.ALPHAS16, method, want_sorted=False)
        _check_learn(got, "tm", groups, CC.ALPHAS16, method)
    ok, code, msg = _learn(hiplib, "tm", groups[:3], [0.1] * 17, expect_ok=False)
    assert not ok and code == hiplib.INVALID_INPUT and "at most 16" in msg and "17" in msg
    for bad in ([1.0], [-0.1], [math.nan], [0.1, 1.5]):
        ok, code, msg = _learn(hiplib, "tm", groups[:3], bad, expect_ok=False)
        assert not ok and code == hiplib.INVALID_INPUT and "Alpha must be in (0, 1)" in msg
    ok, code, msg = _learn(hiplib, "tm", groups[:3], [], expect_ok=False)
    assert not ok and code == hiplib.INVALID_INPUT and msg == R.NO_ALPHA


@pytest.mark.parametrize("layout", ["tm", "sm"])
@pytest.mark.parametrize("method", ["symmetric", "asymmetric", "adaptive"])
def test_learn_content(hiplib, layout, method):
    groups = [g for _, g in CC.content_groups()]
    got = _learn(hiplib, layout, groups, CC.ALPHAS, method)
    _check_learn(got, layout, groups, CC.ALPHAS, method, where=(layout, method))
    sl, su = got[0], got[1]
    names = [n for n, _ in CC.content_groups()]
    if method == "asymmetric":                   # a set that is empty gives 0.0
        assert (sl[:, names.index("all_positive")] == 0.0).all() and (su[:, names.index("all_negative")] == 0.0).all()
        assert (sl[:, names.index("all_zero")] == 0.0).all() and (su[:, names.index("only_minus_zero")] == 0.0).all()
    else:                                        # symmetric: both score rows hold one value
        assert np.array_equal(sl[:, :len(groups)], su[:, :len(groups)], equal_nan=True)


def test_nan_residual_and_masked_groups(hiplib):
    rng = random.Random(5)
    groups = [CC.residuals(rng, n) for n in (70, 5, 64, 130, 9, 300, 2)]
    groups[2][17] = math.nan                     # status 2 there, the neighbours untouched
    groups[5][299] = math.nan                    # ... but this one is masked away
    valids = [[1] * len(g) for g in groups]
    valids[1] = [0] * 5                          # emptied by its mask: status 1
    valids[3] = [int(rng.random() < 0.6) for _ in range(130)]
    valids[5][299] = 0
    valids[6] = [0, 1]
    for layout in ("tm", "sm"):
        for method in ("symmetric", "asymmetric"):
            got = _learn(hiplib, layout, groups, CC.ALPHAS, method, valids=valids)
            assert list(got[4]) == [0, 1, 2, 0, 0, 0, 0]
            _check_learn(got, layout, groups, CC.ALPHAS, method, valids=valids, where=(layout, method))
    # a length of 0 is an empty group as well
    got = _learn(hiplib, "tm", [[], [1.0, -2.0]], [0.1], "symmetric")
    assert list(got[4]) == [1, 0] and math.isnan(got[0][0, 0]) and got[0][0, 1] == 2.0


@pytest.mark.parametrize("layout", ["tm", "sm"])
def test_residuals_formed_on_the_device(hiplib, layout):
    rng = random.Random(11)
    sizes = (1, 28, 64, 140, 257, 2049)
    actual = [[rng.gauss(100.0, 30.0) for _ in range(n)] for n in sizes]
    forecast = [[a + rng.gauss(0.0, 5.0) for a in row] for row in actual]
    groups = [[a - f for a, f in zip(ra, rf)] for ra, rf in zip(actual, forecast)]
    for method in ("symmetric", "asymmetric"):
        ready = _learn(hiplib, layout, groups, CC.ALPHAS, method)
        formed = _learn(hiplib, layout, groups, CC.ALPHAS, method, actual_forecast=(actual, forecast))
        _check_learn(formed, layout, groups, CC.ALPHAS, method)
        for a, b in zip(ready, formed):
            assert np.array_equal(a, b, equal_nan=True)


def test_same_bits_on_two_runs(hiplib):
    groups = CC.shape_batch(False)
    a = _learn(hiplib, "tm", groups, CC.ALPHAS, "asymmetric")
    b = _learn(hiplib, "tm", groups, CC.ALPHAS, "asymmetric")
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


# --------------------------------------------------------------------------------------------
# apply
# --------------------------------------------------------------------------------------------
def _apply(lib, layout, forecasts, scores_lower, scores_upper, method, difficulty=None, use_lengths=True, extra_levels=1):
    """anofox_hip_conformal_apply_device; scores_* are [K][n] lists.  Returns (lower, upper blocks [K + extra x ...], status)."""
    import torch
    L = lib.load()
    dev = "cuda:0"
    n, K = len(forecasts), len(scores_lower)
    H = max(len(f) for f in forecasts)
    ld = (n + 63) // 64 * 64 + 64
    t_pad = H + 2
    stride_s, stride_t = (1, ld) if layout == "tm" else (t_pad, 1)
    f = torch.from_numpy(_place(forecasts, layout, H, ld, n, t_pad)).to(dev)
    d = None if difficulty is None else torch.from_numpy(_place(difficulty, layout, H, ld, n, t_pad, fill=-1.0)).to(dev)
    lens = torch.from_numpy(np.array([len(x) for x in forecasts], dtype=np.int32)).to(dev) if use_lengths else None
    sl = np.full((K, ld), PAD)
    su = np.full((K, ld), PAD)
    sl[:, :n] = scores_lower
    su[:, :n] = scores_upper
    sl, su = torch.from_numpy(sl).to(dev), torch.from_numpy(su).to(dev)
    lo = torch.full((K + extra_levels,) + tuple(f.shape), SENTINEL, dtype=torch.float64, device=dev)
    up = torch.full((K + extra_levels,) + tuple(f.shape), SENTINEL, dtype=torch.float64, device=dev)
    status = torch.full((n,), -5, dtype=torch.int32, device=dev)
    err = lib.AnofoxError()
    torch.cuda.synchronize()
    ok = L.anofox_hip_conformal_apply_device(f.data_ptr(), None if d is None else d.data_ptr(), stride_s, stride_t,
                                             None if lens is None else lens.data_ptr(), n, H, sl.data_ptr(), su.data_ptr(), ld, K, METHODS[method],
                                             lo.data_ptr(), up.data_ptr(), f.numel(), status.data_ptr(), None, C.byref(err))
    assert ok, err.message
    return lo.cpu().numpy(), up.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("layout", ["tm", "sm"])
@pytest.mark.parametrize("h", [1, 28, 65])
def test_apply(hiplib, layout, h):
    rng = random.Random(100 + h)
    n = 70
    alphas = [0.2, 0.1, 0.05]
    forecasts = [[rng.gauss(50.0, 20.0) for _ in range(h if i % 7 else max(1, h // 2))] for i in range(n)]
    res = [CC.residuals(rng, 5 + i) for i in range(n)]
    for method in ("symmetric", "asymmetric", "adaptive"):
        diff = None
        if method == "adaptive":
            diff = [[rng.uniform(0.1, 4.0) for _ in f] for f in forecasts]
            diff[3][0] = 0.0                     # not positive: status 3, NaN bounds
            diff[4][-1] = -1.0
        profiles = [R.conformal_learn(r, alphas, method, "split", [1.0] * len(r))[0] for r in res]
        sl = [[p["scores_lower"][k] for p in profiles] for k in range(3)]
        su = [[p["scores_upper"][k] for p in profiles] for k in range(3)]
        lo, up, status = _apply(hiplib, layout, forecasts, sl, su, method, diff)
        bad = []
        for i in range(n):
            want, e = R.conformal_apply(forecasts[i], profiles[i], None if diff is None else diff[i])
            hi = len(forecasts[i])
            if e is not None:
                assert e == R.DIFFICULTY and status[i] == CC.DIFFICULTY
                want = {"lower": [[math.nan] * hi] * 3, "upper": [[math.nan] * hi] * 3}
            else:
                assert status[i] == CC.OK
            for k in range(3):
                gl, gu = _take(lo[k], layout, i, H_of(lo[k], layout)), _take(up[k], layout, i, H_of(up[k], layout))
                if any(not CC.same_bits(a, b) for a, b in zip(gl[:hi], want["lower"][k])) or any(
                        not CC.same_bits(a, b) for a, b in zip(gu[:hi], want["upper"][k])):
                    bad.append((method, i, k))
                if (gl[hi:] != SENTINEL).any() or (gu[hi:] != SENTINEL).any():
                    bad.append((method, i, k, "beyond the group's steps"))
        assert not bad, bad[:6]
        # the level stride: the block after the last level, and the padding columns, keep their sentinel
        assert (lo[3] == SENTINEL).all() and (up[3] == SENTINEL).all()
        if layout == "tm":
            assert (lo[:, :, n:] == SENTINEL).all() and (up[:, :, n:] == SENTINEL).all()


def H_of(block, layout):
    return block.shape[0] if layout == "tm" else block.shape[1]


def test_apply_without_lengths(hiplib):
    rng = random.Random(3)
    forecasts = [[rng.gauss(0.0, 1.0) for _ in range(7)] for _ in range(5)]
    lo, up, status = _apply(hiplib, "sm", forecasts, [[1.5] * 5], [[0.25] * 5], "asymmetric", use_lengths=False)
    assert (status == 0).all()
    for i, f in enumerate(forecasts):
        assert [float(x) for x in lo[0][i, :7]] == [x - 1.5 for x in f] and [float(x) for x in up[0][i, :7]] == [x + 0.25 for x in f]


# --------------------------------------------------------------------------------------------
# evaluate
# --------------------------------------------------------------------------------------------
def _evaluate(lib, layout, actual, lower, upper, alpha, expect_ok=True):
    import torch
    L = lib.load()
    dev = "cuda:0"
    n = len(actual)
    T = max(1, max(len(a) for a in actual))
    ld = (n + 63) // 64 * 64 + 64
    t_pad = T + 1
    stride_s, stride_t = (1, ld) if layout == "tm" else (t_pad, 1)
    a, l, u = (torch.from_numpy(_place(c, layout, T, ld, n, t_pad)).to(dev) for c in (actual, lower, upper))
    lens = torch.from_numpy(np.array([len(x) for x in actual], dtype=np.int32)).to(dev)
    fig = torch.full((5, ld), SENTINEL, dtype=torch.float64, device=dev)
    status = torch.full((n,), -5, dtype=torch.int32, device=dev)
    err = lib.AnofoxError()
    torch.cuda.synchronize()
    ok = L.anofox_hip_conformal_evaluate_device(a.data_ptr(), l.data_ptr(), u.data_ptr(), stride_s, stride_t, lens.data_ptr(), n, T, alpha,
                                                fig.data_ptr(), ld, status.data_ptr(), None, C.byref(err))
    if not expect_ok:
        return ok, err.code, err.message.decode()
    assert ok, err.message
    return fig.cpu().numpy(), status.cpu().numpy()


def _eval_groups():
    rng = random.Random(77)
    actual, lower, upper = [], [], []
    for n in (1, 2, 28, 64, 65, 140, 0, 333):
        a = [round(rng.gauss(10.0, 4.0), 1) for _ in range(n)]
        l = [round(x - abs(rng.gauss(0.0, 3.0)), 1) if rng.random() < 0.8 else x + 0.5 for x in a]
        u = [round(max(x, y) + abs(rng.gauss(0.0, 3.0)), 1) if rng.random() < 0.8 else x - 0.5 for x, y in zip(a, l)]
        for j in range(0, n, 5):                 # rows ON a bound
            if j % 2:
                l[j] = a[j]
            else:
                u[j] = a[j]
        actual.append(a); lower.append(l); upper.append(u)
    return actual, lower, upper


@pytest.mark.parametrize("layout", ["tm", "sm"])
@pytest.mark.parametrize("alpha", [0.0, 1e-12, 0.1, 0.5, 0.999999])
def test_evaluate(hiplib, layout, alpha):
    actual, lower, upper = _eval_groups()
    fig, status = _evaluate(hiplib, layout, actual, lower, upper, alpha)
    n = len(actual)
    for i in range(n):
        want, e = R.conformal_evaluate(actual[i], lower[i], upper[i], alpha)
        if e is not None:
            assert e == R.EMPTY and status[i] == CC.EMPTY and all(math.isnan(fig[k, i]) for k in range(4)) and fig[4, i] == 0.0
            continue
        assert status[i] == CC.OK
        got = {k: float(fig[j, i]) for j, k in enumerate(hiplib.CONFORMAL_EVAL_FIGURES)}
        for k in ("coverage", "violation_rate", "mean_width", "winkler_score"):
            assert CC.same_bits(got[k], want[k]), (i, k, got[k], want[k])
        assert got["n_observations"] == want["n_observations"]
        assert got["violation_rate"] + got["coverage"] == 1.0
    assert (fig[:, n:] == SENTINEL).all()
    ok, code, msg = _evaluate(hiplib, layout, actual, lower, upper, 1.0, expect_ok=False)
    assert not ok and code == hiplib.INVALID_INPUT and msg == "Invalid input: Alpha must be in (0, 1), got 1"


# --------------------------------------------------------------------------------------------
# every entry gives the same bits
# --------------------------------------------------------------------------------------------
def _arr(x):
    return np.ascontiguousarray(x, dtype=np.float64)


def test_batch_entry_against_the_restatement(api):
    rng = random.Random(2024)
    groups = list(CC.shape_batch(True)[:40]) + [tuple(g) for _, g in CC.content_groups()] + [(), (1.0, math.nan)]
    n = len(groups)
    forecasts = [[rng.gauss(20.0, 5.0) for _ in range(1 + i % 9)] for i in range(n)]
    forecasts[5] = []
    alphas = [0.3, 0.1, 0.0]
    for method in ("symmetric", "asymmetric", "adaptive"):
        diff = [[rng.uniform(0.5, 2.0) for _ in f] for f in forecasts] if method == "adaptive" else None
        if diff:
            diff[7][0] = 0.0
        strategy = "split" if method == "asymmetric" else "jackknife+"
        r = api.conformal_batch([_arr(g) for g in groups], [_arr(f) for f in forecasts], alphas, method=method, strategy=strategy,
                                difficulty=None if diff is None else [_arr(d) for d in diff], want_sorted=True)
        for i in range(n):
            g = list(groups[i])
            if not g:
                want, e = None, R.EMPTY
            elif R.has_nan(g):
                want, e = None, "Invalid input: a residual is NaN"
            else:
                want, e = R.conformalize(g, forecasts[i], alphas, method, strategy, [1.0] * len(g), None if diff is None else diff[i])
            if e is not None:
                assert r["code"][i] != 0 and r["message"][i] == e and r["lower"][i] is None, (method, i, r["message"][i], e)
                continue
            assert r["code"][i] == 0, (method, i, r["message"][i])
            p, _ = R.conformal_learn(g, alphas, method, strategy, [1.0] * len(g))
            assert r["n_residuals"][i] == len(g)
            assert all(CC.same_bits(a, b) for a, b in zip(r["sorted"][i], R.sorted_abs(g))) and len(r["sorted"][i]) == len(g)
            for k in range(3):
                assert CC.same_bits(r["scores_lower"][i][k], p["scores_lower"][k]) and CC.same_bits(r["scores_upper"][i][k], p["scores_upper"][k])
                assert all(CC.same_bits(a, b) for a, b in zip(r["lower"][i][k], want["lower"][k])), (method, i, k)
                assert all(CC.same_bits(a, b) for a, b in zip(r["upper"][i][k], want["upper"][k])), (method, i, k)
    with pytest.raises(api.InvalidInputException, match="JackknifePlus strategy does not support asymmetric"):
        api.conformal_batch([_arr([1.0])], [_arr([1.0])], [0.1], method="asymmetric", strategy="jackknife+")
    with pytest.raises(api.InvalidInputException, match="at most 16"):
        api.conformal_batch([_arr([1.0])], [_arr([1.0])], [0.1] * 17)
    # NULL residuals are dropped
    r = api.conformal_batch([_arr([1.0, 50.0, -3.0, 2.0])], [_arr([10.0])], [0.0], valids=[[True, False, True, True]])
    assert r["n_residuals"][0] == 3 and r["scores_lower"][0][0] == 3.0 and r["upper"][0][0][0] == 13.0


def test_every_entry_gives_the_same_bits(api, hiplib):
    """Device entry, batch entry and the reference-signature singles on the same groups."""
    L = hiplib.load()
    rng = random.Random(9)
    groups = [CC.residuals(rng, n) for n in (1, 10, 64, 140, 300)]
    forecasts = [[rng.gauss(100.0, 10.0) for _ in range(28)] for _ in groups]
    diff = [[rng.uniform(0.2, 3.0) for _ in range(28)] for _ in groups]
    alphas = [0.2, 0.1, 0.05]
    al = _arr(alphas)
    err = hiplib.AnofoxError()
    for method in ("symmetric", "asymmetric", "adaptive"):
        dev = _learn(hiplib, "tm", groups, alphas, method)
        bat = api.conformal_batch([_arr(g) for g in groups], [_arr(f) for f in forecasts], alphas, method=method,
                                  difficulty=[_arr(d) for d in diff] if method == "adaptive" else None)
        for i, g in enumerate(groups):
            ga, fa, da = _arr(g), _arr(forecasts[i]), _arr(diff[i])
            # learn + apply through the reference's v2 pair
            prof = hiplib.CalibrationProfileFFI()
            ones = _arr([1.0] * len(g))
            assert L.anofox_ts_conformal_learn(ga.ctypes.data, None, len(g), al.ctypes.data, 3, METHODS[method], 0,
                                               ones.ctypes.data if method == "adaptive" else None, C.byref(prof), C.byref(err)), err.message
            iv = hiplib.PredictionIntervalsFFI()
            assert L.anofox_ts_conformal_apply(fa.ctypes.data, 28, C.byref(prof), da.ctypes.data if method == "adaptive" else None, C.byref(iv),
                                               C.byref(err)), err.message
            assert prof.n_levels == 3 and prof.n_residuals == len(g) and prof.state_vector_len == 6 and iv.n_forecasts == 28 and iv.n_levels == 3
            for k in range(3):
                assert CC.bits(prof.scores_lower[k]) == CC.bits(dev[0][k, i]) == CC.bits(bat["scores_lower"][i][k]) == CC.bits(prof.state_vector[k])
                assert CC.bits(prof.scores_upper[k]) == CC.bits(dev[1][k, i]) == CC.bits(bat["scores_upper"][i][k]) == CC.bits(prof.state_vector[3 + k])
                assert iv.coverage[k] == 1.0 - alphas[k]
                for t in range(28):
                    assert CC.bits(iv.lower[k * 28 + t]) == CC.bits(bat["lower"][i][k][t]) and CC.bits(iv.upper[k * 28 + t]) == CC.bits(bat["upper"][i][k][t])
            L.anofox_free_calibration_profile(C.byref(prof))
            L.anofox_free_prediction_intervals(C.byref(iv))
            # the v1 singles, level 1
            res = hiplib.ConformalResultFFI()
            if method == "symmetric":
                q = C.c_double()
                assert L.anofox_ts_conformal_quantile(ga.ctypes.data, None, len(g), alphas[1], C.byref(q), C.byref(err)), err.message
                assert CC.bits(q.value) == CC.bits(dev[0][1, i])
                assert L.anofox_ts_conformal_predict(ga.ctypes.data, None, len(g), fa.ctypes.data, 28, alphas[1], C.byref(res), C.byref(err)), err.message
                want_method, want_score = b"split_conformal", dev[0][1, i]
                multi = hiplib.ConformalMultiResultFFI()
                assert L.anofox_ts_conformal_predict_multi(ga.ctypes.data, None, len(g), fa.ctypes.data, 28, al.ctypes.data, 3, C.byref(multi),
                                                           C.byref(err)), err.message
                for k in range(3):
                    assert CC.bits(multi.conformity_scores[k]) == CC.bits(dev[0][k, i]) and multi.coverage_levels[k] == 1.0 - alphas[k]
                    assert all(CC.bits(multi.lower[k * 28 + t]) == CC.bits(bat["lower"][i][k][t]) for t in range(28))
                    assert all(CC.bits(multi.upper[k * 28 + t]) == CC.bits(bat["upper"][i][k][t]) for t in range(28))
                L.anofox_free_conformal_multi_result(C.byref(multi))
                lo_p, up_p = C.POINTER(C.c_double)(), C.POINTER(C.c_double)()
                assert L.anofox_ts_conformal_intervals(fa.ctypes.data, 28, q.value, C.byref(lo_p), C.byref(up_p), C.byref(err)), err.message
                assert all(CC.bits(lo_p[t]) == CC.bits(bat["lower"][i][1][t]) and CC.bits(up_p[t]) == CC.bits(bat["upper"][i][1][t]) for t in range(28))
                L.anofox_free_double_array(lo_p)
                L.anofox_free_double_array(up_p)
            elif method == "asymmetric":
                assert L.anofox_ts_conformal_predict_asymmetric(ga.ctypes.data, None, len(g), fa.ctypes.data, 28, alphas[1], C.byref(res),
                                                                C.byref(err)), err.message
                want_method, want_score = b"asymmetric_conformal", (float(dev[1][1, i]) + float(dev[0][1, i])) / 2.0
            else:
                assert L.anofox_ts_conformal_predict_adaptive(ga.ctypes.data, None, len(g), fa.ctypes.data, da.ctypes.data, 28, alphas[1], C.byref(res),
                                                              C.byref(err)), err.message
                want_method, want_score = b"adaptive_conformal", dev[0][1, i]
            assert res.method == want_method and res.n_forecasts == 28 and res.coverage == 1.0 - alphas[1]
            assert CC.bits(res.conformity_score) == CC.bits(float(want_score))
            for t in range(28):
                assert res.point[t] == forecasts[i][t]
                assert CC.bits(res.lower[t]) == CC.bits(bat["lower"][i][1][t]) and CC.bits(res.upper[t]) == CC.bits(bat["upper"][i][1][t])
            L.anofox_free_conformal_result(C.byref(res))
            # coverage / evaluate / mean width singles against the evaluate device entry
            act = _arr([f + r for f, r in zip(forecasts[i], CC.residuals(rng, 28))])
            lo_k, up_k = _arr(bat["lower"][i][1]), _arr(bat["upper"][i][1])
            fig, _ = _evaluate(hiplib, "sm", [list(act)], [list(lo_k)], [list(up_k)], alphas[1])
            ev = hiplib.ConformalEvaluationFFI()
            assert L.anofox_ts_conformal_evaluate(act.ctypes.data, lo_k.ctypes.data, up_k.ctypes.data, 28, alphas[1], C.byref(ev), C.byref(err)), err.message
            cov, mw = C.c_double(), C.c_double()
            assert L.anofox_ts_conformal_coverage(act.ctypes.data, lo_k.ctypes.data, up_k.ctypes.data, 28, C.byref(cov), C.byref(err))
            assert L.anofox_ts_mean_interval_width(lo_k.ctypes.data, up_k.ctypes.data, 28, C.byref(mw), C.byref(err))
            assert [CC.bits(ev.coverage), CC.bits(ev.violation_rate), CC.bits(ev.mean_width), CC.bits(ev.winkler_score)] == [CC.bits(fig[k, 0]) for k in range(4)]
            assert ev.n_observations == 28 and CC.bits(cov.value) == CC.bits(ev.coverage) and CC.bits(mw.value) == CC.bits(ev.mean_width)


def test_jackknife_profile_round_trip(hiplib):
    """Jackknife+ stores the sorted |r|; apply computes its scores from that vector and meets the split scores."""
    L = hiplib.load()
    rng = random.Random(4)
    g = CC.residuals(rng, 141)
    alphas = [0.5, 0.1]
    ga, al, fa = _arr(g), _arr(alphas), _arr([1.0, 2.0, 3.0])
    err = hiplib.AnofoxError()
    prof = hiplib.CalibrationProfileFFI()
    assert L.anofox_ts_conformal_learn(ga.ctypes.data, None, 141, al.ctypes.data, 2, 0, 2, None, C.byref(prof), C.byref(err)), err.message
    assert prof.state_vector_len == 141 and all(CC.same_bits(prof.state_vector[t], v) for t, v in enumerate(R.sorted_abs(g)))
    iv = hiplib.PredictionIntervalsFFI()
    assert L.anofox_ts_conformal_apply(fa.ctypes.data, 3, C.byref(prof), None, C.byref(iv), C.byref(err)), err.message
    want, e = R.conformalize(g, [1.0, 2.0, 3.0], alphas, "symmetric", "jackknife+")
    split, _ = R.conformalize(g, [1.0, 2.0, 3.0], alphas, "symmetric", "split")
    assert e is None and want == split
    for k in range(2):
        for t in range(3):
            assert CC.same_bits(iv.lower[k * 3 + t], want["lower"][k][t]) and CC.same_bits(iv.upper[k * 3 + t], want["upper"][k][t])
    L.anofox_free_calibration_profile(C.byref(prof))
    L.anofox_free_prediction_intervals(C.byref(iv))
    assert not prof.state_vector and not iv.lower


def test_single_entry_errors_on_the_device_path(hiplib):
    """The texts that need the kernel's answer: a NaN residual, and NULLs that leave nothing."""
    L = hiplib.load()
    err = hiplib.AnofoxError()
    q = C.c_double()
    g = _arr([1.0, math.nan, 2.0])
    assert not L.anofox_ts_conformal_quantile(g.ctypes.data, None, 3, 0.1, C.byref(q), C.byref(err))
    assert err.code == hiplib.COMPUTATION_ERROR and err.message.decode() == "Invalid input: a residual is NaN"
    mask = np.array([0b101], dtype=np.uint64)    # the NaN is NULL: dropped
    assert L.anofox_ts_conformal_quantile(g.ctypes.data, mask.ctypes.data, 3, 0.0, C.byref(q), C.byref(err)), err.message
    assert q.value == 2.0


# --------------------------------------------------------------------------------------------
# fit -> forecast -> calibrate -> score without leaving the device
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["Naive", "SES"])
def test_end_to_end_on_the_device(api, hiplib, model):
    import torch
    from anofox_forecast_amd import device, synth
    L = hiplib.load()
    n, T, h, cal = 64, 60, 7, 14
    Y = np.round(synth.gen_series(synth.SEED_M5, 0, n, T + cal + h, 7, positive=False), 1)
    opts = hiplib.make_options(model, h)
    b = device.DeviceBatch(n, T + cal, opts)
    y = torch.from_numpy(device.pack_time_major(Y[:, :T + cal], b.ld)).to(b.device)
    lens = torch.full((b.ld,), T + cal, dtype=torch.int32, device=b.device)
    b.set_block(y, lens)
    b.run()
    torch.cuda.synchronize()
    r = b.results()
    assert (r["status"].cpu().numpy() == 0).all()
    yhat = r["yhat"]                                                             # [n x h] series-major, on the device
    # calibration residuals from a held-out tail: the last `cal` rows against the value before them (a naive backtest), formed on the device
    actual_cal = torch.from_numpy(np.ascontiguousarray(Y[:, T:T + cal])).to(b.device)            # [n x cal] series-major
    fc_cal = torch.from_numpy(np.ascontiguousarray(np.repeat(Y[:, T - 1:T], cal, axis=1))).to(b.device)
    alphas = [0.2, 0.05]
    out = device.conformal_block(yhat, alphas, actual=actual_cal, calibration_forecast=fc_cal, series_major=True, n_groups=n)
    assert (out["status"].cpu().numpy() == 0).all() and (out["apply_status"].cpu().numpy() == 0).all()
    lower, upper = out["lower"].cpu().numpy(), out["upper"].cpu().numpy()      # [2 x n x h]
    point = yhat.cpu().numpy()
    host = api.conformal_batch([_arr(Y[i, T:T + cal] - Y[i, T - 1]) for i in range(n)], [_arr(point[i]) for i in range(n)], alphas)
    for i in range(n):
        assert host["code"][i] == 0
        for k in range(2):
            assert lower[k, i].tobytes() == host["lower"][i][k].tobytes() and upper[k, i].tobytes() == host["upper"][i][k].tobytes()
    # score the bounds where they lie: the metrics entry's coverage figure equals the evaluate kernel's
    actual = torch.from_numpy(np.ascontiguousarray(Y[:, T + cal:])).to(b.device)
    hl = torch.full((n,), h, dtype=torch.int32, device=b.device)
    ld = 128
    err = hiplib.AnofoxError()
    for k in range(2):
        fig = torch.full((12, ld), SENTINEL, dtype=torch.float64, device=b.device)
        ev = torch.full((5, ld), SENTINEL, dtype=torch.float64, device=b.device)
        st = torch.full((n,), -5, dtype=torch.int32, device=b.device)
        assert L.anofox_hip_metrics_device(actual.data_ptr(), None, None, out["lower"][k].data_ptr(), out["upper"][k].data_ptr(), None, 0, None, 0,
                                           h, 1, hl.data_ptr(), n, h, 1 << 11, 0.5, False, fig.data_ptr(), ld, st.data_ptr(), None, C.byref(err)), err.message
        assert L.anofox_hip_conformal_evaluate_device(actual.data_ptr(), out["lower"][k].data_ptr(), out["upper"][k].data_ptr(), h, 1, hl.data_ptr(),
                                                      n, h, alphas[k], ev.data_ptr(), ld, st.data_ptr(), None, C.byref(err)), err.message
        assert fig[11, :n].cpu().numpy().tobytes() == ev[0, :n].cpu().numpy().tobytes()
        for i in range(n):
            want, e = R.conformal_evaluate(Y[i, T + cal:].tolist(), lower[k, i].tolist(), upper[k, i].tolist(), alphas[k])
            assert e is None and CC.same_bits(float(ev[3, i]), want["winkler_score"]) and CC.same_bits(float(ev[0, i]), want["coverage"])
    b.close()


# --------------------------------------------------------------------------------------------
# the Python scalars and the table mirrors
# --------------------------------------------------------------------------------------------
KATS = CC.load_kats()
REF = CC.RefScalars()


@pytest.mark.parametrize("st", KATS["scalars"], ids=lambda st: f'{st["fn"]}@{st["src"].split("/")[-1]}')
def test_golden_scalars(api, st):
    ok, value = CC.golden_scalar(api, st)
    assert ok, (st["src"], value)


def test_golden_pairs_and_tables(api):
    for st in KATS["pairs"]:
        ok, value = CC.golden_pair(api, st)
        assert ok, (st["src"], value)
    for st in KATS["table_statements"]:
        for what, ok in CC.golden_table(api, KATS, st):
            assert ok, (st["src"], what)


def _same(got, want, where):
    """Nested lists / dicts / floats: equality of bits at the leaves."""
    if isinstance(want, dict):
        assert isinstance(got, dict) and set(got) == set(want), where
        for k in want:
            _same(got[k], want[k], where + (k,))
    elif isinstance(want, (list, tuple)):
        assert len(got) == len(want), where
        for i, (a, b) in enumerate(zip(got, want)):
            _same(a, b, where + (i,))
    elif isinstance(want, float):
        assert CC.same_bits(got, want), (where, got, want)
    else:
        assert got == want, (where, got, want)


def test_scalars_equal_the_restatement(api):
    rng = random.Random(42)
    for n in (1, 7, 64, 141):
        g = CC.residuals(rng, n) + [None]                     # a NULL cell is dropped
        f = [rng.gauss(5.0, 2.0) for _ in range(6)]
        for a in (0.0, 0.1, 0.5):
            _same(api.ts_conformal_quantile(g, a), REF.ts_conformal_quantile(g, a), ("quantile", n, a))
            _same(api.ts_conformal_predict(g, f, a), REF.ts_conformal_predict(g, f, a), ("predict", n, a))
            _same(api.ts_conformal_predict_asymmetric(g, f, a), REF.ts_conformal_predict_asymmetric(g, f, a), ("asymmetric", n, a))
        for method, strategy in (("symmetric", "split"), ("asymmetric", "crossval"), ("symmetric", "jackknife_plus"), ("Asymmetric", "Split")):
            got = api.ts_conformal_learn(g, [0.2, 0.05], method, strategy)
            want = REF.ts_conformal_learn(g, [0.2, 0.05], method.lower(), strategy.lower())
            _same(got, want, ("learn", n, method, strategy))
            _same(api.ts_conformal_apply(f, got), REF.ts_conformal_apply(f, want), ("apply", n, method, strategy))
        s = api.ts_conformal_quantile(g, 0.1)
        iv = api.ts_conformal_intervals(f, s)
        _same(iv, REF.ts_conformal_intervals(f, s), ("intervals", n))
        act = [x + rng.gauss(0.0, 3.0) for x in f]
        _same(api.ts_conformal_coverage(act, iv["lower"], iv["upper"]), REF.ts_conformal_coverage(act, iv["lower"], iv["upper"]), ("coverage", n))
        _same(api.ts_conformal_evaluate(act, iv["lower"], iv["upper"], 0.1), REF.ts_conformal_evaluate(act, iv["lower"], iv["upper"], 0.1), ("evaluate", n))
        _same(api.ts_mean_interval_width(iv["lower"], iv["upper"]), REF.ts_mean_interval_width(iv["lower"], iv["upper"]), ("width", n))


def test_table_mirrors_equal_the_restatement(api):
    rng = random.Random(8)
    n_rows = 400
    keys = [f"s{rng.randrange(9)}" for _ in range(n_rows)]
    null = lambda p: None if rng.random() < p else 1
    actual = [null(0.05) and round(rng.gauss(50.0, 10.0), 1) for _ in range(n_rows)]
    forecast = [null(0.05) and round(rng.gauss(50.0, 10.0), 1) for _ in range(n_rows)]
    point = [null(0.3) and round(rng.gauss(60.0, 10.0), 1) for _ in range(n_rows)]         # not in value order: the macro sorts them
    groups = {"series_id": keys}
    for params in (None, {"alpha": 0.2}, {"alpha": "0.05", "method": "asymmetric"}, {"method": "Asymmetric"}, {"alpha": 0.0}):
        got = api.ts_conformal_by(groups, actual, forecast, point, params)
        _same(got, REF.ts_conformal_by(groups, actual, forecast, point, params), ("by", str(params)))
        assert all(p == sorted(p) for p in got["point"])
        _same(api.ts_conformal_calibrate(actual, forecast, params), REF.ts_conformal_calibrate(actual, forecast, params), ("calibrate", str(params)))
    _same(api.ts_conformal_apply_by(groups, point, 2.5), REF.ts_conformal_apply_by(groups, point, 2.5), ("apply_by",))
    lower = [None if p is None else p - abs(rng.gauss(0.0, 2.0)) for p in point]
    upper = [None if (p is None and rng.random() < 0.5) else (p or 60.0) + abs(rng.gauss(0.0, 2.0)) for p in point]
    got = api.ts_interval_width_by(groups, lower, upper)
    _same(got, REF.ts_interval_width_by(groups, lower, upper), ("width_by",))
    # the mirror of ts_conformal_by is the batch entry: the same bits as the single entries, group by group
    by = api.ts_conformal_by(groups, actual, forecast, point, {"alpha": 0.2})
    for i, g in enumerate(by["series_id"]):
        res = [a - f for k, a, f in zip(keys, actual, forecast) if k == g and a is not None and f is not None]
        pts = sorted(p for k, p in zip(keys, point) if k == g and p is not None)
        _same(api.ts_conformal_predict(res, pts, 0.2), {c: by[c][i] for c in ("point", "lower", "upper", "coverage", "conformity_score", "method")},
              ("single", g))


def test_conformal_block_time_major(hiplib):
    """device.conformal_block on time-major blocks: a validity mask, ragged lengths, the adaptive method and the sorted output."""
    import torch
    from anofox_forecast_amd import device
    rng = random.Random(12)
    n, T, h, ld = 70, 33, 5, 128
    lens = [T if i % 3 else 1 + i % T for i in range(n)]
    groups = [CC.residuals(rng, m) for m in lens]
    valids = [[int(rng.random() < 0.8) for _ in g] for g in groups]
    valids[4] = [0] * len(valids[4])
    forecasts = [[rng.gauss(10.0, 2.0) for _ in range(h)] for _ in range(n)]
    diff = [[rng.uniform(0.5, 2.0) for _ in range(h)] for _ in range(n)]
    dev = "cuda:0"
    up = lambda cols, rows, **kw: torch.from_numpy(_place(cols, "tm", rows, ld, n, 0, **kw)).to(dev)
    alphas = [0.3, 0.05]
    out = device.conformal_block(up(forecasts, h), alphas, residual=up(groups, T), valid=up(valids, T, fill=1, dtype=np.uint8),
                                 lengths=torch.tensor(lens, dtype=torch.int32, device=dev), n_groups=n, method="adaptive",
                                 difficulty=up(diff, h, fill=1.0), want_sorted=True)
    lo, hi, srt = out["lower"].cpu().numpy(), out["upper"].cpu().numpy(), out["sorted"].cpu().numpy()
    status, kept = out["status"].cpu().numpy(), out["n_kept"].cpu().numpy()
    for i in range(n):
        g = [r for r, v in zip(groups[i], valids[i]) if v]
        assert kept[i] == len(g) and status[i] == (CC.OK if g else CC.EMPTY)
        if not g:
            assert np.isnan(lo[:, :h, i]).all() and np.isnan(hi[:, :h, i]).all()
            continue
        want, e = R.conformalize(g, forecasts[i], alphas, "adaptive", "split", [1.0] * len(g), diff[i])
        assert e is None and all(CC.same_bits(a, b) for a, b in zip(srt[:len(g), i], R.sorted_abs(g)))
        for k in range(2):
            assert all(CC.same_bits(a, b) for a, b in zip(lo[k, :, i], want["lower"][k])) and all(CC.same_bits(a, b) for a, b in zip(hi[k, :, i], want["upper"][k]))
    assert (out["apply_status"].cpu().numpy() == 0).all()
