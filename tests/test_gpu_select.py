"""GPU: the selection entries -- anofox_hip_select_winner_device (winner + stable partition), _gather_device, _scatter_device,
_combine_device, anofox_hip_select_batch behind api.select_batch / api.ts_forecast_best_by / api.ts_compare_models_by, and
device.select_block -- against the pure-Python restatement tests/select_ref.py, tests/metrics_ref.py and tests/conformal_ref.py.
The contract (DESIGN.md section 3 "Selection") is equality of bits: every comparison is == on the bits, NaN == NaN; no tolerance
anywhere."""
import ctypes as C

import numpy as np
import pytest

import conformal_ref as CR
import metrics_ref as MR
import select_cases as K
import select_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -777.0


@pytest.fixture(scope="module")
def env(hiplib):
    import torch
    assert torch.cuda.is_available()
    L = hiplib.load()
    from anofox_forecast_amd import api, device
    return {"torch": torch, "L": L, "lib": hiplib, "api": api, "device": device, "dev": torch.device("cuda:0")}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64)))


def same_scores(a, b):
    """Scores against tests/metrics_ref.py: equal bits, except that zeros compare by == (the sign of a zero result is outside the
    metrics contract; the choice treats -0.0 and +0.0 alike)."""
    a, b = np.array(a, dtype=np.float64), np.array(b, dtype=np.float64)
    a[a == 0.0] = 0.0
    b[b == 0.0] = 0.0
    return same_bits(a, b)


# --------------------------------------------------------------------------------------------
# winner + partition alone
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 3, 16])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000, 70000])
def test_winner_and_partition(env, N, M):
    """Synthetic score tables, no fit.  70,000 series are 274 workgroups: with 16 methods the scan runs over 4,385 counts, more than
    one workgroup has lanes and more than one scan chunk."""
    torch, device, dev = env["torch"], env["device"], env["dev"]
    scores, status = K.score_table(N, M, 1000 * N + M)
    for fallback in (-1, 0):
        p = K.table_properties(scores, status, N, M, fallback)
        if fallback == -1 and N >= 63:                       # the inputs are what the test is about
            lose = K.loser_of(M)
            assert all(p["wins"][m] >= 1 for m in range(M) if m != lose) and (lose < 0 or p["wins"][lose] == 0)
            assert p["n_nan"] > 0 and p["n_inf"] > 0 and p["n_status"] > 0 and p["n_none"] > 0
            if M >= 3:
                assert 20 * p["ties"] >= N and p["three_way"] >= 1 and p["zero_tie"] >= 1
        got = device.select_winner_block(torch.from_numpy(scores).to(dev), torch.from_numpy(status).to(dev), fallback, n_series=N)
        torch.cuda.synchronize()
        offsets = got["offsets"].cpu().numpy()
        assert np.array_equal(got["winner"].cpu().numpy(), np.array(p["winner"], dtype=np.int32))
        assert same_bits(got["best_score"].cpu().numpy(), np.array(p["best"]))
        assert np.array_equal(got["from_fallback"].cpu().numpy(), np.array(p["from_fallback"], dtype=np.uint8))
        assert offsets.tolist() == p["offsets"]
        members = got["members"].cpu().numpy()
        assert members[:offsets[M]].tolist() == p["members"] and (members[offsets[M]:] == -1).all()      # nothing written past the end


# --------------------------------------------------------------------------------------------
# gather / scatter alone
# --------------------------------------------------------------------------------------------
def _member_cases(N):
    edge = [s for s in (0, 1, 62, 63, 64, 65, 127, 128, 191, 255, 256, 257, N - 2, N - 1) if 0 <= s < N]
    half = sorted(set(edge) | set(range(3, N, 2)))
    rest = [s for s in range(N) if s not in set(half)]
    return {"straddle": half, "rest": rest, "none": [], "all": list(range(N))}


@pytest.mark.parametrize("t_rows", [1, 50])
@pytest.mark.parametrize("which", ["straddle", "none", "all"])
def test_gather(env, t_rows, which):
    torch, device, dev = env["torch"], env["device"], env["dev"]
    N, ld_src = 300, 384
    rng = np.random.default_rng(t_rows)
    y = rng.normal(size=(t_rows, ld_src))
    lengths = rng.integers(0, t_rows + 1, size=ld_src).astype(np.int32)
    lengths[5] = t_rows + 9                                  # cut to t_rows
    m = _member_cases(N)[which]
    off = 0 if which == "all" else 7                       # (off + n_m stays within the n_series entries a partition has)
    members = np.array([N - 1] * off + m + [0, 0, 0], dtype=np.int32)      # what lies around the range is not read as a member
    n_m = len(m)
    ld_m = max((n_m + 63) // 64 * 64, 64)
    assert ld_m != ld_src
    out = {"y": torch.full((t_rows, ld_m), SENTINEL, dtype=torch.float64, device=dev),
           "lengths": torch.full((ld_m,), -5, dtype=torch.int32, device=dev)}
    g = device.select_gather_block(torch.from_numpy(y).to(dev), torch.from_numpy(lengths).to(dev), torch.from_numpy(members).to(dev), off, n_m,
                                   n_series=N, out=out)
    torch.cuda.synchronize()
    ym, lm = g["y"].cpu().numpy(), g["lengths"].cpu().numpy()
    want_y, want_l = R.gather(y.tolist(), lengths.tolist(), members.tolist(), off, n_m, ld_m)
    assert same_bits(ym, np.array(want_y).reshape(t_rows, ld_m)) and lm.tolist() == want_l
    assert not (ym == SENTINEL).any() and not ym[:, n_m:].any() and not lm[n_m:].any() and (lm >= 0).all() and (lm <= t_rows).all()
    if which == "straddle":
        assert n_m > 64 and {63, 64, 255, 256} <= set(m)


@pytest.mark.parametrize("h", [1, 3])
def test_scatter(env, h):
    torch, device, lib, dev = env["torch"], env["device"], env["lib"], env["dev"]
    N = 300
    cases = _member_cases(N)
    unchosen = [s for s in cases["rest"] if s % 5 == 0]
    second = [s for s in cases["rest"] if s % 5 != 0]
    parts = [cases["straddle"], [], second]
    members = np.array([s for p in parts for s in p], dtype=np.int32)
    winner = np.zeros(N, dtype=np.int32)
    winner[second] = 2
    winner[unchosen] = -1
    rng = np.random.default_rng(h)
    out = {k: torch.full((N, h), SENTINEL, dtype=torch.float64, device=dev) for k in ("yhat", "lower", "upper")}
    out.update({k: torch.full((N,), -5, dtype=torch.int32, device=dev) for k in ("model_code", "status")})
    want = {k: np.full((N, h), np.nan) for k in ("yhat", "lower", "upper")}
    want.update({"model_code": np.zeros(N, dtype=np.int32), "status": np.full(N, lib.INSUFFICIENT_DATA, dtype=np.int32)})
    mt = torch.from_numpy(members).to(dev)
    off = 0
    for p in parts:
        n_m = len(p)
        sub = {k: rng.normal(size=(n_m + 2, h)) for k in ("yhat", "lower", "upper")}       # two rows more than n_m: not scattered
        sub.update({"model_code": rng.integers(1, 200, size=n_m + 2).astype(np.int32), "status": rng.integers(0, 4, size=n_m + 2).astype(np.int32)})
        for k in want:
            if n_m:
                want[k][p] = sub[k][:n_m]
        device.select_scatter_block({k: torch.from_numpy(v).to(dev) for k, v in sub.items()} if n_m else None, mt, off, n_m, out)
        off += n_m
    device.select_scatter_block(None, mt, 0, 0, out, winner=torch.from_numpy(winner).to(dev))
    torch.cuda.synchronize()
    assert len(unchosen) > 5 and off + len(unchosen) == N
    for k in ("yhat", "lower", "upper"):
        got = out[k].cpu().numpy()
        assert not (got == SENTINEL).any() and same_bits(got, want[k]), k
    for k in ("model_code", "status"):
        assert np.array_equal(out[k].cpu().numpy(), want[k]), k


# --------------------------------------------------------------------------------------------
# combine alone
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group_div", [1, 2])
@pytest.mark.parametrize("h", [1, 3])
@pytest.mark.parametrize("R_rows", [1, 65, 300])
def test_combine(env, R_rows, h, group_div):
    torch, device, dev = env["torch"], env["device"], env["dev"]
    M = 16
    blocks, status, scores, winner = K.combine_case(R_rows, h, M, group_div, 7 * R_rows + h)
    if R_rows >= 8:                                          # live counts 0, 1, 2 and 16, a zero score, NaN cells inside live members
        live = {int(((status[:, r] == 0) & ~np.isnan(blocks[:, r, i])).sum()) for r in range(R_rows) for i in range(h)}
        assert {0, 1, 2, 16} <= live and (scores == 0.0).any() and np.isnan(blocks[status == 0]).any()
    tb = [torch.from_numpy(np.ascontiguousarray(blocks[m])).to(dev) for m in range(M)]
    ts, tw, tsc = torch.from_numpy(status).to(dev), torch.from_numpy(winner).to(dev), torch.from_numpy(scores).to(dev)
    for mode in R.MODES:
        got = device.combine_block(tb, mode, status=ts, winner=tw if mode == "pick" else None,
                                   weights=tsc if mode == "inverse_score" else None, group_div=group_div)
        torch.cuda.synchronize()
        want, want_status = R.combine(blocks.tolist(), status.tolist(), mode, winner=winner.tolist(), scores=scores.tolist(), group_div=group_div)
        assert same_bits(got["y"].cpu().numpy(), np.array(want).reshape(R_rows, h)), mode
        assert got["row_status"].cpu().numpy().tolist() == want_status, mode
    # pick is row-wise indexing
    got = device.combine_block(tb, "pick", status=ts, winner=tw, group_div=group_div)["y"].cpu().numpy()
    for r in range(R_rows):
        w = winner[r // group_div]
        assert same_bits(got[r], blocks[w, r] if w >= 0 else np.full(h, np.nan))
    # fewer than 16 members: the padding of the median's network takes no part
    got3 = device.combine_block(tb[:3], "median", status=ts[:3].contiguous())
    want3, _ = R.combine(blocks[:3].tolist(), status[:3].tolist(), "median")
    assert same_bits(got3["y"].cpu().numpy(), np.array(want3).reshape(R_rows, h))


# --------------------------------------------------------------------------------------------
# end to end
# --------------------------------------------------------------------------------------------
def _edge_lengths(folds, T, n):
    """Lengths that hit every edge of every fold (as tests/test_gpu_backtest.py): dead pairs, one test row, full windows, tiny series."""
    cands = [0, 1, 2, T]
    for (_, tr0, tr1, te0, te1) in folds:
        cands += [tr1, tr1 + 1, te0, te0 + 1, te0 + 2, te1, te1 + 1, tr0 + 1]
    cands = [min(max(c, 0), T) for c in cands]
    return np.array([cands[i % len(cands)] for i in range(n)], dtype=np.int32)


def _series(n, T, seed):
    """Four kinds of series so that several methods win: random walks, noisy levels, period-4 seasonal, intermittent counts."""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, T))
    for s in range(n):
        kind = s % 4
        if kind == 0:
            out[s] = 50.0 + np.cumsum(rng.normal(0.0, 2.0, size=T))
        elif kind == 1:
            out[s] = 30.0 + rng.normal(0.0, 3.0, size=T)
        elif kind == 2:
            out[s] = 40.0 + np.tile([8.0, -3.0, -9.0, 4.0], T // 4 + 1)[:T] * (1.0 + s / n) + rng.normal(0.0, 0.5, size=T)
        else:
            out[s] = np.where(rng.random(T) < 0.3, rng.integers(1, 6, size=T), 0).astype(np.float64)
    return np.round(out, 3)


def _block(env, Y, lengths):
    torch, dev = env["torch"], env["dev"]
    n, T = Y.shape
    ld = (n + 63) // 64 * 64
    y = np.zeros((T, ld))
    for s in range(n):
        y[:lengths[s], s] = Y[s, :lengths[s]]
    lens = np.zeros(ld, dtype=np.int32)
    lens[:n] = lengths
    return torch.from_numpy(y).to(dev), torch.from_numpy(lens).to(dev)


SEASONAL = ("SeasonalNaive", "HoltWinters", "AutoETS")      # the others refuse a seasonal_period


def _methods(lib, h, names):
    return [lib.make_options(m, h, seasonal_period=4 if m in SEASONAL else 0, auto_detect=False) for m in names]


def _to_numpy(r):
    keys = ("winner", "best_score", "from_fallback", "scores", "score_status", "members", "yhat", "lower", "upper", "model_code", "status")
    out = {k: r[k].cpu().numpy() for k in keys}
    out["offsets"] = np.asarray(r["offsets"])
    out.update({"bt_" + k: v.cpu().numpy() for k, v in r["selected_backtest"].items()})
    return out


def _check_pick(env, case, names, fallback, metric="rmse"):
    """Everything the contract says about pick mode, on one block."""
    torch, lib, device, api = env["torch"], env["lib"], env["device"], env["api"]
    Y, lengths, folds, h = case["Y"], case["lengths"], case["folds"], case["h"]
    n, T = Y.shape
    F, M = len(folds), len(names)
    methods = _methods(lib, h, names)
    y, lens = _block(env, Y, lengths)
    r = device.select_block(y, lens, methods, folds, metric=metric, mode="pick", fallback=fallback, n_series=n)
    torch.cuda.synchronize()
    got = _to_numpy(r)
    # scores == metrics_ref over the existing rows of every series' F * h backtest cells
    scores_want = np.full((M, n), np.nan)
    status_want = np.ones((M, n), dtype=np.int32)
    for m, bt in enumerate(r["backtests"]):
        a, f = bt["actual"].cpu().numpy().reshape(n, F * h), bt["yhat"].cpu().numpy().reshape(n, F * h)
        for s in range(n):
            keep = ~np.isnan(a[s]) & ~np.isnan(f[s])
            if keep.any():
                scores_want[m, s] = getattr(MR, metric)(a[s][keep].tolist(), f[s][keep].tolist())
                status_want[m, s] = 0
    assert same_scores(got["scores"][:, :n], scores_want) and np.array_equal(got["score_status"], status_want)
    # the choice == select_ref
    winner, best, ff, offsets, members = R.choose(scores_want.tolist(), status_want.tolist(), fallback)
    assert got["winner"].tolist() == winner and same_scores(got["best_score"], np.array(best)) and got["from_fallback"].tolist() == ff
    assert got["offsets"].tolist() == offsets and got["members"][:offsets[M]].tolist() == members
    none = [s for s in range(n) if best[s] != best[s]]
    assert none, "some series have no live pair"
    # every final row == the whole-block run of its winner, column s
    names_got = [""] * n
    for (m, off, n_m, batch) in r["sub_batches"]:
        code = batch.results()["model_code"].cpu().numpy()
        for j in range(n_m):
            names_got[members[off + j]] = batch.model_name(int(code[j]), j)
    for m in range(M):
        whole = device.DeviceBatch(n, T, methods[m], env["dev"])
        whole.set_block(y, lens)
        whole.run()
        torch.cuda.synchronize()
        w = {k: v.cpu().numpy() for k, v in whole.results().items()}
        for s in [s for s in range(n) if winner[s] == m]:
            for k in ("yhat", "lower", "upper"):
                assert same_bits(got[k][s], w[k][s]), (m, s, k)
            assert got["model_code"][s] == w["model_code"][s] and got["status"][s] == w["status"][s], (m, s)
            assert names_got[s] == whole.model_name(int(w["model_code"][s]), s), (m, s)
    for s in [s for s in range(n) if winner[s] < 0]:
        assert np.isnan(got["yhat"][s]).all() and np.isnan(got["lower"][s]).all() and got["status"][s] == lib.INSUFFICIENT_DATA
    # selected_backtest == row-wise indexing of the methods' backtests
    for key in ("yhat", "actual"):
        per = np.stack([bt[key].cpu().numpy() for bt in r["backtests"]])
        want = np.full((n * F, h), np.nan)
        for p in range(n * F):
            if winner[p // F] >= 0:
                want[p] = per[winner[p // F], p]
        assert same_bits(got["bt_" + key], want), key
    valid = ~np.isnan(got["bt_yhat"]) & ~np.isnan(got["bt_actual"])
    assert np.array_equal(got["bt_valid"].astype(bool), valid) and np.array_equal(got["bt_n_rows"], valid.sum(1))
    # conformal_block takes selected_backtest as it lies
    sb = r["selected_backtest"]
    view = lambda t: t.view(n, F * h)
    alphas = (0.1, 0.3)
    c = device.conformal_block(r["yhat"], alphas, actual=view(sb["actual"]), calibration_forecast=view(sb["yhat"]), valid=view(sb["valid"]),
                               series_major=True)
    torch.cuda.synchronize()
    lower, upper, cstatus = c["lower"].cpu().numpy(), c["upper"].cpu().numpy(), c["status"].cpu().numpy()
    a2, f2, v2 = got["bt_actual"].reshape(n, F * h), got["bt_yhat"].reshape(n, F * h), valid.reshape(n, F * h)
    checked = 0
    for s in range(n):
        if not v2[s].any():
            assert cstatus[s] == lib.CONFORMAL_EMPTY
            continue
        resid = [float(a - f) for a, f in zip(a2[s][v2[s]], f2[s][v2[s]])]
        for k, alpha in enumerate(alphas):
            want_c, e = CR.conformal_predict(resid, got["yhat"][s].tolist(), alpha)
            assert e is None and same_bits(lower[k, s], np.array(want_c["lower"])) and same_bits(upper[k, s], np.array(want_c["upper"])), (s, k)
        checked += 1
    assert checked > n // 2
    return {"got": got, "names": names_got, "winner": winner, "methods": methods}


@pytest.fixture(scope="module")
def case(env):
    T, h, n = 60, 3, 67
    folds = env["api"].backtest_fold_bounds(T, h, 3)
    assert len(folds) == 3
    return {"Y": _series(n, T, 5), "lengths": _edge_lengths(folds, T, n), "folds": folds, "h": h}


NAMES = ("Naive", "SES", "SeasonalNaive", "CrostonSBA", "HoltWinters")


def test_end_to_end_pick(env, case):
    lib, api = env["lib"], env["api"]
    res = _check_pick(env, case, NAMES, -1)
    got, winner = res["got"], res["winner"]
    assert len({w for w in winner if w >= 0}) >= 3, "at least three methods win something"
    Y, lengths, folds, h = case["Y"], case["lengths"], case["folds"], case["h"]
    n = len(Y)
    series = [Y[s, :lengths[s]] for s in range(n)]
    # the same bits through the host-buffer entry ...
    b, err = api.select_batch(series, res["methods"], folds, "rmse", "pick", -1)
    assert err["ok"], err
    assert b["winner"].tolist() == winner and same_bits(b["best_score"], got["best_score"]) and same_bits(b["scores"], got["scores"][:, :n])
    for k in ("yhat", "lower", "upper"):
        assert same_bits(b[k], got[k]), k
    assert np.array_equal(b["status"], got["status"]) and b["model_name"] == [nm if st == 0 else "" for nm, st in zip(res["names"], got["status"])]
    assert same_bits(b["backtest_yhat"], got["bt_yhat"]) and same_bits(b["backtest_actual"], got["bt_actual"])
    assert np.array_equal(b["n_rows"], got["bt_n_rows"])
    # ... a second run ...
    again = _check_pick(env, case, NAMES, -1)["got"]
    for k, v in got.items():
        assert same_bits(v, again[k]) if v.dtype == np.float64 else np.array_equal(v, again[k]), k
    # ... and the mirrors
    keep = [s for s in range(n) if lengths[s] > 0]
    group = [f"s{s:02d}" for s in keep for _ in range(lengths[s])]
    day0 = np.datetime64("2024-01-01")
    date = np.concatenate([day0 + np.arange(lengths[s]) for s in keep])
    target = np.concatenate([series[s] for s in keep])
    pairs = [(m, {"seasonal_period": "4"} if m in SEASONAL else None) for m in NAMES]
    t = api.ts_forecast_best_by(group, date, target, pairs, h, "1d", folds=3)
    rows = {}
    for i in range(len(t["yhat"])):
        rows.setdefault(t["id"][i], []).append(i)
    assert list(rows) == [f"s{s:02d}" for s in keep if got["status"][s] == 0]
    for s in keep:
        if got["status"][s] != 0:
            continue
        idx = rows[f"s{s:02d}"]
        assert t["forecast_step"][idx].tolist() == list(range(1, h + 1))
        assert same_bits(t["yhat"][idx], got["yhat"][s]) and same_bits(t["yhat_lower"][idx], got["lower"][s]) and same_bits(t["yhat_upper"][idx], got["upper"][s])
        assert t["selected_method"][idx[0]] == NAMES[winner[s]] and same_bits(t["cv_score"][idx], np.full(h, got["best_score"][s]))
        assert t["model_name"][idx[0]] == res["names"][s]
        assert t["ds"][idx[0]] == day0 + lengths[s]
    cmp_rows, wins = api.ts_compare_models_by(group, date, target, pairs, h, "1d", folds=3)
    assert wins["method"] == list(NAMES) and wins["wins"].tolist() == [sum(1 for s in keep if winner[s] == m) for m in range(len(NAMES))]
    assert same_bits(cmp_rows["score"].reshape(len(keep), len(NAMES)), np.ascontiguousarray(got["scores"][:, keep].T))
    assert cmp_rows["is_winner"].reshape(len(keep), len(NAMES)).argmax(1)[[winner[s] >= 0 for s in keep]].tolist() == [winner[s] for s in keep if winner[s] >= 0]


def test_end_to_end_with_autoets_and_a_fallback(env):
    T, h, n = 60, 3, 65
    folds = env["api"].backtest_fold_bounds(T, h, 2)
    assert len(folds) == 2
    case = {"Y": _series(n, T, 9), "lengths": _edge_lengths(folds, T, n), "folds": folds, "h": h}
    res = _check_pick(env, case, ("Naive", "AutoETS", "CrostonSBA"), 0, metric="mae")
    assert sum(res["got"]["from_fallback"]) > 0 and (res["got"]["winner"] >= 0).all()


@pytest.mark.parametrize("mode", ["mean", "median", "inverse_score"])
def test_end_to_end_ensembles(env, case, mode):
    """An ensemble equals the restatement's combination of the methods' whole-block runs, through select_block and select_batch."""
    torch, lib, device, api = env["torch"], env["lib"], env["device"], env["api"]
    Y, lengths, folds, h = case["Y"], case["lengths"], case["folds"], case["h"]
    n, T = Y.shape
    F = len(folds)
    names = NAMES[:4]
    methods = _methods(lib, h, names)
    y, lens = _block(env, Y, lengths)
    r = device.select_block(y, lens, methods, folds, mode=mode, n_series=n)
    torch.cuda.synchronize()
    got = _to_numpy(r)
    scores = got["scores"][:, :n]
    full, fstat = [], []
    for o in methods:
        whole = device.DeviceBatch(n, T, o, env["dev"])
        whole.set_block(y, lens)
        whole.run()
        torch.cuda.synchronize()
        w = whole.results()
        full.append(w["yhat"].cpu().numpy().tolist())
        fstat.append(w["status"].cpu().numpy().tolist())
    want, row_status = R.combine(full, fstat, mode, scores=scores.tolist())
    assert same_bits(got["yhat"], np.array(want).reshape(n, h))
    assert got["status"].tolist() == [0 if st == 0 else lib.INSUFFICIENT_DATA for st in row_status] and 0 < sum(row_status) < n
    assert np.isnan(got["lower"]).all() and np.isnan(got["upper"]).all()
    bt = [b["yhat"].cpu().numpy().tolist() for b in r["backtests"]]
    bst = [b["status"].cpu().numpy().tolist() for b in r["backtests"]]
    want_bt, _ = R.combine(bt, bst, mode, scores=scores.tolist(), group_div=F)
    assert same_bits(got["bt_yhat"], np.array(want_bt).reshape(n * F, h))
    b, err = api.select_batch([Y[s, :lengths[s]] for s in range(n)], methods, folds, "rmse", mode, -1)
    assert err["ok"], err
    assert same_bits(b["yhat"], got["yhat"]) and np.array_equal(b["status"], got["status"]) and same_bits(b["backtest_yhat"], got["bt_yhat"])
    assert same_bits(b["backtest_actual"], got["bt_actual"]) and np.array_equal(b["n_rows"], got["bt_n_rows"])
    assert b["model_name"] == [mode if st == 0 else "" for st in got["status"]]


# --------------------------------------------------------------------------------------------
# the limits, through every entry
# --------------------------------------------------------------------------------------------
def test_limits_are_refused_through_every_entry(env, case):
    torch, lib, device, api, L, dev = env["torch"], env["lib"], env["device"], env["api"], env["L"], env["dev"]
    Y, lengths, folds, h = case["Y"], case["lengths"], case["folds"], case["h"]
    n = len(Y)
    y, lens = _block(env, Y, lengths)
    o = lambda m="Naive", hh=h: lib.make_options(m, hh, auto_detect=False)
    with pytest.raises(ValueError, match="n_methods 17 exceeds the limit of 16 methods"):
        device.select_block(y, lens, [o()] * 17, folds, n_series=n)
    with pytest.raises(ValueError, match="all methods share one horizon"):
        device.select_block(y, lens, [o(), o("SES", h + 1)], folds, n_series=n)
    scores = torch.zeros((17, 64), dtype=torch.float64, device=dev)
    with pytest.raises(ValueError, match="n_methods 17 exceeds the limit of 16 methods"):
        device.select_winner_block(scores, torch.zeros((17, 10), dtype=torch.int32, device=dev), -1, n_series=10)
    with pytest.raises(ValueError, match="limit of 16 methods"):
        device.combine_block([torch.zeros((4, 2), dtype=torch.float64, device=dev)] * 17, "mean")
    err = lib.AnofoxError()
    tab = (C.c_void_p * 17)(*([scores.data_ptr()] * 17))
    assert not L.anofox_hip_select_combine_device(tab, 17, 4, 2, scores.data_ptr(), 1, None, None, 0, 1, scores.data_ptr(), None, None, C.byref(err))
    assert err.code == lib.INVALID_INPUT and b"limit of 16 methods" in err.message
    series = [Y[s, :lengths[s]] for s in range(n)]
    for methods, text in (([o()] * 17, "n_methods 17 exceeds the limit of 16 methods"), ([o(), o("SES", h + 1)], "all methods share one horizon")):
        b, e = api.select_batch(series, methods, folds)
        assert not e["ok"] and e["code"] == lib.INVALID_INPUT and text in e["message"]
    group = [f"s{s}" for s in range(2) for _ in range(30)]
    date = np.concatenate([np.datetime64("2024-01-01") + np.arange(30)] * 2)
    with pytest.raises(api.InvalidInputException, match="limit of 16 methods"):
        api.ts_forecast_best_by(group, date, np.arange(60.0), ["Naive"] * 17, h, "1d", folds=2)
    with pytest.raises(api.InvalidInputException, match="limit of 16 methods"):
        api.ts_compare_models_by(group, date, np.arange(60.0), ["Naive"] * 17, h, "1d", folds=2)
