"""GPU: the scaled, weighted scores of a hierarchy -- anofox_hip_scale_device, anofox_hip_weighted_scores_device,
anofox_hip_wrmsse_batch, device.scale_block / weighted_scores_block and the api mirrors -- against the pure-Python restatement
tests/scaled_scores_ref.py, composed with the existing hierarchy, metrics and path-score entries, and against tests/hierarchy_ref.py
for the sums.  The contract (DESIGN.md section 3 "Scaled scores") is equality of bits: the sums over rows are serial, the sums over
columns are the wave sum, so every comparison is == on the bit patterns; only the payload of a NaN is exempt (the sign of a zero is
not).  Shapes: tests/scaled_scores_cases.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import hierarchy_ref as H
import path_scores_cases
import scaled_scores_cases as K
import scaled_scores_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(hiplib):
    import torch
    assert torch.cuda.is_available()
    L = hiplib.load()
    from anofox_forecast_amd import api, device
    return {"torch": torch, "L": L, "lib": hiplib, "api": api, "device": device, "dev": torch.device("cuda:0")}


def _up(env, a):
    return env["torch"].from_numpy(np.array(a, order="C")).to(env["dev"])


def _bits(got, want, what):
    same = R.same_bits(got, want)
    assert same.all(), f"{what}: {int((~same).sum())} cells differ, first at {np.argwhere(~same)[0].tolist()}"


def _assert_scale(got, ref, n, what):
    _bits(got["scale"].cpu().numpy()[:, :n], ref["scale"], what + ": scale")
    assert got["first"].cpu().numpy().tolist() == ref["first"].tolist(), what + ": first"
    assert got["status"].cpu().numpy().tolist() == ref["status"].tolist(), what + ": status"


def _pad(block, extra):
    out = np.full((block.shape[0], block.shape[1] + extra), np.nan)
    out[:, :block.shape[1]] = block
    return out


# --------------------------------------------------------------------------------------------
# the scale kernel
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.SCALE_CASES, ids=K.scale_id)
def test_scale_equals_the_restatement(env, case):
    n, T, lag, tail_rows, trim, with_w = case
    block, lens, w = K.make_scale_case(n, T, n + 3 * T + lag, with_w)
    ref = R.scale_block(block, lens, lag, trim, tail_rows, w, n)
    if n >= 63 and T >= 15 and trim:                                 # the cases hold what they say they hold
        want = {1: R.SHORT, 2: R.SHORT, 3: R.CONSTANT, 4: R.NAN, 5: R.OK, 6: R.SHORT, 7: R.SHORT, 8: R.OK}
        assert {c: int(ref["status"][c]) for c in want} == want
        if with_w and tail_rows < T:
            assert ref["status"][9] == R.OK and ref["status"][10] == R.NAN
    kw = {"lag": lag, "trim_leading_zeros": trim, "tail_rows": tail_rows, "n_cols": n}
    y, ln = _up(env, block), _up(env, lens)
    wd = _up(env, w) if with_w else None
    got = env["device"].scale_block(y, ln, w_src=wd, **kw)
    _assert_scale(got, ref, n, "first run")
    assert np.isnan(got["scale"].cpu().numpy()[:, n:]).all()         # the padding columns of the output are not written
    _assert_scale(env["device"].scale_block(y, ln, w_src=wd, **kw), ref, n, "second run")
    wide = env["device"].scale_block(_up(env, _pad(block, 64)), _up(env, np.concatenate([lens, np.full(64, T, dtype=np.int32)])),
                                     w_src=_up(env, _pad(w, 64)) if with_w else None, **kw)
    _assert_scale(wide, ref, n, "a larger ld")


@pytest.mark.parametrize("lag,trim", [(1, True), (1, False), (7, True), (20, False)])
def test_rows_in_flight_do_not_show(env, lag, trim):
    """Columns of one wavefront whose lengths lie on both sides of every block edge (15 / 16 / 17 / 33 and their neighbours): whatever
    block of rows the build loads ahead, the chain is the row order."""
    block, lens, w = K.make_edge_case(lag)
    assert set(K.EDGE_LENGTHS) <= set(lens[:130].tolist())
    ref = R.scale_block(block, lens, lag, trim, 28, w, 130)
    got = env["device"].scale_block(_up(env, block), _up(env, lens), w_src=_up(env, w), lag=lag, trim_leading_zeros=trim, tail_rows=28, n_cols=130)
    _assert_scale(got, ref, 130, "edge lengths")


# --------------------------------------------------------------------------------------------
# the weighted scores
# --------------------------------------------------------------------------------------------
def _assert_weighted(got, ref, n, what):
    scaled = got["scaled"].cpu().numpy()[:, :n]
    cov = ref["covered"]
    _bits(scaled[:, cov], ref["scaled"][:, cov], what + ": scaled")
    assert np.isnan(scaled[:, ~cov]).all(), what + ": a cell no range covers is not touched"
    _bits(got["score"].cpu().numpy(), ref["score"], what + ": score")
    _bits(got["weight_sum"].cpu().numpy(), ref["weight_sum"], what + ": weight_sum")
    assert got["left"].cpu().numpy().tolist() == ref["left"].tolist(), what + ": left"
    _bits(got["total"].cpu().numpy(), ref["total"], what + ": total")
    _bits(got["total_mean"].cpu().numpy(), [ref["total_mean"]], what + ": total_mean")


@pytest.mark.parametrize("case", K.WEIGHTED_CASES, ids=K.weighted_id)
def test_weighted_scores_equal_the_restatement(env, case):
    n, n_loss, transform = case
    loss, scale, weight, status = K.make_weighted_case(n, n_loss, n + n_loss)
    ranges = K.ranges_of(n)
    dl, ds, dw, dst = _up(env, loss), _up(env, scale), _up(env, weight), _up(env, status)
    name = {0: "ratio", 1: "root"}[transform]
    for st, dstat in ((status, dst), (None, None)):
        ref = R.weighted_scores(loss, scale, weight, ranges, transform, st, n)
        got = env["device"].weighted_scores_block(dl, ds, dw, ranges, transform=name, col_status=dstat, n_cols=n)
        _assert_weighted(got, ref, n, "status" if st is not None else "no status")
    if n >= 130:
        assert ref["left"][5:].tolist() == [[-1] * n_loss] * 3 and ref["left"][4].tolist() == [3] * n_loss     # (no status: column 100 stays)
    # one range alone, passed as a tensor, by the integer code of the transform
    one = env["device"].weighted_scores_block(dl, ds, dw, _up(env, np.array([[0, n]], dtype=np.int32)), transform=transform, col_status=dst, n_cols=n)
    _assert_weighted(one, R.weighted_scores(loss, scale, weight, [(0, n)], transform, status, n), n, "one range")


# --------------------------------------------------------------------------------------------
# composition with the hierarchy, metrics and path-score entries
# --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _chain(planned, priced):
    """130 leaves that end on the same date, three groupings, horizon 28: the inputs and the restatement's answer (hierarchy_ref's
    sums, then scaled_scores_ref), computed once."""
    n, T, h = 130, 50, 28
    series, prices = K.make_training(n, T, 1)
    series[5] = np.zeros(len(series[5]))                                     # a leaf that never sold: left out of its level
    series[6][10] = np.nan                                           # a NaN: the leaf and every aggregate above it
    rng = np.random.default_rng(77)
    act = rng.poisson(1.2, size=(n, h)).astype(np.float64)
    fc = np.round(act + rng.normal(0.0, 0.8, size=(n, h)), 3)
    act[9, 3], fc[11, :] = np.nan, np.nan
    rev = [s * p for s, p in zip(series, prices)]
    first = [T - len(s) for s in series]
    if planned:
        column_of = K.make_hierarchy(n, 0)
        n_out, offs, memb = H.plan(column_of.tolist())
        ranges = [(int(g.min()), int(g.max()) + 1) for g in column_of]
    else:
        column_of, n_out, offs, memb, ranges = None, n, list(range(n + 1)), list(range(n)), [(0, n)]

    def block(rows, firsts, t_rows):
        cols = H.aggregate_block(rows, firsts, offs, memb)
        out, lens = np.zeros((t_rows, n_out)), np.zeros(n_out, dtype=np.int32)
        for c, (_lo, m, y, _p) in enumerate(cols):
            out[:m, c], lens[c] = y, m
        return out, lens
    train, lens = block(series, first, T)
    w = block(rev, first, T)[0] if priced else None
    zero = [0] * n
    fca, acta = block([r for r in fc], zero, h)[0], block([r for r in act], zero, h)[0]
    ref = R.wrmsse(train, lens, w, fca, acta, ranges, 1, True, 28)
    return {"series": series, "prices": prices if priced else None, "fc": fc, "act": act, "column_of": column_of, "ranges": ranges, "n_out": n_out,
            "train": train, "lens": lens, "w": w, "fca": fca, "acta": acta, "ref": ref, "T": T, "h": h, "n": n}


def _leaf_block(env, rows, T):
    n = len(rows)
    ld = K.ld_of(n)
    block, lens = np.zeros((T, ld)), np.zeros(ld, dtype=np.int32)
    for s, r in enumerate(rows):
        block[:len(r), s], lens[s] = r, len(r)
    return _up(env, block), _up(env, lens)


def test_aggregate_then_scale_then_weighted_equals_the_restatement(env):
    """aggregate_block -> scale_block on the aggregate as it lies; the mse row of anofox_hip_metrics_device passed by offset, as it
    lies; weighted_scores_block: the device route of the WRMSSE, against the restatement run on hierarchy_ref's sums."""
    c = _chain(True, True)
    torch, dev, device, L, lib = env["torch"], env["dev"], env["device"], env["L"], env["lib"]
    n, T, h, n_out, ref = c["n"], c["T"], c["h"], c["n_out"], c["ref"]
    co = _up(env, c["column_of"])
    plan = device.hierarchy_plan_device(co)
    first = _up(env, np.array([T - len(s) for s in c["series"]] + [0] * (K.ld_of(n) - n), dtype=np.int64))
    y, lens = _leaf_block(env, c["series"], T)
    rev, _ = _leaf_block(env, [s * p for s, p in zip(c["series"], c["prices"])], T)
    agg = device.aggregate_block(y, lens, plan, first=first, n_series=n, t_out=T)
    agg_w = device.aggregate_block(rev, lens, plan, first=first, n_series=n, t_out=T)
    assert agg["lengths"].cpu().numpy()[:n_out].tolist() == c["lens"].tolist()
    sc = device.scale_block(agg["y"], agg["lengths"], w_src=agg_w["y"], lag=1, trim_leading_zeros=True, tail_rows=28, n_cols=n_out)
    _assert_scale(sc, {"scale": ref["scale"], "first": ref["first"], "status": ref["status"]}, n_out, "scale of the aggregate")
    assert ref["status"][0] == R.NAN and (ref["status"] == R.OK).sum() > 100
    # forecasts and actuals up the plan, the mse row of the metrics entry where it lies
    steps = _up(env, np.array([h] * n + [0] * (K.ld_of(n) - n), dtype=np.int32))
    f_agg = device.aggregate_block(_up(env, path_scores_cases.time_major(c["fc"], fill=0.0)), steps, plan, n_series=n, t_out=h)
    a_agg = device.aggregate_block(_up(env, path_scores_cases.time_major(c["act"], fill=0.0)), steps, plan, n_series=n, t_out=h)
    ld = int(f_agg["y"].shape[1])
    figures = torch.full((12, ld), -5.0, dtype=torch.float64, device=dev)
    mstatus = torch.zeros(ld, dtype=torch.int32, device=dev)
    err = lib.AnofoxError()
    assert L.anofox_hip_metrics_device(a_agg["y"].data_ptr(), f_agg["y"].data_ptr(), None, None, None, None, 0, None, 0, 1, ld,
                                       f_agg["lengths"].data_ptr(), n_out, h, 1 << 1, 0.5, True, figures.data_ptr(), ld, mstatus.data_ptr(), None,
                                       C.byref(err)), err.message
    _bits(figures[1, :n_out].cpu().numpy(), ref["mse"], "the mse row")
    ws = device.weighted_scores_block(figures[1], sc["scale"][0], sc["scale"][3], c["ranges"], transform="root", col_status=sc["status"], n_cols=n_out)
    _bits(ws["scaled"].cpu().numpy()[0, :n_out], ref["rmsse"], "rmsse")
    _bits(ws["score"].cpu().numpy()[:, 0], ref["score"], "score")
    assert ws["left"].cpu().numpy()[:, 0].tolist() == ref["left"].tolist()
    _bits(ws["total_mean"].cpu().numpy(), [ref["wrmsse"]], "wrmsse")
    assert ref["left"].tolist()[0] == 1 and ref["left"][2] >= 3 and np.isnan(ref["score"][0]) and not np.isnan(ref["score"][1:]).any()


def test_wspl_of_the_pinball_rows(env):
    """(130 columns, h = 28, 1,000 paths, nine levels): the pinball rows of path_scores_block as they lie, the mad row, the tail row:
    api.wspl_block against the restatement fed with the same rows."""
    n, h, P = 130, 28, 1000
    levels = path_scores_cases.LEVELS
    block, actual = path_scores_cases.make_block(n, h, P, 5)
    train, lens, _w = K.make_scale_case(n, 100, 12, False)
    ranges = [(0, 1), (1, 14), (14, 130), (0, 0)]
    paths = _up(env, path_scores_cases.pad_columns(block))
    out = env["api"].wspl_block(paths, _up(env, path_scores_cases.time_major(actual)), levels, _up(env, train), _up(env, lens), ranges, horizon=h,
                                n_paths=P, n_cols=n, tail_rows=28)
    sref = R.scale_block(train, lens, 1, True, 28, None, n)
    _assert_scale(out["scale"], sref, n, "scale")
    pinball = out["scores"]["pinball"].cpu().numpy()
    assert pinball.shape == (9, n) and out["scores"]["column"].shape[0] == 11
    ref = R.weighted_scores(pinball, sref["scale"][1], sref["scale"][3], ranges, R.RATIO, sref["status"], n)
    _assert_weighted({k: out[k] for k in ("scaled", "score", "weight_sum", "left", "total")} | {"total_mean": out["wspl"]}, ref, n, "wspl")
    assert not np.isnan(ref["total"]).any() and ref["left"][3].tolist() == [-1] * 9


@pytest.mark.parametrize("planned,priced", [(True, True), (True, False), (False, True), (False, False)],
                         ids=["plan-prices", "plan-units", "leaves-prices", "leaves-units"])
def test_wrmsse_batch_equals_the_restatement(env, planned, priced):
    c = _chain(planned, priced)
    ref, n_out = c["ref"], c["n_out"]
    res, err = env["api"].wrmsse_batch(c["series"], c["fc"], c["act"], column_of=c["column_of"], prices=c["prices"], lag=1, trim_leading_zeros=True,
                                       tail_rows=28)
    assert err["ok"], err
    assert res["n_out"] == n_out and res["ld"] == K.ld_of(n_out) and res["ranges"].tolist() == [list(r) for r in c["ranges"]]
    _bits(res["scale"][:, :n_out], ref["scale"], "scale")
    assert res["status"].tolist() == ref["status"].tolist()
    _bits(res["rmsse"], ref["rmsse"], "rmsse")
    _bits(res["score"], ref["score"], "score")
    assert res["left"].tolist() == ref["left"].tolist()
    _bits([res["wrmsse"]], [ref["wrmsse"]], "wrmsse")
    assert not np.isnan(ref["wrmsse"]) and np.isnan(res["scale"][:, n_out:]).all()


def test_scale_batch_equals_the_restatement(env):
    series, prices = K.make_training(70, 40, 3)
    rev = [s * p for s, p in zip(series, prices)]
    got = env["api"].scale_batch(series, w_series=rev, lag=7, trim_leading_zeros=True, tail_rows=5)
    for s in range(70):
        r = R.scale_column(series[s].tolist(), len(series[s]), 7, True, 5, rev[s].tolist())
        _bits([got[k][s] for k in ("msd", "mad", "n_terms", "tail")], [r[k] for k in ("msd", "mad", "n_terms", "tail")], f"series {s}")
        assert (int(got["first"][s]), int(got["status"][s])) == (r["first"], r["status"])


def test_ts_wrmsse_by_on_a_key_sorted_table(env):
    """Two stores x three items, 30 days, sorted by (store, item, date): the GPU route, against the restatement on the sums formed in
    row order."""
    api = env["api"]
    rng = np.random.default_rng(11)
    T, h = 30, 4
    stores, items = ["s1", "s2"], ["a", "b", "c"]
    leaves = [(s, i) for s in stores for i in items]
    vals = {k: rng.poisson(2.0, size=T).astype(np.float64) for k in leaves}
    vals[leaves[1]][:6] = 0.0
    price = {k: np.round(rng.random(T) * 3.0 + 1.0, 2) for k in leaves}
    day0 = np.datetime64("2024-03-01")
    date = np.array([day0 + t for k in leaves for t in range(T)], dtype="datetime64[D]")
    value = np.concatenate([vals[k] for k in leaves])
    prices = np.concatenate([price[k] for k in leaves])
    ids = [np.array([k[0] for k in leaves for _ in range(T)], dtype=object), np.array([k[1] for k in leaves for _ in range(T)], dtype=object)]
    fc = {k: np.round(rng.random(h) * 4.0, 2) for k in leaves}
    act = {k: rng.poisson(2.0, size=h).astype(np.float64) for k in leaves}
    table = {"unique_id": np.array(["|".join(k) for k in leaves for _ in range(h)], dtype=object),
             "date": np.array([day0 + T + t for _ in leaves for t in range(h)], dtype="datetime64[D]"),
             "forecast": np.concatenate([fc[k] for k in leaves]), "actual": np.concatenate([act[k] for k in leaves])}
    info = {}
    out = api.ts_wrmsse_by(date, value, ids, table, {"price": prices, "tail_rows": 7}, info=info)
    assert info["route"] == "gpu"
    # columns level by level: the total, the two stores, the six leaves; every sum in leaf order
    members = [list(range(6)), [0, 1, 2], [3, 4, 5]] + [[k] for k in range(6)]

    def add(rows):
        out = np.zeros((len(rows[0]), len(members)))
        for c, ms in enumerate(members):
            for t in range(len(rows[0])):
                s = 0.0
                for k in ms:
                    s = s + float(rows[k][t])
                out[t, c] = s
        return out
    train = add([vals[k] for k in leaves])
    w = add([vals[k] * price[k] for k in leaves])
    ref = R.wrmsse(train, [T] * 9, w, add([fc[k] for k in leaves]), add([act[k] for k in leaves]), [(0, 1), (1, 3), (3, 9)], 1, True, 7)
    assert out["level"].tolist() == [0, 1, 2, -1] and out["n_series"].tolist() == [1, 2, 6, 9] and out["left_out"].tolist() == [0, 0, 0, 0]
    _bits(out["score"], list(ref["score"]) + [ref["wrmsse"]], "score")
    _bits(info["rmsse"], ref["rmsse"], "rmsse")
    assert info["unique_id"].tolist() == ["AGGREGATED|AGGREGATED", "s1|AGGREGATED", "s2|AGGREGATED"] + ["|".join(k) for k in leaves]
