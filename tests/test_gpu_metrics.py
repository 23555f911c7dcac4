"""GPU: the accuracy metric entries (anofox_ts_mae .. anofox_ts_coverage, anofox_hip_metrics_batch, anofox_hip_metrics_device) and
the mirrors in api.py against the restatement tests/metrics_ref.py.  The contract is equality of bits with
the source's arithmetic, through every entry and both layouts; zeros compare by == and NaN by NaN-ness (the sign of a zero result
and NaN payloads are the two exemptions)."""
import ctypes as C
import math

import numpy as np
import pytest

import metrics_cases as MC
import metrics_ref as R
from test_metrics_cpu import check_scalar

pytestmark = pytest.mark.gpu

KATS = MC.load_kats()
SENTINEL = -777.0
ALL = R.FIGURES


@pytest.fixture(scope="module")
def api(hiplib):
    import torch
    assert torch.cuda.is_available()
    hiplib.load()
    from anofox_forecast_amd import api as A
    return A


def _mask(figures):
    m = 0
    for f in figures:
        m |= 1 << ALL.index(f)
    return m


def _device(lib, layout, blocks, quants=None, levels=None, figures=ALL, quantile=0.5, drop_nan=False, extra_cols=37, expect_ok=True):
    """Through anofox_hip_metrics_device on torch tensors, time-major ('tm': element (s, t) at t * ld_in + s) or series-major
    ('sm': at s * t_pad + t).  `ld` of the outputs is padded; the figures start as a sentinel.  Returns (figures [12 x ld], status)."""
    import torch
    L = lib.load()
    n = len(blocks["actual"])
    T = max(1, max(len(a) for a in blocks["actual"]))
    ld = (n + extra_cols + 63) // 64 * 64
    t_pad = T + 3
    dev = "cuda:0"

    def place(cols):
        if layout == "tm":
            m = np.full((T, ld), 12345.0)
            for i, c in enumerate(cols):
                m[:len(c), i] = c
        else:
            m = np.full((n, t_pad), 12345.0)
            for i, c in enumerate(cols):
                m[i, :len(c)] = c
        return m

    stride_s, stride_t = (1, ld) if layout == "tm" else (t_pad, 1)
    tens = {k: torch.from_numpy(place(v)).to(dev) for k, v in blocks.items() if v is not None}
    tq = None
    if quants:
        tq = torch.from_numpy(np.stack([place(q) for q in quants])).to(dev)
    lv = None if levels is None else np.ascontiguousarray(levels, dtype=np.float64)
    lens = torch.from_numpy(np.array([len(a) for a in blocks["actual"]], dtype=np.int32)).to(dev)
    fig = torch.full((len(ALL), ld), SENTINEL, dtype=torch.float64, device=dev)
    status = torch.full((n,), -5, dtype=torch.int32, device=dev)
    err = lib.AnofoxError()
    ptr = lambda k: tens[k].data_ptr() if k in tens else None
    torch.cuda.synchronize()
    ok = L.anofox_hip_metrics_device(ptr("actual"), ptr("forecast"), ptr("second"), ptr("lower"), ptr("upper"),
                                     None if tq is None else tq.data_ptr(), 0 if tq is None else tq[0].numel(),
                                     None if lv is None else lv.ctypes.data, 0 if lv is None else len(lv), stride_s, stride_t, lens.data_ptr(), n, T,
                                     _mask(figures), quantile, drop_nan, fig.data_ptr(), ld, status.data_ptr(), None, C.byref(err))
    if not expect_ok:
        return ok, err.code, err.message.decode()
    assert ok, err.message
    return fig.cpu().numpy(), status.cpu().numpy()


def _compare(got, want, where):
    bad = [(where, f, i, float(got[f][i]), want[f][i]) for f in want for i in range(len(want[f])) if not MC.same_bits(float(got[f][i]), want[f][i])]
    assert not bad, bad[:8]


def _rows(fig, n, figures=ALL):
    return {f: fig[ALL.index(f), :n] for f in figures}


def _single(lib, f, i, blocks, quants, levels, quantile):
    """Figure f of group i through its single entry: (ok, value, message)."""
    L = lib.load()
    a = np.ascontiguousarray(blocks["actual"][i])
    col = lambda k: np.ascontiguousarray(blocks[k][i])
    p = lambda v: v.ctypes.data if len(v) else np.zeros(1).ctypes.data
    out, err = C.c_double(), lib.AnofoxError()
    n = len(a)
    if f in MC.TWO_INPUT:
        fc = col("forecast")
        ok = getattr(L, "anofox_ts_" + f)(p(a), n, p(fc), n, C.byref(out), C.byref(err))
    elif f in ("rmae", "mase"):
        fc, sc = col("forecast"), col("second")
        ok = getattr(L, "anofox_ts_" + f)(p(a), n, p(fc), n, p(sc), n, C.byref(out), C.byref(err))
    elif f == "quantile_loss":
        fc = col("forecast")
        ok = L.anofox_ts_quantile_loss(p(a), n, p(fc), n, quantile, C.byref(out), C.byref(err))
    elif f == "coverage":
        lo, up = col("lower"), col("upper")
        ok = L.anofox_ts_coverage(p(a), n, p(lo), p(up), C.byref(out), C.byref(err))
    else:
        qs = [np.ascontiguousarray(q[i]) for q in quants]
        arr = (C.c_void_p * len(qs))(*[p(q) for q in qs])
        lv = np.ascontiguousarray(levels, dtype=np.float64)
        ok = L.anofox_ts_mqloss(p(a), n, arr, len(qs), lv.ctypes.data, C.byref(out), C.byref(err))
    return ok, out.value, err.message.decode()


# --------------------------------------------------------------------------------------------
# the reference's own statements
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", KATS["scalar"], ids=lambda c: c["name"])
def test_golden_scalars(api, case):
    check_scalar(case, lambda fn, args: getattr(api, fn)(*args))


@pytest.mark.parametrize("st", KATS["statements"], ids=lambda s: s["name"])
def test_golden_tables(api, st):
    MC.check_statement(api, KATS, st)


# --------------------------------------------------------------------------------------------
# equality of bits: every figure, every entry, both layouts
# --------------------------------------------------------------------------------------------
def test_bits_equal_through_every_entry(api, hiplib):
    blocks, quants = MC.shape_block()
    want, errs = MC.shape_reference()
    n = MC.N_GROUPS
    assert [len(a) for a in blocks["actual"]][:12] == list(MC.LENGTHS) and len(blocks["actual"][-1]) == MC.LONG_ROWS and n == 130
    got = api.metrics_batch(blocks["actual"], blocks["forecast"], blocks["second"], blocks["lower"], blocks["upper"], quants, MC.LEVELS, ALL, 0.9)
    _compare(got, want, "batch")
    assert [m or None for m in got["message"]] == errs and errs[0] == R.EMPTY_TEXT
    first = None
    for layout in ("tm", "sm"):
        for run in range(2):
            fig, status = _device(hiplib, layout, blocks, quants, MC.LEVELS, ALL, 0.9)
            _compare(_rows(fig, n), want, layout)
            assert (status == np.array([0 if len(a) else 1 for a in blocks["actual"]])).all()
            assert (fig[:, n:] == SENTINEL).all()                  # the padded columns stay untouched
            if first is None:
                first = fig[:, :n].copy()
            assert np.array_equal(first.view(np.uint64), fig[:, :n].view(np.uint64))   # the same bits: second run, other layout
    assert np.array_equal(first.view(np.uint64), np.stack([got[f] for f in ALL]).view(np.uint64))        # ... and the batch entry
    for i in (0, n - 1):                                            # the single entries: the first group is empty, the last has 5,000 rows
        for f in ALL:
            ok, v, msg = _single(hiplib, f, i, blocks, quants, MC.LEVELS, 0.9)
            if i == 0:
                assert (ok, math.isnan(v)) == (True, True) if f == "coverage" else (not ok and msg == R.EMPTY_TEXT), (f, ok, msg)
            else:
                assert ok and np.float64(v).tobytes() == first[ALL.index(f), i].tobytes(), (f, v)


def test_only_requested_rows_are_written(hiplib):
    """The seven two-input figures alone (the kernel variant without quantile blocks): the same bits, the other rows untouched."""
    blocks, _ = MC.shape_block()
    want, _ = MC.shape_reference()
    two = {"actual": blocks["actual"], "forecast": blocks["forecast"]}
    for layout in ("tm", "sm"):
        fig, _ = _device(hiplib, layout, two, figures=MC.TWO_INPUT)
        _compare(_rows(fig, MC.N_GROUPS, MC.TWO_INPUT), {f: want[f] for f in MC.TWO_INPUT}, layout)
        others = [ALL.index(f) for f in ALL if f not in MC.TWO_INPUT]
        assert (fig[others] == SENTINEL).all()


# --------------------------------------------------------------------------------------------
# the row filter
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drop_nan", [True, False], ids=["drop", "keep"])
@pytest.mark.parametrize("nan_in", ["actual", "forecast", "second", "lower", "upper", "quantiles"])
def test_row_filter(api, hiplib, nan_in, drop_nan):
    blocks, quants = MC.shape_block(nan_in)
    want, errs = MC.shape_reference(nan_in, drop_nan)
    got = api.metrics_batch(blocks["actual"], blocks["forecast"], blocks["second"], blocks["lower"], blocks["upper"], quants, MC.LEVELS, ALL, 0.9,
                            drop_nan)
    _compare(got, want, "batch")
    assert [m or None for m in got["message"]] == errs
    fig, status = _device(hiplib, "sm", blocks, quants, MC.LEVELS, ALL, 0.9, drop_nan)
    _compare(_rows(fig, MC.N_GROUPS), want, "sm")
    assert (status == np.array([0 if e is None else 1 for e in errs])).all()


def test_filter_uses_the_supplied_blocks_only(api):
    """A NaN in a block that is NOT handed in cannot filter: ts_mae_by filters on actual and forecast alone."""
    nan = float("nan")
    a, f = [np.array([1.0, 2.0, 3.0])], [np.array([2.0, nan, 5.0])]
    got = api.metrics_batch(a, f, figures=("mae",), drop_nan=True)
    assert got["mae"][0] == R.mae([1.0, 3.0], [2.0, 5.0])
    got = api.metrics_batch(a, f, lower=[np.array([nan, 0.0, 0.0])], upper=[np.array([9.0, 9.0, 9.0])], figures=("mae", "coverage"), drop_nan=True)
    assert got["mae"][0] == R.mae([3.0], [5.0]) and got["coverage"][0] == 1.0
    got = api.metrics_batch([np.array([nan, 1.0]), np.array([1.0])], [np.array([1.0, nan]), np.array([3.0])], figures=("mae",), drop_nan=True)
    assert math.isnan(got["mae"][0]) and got["mae"][1] == 2.0      # every row filtered: NaN and the empty-input error, alone
    assert list(got["code"]) == [3, 0] and got["message"] == [R.EMPTY_TEXT, ""]


# --------------------------------------------------------------------------------------------
# special rows
# --------------------------------------------------------------------------------------------
def test_special_rows(api):
    inf, nan = float("inf"), float("nan")
    cases = [
        ([0.0, 0.0, 0.0], [1.0, 2.0, 3.0]),                        # all-zero actuals: MAPE NaN
        ([0.0, 0.0], [0.0, -0.0]),                                 # both zero: sMAPE NaN too; -0.0 forecasts against +0.0 actuals
        ([4.0, 4.0, 4.0, 4.0], [3.0, 4.5, 4.0, 6.0]),              # constant actual: R^2 NaN
        ([1.0, inf, 3.0], [1.5, 2.0, -inf]),                       # +-inf
        ([inf, 1.0], [inf, 1.0]),                                  # inf - inf
        ([1e-17, -1e-17, 2.0], [1e-17, 1e-17, 2.5]),               # below EPSILON: filtered by MAPE; sMAPE's sum of two is filtered too
        ([1e308, -1e308], [-1e308, 1e308]),                        # overflow of the difference and of its square
        ([0.1, 0.2, 0.3], [0.3, 0.2, 0.1]),
    ]
    a = [np.array(c[0]) for c in cases]
    f = [np.array(c[1]) for c in cases]
    s = [x.copy() for x in a]                                       # baseline equal to actual: the ratio is NaN
    lo = [np.array([nan] + [v - 1.0 for v in c[0][1:]]) for c in cases]         # a NaN bound never covers
    up = [np.array([v + 1.0 for v in c[0][:-1]] + [nan]) for c in cases]
    figs = [x for x in ALL if x != "mqloss"]
    for q in (0.0, 0.5, 1.0):
        got = api.metrics_batch(a, f, s, lo, up, figures=figs, quantile=q)
        for i in range(len(cases)):
            want, err = R.group_figures(figs, a[i].tolist(), f[i].tolist(), s[i].tolist(), lo[i].tolist(), up[i].tolist(), quantile=q)
            assert err is None and got["code"][i] == 0
            for x in figs:
                assert MC.same_bits(float(got[x][i]), want[x]), (q, i, x, float(got[x][i]), want[x])
            assert math.isnan(got["mase"][i]) and math.isnan(got["rmae"][i])
    assert math.isnan(got["mape"][0]) and math.isnan(got["mape"][1]) and math.isnan(got["smape"][1]) and math.isnan(got["r2"][2])
    assert got["coverage"][7] == 1.0 / 3.0
    # quantile 1.5: quantile_loss fails per group with the source's text, the other figures are computed
    got = api.metrics_batch(a, f, figures=("mae", "quantile_loss"), quantile=1.5)
    assert (got["code"] == 3).all() and set(got["message"]) == {R.QUANTILE_TEXT} and np.isnan(got["quantile_loss"]).all()
    assert got["mae"][7] == R.mae(cases[7][0], cases[7][1])
    assert api.ts_quantile_loss(cases[7][0], cases[7][1], 1.5) is None


@pytest.mark.parametrize("n_levels", [1, 3, 16])
def test_mqloss_levels(api, hiplib, n_levels):
    rng = np.random.default_rng(n_levels)
    lens = [5, 64, 65, 200]
    a = [np.round(rng.normal(0, 2, n), 1) for n in lens]
    levels = [round((k + 1) / (n_levels + 1), 3) for k in range(n_levels)]
    qs = [[np.round(x + rng.normal(0, 1, len(x)), 1) for x in a] for _ in levels]
    got = api.metrics_batch(a, quantiles=qs, levels=levels, figures=("mqloss",))
    want = [R.mqloss(a[i].tolist(), [q[i].tolist() for q in qs], levels) for i in range(len(a))]
    assert [float(v) for v in got["mqloss"]] == want
    fig, _ = _device(hiplib, "sm", {"actual": a}, qs, levels, ("mqloss",))
    assert [float(v) for v in fig[ALL.index("mqloss"), :len(a)]] == want
    assert api.ts_mqloss(a[0].tolist(), [q[0].tolist() for q in qs], levels) == want[0]


def test_mqloss_limit(api, hiplib):
    from anofox_forecast_amd.api import InvalidInputException
    a = [np.array([1.0, 2.0])]
    with pytest.raises(InvalidInputException, match="at most 16 quantile levels per call, got 17"):
        api.metrics_batch(a, quantiles=[a] * 17, levels=[0.5] * 17, figures=("mqloss",))
    ok, code, msg = _device(hiplib, "sm", {"actual": a}, [a] * 17, [0.5] * 17, ("mqloss",), expect_ok=False)
    assert not ok and code == hiplib.INVALID_INPUT and "at most 16 quantile levels" in msg
    ok, code, msg = _device(hiplib, "sm", {"actual": a, "forecast": a}, figures=("quantile_loss",), quantile=1.5, expect_ok=False)
    assert not ok and code == hiplib.INVALID_INPUT and msg == R.QUANTILE_TEXT
    ok, code, msg = _device(hiplib, "tm", {"actual": a}, figures=("mae",), expect_ok=False)
    assert not ok and code == hiplib.INVALID_INPUT and "'mae' needs forecast" in msg


# --------------------------------------------------------------------------------------------
# fit -> forecast -> score without leaving the device
# --------------------------------------------------------------------------------------------
def test_score_device_results_where_they_lie(hiplib):
    import torch
    from anofox_forecast_amd import device, synth
    L = hiplib.load()
    n, T, h = 70, 60, 7
    Y = np.round(synth.gen_series(synth.SEED_M5, 0, n, T + h, 7, positive=False), 1)
    opts = hiplib.make_options("Naive", h)
    b = device.DeviceBatch(n, T, opts)
    y = torch.from_numpy(device.pack_time_major(Y[:, :T], b.ld)).to(b.device)
    lens = torch.full((b.ld,), T, dtype=torch.int32, device=b.device)
    b.set_block(y, lens)
    b.run()
    torch.cuda.synchronize()
    r = b.results()
    assert (r["status"].cpu().numpy() == 0).all()
    actual = torch.from_numpy(np.ascontiguousarray(Y[:, T:])).to(b.device)          # [n x h], the layout of the results
    hl = torch.full((n,), h, dtype=torch.int32, device=b.device)
    figs = MC.TWO_INPUT + ("quantile_loss", "coverage")
    ld = 128
    fig = torch.full((len(ALL), ld), SENTINEL, dtype=torch.float64, device=b.device)
    status = torch.full((n,), -5, dtype=torch.int32, device=b.device)
    err = hiplib.AnofoxError()
    ok = L.anofox_hip_metrics_device(actual.data_ptr(), r["yhat"].data_ptr(), None, r["lower"].data_ptr(), r["upper"].data_ptr(), None, 0, None, 0,
                                     h, 1, hl.data_ptr(), n, h, _mask(figs), 0.5, False, fig.data_ptr(), ld, status.data_ptr(), None, C.byref(err))
    assert ok, err.message
    got = fig.cpu().numpy()
    yhat, lower, upper = (r[k].cpu().numpy() for k in ("yhat", "lower", "upper"))
    assert (status.cpu().numpy() == 0).all() and (got[:, n:] == SENTINEL).all()
    for i in range(n):
        want, e = R.group_figures(figs, Y[i, T:].tolist(), yhat[i].tolist(), None, lower[i].tolist(), upper[i].tolist(), quantile=0.5)
        assert e is None
        for f in figs:
            assert MC.same_bits(float(got[ALL.index(f), i]), want[f]), (i, f)
    b.close()
