"""The device's AutoARIMA fits against the restatement of tests/arima_ref.py, without the oracle: for every family of
tests/arima_cases.py and both estimation methods the batch runs, the selected fit is read back (anofox_hip_batch_arima_fit) and the
model is replayed in 80-bit arithmetic from the read-back orders and coefficients -- the differencing decisions, n_diff, AICc / AIC /
BIC from the conditional sum of squares on the expanded polynomials, the point forecasts from the one multiplied-out operator, the
roots, the box, the name.  The tolerances are the constants of arima_ref.py, measured on the CPU by tests/test_arima_cpu.py.

Which candidates the search tries and how Nelder-Mead gets to the coefficients is not replayed (the bit-parity tests pin that); here
the read-back model must MEAN what the device forecast."""
import ctypes as C

import numpy as np
import pytest

import arima_cases as X
import arima_ref as A

pytestmark = pytest.mark.gpu

METHODS = ("css", "css-ml")
_RUNS = {}


@pytest.fixture(scope="module")
def env(hiplib):
    import torch
    assert torch.cuda.is_available()
    from anofox_forecast_amd import api
    return api, hiplib


def _block(series, t_max, ld):
    import torch
    Y = np.zeros((t_max, ld))
    lens = np.zeros(ld, dtype=np.int32)
    for s, y in enumerate(series):
        Y[: len(y), s] = y
        lens[s] = len(y)
    return torch.from_numpy(Y).to("cuda:0"), torch.from_numpy(lens).to("cuda:0")


def _read(api, lib, b, series, m):
    """Run the resident block of `b`, then every readback of the handle: records, forecasts, the inspection's criteria, names."""
    import torch
    n = len(series)
    b.run()
    torch.cuda.synchronize()
    fits = (lib.AnofoxHipArimaFit * n)()
    err = lib.AnofoxError()
    assert b.L.anofox_hip_batch_arima_fit(b.handle, fits, C.byref(err)), err.message
    insp = (lib.AnofoxHipInspection * n)()
    assert b.L.anofox_hip_batch_inspect(b.handle, insp, None, None, max(m, 1), C.byref(err)), err.message
    res = {k: v.cpu().numpy().copy() for k, v in b.results().items()}
    recs = []
    for s in range(n):
        r = api.arima_fit_record(fits[s])
        assert r["status"] == res["status"][s] == insp[s].status and r["model_code"] == res["model_code"][s] == insp[s].model_code, s
        assert r["seasonal_period"] == max(m, 1), s
        r.update(point=res["yhat"][s], insp_aic=insp[s].aic, insp_aicc=insp[s].aicc, insp_bic=insp[s].bic,
                 name=b.model_name(r["model_code"], s))
        recs.append(r)
    return recs


def _device_run(api, lib, fam, method):
    """One family through a DeviceBatch over a resident block (no NULLs there: the cleaned series)."""
    from anofox_forecast_amd.device import DeviceBatch
    series = X.cleaned(fam)
    n, T = len(series), max(len(y) for y in series)
    b = DeviceBatch(n, T, lib.make_options("AutoARIMA", fam["h"], seasonal_period=fam["m"]), "cuda:0")
    try:
        b.set_arima_method(lib.ARIMA_CSS_ML if method == "css-ml" else lib.ARIMA_CSS)
        b.set_block(*_block(series, T, b.ld))
        recs = _read(api, lib, b, series, fam["m"])
        second = None
        if fam["name"] == "ragged":                    # a second run on the same handle: nothing of the first may be left
            again = X.family("ragged-second")["series"]
            b.set_block(*_block(again, T, b.ld))
            second = _read(api, lib, b, again, fam["m"])
    finally:
        b.close()
    return recs, second


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


FLOATS = ("phi", "theta", "Phi", "Theta", "constant", "aicc")


def _runs(env, name, method):
    """Both routes of one family and method, once per session; the routes must agree to the bit."""
    key = (name, method)
    if key in _RUNS:
        return _RUNS[key]
    api, lib = env
    fam = X.family(name)
    recs, second = _device_run(api, lib, fam, method)
    host = api.arima_fit_batch(fam["series"], lib.make_options("AutoARIMA", fam["h"], seasonal_period=fam["m"]),
                               method=lib.ARIMA_CSS_ML if method == "css-ml" else lib.ARIMA_CSS, valids=fam.get("valids"))
    for s, (d, hrec) in enumerate(zip(recs, host)):
        assert all(d[k] == hrec[k] for k in api.ARIMA_FIT_INTS), (name, method, s, d, hrec)
        assert all(_same_bits(d[k], hrec[k]) for k in FLOATS), (name, method, s)
        if hrec["ok"]:
            assert _same_bits(d["point"], hrec["point"]) and hrec["model_name"] == d["name"], (name, method, s)
        else:
            assert d["status"] != 0, (name, method, s)
    _RUNS[key] = (recs, second)
    return _RUNS[key]


def _check_unfitted(r, where):
    """Nothing was fitted: a status or a fallback code, NaN in every double, zero orders and counters -- never a stale fit."""
    assert r["status"] != 0 or r["model_code"] < 1000000, where
    assert all(np.all(np.isnan(r[k])) for k in FLOATS), (where, r)
    assert all(r[k] == 0 for k in ("p", "d", "q", "P", "D", "Q", "has_constant", "n_diff", "models_tried", "evals")), (where, r)


def _check_records(name, method, fam, series, recs, worst, seen):
    """Every fitted record of one run against the restatement at its own orders and coefficients."""
    m, h = fam["m"], fam["h"]
    box = name == "box"
    tol = dict(aicc=A.AICC_ABS_BOX if box else A.AICC_ABS, forecast=A.FORECAST_REL_BOX if box else A.FORECAST_REL)
    fitted = exempt = 0
    for s, (y, r) in enumerate(zip(series, recs)):
        where = (name, method, s)
        if len(y) < 3:
            _check_unfitted(r, where)
            continue
        assert r["status"] == 0 and r["model_code"] >= 1000000, (where, r)        # (every series of three values or more gets a model)
        fitted += 1
        fit = X.fit_from_record(r, m)
        # the decisions, the differenced length, the rules of the model
        dec = X.decisions((name, len(y), s), y, m)
        if (fit["d"], fit["D"]) != dec[:2]:
            assert A.on_decision_edge(dec[2]), (where, (fit["d"], fit["D"]), dec)
            exempt += 1
        assert r["n_diff"] == len(y) - fit["d"] - fit["D"] * m, where
        assert not fit["has_constant"] or fit["d"] + fit["D"] <= 1, where
        assert fit["P"] + fit["Q"] + fit["D"] == 0 or m > 1, where
        coefs = fit["phi"] + fit["theta"] + fit["Phi"] + fit["Theta"]
        assert all(abs(v) <= A.COEF_BOX for v in coefs), (where, coefs)
        unused = fit["phi"][fit["p"]:] + fit["theta"][fit["q"]:] + fit["Phi"][fit["P"]:] + fit["Theta"][fit["Q"]:]
        assert all(v == 0.0 for v in unused) and (fit["has_constant"] or fit["constant"] == 0.0), (where, r)
        assert r["models_tried"] >= 1 and r["evals"] >= 1, (where, r)
        assert r["model_code"] == A.model_code(fit) and r["name"] == A.model_name(fit), (where, r["model_code"], r["name"])
        assert _same_bits(r["aicc"], r["insp_aicc"]), where
        rep = X.replay(("gpu", name, len(y), method, s), fit, y, h)
        assert rep["root"] >= A.ROOT_MIN - A.ROOT_MARGIN, (where, rep["root"])
        # criteria: the readback's AICc is the CSS run's, so it is the criterion of these coefficients only without the refit
        k = A.n_parameters(fit)
        if method == "css":
            if rep["degenerate"]:
                pen = 2.0 * k + 2.0 * k * (k + 1.0) / (r["n_diff"] - k - 1.0)
                implied = rep["nu"] * np.exp(A.LD(r["aicc"] - pen) / r["n_diff"])
                # (a sum of squares of exactly zero -- a constant series -- reports the variance floor of 1e-300)
                assert A.degenerate(implied, rep["gross"]) or implied <= rep["nu"] * 1.0e-300 * (1.0 + 1.0e-9), (where, r["aicc"], float(implied), float(rep["gross"]))
            else:
                for key, got in (("aicc", r["aicc"]), ("aic", r["insp_aic"]), ("bic", r["insp_bic"])):
                    d = float(abs(got - rep[key]))
                    worst[key] = max(worst.get(key, 0.0), d)
                    assert d <= tol["aicc"], (where, key, got, float(rep[key]), d)
        d = float(np.max(np.abs(r["point"] - rep["forecast"]))) / (float(np.max(np.abs(y))) or 1.0)
        worst["forecast"] = max(worst.get("forecast", 0.0), d)
        assert d <= tol["forecast"], (where, d, r["point"], np.asarray(rep["forecast"], dtype=float))
        seen["classes"].add((A.shape_class(fit["p"], fit["q"], fit["P"], fit["Q"]), A.ring_class(m)))
        seen["differences"].add((fit["d"], fit["D"]))
    assert exempt <= len(series) // 100, (name, method, exempt)
    return fitted


def _check_refit(name, fam, series, css_recs, ml_recs, worst):
    """ANOFOX_ARIMA_CSS_ML: the CSS run's orders and criterion; the refit's coefficients have an exact likelihood no worse than the CSS
    coefficients'; where the refit does not apply the CSS coefficients come back unchanged."""
    m = fam["m"]
    tol = A.LOGLIK_ABS_BOX if name == "box" else A.LOGLIK_ABS
    moved = 0
    for s, (y, a, b) in enumerate(zip(series, css_recs, ml_recs)):
        if len(y) < 3:
            continue
        assert all(a[k] == b[k] for k in ("p", "d", "q", "P", "D", "Q", "has_constant", "n_diff", "models_tried", "model_code")), (name, s)
        assert _same_bits(a["aicc"], b["aicc"]) and b["evals"] >= a["evals"], (name, s)
        same = all(_same_bits(a[k], b[k]) for k in FLOATS)
        fa, fb = X.fit_from_record(a, m), X.fit_from_record(b, m)
        La, Lb = fa["p"] + m * fa["P"], fa["q"] + m * fa["Q"]
        if (m > 24 and (fa["P"] or fa["Q"])) or max(La, Lb + 1) > 32:
            assert same, (name, s, a, b)
            continue
        if same:
            continue
        moved += 1
        w = A.difference(y, fa["d"], fa["D"], m)
        la, lb = A.exact_loglik(fa, w), A.exact_loglik(fb, w)
        worst["loglik gain"] = max(worst.get("loglik gain", -np.inf), float(lb - la))
        assert lb <= la + tol, (name, s, float(la), float(lb))
    return moved


def _report(what, worst):
    print(f"{what}: worst deviations " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(worst.items())))


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", X.FAMILY_NAMES)
def test_read_back_fit_is_the_model_that_was_forecast(env, name, method):
    fam = X.family(name)
    series = X.cleaned(fam)
    recs, second = _runs(env, name, method)
    worst, seen = {}, {"classes": set(), "differences": set()}
    fitted = _check_records(name, method, fam, series, recs, worst, seen)
    assert fitted == sum(len(y) >= 3 for y in series), (name, fitted)
    if second is not None:
        again = X.family("ragged-second")
        short = [len(y) < 3 for y in again["series"]]
        assert sum(short) == 10 and all(recs[s]["status"] == 0 for s in range(len(recs)) if short[s])      # (they had a fit in the first run)
        _check_records("ragged-second", method, again, again["series"], second, worst, seen)
    if method == "css-ml":
        css_recs, css_second = _runs(env, name, "css")
        moved = _check_refit(name, fam, series, css_recs, recs, worst)
        assert moved >= 1, name                          # the refit is not a no-op
        if second is not None:
            _check_refit("ragged-second", X.family("ragged-second"), X.family("ragged-second")["series"], css_second, second, worst)
    _report(f"{name} [{method}], {fitted} fits", worst)


def test_families_reach_every_pass_variant_ring_and_difference(env):
    """The device's own selections over the families cover exactly the intended (pass variant, home of the ring) and (d, D) pairs."""
    seen = {"classes": set(), "differences": set()}
    for name in X.FAMILY_NAMES:
        fam = X.family(name)
        for y, r in zip(X.cleaned(fam), _runs(env, name, "css")[0]):
            if len(y) >= 3:
                seen["classes"].add((A.shape_class(r["p"], r["q"], r["P"], r["Q"]), A.ring_class(fam["m"])))
                seen["differences"].add((r["d"], r["D"]))
    assert seen["classes"] == X.INTENDED_CLASSES, seen["classes"] ^ X.INTENDED_CLASSES
    assert seen["differences"] == X.INTENDED_DIFFERENCES, seen["differences"]


def test_readback_refuses_what_it_cannot_report(env):
    """Not an AutoARIMA batch, a batch that has not run: false with an error."""
    import torch
    from anofox_forecast_amd.device import DeviceBatch
    api, lib = env
    series = X.family("horizons-h1")["series"][:4]
    T = max(len(y) for y in series)
    for model, ran, want in (("AutoETS", True, "AutoARIMA"), ("AutoARIMA", False, "not been run")):
        b = DeviceBatch(4, T, lib.make_options(model, 3, seasonal_period=7), "cuda:0")
        try:
            b.set_block(*_block(series, T, b.ld))
            if ran:
                b.run()
                torch.cuda.synchronize()
            fits = (lib.AnofoxHipArimaFit * 4)()
            err = lib.AnofoxError()
            assert not b.L.anofox_hip_batch_arima_fit(b.handle, fits, C.byref(err)), model
            assert err.code == lib.INVALID_INPUT and want in err.message.decode(), err.message
        finally:
            b.close()
