"""CPU: the AutoARIMA oracle (oracle/arima.c) against the textbook restatement of tests/arima_ref.py, on every family of
tests/arima_cases.py.  The oracle selects and estimates (oracle_auto_arima_detail); its orders and box-clipped coordinates go to the
restatement, which recomputes in 80-bit arithmetic, by other routes, what the oracle reports: the conditional sum of squares (expanded
polynomials against the cascade of four filters), n - La, sigma2, AICc, the forecasts (one multiplied-out operator against forecast +
integration loops), the admissibility verdict (numpy.roots against the step-down recursion), the two differencing decisions on every
series and every intermediate difference, and the exact likelihood (Durbin-Levinson factorisation against the Chandrasekhar filter).

This is also where the tolerances of arima_ref.py come from: every test prints the worst deviation it saw, the constants are 16 x
the worst over the families, and tests/test_gpu_arima_replay.py holds the device to the same constants without the oracle."""
import ctypes as C

import numpy as np
import pytest

import arima_cases as X
import arima_ref as A
import inspect_cases as K

_SEEN = {"classes": set(), "differences": set(), "families": set()}


def _bind(O):
    L = O.lib()
    L.oracle_arima_kpss_reject.restype = C.c_int
    L.oracle_arima_kpss_reject.argtypes = [C.c_void_p, C.c_int]
    L.oracle_arima_seasonal_strength.restype = C.c_double
    L.oracle_arima_seasonal_strength.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.oracle_arima_ml.restype = C.c_double
    L.oracle_arima_ml.argtypes = [C.POINTER(K.ArimaOrder), C.c_void_p, C.c_void_p, C.c_int]
    L.oracle_arima_roots_ok.restype = C.c_int
    L.oracle_arima_roots_ok.argtypes = [C.POINTER(K.ArimaOrder), C.c_void_p]
    return L


def _levels(y, d, D, m):
    """The series and every intermediate difference the decisions were taken on, in float64 as the oracle differences them."""
    out = [np.ascontiguousarray(y, dtype=np.float64)]
    if D:
        out.append(np.ascontiguousarray(out[-1][m:] - out[-1][:-m]))
    for _ in range(d):
        out.append(np.ascontiguousarray(out[-1][1:] - out[-1][:-1]))
    return out


METHODS = ("css", "css-ml")            # ANOFOX_ARIMA_CSS / ANOFOX_ARIMA_CSS_ML: the oracle's flag oracle_arima_ml_refit


def _family_report(O, name, method):
    """Worst deviations of one family under one estimation method (computed once per session)."""
    key = ("cpu-report", name, method)
    if key in X._CACHE:
        return X._CACHE[key]
    if method == "css-ml":
        _family_report(O, name, "css")        # (the refit is compared with the CSS run's fits)
    L = _bind(O)
    flag = C.c_int.in_dll(L, "oracle_arima_ml_refit")
    flag.value = 1 if method == "css-ml" else 0
    try:
        rep = _measure(O, L, name, method)
    finally:
        flag.value = 0
    X._CACHE[key] = rep
    print(f"{name} [{method}]: {rep['fitted']} fits ({rep['degenerate']} degenerate, {rep['on_box']} on the box, {rep['ml']} likelihoods): "
          f"css {rep['css']:.3e} sigma2 {rep['sigma2']:.3e} aicc {rep['aicc']:.3e} forecast {rep['forecast']:.3e} loglik {rep['loglik']:.3e} "
          f"strength {rep['strength']:.3e} smallest root - {A.ROOT_MIN} = {rep['root_gap']:.3e}, exempt {rep['exempt']}, refits moved {rep['moved']}")
    return rep


def _measure(O, L, name, method):
    fam = X.family(name)
    m, h = fam["m"], fam["h"]
    rep = dict(moved=0, css=0.0, sigma2=0.0, aicc=0.0, forecast=0.0, loglik=0.0, strength=0.0, root_gap=np.inf, exempt=0, fitted=0, ml=0, on_box=0, degenerate=0)
    for s, y in enumerate(X.cleaned(fam)):
        got = K.arima_detail(O, y, m, h) if len(y) >= 3 else None
        dec = X.decisions((name, s), y, m) if len(y) >= 3 else (0, 0, [])
        if got is None:
            continue
        f, fc = got
        o = f.ord
        rep["fitted"] += 1
        # the two decisions, and the statistics on every level they were taken on
        if (o.d, o.D) != dec[:2]:
            assert A.on_decision_edge(dec[2]), (name, s, (o.d, o.D), dec)
            rep["exempt"] += 1
        for lv in _levels(y, o.d, o.D, m)[: 1 + o.D + o.d]:
            if len(lv) > 3:
                k = A.kpss_statistic(lv)
                want = bool(k is not None and len(lv) >= 4 and k > A.KPSS_CRITICAL)
                if bool(L.oracle_arima_kpss_reject(lv.ctypes.data, len(lv))) != want:
                    assert k is not None and abs(k - A.KPSS_CRITICAL) <= A.DECISION_EDGE * A.KPSS_CRITICAL, (name, s, k)
            if m > 1:
                rep["strength"] = max(rep["strength"], abs(float(L.oracle_arima_seasonal_strength(lv.ctypes.data, len(lv), m) - A.seasonal_strength(lv, m))))
        fit = X.fit_from_coordinates((o.p, o.d, o.q, o.P, o.D, o.Q, o.with_constant), f.x[:], m)
        r = X.replay(("cpu", name, method, s), fit, y, h)
        _SEEN["classes"].add((A.shape_class(o.p, o.q, o.P, o.Q), A.ring_class(m)))
        _SEEN["differences"].add((o.d, o.D))
        assert f.n_used == r["n"] == len(y) - o.d - o.D * m and r["nu"] == r["n"] - (o.p + m * o.P), (name, s)
        coefs = fit["phi"] + fit["theta"] + fit["Phi"] + fit["Theta"]
        rep["on_box"] += any(abs(v) == A.COEF_BOX for v in coefs)
        if r["degenerate"]:                      # the fit reproduces the series: both sums of squares are rounding noise
            assert A.degenerate(f.css, r["gross"]), (name, s, f.css, r["gross"])
            rep["degenerate"] += 1
        elif method == "css":                    # (the refit moves the coefficients and leaves css, sigma2 and aicc as the CSS run set them)
            rep["css"] = max(rep["css"], float(abs(f.css - r["css"]) / r["css"]))
            rep["sigma2"] = max(rep["sigma2"], float(abs(f.sigma2 - r["sigma2"]) / r["sigma2"]))
            rep["aicc"] = max(rep["aicc"], float(abs(f.aicc - r["aicc"])))
        scale = float(np.max(np.abs(y))) or 1.0
        rep["forecast"] = max(rep["forecast"], float(np.max(np.abs(fc - r["forecast"]))) / scale)
        # admissibility: the selected model passed the oracle's rule; numpy's roots agree up to the margin
        x = np.array(f.x[:], dtype=np.float64)
        assert L.oracle_arima_roots_ok(C.byref(o), x.ctypes.data), (name, s)
        rep["root_gap"] = min(rep["root_gap"], r["root"] - A.ROOT_MIN)
        # exact likelihood where the device refits (state dimension <= 32, no seasonal terms of a period above 24)
        La, Lb = o.p + m * o.P, o.q + m * o.Q
        if max(La, Lb + 1) <= 32 and not (m > 24 and (o.P or o.Q)) and not r["degenerate"]:
            w = _levels(y, o.d, o.D, m)[-1]
            ml = L.oracle_arima_ml(C.byref(o), x.ctypes.data, w.ctypes.data, len(w))
            assert np.isfinite(ml), (name, s)
            mine = A.exact_loglik(fit, r["w"])
            rep["loglik"] = max(rep["loglik"], float(abs(ml - mine)))
            rep["ml"] += 1
            if method == "css-ml":               # same orders as the CSS run; the refit keeps a point only if its likelihood is no worse
                base = X._CACHE[("cpu-fit", name, "css", s)]
                assert [fit[k] for k in ORDER_KEYS] == [base[k] for k in ORDER_KEYS], (name, s)
                assert mine <= A.exact_loglik(base, r["w"]) + A.LOGLIK_ABS, (name, s)
                rep["moved"] += fit != base
        elif method == "css-ml":                 # no refit: a long period's seasonal terms, a state dimension above 32, a degenerate fit
            if not r["degenerate"]:
                assert fit == X._CACHE[("cpu-fit", name, "css", s)], (name, s)
        X._CACHE[("cpu-fit", name, method, s)] = fit
    _SEEN["families"].add(name)
    return rep


ORDER_KEYS = ("p", "d", "q", "P", "D", "Q", "has_constant")


@pytest.mark.parametrize("name", X.FAMILY_NAMES)
def test_oracle_equals_the_restatement(oracle, name):
    """Every quantity within the constants of arima_ref.py (16 x the worst deviation measured here), with the CSS estimates and with
    the exact-likelihood refit's; no series needs the edge rule."""
    box = name == "box"
    for method in METHODS:
        rep = _family_report(oracle, name, method)
        assert rep["fitted"] == len(X.family(name)["series"]), rep
        assert rep["exempt"] == 0, rep
        assert rep["css"] <= (A.CSS_REL_BOX if box else A.CSS_REL) and rep["sigma2"] <= (A.CSS_REL_BOX if box else A.CSS_REL), rep
        assert rep["aicc"] <= (A.AICC_ABS_BOX if box else A.AICC_ABS), rep
        assert rep["forecast"] <= (A.FORECAST_REL_BOX if box else A.FORECAST_REL), rep
        assert rep["loglik"] <= (A.LOGLIK_ABS_BOX if box else A.LOGLIK_ABS), rep
        assert rep["strength"] <= A.STRENGTH_ABS, rep
        assert rep["root_gap"] >= -A.ROOT_MARGIN, rep
        if box:
            assert rep["on_box"] >= 6, rep
    assert _family_report(oracle, name, "css-ml")["moved"] >= 1, name          # the refit is not a no-op


def test_families_reach_what_they_claim(oracle):
    """The selected models cover every pass variant on every home of the ring and every pair of differences -- exactly the intended
    sets; the cases are what gets adjusted if they do not."""
    for name in X.FAMILY_NAMES:
        for method in METHODS:
            _family_report(oracle, name, method)
    assert _SEEN["classes"] == X.INTENDED_CLASSES, (_SEEN["classes"] ^ X.INTENDED_CLASSES)
    assert _SEEN["differences"] == X.INTENDED_DIFFERENCES, _SEEN["differences"]
    for f in (X.family(n) for n in X.FAMILY_NAMES + ["ragged-second"]):
        assert len(f["series"]) <= 192 and max(len(y) for y in f["series"]) <= 260 and f["h"] <= 40, f["name"]


def test_cascade_equals_the_expanded_form_at_the_start_up_rows(oracle):
    """oracle_arima_css (four cascaded filters) against the two expanded polynomials for every order class at lengths just above
    La = p + m P, where most of the pass is start-up: n - La = 1, 2, 3 and m + 1 -- random coefficients across the whole box."""
    L = oracle.lib()
    L.oracle_arima_css.restype = C.c_double
    L.oracle_arima_css.argtypes = [C.POINTER(K.ArimaOrder), C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)]
    rng = np.random.default_rng(77)
    worst, count = 0.0, 0
    for m in (1, 7, 12, 30):
        for (p, q, P, Q) in [(1, 1, 0, 0), (2, 3, 0, 0), (5, 0, 0, 0), (0, 5, 0, 0), (1, 1, 1, 1), (1, 2, 1, 2), (2, 1, 2, 0), (0, 1, 2, 2), (3, 0, 1, 1), (0, 3, 0, 2)]:
            if m == 1 and (P or Q):
                continue
            for extra in (1, 2, 3, m + 1, 40):
                for c in (0, 1):
                    if p + q + P + Q + c > 6:
                        continue
                    n = p + m * P + extra
                    x = np.concatenate([rng.uniform(-1.2, 1.2, p + q + P + Q), [0.7] * c, np.zeros(6)])[:6].copy()
                    w = rng.normal(0.5, 1.0, n)
                    o = K.ArimaOrder(p, 0, q, P, 0, Q, m, c)
                    css, nu = C.c_double(), C.c_int()
                    L.oracle_arima_css(C.byref(o), x.ctypes.data, w.ctypes.data, n, C.byref(css), C.byref(nu))
                    fit = X.fit_from_coordinates((p, 0, q, P, 0, Q, c), x, m)
                    want, wnu = A.css(fit, w)
                    assert nu.value == wnu == extra, (m, p, q, P, Q, extra)
                    worst = max(worst, float(abs(css.value - want) / want))
                    count += 1
    print(f"cascade against expanded form at the start-up rows: worst relative deviation {worst:.3e} over {count} passes")
    assert worst <= A.CSS_REL_BOX, worst


def test_restatement_basics():
    """The restatement against facts that need no oracle: an AR(1) autocovariance, a white-noise likelihood, a random-walk forecast, a
    seasonal-naive forecast across the wrap, the KPSS lag at 18 and 19, and the criteria's algebra."""
    fit = dict(p=1, d=0, q=0, P=0, D=0, Q=0, m=1, has_constant=False, phi=[0.5, 0, 0, 0, 0], theta=[0.0] * 5, Phi=[0.0, 0.0], Theta=[0.0, 0.0], constant=0.0)
    g = A.autocovariances(fit, 4)
    assert np.allclose(np.asarray(g, dtype=float), [4 / 3, 2 / 3, 1 / 3, 1 / 6], rtol=1e-15)
    wn = dict(fit, p=0, phi=[0.0] * 5)
    w = np.array([1.0, -2.0, 0.5, 3.0])
    assert abs(float(A.exact_loglik(wn, w)) - 0.5 * np.log(np.mean(w * w))) < 1e-15
    rw = dict(wn, d=1)
    assert np.array_equal(np.asarray(A.forecast(rw, [3.0, 5.0, 4.0], 3), dtype=float), [4.0, 4.0, 4.0])
    sn = dict(wn, D=1, m=3)
    assert np.array_equal(np.asarray(A.forecast(sn, [1.0, 2.0, 3.0, 4.0, 5.0, 6.0], 7), dtype=float), [4.0, 5.0, 6.0, 4.0, 5.0, 6.0, 4.0])
    drift = dict(wn, d=1, has_constant=True, constant=2.0)
    assert np.array_equal(np.asarray(A.forecast(drift, [3.0, 5.0, 4.0], 2), dtype=float), [6.0, 8.0])
    assert A.kpss_lag(18) == 0 and A.kpss_lag(19) == 1
    c = A.criteria(50.0, 48, 50, 3)
    assert abs(float(c["aicc"] - (50 * np.log(50.0 / 48) + 6 + 24 / 46))) < 1e-13 and abs(float(c["bic"] - (c["aic"] - 6 + 3 * np.log(50.0)))) < 1e-13
    ar2 = dict(fit, p=2, phi=[-0.99, -0.99, 0, 0, 0])
    assert abs(A.roots_min_modulus(ar2) - 1.0 / np.sqrt(0.99)) < 1e-12
    seas = dict(wn, P=1, m=12, Phi=[0.5, 0.0])
    assert abs(A.roots_min_modulus(seas) - 2.0 ** (1.0 / 12.0)) < 1e-12
