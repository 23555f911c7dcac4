"""No GPU: the ABI of the ARIMA model-path entries (symbols, the options struct, every argument error and its text -- all of them come
before the device is touched) and the restatement tests/arima_paths_ref.py against what it must be: the 80-bit forecasts and
conditional sum of squares of tests/arima_ref.py under zero innovations, an independent closed form, the sampling theory of its
Gaussian paths, and the rules of its statuses and broken paths."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import arima_cases as X
import arima_paths_cases as K
import arima_paths_ref as AP
import arima_ref as A
import ets_paths_ref as E
import inspect_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "anofox_fcst_hip.h")
NEW_SYMBOLS = ("anofox_hip_batch_arima_fit_device", "anofox_hip_arima_innovations_device", "anofox_hip_arima_paths_device",
               "anofox_hip_batch_arima_paths")
ACCEPTED = ((7, 28), (12, 24), (24, 48), (52, 26), (168, 48), (1, 64))          # (m, h) pairs the ring limit must admit


# --------------------------------------------------------------------------------------------
# symbols and validation
# --------------------------------------------------------------------------------------------
def test_symbols_struct_and_constants(hiplib):
    L = hiplib.load()
    header = open(HEADER).read()
    for s in NEW_SYMBOLS:
        assert s in hiplib.EXPORTED_SYMBOLS and hasattr(L, s) and re.search(r"\b%s\(" % s, header), s
    assert C.sizeof(hiplib.AnofoxHipArimaPathsOptions) == 24 and hiplib.AnofoxHipArimaPathsOptions.seed.offset == 16
    for name, value in (("ANOFOX_HIP_ARIMA_PATHS_MAX_PERIOD", hiplib.ARIMA_PATHS_MAX_PERIOD),
                        ("ANOFOX_HIP_ARIMA_PATHS_MAX_LDS_ROWS", hiplib.ARIMA_PATHS_MAX_LDS_ROWS)):
        assert re.search(r"#define %s %d\b" % (name, value), header), name
    assert re.search(r"ANOFOX_ARIMA_PATHS_GAUSSIAN = 0, ANOFOX_ARIMA_PATHS_BOOTSTRAP = 1", header)
    assert re.search(r"ANOFOX_ARIMA_PATHS_NO_MODEL = %d\b" % hiplib.ARIMA_PATHS_NO_MODEL, header)
    assert hiplib.ARIMA_PATHS_INNOVATIONS == {"gaussian": AP.GAUSSIAN, "bootstrap": AP.BOOTSTRAP} and hiplib.ARIMA_PATHS_NO_MODEL == AP.NO_MODEL
    assert (hiplib.ARIMA_PATHS_MAX_PERIOD, hiplib.ARIMA_PATHS_MAX_LDS_ROWS) == (AP.MAX_PERIOD, AP.MAX_LDS_ROWS)
    with pytest.raises(ValueError):
        hiplib.make_arima_paths_options("student")


def _paths_call(hiplib, opts=None, struct_size=None, m=7, pool_rows=8, n_series=0, horizon=5, n_paths=3, ld=64, ld_out=64, t_rows=16):
    """anofox_hip_arima_paths_device on host dummies: every call here is refused, or has n_series = 0 and returns before the device."""
    L = hiplib.load()
    o = hiplib.make_arima_paths_options() if opts is None else opts
    ints = np.zeros(64 * 8, dtype=np.int32)
    dbl = np.zeros(64 * 16)
    err = hiplib.AnofoxError()
    ok = L.anofox_hip_arima_paths_device(ints.ctypes.data, dbl.ctypes.data, ld, dbl.ctypes.data, ints.ctypes.data, t_rows, dbl.ctypes.data,
                                         ints.ctypes.data, dbl.ctypes.data, m, pool_rows, n_series, horizon, n_paths, C.byref(o),
                                         C.sizeof(o) if struct_size is None else struct_size, dbl.ctypes.data, ld_out, ints.ctypes.data,
                                         ints.ctypes.data, None, C.byref(err))
    return bool(ok), int(err.code), err.message.decode()


def test_every_argument_error_names_its_limit_before_the_device(hiplib):
    joint = hiplib.make_arima_paths_options("bootstrap", joint=True)
    bad_mode, bad_joint, joint_gauss = hiplib.make_arima_paths_options(), hiplib.make_arima_paths_options("bootstrap"), hiplib.make_arima_paths_options()
    bad_mode.innovations, bad_joint.joint, joint_gauss.joint = 2, 2, 1
    cases = [
        (dict(struct_size=16), "struct_size is not sizeof(AnofoxHipArimaPathsOptions)"),
        (dict(opts=bad_mode), "innovations 2 is unknown"),
        (dict(opts=bad_joint), "joint 2 is neither 0 nor 1"),
        (dict(opts=joint_gauss), "no joint Gaussian mode"),
        (dict(n_paths=0), "n_paths is 0"),
        (dict(n_paths=2049), "exceeds the limit of 2048 paths"),
        (dict(horizon=0), "horizon must be at least 1"),
        (dict(n_paths=2048, horizon=(1 << 19) + 1), "exceeds the limit of 2^30 rows"),
        (dict(n_series=65, ld_out=64, ld=128), "ld_out is smaller than n_series"),
        (dict(n_series=65, ld_out=128, ld=64), "ld is smaller than n_series"),
        (dict(t_rows=1 << 31), "t_rows exceeds the limit of 2^31 - 1"),
        (dict(m=0), "the seasonal period m is 0"),
        (dict(m=2049), "m = 2049 exceeds the limit of 2048"),
        (dict(m=30, horizon=50), "= 130 exceeds the limit of 128 LDS rows"),
        (dict(m=168, horizon=65), "= 130 exceeds the limit of 128 LDS rows"),
        (dict(opts=joint, pool_rows=(1 << 20) + 1), "pool_rows 1048577 exceeds the limit of 2^20"),
    ]
    for kwargs, text in cases:
        ok, code, message = _paths_call(hiplib, **kwargs)
        assert not ok and code == hiplib.INVALID_INPUT and text in message, (kwargs, code, message)
    for m, h in ACCEPTED:                                      # n_series = 0: accepted, and nothing to do
        assert AP.lds_rows(m, h) <= AP.MAX_LDS_ROWS
        assert _paths_call(hiplib, m=m, horizon=h) == (True, 0, ""), (m, h)
    assert _paths_call(hiplib, m=168, horizon=64) == (True, 0, "")               # 128 rows: the limit itself
    assert _paths_call(hiplib, pool_rows=(1 << 20) + 1) == (True, 0, "")         # (pool_rows is read in joint mode only)
    # the innovations entry and the two batch entries
    L = hiplib.load()
    ints, dbl, err = np.zeros(64 * 8, dtype=np.int32), np.zeros(64 * 16), hiplib.AnofoxError()
    inn = lambda ld=64, m=7, n=0, T=16: L.anofox_hip_arima_innovations_device(ints.ctypes.data, dbl.ctypes.data, ld, dbl.ctypes.data, ints.ctypes.data, m, n,
                                                                              T, dbl.ctypes.data, ints.ctypes.data, dbl.ctypes.data, None, C.byref(err))
    for kwargs, text in ((dict(n=65), "ld is smaller than n_series"), (dict(T=1 << 31), "t_rows exceeds the limit of 2^31 - 1"),
                         (dict(m=0), "the seasonal period m is 0"), (dict(m=2049), "exceeds the limit of 2048")):
        assert not inn(**kwargs) and err.code == hiplib.INVALID_INPUT and text in err.message.decode(), (kwargs, err.message)
    assert inn() and err.code == 0
    o = hiplib.make_arima_paths_options()
    lv = np.array([0.5])
    assert not L.anofox_hip_batch_arima_paths(None, C.byref(o), 8, 10, lv.ctypes.data, 1, 0, None, None, None, None, None, None, C.byref(err))
    assert err.code == hiplib.INVALID_INPUT and "struct_size" in err.message.decode()
    assert not L.anofox_hip_batch_arima_paths(None, C.byref(o), C.sizeof(o), 4096, lv.ctypes.data, 1, 0, None, None, None, None, None, None, C.byref(err))
    assert err.code == hiplib.INVALID_INPUT and "exceeds the limit of 2048 paths" in err.message.decode()
    assert not L.anofox_hip_batch_arima_paths(None, C.byref(o), C.sizeof(o), 10, lv.ctypes.data, 17, 0, None, None, None, None, None, None, C.byref(err))
    assert err.code == hiplib.INVALID_INPUT and "exceeds the limit of 16 levels" in err.message.decode()
    assert not L.anofox_hip_batch_arima_paths(None, C.byref(o), C.sizeof(o), 10, lv.ctypes.data, 1, 0, None, None, None, None, None, None, C.byref(err))
    assert err.code == hiplib.NULL_POINTER
    assert not L.anofox_hip_batch_arima_fit_device(None, None, None, C.byref(err)) and err.code == hiplib.NULL_POINTER


# --------------------------------------------------------------------------------------------
# the restatement against the 80-bit restatement of the fit
# --------------------------------------------------------------------------------------------
_WORST = {"forecast": (0.0, ""), "css": (0.0, ""), "innovations": (0.0, "")}


def _oracle_fit(O, name, s, y, m, h):
    key = ("cpu-fit", name, "css", s)
    if key not in X._CACHE:
        got = IC.arima_detail(O, y, m, h) if len(y) >= 3 else None
        if got is None:
            return None
        o = got[0].ord
        X._CACHE[key] = X.fit_from_coordinates((o.p, o.d, o.q, o.P, o.D, o.Q, o.with_constant), got[0].x[:], m)
    return X._CACHE[key]


@pytest.mark.parametrize("name", X.FAMILY_NAMES)
def test_zero_innovations_give_the_forecast_and_the_css_recursion(oracle, name):
    """With every innovation zero the paths are arima_ref.forecast (80-bit, the multiplied-out operator) and the in-sample
    innovations and sigma^2 are arima_ref.css, on the oracle's fits of every family, within the constants measured here."""
    fam = X.family(name)
    m, h = max(fam["m"], 1), fam["h"]
    worst_f = worst_c = worst_e = 0.0
    fitted = 0
    for s, y in enumerate(X.cleaned(fam)):
        fit = _oracle_fit(oracle, name, s, y, fam["m"], h)
        if fit is None:
            continue
        fitted += 1
        r = X.replay(("cpu", name, "css", s), fit, y, h)
        x, e, css, nu, sigma = AP.css_one(fit, y)
        assert nu == r["nu"] and len(x) == r["n"]
        got = AP.simulate(fit, y, x, e, np.zeros((1, h)))[0]
        scale = float(np.max(np.abs(y))) or 1.0
        worst_f = max(worst_f, float(np.max(np.abs(got - r["forecast"]))) / scale)
        La = fit["p"] + m * fit["P"]
        _, _, e80, _ = A.css(fit, r["w"], detail=True)
        if not r["degenerate"]:
            worst_c = max(worst_c, float(abs(css - r["css"]) / r["css"]), float(abs(sigma * sigma - r["sigma2"]) / r["sigma2"]))
            # the innovations themselves, on the scale of their root mean square
            rms = float(np.sqrt(r["css"] / r["nu"]))
            worst_e = max(worst_e, float(np.max(np.abs(e[La:] - e80[La:]))) / rms)
    assert fitted >= 1
    for k, v in (("forecast", worst_f), ("css", worst_c), ("innovations", worst_e)):
        if v > _WORST[k][0]:
            _WORST[k] = (v, name)
    print(f"{name}: {fitted} fits, forecast {worst_f:.3e} (rel. max |y|), css and sigma^2 {worst_c:.3e} (rel.), innovations {worst_e:.3e} "
          f"(rel. their rms); worst so far {_WORST}")
    assert worst_f <= AP.FORECAST_REL and worst_c <= AP.CSS_REL and worst_e <= AP.INNOVATION_REL, (name, worst_f, worst_c, worst_e)


# --------------------------------------------------------------------------------------------
# an independent closed form and the sampling theory
# --------------------------------------------------------------------------------------------
def _fit(**kw):
    f = dict(p=0, d=0, q=0, P=0, D=0, Q=0, m=1, has_constant=False, phi=[], theta=[], Phi=[], Theta=[], constant=0.0)
    f.update(kw)
    return f


def test_closed_forms_of_ar1_and_integrated_ma1():
    """AR(1), d = 0: y_(T+k) = phi^(k+1) x_T + sum_j phi^j e_(k-j).  MA(1), d = 1: y_(T+k) = y_T - theta e_T + sum_j psi_j e_(k-j) with
    psi_0 = 1 and psi_j = 1 - theta: written out by hand, compared within rounding of a sum of h terms."""
    rng = np.random.default_rng(7)
    h, n_paths = 12, 5
    y = 10.0 + np.cumsum(rng.normal(0, 1, 40))
    draws = rng.normal(0, 1, (n_paths, h))
    phi = 0.7
    f = _fit(p=1, phi=[phi])
    x, e, *_ = AP.css_one(f, y)
    got = AP.simulate(f, y, x, e, draws)
    for p in range(n_paths):
        for k in range(h):
            want = phi ** (k + 1) * y[-1] + sum(phi ** j * draws[p, k - j] for j in range(k + 1))
            assert abs(got[p, k] - want) <= 64 * np.finfo(float).eps * (abs(y[-1]) + np.abs(draws[p]).sum()), (p, k)
    theta = 0.4
    f = _fit(d=1, q=1, theta=[theta])
    x, e, *_ = AP.css_one(f, y)
    got = AP.simulate(f, y, x, e, draws)
    for p in range(n_paths):
        for k in range(h):
            want = y[-1] - theta * e[-1] + draws[p, k] + (1.0 - theta) * draws[p, :k].sum()
            assert abs(got[p, k] - want) <= 64 * np.finfo(float).eps * (abs(y[-1]) + np.abs(draws[p]).sum()), (p, k)


def test_gaussian_paths_have_the_variance_of_the_psi_weights(oracle):
    """ARIMA(1,1,1)(1,0,0)7: Var(y_(T+h)) = sigma^2 sum psi_j^2 with psi from the multiplied-out operator.  The sample variance of P
    paths has relative standard deviation sqrt(2 / (P - 1)); accepted within 5 of them."""
    m, h, n_paths, sigma = 7, 14, 4000, 1.5
    f = _fit(p=1, d=1, q=1, P=1, m=m, phi=[0.5], theta=[0.3], Phi=[0.4])
    rng = np.random.default_rng(11)
    y = X.simulate(rng, 80, phi=(0.5,), theta=(0.3,), Phi=(0.4,), m=m, d=1, sd=sigma, level=30.0)
    orders, coef = AP.blocks_of([f], 1, [len(y)], m)
    Y = y.reshape(-1, 1)
    resid, rl, _ = AP.innovations(orders, coef, Y, [len(y)], m)
    block, status, n_broken = AP.paths(orders, coef, Y, [len(y)], resid, rl, np.array([sigma]), m, n_paths, h, AP.GAUSSIAN, seed=3)
    assert status[0] == AP.OK and n_broken[0] == 0
    cube = block.reshape(n_paths, h)
    ar, ma = [np.asarray(v, dtype=np.float64) for v in A.polynomials(f)]
    full = np.convolve(ar, [1.0, -1.0])
    psi = np.zeros(h)
    for j in range(h):
        psi[j] = (ma[j] if j < len(ma) else 0.0) - sum(full[k] * psi[j - k] for k in range(1, min(j, len(full) - 1) + 1))
    tol = 5.0 * np.sqrt(2.0 / (n_paths - 1))
    for k in range(h):
        want = sigma * sigma * float((psi[:k + 1] ** 2).sum())
        got = float(cube[:, k].var(ddof=1))
        assert abs(got - want) <= tol * want, (k, got, want)


def test_gaussian_draws_are_not_the_ets_stream(oracle):
    a = AP.normal_draws(5, 3, 4, 9)
    b = E.normal_draws(5, 3, 4, 9)
    assert a.shape == b.shape and np.all(np.isfinite(a)) and not np.any(a == b)
    assert np.array_equal(a, AP.normal_draws(5, 3, 4, 9)) and not np.array_equal(a, AP.normal_draws(6, 3, 4, 9))


# --------------------------------------------------------------------------------------------
# statuses and broken paths
# --------------------------------------------------------------------------------------------
def test_statuses_and_their_precedence():
    b = K.batch(7, K.chunk_combos(0)[:20], seed=1)
    resid, rl, sigma = [np.array(v) for v in K.innovations(b)]
    n = b["n"]
    st = lambda **kw: AP.paths(b["orders"], b["coef"], b["y"], b["lengths"], kw.pop("resid", resid), kw.pop("rl", rl), kw.pop("sigma", sigma), 7, 2, 3,
                               draws=np.zeros((2, 3, n)), n_series=n, **kw)[1]
    base = st()
    assert set(base) == {AP.OK, AP.NO_MODEL} and all((base[s] == AP.NO_MODEL) == (s % 9 == 7) for s in range(n))
    good = int(np.flatnonzero(base == AP.OK)[0])
    sg = sigma.copy()
    sg[good] = np.nan
    assert st(sigma=sg)[good] == AP.NAN and st(sigma=sg, innovations=AP.BOOTSTRAP)[good] == AP.OK       # the bootstrap does not read sigma
    short = int(rl[base == AP.OK].min())
    joint = st(innovations=AP.BOOTSTRAP, joint=True, pool_rows=short + 1)
    assert all(joint[s] == (AP.NO_MODEL if base[s] else (AP.RAGGED if rl[s] < short + 1 else AP.OK)) for s in range(n))
    assert all(v in (AP.NO_MODEL, AP.EMPTY) for v in st(innovations=AP.BOOTSTRAP, joint=True, pool_rows=0))
    r2 = resid.copy()
    r2[0, good] = np.nan                                     # the first residual: in the pool, not in a short MA tail
    assert st(resid=r2, innovations=AP.BOOTSTRAP)[good] == AP.NAN
    assert st(resid=r2, innovations=AP.BOOTSTRAP, joint=True, pool_rows=int(rl[good]) + 1)[good] == AP.RAGGED       # RAGGED before NAN
    rl2 = rl.copy()
    rl2[good] += 1
    assert st(rl=rl2)[good] == AP.NO_MODEL


@pytest.mark.parametrize("mode", ["gaussian", "own", "joint"])
def test_the_status_scenario_of_the_gpu_test_is_what_it_claims(oracle, mode):
    sc = K.status_scenario()
    b, n_paths, h = sc["batch"], 3, 9
    block, status, n_broken = AP.paths(sc["orders"], sc["coef"], sc["y"], b["lengths"], sc["resid"], sc["rl"], sc["sigma"], 7, n_paths, h,
                                       AP.GAUSSIAN if mode == "gaussian" else AP.BOOTSTRAP, joint=mode == "joint", pool_rows=sc["joint_rows"], seed=7,
                                       n_series=b["n"])
    K.check_status_scenario(sc, mode, status, n_broken, block, n_paths)


def test_an_overflowing_path_is_broken_from_that_step_on():
    f = _fit(d=2, has_constant=True, constant=1.0e308)
    y = np.array([1.0, 2.0, 4.0, 7.0, 11.0])
    x, e, *_ = AP.css_one(f, y)
    got = AP.simulate(f, y, x, e, np.zeros((1, 6)))[0]
    first = int(np.flatnonzero(np.isnan(got))[0])
    assert 0 < first < 6 and np.all(np.isfinite(got[:first])) and np.all(np.isnan(got[first:]))
