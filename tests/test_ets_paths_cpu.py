"""No GPU: the ABI of the model-path entries (symbols, the options struct, every argument error and its text -- all of them come before
the device is touched) and the restatement tests/ets_paths_ref.py against what it must be: the textbook point forecasts under zero
innovations, an independent closed form for the linear models, the sampling theory of its normal draws, and the broken-path rule."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import ets_paths_cases as K
import ets_paths_ref as E
import inspect_ref as R
import paths_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "anofox_fcst_hip.h")
NEW_SYMBOLS = ("anofox_hip_batch_inspect_device", "anofox_hip_ets_innovations_device", "anofox_hip_ets_paths_device",
               "anofox_hip_batch_ets_paths")
LD = np.longdouble
EPS = np.finfo(np.float64).eps


# --------------------------------------------------------------------------------------------
# symbols and validation
# --------------------------------------------------------------------------------------------
def test_symbols_struct_and_constants(hiplib):
    L = hiplib.load()
    header = open(HEADER).read()
    for s in NEW_SYMBOLS:
        assert s in hiplib.EXPORTED_SYMBOLS and hasattr(L, s) and re.search(r"\b%s\(" % s, header), s
    assert C.sizeof(hiplib.AnofoxHipEtsPathsOptions) == 24 and hiplib.AnofoxHipEtsPathsOptions.seed.offset == 16
    for name, value in (("ANOFOX_HIP_ETS_PATHS_MAX_PERIOD", hiplib.ETS_PATHS_MAX_PERIOD), ("ANOFOX_HIP_ETS_PATHS_MAX_RING", hiplib.ETS_PATHS_MAX_RING)):
        assert re.search(r"#define %s %d\b" % (name, value), header), name
    assert re.search(r"ANOFOX_ETS_PATHS_GAUSSIAN = 0, ANOFOX_ETS_PATHS_BOOTSTRAP = 1", header)
    assert re.search(r"ANOFOX_ETS_PATHS_NO_MODEL = %d\b" % hiplib.ETS_PATHS_NO_MODEL, header)
    assert hiplib.ETS_PATHS_INNOVATIONS == {"gaussian": E.GAUSSIAN, "bootstrap": E.BOOTSTRAP} and hiplib.ETS_PATHS_NO_MODEL == E.NO_MODEL
    assert (hiplib.ETS_PATHS_MAX_PERIOD, hiplib.ETS_PATHS_MAX_RING) == (E.MAX_PERIOD, E.MAX_RING)
    assert (hiplib.PATHS_OK, hiplib.PATHS_EMPTY, hiplib.PATHS_NAN, hiplib.PATHS_RAGGED) == (E.OK, E.EMPTY, E.NAN, E.RAGGED)
    with pytest.raises(ValueError):
        hiplib.make_ets_paths_options("student")


def _device_call(hiplib, opts=None, struct_size=None, m=7, pool=True, pool_rows=8, n_series=0, horizon=5, n_paths=3, ld=64, ld_out=64):
    """anofox_hip_ets_paths_device on host dummies: every call here is refused, or has n_series = 0 and returns before the device."""
    L = hiplib.load()
    o = hiplib.make_ets_paths_options() if opts is None else opts
    ints = np.zeros(64, dtype=np.int32)
    dbl = np.zeros(64 * 16)
    err = hiplib.AnofoxError()
    ok = L.anofox_hip_ets_paths_device(ints.ctypes.data, dbl.ctypes.data, dbl.ctypes.data, ld, m, ints.ctypes.data,
                                       dbl.ctypes.data if pool else None, 1, 64, None, pool_rows, n_series, horizon, n_paths, C.byref(o),
                                       C.sizeof(o) if struct_size is None else struct_size, dbl.ctypes.data, ld_out, ints.ctypes.data,
                                       ints.ctypes.data, None, C.byref(err))
    return bool(ok), int(err.code), err.message.decode()


def test_every_argument_error_names_its_limit_before_the_device(hiplib):
    boot = hiplib.make_ets_paths_options("bootstrap")
    joint_gauss = hiplib.make_ets_paths_options("gaussian", joint=True)
    cases = (
        (dict(struct_size=16), "struct_size is not sizeof(AnofoxHipEtsPathsOptions)"),
        (dict(opts=hiplib.make_ets_paths_options(2)), "innovations 2 is unknown: 0 (Gaussian) or 1 (bootstrap)"),
        (dict(opts=joint_gauss), "no joint Gaussian mode"),
        (dict(n_paths=0), "n_paths is 0"),
        (dict(n_paths=2049), "exceeds the limit of 2048 paths"),
        (dict(horizon=0), "horizon must be at least 1"),
        (dict(n_paths=2048, horizon=(1 << 19) + 1, m=1), "exceeds the limit of 2^30 rows"),
        (dict(n_series=65, ld_out=64, ld=128), "ld_out is smaller than n_series"),
        (dict(n_series=65, ld_out=128, ld=64), "ld is smaller than n_series"),
        (dict(m=0), "m is 0, it must be at least 1"),
        (dict(m=2049), "m = 2049 exceeds the limit of 2048"),
        (dict(m=129, horizon=129), "R = min(m, horizon) = 129 exceeds the limit of 128"),
        (dict(m=2048, horizon=200), "R = min(m, horizon) = 200 exceeds the limit of 128"),
        (dict(opts=boot, pool=False), "the bootstrap needs a pool"),
        (dict(opts=boot, pool_rows=(1 << 20) + 1), "exceeds the limit of 2^20"),
    )
    for kwargs, text in cases:
        ok, code, message = _device_call(hiplib, **kwargs)
        assert not ok and code == hiplib.INVALID_INPUT and message.startswith("Invalid input: ") and text in message, (kwargs, message)
    # at the limits themselves nothing is refused (no series: the call returns before the device)
    for kwargs in (dict(m=128, horizon=500), dict(m=2048, horizon=128), dict(n_paths=2048, horizon=1 << 19, m=1),
                   dict(opts=boot, pool_rows=1 << 20), dict(opts=hiplib.make_ets_paths_options("bootstrap", joint=True))):
        assert _device_call(hiplib, **kwargs) == (True, 0, ""), kwargs
    L = hiplib.load()
    err = hiplib.AnofoxError()
    o = hiplib.make_ets_paths_options()
    assert not L.anofox_hip_ets_paths_device(None, None, None, 64, 7, None, None, 1, 64, None, 0, 0, 5, 3, C.byref(o), C.sizeof(o), None, 64,
                                             None, None, None, C.byref(err)) and err.code == hiplib.NULL_POINTER


def test_batch_entry_and_the_other_entries_without_a_device(hiplib):
    L = hiplib.load()
    levels = np.array([0.1, 0.5, 0.9])
    ld = C.c_size_t(7)

    def sizing(o, struct_size=None, n_paths=10, lv=levels, k=3):
        err = hiplib.AnofoxError()
        ok = L.anofox_hip_batch_ets_paths(None, C.byref(o), C.sizeof(o) if struct_size is None else struct_size, n_paths,
                                          lv.ctypes.data if lv is not None else None, k, 0, None, None, None, None, None, C.byref(ld), C.byref(err))
        return bool(ok), int(err.code), err.message.decode()

    o = hiplib.make_ets_paths_options("bootstrap", joint=True, seed=5)
    # the argument checks come first and name their limit; then the batch, which cannot exist without a device
    assert sizing(o) == (False, hiplib.NULL_POINTER, "Null pointer argument")
    for kwargs, text in ((dict(struct_size=8), "struct_size"), (dict(n_paths=0), "n_paths is 0"), (dict(n_paths=4096), "limit of 2048 paths"),
                         (dict(k=0), "n_levels is 0"), (dict(k=17, lv=np.full(17, 0.5)), "limit of 16 levels"),
                         (dict(lv=np.array([0.1, 1.5, 0.9])), "outside [0, 1]")):
        ok, code, message = sizing(o, **kwargs)
        assert not ok and code == hiplib.INVALID_INPUT and text in message, (kwargs, message)
    ok, code, message = sizing(hiplib.make_ets_paths_options("gaussian", joint=True))
    assert not ok and code == hiplib.INVALID_INPUT and "no joint Gaussian mode" in message
    assert ld.value == 7                                               # (nothing was written by a refused call)
    err = hiplib.AnofoxError()
    assert not L.anofox_hip_batch_inspect_device(None, None, None, None, C.byref(err)) and err.code == hiplib.NULL_POINTER
    d, i = np.zeros(64), np.zeros(64, dtype=np.int32)
    err = hiplib.AnofoxError()
    assert not L.anofox_hip_ets_innovations_device(d.ctypes.data, d.ctypes.data, 64, i.ctypes.data, i.ctypes.data, 65, 1, d.ctypes.data,
                                                   i.ctypes.data, None, C.byref(err))
    assert err.code == hiplib.INVALID_INPUT and "ld is smaller than n_series" in err.message.decode()
    err = hiplib.AnofoxError()
    assert L.anofox_hip_ets_innovations_device(d.ctypes.data, d.ctypes.data, 64, i.ctypes.data, i.ctypes.data, 0, 1, d.ctypes.data,
                                               i.ctypes.data, None, C.byref(err))
    from anofox_forecast_amd import api
    with pytest.raises(api.InvalidInputException, match="must be ETS or AutoETS"):
        api.ts_forecast_quantiles_by([], [], [], "Naive", 3, "1d", [0.5], paths="model_gaussian")
    with pytest.raises(api.InvalidInputException, match="is unknown"):
        api.ts_forecast_quantiles_by([], [], [], "AutoETS", 3, "1d", [0.5], paths="student")


# --------------------------------------------------------------------------------------------
# the restatement
# --------------------------------------------------------------------------------------------
def closed_form(rec, n, notation, m, h, dtype):
    """inspect_ref.forecast in the number format `dtype`: the textbook point forecasts of steps 1..h from the final states."""
    e, t, s = R.parts(notation)
    phi = dtype(rec["phi"]) if t in ("Ad", "Md") else dtype(1)
    damp = np.cumsum(phi ** np.arange(1, h + 1).astype(dtype))
    f = np.full(h, dtype(rec["level"]))
    if t in ("A", "Ad"):
        f = f + damp * dtype(rec["trend"])
    elif t in ("M", "Md"):
        f = f * dtype(rec["trend"]) ** damp
    if s != "N":
        st = np.asarray(rec["seasonal_states"], dtype=dtype)
        seas = np.array([st[(n + i - 1) % m] for i in range(1, h + 1)], dtype=dtype)
        f = f + seas if s == "A" else f * seas
    return f


@pytest.mark.parametrize("m", [1, 4, 7])
def test_zero_innovations_follow_the_textbook_point_forecasts(oracle, m):
    """All 25 specs: with a pool of zeros every path is the point forecast.  The margin is 16 x the deviation between the float64 and
    the long-double evaluation of the closed form on the same records, measured here (the ratios: DESIGN.md section 3)."""
    h, n, n_paths = 8, 50, 2
    rec = K.records(n, m, seed=11)
    block, status, n_broken = E.paths(rec["spec"], rec["info"], rec["states"], m, rec["lengths"], n_paths, h, E.BOOTSTRAP,
                                      pool=np.zeros((4, n)), seed=3)
    assert (status == E.OK).all() and (n_broken == 0).all() and not np.isnan(block).any()
    cube = block.reshape(n_paths, h, n)
    noise, worst = 0.0, 0.0
    for s in range(n):
        notation = R.notation_of(int(rec["spec"][s]))
        r = K.record_of(rec, s, m)
        f80 = closed_form(r, int(rec["lengths"][s]), notation, m, h, LD)
        assert R.dev(R.forecast(r, int(rec["lengths"][s]), notation, m, h), f80) == 0.0      # the closed form IS inspect_ref.forecast
        noise = max(noise, R.dev(closed_form(r, int(rec["lengths"][s]), notation, m, h, np.float64), f80))
        worst = max(worst, max(R.dev(cube[p, :, s], f80) for p in range(n_paths)))
    print(f"m={m}: noise {noise:.3e}, worst deviation {worst:.3e}, ratio {worst / noise if noise else float('nan'):.2f} of 16")
    assert noise > 0.0 and worst <= 16.0 * noise, (m, worst, noise)


@pytest.mark.parametrize("innovations", [E.GAUSSIAN, E.BOOTSTRAP])
@pytest.mark.parametrize("notation", ["ANN", "AAN"])
def test_linear_models_equal_an_independent_closed_form(oracle, notation, innovations):
    """y_k = l + (k + 1) b + alpha sum_{i<k} e_i + beta sum_{j<=k} sum_{i<j} e_i + e_k (0-based k; ANN has no b and beta terms), built with
    np.cumsum in long double from the same draws.  Margin: the forward error bound of a serial sum of k + 2 terms, (k + 2) eps
    sum |terms|.  A draw in the wrong step or state misses it by orders of magnitude."""
    m, h, n, n_paths = 4, 9, 7, 26
    rec = K.records(n, m, seed=5, notation=notation)
    pool = K.pool(rec, 13, seed=2)
    block, status, n_broken = E.paths(rec["spec"], rec["info"], rec["states"], m, rec["lengths"], n_paths, h, innovations, pool=pool, seed=77)
    assert (status == E.OK).all() and (n_broken == 0).all()
    e = E.innovations_of(rec["spec"], rec["info"], rec["lengths"], n_paths, h, innovations, status, pool, None, pool.shape[0], False, 77).astype(LD)
    assert np.abs(e).min() > 0.0 and len(np.unique(e)) > (h * n if innovations == E.BOOTSTRAP else n_paths * h * n - 1)
    cube = block.reshape(n_paths, h, n).astype(LD)
    alpha, level = rec["info"][0].astype(LD), rec["states"][0].astype(LD)
    before = np.cumsum(e, axis=1) - e                                   # sum_{i<k} e_i
    k1 = np.arange(1, h + 1).astype(LD)[None, :, None]
    want = level[None, None, :] + alpha[None, None, :] * before + e
    terms = np.abs(level)[None, None, :] + alpha[None, None, :] * (np.cumsum(np.abs(e), axis=1) - np.abs(e)) + np.abs(e)
    if notation == "AAN":
        beta, growth = rec["info"][1].astype(LD), rec["states"][1].astype(LD)
        want = want + k1 * growth[None, None, :] + beta[None, None, :] * np.cumsum(before, axis=1)
        terms = terms + k1 * np.abs(growth)[None, None, :] + beta[None, None, :] * np.cumsum(np.cumsum(np.abs(e), axis=1) - np.abs(e), axis=1)
    margin = (k1 + 1) * LD(EPS) * terms
    ratio = float(np.max(np.abs(cube - want) / margin))
    print(f"{notation} innovations {innovations}: worst error / margin {ratio:.3f}")
    assert ratio <= 1.0, ratio
    # the check bites: the next step's draw in place of this one's is far outside
    assert float(np.max(np.abs(cube[:, :-1] - (want[:, :-1] - e[:, :-1] + e[:, 1:])) / margin[:, :-1])) > 1e6


NORMAL_SEED = 20260321


def test_normal_draws(oracle):
    """2^16 draws of one seed: mean and variance inside the 5-sigma bounds of sampling theory, the tails cut below 6.77, and every draw
    where the contract puts it: words (w0, w1) serve steps 4j and 4j + 1 as r cos and r sin, (w2, w3) steps 4j + 2 and 4j + 3."""
    n_series, n_paths, h = 16, 64, 64
    z = E.normal_draws(NORMAL_SEED, n_series, n_paths, h)
    N = z.size
    assert N == 1 << 16 and not np.isnan(z).any()
    assert abs(z.mean()) <= 5.0 / math.sqrt(N), z.mean()
    assert abs(z.var() - 1.0) <= 5.0 * math.sqrt(2.0 / N), z.var()
    assert np.abs(z).max() < 6.77
    assert math.sqrt(-2.0 * math.log(0.5 * 2.0 ** -32)) < 6.77             # the largest |z| the 32-bit uniform can give
    w = E.normal_words(NORMAL_SEED, n_series, n_paths, h).astype(np.float64)      # [4, P, blocks, n]
    for pair in (0, 1):
        u1, u2 = (w[2 * pair] + 0.5) * 2.0 ** -32, (w[2 * pair + 1] + 0.5) * 2.0 ** -32
        r = np.sqrt(-2.0 * np.log(u1))
        even, odd = z[:, 2 * pair::4, :], z[:, 2 * pair + 1::4, :]
        assert even.shape == u1.shape and odd.shape == u1.shape
        assert np.max(np.abs(even - r * np.cos(2.0 * math.pi * u2))) < 1e-12 and np.max(np.abs(odd - r * np.sin(2.0 * math.pi * u2))) < 1e-12
    # the words are those of counter (p, s, block, 2) under the seed's key
    for p, s, blk in ((0, 0, 0), (63, 15, 15), (7, 3, 9)):
        assert tuple(int(v) for v in w[:, p, blk, s]) == P.philox4x32_10((p, s, blk, 2), P.key_of(NORMAL_SEED))
    # a horizon that ends inside a block and inside a pair takes the leading draws of the same blocks
    assert P.same_bits(E.normal_draws(NORMAL_SEED, 5, 3, 7), E.normal_draws(NORMAL_SEED, 5, 3, 64)[:, :7, :]).all()


def broken_record():
    """AMdN: a growth rate of 1 that innovations of -50 on a level of 10 drive to 1 + 0.3 (-50) / 10 = -0.5 after the first step."""
    info = np.full((8, 2), np.nan)
    states = np.full((3, 2), np.nan)
    info[0], info[1], info[3], info[7] = 0.3, 0.3, 0.9, 40.0
    states[0], states[1] = 10.0, 1.0
    return {"spec": np.array([R.spec_id("AMdN")] * 2, dtype=np.int32), "info": info, "states": states, "lengths": np.array([40, 41], dtype=np.int32)}


def test_broken_paths_are_nan_from_the_step_on_and_counted(oracle):
    rec = broken_record()
    pool = np.stack([np.full(6, -50.0), np.full(6, 0.25)], axis=1)     # series 1 stays whole
    n_paths, h = 5, 6
    block, status, n_broken = E.paths(rec["spec"], rec["info"], rec["states"], 1, rec["lengths"], n_paths, h, E.BOOTSTRAP, pool=pool, seed=1)
    cube = block.reshape(n_paths, h, 2)
    assert (status == E.OK).all() and list(n_broken) == [n_paths, 0]
    assert (cube[:, 0, 0] == 10.0 - 50.0).all() and np.isnan(cube[:, 1:, 0]).all() and np.isfinite(cube[:, :, 1]).all()
    # statuses: a spec that is none of the 25, no observation, a NaN parameter the spec reads and one it does not
    rec = K.records(6, 4, seed=9, notation="AAdA")
    rec["spec"][0] = R.spec_id("MAN") + 1                               # "MAA"
    rec["spec"][1] = 30
    rec["lengths"][2] = 0
    rec["info"][3, 3] = np.nan                                          # phi: read by AAdA
    rec["info"][4, 4] = np.nan                                          # aic: not read
    rec["states"][2 + (int(rec["lengths"][5]) + 2) % 4, 5] = np.nan     # the seasonal state of step 2's phase
    block, status, n_broken = E.paths(rec["spec"], rec["info"], rec["states"], 4, rec["lengths"], 3, 5, E.GAUSSIAN, seed=1)
    assert list(status) == [E.NO_MODEL, E.NO_MODEL, E.NO_MODEL, E.NAN, E.OK, E.NAN] and list(n_broken) == [3, 3, 3, 3, 0, 3]
    assert np.isnan(block[:, [0, 1, 2, 3, 5]]).all() and np.isfinite(block[:, 4]).all()
