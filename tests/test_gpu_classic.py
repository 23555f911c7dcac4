"""GPU: the classic smoothing family (SES, SESOptimized, Holt, HoltWinters, SeasonalES, SeasonalESOptimized, the closed-form
baselines, the default ETS chain) past the one-launch batch size, against the CPU oracle and a plain long-double restatement.

Comparison rule: tests/test_gpu_parity.py _compare / _rel -- forecast, lower and upper within REL_TOL = 1e-12 relative, model names
and error codes exact, "bit for bit" is np.array_equal.

Against the restatement (tests/classic_ref.py) the closed-form kernels get four times what the oracle achieves against it:
the oracle's worst case over the shared cases is 1.469e-14 (measured on the CPU by tests/test_classic_cpu.py, pinned there as
classic_ref.ORACLE_VS_LONGDOUBLE = 1.5e-14), so the kernels are allowed 6e-14.

The schedule a batch of n series lands on (csrc/host_api.hip run_classic; the constants are read from that function's text by
_schedule(), tests/test_classic_cpu.py pins their values):
  n <= TINY_BATCH_PROBLEMS (1,024)  one launch, one wave per problem
  else                              len(BUDGET) = 9 rounds: round 0 on four lanes per problem with BUDGET[0] = 24 passes (from 4 x 65,536
                                    series on: the sequential driver with 7/4 of it), rounds >= 1 behind compaction + column gather with the
                                    driver picked on the device from the live count (> spec_below = 8,192: sequential; <= spec2_below = 1,024:
                                    one wave per problem; else four lanes)
AnofoxHipStats.fit_kernel_launches counts one per round of every run_classic call of the run (HoltWinters makes two: its own fit and
Holt's for the series with fewer than two seasons), so it tells the one-launch schedule from the nine rounds; it does not tell which
driver a round picked.  That is argued from the constants: a batch of 3,000 has at most 3,000 <= 8,192 live problems after round 0
(four lanes, then one wave once <= 1,024 are left); of 12,000 series about 11,400 are fitted, and max_passes / total_passes show that
the fits outlive round 0's 24 passes (a problem that ended in round 0 reports at most 24 + 1 passes), so round 1 starts above 8,192.

The one-parameter members (SESOptimized, SeasonalESOptimized) on count-sized data never leave round 0: Nelder-Mead stops when the
simplex is within xatol = 1e-4 AND the values within the ABSOLUTE fatol = 1e-8 (csrc/nm.hpp), and in one dimension, from a simplex of
0.025, that takes 5 ... 20 iterations on synth.gen_series counts (sums of squares of order 1e2) -- measured max_passes 22 ... 24
(two start passes and the final one included) at every batch size, against the 26 that (d) asks for.  Sums of squares of order 1e8
make the value criterion the binding one: of 200 such series multiplied by 1,000, 92 % need more than 24 iterations (median 28) in a
plain restatement of that stopping rule on the CPU, and the kernels report max_passes 115 ... 138.  So these two models run every size
twice, on the counts as they are ((a) - (c)) and multiplied by 1,000 ((a) - (d): about 10,000 of 12,000 problems enter round 1, above
spec_below).  Holt and HoltWinters leave round 0 on the counts themselves: max_passes 85 ... 287 in the nine-round cases.
"""
import os
import re

import numpy as np
import pytest

import classic_ref as R
from test_gpu_parity import REL_TOL, _compare, _rel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_VS_LONGDOUBLE = 4 * R.ORACLE_VS_LONGDOUBLE
RUN_CLASSIC_CALLS = {"SESOptimized": 1, "Holt": 1, "SeasonalESOptimized": 1, "HoltWinters": 2}      # host_api.hip run_group, per model


@pytest.fixture(scope="module")
def env(hiplib, oracle):
    import torch
    assert torch.cuda.is_available()
    from anofox_forecast_amd import api, synth
    return api, oracle, hiplib, synth


def _schedule():
    """The constants of run_classic, from its text."""
    host = open(os.path.join(ROOT, "anofox-forecast_amd", "csrc", "host_api.hip")).read()
    body = host[host.index("void run_classic("):]
    body = body[:body.index("\n}\n")]
    g = lambda text, pat: re.search(pat, text).groups()
    a, b = g(body, r"seq0 = n >= (\d+)u \* (\d+)u;")
    below = g(body, r"f\.spec_below = (\d+); f\.spec2_below = (\d+);")
    return {"tiny": int(g(host, r"constexpr int TINY_BATCH_PROBLEMS = (\d+);")[0]),
            "budget": [int(x) for x in g(body, r"static const int BUDGET\[\] = \{([^}]*)\};")[0].split(",")],
            "spec_below": int(below[0]), "spec2_below": int(below[1]), "seq0": int(a) * int(b)}


def _expected_launches(model, n):
    sc = _schedule()
    return RUN_CLASSIC_CALLS[model] * (1 if n <= sc["tiny"] else len(sc["budget"]))


def _kw(m):
    return {"seasonal_period": m} if m else {"auto_detect": False}


def _batch_data(synth, n, m, start, scale=1.0):
    """n ragged series (multiplied by `scale`), half strictly positive and half counts with zeros: lengths in [2m, 2m + 40] (seasonal) or [40, 60], with a
    few empty, too short (2), shorter than one season / than two seasons, and constant series at strides that are no multiple of the
    wave, so that statuses differ inside a wave."""
    mm = m or 1
    T = 2 * mm + 40 if m else 60
    Y = np.empty((n, T))
    half = n // 2
    Y[:half] = synth.gen_series(synth.SEED_M5, start, half, T, max(mm, 2), positive=True)
    Y[half:] = synth.gen_series(synth.SEED_STRESS, start, n - half, T, max(mm, 2), positive=False)
    rng = np.random.default_rng(start + 7 * n + mm)
    lens = rng.integers(2 * mm, 2 * mm + 41, n) if m else rng.integers(40, 61, n)
    idx = np.arange(n)
    lens[idx % 97 == 5] = 0
    lens[idx % 89 == 7] = 2
    lens[idx % 83 == 11] = max(3, mm - 1)              # shorter than one season (a seasonal model), else just short
    lens[idx % 73 == 13] = max(3, 2 * mm - 1)          # one observation short of two seasons: Holt-Winters falls back to Holt
    Y *= scale
    Y[idx % 79 == 17] = 5.0
    Y[np.arange(T)[None, :] >= lens[:, None]] = 0.0
    return Y, lens.astype(np.int32)


def _device_run(lib, Y, lens, model, h, **kw):
    """One device-resident run: result arrays, the name of every series, the run statistics."""
    import torch
    from anofox_forecast_amd.device import DeviceBatch, pack_time_major
    n, T = Y.shape
    b = DeviceBatch(n, T, lib.make_options(model, h, **kw), "cuda:0")
    try:
        ln = np.zeros(b.ld, dtype=np.int32)
        ln[:n] = lens
        b.set_block(torch.from_numpy(pack_time_major(Y, b.ld)).to("cuda:0"), torch.from_numpy(ln).to("cuda:0"))
        b.run()
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy().copy() for k, v in b.results().items()}
        name_of = {int(c): b.model_name(int(c)) for c in np.unique(out["model_code"])}
        out["names"] = np.array([name_of[int(c)] for c in out["model_code"]])
        out["stats"] = b.stats()
    finally:
        b.close()
    return out


def _assert_oracle(O, out, Y, lens, model, h, pick=None, **kw):
    """(a): every series (or those of `pick`) equals the oracle -- codes and names exactly, figures within REL_TOL."""
    pick = np.arange(len(lens)) if pick is None else np.asarray(pick)
    T = Y.shape[1]
    sub, sl = Y[pick], lens[pick]
    concat = sub[np.arange(T)[None, :] < sl[:, None]]
    ref = O.forecast_batch(concat, np.concatenate([[0], np.cumsum(sl, dtype=np.int64)]), O.make_options(model, h, **kw))
    assert np.array_equal(out["status"][pick], ref["status"]), (model, kw, np.nonzero(out["status"][pick] != ref["status"])[0][:8])
    ok = ref["status"] == 0
    assert ok.any() and not ok.all()
    assert np.array_equal(out["names"][pick][ok], np.array(ref["names"])[ok]), (model, kw)
    worst = max(_rel(out[k][pick][ok], ref[k][ok]) for k in ("yhat", "lower", "upper"))
    assert worst <= REL_TOL, (model, kw, worst)
    return worst


def _assert_same_bits(a, b, what):
    for k in ("yhat", "lower", "upper", "model_code", "status"):
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def _chunked(lib, Y, lens, model, h, chunk, **kw):
    """The same series in batches of at most `chunk` (the one-launch schedule), put together again."""
    parts = [_device_run(lib, Y[a:a + chunk], lens[a:a + chunk], model, h, **kw) for a in range(0, len(lens), chunk)]
    assert all(p["stats"]["fit_kernel_launches"] == _expected_launches(model, min(chunk, len(lens))) for p in parts)
    return {k: np.concatenate([p[k] for p in parts]) for k in ("yhat", "lower", "upper", "model_code", "status")}


ONE_PARAMETER = ("SESOptimized", "SeasonalESOptimized")           # their fits leave round 0 only on data of larger magnitude (module docstring)
SCHEDULE_MODELS = ([("SESOptimized", 0, 1.0), ("SESOptimized", 0, 1000.0), ("Holt", 0, 1.0)] + [("HoltWinters", m, 1.0) for m in (7, 12, 70)]
                   + [("SeasonalESOptimized", m, sc) for m in (7, 12, 70) for sc in (1.0, 1000.0)])


@pytest.mark.parametrize("n", [1024, 1025, 3000, 12000])
@pytest.mark.parametrize("model,m,scale", SCHEDULE_MODELS)
def test_schedule_classes_match_oracle_and_the_one_launch_path(env, model, m, scale, n):
    """The optimised four over the batch sizes that change the schedule -- the last one-launch size, the first nine-round size, a
    batch whose later rounds start on four lanes per problem, one whose later rounds start on the sequential driver and thin through
    both thresholds -- and, for the seasonal two, the three ring classes: registers (m = 7), LDS (12), HBM scratch (70: its area is
    max((n + 15) / 16, min(n, 1,024)) x m x 64 doubles, the first term decides from n = 16,385 on, the second covers every launch here).
    (a) every series equals the oracle; (b) the same series in chunks of <= 1,024 give the same bits, names and codes; (c) the
    launch count is the one run_classic gives this size; (d) the fits outlive round 0's budget (the one-parameter models: on the
    data multiplied by 1,000 -- on counts their fits end inside round 0, see the module docstring)."""
    api, O, lib, synth = env
    sc = _schedule()
    assert sc["tiny"] == 1024 and sc["spec2_below"] < 3000 <= sc["spec_below"] < 0.9 * 12000
    h = 5
    Y, lens = _batch_data(synth, n, m, 1000 * (m + 1) + n, scale)
    out = _device_run(lib, Y, lens, model, h, **_kw(m))
    st = out["stats"]
    print(f"{model} m={m} x{scale:g} n={n}: fit_kernel_launches {st['fit_kernel_launches']}, max_passes {st['max_passes']}, "
          f"total_passes {st['total_passes']}, n ok {(out['status'] == 0).sum()}")
    worst = _assert_oracle(O, out, Y, lens, model, h, **_kw(m))                           # (a)
    if n > sc["tiny"]:
        _assert_same_bits(out, _chunked(lib, Y, lens, model, h, sc["tiny"], **_kw(m)), (model, m, n))   # (b)
    assert st["fit_kernel_launches"] == _expected_launches(model, n), (st, worst)         # (c)
    if n > sc["tiny"] and (scale > 1.0 or model not in ONE_PARAMETER):
        assert st["max_passes"] > sc["budget"][0] + 1, st                                 # (d): more than round 0's passes + the final one


@pytest.mark.parametrize("model,m", [("HoltWinters", 4), ("Holt", 0)])
def test_sequential_first_round(env, model, m):
    """262,144 series x 24 observations: from 4 x 65,536 series on, round 0 runs the sequential driver (one lane per problem) with 7/4
    of the budget.  Three 1,024-column slices (first, middle, last) equal the same columns run alone on the one-launch path bit for
    bit, and 300 sampled series equal the oracle."""
    api, O, lib, synth = env
    sc = _schedule()
    n, T, h = 262144, 24, 4
    assert n >= sc["seq0"] and n // 2 < sc["seq0"]
    rng = np.random.default_rng(262144 + m)
    t = np.arange(T)
    Y = (20.0 + rng.normal(0.0, 4.0, (n, 1)) + 0.2 * rng.normal(0.0, 1.0, (n, 1)) * t[None, :]
         + 3.0 * np.sin(2 * np.pi * (t[None, :] + rng.integers(0, 4, (n, 1))) / 4.0) + rng.normal(0.0, 1.0, (n, T)))
    lens = rng.integers(8, T + 1, n).astype(np.int32)
    idx = np.arange(n)
    lens[idx % 97 == 5] = 0
    lens[idx % 89 == 7] = 2
    lens[idx % 73 == 13] = 7                     # fewer than two seasons of 4
    Y[idx % 79 == 17] = 5.0
    Y[t[None, :] >= lens[:, None]] = 0.0
    out = _device_run(lib, Y, lens, model, h, **_kw(m))
    st = out["stats"]
    print(f"{model} m={m} n={n}: fit_kernel_launches {st['fit_kernel_launches']}, max_passes {st['max_passes']}, total_passes {st['total_passes']}")
    assert st["fit_kernel_launches"] == _expected_launches(model, n), st
    assert st["max_passes"] > (sc["budget"][0] * 7) // 4 + 1, st
    for a in (0, n // 2 - 512, n - 1024):
        alone = _device_run(lib, Y[a:a + 1024], lens[a:a + 1024], model, h, **_kw(m))
        assert alone["stats"]["fit_kernel_launches"] == _expected_launches(model, 1024)
        _assert_same_bits({k: out[k][a:a + 1024] for k in ("yhat", "lower", "upper", "model_code", "status")}, alone, (model, a))
    _assert_oracle(O, out, Y, lens, model, h, pick=np.sort(rng.choice(n, 300, replace=False)), **_kw(m))


@pytest.mark.parametrize("model,m", [("SESOptimized", 0), ("Holt", 0), ("HoltWinters", 12), ("SeasonalESOptimized", 12), ("HoltWinters", 70)])
def test_device_entry_and_host_entry_agree(env, model, m):
    """3,000 series through anofox_ts_forecast_batch (host buffers, packed and uploaded by the library) and through the device-resident
    batch: the same bits, names and codes."""
    api, O, lib, synth = env
    n, h = 3000, 5
    Y, lens = _batch_data(synth, n, m, 77000 + m, 1000.0 if model in ONE_PARAMETER else 1.0)
    dev = _device_run(lib, Y, lens, model, h, **_kw(m))
    got, berr = api.forecast_batch([Y[s, :lens[s]] for s in range(n)], lib.make_options(model, h, **_kw(m)))
    assert berr["ok"], berr
    for s in range(n):
        assert (got[s]["code"] if not got[s]["ok"] else 0) == dev["status"][s], (s, got[s], dev["status"][s])
        if got[s]["ok"]:
            assert got[s]["model_name"] == dev["names"][s]
            for k, dk in (("point", "yhat"), ("lower", "lower"), ("upper", "upper")):
                assert np.array_equal(got[s][k], dev[dk][s]), (model, s, k)


def test_fallback_chain_borrows_the_spec_lanes_gather_block(env):
    """The two ways the round path gets its gather block.  A fresh classic batch allocates its own (every nine-round case above).  A
    batch with ETS spec lanes lends the first lane's block to the family: AutoETS over 1,100 series (past the one-launch size) of
    which some 230 cannot be fitted by any spec -- constant series and series of three observations -- and go down the fallback chain
    HoltWinters / Holt / SES through run_classic's nine rounds on that borrowed block.  (A batch's model is fixed when it is created,
    so "AutoETS, then HoltWinters, on one handle" is this chain.)  Every series equals the oracle, names included."""
    api, O, lib, synth = env
    n, T, h, m = 1100, 44, 4, 7
    Y = synth.gen_series(synth.SEED_M5, 55000, n, T, m, positive=False)
    rng = np.random.default_rng(55)
    lens = rng.integers(30, T + 1, n).astype(np.int32)
    idx = np.arange(n)
    const = idx % 7 == 3
    Y[const] = np.round(rng.normal(9.0, 3.0, (int(const.sum()), 1)))
    lens[const] = rng.integers(3, T + 1, int(const.sum()))          # constant series either side of two seasons: HoltWinters, Holt or SES
    lens[idx % 31 == 4] = 3
    lens[idx % 97 == 5] = 0
    Y[np.arange(T)[None, :] >= lens[:, None]] = 0.0
    out = _device_run(lib, Y, lens, "AutoETS", h, seasonal_period=m)
    names = set(out["names"][out["status"] == 0])
    assert "AutoETS" in names and len(names) > 1, names                 # the chain's own name beside selected specs
    print(f"AutoETS n={n}: {int((out['names'] == 'AutoETS').sum())} series on the fallback chain, stats {out['stats']}")
    _assert_oracle(O, out, Y, lens, "AutoETS", h, seasonal_period=m)


def _boundary_series(synth, n, m, start):
    """n series with the lengths {m, m+1, 2m-1, 2m, 2m+1, 5m+3} in turn, positive and with zeros in turn."""
    T = 5 * m + 3
    Yp = synth.gen_series(synth.SEED_M5, start, n, T, m, positive=True)
    Yz = synth.gen_series(synth.SEED_STRESS, start, n, T, m, positive=False)
    L = (m, m + 1, 2 * m - 1, 2 * m, 2 * m + 1, 5 * m + 3)
    return [(Yp if (s // 6) % 2 else Yz)[s, : L[s % 6]] for s in range(n)]


@pytest.mark.parametrize("m", [2, 23, 24, 48, 49])
def test_one_launch_kernel_period_boundaries(env, m):
    """SeasonalES and SES stay on the one-launch classic_kernel: four candidate rings per lane in LDS up to CLASSIC_LDS_PERIOD = 48, in
    an HBM scratch from 49 on, and an opt-in to more than 48 KB of dynamic LDS in between.  SeasonalES asks for
    8 * nm_lds_doubles<1>() + 8 * NM_K * m * 64 = 2,048 + 2,048 m bytes (nm_lds_doubles<1>() = ((1+1)*1 + (1+1)) * 64 = 256 doubles):
    49,152 bytes = 48 KB exactly at m = 23 (no opt-in), 51,200 at m = 24 (opt-in).  65 and 127 series: the last wave is partial;
    lengths around one and two seasons; horizons below and above a season."""
    api, O, lib, synth = env
    for n in (65, 127):
        series = _boundary_series(synth, n, m, 31000 + 100 * m + n)
        for h in (1, m + 3):
            _compare(api, O, lib, series, "SeasonalES", h, seasonal_period=m)
            if m == 2:
                _compare(api, O, lib, series, "SES", h, auto_detect=False)


@pytest.mark.parametrize("m", [2, 24, 48, 49, 64, 65])
def test_round_kernel_ring_boundaries(env, m):
    """HoltWinters and SeasonalESOptimized on the round kernels (one launch at this size): the run-time LDS ring at its smallest (2) and
    largest (ETS_LDS_PERIOD = 64), the first HBM-ring period (65), and the periods around the one-launch kernel's own limit (48 / 49),
    which must mean nothing here.  65 and 127 series, lengths around one and two seasons, horizons below and above a season."""
    api, O, lib, synth = env
    for n in (65, 127):
        series = _boundary_series(synth, n, m, 41000 + 100 * m + n)
        for h in (1, m + 3):
            _compare(api, O, lib, series, "HoltWinters", h, seasonal_period=m)
            _compare(api, O, lib, series, "SeasonalESOptimized", h, seasonal_period=m)


@pytest.mark.parametrize("h", R.CASE_HORIZONS)
def test_closed_form_members_match_the_restatement(env, h):
    """Naive, SeasonalNaive (period 1, 7, n, n + 1), SMA (window 0 = default, 1, 5, n, n + 3), RandomWalkDrift and the toy ARIMA at
    lengths 1 ... 6 and beyond, SES and SeasonalES at their fixed constants: the kernels against the long-double restatement (error
    codes exactly, forecasts within four times the oracle's own distance from it) and, as everywhere, against the oracle."""
    api, O, lib, synth = env
    worst = 0.0
    for model, kw, series in R.closed_form_cases():
        got, berr = api.forecast_batch(series, lib.make_options(model, h, auto_detect=False, **kw))
        assert berr["ok"], (model, berr)
        for y, g in zip(series, got):
            code, p = R.point(model, y, h, period=max(kw.get("seasonal_period", 0), 1), window=kw.get("window", 0))
            assert (0 if g["ok"] else g["code"]) == code, (model, kw, len(y), g)
            if code == 0:
                worst = max(worst, R.rel(g["point"], p))
                lo, hi = R.intervals(g["point"], y, 0.90)
                assert R.rel(g["lower"], lo) <= KERNEL_VS_LONGDOUBLE and R.rel(g["upper"], hi) <= KERNEL_VS_LONGDOUBLE, (model, kw, len(y))
        _compare(api, O, lib, series, model, h, auto_detect=False, **kw)
    print(f"h={h}: kernels against the long-double restatement: worst {worst:.3e} (allowed {KERNEL_VS_LONGDOUBLE:.1e})")
    assert worst <= KERNEL_VS_LONGDOUBLE, worst


@pytest.mark.parametrize("model,kw", [("SES", {"auto_detect": False}), ("HoltWinters", {"seasonal_period": 7}), ("Naive", {"auto_detect": False}),
                                      ("ETS", {"seasonal_period": 7})])
def test_confidence_levels(env, model, kw):
    """confidence_level 0.5 / 0.8 / 0.99 / 0.999 for one model of each kernel, against the oracle and against properties the oracle
    cannot share a mistake in: the interval is symmetric about the point forecast, its half width over sqrt(step) is one number per
    series, and the widths of two levels are in the ratio of their z values -- forecast.rs:2570-2576: z = 2.576 from 0.99, 1.96 from
    0.95, 1.645 from 0.90, 1.28 from 0.80, else 1.0.  (The bounds are point -/+ width rounded to fp64, so the properties hold to
    REL_TOL on the scale max(1, |point|, width) of the rounded operands.)"""
    api, O, lib, synth = env
    z_of = lambda c: 2.576 if c >= 0.99 else 1.96 if c >= 0.95 else 1.645 if c >= 0.90 else 1.28 if c >= 0.80 else 1.0
    Y = synth.gen_series(synth.SEED_M5, 66000, 40, 70, 7, positive=True)
    series = [Y[s, : 70 - (s % 6) * 4] for s in range(40)]
    h = 6
    half = {}
    for conf in (0.5, 0.8, 0.99, 0.999):
        _compare(api, O, lib, series, model, h, confidence_level=conf, **kw)
        got, berr = api.forecast_batch(series, lib.make_options(model, h, confidence_level=conf, **kw))
        assert berr["ok"] and all(g["ok"] for g in got)
        p, lo, hi = (np.array([g[k] for g in got]) for k in ("point", "lower", "upper"))
        scale = np.maximum(1.0, np.maximum(np.abs(p), hi - p))
        assert np.all(hi - p >= 0.0) and np.mean(hi - p > 0.0) > 0.8                        # (a constant series has no width)
        assert np.max(np.abs((hi - p) - (p - lo)) / scale) <= REL_TOL, conf
        unit = (hi - p) / np.sqrt(np.arange(1, h + 1))[None, :]
        assert np.max(np.abs(unit - unit[:, :1]) / scale) <= REL_TOL, conf
        half[conf] = hi - p
    for c1, c2 in ((0.5, 0.8), (0.8, 0.99), (0.99, 0.999), (0.5, 0.999)):
        scale = np.maximum(1.0, np.maximum(np.abs(p), half[c2]))
        assert np.max(np.abs(half[c2] * z_of(c1) - half[c1] * z_of(c2)) / (z_of(c1) * scale)) <= REL_TOL, (c1, c2)
    assert z_of(0.5) == 1.0 and z_of(0.999) == z_of(0.99) == 2.576 and z_of(0.8) == 1.28


FAMILY = [("Naive", {"auto_detect": False}), ("SeasonalNaive", {"seasonal_period": 7}), ("SMA", {"auto_detect": False}),
          ("RandomWalkDrift", {"auto_detect": False}), ("ARIMA", {"auto_detect": False}), ("SES", {"auto_detect": False}),
          ("SESOptimized", {"auto_detect": False}), ("Holt", {"auto_detect": False}), ("HoltWinters", {"seasonal_period": 7}),
          ("SeasonalES", {"seasonal_period": 7}), ("SeasonalESOptimized", {"seasonal_period": 7}), ("ETS", {"seasonal_period": 7})]


@pytest.mark.parametrize("model,kw", FAMILY)
def test_fitted_values_residuals_and_mse(env, model, kw):
    """include_fitted / include_residuals for every model of the family: fitted values, residuals and mse against the oracle's (the
    reference derives them from the model TYPE, forecast.rs:2593-2643: Naive and SeasonalNaive by their own rule, every other member by
    SES at 0.3; tests/test_classic_cpu.py holds the oracle's to the restatement of that rule)."""
    api, O, lib, synth = env
    Y = synth.gen_series(synth.SEED_M5, 67000, 30, 64, 7, positive=True)
    series = [Y[s, : 64 - (s % 7) * 8] for s in range(30)] + [np.array([3.0, 1.0, 2.0]), np.full(9, 4.0)]
    for flags in ({"include_fitted": True, "include_residuals": True}, {"include_fitted": True}, {"include_residuals": True}):
        got, berr = api.forecast_batch(series, lib.make_options(model, 3, **flags, **kw))
        assert berr["ok"], berr
        oo = O.make_options(model, 3, **flags, **kw)
        for s, y in enumerate(series):
            ref = O.forecast(y, oo)
            assert got[s]["ok"] == ref["ok"], (model, s, got[s], ref)
            if not ref["ok"]:
                assert got[s]["code"] == ref["code"]
                continue
            for k in ("fitted", "residuals"):
                assert (k in got[s]) == (k in ref) == bool(flags.get("include_" + k)), (model, s, k)
                if k in ref:
                    assert len(got[s][k]) == len(y) and _rel(got[s][k], ref[k]) <= REL_TOL, (model, s, k)
            assert _rel(np.array([got[s]["mse"]]), np.array([ref["mse"]])) <= REL_TOL, (model, s)
