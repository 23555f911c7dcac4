"""The oracle's ETS records against the restatement of tests/ets_ref.py, without a GPU: on every case of tests/ets_cases.py the
start states of oracle/ets.c (ets_init_states) and the fitted values, final level, trend, all m seasonal states and point forecasts of
its records equal the textbook recursion, run in 80-bit arithmetic from the classical-decomposition / least-squares start at the
record's own parameters, within max(1e-12, F x the series' own float64-to-80-bit noise).  oracle/ets.c is "the same operations in the
same order" as the kernels and was rewritten together with them; this file is the witness that does not share their operation order.
It also fixes what tests/test_gpu_ets_replay.py inherits: the factor F, the share of quiet series in every fitted family, the
distance of every series from every start-state clamp, and which step of the damped growth rate takes which power.

What this file sees, tried on scratch copies of oracle/ets.c: full instead of half end weights in the even-period moving average,
gamma e / q taken with 1 / s in the additive-error multiplicative-season branch and K = 2 m in place of max(10, 2 m) each fail it
(13, 7 and 9 tests).  It does NOT see the binomial series of b^phi one degree short: by the series' own bound that moves a step by
|C(phi, 11)| 16^-11 < 5e-16, two units in the last place, far below the 1e-12 floor every comparison of this suite stands on.
"""
import numpy as np
import pytest

import ets_cases as X
import ets_ref as E
import inspect_cases as K
import inspect_ref as R

RATIOS = {}                      # (case, series) -> (oracle deviation, noise): what F is measured on


def _compare(O, key, series, notation, m, h, recs, points, clamp=None):
    """Records of one batch against the restatement.  Returns (worst deviation / tolerance, its deviation, its tolerance, noises)."""
    reps = X.replays(key, series, notation, m, h, recs)
    worst, noises = (0.0, 0.0, X.REL_TOL), []
    for s, (y, rec, rep) in enumerate(zip(series, recs, reps)):
        if rec is None:
            continue
        where = key + (s,)
        X.check_clamps(rep["clamps"], clamp, where)
        # the start states of oracle/ets.c themselves, at the tolerance their own conditioning gives
        got = dict(zip(("level", "growth", "seasonal"), X.oracle_start(O, y, notation, m)))
        s64, s80 = rep["start64"], rep["start80"]
        keys = [k for k in got if s80[k] is not None]
        start_noise = max(R.dev(s64[k], s80[k]) for k in keys)
        d0 = max(R.dev(got[k], s80[k]) for k in keys)
        assert d0 <= max(X.REL_TOL, X.F * start_noise), (where, notation, "start states", d0, start_noise)
        d = E.deviation(X.record_quantities(rec, points[s], notation), rep["q80"])
        RATIOS[where] = (d, rep["noise"])
        noises.append(rep["noise"])
        if d / rep["tol"] >= worst[0]:
            worst = (d / rep["tol"], d, rep["tol"])
        assert d <= rep["tol"], (where, notation, d, rep["tol"], rep["noise"],
                                 {k: R.dev(X.record_quantities(rec, points[s], notation)[k], rep["q80"][k]) for k in rep["q80"]})
    return worst, noises


def _conditioning(noises, where):
    """The two conditions on a fitted family: three quarters of its series are quiet (held at the 1e-12 floor), none is wild."""
    quiet = sum(1 for v in noises if v <= X.QUIET_NOISE)
    assert 4 * quiet >= 3 * len(noises), (where, quiet, len(noises))
    assert max(noises) <= X.WORST_NOISE, (where, max(noises))
    return quiet


def _every_spec(O, spec):
    series, m, h = K.every_spec(spec)
    recs = [K.oracle_record(O, ("spec", spec, s), y, m, R.spec_id(spec)) for s, y in enumerate(series)]
    fcs = [K.oracle_forecast(O, ("spec", spec, s), y, None, "ETS", h, ets_model=spec, seasonal_period=m) for s, y in enumerate(series)]
    assert all(r is not None and f["ok"] for r, f in zip(recs, fcs)), spec
    return _compare(O, ("spec", spec), series, spec, m, h, recs, [f["point"] for f in fcs])


@pytest.mark.parametrize("spec", R.SPECS)
def test_every_spec_oracle_record_is_the_recursion(oracle, spec):
    worst, noises = _every_spec(oracle, spec)
    quiet = _conditioning(noises, spec)
    print(f"{spec}: worst deviation {worst[1]:.2e} at tolerance {worst[2]:.2e}; {quiet} of {len(noises)} series quiet, worst noise {max(noises):.2e}")


def _ring(O, period, spec):
    series, h = K.ring_class(period)
    recs = [K.oracle_record(O, ("ring", period, spec, s), y, period, R.spec_id(spec)) for s, y in enumerate(series)]
    fcs = [K.oracle_forecast(O, ("ring", period, spec, s), y, None, "ETS", h, ets_model=spec, seasonal_period=period) for s, y in enumerate(series)]
    assert all((r is not None) == f["ok"] for r, f in zip(recs, fcs)), (period, spec)
    assert recs[24] is None and sum(r is not None for r in recs) >= 21, (period, spec)          # one season short: no record
    return _compare(O, ("ring", period, spec), series, spec, period, h, recs, [f.get("point") for f in fcs])


@pytest.mark.parametrize("period", K.RING_PERIODS)
def test_ring_class_oracle_record_is_the_recursion(oracle, period):
    for spec in K.RING_SPECS:
        worst, noises = _ring(oracle, period, spec)
        quiet = _conditioning(noises, (period, spec))
        print(f"m = {period} {spec}: worst deviation {worst[1]:.2e} at tolerance {worst[2]:.2e}; {quiet} of {len(noises)} series quiet, "
              f"worst noise {max(noises):.2e}")


def _fixed(O, name):
    case = X.fixed_cases()[name]
    series, m, h = case["series"], case["m"], case["h"]
    offs = np.concatenate([[0], np.cumsum([len(y) for y in series])])
    vals = np.concatenate(series)
    out = []
    for r, (spec, params) in enumerate(case["runs"]):
        recs = [X.oracle_fixed_record(O, y, spec, m, params) for y in series]
        fb = O.ets_fixed_batch(vals, offs, spec, m, *params, h)
        for s, (y, rec) in enumerate(zip(series, recs)):
            assert (fb["status"][s] == 0) == (rec is not None), (name, spec, s, fb["status"][s])
            if rec is None:
                continue
            e, t, sn = R.parts(spec)
            want = (params[0], params[1] if t != "N" else None, params[2] if sn != "N" else None, params[3] if t in ("Ad", "Md") else None)
            for k, v in zip(("alpha", "beta", "gamma", "phi"), want):           # the given parameters, in model terms, exactly
                assert (np.isnan(rec[k]) if v is None else rec[k] == v), (name, spec, s, k, rec[k], v)
            lo, hi = E.intervals(fb["yhat"][s], y, 0.90, E.LD)
            assert max(R.dev(fb["lower"][s], lo), R.dev(fb["upper"][s], hi)) <= X.REL_TOL, (name, spec, s)
        worst, noises = _compare(O, ("fixed", name, r), series, spec, m, h, recs, fb["yhat"], case["clamp"])
        out.append((spec, params, worst, noises, X.replays(("fixed", name, r), series, spec, m, h, recs)))
    return case, out


@pytest.mark.parametrize("name", sorted(X.fixed_cases()))
def test_fixed_parameter_oracle_record_is_the_recursion(oracle, name):
    case, runs = _fixed(oracle, name)
    fitted = 0
    for spec, params, worst, noises, reps in runs:
        fitted += len(noises)
        if noises:
            assert max(noises) <= X.WORST_NOISE, (name, spec, max(noises))
            print(f"{name} {spec} alpha {params[0]:.3g} phi {params[3]:.3g}: worst deviation {worst[1]:.2e} at tolerance {worst[2]:.2e}, "
                  f"worst noise {max(noises):.2e}")
    assert fitted >= len(runs), (name, fitted)                     # (series too short for a spec are there on purpose; not all of them)
    if name == "corner-MMdM":
        # both powers of the damped growth rate: a run whose every step stays inside |b - 1| <= 1/16 (the binomial series) and a run
        # with a step outside it (the table-driven power), neither within a millionth of the threshold
        far = [max(rep["far"] for rep in reps if rep is not None) for _, _, _, _, reps in runs]
        assert min(far) < X.POW_NEAR1_R * (1.0 - 1.0e-6) and max(far) > X.POW_NEAR1_R * (1.0 + 1.0e-6), far
        print(f"{name}: largest |b - 1| per run " + ", ".join(f"{v:.3g}" for v in far))


def _auto(O):
    series, h = X.auto_case()
    recs = [K.oracle_record(O, ("ets-auto", s), y, 7) for s, y in enumerate(series)]
    fcs = [K.oracle_forecast(O, ("ets-auto", s), y, None, "AutoETS", h, seasonal_period=7) for s, y in enumerate(series)]
    by_spec = {}
    for s, (rec, fc) in enumerate(zip(recs, fcs)):
        spec = R.notation_of_name(fc["model_name"]) if fc["ok"] else None
        assert (rec is not None) == (spec is not None), (s, fc)
        if spec is not None:
            assert R.notation_of(rec["spec_id"]) == spec, (s, spec)
            by_spec.setdefault(spec, []).append(s)
    return series, h, recs, fcs, by_spec


def test_autoets_oracle_record_is_the_recursion(oracle):
    O = oracle
    series, h, recs, fcs, by_spec = _auto(O)
    assert all(np.any(y[:21] == 0.0) for y in series[:64]) and sum(1 for y in series[64:] if np.all(y > 0.0)) == 3
    noises = []
    for spec, idx in sorted(by_spec.items()):
        sub = [series[s] for s in idx]
        worst, nz = _compare(O, ("auto", spec), sub, spec, 7, h, [recs[s] for s in idx], [fcs[s]["point"] for s in idx])
        noises += nz
        print(f"AutoETS {spec} ({len(idx)} series): worst deviation {worst[1]:.2e} at tolerance {worst[2]:.2e}, worst noise {max(nz):.2e}")
    assert len(noises) >= 60, len(noises)
    _conditioning(noises, "AutoETS")


@pytest.mark.parametrize("conf", X.CONFIDENCES + (0.5,))
def test_intervals_follow_the_table(oracle, conf):
    """lower / upper of the oracle's forecast path are point -/+ z sd sqrt(i) with the population sd and the five-step z."""
    O = oracle
    series, m, h = K.every_spec("AAA")
    worst = 0.0
    for y in series[:6]:
        fc = O.forecast(y, O.make_options("ETS", h, ets_model="AAA", seasonal_period=m, confidence_level=conf))
        lo, hi = E.intervals(fc["point"], y, conf, E.LD)
        worst = max(worst, R.dev(fc["lower"], lo), R.dev(fc["upper"], hi))
    print(f"confidence {conf}: worst interval deviation {worst:.2e}")
    assert worst <= X.REL_TOL, (conf, worst)


def test_the_factor_covers_every_case(oracle):
    """F of ets_cases.py is four times the largest ratio (oracle deviation from the 80-bit replay) / (the replay's own noise) over every
    series of every case whose noise exceeds 1e-15 -- recomputed here from all of them, so a new case cannot slip under a stale F."""
    O = oracle
    for spec in R.SPECS:
        _every_spec(O, spec)
    for period in K.RING_PERIODS:
        for spec in K.RING_SPECS:
            _ring(O, period, spec)
    for name in X.fixed_cases():
        _fixed(O, name)
    series, h, recs, fcs, by_spec = _auto(O)
    for spec, idx in by_spec.items():
        _compare(O, ("auto", spec), [series[s] for s in idx], spec, 7, h, [recs[s] for s in idx], [fcs[s]["point"] for s in idx])
    noisy = {k: d / nz for k, (d, nz) in RATIOS.items() if nz > 1.0e-15}
    top = max(noisy, key=noisy.get)
    print(f"{len(RATIOS)} series, {len(noisy)} with noise above 1e-15; largest ratio {noisy[top]:.3f} at {top} "
          f"(deviation {RATIOS[top][0]:.2e}, noise {RATIOS[top][1]:.2e}); F = {X.F}")
    assert 0.5 * X.MEASURED_RATIO <= noisy[top] <= 1.02 * X.MEASURED_RATIO, (noisy[top], X.MEASURED_RATIO)
