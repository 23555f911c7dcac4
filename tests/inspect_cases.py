"""Input families of the fit-state readback tests, shared by tests/test_inspect_cpu.py (the oracle's record meets the identities of
inspect_ref.py) and tests/test_gpu_inspect.py (the kernels' record equals the oracle's and meets them too).  Shapes are the smallest
that still reach each branch of the readback: every residue of the length modulo the period, lengths that end inside a streamed
block, one full wave plus a partial one, every ring class."""
from __future__ import annotations

import ctypes as C

import numpy as np

import inspect_ref as R
from anofox_forecast_amd import synth

RING_SPECS = ("AAA", "MAdM", "AMdA", "MNM")
RING_PERIODS = (12, 5, 24, 64, 65, 70)       # compile-time ring; LDS ring smallest .. largest; HBM ring and its prefetch loop
EXPLAIN_SPECS = ("AAdA", "MAM", "AMdM")
TUNES = ("seq_rounds=0;gather=1", "seq_rounds=6;gather=0", "spec2_below=100000", "k4=1", "compact=1", "compact=2")


def every_spec(notation):
    """70 strictly positive series (one full wave plus a wave of 6), lengths 97 - (s % 11): every residue modulo 7, ends inside
    streamed blocks.  Returns (series, period, horizon): period 7 for a seasonal spec, 1 otherwise; h = 2 m + 3 wraps the phases twice."""
    m = 7 if notation[-1] != "N" else 1
    Y = synth.gen_series(synth.SEED_M5, 8100, 70, 97, 7, positive=True)
    return [Y[s, : 97 - (s % 11)] for s in range(70)], m, 2 * m + 3


def ring_class(m):
    """24 strictly positive series of T = 5 m + 37 with lengths T - 3 (s % 7), then one series of 2 m - 1 and one of exactly 2 m
    observations (the END of the first two generated series that move there: a constant run -- the head before the first sale, a
    product that never sells -- is fitted with SSE = 0, and the criteria are then the -1e10 floor of the likelihood, not a
    logarithm).  Returns (series, horizon)."""
    T = 5 * m + 37
    Y = synth.gen_series(synth.SEED_M5, 8200 + m, 24, T, m, positive=True)
    a, b = [s for s in range(24) if np.ptp(Y[s, T - 2 * m + 1:]) > 0][:2]
    return [Y[s, : T - 3 * (s % 7)] for s in range(24)] + [Y[a, T - (2 * m - 1):], Y[b, T - 2 * m:]], m + 3


def auto_mixed():
    """130 ragged series, strictly positive and raw counts interleaved (multiplicative specs run on the gathered positive list; a
    series of zeros and counts leaves them nothing to fit), then a constant series, an all-zero one, arange(5), a two-point one, an
    empty one, and 10 series with NULLs.  Returns (series, valids, kind) with kind[s] in {"positive", "counts", "edge", "nulls"}."""
    Yp = synth.gen_series(synth.SEED_M5, 8400, 65, 120, 7, positive=True)
    Yi = synth.gen_series(synth.SEED_M5, 8500, 75, 120, 7)
    series, kind = [], []
    for s in range(130):
        n = 120 - (s % 13) * 5 - (s % 3)
        series.append((Yp if s % 2 == 0 else Yi)[s // 2, :n].copy())
        kind.append("positive" if s % 2 == 0 else "counts")
    series += [np.full(30, 42.0), np.zeros(40), np.arange(5.0), np.array([1.0, 2.0]), np.array([])]
    kind += ["edge"] * 5
    valids = [np.ones(len(y), bool) for y in series]
    rng = np.random.default_rng(8600)
    for s in range(10):
        n = 60 + 5 * s
        y = (Yp[55 + s, :n] if s % 2 == 0 else Yi[65 + s, :n]).copy()
        v = np.ones(n, bool)
        v[rng.integers(0, n, size=1 + n // 12)] = False
        if s == 3:
            v[0] = False
        if s == 6:
            v[-1] = False
        series.append(y)
        valids.append(v)
        kind.append("nulls")
    return series, valids, kind


def tune_subset(tune, kind):
    """Indices of auto_mixed() a tune setting runs on: k4 the raw counts (the automatic choice of that driver), compact storage the
    count-valued series (an interpolated NULL is not a count), every other setting the whole batch."""
    if tune.startswith("k4"):
        return [s for s, k in enumerate(kind) if k == "counts"]
    if tune.startswith("compact"):
        return [s for s, k in enumerate(kind) if k in ("positive", "counts")]
    return list(range(len(kind)))


def arima(m):
    """Ragged M5-shape series for AutoARIMA: 40 at m = 7, 16 without a period."""
    n = 40 if m > 1 else 16
    Y = synth.gen_series(synth.SEED_M5, 8700 + m, n, 150, 7)
    return [Y[s, : 150 - (s % 9) * 6] for s in range(n)]


def explain_groups(m):
    """7 groups of lengths 85..91 (every residue modulo 7 and modulo 5), one NULL target each.  Returns (group, date, target) columns,
    shuffled."""
    Y = synth.gen_series(synth.SEED_M5, 8900 + m, 7, 91, m, positive=True)
    grp, ds, tgt = [], [], []
    for g in range(7):
        n = 85 + g
        for t in range(n):
            grp.append(f"g{g}")
            ds.append(t)
            tgt.append(None if t == 11 + 9 * g else float(Y[g, t]))
    perm = np.random.default_rng(8901).permutation(len(grp))
    return (np.array(grp, dtype=object)[perm], np.array(ds)[perm], np.array(tgt, dtype=object)[perm])


def clean(O, y, valid):
    """The series the models see: NULL slots interpolated the way the forecast path does it."""
    y = np.ascontiguousarray(y, dtype=np.float64)
    if valid is None or len(y) == 0 or bool(np.all(valid)):
        return y
    out = np.zeros(len(y))
    mask = O.validity_mask(valid)
    O.lib().oracle_fill_nulls_interpolate(y.ctypes.data, mask.ctypes.data, C.c_size_t(len(y)), out.ctypes.data)
    return out


class ArimaOrder(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("p", "d", "q", "P", "D", "Q", "s", "with_constant")]


class ArimaFit(C.Structure):
    _fields_ = [("ord", ArimaOrder), ("x", C.c_double * 6), ("css", C.c_double), ("sigma2", C.c_double), ("aicc", C.c_double),
                ("n_used", C.c_int), ("evals", C.c_int), ("iters", C.c_int)]


def arima_detail(O, y, period, h):
    """oracle_auto_arima_detail (oracle/arima.h): the selected fit and its forecasts, or None when nothing can be fitted."""
    L = O.lib()
    L.oracle_auto_arima_detail.restype = C.c_int
    L.oracle_auto_arima_detail.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(ArimaFit), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    y = np.ascontiguousarray(y, dtype=np.float64)
    fit, out, tried, evals = ArimaFit(), np.zeros(max(h, 1)), C.c_int(), C.c_int()
    if not L.oracle_auto_arima_detail(y.ctypes.data, len(y), int(period), int(h), out.ctypes.data, C.byref(fit), C.byref(tried), C.byref(evals)):
        return None
    return fit, out[:h]


_REFS = {}


def _frozen(d):
    if d is not None:
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return d


def oracle_record(O, key, y, period, sid=-1):
    """O.ets_inspect, computed once per (case, series) of a session and handed out unchanged."""
    key = ("record",) + tuple(key)
    if key not in _REFS:
        _REFS[key] = _frozen(O.ets_inspect(y, period, spec_id=sid) if len(y) >= 3 else None)
    return _REFS[key]


def oracle_forecast(O, key, y, valid, model, h, **kw):
    """O.forecast of the same series and options, computed once per (case, series) of a session."""
    key = ("forecast",) + tuple(key)
    if key not in _REFS:
        _REFS[key] = _frozen(O.forecast(y, O.make_options(model, h, **kw), valid))
    return _REFS[key]


REL_TOL = 1e-12                      # the suite's parity tolerance (tests/test_gpu_parity.py)


def check_identities(rec, y, notation, m, point, worst, where):
    """Component rule, parameter regions and the three identities of inspect_ref.py on one record, asserted at REL_TOL; `worst`
    collects the largest deviation of each identity for the test's report."""
    assert R.component_rule(rec, notation, m) == [], (where, notation, R.component_rule(rec, notation, m))
    assert R.parameter_rule(rec, notation) == [], (where, notation, R.parameter_rule(rec, notation))
    for k, d in R.identities(rec, y, notation, m, point).items():
        worst[k] = max(worst.get(k, 0.0), d)
        assert d <= REL_TOL, (where, notation, k, d)
