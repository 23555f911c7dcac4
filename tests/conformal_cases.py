"""Cases shared by tests/test_conformal_cpu.py and tests/test_gpu_conformal.py: the golden statements, the ragged shape batches of
the bit-equality tests, the content cases, and what the restatement (tests/conformal_ref.py) expects of a learn call."""
import functools
import json
import math
import os
import random
import struct

import conformal_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
# every tile boundary of the sorting network (64 .. 2,048 keys), the LDS limit, and the global-workspace path above it
SIZES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 2047, 2048, 2049, 4097)
# the same with the largest group at 140 rows (a 5-fold x 28-step backtest): the 256-key tile, 16 waves per workgroup
SMALL_SIZES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 140)
N_GROUPS = 130                       # neighbouring waves hold different tiles' worth of live keys; the last workgroup is partial
ALPHAS = (0.0, 0.05, 0.1, 0.5, 0.999999)
ALPHAS16 = tuple(round(0.01 + 0.06 * k, 2) for k in range(16))
OK, EMPTY, NAN, DIFFICULTY = 0, 1, 2, 3


def load_kats():
    return json.load(open(os.path.join(HERE, "golden", "conformal_kats.json")))


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def same_bits(got, want):
    """Equality of bits; NaN by NaN-ness (payloads are exempt)."""
    if want != want:
        return got != got
    return got == got and bits(float(got)) == bits(float(want))


def residuals(rng, n):
    """n residuals of both signs with ties (one decimal), a few exact zeros and some values that are not round."""
    out = []
    for _ in range(n):
        u = rng.random()
        if u < 0.05:
            out.append(0.0)
        elif u < 0.7:
            out.append(round(rng.gauss(0.0, 3.0), 1))
        else:
            out.append(rng.gauss(0.5, 40.0))
    return out


@functools.lru_cache(maxsize=None)
def shape_batch(small=False):
    """130 ragged groups whose sizes walk SIZES (or SMALL_SIZES) in order."""
    sizes = SMALL_SIZES if small else SIZES
    rng = random.Random(20240611 + int(small))
    return tuple(tuple(residuals(rng, sizes[i % len(sizes)])) for i in range(N_GROUPS))


def content_groups():
    """(name, residuals) of the content cases; none holds a NaN."""
    inf = math.inf
    return [
        ("all_positive", [0.5, 1.25, 3.0, 0.1, 7.5, 2.0, 2.0]),
        ("all_negative", [-0.5, -1.25, -3.0, -0.1, -7.5, -2.0, -2.0]),
        ("all_zero", [0.0] * 9),
        ("minus_zero", [-0.0, 0.0, -0.0, 1.0, -1.0]),
        ("only_minus_zero", [-0.0, -0.0, -0.0]),
        ("heavy_ties", [1.0, -1.0] * 40 + [2.0] * 3 + [-2.0] * 70),
        ("plus_inf", [1.0, inf, -2.0, 3.0]),
        ("minus_inf", [1.0, -inf, -2.0, 3.0]),
        ("both_inf", [inf, -inf, 0.5]),
        ("single", [-4.25]),
        ("single_zero", [0.0]),
        ("tiny", [5e-324, -5e-324, 1e-300, -1e308, 1e308]),
    ]


def expect_learn(res, alphas, method, valid=None):
    """(status, sorted |r| or None, scores_lower, scores_upper, n_kept) of one group as the learn kernel reports it: the restatement's
    conformal_learn on the rows kept, NaN scores for an empty group and for one with a NaN residual."""
    kept = [r for i, r in enumerate(res) if valid is None or valid[i]]
    nan = [math.nan] * len(alphas)
    if not kept:
        return EMPTY, None, nan, nan, 0
    if R.has_nan(kept):
        return NAN, None, nan, nan, len(kept)
    p, e = R.conformal_learn(kept, list(alphas), method, "split", [1.0] * len(kept) if method == "adaptive" else None)
    assert e is None, e
    return OK, R.sorted_abs(kept), p["scores_lower"], p["scores_upper"], len(kept)


def check(value, op, *args):
    if op == "abs_diff_lt":
        return abs(value - args[0]) < args[1]
    if op == "eq":
        return value == args[0]
    if op == "gt":
        return value > args[0]
    if op == "lt":
        return value < args[0]
    if op == "ge":
        return value >= args[0]
    if op == "le":
        return value <= args[0]
    raise KeyError(op)


class RefScalars:
    """The SQL-level functions of api.py answered by the restatement: None where the source answers NULL (a NULL or empty list,
    lists of different lengths, every failure of the call)."""

    @staticmethod
    def _vals(x):
        return None if x is None else [float(v) for v in x if v is not None]

    def ts_conformal_quantile(self, residuals, alpha):
        r = self._vals(residuals)
        if not r or alpha is None:
            return None
        return R.conformal_quantile(r, alpha)[0]

    def ts_conformal_intervals(self, forecasts, score):
        f = self._vals(forecasts)
        if not f or score is None:
            return None
        lo, up = R.conformal_intervals(f, score)
        return {"lower": lo, "upper": up}

    def ts_conformal_predict(self, residuals, forecasts, alpha):
        r, f = self._vals(residuals), self._vals(forecasts)
        if not r or not f or alpha is None:
            return None
        return R.conformal_predict(r, f, alpha)[0]

    def ts_conformal_predict_asymmetric(self, residuals, forecasts, alpha):
        r, f = self._vals(residuals), self._vals(forecasts)
        if not r or not f or alpha is None:
            return None
        return R.conformal_predict_asymmetric(r, f, alpha)[0]

    def ts_conformal_learn(self, residuals, alphas, method="symmetric", strategy="split"):
        r, a = self._vals(residuals), self._vals(alphas)
        if not r or not a:
            return None
        p = R.conformal_learn(r, a, method, {"jackknife_plus": "jackknife+"}.get(strategy, strategy), None)[0]
        if p is not None and p["strategy"] == "jackknife+":
            p["strategy"] = "jackknife_plus"                 # StrategyToString
        return p

    def ts_conformal_apply(self, forecasts, profile):
        f = self._vals(forecasts)
        if not f or profile is None:
            return None
        p = dict(profile, strategy={"jackknife_plus": "jackknife+"}.get(profile["strategy"], profile["strategy"]))
        return R.conformal_apply(f, p, None)[0]

    def ts_conformal_coverage(self, actuals, lower, upper):
        a, l, u = self._vals(actuals), self._vals(lower), self._vals(upper)
        if not a or len(a) != len(l) or len(a) != len(u):
            return None
        return R.conformal_coverage(a, l, u)[0]

    def ts_conformal_evaluate(self, actuals, lower, upper, alpha):
        a, l, u = self._vals(actuals), self._vals(lower), self._vals(upper)
        if not a or len(a) != len(l) or len(a) != len(u) or alpha is None:
            return None
        return R.conformal_evaluate(a, l, u, alpha)[0]

    def ts_mean_interval_width(self, lower, upper):
        l, u = self._vals(lower), self._vals(upper)
        if not l or len(l) != len(u):
            return None
        return R.mean_interval_width(l, u)

    # the table macros (ts_macros.cpp:1446-1584), quirks included
    @staticmethod
    def _groups(keys, keep):
        order, members = [], {}
        for i, k in enumerate(keys):
            if not keep[i]:
                continue
            if k not in members:
                members[k] = []
                order.append(k)
            members[k].append(i)
        return order, members

    def ts_conformal_by(self, group_columns, actual, forecast, point_forecast, params=None):
        (name, keys), = group_columns.items()
        alpha = float((params or {}).get("alpha", 0.1))
        asym = (params or {}).get("method", "symmetric") == "asymmetric"
        r_order, r_mem = self._groups(keys, [a is not None and f is not None for a, f in zip(actual, forecast)])
        _, p_mem = self._groups(keys, [p is not None for p in point_forecast])
        order = [g for g in r_order if g in p_mem]
        out = {name: order}
        rows = []
        for g in order:
            res = [actual[i] - forecast[i] for i in r_mem[g]]
            pts = sorted(point_forecast[i] for i in p_mem[g])
            rows.append((self.ts_conformal_predict_asymmetric if asym else self.ts_conformal_predict)(res, pts, alpha))
        for c in ("point", "lower", "upper", "coverage", "conformity_score", "method"):
            out[c] = [None if r is None else r[c] for r in rows]
        return out

    def ts_conformal_calibrate(self, actual, forecast, params=None):
        alpha = float((params or {}).get("alpha", 0.1))
        res = [a - f for a, f in zip(actual, forecast) if a is not None and f is not None]
        return {"conformity_score": self.ts_conformal_quantile(res, alpha), "coverage": 1.0 - alpha, "n_residuals": len(res)}

    def ts_conformal_apply_by(self, group_columns, forecast, score):
        (name, keys), = group_columns.items()
        order, mem = self._groups(keys, [f is not None for f in forecast])
        rows = [self.ts_conformal_intervals(sorted(forecast[i] for i in mem[g]), score) for g in order]
        return {name: order, "lower": [None if r is None else r["lower"] for r in rows], "upper": [None if r is None else r["upper"] for r in rows]}

    def ts_interval_width_by(self, group_columns, lower, upper):
        (name, keys), = group_columns.items()
        order, mem = self._groups(keys, [l is not None and u is not None for l, u in zip(lower, upper)])
        return {name: order,
                "mean_width": [self.ts_mean_interval_width(sorted(lower[i] for i in mem[g]), sorted(upper[i] for i in mem[g])) for g in order],
                "n_intervals": [len(mem[g]) for g in order]}


def _field(value, field):
    if field is None or value is None:
        return value
    if field in ("n_levels",):
        return len(value["alphas"])
    if field in ("n_forecasts",):
        return len(value["point"])
    if field.endswith("]"):
        name, idx = field[:-1].split("[")
        return value[name][int(idx)]
    return value[field]


def _holds(value, chk):
    op, args = chk[0], chk[1:]
    if op == "not_null":
        return value is not None
    if op == "null":
        return value is None
    if value is None:
        return False
    if op == "between":
        return args[0] <= value <= args[1]
    return check(value, op, *args)


def _fn(impl, name):
    """The function of that name; the restatement has no aliases, so anofox_fcst_ts_x falls back to ts_x there."""
    return getattr(impl, name, None) or getattr(impl, name.replace("anofox_fcst_", ""))


def golden_scalar(impl, st):
    """Runs one golden scalar statement through `impl` (api.py, or RefScalars) and returns (holds, value)."""
    if st["fn"] == "ts_conformal_apply_of_learn":
        r, a, m, s, f = st["args"]
        value = impl.ts_conformal_apply(f, impl.ts_conformal_learn(r, a, m, s))
    else:
        value = _fn(impl, st["fn"])(*st["args"])
    value = _field(value, st["field"])
    return _holds(value, st["check"]), value


def golden_pair(impl, st):
    a = _fn(impl, st["fn"])(*st["args"])
    b = _fn(impl, st["fn2"])(*st["args2"])
    return check(a, st["check"], b), (a, b)


def golden_table(impl, kats, st):
    """Runs one golden table statement; returns a list of (what, holds)."""
    t = kats["tables"][st["table"]]
    cols = [t[c] for c in st["cols"]]
    out = []
    if st["fn"] == "ts_conformal_calibrate":
        r = impl.ts_conformal_calibrate(*cols, st["params"])
        out.append(("columns", len(r) == st["n_columns"]))
        out += [(f, _holds(r[f], [op, v])) for f, op, v in st["checks"]]
    elif st["fn"] == "ts_conformal_calibrate_pair":
        a, b = (impl.ts_conformal_calibrate(*cols, p)["conformity_score"] for p in st["params"])
        out.append(("pair", check(a, st["check"], b)))
    else:
        groups = {st["group"]: t[st["group"]]}
        if st["fn"] == "ts_conformal_apply_by":
            r = impl.ts_conformal_apply_by(groups, *cols, st["score"])
        elif st["fn"] == "ts_interval_width_by":
            r = impl.ts_interval_width_by(groups, *cols)
        else:
            r = impl.ts_conformal_by(groups, *cols, st["params"])
        keys = list(r[st["group"]])
        out.append(("rows", len(keys) == st["n_rows"] and len(set(keys)) == st["n_rows"]))
        for g, want in st.get("expect", {}).items():
            i = keys.index(g)
            for f, v in want.items():
                got = r[f[:-1]][i][0] if f.endswith("0") else r[f][i]
                out.append(((g, f), got == v))
        if st["fn"] == "ts_conformal_by":
            out.append(("not null", all(x is not None for x in r["lower"])))
    return out
