"""Cases shared by tests/test_metrics_cpu.py and tests/test_gpu_metrics.py: the golden statements, the shape block of the
bit-equality test, and api.metrics_batch answered by the restatement (tests/metrics_ref.py)."""
import functools
import json
import math
import os

import numpy as np

import metrics_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
FIGURES = R.FIGURES
TWO_INPUT = ("mae", "mse", "rmse", "mape", "smape", "r2", "bias")
# the lengths of the shape block, in order, repeated over the groups; the last group has 5,000 rows (the 64-row tiles wrap many times)
LENGTHS = (0, 1, 2, 3, 27, 28, 63, 64, 65, 127, 128, 129)
N_GROUPS = 130                       # two full waves and a partial one
LONG_ROWS = 5000
LEVELS = (0.1, 0.5, 0.9)


def load_kats():
    return json.load(open(os.path.join(HERE, "golden", "metrics_kats.json")))


def same_bits(got, want):
    """Equality of bits as far as the contract goes: NaN by NaN-ness (payloads are exempt), zeros by == (their sign is exempt)."""
    if want != want:
        return got != got
    return got == want


def check(value, op, *args):
    if op == "abs_diff_lt":
        return abs(value - args[0]) < args[1]
    if op == "gt":
        return value > args[0]
    if op == "lt":
        return value < args[0]
    if op == "round":
        return round(value, args[0]) == args[1]
    raise KeyError(op)


def table_statement(kats, st):
    """(group_columns dict, date, value columns) of a golden table statement, with its WHERE applied."""
    cols = kats["tables"][st["table"]]["columns"]
    n = len(cols[st["date"]])
    keep = [i for i in range(n) if all(cols[k][i] == v for k, v in st.get("where", {}).items())]
    groups = {g: [cols[g][i] for i in keep] for g in st["groups"]}
    date = np.array([cols[st["date"]][i] for i in keep], dtype=np.int64)
    values = [np.array([cols[c][i] for i in keep], dtype=np.float64) for c in st["cols"]]
    return groups, date, values


def run_statement(A, kats, st):
    groups, date, values = table_statement(kats, st)
    fn = getattr(A, st["fn"])
    if "quantile" in st:
        return fn(groups, date, *values, st["quantile"])
    return fn(groups, date, *values)


def check_statement(A, kats, st):
    t = run_statement(A, kats, st)
    metric = [k for k in t if k not in st["groups"]]
    assert len(metric) == 1 and list(t)[:len(st["groups"])] == st["groups"]
    n = len(t[metric[0]])
    if "n_rows" in st:
        assert n == st["n_rows"]
    for g, k in st.get("n_distinct", {}).items():
        assert len(set(t[g])) == k
    if "expect" in st:
        assert metric[0] == st["column"]
        rows = {tuple(t[g][i] for g in st["groups"]): t[metric[0]][i] for i in range(n)}
        assert len(rows) == len(st["expect"])
        for key, v in st["expect"]:
            assert rows[tuple(key)] == v, (st["name"], key, rows[tuple(key)], v)


def ref_metrics_batch(actual, forecast=None, second=None, lower=None, upper=None, quantiles=None, levels=None, figures=("mae",), quantile=0.5,
                      drop_nan=False):
    """api.metrics_batch answered by the restatement: the same arguments, the same dict."""
    names = [str(f).lower() for f in figures]
    n = len(actual)
    out = {f: np.full(n, np.nan) for f in names}
    code, message = np.zeros(n, dtype=np.int32), []
    for i in range(n):
        pick = lambda cols: None if cols is None else list(cols[i])
        qs = None if quantiles is None else [list(q[i]) for q in quantiles]
        fig, err = R.group_figures(names, list(actual[i]), pick(forecast), pick(second), pick(lower), pick(upper), qs, levels, quantile, drop_nan)
        for f in names:
            out[f][i] = fig[f]
        code[i] = 0 if err is None else 3
        message.append(err or "")
    out["code"], out["message"] = code, message
    return out


def shape_lengths():
    lens = [LENGTHS[i % len(LENGTHS)] for i in range(N_GROUPS)]
    lens[-1] = LONG_ROWS
    return lens


@functools.lru_cache(maxsize=None)
def shape_block(nan_in=None):
    """The blocks of the bit-equality test: per group actual, forecast, second, lower, upper and three quantile forecasts, every
    value rounded to one decimal so that exact ties, exact zeros (MAPE's and sMAPE's filters) and covered bounds occur.  nan_in:
    the name of one block to sprinkle NaNs into (every 7th row, starting at the group's index mod 7)."""
    rng = np.random.default_rng(20261018)
    blocks = {k: [] for k in ("actual", "forecast", "second", "lower", "upper")}
    quants = [[] for _ in LEVELS]
    for i, n in enumerate(shape_lengths()):
        a = np.round(rng.normal(0.0, 2.0, n), 1)
        f = np.round(a + rng.normal(0.0, 1.0, n), 1)
        f[::5] = a[::5]                                            # exact hits; together with a == 0.0 the rows sMAPE skips
        blocks["actual"].append(a)
        blocks["forecast"].append(f)
        blocks["second"].append(np.round(a + rng.normal(0.0, 1.5, n), 1))
        blocks["lower"].append(np.round(f - 1.0, 1))
        blocks["upper"].append(np.round(f + 1.0, 1))
        for k, z in enumerate((-1.3, 0.0, 1.3)):
            quants[k].append(np.round(f + z, 1))
    if nan_in is not None:
        target = quants[1] if nan_in == "quantiles" else blocks[nan_in]
        for i, col in enumerate(target):
            col[i % 7::7] = np.nan
    return blocks, quants


@functools.lru_cache(maxsize=None)
def shape_reference(nan_in=None, drop_nan=False):
    """Every figure of every group of shape_block by the restatement: ({figure: [values]}, [error text or None]).  Computed once."""
    blocks, quants = shape_block(nan_in)
    out = {f: [] for f in FIGURES}
    errs = []
    for i in range(N_GROUPS):
        fig, err = R.group_figures(FIGURES, blocks["actual"][i].tolist(), blocks["forecast"][i].tolist(), blocks["second"][i].tolist(),
                                   blocks["lower"][i].tolist(), blocks["upper"][i].tolist(), [q[i].tolist() for q in quants], list(LEVELS),
                                   0.9, drop_nan)
        for f in FIGURES:
            out[f].append(fig[f])
        errs.append(err)
    return out, errs


def is_nan(v):
    return isinstance(v, float) and math.isnan(v)
