"""Shared by tests/test_quality_cpu.py and tests/test_gpu_quality.py: the golden statements of tests/golden/quality_kats.json with
their evaluators, and the series families the GPU entries are compared on.  Nothing here imports the library."""
import json
import math
import os
import random

import quality_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
same_bits = R.same_bits
bits = R.bits

# every length at which the kernel takes another path: the 64-row load chunks, the power-of-two pads of the sorting network, the
# LDS tile limit (2,048) and the workspace kernel beyond it
LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 29, 30, 31, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049, 5000)
WIDTHS = (1, 63, 64, 65, 257)


def load_kats():
    with open(os.path.join(HERE, "golden", "quality_kats.json")) as fh:
        return json.load(fh)


class RefImpl:
    """The SQL functions by the restatement; the GPU tests pass the api module's mirrors through ApiImpl instead."""

    def scalar(self, values):
        return R.scalar(values)

    def table(self, fn, group, date, value, **kw):
        return R.table(group, date, value)

    def summary(self, group, date, value, **kw):
        return R.summary(group, date, value)

    def agg(self, fn, ts, value):
        return R.agg(ts, value)


def check(kind, got):
    op = kind[0]
    if op == "null":
        return got is None
    if got is None:
        return False
    if op == "not_null":
        return True
    if op == "eq":
        return got is kind[1] if isinstance(kind[1], bool) else (not isinstance(got, bool) and got == kind[1])
    if op == "bits":
        return same_bits(got, float.fromhex(kind[1]))
    if op == "ge":
        return got >= kind[1]
    if op == "gt":
        return got > kind[1]
    if op == "lt":
        return got < kind[1]
    if op == "between":
        return kind[1] <= got <= kind[2]
    raise ValueError(op)


def golden_scalar(impl, st):
    got = impl.scalar(*st["args"])
    value = got if st["field"] is None or got is None else got[st["field"]]
    return check(st["check"], value), value


def golden_pair(impl, st):
    a, b = impl.scalar(*st["args"])[st["field"]], impl.scalar(*st["other_args"])[st["field"]]
    return {"lt": a < b, "gt": a > b, "eq": a == b}[st["op"]], (a, b)


def golden_table(impl, kats, st):
    t = kats["tables"][st["table"]]
    fn, kind = st["fn"], st["check"]
    if fn.endswith("_agg"):
        rows = [i for i, g in enumerate(t["group"]) if g == st["group"]]
        got = impl.agg(fn, [t["date"][i] for i in rows], [t["value"][i] for i in rows])
        return check(kind, None if got is None else got[st["field"]]), got
    if fn.endswith("_summary"):
        got = impl.summary(t["group"], t["date"], t["value"], **st["args"])
        if kind[0] == "classes_add_up":
            return got["n_good"] + got["n_fair"] + got["n_poor"] == got["n_total"], got
        return check(kind, got[st["field"]]), got
    got = impl.table(fn, t["group"], t["date"], t["value"], **st["args"])
    if kind[0] == "row_count":
        return len(got["unique_id"]) == kind[1] and all(len(got[f]) == kind[1] for f in R.FIELDS) and len(got) == 9, got
    row = got["unique_id"].index(st["group"])
    return check(kind, got[st["field"]][row]), got


# --------------------------------------------------------------------------------------------
# series families
# --------------------------------------------------------------------------------------------
def ar1(rng, n, phi):
    x, out = 0.0, []
    for _ in range(n):
        x = phi * x + rng.gauss(0.0, 1.0)
        out.append(x)
    return out


def poisson_zeros(rng, n):
    out = []
    for _ in range(n):
        if rng.random() < 0.6:
            out.append(0.0)
        else:
            k, p, l = 0, rng.random(), math.exp(-2.5)
            while p > l:
                k += 1
                p *= rng.random()
            out.append(float(k))
    return out


def family(rng, name, n):
    if name == "poisson":
        return poisson_zeros(rng, n)
    if name == "positive":
        return [rng.lognormvariate(1.0, 0.8) for _ in range(n)]
    if name == "level":
        return [1e6 + rng.gauss(0.0, 3.0) for _ in range(n)]
    if name == "constant":
        return [42.5] * n
    if name == "near_constant":                  # steps of one ulp below 1.0 (2^-53): inside EPSILON of the first value
        return [1.0 - 2.0 ** -53 * float(rng.randrange(2)) for _ in range(n)]
    if name == "ar99":
        return ar1(rng, n, 0.99)
    if name == "ar50":
        return ar1(rng, n, 0.5)
    if name == "ramp":
        return [0.25 * float(i) - 3.0 for i in range(n)]
    if name == "spikes":
        return [rng.gauss(10.0, 1.0) + (500.0 if rng.random() < 0.02 else 0.0) for _ in range(n)]
    if name == "zeros":
        return [rng.choice((0.0, -0.0)) for _ in range(n)]
    if name == "zeros_and_ones":
        return [rng.choice((0.0, -0.0, 0.0, -0.0, 1.0, -1.0)) for _ in range(n)]
    if name == "inf":
        return [rng.choice((math.inf, -math.inf)) if rng.random() < 0.05 else rng.gauss(0.0, 1.0) for _ in range(n)]
    if name == "plus_inf":
        return [math.inf if i % 11 == 3 else float(i % 5) for i in range(n)]
    if name == "nan":
        out = [rng.gauss(0.0, 1.0) for _ in range(n)]
        if n:
            out[rng.randrange(n)] = math.nan
        return out
    raise ValueError(name)


FAMILIES = ("poisson", "positive", "level", "constant", "near_constant", "ar99", "ar50", "ramp", "spikes", "zeros", "zeros_and_ones", "inf",
            "plus_inf", "nan")


def with_nulls(rng, series, p=0.03):
    return [None if rng.random() < p else v for v in series]


def length_batch(nulls):
    """One series per length of LENGTHS (positive reals); with `nulls` about 3 % of the rows are NULL (and at least one where the
    series has rows), so that the compacted count leaves the boundaries."""
    rng = random.Random(17 if nulls else 16)
    out = []
    for n in LENGTHS:
        s = family(rng, "positive", n)
        if nulls and n:
            s = with_nulls(rng, s)
            s[rng.randrange(n)] = None
        out.append(s)
    return out


def family_batch():
    """Every family at four lengths around the chunk and pad boundaries, raw and with NULLs; then the special series."""
    rng = random.Random(23)
    out = []
    for name in FAMILIES:
        for n in (5, 64, 100, 333):
            s = family(rng, name, n)
            out.append((f"{name}/{n}", s))
            out.append((f"{name}/{n}/nulls", with_nulls(rng, s, 0.1)))
    out.append(("all_null", [None] * 40))
    out.append(("one_value", [None] * 20 + [3.5] + [None] * 30))
    out.append(("two_values", [None, 1.0, None, 1.0 + 2.0 ** -52]))
    out.append(("masked_nan", [1.0, None, 2.0, 4.0]))
    out.append(("empty", []))
    return out


def width_batch(width):
    """`width` series of mixed lengths up to 140 from every family, NULLs in every third."""
    rng = random.Random(1000 + width)
    out = []
    for i in range(width):
        s = family(rng, FAMILIES[i % len(FAMILIES)], rng.randrange(0, 141))
        out.append(with_nulls(rng, s, 0.05) if i % 3 == 0 else s)
    return out


def split(series):
    """(values with 0.0 at the NULLs, validity) of a list with None at the NULLs."""
    return [0.0 if v is None else float(v) for v in series], [v is not None for v in series]
