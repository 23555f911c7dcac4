"""Deterministic case families for the hierarchy tests, and the evaluator of the golden pins.

A case is a dict: "series" (list of fp64 arrays), "first" (int64 [n]), "valids" / "presents" (lists of bool arrays or None),
"column_of" (int32 [G, n]; -1 = none) and the CSR plan hierarchy_ref.plan makes of it ("n_out", "offsets", "members").  The
restatement's answer is computed once per case and cached (expected()).

Every family holds values for which the order of the additions changes the bits: mixes of 1e16, 1.0, -1e16 and 0.1, denormals,
and -- in cases of their own -- +-inf and NaN.  The assertion at the bottom of this file checks, on the CPU and under the
restatement alone, that adding each wide column's members in REVERSED order changes the bits of at least half of the cells of
every family's wide columns: an order-agnostic kernel cannot pass the bit comparisons.
"""
from __future__ import annotations

import functools

import numpy as np

import hierarchy_ref as R

WIDTHS = (1, 2, 63, 64, 65, 128, 129, 200)       # member counts per column: around one and two tiles of the tile route
ROWS = (1, 2, 63, 64, 65, 130, 257)              # grid rows: around one row tile of either route, and several
N_SERIES = 230
WIDE = 63                                        # "wide" columns of the order-sensitivity condition
PALETTE = np.array([1e16, 1.0, -1e16, 0.1, 0.3, 7.7, -2.5, 5e-324, 3e-310, 1e-3, 123456.789, -0.1])


def _values(rng, n):
    return PALETTE[rng.integers(0, len(PALETTE), size=n)] * rng.integers(1, 4, size=n)


def mixed_plan(n=N_SERIES, seed=7):
    """One plan that mixes every width, each once with consecutive and once with scattered members, plus a column in which one
    series appears twice and one column nobody maps to.  Every column is one grouping (the duplicate needs a second one)."""
    rng = np.random.default_rng(seed)
    columns = []
    for w in WIDTHS:
        s0 = (7 * w) % (n - w + 1)
        columns.append(list(range(s0, s0 + w)))
        columns.append(sorted(rng.choice(n, size=w, replace=False).tolist()))
    order = rng.permutation(len(columns)).tolist()               # wide and narrow columns side by side in one wave
    columns = [columns[i] for i in order]
    empty = 5
    columns.insert(empty, [])
    dup = len(columns)
    columns.append([5, 9, 140])
    column_of = -np.ones((len(columns) + 1, n), dtype=np.int32)
    for c, ms in enumerate(columns):
        column_of[c, ms] = c
    column_of[len(columns), 9] = dup                             # series 9 a second time in the same column
    return column_of, empty, dup


def _finish(case):
    n_out, offsets, members = R.plan(case["column_of"].tolist())
    case.update(n_out=n_out, offsets=np.array(offsets, dtype=np.int32), members=np.array(members, dtype=np.int32),
                n_series=len(case["series"]))
    case.setdefault("valids", None)
    case.setdefault("presents", None)
    return case


def widths_case(T, ragged, seed=0):
    rng = np.random.default_rng(1000 * T + 10 * seed + int(ragged))
    column_of, empty, dup = mixed_plan()
    n = column_of.shape[1]
    if ragged:
        first = rng.integers(-70, 71, size=n).astype(np.int64)           # spans start and end inside tiles
        lens = rng.integers(1, T + 1, size=n)
    else:
        first = np.full(n, 11, dtype=np.int64)
        lens = np.full(n, T)
    lens[17] = 0                                                         # a series of length 0
    series = [_values(rng, int(k)) for k in lens]
    return _finish({"name": f"widths_T{T}_{'ragged' if ragged else 'equal'}", "family": "widths", "series": series, "first": first,
                    "column_of": column_of, "empty_column": empty, "dup_column": dup})


def masks_case(T=70, seed=3):
    """present holes inside a column's span, NULL values, a single-member column whose value is -0.0, an all-absent column."""
    rng = np.random.default_rng(seed)
    column_of, empty, dup = mixed_plan()
    n = column_of.shape[1]
    first = rng.integers(0, 9, size=n).astype(np.int64)
    series = [_values(rng, T) for _ in range(n)]
    presents = [rng.random(T) > 0.2 for _ in range(n)]
    valids = [rng.random(T) > 0.15 for _ in range(n)]
    for s in range(n):
        presents[s][20 - first[s]:24 - first[s]] = False                 # grid rows 20 .. 23: a hole in EVERY column
        presents[s][0] = presents[s][T - 1] = True
    extra = column_of.shape[0]
    column_of = np.vstack([column_of, -np.ones((2, n), dtype=np.int32)])
    n_cols = int(column_of.max()) + 1
    column_of[extra, 33] = n_cols                                        # single member: -0.0 in, +0.0 out
    series[33] = np.where(np.arange(T) % 2 == 0, -0.0, series[33])
    valids[33][:] = True
    column_of[extra + 1, 41] = n_cols + 1                                # every row of its only member is absent
    column_of[:extra, 41] = -1
    presents[41][:] = False
    return _finish({"name": "masks", "family": "masks", "series": series, "first": first, "column_of": column_of, "valids": valids,
                    "presents": presents, "empty_column": empty, "dup_column": dup, "negzero_column": n_cols, "absent_column": n_cols + 1,
                    "hole_rows": (20, 24)})


def nonfinite_case(T=66, seed=5):
    rng = np.random.default_rng(seed)
    column_of, empty, dup = mixed_plan()
    n = column_of.shape[1]
    series = [_values(rng, T) for _ in range(n)]
    for s in range(2, n, 40):                                            # a few series: most cells stay finite and order-sensitive
        at = rng.choice(T, size=3, replace=False)
        series[s][at] = [np.inf, -np.inf, np.nan]
    return _finish({"name": "nonfinite", "family": "nonfinite", "series": series, "first": np.zeros(n, dtype=np.int64),
                    "column_of": column_of, "empty_column": empty, "dup_column": dup})


def prefix_case(n_leaf=40, T=60, seed=11):
    """A key-sorted block under a prefix hierarchy (2 states x 5 stores x 4 items): level 0 the total, level 1 the state, level 2 the
    store, level 3 the leaf -- columns numbered as the byte-sorted unique_ids are.  No hole: the result goes into the batch layer."""
    rng = np.random.default_rng(seed)
    ids = [(f"S{s // 20}", f"T{s // 4:02d}", f"I{s:03d}") for s in range(n_leaf)]
    series = [np.round(50.0 + 20.0 * rng.random(T) + 5.0 * np.sin(np.arange(T) * 0.9 + s), 3) + 0.1 for s in range(n_leaf)]
    series[3] = series[3] + 1e16
    series[4] = series[4] - 1e16
    uid = [[R.build_unique_id(list(k), level) for k in ids] for level in range(4)]
    names = sorted({u for level in uid for u in level}, key=lambda u: u.encode("utf-8"))
    column = {u: c for c, u in enumerate(names)}
    column_of = np.array([[column[u] for u in level] for level in uid], dtype=np.int32)
    return _finish({"name": "prefix", "family": "prefix", "series": series, "first": np.zeros(n_leaf, dtype=np.int64), "column_of": column_of,
                    "ids": ids, "unique_ids": names})


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = [widths_case(T, ragged) for T in ROWS for ragged in (False, True)]
    cases += [masks_case(), nonfinite_case(), prefix_case()]
    return {c["name"]: c for c in cases}


CASE_NAMES = [f"widths_T{T}_{k}" for T in ROWS for k in ("equal", "ragged")] + ["masks", "nonfinite", "prefix"]


@functools.lru_cache(maxsize=None)
def expected(name, reverse=False):
    """The restatement's columns of a case: [(first, length, values, present)], computed once."""
    c = all_cases()[name]
    return R.aggregate_block(c["series"], c["first"], c["offsets"].tolist(), c["members"].tolist(), c["valids"], c["presents"], reverse=reverse)


def expected_block(name, t_out, ld_out, y_fill=0.0, p_fill=0):
    """The restatement as the output block [t_out x ld_out] (columns >= n_out and nothing else keep the fill values)."""
    c = all_cases()[name]
    cols = expected(name)
    y = np.full((t_out, ld_out), y_fill, dtype=np.float64)
    p = np.full((t_out, ld_out), p_fill, dtype=np.uint8)
    y[:, :c["n_out"]] = 0.0
    p[:, :c["n_out"]] = 0
    for k, (_f, length, vals, pres) in enumerate(cols):
        rows = min(length, t_out)                        # rows >= t_out of a longer column are not written
        y[:rows, k] = vals[:rows]
        p[:rows, k] = pres[:rows]
    return y, p, np.array([k[1] for k in cols], dtype=np.int32), np.array([k[0] for k in cols], dtype=np.int64)


def pack(case, pad=0, sentinel=np.nan):
    """The source block of a case: (y [T x ld], valid, present (uint8 or None), lengths int32 [ld], first int64 [ld]); ld is
    n_series + pad, and the pad columns and the rows past a series' length hold the sentinel."""
    n = case["n_series"]
    T = max([len(s) for s in case["series"]] + [1])
    ld = n + pad
    y = np.full((T, ld), sentinel, dtype=np.float64)
    valid = None if case["valids"] is None else np.ones((T, ld), dtype=np.uint8)
    present = None if case["presents"] is None else np.ones((T, ld), dtype=np.uint8)
    lengths = np.zeros(ld, dtype=np.int32)
    first = np.zeros(ld, dtype=np.int64)
    for s in range(n):
        k = len(case["series"][s])
        y[:k, s] = case["series"][s]
        lengths[s] = k
        first[s] = case["first"][s]
        if valid is not None:
            valid[:k, s] = case["valids"][s]
            y[:k, s][~np.asarray(case["valids"][s], dtype=bool)] = sentinel       # a NULL slot's value must not be read
        if present is not None:
            present[:k, s] = case["presents"][s]
    return y, valid, present, lengths, first


def order_sensitivity(name):
    """Share of the cells of a case's wide columns whose bits change when the members are added in reversed order."""
    c = all_cases()[name]
    fwd, rev = expected(name), expected(name, True)
    cells = changed = 0
    for k in range(c["n_out"]):
        if c["offsets"][k + 1] - c["offsets"][k] < WIDE or fwd[k][1] == 0:
            continue
        keep = fwd[k][3] != 0
        same = R.same_bits(fwd[k][2], rev[k][2])[keep]
        cells += int(same.size)
        changed += int((~same).sum())
    return changed, cells


def check_order_sensitivity():
    """The condition of the bit comparisons: per family, reversing the order changes at least half of the wide columns' cells."""
    by_family = {}
    for name in CASE_NAMES:
        fam = all_cases()[name]["family"]
        if fam == "prefix":
            continue                                     # 40 leaves: no wide column
        ch, n = order_sensitivity(name)
        a, b = by_family.get(fam, (0, 0))
        by_family[fam] = (a + ch, b + n)
    for fam, (ch, n) in by_family.items():
        assert n > 0 and 2 * ch >= n, f"family {fam}: only {ch} of {n} wide cells depend on the order of addition"
    return by_family


# ---- the golden pins ----
def _cells(table, name):
    cells = table["columns"][name]
    kind = table.get("types", {}).get(name)
    if kind == "DATE":
        return np.array(cells, dtype="datetime64[D]")
    if kind == "TIMESTAMP":
        return np.array(cells, dtype="datetime64[us]")
    return list(cells)


def _call(fns, function, table, args, params):
    """`table` is {"columns", "types"}; the output is a dict of columns in the function's own column order."""
    if function in ("ts_aggregate_hierarchy", "ts_combine_keys"):
        return fns[function](_cells(table, args[0]), _cells(table, args[1]), [_cells(table, a) for a in args[2:]], params, args[0], args[1])
    if function == "ts_split_keys":
        return fns[function](_cells(table, args[0]), _cells(table, args[1]), _cells(table, args[2]), params.get("separator", "|"),
                             params.get("columns"), args[1], args[2])
    return fns[function]([_cells(table, a) for a in args], params.get("separator", "|"))


def _as_table(out):
    types = {}
    for k, v in out.items():
        if isinstance(v, np.ndarray) and np.issubdtype(v.dtype, np.datetime64):
            types[k] = "DATE" if np.datetime_data(v.dtype)[0] == "D" else "TIMESTAMP"
    return {"columns": {k: [str(x) for x in v] if k in types else list(v) for k, v in out.items()}, "types": types}


def _cell(v):
    if isinstance(v, np.datetime64):
        return str(v)
    if isinstance(v, (np.floating, np.integer, np.bool_)):
        return v.item()
    return v


def run_pins(fns, golden):
    """Evaluates every pin with the functions `fns` (api-style signatures) and returns the failures as strings."""
    outputs, failures = [], []
    for i, p in enumerate(golden["pins"]):
        table = _as_table(outputs[p["table"]["from"]]) if isinstance(p["table"], dict) else golden["tables"][p["table"]]
        out = _call(fns, p["function"], table, p["args"], p["params"])
        outputs.append(out)
        got = None
        if p["check"] in ("cell", "cell_contains"):
            got = _cell(out[p["field"]])
            ok = (p["value"] in got) if p["check"] == "cell_contains" else got == p["value"] and type(got) is type(p["value"])
        elif p["check"] == "date_type":
            col = out[p["args"][0]]
            got = "DATE" if np.datetime_data(col.dtype)[0] == "D" else "TIMESTAMP"
            ok = got == p["value"]
        else:
            n_rows = len(next(iter(out.values())))
            keep = np.ones(n_rows, dtype=bool)
            for col, want in p["where"].items():
                if col == "like":
                    keep &= np.array([want[1] in str(v) for v in out[want[0]]], dtype=bool)
                else:
                    keep &= np.array([_cell(v) == want for v in out[col]], dtype=bool)
            rows = np.nonzero(keep)[0]
            if p["limit"] is not None:
                rows = rows[:p["limit"]]
            if p["check"] == "count":
                got = int(len(rows))
            elif p["check"] == "count_distinct":
                got = len({out["unique_id"][r] for r in rows})
            elif p["check"] == "column":
                got = [_cell(out[p["field"]][r]) for r in rows]
            else:
                got = [[_cell(out[f][r]) for f in p["field"]] for r in rows]
            ok = got == p["value"]
        if not ok:
            failures.append(f"pin {i} ({p['src']}, {p['function']}): got {got!r}, expected {p['value']!r}")
    return failures


def ref_functions():
    """The restatement behind api-style signatures, for run_pins."""
    def to_us(d):
        d = np.asarray(d)
        if np.datetime_data(d.dtype)[0] == "D":
            return [None if np.isnat(x) else int(x.astype(np.int64)) * 86400000000 for x in d], d.dtype
        return [None if np.isnat(x) else int(x.astype("datetime64[us]").astype(np.int64)) for x in d], d.dtype

    def from_us(us, dtype):
        if np.datetime_data(dtype)[0] == "D":
            return (np.array(us, dtype=np.int64) // 86400000000).astype("datetime64[D]")
        return np.array(us, dtype=np.int64).astype("datetime64[us]")

    def aggregate(date, value, ids, params, date_name, value_name):
        us, dtype = to_us(date)
        rows = R.aggregate(us, list(value), ids, params.get("separator", "|"), params.get("aggregate_keyword", "AGGREGATED"))
        return {"unique_id": np.array([r[0] for r in rows], dtype=object), date_name: from_us([r[1] for r in rows], dtype),
                value_name: np.array([r[2] for r in rows], dtype=np.float64)}

    def combine(date, value, ids, params, date_name, value_name):
        return {"unique_id": np.array(R.combine_keys(ids, params.get("separator", "|")), dtype=object), date_name: date, value_name: value}

    def split(unique_id, date, value, separator, columns, date_name, value_name):
        names, rows, kept = R.split_keys(list(unique_id), separator, columns)
        out = {c: np.array([r[i] for r in rows], dtype=object) for i, c in enumerate(names)}
        out[date_name] = np.asarray(date)[kept]
        out[value_name] = np.asarray(value)[kept]
        return out

    return {"ts_aggregate_hierarchy": aggregate, "ts_combine_keys": combine, "ts_split_keys": split,
            "ts_validate_separator": lambda ids, separator: R.validate_separator(ids, separator)}
