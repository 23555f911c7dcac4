"""Shared inputs of the data-preparation tests: the reference's own statements as data (tests/golden/dataprep_kats.json, from
ts_fill_gaps_native.test, ts_gaps.test, ts_imputation.test, ts_filter.test, the data-prep statements of
extension_comparison.test and ts_type_preservation.test, and the unit tests of imputation.rs / gaps.rs), the way a statement is
run through the mirrors of anofox_forecast_amd.api and checked, the GPU batch call restated on tests/dataprep_ref.py, and the seeded
shapes of the GPU comparison."""
import json
import os

import numpy as np

import dataprep_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
US_PER_DAY = 86400 * 1000000
FIGURES = ("n_input", "n_null_input", "n_inserted", "n_trim_front", "n_trim_back", "n_null_output", "n_nonzero_output", "status")


def load_kats():
    with open(os.path.join(HERE, "golden", "dataprep_kats.json")) as f:
        return json.load(f)


def table_columns(table):
    """The columns of a golden table as the mirrors take them: dates as datetime64[D] / [us] / int32 / int64, a DOUBLE column as
    an object array with None at the NULLs."""
    cols = {}
    for j, (name, kind) in enumerate(zip(table["columns"], table["kinds"])):
        cells = [r[j] for r in table["rows"]]
        if kind == "DATE":
            cols[name] = np.array(cells, dtype="datetime64[D]")
        elif kind == "TIMESTAMP":
            cols[name] = np.array([c.replace(" ", "T") for c in cells], dtype="datetime64[us]")
        elif kind == "BIGINT":
            cols[name] = np.array(cells, dtype=np.int64)
        elif kind == "INTEGER" and name in ("date_col", "date", "dt"):
            cols[name] = np.array(cells, dtype=np.int32)
        else:
            cols[name] = np.array(cells, dtype=object)
    return cols


def kind_of(col):
    col = np.asarray(col)
    if np.issubdtype(col.dtype, np.datetime64):
        return "DATE" if np.datetime_data(col.dtype)[0] == "D" else "TIMESTAMP"
    return "INTEGER" if col.dtype == np.int32 else "BIGINT"


def run_statement(A, st, tables):
    """The statement through the mirror of its macro: a dict of columns (group, date, value first, as the table names them)."""
    t = tables[st["table"]]
    cols = table_columns(t)
    g, d, v = t["columns"][:3]
    extra = {n: cols[n] for n in t["columns"][3:]}
    fn = getattr(A, st["fn"])
    a = st["args"]
    base = st["fn"].replace("anofox_fcst_", "")
    if base == "ts_fill_gaps_by":
        return fn(cols[g], cols[d], cols[v], a["frequency"], group_name=g, date_name=d, value_name=v)
    if base.startswith("ts_fill_nulls_"):
        args = (a["fill_value"],) if base == "ts_fill_nulls_const_by" else ()
        return fn(cols[g], cols[d], cols[v], *args, group_name=g, date_name=d, value_name=v, extra=extra)
    if base in ("ts_drop_leading_zeros_by", "ts_drop_trailing_zeros_by", "ts_drop_edge_zeros_by"):
        return fn(cols[g], cols[d], cols[v], group_name=g, date_name=d, value_name=v, extra=extra)
    extra = dict(extra, **{d: cols[d]})                            # the drop filters are SELECT *: the date column passes through
    if base == "ts_drop_short_by":
        return fn(cols[g], a["min_length"], cols[v], group_name=g, value_name=v, extra=extra)
    if base == "ts_drop_gappy_by":
        return fn(cols[g], cols[v], a["max_gap_ratio"], group_name=g, value_name=v, extra=extra)
    return fn(cols[g], cols[v], group_name=g, value_name=v, extra=extra)


def _cell(x):
    if isinstance(x, np.datetime64):
        s = str(x).replace("T", " ")
        return s if len(s) == 10 else s[:19]
    if isinstance(x, (np.integer,)):
        return int(x)
    if isinstance(x, (np.floating,)):
        return float(x)
    return x


def check_statement(out, st, tables):
    t = tables[st["table"]]
    g, d, v = t["columns"][:3]
    e = st["expect"]
    n = len(out[g])
    rows = list(range(n))
    w = e.get("where")
    if w:
        for k in range(0, len(w), 2 if w[1] != "in" else 3):
            col, op = w[k], w[k + 1]
            col = {"value": v}.get(col, col)
            if op == "not_null":
                rows = [i for i in rows if out[col][i] is not None]
            elif op == "is_null":
                rows = [i for i in rows if out[col][i] is None]
            else:
                rows = [i for i in rows if out[col][i] in w[k + 2]]
    if "count" in e:
        assert len(rows) == e["count"], (st["name"], len(rows), e["count"])
    if "count_distinct" in e:
        col, want = e["count_distinct"]
        assert len(set(out[col][i] for i in rows)) == want, (st["name"], out[col])
    if "sum" in e:
        col, want = e["sum"]
        assert sum(out[col][i] for i in rows) == want, (st["name"], out[col])
    if "cell" in e:                                                # ORDER BY date LIMIT 1 OFFSET k
        col, k, want = e["cell"]
        order = np.argsort(np.asarray(out[d]), kind="stable")
        assert out[col][int(order[k])] == want, (st["name"], out[col])
    if "columns" in e:
        names, want = e["columns"]
        order = np.argsort(np.asarray(out[d]), kind="stable")
        got = [[_cell(out[c][int(i)]) for c in names] for i in order]
        assert got == want, (st["name"], got)
    if "date_kind" in e:
        assert kind_of(out[d]) == e["date_kind"], (st["name"], np.asarray(out[d]).dtype)
    if "rows" in e:
        got = sorted(([_cell(out[g][i]), _cell(np.asarray(out[d])[i]), _cell(out[v][i])] for i in range(n)), key=lambda r: (r[0], r[1]))
        assert got == e["rows"], (st["name"], got)


# --------------------------------------------------------------------------------------------
# the GPU batch call restated (the mirrors' host logic runs unchanged on top of it)
# --------------------------------------------------------------------------------------------
def to_cells(values, valid=None):
    """A float array and its validity as the restatement's list: None at a NULL."""
    vals = [float(x) for x in values]
    if valid is None:
        return vals
    return [x if ok else None for x, ok in zip(vals, valid)]


def ref_prepare_batch(series, valids=None, dates=None, gaps=False, frequency_micros=0, frequency_type="FIXED", trim="none", fill="none",
                      fill_value=0.0):
    out = []
    for i, s in enumerate(series):
        cells = to_cells(s, valids[i] if valids is not None and valids[i] is not None else None)
        d = [int(x) for x in dates[i]] if dates is not None else None
        r = R.prepare(d, cells, gaps=gaps, frequency_micros=frequency_micros, ftype=frequency_type, trim=trim, fill=fill,
                      fill_value=fill_value, sort=True)
        out.append(as_batch_result(r))
    return out


def as_batch_result(r):
    """A result of dataprep_ref.prepare in the form of api.prepare_batch."""
    return {"values": np.array([np.nan if x is None else x for x in r["values"]], dtype=np.float64),
            "valid": np.array([x is not None for x in r["values"]], dtype=bool),
            "dates": np.array(r["dates"], dtype=np.int64) if r["dates"] is not None else None,
            "figures": dict(zip(FIGURES, r["figures"])), "min": r["min"], "max": r["max"]}


def same_result(a, b):
    """Two results in the form of api.prepare_batch hold the same bits: values, validity, dates, figures, min and max."""
    if a["figures"] != b["figures"] or len(a["values"]) != len(b["values"]):
        return False
    if not np.array_equal(np.asarray(a["valid"], dtype=bool), np.asarray(b["valid"], dtype=bool)):
        return False
    if not np.array_equal(np.asarray(a["values"], dtype=np.float64).view(np.uint64), np.asarray(b["values"], dtype=np.float64).view(np.uint64)):
        return False
    if (a["dates"] is None) != (b["dates"] is None) or (a["dates"] is not None and not np.array_equal(a["dates"], b["dates"])):
        return False
    return all(R.bits(a[k]) == R.bits(b[k]) or (a[k] != a[k] and b[k] != b[k]) for k in ("min", "max"))


# --------------------------------------------------------------------------------------------
# seeded shapes
# --------------------------------------------------------------------------------------------
NULL_PATTERNS = ("none", "all", "single_front", "single_middle", "single_back", "leading", "trailing", "run1", "run2", "run15", "run16",
                 "run17", "alternating")


def null_pattern(name, n):
    """Validity of n rows: True = valid."""
    ok = np.ones(n, dtype=bool)
    if n == 0:
        return ok
    if name == "all":
        ok[:] = False
    elif name.startswith("single_"):
        ok[:] = False
        ok[{"front": 0, "middle": n // 2, "back": n - 1}[name[7:]]] = True
    elif name == "leading":
        ok[:max(1, n // 3)] = False
    elif name == "trailing":
        ok[n - max(1, n // 3):] = False
    elif name.startswith("run"):
        k = int(name[3:])
        lo = min(max(1, n // 4), n)
        ok[lo:min(n - 1, lo + k)] = False                        # an interior run when the series is long enough
    elif name == "alternating":
        ok[1::2] = False
    return ok


def ragged_lengths(n_series, t_rows, rng):
    """Lengths 0 .. t_rows with 0, 1 and t_rows present in the first wave when there is room."""
    ln = rng.integers(0, t_rows + 1, size=n_series)
    for k, v in enumerate((t_rows, 0, 1)):
        if k < n_series:
            ln[k] = min(v, t_rows)
    return ln.astype(np.int64)
