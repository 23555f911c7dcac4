"""Pure-Python restatement of ts_aggregate_hierarchy and its string companions, independent of the library.

The operator (src/table_functions/ts_aggregate_hierarchy.cpp:246-386 of the reference) buffers the rows that have a date (a NULL
value is 0.0, a NULL id is the string "NULL"), then walks them in table order and, for every level 0 .. N, does
`aggregations[BuildUniqueId(level)][date] += value` on a std::map whose cells start as +0.0; the cells come out sorted by unique_id
(byte order), then date.  `aggregate` is that, statement for statement.  `aggregate_block` is the same chain for the block form the
kernels take (series on a common date grid, a CSR plan whose member order is the order of the additions).

Nothing here imports the package under test.
"""
from __future__ import annotations

import numpy as np


def build_unique_id(id_values, level, separator="|", aggregate_keyword="AGGREGATED"):
    """BuildUniqueId (:108-130)."""
    result = ""
    for i in range(len(id_values)):
        if i > 0:
            result += separator
        result += id_values[i] if i < level else aggregate_keyword
    return result


def collect(dates, values, ids):
    """The in-out function (:246-313): rows as (date, value, [id strings]); a NULL date drops the row."""
    rows = []
    for r in range(len(dates)):
        if dates[r] is None:
            continue
        value = 0.0 if values[r] is None else float(values[r])
        rows.append((dates[r], value, ["NULL" if col[r] is None else str(col[r]) for col in ids]))
    return rows


def aggregate(dates, values, ids, separator="|", aggregate_keyword="AGGREGATED"):
    """The finalize (:343-386): [(unique_id, date, value)] sorted by (unique_id bytes, date)."""
    aggregations = {}
    for date, value, id_values in collect(dates, values, ids):
        for level in range(len(ids) + 1):
            unique_id = build_unique_id(id_values, level, separator, aggregate_keyword)
            by_date = aggregations.setdefault(unique_id, {})
            by_date[date] = by_date.get(date, 0.0) + value
    out = []
    for unique_id in sorted(aggregations, key=lambda u: u.encode("utf-8")):
        for date in sorted(aggregations[unique_id]):
            out.append((unique_id, date, aggregations[unique_id][date]))
    return out


def plan(column_of):
    """CSR plan of a [n_groupings][n_series] table of output columns (-1: none): (n_out, col_offsets, members), the members of a
    column in (series, grouping) order -- the order in which a row and then its levels reach a cell."""
    column_of = [list(g) for g in column_of]
    n_series = len(column_of[0]) if column_of else 0
    n_out = max([c for g in column_of for c in g] + [-1]) + 1
    cols = [[] for _ in range(n_out)]
    for s in range(n_series):
        for g in range(len(column_of)):
            if column_of[g][s] >= 0:
                cols[column_of[g][s]].append(s)
    offsets = [0]
    for c in cols:
        offsets.append(offsets[-1] + len(c))
    return n_out, offsets, [s for c in cols for s in c]


def aggregate_block(series, first, col_offsets, members, valids=None, presents=None, reverse=False):
    """The same chain on the block form: series[s][t] sits at grid position first[s] + t; column c adds its members in plan order
    (reverse=True: in the opposite order -- only to show that the order matters).  Returns per column (first, length, values,
    present): the span from the smallest to the largest position that has a row, 0.0 / 0 where no member has one."""
    out = []
    for c in range(len(col_offsets) - 1):
        cell = {}
        ms = members[col_offsets[c]:col_offsets[c + 1]]
        for s in (reversed(ms) if reverse else ms):
            for t in range(len(series[s])):
                if presents is not None and presents[s] is not None and not presents[s][t]:
                    continue
                null = valids is not None and valids[s] is not None and not valids[s][t]
                g = int(first[s]) + t
                cell[g] = cell.get(g, 0.0) + (0.0 if null else float(series[s][t]))
        if not cell:
            out.append((0, 0, np.zeros(0), np.zeros(0, dtype=np.uint8)))
            continue
        lo, hi = min(cell), max(cell)
        y = np.zeros(hi - lo + 1)
        p = np.zeros(hi - lo + 1, dtype=np.uint8)
        for g, v in cell.items():
            y[g - lo] = v
            p[g - lo] = 1
        out.append((lo, hi - lo + 1, y, p))
    return out


def same_bits(a, b):
    """Elementwise: equal bit patterns, or both NaN (the payload of a NaN is exempt; the sign of a zero is not)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


# ---- the three string companions ----
def combine_keys(ids, separator="|"):
    """ts_combine_keys.cpp:180-189."""
    n = len(ids[0]) if ids else 0
    return [separator.join("NULL" if col[r] is None else str(col[r]) for col in ids) for r in range(n)]


def split_string(text, separator):
    """ts_split_keys.cpp:127-143."""
    if separator == "":
        return [text]
    result, start = [], 0
    end = text.find(separator)
    while end != -1:
        result.append(text[start:end])
        start = end + len(separator)
        end = text.find(separator, start)
    result.append(text[start:])
    return result


def split_keys(unique_ids, separator="|", columns=None):
    """ts_split_keys.cpp:209-226, 343-357: (column names, rows of parts, kept row indices)."""
    names = [c for c in (columns or []) if c is not None] or ["id_part_1", "id_part_2", "id_part_3"]
    rows, kept = [], []
    for r, u in enumerate(unique_ids):
        if u is None:
            continue
        parts = split_string(str(u), separator)
        while len(parts) < len(names):
            parts.append("")
        rows.append(parts[:len(names)])
        kept.append(r)
    return names, rows, kept


def validate_separator(ids, separator="|"):
    """ts_validate_separator.cpp:153-259."""
    distinct = set()
    for col in ids:
        for v in col:
            if v is not None:
                distinct.add(str(v))
    conflicting = [v for v in sorted(distinct, key=lambda u: u.encode("utf-8")) if v.find(separator) != -1]
    if not conflicting:
        message = "Separator is safe to use"
    else:
        message = "Separator '" + separator + "' found in " + str(len(conflicting)) + " value(s). Try: "
        suggestions = []
        for alt in ("-", ".", "::", "__", "#"):
            if separator != alt and separator.find(alt) == -1:
                suggestions.append("'" + alt + "'")
        message += ", ".join(suggestions)
    return {"separator": separator, "is_valid": not conflicting, "n_conflicts": len(conflicting), "conflicting_values": conflicting,
            "message": message}
