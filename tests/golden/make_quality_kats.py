"""Writes tests/golden/quality_kats.json: the statements of the reference's test/sql/ts_data_quality.test, ts_summary.test:100-277,
extension_comparison.test:203-214, ts_varchar_edge_cases.test:110-124 and the unit tests at the end of quality.rs, transcribed by
hand as DATA -- the function, its inputs, the field of the result that is looked at, a check kind with its operands, and the
source file:line.  No SQL or Rust text is kept.  A date is the day number within its table; None is NULL.

Not transcribed: quality.rs test_temporal_score's cases with gaps, test_count_gaps and test_generate_quality_report -- no entry of
the extension reaches count_gaps or generate_quality_report; the helper-level cases of an EMPTY value slice
are pinned through an all-NULL list, the one way a caller reaches them.

The last block is a worked example, pinned exactly (hex floats): [1, 2, 3, 4, 5] has structural 5/5 * 0.7 + (5/30) * 0.3 = 0.75,
quartile indices 1 and 3 (no outliers, no extremes), lag-1 autocorrelation 0.4, so overall (0.75 + 1 + 1 + 1) / 4 = 0.9375.

Run:  python tests/golden/make_quality_kats.py
"""
import json
import math
import os

HERE = os.path.dirname(os.path.abspath(__file__))
T = "test/sql/ts_data_quality.test"
S = "test/sql/ts_summary.test"
X = "test/sql/extension_comparison.test"
V = "test/sql/ts_varchar_edge_cases.test"
RS = "crates/anofox-fcst-core/src/quality.rs"
FIVE = [1.0, 2.0, 3.0, 4.0, 5.0]
TEN = [float(i) for i in range(1, 11)]
HOLES = [1.0, None, 3.0, None, 5.0]
FIFTY = [float(i) for i in range(50)]
NORMAL = [50.0 + float(i % 10) - 5.0 for i in range(100)]
OUTLIERS = [float(i) for i in range(100)] + [1000.0, -500.0]
SINE = [math.sin(float(i) * 0.1) * 10.0 for i in range(50)]
EVERY_FIFTH = [None if i % 5 == 0 else float(i) + float(i % 7) for i in range(100)]
SCORES = ("structural_score", "temporal_score", "magnitude_score", "behavioral_score", "overall_score")

# scalar statements: args of _ts_data_quality, field (None: the value itself), check
SCALARS = (
    [([FIVE], f, ["not_null"], f"{T}:{line}") for f, line in zip(
        SCORES + ("n_gaps", "n_missing", "is_constant"), (15, 21, 27, 33, 39, 45, 51, 57))]
    + [
        ([FIVE], "overall_score", ["ge", 0.0], f"{T}:67"),
        ([FIVE], "structural_score", ["ge", 0.0], f"{T}:72"),
        ([TEN], "overall_score", ["gt", 0.5], f"{T}:82"),
        ([TEN], "n_gaps", ["eq", 0], f"{T}:88"),
        ([TEN], "n_missing", ["eq", 0], f"{T}:94"),
        ([[5.0] * 8], "is_constant", ["eq", True], f"{T}:104"),
        ([[float(i) for i in range(1, 9)]], "is_constant", ["eq", False], f"{T}:110"),
        ([HOLES], "n_missing", ["eq", 2], f"{T}:120"),
        ([HOLES], "overall_score", ["ge", 0.0], f"{T}:126"),
        ([None], None, ["null"], f"{T}:136"),
        ([FIVE], "n_gaps", ["eq", 0], f"{X}:207"),
        ([HOLES], "n_missing", ["eq", 2], f"{X}:212"),
        # quality.rs unit tests
        ([[1.0, 2.0, None, 4.0, 5.0]], "n_missing", ["eq", 1], f"{RS}:309"),
        ([[1.0, 2.0, None, 4.0, 5.0]], "is_constant", ["eq", False], f"{RS}:310"),
        ([[5.0] * 10], "is_constant", ["eq", True], f"{RS}:317"),
        ([FIFTY], "structural_score", ["gt", 0.9], f"{RS}:325"),
        ([[None] * 5], "structural_score", ["eq", 0.0], f"{RS}:336"),
        ([[float(i) for i in range(100)]], "temporal_score", ["eq", 1.0], f"{RS}:346"),
        ([NORMAL], "magnitude_score", ["gt", 0.8], f"{RS}:375"),
        ([[None] * 3], "magnitude_score", ["eq", 0.0], f"{RS}:392"),
        ([[5.0] * 20], "behavioral_score", ["eq", 0.0], f"{RS}:403"),
        ([SINE], "behavioral_score", ["gt", 0.5], f"{RS}:411"),
        ([[1.0, 2.0]], "behavioral_score", ["eq", 0.5], f"{RS}:419"),
    ]
    + [([EVERY_FIFTH], f, ["between", 0.0, 1.0], f"{RS}:{line}") for f, line in zip(SCORES, (467, 471, 475, 479, 483))]
    # the worked example, exact
    + [([FIVE], f, ["bits", float(v).hex()], f"{RS}:66-113 worked by hand")
       for f, v in zip(SCORES, (0.75, 1.0, 1.0, 1.0, 0.9375))]
    + [([FIVE], "n_missing", ["eq", 0], f"{RS}:66-113 worked by hand"), ([FIVE], "is_constant", ["eq", False], f"{RS}:66-113 worked by hand")]
)

# pairs: field of the first call against the same field of the second
PAIRS = [
    ([[1.0, 2.0, 3.0] + [None] * 10], "structural_score", "lt", [FIFTY], f"{RS}:331"),
    ([OUTLIERS], "magnitude_score", "lt", [NORMAL], f"{RS}:387"),
]


def table(groups):
    """{"group", "date", "value"} columns from (key, values) blocks; a block's dates are 0 .. len - 1 unless given."""
    g, d, v = [], [], []
    for block in groups:
        key, values = block[0], block[1]
        dates = block[2] if len(block) > 2 else list(range(len(values)))
        g += [key] * len(values)
        d += dates
        v += values
    return {"group": g, "date": d, "value": v}


def tables():
    by = [(("A" if i <= 10 else "B"), i % 10, float(i % 10 + 1)) for i in range(1, 21)]
    # the VARCHAR column of ts_varchar_edge_cases.test holds the shortest text of each double, so the cast back is the double itself
    varchar = lambda f: [float(repr(f(i))) for i in range(60)]
    return {
        "quality_test": table([("A", [float(i + 1) for i in range(10)])]),
        "test_dq_by": {"group": [r[0] for r in by], "date": [r[1] for r in by], "value": [r[2] for r in by]},
        "test_dq_agg": table([("A", [float(i + 1) for i in range(10)]), ("B", [5.0] * 10)]),
        "test_series": table([("A", [float(i + 1) for i in range(10)]), ("B", [float(i * 2) for i in range(5)]),
                              ("C", [float(i * 3) for i in range(8)])]),
        "constant_series": table([("X", [5.0] * 10)]),
        "series_nulls": table([("Y", [None if i % 3 == 0 else float(i) for i in range(10)])]),
        "comprehensive_series": table([("good1", [float(10 + i * 2) for i in range(20)]),
                                       ("good2", [50.0 + 10.0 * math.sin(i * 3.14159 / 6) for i in range(24)]),
                                       ("medium1", [float(20 + i) for i in range(6)]), ("constant1", [100.0] * 10)]),
        "varchar_data": table([("A", varchar(lambda i: 10.0 + i * 0.5 + math.sin(i * 3.14159 / 7) * 2)),
                               ("B", varchar(lambda i: 20.0 + i * 0.3 + math.cos(i * 3.14159 / 7) * 3))]),
    }


# table statements: fn, table, extra arguments, group filter (agg: the rows of one group; None: all rows, grouped by the caller),
# field, check
TABLE_STATEMENTS = [
    ("ts_data_quality", "quality_test", {"n_short": 5, "frequency": "1 day"}, None, None, ["row_count", 1], f"{T}:151"),
    ("ts_data_quality_by", "test_dq_by", {"n_short": 3, "frequency": "1d"}, None, None, ["row_count", 2], f"{T}:172"),
    ("ts_data_quality_agg", "test_dq_agg", {}, "A", "overall_score", ["not_null"], f"{T}:198"),
    ("ts_data_quality_agg", "test_dq_agg", {}, "A", "structural_score", ["not_null"], f"{T}:206"),
    ("ts_data_quality_agg", "test_dq_agg", {}, "B", "is_constant", ["eq", True], f"{T}:214"),
    ("ts_data_quality_agg", "test_dq_agg", {}, "A", "is_constant", ["eq", False], f"{T}:222"),
    ("ts_data_quality_agg", "test_dq_agg", {}, "A", "is_constant", ["eq", False], f"{T}:230"),
    ("ts_data_quality_agg", "test_dq_agg", {}, "B", "is_constant", ["eq", True], f"{T}:230"),
    ("ts_data_quality_agg", "test_dq_agg", {}, "A", "overall_score", ["between", 0.0, 1.0], f"{T}:240"),
    ("anofox_fcst_ts_data_quality_agg", "test_dq_agg", {}, "A", "overall_score", ["not_null"], f"{T}:249"),
    ("ts_data_quality_summary", "test_series", {"n_short": 5}, None, "n_total", ["eq", 3], f"{S}:111"),
    ("ts_data_quality_summary", "test_series", {"n_short": 5}, None, None, ["classes_add_up"], f"{S}:117"),
    ("ts_data_quality_summary", "test_series", {"n_short": 5}, None, "avg_score", ["between", 0.0, 1.0], f"{S}:123"),
    ("ts_data_quality_summary", "test_series", {"n_short": 5}, None, "n_good", ["ge", 0], f"{S}:134"),
    ("ts_data_quality_summary", "test_series", {"n_short": 5}, None, "n_fair", ["ge", 0], f"{S}:140"),
    ("ts_data_quality_summary", "test_series", {"n_short": 5}, None, "n_poor", ["ge", 0], f"{S}:146"),
    ("ts_data_quality_summary", "test_series", {"n_short": 3}, None, "n_total", ["eq", 3], f"{S}:157"),
    ("ts_data_quality_summary", "test_series", {"n_short": 10}, None, "n_total", ["eq", 3], f"{S}:162"),
    ("ts_data_quality_summary", "constant_series", {"n_short": 5}, None, "n_total", ["eq", 1], f"{S}:180"),
    ("ts_data_quality_summary", "series_nulls", {"n_short": 5}, None, "n_total", ["eq", 1], f"{S}:194"),
    ("ts_data_quality_summary", "comprehensive_series", {"n_short": 5}, None, "n_total", ["eq", 4], f"{S}:241"),
] + [
    ("ts_data_quality_summary", "test_series", {"n_short": 5}, None, f, ["not_null"], f"{S}:{line}")
    for f, line in zip(("n_total", "n_good", "n_fair", "n_poor", "avg_score"), (270, 271, 272, 273, 274))
] + [
    ("ts_data_quality", "varchar_data", {"n_short": 10, "frequency": "1d"}, None, None, ["row_count", 2], f"{V}:114"),
    ("ts_data_quality", "varchar_data", {"n_short": 10, "frequency": "1d"}, "A", "overall_score", ["not_null"], f"{V}:120"),
]


def main():
    doc = {
        "scalars": [{"fn": "_ts_data_quality", "args": a, "field": f, "check": c, "src": s} for a, f, c, s in SCALARS],
        "pairs": [{"fn": "_ts_data_quality", "args": a, "field": f, "op": op, "other_args": b, "src": s} for a, f, op, b, s in PAIRS],
        "tables": tables(),
        "table_statements": [{"fn": fn, "table": t, "args": a, "group": g, "field": f, "check": c, "src": s}
                             for fn, t, a, g, f, c, s in TABLE_STATEMENTS],
    }
    with open(os.path.join(HERE, "quality_kats.json"), "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
