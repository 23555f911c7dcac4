"""Writes tests/golden/conformal_kats.json: the statements of the reference's test/sql/ts_conformal.test and the numeric examples of
conformal.rs's doc comments and unit tests, transcribed by hand as DATA -- the function, its inputs, the field of the result that
is looked at, a check kind with its operands, and the source file:line.  No SQL or Rust text is kept.

Not transcribed: the statements that only DESCRIBE a result or count its rows without looking at a value are kept as row-count
checks; ts_conformal.test's `conformal_backtest` table draws its forecasts from RANDOM(), so only the statements whose answer does
not depend on the draw are kept (the table here draws from a fixed seed); test/sql/ts_conformal_coverage.test is one pipeline
over 100,000 RANDOM() rows and ts_forecast_by with statistical thresholds (coverage >= 0.85 ...), which holds no statement that
can be pinned as data -- tests/test_gpu_conformal.py::test_end_to_end_on_the_device restates that workflow in small.

Run:  python tests/golden/make_conformal_kats.py
"""
import json
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
T = "test/sql/ts_conformal.test"
RS = "crates/anofox-fcst-core/src/conformal.rs"
TEN = [0.5, -0.3, 0.8, -0.2, 0.4, -0.6, 0.3, -0.4, 0.7, -0.5]
ONE_TO_20 = [float(i) for i in range(1, 21)]

# scalar statements: fn, args, field (None: the value itself; "lower[0]": element 0 of field lower), check
SCALARS = [
    ("ts_conformal_quantile", [[1.0, 2.0, 3.0, 4.0, 5.0], 0.1], None, ["abs_diff_lt", 4.6, 0.5], f"{T}:16"),
    ("ts_conformal_quantile", [[1.0, 2.0, 3.0, 4.0, 5.0], 0.5], None, ["abs_diff_lt", 3.0, 0.5], f"{T}:32"),
    ("ts_conformal_quantile", [[1.0], 0.1], None, ["not_null"], f"{T}:167"),
    ("ts_conformal_quantile", [[float(i) for i in range(1, 11)], 0.01], None, ["gt", 9.0], f"{T}:173"),
    ("ts_conformal_intervals", [[10.0, 20.0, 30.0], 2.0], "lower", ["eq", [8.0, 18.0, 28.0]], f"{T}:52"),
    ("ts_conformal_intervals", [[10.0, 20.0, 30.0], 2.0], "upper", ["eq", [12.0, 22.0, 32.0]], f"{T}:62"),
    ("ts_conformal_intervals", [[5.0, 10.0], 0.0], "lower", ["eq", [5.0, 10.0]], f"{T}:73"),
    ("ts_conformal_intervals", [[5.0, 10.0], 0.0], "upper", ["eq", [5.0, 10.0]], f"{T}:73"),
    ("ts_conformal_predict", [[-2.0, -1.0, 0.0, 1.0, 2.0], [100.0, 200.0], 0.1], "point", ["eq", [100.0, 200.0]], f"{T}:94"),
    ("ts_conformal_predict", [[1.0, 2.0, 3.0], [50.0], 0.1], "method", ["eq", "split_conformal"], f"{T}:102"),
    ("ts_conformal_predict", [[1.0, 2.0, 3.0, 4.0, 5.0], [10.0], 0.1], "lower[0]", ["lt", 10.0], f"{T}:109"),
    ("ts_conformal_predict", [[1.0, 2.0, 3.0, 4.0, 5.0], [10.0], 0.1], "upper[0]", ["gt", 10.0], f"{T}:110"),
    ("ts_conformal_predict", [[1.0, 2.0, 3.0], [100.0], 0.2], "coverage", ["eq", 0.8], f"{T}:180"),
    ("ts_conformal_predict_asymmetric", [[-1.0, -1.0, 0.0, 2.0, 4.0], [100.0], 0.1], "method", ["eq", "asymmetric_conformal"], f"{T}:121"),
    ("ts_conformal_predict_asymmetric", [[1.0, 2.0, 3.0], [50.0], 0.1], "coverage", ["eq", 0.9], f"{T}:127"),
    ("ts_mean_interval_width", [[8.0, 18.0], [12.0, 22.0]], None, ["eq", 4.0], f"{T}:138"),
    ("ts_mean_interval_width", [[0.0, 10.0], [5.0, 20.0]], None, ["eq", 7.5], f"{T}:145"),
    ("ts_mean_interval_width", [[0.0], [10.0]], None, ["eq", 10.0], f"{T}:151"),
    ("anofox_fcst_ts_mean_interval_width", [[0.0, 5.0], [10.0, 15.0]], None, ["eq", 10.0], f"{T}:157"),
    ("ts_conformal_evaluate", [[100.0, 110.0, 120.0, 130.0, 140.0], [95.0, 105.0, 115.0, 125.0, 135.0], [105.0, 115.0, 125.0, 135.0, 145.0], 0.1],
     "coverage", ["eq", 1.0], f"{T}:370"),
    ("ts_conformal_evaluate", [[100.0, 110.0, 150.0], [95.0, 105.0, 115.0], [105.0, 115.0, 125.0], 0.1], "violation_rate", ["gt", 0.0], f"{T}:381"),
    ("ts_conformal_evaluate", [[100.0, 110.0], [95.0, 105.0], [105.0, 115.0], 0.1], "n_observations", ["eq", 2], f"{T}:399"),
    ("ts_conformal_evaluate", [[100.0, 110.0], [95.0, 105.0], [105.0, 115.0], 0.1], "winkler_score", ["not_null"], f"{T}:399"),
    ("ts_conformal_coverage", [[100.0, 110.0, 120.0], [95.0, 105.0, 115.0], [105.0, 115.0, 125.0]], None, ["eq", 1.0], f"{T}:440"),
    # conformal.rs: doc comments and unit tests
    ("ts_conformal_quantile", [TEN, 0.1], None, ["gt", 0.0], f"{RS}:114"),
    ("ts_conformal_quantile", [TEN, 0.1], None, ["le", 0.801], f"{RS}:1193"),
    ("ts_conformal_quantile", [[1.0, -1.0, 2.0, -2.0, 3.0, -3.0, 4.0, -4.0, 5.0, -5.0], 0.5], None, ["between", 2.0, 4.0], f"{RS}:1202"),
    ("ts_conformal_quantile", [[1.0, 2.0, 3.0], -0.1], None, ["null"], f"{RS}:1209"),
    ("ts_conformal_intervals", [[100.0, 105.0, 110.0], 5.0], "lower", ["eq", [95.0, 100.0, 105.0]], f"{RS}:168"),
    ("ts_conformal_intervals", [[100.0, 105.0, 110.0], 5.0], "upper", ["eq", [105.0, 110.0, 115.0]], f"{RS}:169"),
    ("ts_conformal_predict", [TEN, [100.0, 105.0, 110.0], 0.1], "point", ["eq", [100.0, 105.0, 110.0]], f"{RS}:199"),
    ("ts_conformal_predict", [TEN, [100.0, 105.0, 110.0], 0.1], "coverage", ["eq", 0.9], f"{RS}:200"),
    ("ts_conformal_learn", [TEN, [0.1, 0.05], "symmetric", "split"], "n_levels", ["eq", 2], f"{RS}:692"),
    ("ts_conformal_apply_of_learn", [TEN, [0.1], "symmetric", "split", [100.0, 105.0, 110.0]], "n_forecasts", ["eq", 3], f"{RS}:889"),
]

# pairs: the first call's value against the second's
PAIRS = [
    ("ts_conformal_quantile", [ONE_TO_20, 0.05], "gt", "ts_conformal_quantile", [ONE_TO_20, 0.1], f"{T}:23"),
    ("anofox_fcst_ts_conformal_quantile", [[1.0, 2.0, 3.0], 0.1], "eq", "ts_conformal_quantile", [[1.0, 2.0, 3.0], 0.1], f"{T}:39"),
]


def tables():
    rng = random.Random(20240101)
    back = {"series_id": [], "actual": [], "forecast": []}
    for i in range(30):
        for sid in ("A", "B"):
            base = 100.0 + i + (10 if sid == "A" else 0)
            back["series_id"].append(sid)
            back["actual"].append(base)
            back["forecast"].append(base + (rng.random() - 0.5) * 5)        # the source draws RANDOM(); a fixed seed here
    fc = {"series_id": [], "point_forecast": []}
    for i in range(7):
        for sid in ("A", "B"):
            fc["series_id"].append(sid)
            fc["point_forecast"].append(130.0 + i + (10 if sid == "A" else 0))
    iv = {"series_id": [], "lower_bound": [], "upper_bound": []}
    for i in range(1, 6):
        for sid in ("A", "B"):
            iv["series_id"].append(sid)
            iv["lower_bound"].append(100.0 + i)
            iv["upper_bound"].append(110.0 + i + (5 if sid == "A" else 0))
    bt = {"group_col": [], "actual": [], "forecast": [], "point_forecast": []}
    for i in range(1, 21):
        bt["group_col"].append(f"product_{i % 2 + 1}")
        bt["actual"].append(100.0 + i)
        bt["forecast"].append(100.0 + i + (2.0 if i % 3 == 0 else -1.0))
        bt["point_forecast"].append(100.0 + i)
    return {"conformal_backtest": back, "conformal_forecasts": fc, "test_intervals": iv, "conformal_test_backtest": bt}


TABLE_STATEMENTS = [
    {"fn": "ts_conformal_calibrate", "table": "conformal_backtest", "cols": ["actual", "forecast"], "params": {"alpha": 0.1},
     "checks": [["conformity_score", "gt", 0.0], ["coverage", "eq", 0.9], ["n_residuals", "eq", 60]], "n_columns": 3, "src": f"{T}:216-245"},
    {"fn": "ts_conformal_calibrate_pair", "table": "conformal_backtest", "cols": ["actual", "forecast"], "params": [{"alpha": 0.2}, {"alpha": 0.1}],
     "check": "lt", "src": f"{T}:250"},
    {"fn": "ts_conformal_apply_by", "table": "conformal_forecasts", "group": "series_id", "cols": ["point_forecast"], "score": 5.0, "n_rows": 2,
     "expect": {"A": {"lower0": 135.0, "upper0": 145.0}, "B": {"lower0": 125.0, "upper0": 135.0}}, "src": f"{T}:262-284"},
    {"fn": "ts_interval_width_by", "table": "test_intervals", "group": "series_id", "cols": ["lower_bound", "upper_bound"], "n_rows": 2,
     "expect": {"A": {"mean_width": 15.0, "n_intervals": 5}, "B": {"mean_width": 10.0, "n_intervals": 5}}, "src": f"{T}:303-327"},
    {"fn": "ts_conformal_by", "table": "conformal_test_backtest", "group": "group_col", "cols": ["actual", "forecast", "point_forecast"],
     "params": {"alpha": "0.1"}, "n_rows": 2, "src": f"{T}:420"},
]


def main():
    out = {"scalars": [{"fn": f, "args": a, "field": fld, "check": c, "src": s} for f, a, fld, c, s in SCALARS],
           "pairs": [{"fn": f, "args": a, "check": op, "fn2": g, "args2": b, "src": s} for f, a, op, g, b, s in PAIRS],
           "tables": tables(), "table_statements": TABLE_STATEMENTS}
    path = os.path.join(HERE, "conformal_kats.json")
    json.dump(out, open(path, "w"), indent=1)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
