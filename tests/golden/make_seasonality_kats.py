"""Writes tests/golden/seasonality_kats.json: the inputs and expected results of the reference's statements about
ts_detect_seasonality and ts_analyze_seasonality (test/sql/ts_seasonality.test, test/sql/extension_comparison.test:197), as data --
literal lists, the field looked at, the kind of check and its value -- not the statements themselves.

check kinds: "not_null" (the result, or its field, is not NULL), "is_null", "length_ge" (the list has at least `value` elements),
"ge" (the field is >= value), "eq" (the field equals value), "contains" (the list field holds value)."""
import json
import math
import os

HERE = os.path.dirname(os.path.abspath(__file__))

P4_16 = [1.0, 2.0, 3.0, 4.0] * 4
P4_12 = [1.0, 2.0, 3.0, 4.0] * 3
P40_16 = [10.0, 20.0, 30.0, 40.0] * 4
SRC = "test/sql/ts_seasonality.test"


def st(line, function, values, check, value=None, field=None, src=SRC):
    return {"src": f"{src}:{line}", "function": function, "input": values, "field": field, "check": check, "value": value}


def main():
    sine = [math.sin(i * 3.14159 * 2 / 12.0) * 10 + 50 for i in range(120)]
    statements = [
        st(15, "ts_detect_seasonality", P4_16, "length_ge", 0),
        st(21, "ts_detect_seasonality", [float(i) for i in range(1, 11)], "not_null"),
        st(27, "ts_detect_seasonality", [5.0] * 8, "not_null"),
        st(37, "ts_analyze_seasonality", P4_12, "not_null", field="detected_periods"),
        st(43, "ts_analyze_seasonality", P4_12, "not_null", field="primary_period"),
        st(49, "ts_analyze_seasonality", P4_12, "not_null", field="seasonal_strength"),
        st(55, "ts_analyze_seasonality", P4_12, "not_null", field="trend_strength"),
        st(65, "ts_analyze_seasonality", P40_16, "contains", 4, field="detected_periods"),
        st(71, "ts_analyze_seasonality", P40_16, "eq", 4, field="primary_period"),
        st(81, "ts_analyze_seasonality", P4_12, "ge", 0, field="seasonal_strength"),
        st(87, "ts_analyze_seasonality", P4_12, "ge", 0, field="trend_strength"),
        st(97, "ts_detect_seasonality", None, "is_null"),
        st(103, "ts_analyze_seasonality", None, "is_null"),
        st(197, "ts_detect_seasonality", sine, "length_ge", 0, src="test/sql/extension_comparison.test"),
    ]
    with open(os.path.join(HERE, "seasonality_kats.json"), "w") as fh:
        json.dump({"statements": statements}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
