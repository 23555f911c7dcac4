"""Writes tests/golden/hierarchy_sql.json: the tables, calls and expected cells of the reference's statements about
ts_aggregate_hierarchy, ts_combine_keys, ts_split_keys and ts_validate_separator (test/sql/ts_aggregate_hierarchy.test and the
hierarchy part of test/sql/ts_multi_key.test), as data -- the literal tables, which columns go in, the parameters, the row filter,
the kind of check and its value -- not the statements themselves.

A table is {"columns": {name: [cells]}, "types": {name: "DATE" | "TIMESTAMP"}} (other columns are strings or numbers; None = NULL).
A pin is {"src", "function", "table", "args": [column names in call order], "params" (the MAP or the named parameters), "where"
({output column: value} equality filter, or {"like": [column, substring]}), "check", "value"}.  A pin whose "table" is
{"from": <index of an earlier pin>} takes that pin's whole output as its input table (the round trip aggregate -> split).

check kinds: "count" (rows left by the filter), "count_distinct" (distinct unique_id), "column" (the cells of column `field` of the
rows left, in order), "rows" (the cells of the columns `field` = [names], first `limit` rows), "date_type" (type of the date column),
"cell" (one-row results: the cell of column `field`), "cell_contains" (substring of that cell)."""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
AGG = "test/sql/ts_aggregate_hierarchy.test"
MK = "test/sql/ts_multi_key.test"
D1, D2, F1 = "2024-01-01", "2024-01-02", "2024-02-01"


def table(names, rows, types=None):
    return {"columns": {n: [r[i] for r in rows] for i, n in enumerate(names)}, "types": types or {}}


TABLES = {
    "hier_sales_3": table(["region_id", "store_id", "item_id", "sale_date", "quantity"], [
        ("EU", "STORE001", "SKU42", D1, 100), ("EU", "STORE001", "SKU43", D1, 50), ("EU", "STORE002", "SKU44", D1, 75),
        ("US", "STORE003", "SKU45", D1, 200)], {"sale_date": "DATE"}),
    "hier_sales_2": table(["region", "store", "sale_date", "quantity"], [
        ("East", "Store1", D1, 100), ("East", "Store2", D1, 150), ("West", "Store3", D1, 200)], {"sale_date": "DATE"}),
    "hier_sales_4": table(["country", "region", "store", "item", "sale_date", "quantity"], [
        ("US", "East", "Store1", "SKU001", D1, 100), ("US", "East", "Store1", "SKU002", D1, 150), ("US", "West", "Store2", "SKU001", D1, 200),
        ("EU", "North", "Store3", "SKU001", D1, 250)], {"sale_date": "DATE"}),
    "ts_sales": table(["region", "store", "ts", "quantity"], [
        ("East", "Store1", "2024-01-01T10:00:00", 100), ("West", "Store2", "2024-01-01T10:00:00", 200)], {"ts": "TIMESTAMP"}),
    "multi_date_sales": table(["region", "store", "sale_date", "quantity"], [
        ("East", "Store1", D1, 100), ("East", "Store1", D2, 110), ("West", "Store2", D1, 200), ("West", "Store2", D2, 210)],
        {"sale_date": "DATE"}),
    "null_sales": table(["region", "store", "sale_date", "quantity"], [
        ("East", "Store1", D1, 100), ("East", None, D1, 50), (None, "Store2", D1, 200)], {"sale_date": "DATE"}),
    "sales": table(["region_id", "store_id", "item_id", "sale_date", "quantity"], [
        ("EU", "STORE001", "SKU42", D1, 100), ("EU", "STORE001", "SKU42", D2, 110), ("US", "STORE002", "SKU44", D1, 200)],
        {"sale_date": "DATE"}),
    "forecast_results": table(["unique_id", "forecast_date", "point_forecast"], [
        ("EU|STORE001|SKU42", F1, 120.0), ("EU|STORE001|AGGREGATED", F1, 200.0), ("EU|AGGREGATED|AGGREGATED", F1, 500.0),
        ("AGGREGATED|AGGREGATED|AGGREGATED", F1, 1000.0)], {"forecast_date": "DATE"}),
    "dash_results": table(["unique_id", "ds", "forecast"], [("EU-STORE001-SKU42", F1, 100.0)], {"ds": "DATE"}),
    "workflow_sales": table(["region", "store", "item", "dt", "qty"], [
        ("EU", "S1", "A", D1, 10), ("EU", "S1", "B", D1, 20), ("US", "S2", "C", D1, 30)], {"dt": "DATE"}),
    "test_ids": table(["region_id", "store_id", "item_id"], [
        ("EU", "STORE001", "SKU42"), ("EU", "STORE001", "SKU43"), ("US", "STORE002", "SKU44")]),
    "test_conflict": table(["region_id", "store_id", "item_id"], [("EU", "STORE|001", "SKU42")]),
}

H3 = ["sale_date", "quantity", "region_id", "store_id", "item_id"]
H2 = ["sale_date", "quantity", "region", "store"]
H4 = ["sale_date", "quantity", "country", "region", "store", "item"]
FR = ["unique_id", "forecast_date", "point_forecast"]
PARTS = ["id_part_1", "id_part_2", "id_part_3"]
IDS3 = ["region_id", "store_id", "item_id"]
TOTAL3 = "AGGREGATED|AGGREGATED|AGGREGATED"


def pin(src, line, function, tab, args, check, value, params=None, where=None, field=None, limit=None):
    return {"src": f"{src}:{line}", "function": function, "table": tab, "args": args, "params": params or {}, "where": where or {},
            "check": check, "value": value, "field": field, "limit": limit}


def agg(line, tab, args, check, value, src=AGG, **kw):
    return pin(src, line, "ts_aggregate_hierarchy", tab, args, check, value, **kw)


def main():
    uid = lambda u: {"unique_id": u}
    pins = [
        agg(22, "hier_sales_3", H3, "count_distinct", 10),
        agg(30, "hier_sales_3", H3, "count", 1, where=uid(TOTAL3)),
        agg(38, "hier_sales_3", H3, "column", [425.0], where=uid(TOTAL3), field="quantity"),
        agg(46, "hier_sales_3", H3, "column", [225.0], where=uid("EU|AGGREGATED|AGGREGATED"), field="quantity"),
        agg(54, "hier_sales_3", H3, "column", [150.0], where=uid("EU|STORE001|AGGREGATED"), field="quantity"),
        agg(62, "hier_sales_3", H3, "column", [100.0], where=uid("EU|STORE001|SKU42"), field="quantity"),
        agg(81, "hier_sales_2", H2, "count_distinct", 6),
        agg(89, "hier_sales_2", H2, "column", [450.0], where=uid("AGGREGATED|AGGREGATED"), field="quantity"),
        agg(97, "hier_sales_2", H2, "column", [250.0], where=uid("East|AGGREGATED"), field="quantity"),
        agg(105, "hier_sales_2", H2, "column", [100.0], where=uid("East|Store1"), field="quantity"),
        agg(126, "hier_sales_4", H4, "count_distinct", 13),
        agg(134, "hier_sales_4", H4, "column", [700.0], where=uid("AGGREGATED|AGGREGATED|AGGREGATED|AGGREGATED"), field="quantity"),
        agg(142, "hier_sales_4", H4, "column", [450.0], where=uid("US|AGGREGATED|AGGREGATED|AGGREGATED"), field="quantity"),
        agg(150, "hier_sales_4", H4, "column", [250.0], where=uid("US|East|AGGREGATED|AGGREGATED"), field="quantity"),
        agg(162, "hier_sales_2", H2, "count", 1, params={"separator": "::"}, where=uid("AGGREGATED::AGGREGATED")),
        agg(171, "hier_sales_2", H2, "count", 1, params={"aggregate_keyword": "ALL"}, where=uid("ALL|ALL")),
        agg(180, "hier_sales_2", H2, "column", [450.0], params={"separator": "-", "aggregate_keyword": "TOTAL"}, where=uid("TOTAL-TOTAL"),
            field="quantity"),
        agg(193, "hier_sales_2", H2, "date_type", "DATE"),
        agg(207, "ts_sales", ["ts", "quantity", "region", "store"], "date_type", "TIMESTAMP"),
        agg(228, "multi_date_sales", H2, "count", 10),
        agg(236, "multi_date_sales", H2, "column", [300.0], where={"unique_id": "AGGREGATED|AGGREGATED", "sale_date": D1}, field="quantity"),
        agg(244, "multi_date_sales", H2, "column", [320.0], where={"unique_id": "AGGREGATED|AGGREGATED", "sale_date": D2}, field="quantity"),
        agg(263, "null_sales", H2, "count", 3, where={"like": ["unique_id", "NULL"]}),
        agg(271, "null_sales", H2, "column", [350.0], where=uid("AGGREGATED|AGGREGATED"), field="quantity"),
        agg(283, "multi_date_sales", H2, "rows", [["AGGREGATED|AGGREGATED", D1], ["AGGREGATED|AGGREGATED", D2], ["East|AGGREGATED", D1],
                                                  ["East|AGGREGATED", D2]], field=["unique_id", "sale_date"], limit=4),
        pin(AGG, 305, "ts_combine_keys", "sales", H3, "count_distinct", 2),
        pin(AGG, 313, "ts_combine_keys", "sales", H3, "column", ["EU|STORE001|SKU42"], where={"like": ["unique_id", "SKU42"]}, field="unique_id",
            limit=1),
        pin(AGG, 321, "ts_combine_keys", "sales", H3[:4], "column", ["EU|STORE001"], where={"like": ["unique_id", "EU"]}, field="unique_id",
            limit=1),
        pin(AGG, 329, "ts_combine_keys", "sales", H3, "column", ["EU-STORE001-SKU42"], params={"separator": "-"},
            where={"like": ["unique_id", "EU"]}, field="unique_id", limit=1),
        pin(AGG, 338, "ts_combine_keys", "sales", H3, "count", 3),
        pin(AGG, 358, "ts_split_keys", "forecast_results", FR, "rows", [["EU", "STORE001", "SKU42"]],
            where={"id_part_1": "EU", "id_part_3": "SKU42"}, field=PARTS),
        pin(AGG, 366, "ts_split_keys", "forecast_results", FR, "rows", [["EU", "STORE001", "AGGREGATED"]],
            where={"id_part_1": "EU", "id_part_3": "AGGREGATED", "id_part_2": "STORE001"}, field=PARTS),
        pin(AGG, 374, "ts_split_keys", "forecast_results", FR, "rows", [["AGGREGATED", "AGGREGATED", "AGGREGATED"]],
            where={"id_part_1": "AGGREGATED", "id_part_2": "AGGREGATED", "id_part_3": "AGGREGATED"}, field=PARTS),
        pin(AGG, 387, "ts_split_keys", "dash_results", ["unique_id", "ds", "forecast"], "rows", [["EU", "STORE001", "SKU42"]],
            params={"separator": "-"}, field=PARTS),
        pin(AGG, 396, "ts_split_keys", "forecast_results", FR, "count", 4),
        pin(AGG, 404, "ts_split_keys", "forecast_results", FR, "rows", [["EU", "STORE001", "SKU42"]],
            params={"columns": ["region", "store", "item"]}, where={"region": "EU", "item": "SKU42"}, field=["region", "store", "item"]),
    ]
    # the round trip (:425-451): aggregate, check the total, split the aggregate's output, check two rows
    pins.append(agg(431, "workflow_sales", ["dt", "qty", "region", "store", "item"], "column", [60.0], where=uid(TOTAL3), field="qty"))
    trip = len(pins) - 1
    pins += [
        pin(AGG, 443, "ts_split_keys", {"from": trip}, ["unique_id", "dt", "qty"], "count", 1,
            where={"id_part_1": "AGGREGATED", "id_part_2": "AGGREGATED", "id_part_3": "AGGREGATED"}),
        pin(AGG, 449, "ts_split_keys", {"from": trip}, ["unique_id", "dt", "qty"], "column", [10.0],
            where={"id_part_1": "EU", "id_part_2": "S1", "id_part_3": "A"}, field="qty"),
        # test/sql/ts_multi_key.test: the separator check and the hierarchy statements that differ from the file above
        pin(MK, 22, "ts_validate_separator", "test_ids", IDS3, "cell", True, field="is_valid"),
        pin(MK, 28, "ts_validate_separator", "test_ids", IDS3, "cell", 0, field="n_conflicts"),
        pin(MK, 34, "ts_validate_separator", "test_ids", IDS3[:2], "cell", True, field="is_valid"),
        pin(MK, 40, "ts_validate_separator", "test_ids", IDS3, "cell", True, params={"separator": "-"}, field="is_valid"),
        pin(MK, 51, "ts_validate_separator", "test_conflict", IDS3, "cell", False, field="is_valid"),
        pin(MK, 56, "ts_validate_separator", "test_conflict", IDS3, "cell", 1, field="n_conflicts"),
        pin(MK, 62, "ts_validate_separator", "test_conflict", IDS3, "cell_contains", "Try", field="message"),
        agg(132, "hier_sales_3", H3, "count_distinct", 10, src=MK),
        agg(156, "hier_sales_3", H3, "count", 1, src=MK, where=uid("EU|AGGREGATED|AGGREGATED")),
        agg(172, "hier_sales_3", H3, "count", 1, src=MK, where=uid("EU|STORE001|AGGREGATED")),
        agg(196, "hier_sales_3", H3, "count", 1, src=MK, params={"separator": "-"}, where=uid("AGGREGATED-AGGREGATED-AGGREGATED")),
        agg(205, "hier_sales_3", H3, "count", 1, src=MK, params={"aggregate_keyword": "TOTAL"}, where=uid("TOTAL|TOTAL|TOTAL")),
        agg(293, "workflow_sales", ["dt", "qty", "region", "store", "item"], "column", [60.0], src=MK, where=uid(TOTAL3), field="qty"),
    ]
    with open(os.path.join(HERE, "hierarchy_sql.json"), "w") as fh:
        json.dump({"tables": TABLES, "pins": pins}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
