"""ts_aggregate_hierarchy without a GPU: the restatement against the reference's recorded statements, the host-only plan entry
against a Python CSR, every limit with its message, the mirror's consistent-order test with its host fallback, and the three string
mirrors.  (The nnz limit of 2^31 - 1 plan entries would need an 8 GiB column_of table and is not exercised.)"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hierarchy_cases as HC  # noqa: E402
import hierarchy_ref as R  # noqa: E402

from anofox_forecast_amd import api, lib  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
INVALID_INPUT, NULL_POINTER = 2, 1


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "hierarchy_sql.json")) as fh:
        return json.load(fh)


def test_restatement_against_every_pin(golden):
    assert len(golden["pins"]) >= 50
    assert HC.run_pins(HC.ref_functions(), golden) == []


def test_restatement_chain_and_zero_signs():
    # ((0.0 + 1e16) + 1.0) + -1e16 is 0.0, not 1.0: the order is the table's; a lone -0.0 comes out as +0.0
    rows = R.aggregate([1, 1, 1, 2], [1e16, 1.0, -1e16, -0.0], [["a", "a", "b", "c"]])
    cells = {(u, d): v for u, d, v in rows}
    assert cells[("AGGREGATED", 1)] == 0.0 and cells[("a", 1)] == 1e16 and cells[("b", 1)] == -1e16
    assert np.signbit(cells[("c", 2)]) == False and np.signbit(cells[("AGGREGATED", 2)]) == False  # noqa: E712
    assert [r[0] for r in rows] == ["AGGREGATED", "AGGREGATED", "a", "b", "c"]
    # NULL date dropped, NULL value is 0.0 and the row exists, NULL id is "NULL"
    rows = R.aggregate([None, 5, 5], [1.0, None, 2.0], [["x", None, "x"]])
    assert rows == [("AGGREGATED", 5, 2.0), ("NULL", 5, 0.0), ("x", 5, 2.0)]


def test_block_restatement_equals_operator_restatement():
    c = HC.all_cases()["prefix"]
    T = len(c["series"][0])
    dates, values, ids = [], [], [[], [], []]
    for t in range(T):                       # a table sorted by (date, ids)
        for s, key in enumerate(c["ids"]):
            dates.append(t); values.append(float(c["series"][s][t]))
            for k in range(3):
                ids[k].append(key[k])
    rows = R.aggregate(dates, values, ids)
    cols = HC.expected("prefix")
    flat = [(c["unique_ids"][k], f + t, cols[k][2][t]) for k, (f, n, _v, _p) in enumerate(cols) for t in range(n)]
    assert [(u, d) for u, d, _ in rows] == [(u, d) for u, d, _ in flat]
    assert R.same_bits([v for *_, v in rows], [v for *_, v in flat]).all()


def test_order_of_addition_matters_in_every_family():
    shares = HC.check_order_sensitivity()
    assert set(shares) == {"widths", "masks", "nonfinite"}


# ---- anofox_hip_hierarchy_plan ----
def _plan_raw(co, sizing=False):
    L = lib.load()
    co = np.ascontiguousarray(co, dtype=np.int32)
    G, n = co.shape
    n_out, nnz, err = C.c_size_t(99), C.c_size_t(99), lib.AnofoxError()
    ok = L.anofox_hip_hierarchy_plan(co.ctypes.data, G, n, C.byref(n_out), C.byref(nnz), None, None, C.byref(err))
    if sizing or not ok:
        return ok, n_out.value, nnz.value, err
    offs = np.full(n_out.value + 1, -7, dtype=np.int32)
    memb = np.full(max(nnz.value, 1), -7, dtype=np.int32)
    ok = L.anofox_hip_hierarchy_plan(co.ctypes.data, G, n, C.byref(n_out), C.byref(nnz), offs.ctypes.data, memb.ctypes.data, C.byref(err))
    return ok, n_out.value, offs, memb[:nnz.value]


def test_plan_against_python_csr():
    co = np.array([[0, 0, 3, -1, 3, 0],          # column 0: series 0, 1, 5; column 3: series 2, 4
                   [3, -1, 3, -1, 5, 0],         # series 2 twice in column 3, series 5 twice in column 0; columns 1, 2, 4 empty
                   [-1, -1, -1, -1, -1, -1]], dtype=np.int32)
    ok, n_out, offs, memb = _plan_raw(co)
    r_out, r_offs, r_memb = R.plan(co.tolist())
    assert ok and n_out == r_out == 6
    assert offs.tolist() == r_offs == [0, 4, 4, 4, 8, 8, 9]
    assert memb.tolist() == r_memb == [0, 1, 5, 5, 0, 2, 2, 4, 4]
    ok, n_out, nnz, _ = _plan_raw(co, sizing=True)
    assert ok and (n_out, nnz) == (6, 9)
    for name in ("widths_T2_equal", "masks", "prefix"):
        c = HC.all_cases()[name]
        n2, o2, m2 = lib.hierarchy_plan(c["column_of"])
        assert n2 == c["n_out"] and o2.tolist() == c["offsets"].tolist() and m2.tolist() == c["members"].tolist()
    ok, n_out, offs, memb = _plan_raw(-np.ones((2, 4), dtype=np.int32))
    assert ok and n_out == 0 and offs.tolist() == [0] and len(memb) == 0


def test_plan_limits():
    ok, _, _, err = _plan_raw(np.array([[0, -2]], dtype=np.int32))
    assert not ok and err.code == INVALID_INPUT and b"below -1" in err.message
    ok, _, _, err = _plan_raw(np.array([[0, 2**31 - 1]], dtype=np.int32))
    assert not ok and err.code == INVALID_INPUT and b"n_out exceeds the limit of 2^31 - 1" in err.message
    L = lib.load()
    err, n_out, nnz = lib.AnofoxError(), C.c_size_t(), C.c_size_t()
    co = np.zeros(4, dtype=np.int32)
    offs = np.zeros(2, dtype=np.int32)
    assert not L.anofox_hip_hierarchy_plan(co.ctypes.data, 1, 4, C.byref(n_out), C.byref(nnz), offs.ctypes.data, None, C.byref(err))
    assert err.code == NULL_POINTER
    assert not L.anofox_hip_hierarchy_plan(co.ctypes.data, 1, 2**31, C.byref(n_out), C.byref(nnz), None, None, C.byref(err))
    assert err.code == INVALID_INPUT and b"2^31 - 1 series" in err.message


# ---- the limits of the batch entry: all found on the host, before a device is touched ----
def _batch_sizing(values, lengths, first, column_of, opts=None, struct_size=None, t_out=0, ld_out=0, out_y=None):
    L = lib.load()
    n = len(values)
    ptrs = (C.c_void_p * n)(*[v.ctypes.data for v in values])
    lens = (C.c_size_t * n)(*lengths)
    fst = np.ascontiguousarray(first, dtype=np.int64)
    co = np.ascontiguousarray(column_of, dtype=np.int32).reshape(-1, n)
    opts = opts or lib.make_hierarchy_options()
    n_out, t, ld, err = C.c_size_t(), C.c_size_t(), C.c_size_t(), lib.AnofoxError()
    ok = L.anofox_hip_hierarchy_batch(ptrs, None, None, lens, fst.ctypes.data, n, co.ctypes.data, co.shape[0], C.byref(opts),
                                      C.sizeof(opts) if struct_size is None else struct_size, t_out, ld_out, out_y, None, None, None,
                                      C.byref(n_out), C.byref(t), C.byref(ld), C.byref(err))
    return ok, (n_out.value, t.value, ld.value), err


def test_batch_sizing_call_needs_no_device():
    v = [np.arange(5.0), np.arange(3.0), np.zeros(0)]
    ok, sizes, err = _batch_sizing(v, [5, 3, 0], [10, 13, 0], [[0, 0, 0], [1, 2, 70]])
    assert ok, err.message
    assert sizes == (71, 6, 128)          # column 0 spans grid 10 .. 15; the empty series gives column 70 length 0


def test_batch_limits():
    v = [np.arange(4.0), np.arange(4.0)]
    ok, _, err = _batch_sizing(v, [1, 1], [0, 2**30], [[0, 0]])
    assert not ok and err.code == INVALID_INPUT and b"above the limit of 2^30" in err.message and b"output column 0 spans 1073741825 rows" in err.message
    ok, sizes, err = _batch_sizing(v, [1, 1], [0, 2**30 - 1], [[0, 0]])
    assert ok and sizes[1] == 2**30
    ok, _, err = _batch_sizing(v, [1, 1], [0, 2**61 + 1], [[0, 1]])
    assert not ok and err.code == INVALID_INPUT and b"outside the limit of +-2^61" in err.message
    ok, _, err = _batch_sizing(v, [2**30 + 1, 1], [0, 0], [[0, 1]])           # refused before any value is read
    assert not ok and err.code == INVALID_INPUT and b"longer than the limit of 2^30 rows" in err.message
    ok, _, err = _batch_sizing(v, [4, 4], [0, 0], [[0, -3]])
    assert not ok and err.code == INVALID_INPUT and b"below -1" in err.message
    ok, _, err = _batch_sizing(v, [4, 4], [0, 0], [[0, 2**31 - 1]])
    assert not ok and err.code == INVALID_INPUT and b"n_out exceeds the limit of 2^31 - 1" in err.message
    ok, _, err = _batch_sizing(v, [4, 4], [0, 0], [[0, 1]], struct_size=8)
    assert not ok and err.code == INVALID_INPUT and b"struct_size" in err.message
    ok, _, err = _batch_sizing(v, [4, 4], [0, 0], [[0, 1]], opts=lib.make_hierarchy_options(3))
    assert not ok and err.code == INVALID_INPUT and b"route must be 0" in err.message
    out = np.zeros((4, 64))
    ok, _, err = _batch_sizing(v, [4, 4], [0, 0], [[0, 1]], t_out=5, ld_out=64, out_y=out.ctypes.data)
    assert not ok and err.code == INVALID_INPUT and b"not what the sizing call returns" in err.message


def test_device_entry_limits_found_on_the_host():
    L = lib.load()
    opts, err = lib.make_hierarchy_options(), lib.AnofoxError()
    buf = np.zeros(64)
    p = buf.ctypes.data                       # never dereferenced: every call below is refused first
    call = lambda **k: L.anofox_hip_hierarchy_device(p, None, None, k.get("ld", 8), p, None, k.get("n", 8), k.get("t_rows", 4), p, p,
                                                     k.get("n_out", 2), k.get("nnz", 4), C.byref(opts), k.get("size", C.sizeof(opts)),
                                                     k.get("t_out", 4), p, None, k.get("ld_out", 64), p, p, None, C.byref(err))
    assert not call(size=4) and err.code == INVALID_INPUT and b"struct_size" in err.message
    assert not call(ld=4) and err.code == INVALID_INPUT and b"ld is smaller than n_series" in err.message
    assert not call(ld_out=1) and err.code == INVALID_INPUT and b"ld_out is smaller than n_out" in err.message
    assert not call(n_out=2**31) and err.code == INVALID_INPUT and b"limited to 2^31 - 1" in err.message
    assert not call(nnz=2**31) and err.code == INVALID_INPUT and b"limited to 2^31 - 1" in err.message
    assert not call(t_out=2**30 + 1) and err.code == INVALID_INPUT and b"limited to 2^30 rows" in err.message
    assert not call(t_rows=2**30 + 1) and err.code == INVALID_INPUT and b"limited to 2^30 rows" in err.message


# ---- the mirror: which tables may take the GPU route, and the host fallback ----
def _table(order):
    """(leaf, day, value) triples -> the mirror's arguments."""
    leaves = {"a": ("EU", "S1"), "b": ("EU", "S2"), "c": ("US", "S3")}
    date = np.array([f"2024-01-{d:02d}" for _l, d, _v in order], dtype="datetime64[D]")
    return date, [v for *_, v in order], [[leaves[l][0] for l, *_ in order], [leaves[l][1] for l, *_ in order]]


def _assert_equals_restatement(date, value, ids, got):
    us = [None if np.isnat(d) else int(d.astype(np.int64)) for d in date]
    want = R.aggregate(us, value, ids)
    assert list(got["unique_id"]) == [r[0] for r in want]
    assert [int(d.astype(np.int64)) for d in got["date"]] == [r[1] for r in want]
    assert R.same_bits(got["value"], [r[2] for r in want]).all()


def test_mirror_falls_back_when_dates_arrive_in_two_leaf_orders():
    order = [("a", 1, 1e16), ("b", 1, 1.0), ("c", 1, 1.0), ("c", 2, 1.0), ("b", 2, 1.0), ("a", 2, 1e16)]
    date, value, ids = _table(order)
    info = {}
    got = api.ts_aggregate_hierarchy(date, value, ids, info=info)
    assert info["route"] == "host"
    _assert_equals_restatement(date, value, ids, got)
    total = {str(d): v for u, d, v in zip(got["unique_id"], got["date"], got["value"]) if u == "AGGREGATED|AGGREGATED"}
    assert total == {"2024-01-01": 1e16, "2024-01-02": 1e16 + 2.0}       # the two days were summed in the two orders of the table


def test_mirror_falls_back_on_a_duplicated_leaf_date():
    order = [("a", 1, 1e16), ("b", 1, 1.0), ("a", 1, -1e16), ("a", 2, 3.0), ("b", 2, 0.1)]
    date, value, ids = _table(order)
    info = {}
    got = api.ts_aggregate_hierarchy(date, value, ids, info=info)
    assert info["route"] == "host"
    _assert_equals_restatement(date, value, ids, got)


def test_mirror_order_test():
    # sorted by (ids, date) and by (date, ids) -- also when a leaf misses the first date -- one numbering exists; else none
    s1, s2, s3 = ("EU", "S1"), ("EU", "S2"), ("US", "S3")
    f = api._hierarchy_leaf_order
    # (ids, date): S1 d0 d1, S2 d0 d1, S3 d0 d1 -- leaves numbered by first appearance
    assert f(np.array([0, 0, 1, 1, 2, 2]), np.array([0, 1, 0, 1, 0, 1]), [s1, s2, s3]).tolist() == [0, 1, 2]
    # (date, ids) with S1 missing on the first date: d0 S2 S3, d1 S1 S2 S3 -- first appearance S2, S3, S1 fails, the sorted keys work
    assert f(np.array([0, 1, 2, 0, 1]), np.array([0, 0, 1, 1, 1]), [s2, s3, s1]).tolist() == [1, 2, 0]
    assert f(np.array([0, 1, 1, 0]), np.array([0, 0, 1, 1]), [s1, s2]) is None          # two orders
    assert f(np.array([0, 0]), np.array([0, 0]), [s1]) is None                          # a (leaf, date) twice


def test_mirror_bind_errors_and_parameters():
    d = np.array(["2024-01-01"], dtype="datetime64[D]")
    with pytest.raises(api.InvalidInputException, match=r"ts_aggregate_hierarchy requires at least 3 columns: date_col, value_col, and at "
                                                        r"least one id_col\. Got 2 columns\."):
        api.ts_aggregate_hierarchy(d, [1.0], [])
    with pytest.raises(api.InvalidInputException, match=r"ts_combine_keys requires at least 3 columns.*Got 2 columns\."):
        api.ts_combine_keys(d, [1.0], [])
    with pytest.raises(api.InvalidInputException, match=r"ts_validate_separator requires at least 1 ID column\."):
        api.ts_validate_separator([])
    with pytest.raises(api.InvalidInputException, match="Date column must be DATE, TIMESTAMP, INTEGER, or BIGINT"):
        api.ts_aggregate_hierarchy(np.array([1.5]), [1.0], [["a"]])
    # an empty input and an input of NULL dates give no rows, with the date type kept
    got = api.ts_aggregate_hierarchy(np.array(["NaT"], dtype="datetime64[us]"), [1.0], [["a"]], date_name="ts", value_name="q")
    assert list(got) == ["unique_id", "ts", "q"] and len(got["q"]) == 0 and got["ts"].dtype == np.dtype("datetime64[us]")
    assert api.anofox_fcst_ts_aggregate_hierarchy is api.ts_aggregate_hierarchy and api.anofox_fcst_ts_split_keys is api.ts_split_keys
    assert api.anofox_fcst_ts_combine_keys is api.ts_combine_keys and api.anofox_fcst_ts_validate_separator is api.ts_validate_separator


def test_string_mirrors_against_the_golden_statements(golden):
    fns = dict(HC.ref_functions())           # the aggregate stays the restatement here: its mirror runs on the GPU
    fns.update(ts_combine_keys=api.ts_combine_keys, ts_split_keys=api.ts_split_keys, ts_validate_separator=api.ts_validate_separator)
    assert HC.run_pins(fns, golden) == []


def test_string_mirrors_against_the_restatement():
    ids = [["a|b", None, "c", "a|b"], ["x", "y::z", None, "-"]]
    for sep in ("|", "::", "-", "", "#"):
        assert list(api.ts_combine_keys([1, 2, 3, 4], [1.0] * 4, ids, {"separator": sep})["unique_id"]) == R.combine_keys(ids, sep)
        if sep:
            assert api.ts_validate_separator(ids, sep) == R.validate_separator(ids, sep)
        uids = ["a|b|c|d", "a", None, "", "a||b", "x::y"]
        for columns in (None, ["p", None, "q"], ["one"]):
            got = api.ts_split_keys(uids, np.arange(6), np.arange(6.0), sep, columns)
            names, rows, kept = R.split_keys(uids, sep, columns)
            assert list(got)[:len(names)] == names and list(got)[len(names):] == ["date", "value"]
            assert [[got[c][r] for c in names] for r in range(len(kept))] == rows
            assert got["date"].tolist() == kept
    assert api.ts_validate_separator([["STORE|001", "A|B", "ok"]])["message"] == "Separator '|' found in 2 value(s). Try: '-', '.', '::', '__', '#'"
    assert api.ts_validate_separator([["a-b"]], "-")["message"] == "Separator '-' found in 1 value(s). Try: '.', '::', '__', '#'"
