"""CPU: the restatement of the data-preparation chain (tests/dataprep_ref.py) against the reference's own statements
(tests/golden/dataprep_kats.json) through the host logic of the mirrors, with the GPU batch call replaced by the restatement;
its interpolate against the oracle's NULL fill; the stage identities; and the layouts of the new structs through ctypes."""
import ctypes as C

import numpy as np
import pytest

import dataprep_cases as DC
import dataprep_ref as R

KATS = DC.load_kats()


@pytest.fixture()
def api(monkeypatch):
    from anofox_forecast_amd import api as A
    monkeypatch.setattr(A, "prepare_batch", DC.ref_prepare_batch)
    return A


@pytest.mark.parametrize("st", KATS["statements"], ids=lambda s: s["name"])
def test_golden_statements(api, st):
    if "error" in st["expect"]:
        with pytest.raises(api.InvalidInputException, match=st["expect"]["error"].replace("(", r"\(").replace(")", r"\)")):
            DC.run_statement(api, st, KATS["tables"])
        return
    DC.check_statement(DC.run_statement(api, st, KATS["tables"]), st, KATS["tables"])


@pytest.mark.parametrize("case", KATS["unit"], ids=lambda c: c["name"])
def test_unit_statements(case):
    if case["op"] == "gaps":
        d, v = R.fill_gaps(case["dates"], case["values"], case["frequency_micros"], case["frequency_type"])
        assert d == case["expect_dates"] and v == case["expect"]
    else:
        assert R.fill_nulls(case["values"], case["op"], case.get("fill_value", 0.0)) == case["expect"]


def test_fixed_frequency_must_be_positive():
    with pytest.raises(ValueError, match="Frequency must be positive for fixed intervals"):
        R.fill_gaps([0, 5], [1.0, 2.0], 0, "FIXED")
    assert R.fill_gaps([0, 5], [1.0, 2.0], 0, "MONTHLY") == ([0, 5], [1.0, 2.0])     # the calendar types ignore the value


def test_gaps_edges():
    day = DC.US_PER_DAY
    assert R.fill_gaps([], [], day) == ([], []) and R.fill_gaps([7], [None], day) == ([7], [None])
    # truncation: 2.9 steps insert one row; rows closer than f, duplicates and descending rows insert nothing
    assert R.fill_gaps([0, 29], [1.0, 2.0], 10)[0] == [0, 10, 29]
    assert R.fill_gaps([0, 3, 3, 2], [1.0, 2.0, 3.0, 4.0], 10, sort=False)[0] == [0, 3, 3, 2]
    assert R.fill_gaps([30, 0], [1.0, 2.0], 10, sort=False)[0] == [30, 0] and R.fill_gaps([30, 0], [1.0, 2.0], 10)[0] == [0, 10, 20, 30]
    # Jan-31 to Mar-31: February's row is dated at the start of the month, the original rows keep their dates
    jan31, mar31 = 19388 * day, (19388 + 59) * day
    assert R.fill_gaps([jan31, mar31], [1.0, 2.0], 0, "MONTHLY")[0] == [jan31, 19389 * day, mar31]
    # quarter and year boundaries: 2022-12-31 -> 2023-07-01 misses Q1 and Q2; 2021-12-31 -> 2024-01-01 misses 2022 and 2023
    d = lambda s: int(np.datetime64(s, "D").astype(np.int64)) * day
    assert R.fill_gaps([d("2022-12-31"), d("2023-07-01")], [1.0, 2.0], 0, "QUARTERLY")[0] == [d("2022-12-31"), d("2023-01-01"), d("2023-04-01"),
                                                                                             d("2023-07-01")]
    assert R.fill_gaps([d("2021-12-31"), d("2024-01-01")], [1.0, 2.0], 0, "YEARLY")[0] == [d("2021-12-31"), d("2022-01-01"), d("2023-01-01"),
                                                                                          d("2024-01-01")]
    # a pre-1970 date with a negative microsecond remainder reads as 1970-01-01 (micros_to_datetime's fallback)
    odd = d("1969-03-15") - 1
    assert R.fill_gaps([odd, d("1970-04-01")], [1.0, 2.0], 0, "MONTHLY")[0] == [odd, d("1970-02-01"), d("1970-03-01"), d("1970-04-01")]
    assert R.fill_gaps([d("1969-03-15"), d("1969-06-01")], [1.0, 2.0], 0, "MONTHLY")[0] == [d("1969-03-15"), d("1969-04-01"), d("1969-05-01"),
                                                                                          d("1969-06-01")]


def test_month_start_against_numpy():
    for y in (1600, 1899, 1900, 1969, 1970, 2000, 2023, 2024, 2100, 2400):
        for m in range(1, 13):
            assert R.month_start_micros(y, m) == int(np.datetime64(f"{y:04d}-{m:02d}-01", "D").astype(np.int64)) * DC.US_PER_DAY


def test_zero_rules():
    """ts_macros.cpp:208-256: non-zero is `value != 0 AND value IS NOT NULL`."""
    nan = float("nan")
    assert R.trim_bounds([0.0, -0.0, None, 1.0, 0.0, None], "edge") == (3, 2)
    assert R.trim_bounds([0.0, nan, 0.0], "edge") == (1, 1)                 # NaN is non-zero
    assert R.trim_bounds([-0.0, 0.0, None], "leading") == (3, 0) and R.trim_bounds([-0.0, 0.0, None], "trailing") == (0, 3)
    assert R.trim_bounds([1e-300, 0.0], "edge") == (0, 1)                   # no epsilon: the macros compare with 0
    assert R.trim_bounds([1.0, 2.0], "edge") == (0, 0) and R.trim_bounds([], "edge") == (0, 0)


def test_min_max_rank_nan_above_numbers():
    nan = float("nan")
    assert R.min_max([1.0, nan, -2.0, None])[0] == -2.0 and np.isnan(R.min_max([1.0, nan, -2.0, None])[1])
    assert all(np.isnan(x) for x in R.min_max([nan, nan])) and all(np.isnan(x) for x in R.min_max([None]))
    assert R.min_max([3.0, 3.0]) == (3.0, 3.0)


@pytest.mark.parametrize("seed", range(4))
def test_interpolate_equals_oracle(oracle, seed):
    rng = np.random.default_rng(900 + seed)
    L = oracle.lib()
    for n in (1, 2, 3, 16, 17, 33, 70, 200):
        for p in (0.0, 0.2, 0.6, 0.95, 1.0):
            y = rng.normal(10.0, 3.0, n)
            ok = rng.random(n) >= p
            out = np.full(n, -1.0)
            m = oracle.validity_mask(ok)
            L.oracle_fill_nulls_interpolate(y.ctypes.data, m.ctypes.data, n, out.ctypes.data)
            ref = R.fill_nulls_interpolate(DC.to_cells(y, ok))
            assert np.array_equal(out.view(np.uint64), np.array(ref, dtype=np.float64).view(np.uint64)), (n, p)


def _seeded_series(rng, n):
    vals = rng.choice([0.0, -0.0, 1.5, -2.0, float("nan"), 4.25], size=n, p=[0.4, 0.05, 0.2, 0.15, 0.05, 0.15])
    ok = rng.random(n) > 0.3
    day = DC.US_PER_DAY
    dates = np.cumsum(rng.choice([1, 1, 1, 2, 4], size=n)) * day
    return [int(x) for x in dates], DC.to_cells(vals, ok)


@pytest.mark.parametrize("seed", range(6))
def test_stage_identities(seed):
    rng = np.random.default_rng(40 + seed)
    for n in (0, 1, 2, 5, 17, 40):
        d, v = _seeded_series(rng, n)
        # the gaps output contains every input row, in order, and only NULLs besides
        gd, gv = R.fill_gaps(d, v, DC.US_PER_DAY)
        it = iter(zip(gd, gv))
        for row in zip(d, v):
            assert any(R.same_values([row[1]], [x[1]]) and row[0] == x[0] for x in it)
        assert sum(1 for x in gv if x is None) - sum(1 for x in v if x is None) == len(gv) - len(v)
        # trim then const 0 == const 0 then trim, on the leading side (a NULL and a 0 are both not non-zero)
        a = R.prepare(d, v, trim="leading", fill="const", fill_value=0.0)
        filled = R.fill_nulls_const(v, 0.0)
        front, _ = R.trim_bounds(filled, "leading")
        assert R.same_values(a["values"], filled[front:]) and a["figures"][3] == front
        # count mode gives the lengths of the full run
        for opts in (dict(gaps=True, frequency_micros=DC.US_PER_DAY, trim="edge", fill="interpolate"), dict(trim="trailing", fill="mean")):
            full = R.prepare(d, v, t_out=10 ** 6, **opts)
            cnt = R.prepare(d, v, **opts)
            assert cnt["figures"] == full["figures"] and len(cnt["values"]) == len(full["values"])
            need = cnt["figures"][0] + cnt["figures"][2] - cnt["figures"][3] - cnt["figures"][4]
            assert need == len(full["values"])
            if need > 0:
                assert R.prepare(d, v, t_out=need - 1, **opts)["figures"][7] == 1 and R.prepare(d, v, t_out=need, **opts)["figures"][7] == 0


def test_struct_layouts(hiplib):
    lib = hiplib
    assert (C.sizeof(lib.FilledValuesResult), C.sizeof(lib.GapFillResult), C.sizeof(lib.AnofoxHipPrepOptions)) == (24, 32, 32)
    assert lib.GapFillResult.length.offset == 24 and lib.FilledValuesResult.length.offset == 16
    assert lib.AnofoxHipPrepOptions.frequency_micros.offset == 8 and lib.AnofoxHipPrepOptions.fill_value.offset == 24
    assert lib.AnofoxHipPrepared.figures.offset == 32 and C.sizeof(lib.AnofoxHipPrepared) == 112
    L = lib.load()
    for s in ("anofox_hip_prepare_device", "anofox_hip_prepare_batch", "anofox_hip_free_prepared", "anofox_ts_fill_gaps",
              "anofox_ts_fill_nulls_interpolate", "anofox_free_double_array"):
        assert s in lib.EXPORTED_SYMBOLS and hasattr(L, s)


def test_argument_errors_need_no_gpu(hiplib):
    """The checks in front of the device: NULL pointers, the frequency rule, struct_size, overlap."""
    lib = hiplib
    L = lib.load()
    err = lib.AnofoxError()
    r = lib.GapFillResult()
    y = np.zeros(4)
    d = np.arange(4, dtype=np.int64)
    assert not L.anofox_ts_fill_gaps(d.ctypes.data, y.ctypes.data, None, 4, 0, 0, C.byref(r), C.byref(err))
    assert err.code == lib.INVALID_FREQUENCY and err.message.decode() == "Frequency must be positive for fixed intervals"
    assert not L.anofox_ts_fill_gaps(None, y.ctypes.data, None, 4, 1, 0, C.byref(r), C.byref(err))
    assert err.code == lib.NULL_POINTER and err.message.decode() == "Null pointer argument"
    q = C.POINTER(C.c_double)()
    assert not L.anofox_ts_fill_nulls_mean(None, None, 4, C.byref(q), C.byref(err)) and err.code == lib.NULL_POINTER
    o = lib.make_prep_options(gaps=True, frequency_micros=1)
    one = C.c_void_p(8)                                            # never dereferenced: the argument checks come first
    args = lambda size, dates, yo: (one, None, dates, 64, one, 1, 4, C.byref(o), size, 4, yo, None, None, one, one, one, None, C.byref(err))
    assert not L.anofox_hip_prepare_device(*args(8, one, None)) and err.code == lib.INVALID_INPUT
    assert not L.anofox_hip_prepare_device(*args(C.sizeof(o), None, None)) and err.code == lib.INVALID_INPUT       # gaps without dates
    assert not L.anofox_hip_prepare_device(*args(C.sizeof(o), C.c_void_p(1 << 20), one)) and err.code == lib.INVALID_INPUT   # y_out overlaps y
    assert "overlaps" in err.message.decode()
