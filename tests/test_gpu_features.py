"""GPU: the feature entries (anofox_ts_features, anofox_hip_features_batch, anofox_hip_features_device), device.features_block and
the mirrors of api.py against the restatement tests/features_ref.py.

The contract: equality of bits -- up to the sign of a zero and the payload of a NaN -- for every count, flag,
location, order statistic and in-order sum, for the presence bits and the status; 16 x the measured noise of ln or sin / cos for
the figures that pass through them (tests/features_cases.py measures it per series; tests/test_features_cpu.py checks the
measurements).  Every entry gives the same bits as every other, on every run."""
import ctypes as C
import math
import random

import numpy as np
import pytest

import features_cases as FC
import features_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
ISENT = -555
PAD = 12345.0
NAMES = R.SORTED_NAMES

# the rows each kernel writes (csrc/features.hip)
_SORT = {"median", "quantile_0.1", "quantile_0.25", "quantile_0.75", "quantile_0.9", "count_unique", "ratio_value_number_to_length",
         "has_duplicate", "percentage_of_reoccurring_datapoints_to_all_datapoints", "percentage_of_reoccurring_values_to_all_values",
         "sum_of_reoccurring_values", "sum_of_reoccurring_datapoints"}
_SCAN = {"count_above_mean", "count_below_mean", "percentage_above_mean", "zero_crossing_rate", "longest_strike_above_mean",
         "longest_strike_below_mean", "number_peaks", "number_peaks_threshold_1", "number_peaks_threshold_2", "first_location_of_maximum",
         "last_location_of_maximum", "first_location_of_minimum", "last_location_of_minimum", "has_duplicate_max", "has_duplicate_min",
         "ratio_beyond_r_sigma_1", "ratio_beyond_r_sigma_2", "ratio_beyond_r_sigma_3", "benford_correlation", "binned_entropy",
         "permutation_entropy", "lempel_ziv_complexity"}
_MATCH = {"sample_entropy", "approximate_entropy"}
_DFT = set(R.TRIG_FEATURES)
KERNEL_ROWS = {"sort": _SORT, "scan": _SCAN, "match": _MATCH, "dft": _DFT,
               "chains": set(NAMES) - _SORT - _SCAN - _MATCH - _DFT}


@pytest.fixture(scope="module")
def api(hiplib):
    import torch
    assert torch.cuda.is_available()
    hiplib.load()
    from anofox_forecast_amd import api as A
    return A


def _device(lib, batch, families=None, extra_cols=37, t_extra=0):
    """anofox_hip_features_families_device on torch tensors; the outputs start as a sentinel.  Returns (fp [117 x ld], int [3 x ld])."""
    import torch
    L = lib.load()
    dev = "cuda:0"
    n = len(batch)
    T = max(1, max(len(s) for s in batch)) + t_extra
    ld = (n + extra_cols + 63) // 64 * 64
    y = np.full((T, ld), PAD)
    v = np.ones((T, ld), dtype=np.uint8)
    any_null = False
    for i, s in enumerate(batch):
        vals, ok = FC.split(s)
        y[:len(s), i] = vals
        v[:len(s), i] = ok
        any_null = any_null or not all(ok)
    lens = torch.from_numpy(np.array([len(s) for s in batch], dtype=np.int32)).to(dev)
    yd = torch.from_numpy(y).to(dev)
    vd = torch.from_numpy(v).to(dev) if any_null else None
    fp = torch.full((lib.N_FEATURES, ld), SENTINEL, dtype=torch.float64, device=dev)
    it = torch.full((3, ld), ISENT, dtype=torch.int64, device=dev)
    mask = sum(1 << lib.FEATURES_FAMILIES.index(f) for f in families) if families is not None else 31
    err = lib.AnofoxError()
    torch.cuda.synchronize()
    ok = L.anofox_hip_features_families_device(yd.data_ptr(), None if vd is None else vd.data_ptr(), ld, lens.data_ptr(), n, T, mask,
                                               fp.data_ptr(), it.data_ptr(), None, C.byref(err))
    assert ok, err.message
    return fp.cpu().numpy(), it.cpu().numpy()


def _present(words):
    return {NAMES[i] for i in range(len(NAMES)) if (int(words[i // 64]) >> (i % 64)) & 1}


def _check_device(got, batch, where="", rows=None):
    fp, it = got
    n = len(batch)
    bad = []
    for i, s in enumerate(batch):
        if rows is None or "length" in rows:
            words = [int(it[0, i]) & (2 ** 64 - 1), int(it[1, i]) & (2 ** 64 - 1)]
            present, status = _present(words), int(it[2, i])
        else:                                                     # a kernel alone that does not write them
            assert (it[:, i] == ISENT).all()
            want = FC.expected(s)
            present, status = set(want["features"]), want["status"]
        values = {name: fp[k, i] for k, name in enumerate(NAMES)}
        if rows is not None:
            want = FC.expected(s)
            for name in NAMES:
                if name not in rows:
                    assert values[name] == SENTINEL, (where, name, "written by another kernel's launch")
                    values[name] = want["features"].get(name, math.nan)
        bad += FC.check(values, present, status, s, f"{where} series {i} n={len(s)}")
    assert not bad, bad[:8]
    assert (fp[:, n:] == SENTINEL).all() and (it[:, n:] == ISENT).all()        # ld > n_series: the other columns are untouched


def _family_batch(family):
    return [FC.series(family, n) for n in FC.SHORT_LENGTHS]


@pytest.mark.parametrize("family", list(FC.FAMILIES))
def test_families_at_every_short_length(hiplib, family):
    """One ragged block per family: the lengths 1 .. 257, ld > n_series, the padding columns untouched."""
    batch = _family_batch(family)
    _check_device(_device(hiplib, batch), batch, family)


@pytest.mark.parametrize("case", FC.long_cases(), ids=lambda c: f"{c[0]}-{c[1]}")
def test_tile_edge_and_workspace_route(hiplib, case):
    """2,047 and 2,048 rows fill the LDS tile, 2,049 take the workspace route; a short series rides in the same block."""
    batch = [FC.series(*case), FC.series("walk", 65)]
    _check_device(_device(hiplib, batch), batch, str(case))


@pytest.mark.parametrize("kernel", ["chains", "sort", "scan", "match", "dft"])
def test_each_kernel_alone(hiplib, kernel):
    """A launch of one family writes its own rows and nothing else, and they are right without the other kernels."""
    batch = [FC.series(f, n) for f, n in (("walk", 257), ("ties", 65), ("nulls", 64), ("nan", 21), ("inf", 20), ("constant", 12),
                                           ("sum_order", 63), ("decades", 19), ("monotone", 5), ("alternating", 2), ("walk", 1))]
    _check_device(_device(hiplib, batch, families=[kernel]), batch, kernel, rows=KERNEL_ROWS[kernel])
    assert sum(len(r) for r in KERNEL_ROWS.values()) == 117


def test_one_series_alone_and_length_above_t_rows_is_cut(hiplib):
    s = FC.series("walk", 21)
    _check_device(_device(hiplib, [s], extra_cols=0), [s], "alone")
    import torch
    from anofox_forecast_amd import device
    full = FC.series("walk", 65)
    y = torch.full((21, 64), PAD, dtype=torch.float64, device="cuda:0")
    y[:, 0] = torch.tensor(s, dtype=torch.float64)
    lens = torch.tensor([len(full)] + [0] * 63, dtype=torch.int32, device="cuda:0")              # longer than the block: cut to 21 rows
    r = device.features_block(y, lens, n_series=1)
    fp, it = r["features"].cpu().numpy(), r["figures"].cpu().numpy()
    bad = FC.check({name: fp[k, 0] for k, name in enumerate(NAMES)}, _present([int(it[0, 0]) & (2 ** 64 - 1), int(it[1, 0])]), it[2, 0], s)
    assert not bad, bad
    assert np.isnan(fp[:, 1:]).all() and (it[:, 1:] == -1).all()


def _cycle_batch(count):
    pool = [FC.series(f, n) for f in FC.FAMILIES for n in (1, 2, 3, 5, 7, 12, 21, 64, 65)]
    return [pool[i % len(pool)] for i in range(count)]


def test_three_hundred_series_through_the_batch_entry(hiplib, api):
    batch = _cycle_batch(300)
    r = api.features_batch([np.array(FC.split(s)[0]) for s in batch], [FC.split(s)[1] for s in batch])
    assert r["names"] == NAMES and r["features"].shape == (300, 117)
    bad = []
    for i, s in enumerate(batch):
        present = {NAMES[k] for k in np.nonzero(r["present"][i])[0]}
        bad += FC.check(dict(zip(NAMES, r["features"][i])), present, r["status"][i], s, f"batch series {i}")
    assert not bad, bad[:8]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_same_bits_on_two_runs_and_through_every_entry(hiplib, api):
    batch = [FC.series(f, n) for f, n in (("walk", 65), ("ties", 21), ("decades", 64), ("sum_order", 257), ("inf", 12), ("nan", 7),
                                           ("constant", 3), ("monotone", 1), ("alternating", 11), ("walk", 256))]
    fp1, it1 = _device(hiplib, batch)
    fp2, it2 = _device(hiplib, batch, extra_cols=100, t_extra=3)
    n = len(batch)
    assert (_bits(fp1[:, :n]) == _bits(fp2[:, :n])).all() and (it1[:, :n] == it2[:, :n]).all()
    r = api.features_batch([np.array(s) for s in batch])
    assert (_bits(r["features"]) == _bits(fp1[:, :n].T)).all()
    assert (r["status"] == it1[2, :n]).all()
    for i, s in enumerate(batch):
        if it1[2, i] == hiplib.FEATURES_NAN:
            with pytest.raises(api.InvalidInputException, match="Invalid input: a value is NaN"):
                api.ts_features_single(s)
            continue
        single = api.ts_features_single(s)
        assert list(single) == [name for k, name in enumerate(NAMES) if r["present"][i, k]]      # only what the source inserts, sorted
        assert all(_bits(single[name]) == _bits(fp1[NAMES.index(name), i]) for name in single)
    # the mirror: one group per series, rows in time order
    cols = api.ts_features_columns()
    assert list(cols) == list(R.DUMMY_COLUMNS) and len(cols) == 116
    group = [i for i, s in enumerate(batch) for _ in s]
    date = np.array([t for s in batch for t in range(len(s))], dtype=np.int64)
    value = [x for s in batch for x in s]
    by = api.ts_features_by(group, date, value)
    assert by["id"] == list(range(n))
    for i in range(n):
        for name in cols:
            k = NAMES.index(name)
            want = fp1[k, i] if r["present"][i, k] else math.nan
            assert R.same(by[name][i], want) and (want != want or _bits(by[name][i]) == _bits(want)), (i, name)


def test_ts_features_by_against_the_restatement(api):
    """The operator's rules: rows in any order are sorted by (timestamp, value), a NULL value is NaN, a NULL date drops the row, the
    groups come in first-arrival order, 116 columns."""
    rng = random.Random(5)
    rows = []
    for g, (fam, n) in enumerate((("walk", 21), ("ties", 12), ("monotone", 7), ("walk", 5), ("constant", 3), ("decades", 19))):
        for t, x in enumerate(FC.series(fam, n)):
            rows.append((f"g{g % 5}" if g < 5 else None, t // 2 if fam == "ties" else t, x))     # ties: equal timestamps, sorted by value
    rows.append(("g3", 99, None))                                                                # a NULL value: the group turns NaN
    rows.append(("g1", None, 4.0))                                                               # a NULL date: dropped
    rng.shuffle(rows)
    group, ts, value = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]
    want = R.ts_features_by(group, ts, value)
    ids, groups = R.operator_series(group, ts, value)
    got = api.ts_features_by(group, np.array([np.datetime64("NaT") if t is None else np.datetime64(t, "us") for t in ts]), value)
    assert got["id"] == want["id"] == ids and list(got)[1:] == list(R.DUMMY_COLUMNS) and len(ids) == 6
    for c in R.DUMMY_COLUMNS:
        if c not in R.LOG_FEATURES + R.TRIG_FEATURES:
            assert all(R.same(a, b) for a, b in zip(got[c], want[c])), (c, got[c], want[c])
    bad = []
    for k, s in enumerate(groups):                                # every column, with the tolerances of the series the rules built
        e = FC.expected(s)
        values = {c: got[c][k] for c in R.DUMMY_COLUMNS}
        values["autocorrelation_lag10"] = e["features"].get("autocorrelation_lag10", math.nan)       # no column of the operator
        bad += FC.check(values, set(e["features"]), e["status"], s, f"group {ids[k]}")
    assert not bad, bad[:8]
    k = ids.index("g3")
    assert got["length"][k] == 6.0 and all(math.isnan(got[c][k]) for c in R.DUMMY_COLUMNS if c != "length")


def test_agg_table_and_list(api):
    s = FC.series("walk", 21)
    ts = np.arange(21, dtype=np.int64)[::-1].copy()
    agg = api.ts_features_agg(ts, s[::-1])
    single = api.ts_features_single(s)
    assert list(agg) == list(R.DUMMY_COLUMNS) and all(_bits(agg[c]) == _bits(single[c]) for c in agg)
    short = api.ts_features_agg(np.arange(3, dtype=np.int64), [1.0, None, 2.0])               # the NULL value is dropped: two values
    assert short["length"] == 2.0 and math.isnan(short["autocorrelation_lag3"]) and math.isnan(short["fft_coefficient_5_abs"])
    assert api.ts_features_agg(np.arange(2, dtype=np.int64), [None, None]) is None
    assert api.ts_features_agg(np.arange(2, dtype=np.int64), [1.0, math.nan]) is None
    assert api.ts_features is api.ts_features_agg
    table = api.ts_features_table(ts, s[::-1])
    assert list(table) == list(R.DUMMY_COLUMNS) and all(_bits(table[c][0]) == _bits(agg[c]) for c in table)
    assert api.ts_features_list() == R.list_features()


def test_prepare_features_chain(api):
    """prepare_block -> features_block on the device equals the host route on the same series."""
    import torch
    from anofox_forecast_amd import device
    rng = random.Random(31)
    n, ld = 40, 64
    raw = []
    for i in range(n):
        body = list(FC.series(("walk", "ties", "sum_order", "monotone")[i % 4], (21, 64, 65, 12)[i % 4]))
        body[0] = body[0] if body[0] != 0.0 else 1.0
        raw.append([0.0] * rng.randrange(0, 4) + body)
    T = max(len(s) for s in raw)
    y = np.full((T, ld), PAD)
    for i, s in enumerate(raw):
        y[:len(s), i] = s
    dev = "cuda:0"
    lens = torch.tensor([len(s) for s in raw] + [0] * (ld - n), dtype=torch.int32, device=dev)
    prep = device.prepare_block(torch.from_numpy(y).to(dev), lens, None, n_series=n, trim="leading")
    r = device.features_block(prep["y"], prep["lengths"], prep["valid"], n_series=n)
    fp, it = r["features"].cpu().numpy(), r["figures"].cpu().numpy()
    trimmed = []
    for s in raw:
        k = 0
        while k < len(s) and s[k] == 0.0:
            k += 1
        trimmed.append(s[k:])
    assert [len(s) for s in trimmed] == prep["lengths"][:n].cpu().tolist()
    host = api.features_batch([np.array(s) for s in trimmed])
    assert (_bits(host["features"]) == _bits(fp[:, :n].T)).all() and (host["status"] == it[2, :n]).all() and (it[2, :n] == 0).all()
    assert np.isnan(fp[:, n:]).all() and (it[:, n:] == -1).all()
