"""CPU: the restatement tests/quality_ref.py of the data quality figures meets every golden statement of
tests/golden/quality_kats.json and the edges of quality.rs's step functions.  No GPU and no library: this is the yardstick the GPU
entries are compared with, bit for bit, in tests/test_gpu_quality.py."""
import json
import math
import os
import random

import pytest

import quality_cases as QC
import quality_ref as R

KATS = QC.load_kats()
IMPL = QC.RefImpl()


def _q(series):
    d, status = R.data_quality(series)
    assert status == R.OK
    return d


def test_golden_file_is_what_its_script_writes(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_quality_kats", os.path.join(QC.HERE, "golden", "make_quality_kats.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.HERE = str(tmp_path)
    mod.main()
    with open(tmp_path / "quality_kats.json") as fh:
        assert json.load(fh) == KATS


@pytest.mark.parametrize("st", KATS["scalars"], ids=lambda st: f'{st["field"]}@{st["src"].split("/")[-1]}')
def test_golden_scalars(st):
    ok, value = QC.golden_scalar(IMPL, st)
    assert ok, (st["src"], value)


def test_golden_pairs_and_tables():
    for st in KATS["pairs"]:
        ok, value = QC.golden_pair(IMPL, st)
        assert ok, (st["src"], value)
    for st in KATS["table_statements"]:
        ok, value = QC.golden_table(IMPL, KATS, st)
        assert ok, (st["src"], value)


def test_worked_example():
    d = _q([1.0, 2.0, 3.0, 4.0, 5.0])
    assert d["structural_score"].hex() == "0x1.8000000000000p-1" and d["overall_score"] == 0.9375
    assert R.quartiles([5.0, 3.0, 1.0, 4.0, 2.0]) == (2.0, 4.0)
    assert R.magnitude_counts([1.0, 2.0, 3.0, 4.0, 5.0]) == (0, 0)
    assert abs(R.autocorrelation1([1.0, 2.0, 3.0, 4.0, 5.0]) - 0.4) < 1e-15
    assert 1.0 - 0.2 == 0.8                      # the penalised behavioral score is the double 0.8


def test_empty_and_all_null():
    d = _q([])
    assert all(d[f] == 0.0 for f in R.FP_FIELDS) and d["n_missing"] == 0 and d["n_gaps"] == 0 and d["is_constant"] is False
    d = _q([None] * 7)
    assert (d["structural_score"], d["temporal_score"], d["magnitude_score"], d["behavioral_score"]) == (0.0, 1.0, 0.0, 0.5)
    assert d["overall_score"] == 0.375 and d["is_constant"] is True and d["n_missing"] == 7
    assert R.scalar([]) is None and R.scalar(None) is None and R.scalar([None])["overall_score"] == 0.375


@pytest.mark.parametrize("k", [0, 1, 2, 3, 4])
def test_short_series(k):
    x = [2.0, 7.0, 3.0, 11.0][:k]
    d = _q(x + [None])
    assert d["n_missing"] == 1 and d["is_constant"] is (k < 2)
    assert d["behavioral_score"] == (0.5 if k < 3 else 1.0)
    assert d["magnitude_score"] == (0.0 if k == 0 else 1.0)
    want = 0.0 if k == 0 else float(k) / float(k + 1) * 0.7 + float(k) / 30.0 * 0.3
    assert d["structural_score"] == want
    if k:                                       # the quartile indices (k * 0.25) as usize, (k * 0.75) as usize
        srt = sorted(x)
        assert R.quartiles(x) == (srt[(0, 0, 0, 0, 1)[k]], srt[(0, 0, 1, 2, 3)[k]])


@pytest.mark.parametrize("k", [29, 30, 31])
def test_length_factor_saturates_at_thirty(k):
    d = _q([float(i % 7) for i in range(k)])
    want = 1.0 * 0.7 + (float(k) / 30.0 if k < 30 else 1.0) * 0.3
    assert d["structural_score"] == min(want, 1.0) and (d["structural_score"] < 1.0) == (k < 30)


def test_epsilon_edge_of_constancy():
    below = 1.0 - 2.0 ** -53                     # the double just below 1.0: one ulp there is 2^-53 < EPSILON
    assert _q([1.0, below])["is_constant"] is True and _q([below, 1.0, below, below])["is_constant"] is True
    assert _q([1.0, 1.0 + 2.0 ** -52])["is_constant"] is False            # |difference| == EPSILON is not below it
    assert _q([1.0, 1.0, 1.0 + 2.0 ** -52])["is_constant"] is False
    # constancy is the absolute test of the FIRST value, the variance test its own: three values inside EPSILON are 'constant' to both
    d = _q([1.0, below, 1.0, below])
    assert d["is_constant"] is True and d["behavioral_score"] == 0.0
    # large equal values are constant; large values one ulp apart are not
    assert _q([1e6] * 5)["is_constant"] is True and _q([1e6, 1e6 + 2.0 ** -33])["is_constant"] is False


def test_autocorrelation_penalty():
    rng = random.Random(7)
    high, low = QC.ar1(rng, 600, 0.99), QC.ar1(rng, 600, 0.5)
    assert abs(R.autocorrelation1(high)) > 0.95 and abs(R.autocorrelation1(low)) < 0.95
    assert _q(high)["behavioral_score"] == 0.8 and _q(low)["behavioral_score"] == 1.0
    assert _q([float(i) for i in range(200)])["behavioral_score"] == 0.8     # a ramp is its own neighbour


def test_spike_beyond_four_deviations():
    x = [10.0 + float(i % 3) for i in range(99)] + [1000.0]
    assert R.magnitude_counts(x) == (1, 1)
    assert _q(x)["magnitude_score"] == R.clamp01(1.0 - (1.0 / 100.0) * 2.0 - (1.0 / 100.0) * 3.0)
    y = [10.0 + float(i % 3) for i in range(9)] + [1000.0]       # ten values: the spike is an outlier but within 4 deviations
    assert R.magnitude_counts(y) == (1, 0)


def test_counts_with_zero_interquartile_range():
    x = [5.0] * 18 + [5.5, 4.0]                  # q1 == q3: every value off the plateau is an outlier
    assert R.quartiles(x) == (5.0, 5.0) and R.magnitude_counts(x)[0] == 2
    assert _q(x)["magnitude_score"] == R.clamp01(1.0 - (2.0 / 20.0) * 2.0 - (float(R.magnitude_counts(x)[1]) / 20.0) * 3.0)
    z = [-1.0] * 5 + [0.0] * 11 + [1.0] * 4      # sorted[5] == sorted[15] == 0: nine outliers of twenty, none beyond 4 deviations
    assert R.magnitude_counts(z) == (9, 0) and _q(z)["magnitude_score"] == 1.0 - (9.0 / 20.0) * 2.0
    # signed zeros: the order of -0.0 and +0.0 changes no count
    assert R.magnitude_counts([0.0, -0.0, -0.0, 0.0, 1.0]) == R.magnitude_counts([-0.0, 0.0, 0.0, -0.0, 1.0])


def test_infinities_follow_the_arithmetic_and_nan_is_refused():
    d = _q([1.0, math.inf, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0])
    assert d["is_constant"] is False and d["behavioral_score"] == 1.0      # variance NaN: no comparison holds
    assert d["magnitude_score"] == 0.75                                      # the infinity is an outlier, |inf - inf| > NaN is not
    assert _q([math.inf, math.inf])["is_constant"] is False                # inf - inf is NaN
    d, status = R.data_quality([1.0, math.nan, None])
    assert status == R.NAN and all(math.isnan(d[f]) for f in R.FP_FIELDS) and d["n_missing"] == 1 and d["is_constant"] is False
    assert R.scalar([1.0, math.nan]) is None


def test_sums_are_sequential():
    """Left to right from 0.0: a value that pairwise summation would keep is absorbed."""
    x = [1e16, 1.0, 1.0, 1.0, 1.0, -1e16, 3.0, 5.0]
    assert R.mean_of(x) == 1.0 and sum(x) == 8.0 and math.fsum(x) == 12.0


def test_table_functions():
    group = ["b", "a", "b", "a", "b", "c", "c"]
    date = [2, 5, 1, None, 0, 1, 0]
    value = [3.0, 1.0, 2.0, 9.0, None, math.nan, 1.0]
    t = R.table(group, date, value)
    assert t["unique_id"] == ["b", "a", "c"] and len(t) == 9
    assert t["n_missing"] == [1, 0, None] and t["overall_score"][2] is None
    assert t["overall_score"][0] == _q([None, 2.0, 3.0])["overall_score"] and t["overall_score"][1] == _q([1.0, 9.0])["overall_score"]
    s = R.summary(group, date, value)
    assert s["n_total"] == 3 and s["n_good"] + s["n_fair"] + s["n_poor"] == 2
    assert R.summary([], [], []) == {"n_total": 0, "n_good": None, "n_fair": None, "n_poor": None, "avg_score": None}
    assert R.agg([3, 1, None, 2, 1], [1.0, 5.0, 7.0, None, 2.0]) == R.scalar([2.0, 5.0, 1.0])
    assert R.agg([None], [1.0]) is None


def test_families_are_deterministic():
    a, b = QC.family_batch(), QC.family_batch()
    assert [n for n, _ in a] == [n for n, _ in b] and all(
        len(x) == len(y) and all((p is None and q is None) or QC.same_bits(p, q) for p, q in zip(x, y)) for (_, x), (_, y) in zip(a, b))
    assert [len(s) for s in QC.length_batch(False)] == list(QC.LENGTHS)
