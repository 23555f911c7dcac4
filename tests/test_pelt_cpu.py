"""CPU: the two restatements of the reference's PELT (tests/pelt_ref.py) against each other and against the answers of the unit tests
of changepoint.rs, and the two properties that make the GPU comparison of tests/test_gpu_pelt.py discriminating: the tie family
changes its changepoints under another tie rule, and the noise family changes the bits of its cost under another summation.  Then
what the C ABI shows without a GPU: the NULL-pointer error of the single entry, the new symbols, the struct layout."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import pelt_cases as K
import pelt_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

def _same(a, b):
    return a[0] == b[0] and R.bits(a[1]) == R.bits(b[1])


def test_rust_unit_test_answers():
    """changepoint.rs tests: the series and what both restatements give for them."""
    for name, v, ms, cps, cost in K.RUST_UNIT:
        for detect in (R.literal, R.fast):
            got = detect(v, ms, 0.0)
            assert got[0] == cps and got[1] == cost, (name, detect.__name__, got)
    assert R.bits(R.literal(K.RUST_UNIT[0][1], 5, 0.0)[1]) == R.bits(2.0 * math.log(100.0))     # f[n] = pen: one changepoint, exact segments


@pytest.mark.parametrize("family", ["b", "c", "d"])
def test_the_two_restatements_agree_bit_for_bit(family):
    """Every case of the family, the lengths around the 256-lane edge and 300 included: there the GPU tests rest on `fast` alone."""
    cases = getattr(K, "family_" + family)()
    assert len(cases) >= 20 and (family == "d" or max(len(v) for _, v, _, _ in cases) == 300)
    for name, v, ms, pen in cases:
        assert _same(R.literal(v, ms, pen), R.fast(v, ms, pen)), name


def test_size_and_penalty_rules():
    v = K.noise_series(np.random.default_rng(3), 40)
    assert R.literal(v, 0, 0.0) == R.literal(v, 1, 0.0) == R.literal(v, -3, 0.0)                 # min_size.max(1)
    assert R.literal(v, 2 ** 31 - 1, 0.0) == ([], 0.0)
    assert R.literal(v[:3], 2, 0.0) == ([], 0.0) and R.literal(v[:4], 2, 0.0) != ([], 0.0)       # n < 2 ms
    auto = R.literal(v, 2, 0.0)
    assert _same(auto, R.literal(v, 2, float("nan"))) and _same(auto, R.literal(v, 2, -1.0))     # `if penalty > 0.0`
    assert _same(auto, R.literal(v, 2, 2.0 * math.log(40.0)))
    assert R.literal(v, 2, 1e300)[0] == []
    for n in (0, 1):
        assert R.literal(v[:n], 1, 0.0) == ([], 0.0)
    # a NaN among the values: candidates over it are NaN and never taken; f[n] itself is +inf when no candidate is finite
    w = v.copy()
    w[0] = float("nan")
    cps, cost = R.literal(w, 2, 0.0)
    assert cost == float("inf") and cps == []


def test_tie_family_changes_under_a_last_minimum_rule():
    """Another tie rule is visible in the changepoints of family (c), and often: of 4,000 random tie series of 6-12 rows 488 changed
    when this was written."""
    changed = sum(R.fast(v, ms, pen)[0] != R.fast(v, ms, pen, rule="last")[0] for _, v, ms, pen in K.family_c())
    assert changed >= 10, changed
    many = sum(R.fast(v, ms, pen)[0] != R.fast(v, ms, pen, rule="last")[0] for v, ms, pen in K.random_ties(4000))
    assert many >= 200, many


def test_noise_family_changes_under_prefix_sum_costs():
    """Sum of squares minus squared sum over n, from prefix sums, changes the bits of the cost of EVERY case of family (b)."""
    cases = K.family_b()
    assert len(cases) == 60
    for name, v, ms, pen in cases:
        assert R.bits(R.fast(v, ms, pen)[1]) != R.bits(R.fast(v, ms, pen, cost="prefix")[1]), name


def test_case_names_are_unique():
    """The GPU tests keep one reference per (name, setting)."""
    names = [c[0] for c in K.small_families() + K.family_e()]
    assert len(set(names)) == len(names)


def test_long_case_leaves_few_candidates():
    """Family (e): one row above the LDS tile; min_size 900 leaves candidates only for tau = 0 and the last 250 t*."""
    (name, v, ms, pen), = K.family_e()
    assert len(v) == K.TILE + 1 and len(v) - 2 * ms + 1 == 250


def test_scalar_mirror_of_the_restatement():
    assert R.scalar(None) is None and R.scalar([1.0]) is None and R.scalar([None, 1.0, None]) is None
    v = [1.0, 1.0, None, 1.0, 1.0, 10.0, None, 10.0, 10.0, 10.0]
    assert R.scalar(v) == {"changepoints": [4], "n_changepoints": 1, "cost": 4.1588830833596715}


def test_single_entry_null_pointers_and_symbols(hiplib):
    L = hiplib.load()
    for sym in ("anofox_ts_detect_changepoints", "anofox_free_changepoint_result", "anofox_hip_pelt_batch", "anofox_hip_pelt_device"):
        assert sym in hiplib.EXPORTED_SYMBOLS and hasattr(L, sym), sym
    res = hiplib.ChangepointResult()
    y = np.zeros(8)
    for values, out in ((None, C.byref(res)), (y.ctypes.data, None)):
        err = hiplib.AnofoxError()
        assert not L.anofox_ts_detect_changepoints(values, 8, 2, 0.0, out, C.byref(err))
        assert err.code == hiplib.NULL_POINTER and err.message == b"Null pointer argument"
    assert not L.anofox_ts_detect_changepoints(None, 8, 2, 0.0, None, None)          # a NULL error struct is allowed
    L.anofox_free_changepoint_result(None)
    L.anofox_free_changepoint_result(C.byref(res))
    err = hiplib.AnofoxError()
    assert not L.anofox_hip_pelt_device(None, 64, None, 1, 8, 2, 0.0, None, None, None, None, C.byref(err)) and err.code == hiplib.NULL_POINTER
    err = hiplib.AnofoxError()
    assert not L.anofox_hip_pelt_batch(None, None, None, 1, 2, 0.0, None, None, None, None, C.byref(err)) and err.code == hiplib.NULL_POINTER


def test_changepoint_result_layout():
    """ChangepointResult as gcc lays out include/anofox_fcst_hip.h (the reference's layout: pointer, size_t, double) and as lib.py
    mirrors it."""
    from anofox_forecast_amd import lib
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "anofox_fcst_hip.h"
int main(void) {
    printf("%zu %zu %zu %zu\n", sizeof(ChangepointResult), offsetof(ChangepointResult, changepoints),
           offsetof(ChangepointResult, n_changepoints), offsetof(ChangepointResult, cost));
    return 0;
}
'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "layout.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "layout")
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        out = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert out == [24, 0, 8, 16]
    T = lib.ChangepointResult
    assert [C.sizeof(T), T.changepoints.offset, T.n_changepoints.offset, T.cost.offset] == out
