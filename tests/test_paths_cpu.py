"""No GPU: the restatement tests/paths_ref.py against the published Philox4x32-10 answers and its own properties, the ABI of the
sample-path entries (symbols, the options struct, every argument error and its text through all three entries -- all of them come
before the device is touched), the host-only checks under sanitizers, and the independence of the restatement."""
import ctypes as C
import itertools
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import paths_cases as K
import paths_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "anofox_fcst_hip.h")
NEW_SYMBOLS = ("anofox_hip_paths_device", "anofox_hip_path_quantiles_device", "anofox_hip_paths_batch")

# counter | key -> output: the published known answers of philox4x32 with 10 rounds
PHILOX_KATS = (
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


# --------------------------------------------------------------------------------------------
# random numbers
# --------------------------------------------------------------------------------------------
def test_philox_known_answers():
    for counter, key, want in PHILOX_KATS:
        assert R.philox4x32_10(counter, key) == want
        got = R.philox_words(*counter, key[0] | (key[1] << 32))
        assert tuple(int(w) for w in got.reshape(4)) == want


def test_vector_form_equals_the_scalar_statement():
    seed = 0x0123456789ABCDEF
    for joint in (False, True):
        u = R.draws(seed, 5, 7, 9, joint)
        assert u.shape == (7, 9, 5)
        for p, k, s in itertools.product(range(7), range(9), range(5)):
            assert int(u[p, k, s]) == R.draw(seed, s, p, k, joint)


def test_counter_layout():
    assert R.counter(3, 5, 9, False) == (5, 3, 2, 0) and R.counter(3, 5, 9, True) == (5, 0, 2, 1)
    assert R.key_of(0x1122334455667788) == (0x55667788, 0x11223344)
    own, joint = R.draws(11, 4, 6, 8, False), R.draws(11, 4, 6, 8, True)
    assert (joint == joint[:, :, :1]).all()                             # joint: the same draw for every series of a (path, step)
    assert len({tuple(own[:, :, s].reshape(-1)) for s in range(4)}) == 4  # independent: every series has its own stream
    assert (own[:, :, 0] != joint[:, :, 0]).any()                        # series 0's own stream is not the joint stream (counter word 3)
    # the four steps of a block are the four words of ONE Philox call
    for k in range(8):
        assert int(own[2, k, 1]) == R.philox4x32_10((2, 1, k >> 2, 0), R.key_of(11))[k & 3]
    assert (R.draws(11, 4, 6, 8, False) == own).all() and (R.draws(12, 4, 6, 8, False) != own).any()


def test_index_rule():
    rng = np.random.default_rng(7)
    us = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF] + [int(v) for v in rng.integers(0, 2**32, size=200)]
    for u in us:
        assert R.index(u, 1) == 0
        for n in (2, 3, 1913, 1 << 20):
            assert 0 <= R.index(u, n) < n
    assert R.index(0xFFFFFFFF, 1913) == 1912 and R.index(0x80000000, 2) == 1 and R.index(0x7FFFFFFF, 2) == 0


def test_index_frequencies_pass_a_chi_square_check():
    """200,000 draws of the restatement with a fixed seed into n = 7, 50 and 1,913 cells.  The bound is the chi-square distribution's:
    with d = n - 1 degrees of freedom the statistic has mean d and variance 2d, and by the Wilson-Hilferty cube-root approximation
    its quantile at z standard deviations is d * (1 - 2 / (9d) + z * sqrt(2 / (9d)))^3.  z = 4.5 is a one-sided tail of 3.4e-6: a
    uniform generator fails one of the three checks with probability about 1e-5; the rule's own bias, n / 2^32, moves the statistic
    by less than 1e-3 at these sizes."""
    draws = R.draws(20261020, 50, 1000, 4, False).reshape(-1)           # 200,000 draws
    assert draws.size == 200000
    for n in (7, 50, 1913):
        j = ((draws * np.uint64(n)) >> np.uint64(32)).astype(np.int64)
        assert j.min() >= 0 and j.max() < n
        counts = np.bincount(j, minlength=n).astype(np.float64)
        expect = draws.size / n
        chi2 = float(((counts - expect) ** 2 / expect).sum())
        d = n - 1.0
        bound = d * (1.0 - 2.0 / (9.0 * d) + 4.5 * (2.0 / (9.0 * d)) ** 0.5) ** 3
        assert chi2 < bound, (n, chi2, bound)


# --------------------------------------------------------------------------------------------
# paths
# --------------------------------------------------------------------------------------------
def test_block_form_equals_the_scalar_statement():
    for mode, joint in itertools.product(R.MODES, (False, True)):
        pts = K.make_points(5, 9, 3)
        pools, rows = K.make_pools(5, 3, joint)
        block, status = R.paths(pts, pools, 6, mode, joint, seed=99, pool_rows=rows)
        assert block.shape == (6 * 9, 5) and (status == R.OK).all()
        for s, p in itertools.product(range(5), range(6)):
            want = R.one_path(pts[s], pools[s], len(pools[s]), 99, s, p, mode, joint)
            assert R.same_bits(block[p * 9:(p + 1) * 9, s], want).all(), (mode, joint, s, p)


def test_cumulative_order_shows_in_the_bits():
    """[1e16, 1.0, -1e16, 3.0]: the serial sum in draw order differs in bits from a reordered sum of the same draws, so an equality
    test against the restatement sees the order of the additions."""
    pool = [1e16, 1.0, -1e16, 3.0]
    pts = np.zeros((1, 8))
    block, _ = R.paths(pts, [pool], 64, "cumulative", False, seed=5)
    seen = 0
    for p in range(64):
        e = [pool[R.index(R.draw(5, 0, p, k, False), 4)] for k in range(8)]
        serial = 0.0
        for v in e:
            serial = serial + v
        assert R.same_bits(block[p * 8 + 7, 0], serial).all()
        backwards = 0.0
        for v in reversed(e):
            backwards = backwards + v
        pairwise = ((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7]))
        seen += (backwards != serial) or (pairwise != serial)
    assert seen >= 16, seen                                             # many of the 64 paths tell the orders apart


def test_independent_with_a_one_row_pool():
    pts = K.make_points(3, 5, 1)
    block, status = R.paths(pts, [[2.5], [-0.0], [1e300]], 4, "independent", False, seed=1)
    assert (status == R.OK).all()
    for p in range(4):
        assert R.same_bits(block[p * 5:(p + 1) * 5, :], (pts + np.array([[2.5], [-0.0], [1e300]])).T).all()
    cum, _ = R.paths(pts, [[2.5], [-0.0], [1e300]], 1, "cumulative", False, seed=1)
    assert cum[4, 0] == pts[0, 4] + ((((0.0 + 2.5) + 2.5) + 2.5) + 2.5 + 2.5)


def test_statuses_of_the_restatement():
    nan = float("nan")
    pts = np.ones((6, 3))
    pts[4, 1] = nan
    pools = [[1.0, 2.0], [], [1.0, nan, 3.0], [1.0, 2.0, nan], [1.0], [np.inf, -np.inf]]
    lengths = [2, 0, 3, 2, 1, 2]                                        # series 3: the NaN lies beyond the length
    block, status = R.paths(pts, pools, 8, "cumulative", False, seed=2, lengths=lengths, pool_rows=4)
    assert list(status) == [R.OK, R.EMPTY, R.NAN, R.OK, R.NAN, R.OK]
    for s in range(6):
        assert np.isnan(block[:, s]).all() == (status[s] != R.OK)
    assert np.isinf(block[:, 5]).any()                                  # +-inf are ordinary values
    _, joint = R.paths(pts, pools, 2, "cumulative", True, seed=2, lengths=[2, 0, 3, 2, 1, 2], pool_rows=2)
    assert list(joint) == [R.OK, R.RAGGED, R.RAGGED, R.OK, R.RAGGED, R.OK]
    assert R.series_status([1.0], [], 0, 0, True) == R.EMPTY             # joint with pool_rows 0: equal lengths, and empty


# --------------------------------------------------------------------------------------------
# quantiles
# --------------------------------------------------------------------------------------------
def test_quantile_levels():
    s = [1.0, 2.0, 4.0, 8.0, 16.0]
    assert R.compute_quantile(s, 0.0) == 1.0 and R.compute_quantile(s, 1.0) == 16.0 and R.compute_quantile(s, 0.5) == 4.0
    assert R.compute_quantile(s, -0.5) == 1.0 and R.compute_quantile(s, 1.5) == 16.0
    assert R.compute_quantile(s, 0.25) == 2.0                           # q * (P - 1) = 1: integral
    idx = 0.3 * 4.0                                                     # not integral
    assert R.compute_quantile(s, 0.3) == 2.0 * (1.0 - (idx - 1.0)) + 4.0 * (idx - 1.0)
    for q in (0.0, 0.3, 0.5, 1.0):
        assert R.compute_quantile([7.5], q) == 7.5                      # P = 1
    block = np.array(s[::-1]).reshape(5, 1)                             # one column, one step, unsorted
    got, status = R.quantiles(block, 1, 5, [0.0, 0.25, 0.3, 0.5, 1.0])
    assert list(got[:, 0, 0]) == [R.compute_quantile(s, q) for q in (0.0, 0.25, 0.3, 0.5, 1.0)] and list(status) == [R.OK]


def test_the_two_zeros_in_key_order():
    assert R.order_key(-0.0) < R.order_key(0.0) and R.order_key(-1.0) < R.order_key(-0.0) and R.order_key(0.0) < R.order_key(5e-324)
    assert R.order_key(float("-inf")) < R.order_key(-1e308) and R.order_key(1e308) < R.order_key(float("inf")) < R.order_key(float("nan"))
    assert R.sort_total([0.0, -0.0, 0.0, -0.0]) == [-0.0, -0.0, 0.0, 0.0]
    assert R.same_bits(R.sort_total([0.0, -0.0, 1.0, -1.0]), [-1.0, -0.0, 0.0, 1.0]).all()
    vals = np.array([0.0, -0.0, 3.5, -np.inf, np.inf, -2.0, 5e-324])
    assert R.same_bits(R.values_of(R.keys_of(vals)), vals).all()
    assert [int(k) for k in R.keys_of(vals)] == [R.order_key(v) for v in vals]
    got, _ = R.quantiles(np.array([0.0, -0.0, 0.0, -0.0]).reshape(4, 1), 1, 4, [0.0, 1.0 / 3.0, 2.0 / 3.0, 1.0])
    # the ends read a value as it is; an interpolated level is a sum, and -0.0 * 1.0 + 0.0 * 0.0 is +0.0
    assert R.same_bits(got[:, 0, 0], [-0.0, 0.0, 0.0, 0.0]).all()
    s = R.sort_total([0.0, -0.0, 0.0, -0.0])
    assert R.same_bits(got[:, 0, 0], [R.compute_quantile(s, q) for q in (0.0, 1.0 / 3.0, 2.0 / 3.0, 1.0)]).all()
    assert R.same_bits(R.compute_quantile([-0.0, -0.0, 0.0], 0.25), -0.0 * 0.5 + -0.0 * 0.5).all()       # between two negative zeros: -0.0


def test_quantile_block_equals_the_list_statement():
    rng = np.random.default_rng(4)
    P, h, n = 13, 3, 4
    block = np.round(rng.normal(size=(P * h, n)), 1)
    block[5, 2] = np.nan
    got, status = R.quantiles(block, h, P, K.LEVELS)
    assert list(status) == [R.OK, R.OK, R.NAN, R.OK] and np.isnan(got[:, 2, :]).all()
    for c in (0, 1, 3):
        for k in range(h):
            s = R.sort_total(block[k::h, c])
            assert R.same_bits(got[:, c, k], [R.compute_quantile(s, q) for q in K.LEVELS]).all()


# --------------------------------------------------------------------------------------------
# the ABI
# --------------------------------------------------------------------------------------------
def test_symbols_declared_and_exported(hiplib):
    text = open(HEADER).read()
    L = hiplib.load()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % s, text), s
        assert s in hiplib.EXPORTED_SYMBOLS and hasattr(L, s)
        assert "conformal" not in s
    assert "#define ANOFOX_HIP_PATHS_MAX_PATHS 2048" in text and hiplib.PATHS_MAX_PATHS == R.MAX_PATHS == 2048
    assert "#define ANOFOX_HIP_PATHS_MAX_LEVELS 16" in text and hiplib.PATHS_MAX_LEVELS == R.MAX_LEVELS == 16
    assert "#define ANOFOX_HIP_PATHS_MAX_POOL_ROWS 1048576" in text and hiplib.PATHS_MAX_POOL_ROWS == R.MAX_POOL_ROWS == 1 << 20
    assert hiplib.PATHS_MODES == {"cumulative": 0, "independent": 1} and list(hiplib.PATHS_MODES) == list(R.MODES)
    assert (hiplib.PATHS_OK, hiplib.PATHS_EMPTY, hiplib.PATHS_NAN, hiplib.PATHS_RAGGED) == (R.OK, R.EMPTY, R.NAN, R.RAGGED)


def test_options_struct_matches_its_ctypes_mirror(hiplib):
    src = r"""
#include <stdio.h>
#include <stddef.h>
#include "anofox_fcst_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(AnofoxHipPathsOptions), offsetof(AnofoxHipPathsOptions, mode), offsetof(AnofoxHipPathsOptions, joint),
         offsetof(AnofoxHipPathsOptions, route), offsetof(AnofoxHipPathsOptions, reserved), offsetof(AnofoxHipPathsOptions, seed));
  printf("%d %d %d %d\n", (int)ANOFOX_PATHS_CUMULATIVE, (int)ANOFOX_PATHS_INDEPENDENT, (int)ANOFOX_PATHS_ROUTE_AUTO, (int)ANOFOX_PATHS_ROUTE_LANE);
  return 0; }"""
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = subprocess.check_output([os.path.join(d, "t")]).decode().split("\n")
    cls = hiplib.AnofoxHipPathsOptions
    assert [int(v) for v in out[0].split()] == [C.sizeof(cls)] + [getattr(cls, f).offset for f in ("mode", "joint", "route", "reserved", "seed")]
    assert C.sizeof(cls) == 24
    assert [int(v) for v in out[1].split()] == [hiplib.PATHS_MODES["cumulative"], hiplib.PATHS_MODES["independent"],
                                                hiplib.PATHS_ROUTES["auto"], hiplib.PATHS_ROUTES["lane"]]
    o = hiplib.make_paths_options("independent", True, 0xFEDCBA9876543210, "lane")
    assert (o.mode, o.joint, o.route, o.reserved, o.seed) == (1, 1, 1, 0, 0xFEDCBA9876543210)
    with pytest.raises(ValueError, match="unknown mode"):
        hiplib.make_paths_options("additive")
    with pytest.raises(ValueError, match="unknown route"):
        hiplib.make_paths_options(route="tile")


def _no_device(hiplib):
    return hiplib.load().anofox_hip_device_count() <= 0


_P = np.zeros(64)                                            # never dereferenced: every call below is refused first
_LEVELS = np.array([0.1, 0.5, 0.9])


def _generate(hiplib, L, err, **k):
    p = _P.ctypes.data
    o = hiplib.make_paths_options(k.get("mode", 0), k.get("joint", 0), 1, k.get("route", 0))
    return L.anofox_hip_paths_device(k.get("point", p), 1, 64, k.get("pool", p), 1, 64, None, k.get("pool_rows", 1), k.get("n", 10), k.get("h", 1),
                                     k.get("P", 4), C.byref(o) if k.get("options", True) else None, k.get("struct_size", C.sizeof(o)),
                                     k.get("out", p), k.get("ld_out", 64), k.get("status", p), None, C.byref(err))


def _quantiles(hiplib, L, err, **k):
    p = _P.ctypes.data
    lv = np.ascontiguousarray(k.get("levels", _LEVELS), dtype=np.float64)
    return L.anofox_hip_path_quantiles_device(k.get("paths", p), k.get("ld", 64), k.get("n", 10), k.get("h", 1), k.get("P", 4),
                                              lv.ctypes.data if k.get("have_levels", True) else None, k.get("n_levels", len(lv)),
                                              k.get("out", p), k.get("status", p), None, C.byref(err))


def _batch(hiplib, L, err, **k):
    n, h = k.get("n", 2), k.get("h", 2)
    pts = np.zeros((max(n, 1), min(max(h, 1), 4)))          # (read only by a call that passes every check: h = 2)
    pools = [np.arange(3.0)] * n
    ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in pools])
    lens = (C.c_size_t * max(n, 1))(*k.get("lengths", [3] * n))
    lv = np.ascontiguousarray(k.get("levels", _LEVELS), dtype=np.float64)
    o = hiplib.make_paths_options(k.get("mode", 0), k.get("joint", 0), 1, k.get("route", 0))
    co = k.get("column_of")
    co = None if co is None else np.ascontiguousarray(co, dtype=np.int32)
    n_out, ld = C.c_size_t(), C.c_size_t()
    q = np.zeros((16, 64, 4))
    st = np.zeros(64, dtype=np.int32)
    sizing = k.get("sizing", False)
    ok = L.anofox_hip_paths_batch(pts.ctypes.data if k.get("points", True) else None, ptrs, lens, n, h, k.get("P", 4),
                                  C.byref(o) if k.get("options", True) else None, k.get("struct_size", C.sizeof(o)), lv.ctypes.data,
                                  k.get("n_levels", len(lv)), None if co is None else co.ctypes.data, 0 if co is None else co.shape[0],
                                  k.get("ld", 64), None if sizing else q.ctypes.data, st.ctypes.data, None, None, C.byref(n_out), C.byref(ld),
                                  C.byref(err))
    return ok, n_out.value, ld.value


SHARED_ERRORS = (                                             # refused alike by every entry that takes the argument
    ({"P": 0}, "n_paths is 0"),
    ({"P": 2049}, "n_paths 2049 exceeds the limit of 2048 paths per call"),
    ({"h": 0}, "horizon must be at least 1"),
    ({"P": 2048, "h": (1 << 19) + 1}, "exceeds the limit of 2^30 rows"),
)
OPTION_ERRORS = (
    ({"struct_size": 16}, "struct_size is not sizeof(AnofoxHipPathsOptions)"),
    ({"mode": 2}, "mode 2 is unknown: 0 (cumulative) or 1 (independent)"),
    ({"route": 7}, "route 7 is unknown: 0 (automatic) or 1 (lanes over series)"),
    ({"joint": 2}, "joint 2 is neither 0 nor 1"),
)
LEVEL_ERRORS = (
    ({"levels": [0.5] * 17}, "n_levels 17 exceeds the limit of 16 levels per call"),
    ({"n_levels": 0}, "n_levels is 0"),
    ({"levels": [0.1, 1.25]}, "level 1 is 1.25, outside [0, 1]"),
    ({"levels": [-0.5, 0.5]}, "level 0 is -0.5, outside [0, 1]"),
    ({"levels": [0.1, 0.2, float("nan")]}, "level 2 is"),
)


def test_device_entries_refuse_bad_arguments_without_a_device(hiplib):
    L = hiplib.load()
    err = hiplib.AnofoxError()
    for kw, text in SHARED_ERRORS + OPTION_ERRORS + (
            ({"pool_rows": (1 << 20) + 1}, "pool_rows 1048577 exceeds the limit of 2^20 = 1048576 rows per pool"),
            ({"ld_out": 9}, "ld_out is smaller than n_series")):
        assert not _generate(hiplib, L, err, **kw)
        assert err.code == hiplib.INVALID_INPUT and text in err.message.decode(), (kw, err.message)
    for kw, text in SHARED_ERRORS + LEVEL_ERRORS + (({"ld": 9}, "ld is smaller than n_cols"),):
        assert not _quantiles(hiplib, L, err, **kw)
        assert err.code == hiplib.INVALID_INPUT and text in err.message.decode(), (kw, err.message)
    for call, kw in ((_generate, {"options": False}), (_generate, {"point": None}), (_generate, {"pool": None}), (_generate, {"out": None}),
                     (_generate, {"status": None}), (_quantiles, {"paths": None}), (_quantiles, {"out": None}), (_quantiles, {"status": None}),
                     (_quantiles, {"have_levels": False})):
        assert not call(hiplib, L, err, **kw)
        assert err.code == hiplib.NULL_POINTER and err.message == b"Null pointer argument", kw
    if _no_device(hiplib):                                   # with valid arguments: the loud failure, never a CPU answer
        for call in (_generate, _quantiles):
            assert not call(hiplib, L, err)
            assert err.code == hiplib.INTERNAL_ERROR and b"no CPU fallback" in err.message


def test_batch_entry_refuses_bad_requests_and_sizes_without_a_device(hiplib):
    L = hiplib.load()
    err = hiplib.AnofoxError()
    for kw, text in SHARED_ERRORS + OPTION_ERRORS + LEVEL_ERRORS + (
            ({"lengths": [3, (1 << 20) + 1]}, "pool_rows 1048577 exceeds the limit of 2^20"),
            ({"column_of": [[0, -2]]}, "a column_of entry is below -1"),
            ({"ld": 128}, "ld is not what the sizing call returns")):
        ok, _, _ = _batch(hiplib, L, err, **kw)
        assert not ok and err.code == hiplib.INVALID_INPUT and text in err.message.decode(), (kw, err.message)
    for kw in ({"options": False}, {"points": False}):
        ok, _, _ = _batch(hiplib, L, err, **kw)
        assert not ok and err.code == hiplib.NULL_POINTER, kw
    # the sizing call needs no device: the leaves, then a plan
    assert _batch(hiplib, L, err, n=2, sizing=True) == (True, 2, 64)
    assert _batch(hiplib, L, err, n=2, sizing=True, column_of=[[0, 0], [1, 2]]) == (True, 3, 64)
    co = np.stack([np.zeros(70, dtype=np.int32), 1 + np.arange(70, dtype=np.int32)])
    assert _batch(hiplib, L, err, n=70, sizing=True, column_of=co) == (True, 71, 128)
    if _no_device(hiplib):
        ok, _, _ = _batch(hiplib, L, err)
        assert not ok and err.code == hiplib.INTERNAL_ERROR and b"no CPU fallback" in err.message


def test_python_entries_refuse_the_limits(hiplib):
    from anofox_forecast_amd import api
    pts, pools = np.zeros((2, 3)), [np.arange(4.0), np.arange(4.0)]
    for kw, text in (({"n_paths": 0}, "n_paths is 0"), ({"n_paths": 2049}, "exceeds the limit of 2048 paths"),
                     ({"levels": [0.5] * 17}, "exceeds the limit of 16 levels"), ({"levels": [2.0]}, "outside [0, 1]")):
        args = {"levels": [0.1, 0.9], "n_paths": 8}
        args.update(kw)
        res, err = api.paths_batch(pts, pools, **args)
        assert not err["ok"] and err["code"] == hiplib.INVALID_INPUT and text in err["message"], (kw, err)
    with pytest.raises(ValueError, match="unknown mode"):
        api.paths_batch(pts, pools, [0.5], mode="additive")
    res, err = api.paths_batch(np.zeros((2, 3)), [np.zeros(1 << 20), np.zeros((1 << 20) + 1)], [0.5], n_paths=2)
    assert not err["ok"] and "exceeds the limit of 2^20" in err["message"]
    if _no_device(hiplib):
        res, err = api.paths_batch(pts, pools, [0.1, 0.9], n_paths=8)
        assert not err["ok"] and err["code"] == hiplib.INTERNAL_ERROR and "no CPU fallback" in err["message"]
        assert np.isnan(res["quantiles"]).all() and res["quantiles"].shape == (2, 2, 3)


# --------------------------------------------------------------------------------------------
# the host-only logic under sanitizers, and the independence of the restatement
# --------------------------------------------------------------------------------------------
def test_host_paths_plan_under_sanitizers():
    """csrc/host_paths_plan.hpp -- every argument check of the three entries and the batch entry's shapes -- compiled on its own (no
    HIP) and run under ASan + UBSan (tests/c_abi/paths_san.cpp)."""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "paths_san")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               os.path.join(ROOT, "tests", "c_abi", "paths_san.cpp"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("paths_san: ok"), (r.stdout, r.stderr[-3000:])


def test_the_product_never_imports_the_restatement():
    pkg = os.path.join(ROOT, "anofox-forecast_amd")
    for base, _dirs, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                assert "paths_ref" not in open(os.path.join(base, f), errors="replace").read(), f
    for f in ("__graft_entry__.py", "bench.py", "anofox_forecast_amd.py"):
        assert "paths_ref" not in open(os.path.join(ROOT, f)).read(), f
    for f in ("paths_ref.py", "paths_cases.py"):
        assert "anofox_forecast_amd" not in open(os.path.join(ROOT, "tests", f)).read(), f
