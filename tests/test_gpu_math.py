"""GPU: the kernels' own elementary functions -- dm_log, dm_exp, dm_scalbn, dm_pow_step (tables in LDS), dm_pow_near1(_coef),
dm_pow_pos (csrc/det_math.hpp) and per_sincos (csrc/det_trig.hpp) -- evaluated by anofox_hip_selftest_math at the operands of
tests/math_cases.py.  The parity contract is "same bits as the checker, and the checker is accurate"; both halves are asserted here
on the functions themselves: every bit of every result equals oracle_det_eval's (a NaN may differ in payload, a zero may not
differ in sign), at workgroup sizes 64, 256 and NM_BLOCK and at n around a workgroup's edge (for pow_step that is the test of the
LDS table copy and of threads that leave early), twice; and the device results meet the caps of math_cases against the longdouble
reference without the checker in between.  tests/test_math_cpu.py holds the checker to the same caps."""
import ctypes as C

import numpy as np
import pytest

import math_cases as M

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def dev(hiplib):
    """dev(fn, x, y, block) -> results of the device entry: one array, for "sincos" the pair (sin, cos)."""
    import torch
    assert torch.cuda.is_available()
    L = hiplib.load()

    def run(fn, x, y=None, block=hiplib.NM_BLOCK):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = None if y is None else np.ascontiguousarray(y, dtype=np.float64)
        out = np.full(x.shape, np.nan)
        out2 = np.full(x.shape, np.nan) if fn == "sincos" else None
        err = hiplib.AnofoxError()
        ok = L.anofox_hip_selftest_math(hiplib.MATH_FNS[fn], x.ctypes.data, None if y is None else y.ctypes.data, x.size, int(block),
                                        out.ctypes.data, None if out2 is None else out2.ctypes.data, C.byref(err))
        assert ok, (fn, x.size, block, err.code, err.message)
        return (out, out2) if fn == "sincos" else (out,)

    return run


@pytest.fixture(scope="module")
def full(dev, hiplib):
    """The device's results on the whole list of a function at the fit kernels' workgroup size: computed once, shared."""
    cache = {}

    def get(fn):
        if fn not in cache:
            x, y = M.cases(fn)
            cache[fn] = dev(fn, x, y, hiplib.NM_BLOCK)
            for a in cache[fn]:
                a.setflags(write=False)
        return cache[fn]

    return get


def _assert_same(fn, got, want, x, y, what):
    for g, w in zip(got, want):
        same = M.same_bits(g, w)
        if not same.all():
            i = int(np.argmin(same))
            raise AssertionError(f"{fn} {what}: {int((~same).sum())} of {same.size} results differ; first at operand {i}: x = {float(x[i]).hex()}"
                                 + (f", y = {float(y[i]).hex()}" if y is not None else "") + f": {float(g[i]).hex()} against {float(w[i]).hex()}")


@pytest.mark.parametrize("fn", M.FNS)
def test_device_function_has_the_checkers_bits(dev, full, hiplib, oracle, fn):
    """0 differing bits between dm_* / per_sincos and det_* at every operand, at each workgroup size."""
    x, y = M.cases(fn)
    want = oracle.det_eval(fn, x, y)
    want = want if isinstance(want, tuple) else (want,)
    _assert_same(fn, full(fn), want, x, y, f"device against checker, {hiplib.NM_BLOCK} threads")
    for block in (64, 256):
        _assert_same(fn, dev(fn, x, y, block), want, x, y, f"device against checker, {block} threads")


@pytest.mark.parametrize("fn", M.FNS)
def test_launch_shape_does_not_move_a_bit(dev, full, hiplib, fn):
    """The same operands at n = 1, 63, 64, 65, one workgroup + 1 and at a window that does not start at the list's head, for each
    workgroup size: a result depends on its operand alone.  For pow_step the last workgroup holds threads past n, which fill the
    LDS tables and leave: the threads that stay must read whole tables."""
    x, y = M.cases(fn)
    ref = full(fn)
    for block in (64, 256, hiplib.NM_BLOCK):
        for n in (1, 63, 64, 65, block + 1):
            n = min(n, x.size)
            last = x.size - n
            for lo in sorted({0, last, min(1000 + block // 2, last)}):
                sl = slice(lo, lo + n)
                got = dev(fn, x[sl], None if y is None else y[sl], block)
                _assert_same(fn, got, tuple(r[sl] for r in ref), x[sl], None if y is None else y[sl], f"n = {n} from {lo}, {block} threads")


@pytest.mark.parametrize("fn", M.FNS)
def test_device_function_meets_the_caps_without_the_checker(full, fn):
    """The accuracy and the exact cases of math_cases, asserted on the device's results against the longdouble reference."""
    M.check_exact(fn, *full(fn))
    M.check_caps(fn, *full(fn))


@pytest.mark.parametrize("fn", M.FNS)
def test_two_calls_give_the_same_bits(dev, full, fn):
    x, y = M.cases(fn)
    _assert_same(fn, dev(fn, x, y), full(fn), x, y, "second call against first")


def test_entry_runs_nothing_for_no_operands_and_takes_a_null_error(hiplib, dev):
    """n = 0 is a success that touches nothing; err may be NULL.  (The refusals need no GPU: tests/test_math_cpu.py.)"""
    L = hiplib.load()
    x, out = np.array([1.0, 2.0]), np.full(2, -7.0)
    err = hiplib.AnofoxError()
    assert L.anofox_hip_selftest_math(0, None, None, 0, 64, None, None, C.byref(err))
    assert L.anofox_hip_selftest_math(0, x.ctypes.data, None, 0, 256, out.ctypes.data, None, C.byref(err)) and np.all(out == -7.0)
    assert L.anofox_hip_selftest_math(0, x.ctypes.data, None, 2, 64, out.ctypes.data, None, None)
    assert out[0] == 0.0 and abs(out[1] - np.log(2.0)) < 1e-15
