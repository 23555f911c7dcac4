"""Operands, reference and error caps of the elementary-function tests (test_math_cpu.py, test_gpu_math.py).

The functions are the checker's det_log / det_exp / det_scalbn / det_pow_step / det_pow_near1 / det_pow_pos (oracle/det_math.h) and
det_sincos (oracle/det_trig.h), and their device twins dm_* (csrc/det_math.hpp) and per_sincos (csrc/det_trig.hpp).  The operands
are seeded and generated, at most about 2e5 per function: an edge list per function (every literal threshold of the code with both
neighbours, every branch of the exponent arithmetic, the special values) plus random samples of each documented domain.  The
reference is numpy longdouble (x87 extended: 64-bit significand, a resolution of 2^-11 of a double's ulp); require_longdouble()
fails loudly where longdouble is a plain double and the comparison would pass vacuously.

The caps are stated in ulps of the reference (the ulp floored at 2^-1074), per function and per domain.  Each constant below sits
beside the worst value measured on THIS operand list against the longdouble reference and the operand where it occurs;
`python tests/math_cases.py` prints those figures again.
"""
import functools

import numpy as np

FNS = ("log", "exp", "scalbn", "pow_step", "pow_near1", "pow_pos", "sincos")

# ---- caps -----------------------------------------------------------------------------------------------------------------------
# log, exp, pow_near1: the code's own claim, below one ulp.
CAP_LOG = 1.0            # measured 0.8184 ulp at x = 0x1.670b6625420edp+0
CAP_EXP = 1.0            # measured 0.8486 ulp at x = 0x1.42242fe6db3b2p+9 (normal results);
#                          0.8911 ulp of 2^-1074 at x = -0x1.6262aa1ee5b02p+9 (subnormal results)
CAP_POW_NEAR1 = 1.0      # measured 0.8320 ulp at r = -0x1p-4, y = 0x1.1de6f4f37c13ep-2
# sincos: 2^-53 ABSOLUTE for every accepted argument (|x| < 2^52), and one ulp of the result for |x| < 2^24 where the result is not
# next to a zero.  Why these two limits go together: the tail of the reduction, r0 - y0, is rounded at the scale of r0 ~ k p2
# (p2 = 6.1e-17) once y0 has cancelled below it, an absolute error of up to 2^-53 k p2.  For |x| < 2^24, k p2 < 2^-30 and the error is
# below 2^-84: under 2^-5 ulp of any result of at least 2^-26 (ulp >= 2^-79).  Past 2^24 the same error reaches 2^-55 at |x| ~ 2^52
# (k p2 = 0.28): harmless in absolute terms, several ulps of a result of 1e-2 (measured 11.6 ulp of cos at the predecessor of 2^52).
CAP_SINCOS_ABS = 2.0 ** -53      # measured 0.7456 (sin, x = -0x1.7c21f95a872a1p+6) and 0.7744 (cos, x = 0x1.036642d9ada78p+22) x 2^-53
CAP_SINCOS_ULP = 1.0             # |x| < SINCOS_ULP_DOMAIN, |result| >= SINCOS_NEAR_ZERO; measured 0.7456 (sin) and 0.7744 (cos) ulp, same operands
SINCOS_NEAR_ZERO = 2.0 ** -26
SINCOS_ULP_DOMAIN = 2.0 ** 24
# Next to a zero of sin or cos (|result| < SINCOS_NEAR_ZERO) the error in ulps of the tiny result has NO cap.  What is asserted is
# that the worst case EXCEEDS one ulp for as long as the reduction stays as it is: a repair of the reduction then shows up as a
# change, and an operand list without the k pi/2 points does not pass for a test of them.
# Measured: sin 3480.5 ulp at x = -0x1.169f35e214714p+22, cos 148593.9 ulp at x = 0x1.9eb7148f354d6p+20 (the nearest double to 1082091 pi/2).
SINCOS_NEAR_ZERO_EXCEEDS = 1.0
# pow_step, pow_pos: B (1 + |y ln x|) ulp.  The error grows with |y ln x| because t = y * ln x is rounded once, as one double: half
# an ulp of t is up to |t| 2^-53 absolute in the exponent, which is |t| / 2 to |t| ulps of the result.  B is the worst
# error / (1 + |y ln x|) measured on this list, times 1.25 (the margin covers the reference's own 2^-11 ulp resolution and a
# platform whose longdouble functions round differently).  A B above 4 would mean that something other than the single rounding
# of t is wrong: two half-ulp errors at the scale of t, times the factor <= 2 between relative error and ulps, bound it at 4.
B_POW_STEP = 1.25 * 2.6908   # measured 2.6908 at x = 0x1.8659eb9cfcda2p+776, y = 0x1.f7068186559d7p-1, where the error is 1425.8 ulp;
#                              on [1/2, 2] the worst error is 2.134 ulp at x = 0x1.ef5efcfd85d72p+0, y = 0x1.ff53967c7cdd5p-1
B_POW_POS = 1.25 * 1.6842    # measured 1.6842 at x = 0x1.62ff8f822d047p-2, y = 0x1.1af0aebfb6256p+5 (worst error 601.5 ulp at x = 2^100,
#                              y = 0x1.e996885e000a0p+2)
B_LIMIT = 4.0


def require_longdouble():
    assert np.finfo(np.longdouble).nmant >= 63, "numpy longdouble has no more precision than float64 here: the reference would be vacuous"


def _bits(u):
    return np.asarray(u, dtype=np.uint64).view(np.float64)


def _neigh(v):
    v = np.float64(v)
    return [np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)]


def _rand_mant(rng, n):
    """n doubles in [1, 2) with random 52-bit significands."""
    return _bits(rng.integers(0, 1 << 52, n, dtype=np.uint64) | np.uint64(0x3ff0000000000000))


# ---- operands -------------------------------------------------------------------------------------------------------------------
LOG_SPECIAL = np.array([0.0, -0.0, -1.0, np.nan, np.inf, -np.inf])
EXP_THRESHOLDS = (709.782712893383973096, -745.13321910194110842, 0.34657359027997264, 3.725290298461914e-09)
EXP_SPECIAL = np.array([0.0, -0.0, np.nan, np.inf, -np.inf])
POW_STEP_Y = np.array([1.0, 2.0 ** -20, 0.8, 0.85, 0.9, 0.95, 0.98])
SINCOS_SPECIAL = np.array([0.0, -0.0, 2.0 ** -100, -2.0 ** -100, 2.0 ** 52, -2.0 ** 52, np.nextafter(2.0 ** 52, 0.0),
                           -np.nextafter(2.0 ** 52, 0.0), np.inf, -np.inf, np.nan])


# the worst operands of a 2e6-point search per domain against binary128 (the survey behind these tests): kept as edge cases
_H = float.fromhex
WORST_KNOWN = {
    "log": ([_H("0x1.670b6625420edp+0")], None),
    "exp": ([_H("0x1.42242fe6db3b2p+9"), _H("-0x1.6262aa1ee5b02p+9")], None),
    "pow_step": ([_H("0x1.e25e070fb600cp+0"), _H("0x1.ef5efcfd85d72p+0"), _H("0x1.8659eb9cfcda2p+776")],
                 [_H("0x1.df688a45c2364p-1"), _H("0x1.ff53967c7cdd5p-1"), _H("0x1.f7068186559d7p-1")]),
    "pow_near1": ([-2.0 ** -4], [_H("0x1.1de6f4f37c13ep-2")]),
    "pow_pos": ([_H("0x1.fd056ba9e6924p+1")], [_H("0x1.8199aad0f0fp+5")]),
    "sincos": ([_H("0x1.9eb7148f354d6p+20"), _H("-0x1.6c6cbc45dc8dep+6"), _H("0x1.036642d9ada78p+22")], None),
}


def _log_cases():
    rng = np.random.default_rng(20260101)
    split = int(0x3fe6a09e00000000)                                     # the mantissa split of the reduction (sqrt(2)/2)
    edge = [5e-324, *_neigh(2.0 ** -1022), *_neigh(1.0)]
    for top in (0x3fe, 0x3ff, 0x400, 0x001, 0x7fe):                      # the split at several exponents, the reduced one first
        u = (split & 0x000fffffffffffff) | (top << 52)
        edge += list(_bits([u - 1, u, u + 1]))
    x = np.concatenate([LOG_SPECIAL, edge, np.ldexp(1.0, np.arange(-1074, 1024)),
                        _bits(rng.integers(1, 0x7ff0000000000000, 60000, dtype=np.uint64)),
                        np.exp(rng.uniform(-np.log(2.0), np.log(2.0), 60000))])
    return x, None


def _exp_cases():
    rng = np.random.default_rng(20260102)
    edge = []
    for t in EXP_THRESHOLDS:
        edge += _neigh(t)
    for t in EXP_THRESHOLDS[2:]:                                        # the two thresholds on |x|: the negative side as well
        edge += _neigh(-t)
    tiny = np.ldexp(rng.uniform(1.0, 2.0, 4000), rng.integers(-40, -20, 4000)) * rng.choice([-1.0, 1.0], 4000)
    x = np.concatenate([EXP_SPECIAL, edge, rng.uniform(-745.2, -708.0, 20000), rng.uniform(709.0, 709.79, 10000),
                        rng.uniform(-1.0, 1.0, 60000), rng.uniform(-745.2, 709.8, 60000), tiny])
    return x, None


SCALBN_X = np.array([1.0, 1.5, 2.0 ** -1022, np.finfo(np.float64).max, 1.5 * 2.0 ** -1060, 5e-324, -1.5])
SCALBN_N = np.array([s * n for n in (0, 1, 52, 53, 54, 1021, 1022, 1023, 1024, 1074, 1075, 2045, 2046, 2047, 2048, 3000) for s in (1, -1)])


def _scalbn_cases():
    x, n = np.meshgrid(SCALBN_X, SCALBN_N.astype(np.float64), indexing="ij")
    return x.ravel(), n.ravel()


def _pow_step_edges():
    """(x, y): the ends of the domain, every bucket edge 1 + j/128 with its predecessor at exponents -1, 0, 1, x = 1, (4, 1/2)."""
    xs = [2.0 ** -1000, 2.0 ** 1000, 1.0, 4.0]
    for e in (-1, 0, 1):
        for j in range(128):
            m = np.ldexp(1.0 + j / 128.0, e)
            xs += [np.nextafter(m, 0.0), m]
    x, y = np.meshgrid(np.array(xs), POW_STEP_Y, indexing="ij")
    return np.concatenate([x.ravel(), [4.0]]), np.concatenate([y.ravel(), [0.5]])


def _pow_step_cases():
    rng = np.random.default_rng(20260103)
    ex, ey = _pow_step_edges()
    n_dom, n_neg, n_mid = 90000, 30000, 30000
    dom = np.ldexp(_rand_mant(rng, n_dom), rng.integers(-1000, 1000, n_dom))                # [2^-1000, 2^1000)
    neg = np.ldexp(_rand_mant(rng, n_neg), rng.integers(-1000, 0, n_neg))                   # x < 1: n is negative
    mid = np.exp(rng.uniform(-np.log(2.0), np.log(2.0), 2 * n_mid))                         # [1/2, 2]
    x = np.concatenate([ex, dom, neg, mid])
    y = np.concatenate([ey, 1.0 - rng.random(n_dom), 1.0 - rng.random(n_neg), rng.uniform(0.8, 0.98, n_mid), 1.0 - rng.random(n_mid)])
    return x, y


POW_NEAR1_R = np.array([0.0, 2.0 ** -4, -2.0 ** -4, 2.0 ** -60, -2.0 ** -60])


def _pow_near1_cases():
    rng = np.random.default_rng(20260104)
    er, ey = np.meshgrid(POW_NEAR1_R, np.array([1.0, 0.5, 2.0 ** -20, 0.9, 0.98, 1.0 / 3.0]), indexing="ij")
    n1, n2, n3 = 100000, 20000, 2000
    small = np.ldexp(rng.uniform(1.0, 2.0, n2), rng.integers(-60, -4, n2)) * rng.choice([-1.0, 1.0], n2)
    r = np.concatenate([er.ravel(), rng.uniform(-2.0 ** -4, 2.0 ** -4, n1), small, rng.uniform(-2.0 ** -4, 2.0 ** -4, n3)])
    y = np.concatenate([ey.ravel(), 1.0 - rng.random(n1), 1.0 - rng.random(n2), np.ones(n3)])
    return r, y


def _pow_pos_cases():
    rng = np.random.default_rng(20260105)
    n1, n2 = 100000, 10000
    x = np.concatenate([np.exp(rng.uniform(-np.log(4.0), np.log(4.0), n1)),
                        np.full(n2, 2.0 ** 100), np.full(n2, 2.0 ** -100),            # results that overflow (y > 10.24) and underflow (y > 10.74)
                        np.ones(200), np.exp(rng.uniform(-np.log(4.0), np.log(4.0), 200)), [0.25, 4.0, 4.0, 0.25]])
    y = np.concatenate([rng.uniform(0.0, 50.0, n1), rng.uniform(0.0, 50.0, n2), rng.uniform(0.0, 50.0, n2),
                        rng.uniform(0.0, 50.0, 200), np.zeros(200), [50.0, 50.0, 0.5, 0.5]])
    return x, y


def _sincos_cases():
    rng = np.random.default_rng(20260106)
    half_pi = np.longdouble("1.57079632679489661923132169163975144209858469968755")
    ks = np.concatenate([np.arange(-20000, 20001), rng.integers(20001, 10 ** 7, 10000), -rng.integers(20001, 10 ** 7, 10000)])
    near = (ks.astype(np.longdouble) * half_pi).astype(np.float64)      # the nearest doubles to k pi/2: every quadrant, both signs
    two_pi = -2.0 * np.pi
    phases = []
    for n in range(1, 66):                                               # the phases of a DFT, as the kernels build them: ((-2 pi) k) t / n
        k, t = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
        phases.append(((two_pi * k) * t / float(n)).ravel())
    for n in (255, 256, 257, 2047, 2048, 2049):
        idx = np.unique(np.concatenate([np.arange(0, n, max(n // 37, 1)), [1, 2, n // 4, n // 2, n - 2, n - 1]])).astype(np.float64)
        k, t = np.meshgrid(idx, idx, indexing="ij")
        phases.append(((two_pi * k) * t / float(n)).ravel())
    x = np.concatenate([SINCOS_SPECIAL, near, np.unique(np.concatenate(phases)), rng.uniform(-2.0 ** 24, 2.0 ** 24, 50000)])
    return x, None


_CASES = {"log": _log_cases, "exp": _exp_cases, "scalbn": _scalbn_cases, "pow_step": _pow_step_cases, "pow_near1": _pow_near1_cases,
          "pow_pos": _pow_pos_cases, "sincos": _sincos_cases}


@functools.lru_cache(maxsize=None)
def cases(fn):
    """(x, y) of function fn, read-only float64 arrays; y is None where the function takes one operand."""
    x, y = _CASES[fn]()
    if fn in WORST_KNOWN:
        x = np.concatenate([x, WORST_KNOWN[fn][0]])
        y = None if y is None else np.concatenate([y, WORST_KNOWN[fn][1]])
    x = np.ascontiguousarray(x, dtype=np.float64)
    x.setflags(write=False)
    if y is not None:
        y = np.ascontiguousarray(y, dtype=np.float64)
        assert y.shape == x.shape
        y.setflags(write=False)
    assert x.size <= 210000, (fn, x.size)
    return x, y


# ---- reference ------------------------------------------------------------------------------------------------------------------
def reference_at(fn, x, y=None):
    """The function in longdouble at the double operands x (, y): one array, for "sincos" the pair (sin, cos).  Operands outside the
    function's domain give whatever longdouble arithmetic gives (NaN, inf): the tests assert those cases by equality instead."""
    require_longdouble()
    lx = np.asarray(x, dtype=np.float64).astype(np.longdouble)
    ly = None if y is None else np.asarray(y, dtype=np.float64).astype(np.longdouble)
    with np.errstate(all="ignore"):
        if fn == "log":
            return np.log(lx)
        if fn == "exp":
            return np.exp(lx)
        if fn == "scalbn":
            return np.ldexp(lx, np.asarray(y, dtype=np.float64).astype(np.int64).clip(-16000, 16000).astype(np.int32))      # exact
        if fn in ("pow_step", "pow_pos"):
            return np.power(lx, ly)
        if fn == "pow_near1":
            return np.power(np.longdouble(1) + lx, ly)
        if fn == "sincos":
            return np.sin(lx), np.cos(lx)
    raise KeyError(fn)


@functools.lru_cache(maxsize=None)
def reference(fn):
    """reference_at on cases(fn), computed once and shared (read-only)."""
    x, y = cases(fn)
    r = reference_at(fn, x, y)
    for a in (r if isinstance(r, tuple) else (r,)):
        a.setflags(write=False)
    return r


def ulps(got, ref):
    """|got - ref| in ulps of a double in |ref|'s binade, the ulp floored at 2^-1074 (and capped at the largest binade's 2^971).
    An infinite `got` is exact where |ref| >= 2^1024 and counts as 2^1024, the least value that rounds to it, elsewhere.  A NaN
    `got` at a finite ref is an infinite error; NaN where ref is NaN or infinite (the tests assert those cases by equality)."""
    require_longdouble()
    ref = np.asarray(ref, dtype=np.longdouble)
    g = np.asarray(got, dtype=np.float64).astype(np.longdouble)
    big = np.ldexp(np.longdouble(1), 1024)
    with np.errstate(all="ignore"):
        over = np.isinf(g) & (np.sign(g) == np.sign(ref)) & (np.abs(ref) >= big)          # an overflow that is the correct rounding
        g = np.where(over, ref, np.where(np.isinf(g), np.sign(g) * big, g))
        _, e = np.frexp(np.abs(ref))                                     # |ref| = m 2^e, m in [1/2, 1): ulp = 2^(e - 53)
        e = np.where(ref == 0, -2000, e)
        ulp = np.ldexp(np.longdouble(1), (np.clip(e, -1021, 1024) - 53).astype(np.int32))
        out = np.abs(g - ref) / ulp
        out = np.where(np.isnan(g), np.inf, out)
        out = np.where(np.isfinite(ref), out, np.nan)
    return out


def same_bits(a, b):
    """Elementwise: the same bit pattern, or both NaN (a NaN may differ in payload; a zero may not differ in sign)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def pow_scale(x, y):
    """1 + |y ln x|, the factor of the pow_step / pow_pos cap (float64 is ample for a factor)."""
    with np.errstate(all="ignore"):
        return 1.0 + np.abs(np.asarray(y, dtype=np.float64) * np.log(np.asarray(x, dtype=np.float64)))


# ---- the figures of each function on its operand list: what the tests assert and what `python tests/math_cases.py` prints -------------
def worst(err, *operands):
    """(largest finite err, the operands there as hex strings)."""
    err = np.where(np.isnan(err), -1.0, err)
    i = int(np.argmax(err))
    return float(err[i]), tuple(float(o[i]).hex() for o in operands if o is not None)


def figures(fn, got, got2=None):
    """The measured figures of results `got` (the checker's or the device's) at cases(fn): dict name -> (value, operands)."""
    x, y = cases(fn)
    ref = reference(fn)
    out = {}
    if fn == "log":
        ok = (x > 0) & np.isfinite(x)
        out["ulp"] = worst(np.where(ok, ulps(got, ref), np.nan), x)
    elif fn == "exp":
        ok = (x >= EXP_THRESHOLDS[1]) & (x <= EXP_THRESHOLDS[0])
        err = np.where(ok, ulps(got, ref), np.nan)
        sub = np.asarray(ref < np.longdouble(2.0 ** -1022))
        out["ulp"] = worst(np.where(~sub, err, np.nan), x)
        out["ulp_subnormal"] = worst(np.where(sub, err, np.nan), x)
    elif fn == "pow_near1":
        out["ulp"] = worst(ulps(got, ref), x, y)
    elif fn in ("pow_step", "pow_pos"):
        out["B"] = worst(np.asarray(ulps(got, ref), dtype=np.float64) / pow_scale(x, y), x, y)
        out["ulp"] = worst(ulps(got, ref), x, y)
    elif fn == "sincos":
        ok = np.abs(x) < SINCOS_ULP_DOMAIN
        small = np.abs(x) < 2.0 ** 52
        for name, g, r in (("sin", got, ref[0]), ("cos", got2, ref[1])):
            err = np.where(ok, ulps(g, r), np.nan)
            nz = np.asarray(np.abs(r) < np.longdouble(SINCOS_NEAR_ZERO))
            out[name + "_ulp"] = worst(np.where(~nz, err, np.nan), x)
            out[name + "_near_zero_ulp"] = worst(np.where(nz, err, np.nan), x)
            with np.errstate(all="ignore"):
                aerr = np.abs(np.asarray(g, dtype=np.float64).astype(np.longdouble) - r)
            out[name + "_abs_2^-53"] = worst(np.where(small, np.asarray(aerr * np.longdouble(2.0 ** 53), dtype=np.float64), np.nan), x)
    return out


# ---- the assertions, shared by the CPU test (the checker's results) and the GPU test (the device's) ---------------------------------
def _show(fn, fig):
    for k, (v, at) in fig.items():
        print(f"{fn:10s} {k:22s} {v:14.4f}  at {', '.join(at)}")


def check_caps(fn, got, got2=None):
    """The caps of math_cases on results at cases(fn); shared with the GPU test.  Prints every figure before it asserts."""
    fig = figures(fn, got, got2)
    _show(fn, fig)
    if fn == "log":
        assert 0.5 < fig["ulp"][0] <= CAP_LOG, fig
    elif fn == "exp":
        assert 0.5 < fig["ulp"][0] <= CAP_EXP and 0.5 < fig["ulp_subnormal"][0] <= CAP_EXP, fig
    elif fn == "pow_near1":
        assert 0.5 < fig["ulp"][0] <= CAP_POW_NEAR1, fig
    elif fn in ("pow_step", "pow_pos"):
        b = B_POW_STEP if fn == "pow_step" else B_POW_POS
        assert b <= B_LIMIT
        assert 0.5 < fig["B"][0] <= b, fig
    elif fn == "sincos":
        for name in ("sin", "cos"):
            assert 0.5 < fig[name + "_ulp"][0] <= CAP_SINCOS_ULP, fig
            assert fig[name + "_abs_2^-53"][0] * 2.0 ** -53 <= CAP_SINCOS_ABS, fig
            assert fig[name + "_near_zero_ulp"][0] > SINCOS_NEAR_ZERO_EXCEEDS, fig
    return fig


def check_exact(fn, got, got2=None):
    """The equalities at cases(fn): special values, exact results, thresholds.  Shared with the GPU test."""
    x, y = cases(fn)
    got = np.asarray(got)

    def at(xv, yv=None):
        m = same_bits(x, np.full_like(x, xv))
        if yv is not None:
            m &= same_bits(y, np.full_like(y, yv))
        assert m.any(), (fn, xv, yv)
        return m

    def all_bits(mask, want):
        assert same_bits(got[mask], np.full(int(mask.sum()), want)).all(), (fn, want, got[mask][:4])

    if fn == "log":
        all_bits(at(0.0), -np.inf)
        all_bits(at(-0.0), -np.inf)
        all_bits(at(np.inf), np.inf)
        all_bits(at(1.0), 0.0)                                            # +0, not -0
        for v in (-1.0, np.nan, -np.inf):
            assert np.isnan(got[at(v)]).all()
        p2 = np.ldexp(1.0, np.arange(-1074, 1024))                        # every power of two: k ln2 rounded once, from the longdouble ln2
        ln2 = np.log(np.longdouble(2))
        m = np.isin(x, p2) & (x != 1.0)
        k = np.round(np.log2(x[m]))
        assert np.max(ulps(got[m], k.astype(np.longdouble) * ln2)) <= 0.5 + 2.0 ** -10
    elif fn == "exp":
        t_over, t_under, _, t_tiny = EXP_THRESHOLDS
        all_bits(at(0.0), 1.0)
        all_bits(at(-0.0), 1.0)
        all_bits(at(np.inf), np.inf)
        all_bits(at(-np.inf), 0.0)
        assert np.isnan(got[at(np.nan)]).all()
        # the overflow threshold is the largest argument with a finite result, the underflow threshold the smallest with a non-zero one
        # (exp(t_under) = 2^-1075 (1 + 1.6e-14): the correctly rounded result there is 2^-1074, and 0 one ulp further out)
        assert np.isfinite(got[at(t_over)]).all() and np.all(got[at(t_over)] > float.fromhex('0x1.fffffffffffp+1023'))
        all_bits(at(np.nextafter(t_over, np.inf)), np.inf)
        all_bits(at(t_under), 5e-324)
        all_bits(at(np.nextafter(t_under, -np.inf)), 0.0)
        all_bits(at(np.nextafter(t_under, 0.0)), 5e-324)
        assert float(reference_at("exp", [t_under])[0] / np.ldexp(np.longdouble(1), -1075)) > 1.0      # ... by the reference, not by the code
        assert float(reference_at("exp", [np.nextafter(t_under, -np.inf)])[0] / np.ldexp(np.longdouble(1), -1075)) < 1.0
        for s in (1.0, -1.0):                                             # at and below 2^-28 the result is 1 + x, rounded once
            for v in (s * t_tiny, s * np.nextafter(t_tiny, 0.0)):
                all_bits(at(v), 1.0 + v)
        assert np.all(got[(x > t_over)] == np.inf) and np.all(got[x < t_under] == 0.0)
    elif fn == "scalbn":
        with np.errstate(over="ignore"):
            want = reference(fn).astype(np.float64)                     # the exact product, rounded once (inf past the largest double)
        assert same_bits(got, want).all(), [(float(a).hex(), int(b)) for a, b in zip(x, y)][int(np.argmin(same_bits(got, want)))]
    elif fn == "pow_step":
        all_bits(same_bits(x, np.ones_like(x)), 1.0)                    # 1^y
        all_bits(at(4.0, 0.5), 2.0)
    elif fn == "pow_near1":
        m = y == 1.0
        assert m.sum() >= 2000 and same_bits(got[m], 1.0 + x[m]).all()  # y = 1: exactly 1 + r, rounded once
        all_bits(x == 0.0, 1.0)                                           # r = 0: exactly 1
    elif fn == "pow_pos":
        all_bits(x == 1.0, 1.0)
        all_bits(y == 0.0, 1.0)
        ref = reference(fn)
        over = np.asarray(ref >= np.ldexp(np.longdouble(1), 1025))        # far past the ends of the range: inf and 0, not garbage
        under = np.asarray(ref <= np.ldexp(np.longdouble(1), -1080))
        assert over.sum() > 1000 and under.sum() > 1000
        assert np.all(got[over] == np.inf) and same_bits(got[under], np.zeros(int(under.sum()))).all()
    elif fn == "sincos":
        got2 = np.asarray(got2)
        # (sin(-0) comes out as +0: the reduction's first step adds +0 to -0.  A sum of phases does not see the sign of a zero term;
        #  device and checker agree on it, which is what test_gpu_math.py asserts.)
        assert np.all(got[at(0.0) | at(-0.0)] == 0.0) and np.all(got2[at(0.0) | at(-0.0)] == 1.0)
        for v in (2.0 ** -100, -2.0 ** -100):
            assert np.all(got[at(v)] == v) and np.all(got2[at(v)] == 1.0)
        top = np.nextafter(2.0 ** 52, 0.0)
        for v in (2.0 ** 52, -2.0 ** 52, np.inf, -np.inf, np.nan):        # NaN at and above 2^52 ...
            assert np.isnan(got[at(v)]).all() and np.isnan(got2[at(v)]).all()
        for v in (top, -top):                                             # ... and a value just below it
            assert np.isfinite(got[at(v)]).all() and np.isfinite(got2[at(v)]).all()
        fin = np.abs(x) < 2.0 ** 52
        assert np.all(np.abs(got[fin]) <= 1.0) and np.all(np.abs(got2[fin]) <= 1.0)


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import oracle as O
    for fn in FNS:
        x, y = cases(fn)
        g = O.det_eval(fn, x, y)
        f = figures(fn, *g) if fn == "sincos" else figures(fn, g)
        print(fn, x.size, "operands")
        for k, (v, at) in f.items():
            print(f"    {k:22s} {v:14.4f}  at {', '.join(at)}")
