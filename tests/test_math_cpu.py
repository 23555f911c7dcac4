"""CPU: the checker's elementary functions (oracle/det_math.h: det_log, det_exp, det_scalbn, det_pow_step, det_pow_near1,
det_pow_pos; oracle/det_trig.h: det_sincos, the C copy of the kernels' per_sincos) against a numpy longdouble reference at the
operands of tests/math_cases.py, under the caps stated there: one ulp for log, exp and pow_near1; for sincos 2^-53 absolute, one
ulp of the result away from the zeros, and MORE than one ulp next to them for as long as the reduction stays as it is;
B (1 + |y ln x|) ulp for pow_step and pow_pos.  The exact cases are equalities.  The longdouble reference itself is checked
against 60-digit mpmath where mpmath can be imported.  tests/test_gpu_math.py compares the device functions with these, bit for bit."""
import numpy as np
import pytest

import math_cases as M


@pytest.fixture(scope="module")
def ev(oracle):
    oracle.lib()
    return oracle.det_eval


@pytest.mark.parametrize("fn", M.FNS)
def test_operand_lists_cover_their_edges(fn):
    """The lists are what the tests are worth: every edge the functions branch on is present, and the lists do not change."""
    M.require_longdouble()
    x, y = M.cases(fn)
    assert (y is None) == (fn in ("log", "exp", "sincos")) and x.size <= 210000
    x2, y2 = M._CASES[fn]()
    assert M.same_bits(x[:x2.size], x2).all()                             # seeded: the same list every time
    if fn == "log":
        hx = x.view(np.uint64) >> np.uint64(32)
        assert ((hx == 0x3fe6a09e) & (x.view(np.uint64) & np.uint64(0xffffffff) == 0)).any() and (hx == 0x3fe6a09d).any()
        assert np.isin(np.ldexp(1.0, np.arange(-1074, 1024)), x).all()
        assert ((x > 0) & (x < 2.0 ** -1022)).sum() > 50                   # subnormal arguments: the scaling branch
    elif fn == "exp":
        for t in M.EXP_THRESHOLDS:
            assert np.isin([np.nextafter(t, -np.inf), t, np.nextafter(t, np.inf)], x).all()
        assert ((x < -708.4) & (x > -745.14)).sum() > 10000 and ((x > 709.0896) & (x <= 709.7827)).sum() > 5000   # scalbn's two outer branches
    elif fn == "scalbn":
        assert {1022, -1022, 1023, -1023, 1024, -1024, 2045, -2045, 2046, -2046, 2047, -2047, 3000, -3000} <= set(y.astype(int))
    elif fn == "pow_step":
        for e in (-1, 0, 1):
            edges = np.ldexp(1.0 + np.arange(128) / 128.0, e)
            assert np.isin(edges, x).all() and np.isin(np.nextafter(edges, 0.0), x).all()
        assert (x < 1.0).sum() > 30000 and np.isin([2.0 ** -1000, 2.0 ** 1000], x).all()
        assert np.all((y > 0) & (y <= 1.0)) and np.all((x >= 2.0 ** -1000) & (x <= 2.0 ** 1000))      # the documented domain, nothing else
        assert np.isin([1.0, 2.0 ** -20, 0.8, 0.98], y).all()
    elif fn == "pow_near1":
        assert np.isin(M.POW_NEAR1_R, x).all() and np.all(np.abs(x) <= 2.0 ** -4) and np.all((y > 0) & (y <= 1.0))
    elif fn == "pow_pos":
        assert np.all(x > 0) and np.all((y >= 0) & (y <= 50.0))
    elif fn == "sincos":
        k = np.round(x / (np.pi / 2))
        with np.errstate(invalid="ignore"):
            near = np.abs(x - k * (np.pi / 2)) <= 4 * np.spacing(np.abs(x))
        assert near.sum() > 50000 and {0, 1, 2, 3} == set((k[near].astype(np.int64) & 3).tolist()) and (k[near] < 0).sum() > 20000
        assert np.isin(M.SINCOS_SPECIAL[:8], x).all()


@pytest.mark.parametrize("fn", M.FNS)
def test_checker_function_meets_its_caps(ev, fn):
    x, y = M.cases(fn)
    got = ev(fn, x, y)
    if fn == "sincos":
        M.check_exact(fn, *got)
        M.check_caps(fn, *got)
    else:
        M.check_exact(fn, got)
        M.check_caps(fn, got)


def test_sincos_symmetry_and_quadrants(ev):
    """Away from zero sin is odd and cos is even in every bit (the reduction and the kernels are odd / even operation by operation), and a quadrant
    turn swaps the kernels: sin(x) at the nearest double to k pi/2 is +-1 for odd k, cos(x) for even k, within one ulp."""
    x, _ = M.cases("sincos")
    x = x[(np.abs(x) < 2.0 ** 52) & (x != 0.0)]                            # (not the zeros: sin(-0) is +0, see math_cases.check_exact)
    s, c = ev("sincos", x)
    s2, c2 = ev("sincos", -x)
    assert M.same_bits(s2, -s).all() and M.same_bits(c2, c).all()
    k = np.arange(-20000, 20001)
    xs = (k.astype(np.longdouble) * np.longdouble("1.57079632679489661923132169163975144209858469968755")).astype(np.float64)
    s, c = ev("sincos", xs)
    want_s = np.where(k % 2 == 0, 0.0, np.where(k % 4 == 1, 1.0, -1.0))
    want_c = np.where(k % 2 != 0, 0.0, np.where(k % 4 == 0, 1.0, -1.0))
    assert np.max(np.abs(s - want_s)) < 1e-11 and np.max(np.abs(c - want_c)) < 1e-11      # the quadrant (|x - k pi/2| <= ulp(31416)/2 = 1.8e-12)
    odd, even = k % 2 != 0, k % 2 == 0
    assert np.all(np.abs(s[odd] - want_s[odd]) <= 2.0 ** -53) and np.all(np.abs(c[even] - want_c[even]) <= 2.0 ** -53)


def test_the_cases_the_old_sample_missed(ev):
    """The two statements the tree made and no test checked.  det_pow_step was documented "below 1.5 ulp over the domain": it is not
    even on [1/2, 2] (tests/test_host_logic.py's 1,500 seeded points miss these operands).  per_sincos was documented "below one ulp
    for every argument": not next to a zero.  Pinned at the operands of the survey, so the corrected comments stay honest."""
    h = float.fromhex
    x = np.array([h("0x1.e25e070fb600cp+0"), h("0x1.ef5efcfd85d72p+0"), h("0x1.8659eb9cfcda2p+776")])
    y = np.array([h("0x1.df688a45c2364p-1"), h("0x1.ff53967c7cdd5p-1"), h("0x1.f7068186559d7p-1")])
    u = np.asarray(M.ulps(ev("pow_step", x, y), M.reference_at("pow_step", x, y)), dtype=np.float64)
    print("pow_step ulps", u)
    assert np.all(u[:2] > 2.0) and np.all(u[:2] < 2.2) and 1400.0 < u[2] < 1450.0
    assert np.all(u <= M.B_POW_STEP * M.pow_scale(x, y))
    xs = np.array([h("0x1.9eb7148f354d6p+20"), h("-0x1.6c6cbc45dc8dep+6")])
    s, c = ev("sincos", xs)
    rs, rc = M.reference_at("sincos", xs)
    print("sincos ulps", M.ulps(s, rs), M.ulps(c, rc))
    assert float(M.ulps(c, rc)[0]) > 1e5 and float(max(M.ulps(s, rs)[1], M.ulps(c, rc)[1])) > 100.0
    assert np.all(np.abs(s.astype(np.longdouble) - rs) <= 2.0 ** -53) and np.all(np.abs(c.astype(np.longdouble) - rc) <= 2.0 ** -53)


def test_device_entry_checks_its_arguments_before_it_touches_a_device(hiplib):
    """anofox_hip_selftest_math refuses a workgroup size other than 64 / 256, an unknown function and a missing array with an error
    and a message, writes nothing, and is in the symbol list; this needs no GPU.  What it computes: tests/test_gpu_math.py."""
    import ctypes as C
    L = hiplib.load()
    assert "anofox_hip_selftest_math" in hiplib.EXPORTED_SYMBOLS and hiplib.NM_BLOCK == 64
    assert hiplib.MATH_FNS == {fn: i for i, fn in enumerate(M.FNS)}
    from oracle import oracle as O
    assert O.MATH_FNS == hiplib.MATH_FNS
    x, out = np.array([1.0, 2.0]), np.full(2, -7.0)
    for fn, block, xp, yp, op, o2p, code in ((0, 128, x, None, out, None, 2), (0, 0, x, None, out, None, 2), (0, 1024, x, None, out, None, 2),
                                             (7, 64, x, None, out, None, 2), (-1, 256, x, None, out, None, 2), (3, 64, x, None, out, None, 1),
                                             (6, 64, x, None, out, None, 1), (0, 64, None, None, out, None, 1), (0, 256, x, None, None, None, 1)):
        err = hiplib.AnofoxError()
        ok = L.anofox_hip_selftest_math(fn, None if xp is None else xp.ctypes.data, None if yp is None else yp.ctypes.data, 2, block,
                                        None if op is None else op.ctypes.data, None if o2p is None else o2p.ctypes.data, C.byref(err))
        assert not ok and err.code == code and err.message, (fn, block, err.code, err.message)
        assert np.all(out == -7.0)
    assert not L.anofox_hip_selftest_math(0, x.ctypes.data, None, (1 << 28) + 1, 64, out.ctypes.data, None, None)      # err may be NULL


def test_ulps_and_same_bits_measure_what_they_say():
    """The yardstick itself: ulps() on hand-made cases, same_bits() on zeros and NaNs."""
    M.require_longdouble()
    one = np.longdouble(1)
    assert M.ulps([1.0], [one])[0] == 0 and M.ulps([np.nextafter(1.0, 2.0)], [one])[0] == 1.0
    assert M.ulps([np.nextafter(1.0, 0.0)], [one])[0] == 0.5               # ulp of the reference's binade, [1, 2)
    assert M.ulps([1.0], [one + np.ldexp(one, -53)])[0] == 0.5
    assert M.ulps([0.0], [np.ldexp(one, -1075)])[0] == 0.5 and M.ulps([5e-324], [np.longdouble(0)])[0] == 1.0   # floored at 2^-1074
    assert M.ulps([2.0 ** -1022], [np.ldexp(one, -1022) + np.ldexp(one, -1074)])[0] == 1.0
    assert M.ulps([np.inf], [np.ldexp(one, 2000)])[0] == 0 and M.ulps([np.inf], [np.ldexp(one, 1023)])[0] == 2.0 ** 52
    assert M.ulps([np.nan], [one])[0] == np.inf and np.isnan(M.ulps([1.0], [np.longdouble(np.inf)])[0]) and np.isnan(M.ulps([1.0], [np.longdouble(np.nan)])[0])
    assert not M.same_bits([0.0], [-0.0])[0] and M.same_bits([np.nan], [-np.nan])[0] and not M.same_bits([np.nan], [1.0])[0]
    assert not M.same_bits([1.0], [np.nextafter(1.0, 2.0)])[0]


@pytest.mark.parametrize("fn", [f for f in M.FNS if f != "scalbn"])
def test_longdouble_reference_against_mpmath(fn):
    """The reference's own error: about 2,000 operands per function against 60-digit mpmath, within 2^-60 relative (an ulp of a
    double's result is 2^-52 relative: the reference resolves better than 2^-7 of it)."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 60
    M.require_longdouble()
    x, y = M.cases(fn)
    rng = np.random.default_rng(7)
    idx = np.unique(np.concatenate([np.arange(0, min(x.size, 400)), rng.integers(0, x.size, 1600), np.arange(x.size - 10, x.size)]))
    ref = M.reference(fn)

    def to_mp(v):                                                         # a longdouble, exactly: (head + tail) 2^e, whatever its exponent
        m, e = np.frexp(v)
        hi = float(m)
        return mp.ldexp(mp.mpf(hi) + mp.mpf(float(m - np.longdouble(hi))), int(e))

    worst = 0.0
    for i in idx:
        xi = mp.mpf(float(x[i]))
        yi = None if y is None else mp.mpf(float(y[i]))
        if fn == "log":
            if not (x[i] > 0 and np.isfinite(x[i])):
                continue
            pairs = [(mp.log(xi), ref[i])]
        elif fn == "exp":
            if not np.isfinite(x[i]):
                continue
            pairs = [(mp.exp(xi), ref[i])]
        elif fn in ("pow_step", "pow_pos"):
            pairs = [(mp.power(xi, yi), ref[i])]
        elif fn == "pow_near1":
            pairs = [(mp.power(1 + xi, yi), ref[i])]
        else:
            if not abs(x[i]) < 2.0 ** 52:
                continue
            pairs = [(mp.sin(xi), ref[0][i]), (mp.cos(xi), ref[1][i])]
        for want, got in pairs:
            if want == 0:
                assert got == 0
                continue
            worst = max(worst, float(abs(to_mp(got) - want) / abs(want)))
    print(fn, "longdouble reference vs mpmath: worst relative error 2^%.2f" % (np.log2(worst) if worst > 0 else -np.inf))
    assert worst <= 2.0 ** -60, worst
