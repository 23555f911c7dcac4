// det_trig.hpp -- sin and cos for the kernels that evaluate a phase (periods.hip, features.hip): a two-term Cody-Waite reduction by
// fused multiply-adds, exact in its first step, then fdlibm's kernels on [-pi/4, pi/4].  The same bits on every run, and the bits of
// oracle/det_trig.h (det_sincos) at every argument.  Accuracy (tests/math_cases.py, measured against an extended-precision reference):
// the ABSOLUTE error is below 2^-53 for every accepted argument, and for |x| < 2^24 the error is below one ulp of the result wherever
// |result| >= 2^-26.  It is NOT below one ulp of a result next to a zero of sin or cos (up to 1.5e5 ulp of a result of 1e-16 at the
// nearest double to 1082091 pi/2; 640 ulp among the DFT phases -2 pi k t / n, n <= 2049): see the tail line below.  The sums that
// use these values (periodograms, DFT coefficients) care about the absolute error only.
#pragma once
#include <hip/hip_runtime.h>

namespace anofox {

namespace {

// sin and cos of x.  k = nearest integer to x 2/pi; x - k p1 is exact (both are multiples of ulp(p1) and the difference is below 1),
// the second step leaves a head y0 and a tail y1 for the kernels.  |x| < 2^52 is accepted; pi/2 - p1 - p2 = p3 = -1.5e-33 goes into
// the tail.  What limits the accuracy is the tail's r0 - y0: when x is next to a multiple of pi/2, y0 cancels far below r0 ~ k p2 and the
// difference is rounded at the scale of r0, an absolute error of up to 2^-53 k p2 (below 2^-84 for |x| < 2^24, 2^-55 at |x| ~ 2^52) that is
// the whole relative error of a tiny result.  Taking k p2 as an exact two-product would repair it and move bits of periods.hip and
// features.hip at the 1e-26 level, for about nine more fp64 operations per call; tests/test_math_cpu.py asserts the present behaviour
// so that such a repair shows.  sin(-0) is +0 (r0 adds +0 to -0): a sum of phases does not see the sign of a zero term.
__device__ __forceinline__ void per_sincos(double x, double &s, double &c)
{
    const double two_over_pi = 6.36619772367581382433e-01;
    const double p1 = 1.57079632679489655800e+00, p2 = 6.12323399573676603587e-17, p3 = -1.49738490485916983766e-33;
    if (!(fabs(x) < 0x1p52)) { s = c = __builtin_nan(""); return; }
    const double k = __builtin_rint(x * two_over_pi);
    const double r0 = fma(-k, p1, x);
    const double y0 = fma(-k, p2, r0);
    const double y1 = fma(-k, p3, fma(-k, p2, r0 - y0));
    const double z = y0 * y0;
    // fdlibm __kernel_sin(y0, y1, 1)
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
                 S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const double v = z * y0;
    const double rs = fma(z, fma(z, fma(z, fma(z, S6, S5), S4), S3), S2);
    const double sn = y0 - ((z * (0.5 * y1 - v * rs) - y1) - v * S1);
    // fdlibm __kernel_cos(y0, y1)
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
                 C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const double w = z * z;
    const double rc = z * fma(z, fma(z, C3, C2), C1) + (w * w) * fma(z, fma(z, C6, C5), C4);
    const double hz = 0.5 * z, w1 = 1.0 - hz;
    const double cs = w1 + (((1.0 - w1) - hz) + (z * rc - y0 * y1));
    const int q = (int)((long long)k & 3);
    const double a = (q & 1) ? cs : sn, b = (q & 1) ? sn : cs;
    s = (q & 2) ? -a : a;
    c = ((q + 1) & 2) ? -b : b;
}

} // namespace

} // namespace anofox
