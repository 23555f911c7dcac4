/*
 * det_trig.h -- TEST INFRASTRUCTURE (oracle).  Not part of the product.
 *
 * CPU restatement of per_sincos (csrc/det_trig.hpp): the same operations in the same order, fma() where the kernel writes fma, every
 * other +, -, * one IEEE-754 binary64 operation (the build uses -ffp-contract=off).  The kernels that evaluate a phase
 * (periods.hip, features.hip) are checked against their sources with a tolerance, so nothing else in the oracle calls this; it
 * exists so that the device function can be compared bit for bit at given operands (tests/test_gpu_math.py) and measured against
 * an extended-precision reference without a GPU (tests/test_math_cpu.py).
 *
 * Accuracy (tests/math_cases.py): the ABSOLUTE error stays below 2^-53 for |x| < 2^24, and the error is below one ulp of the result
 * wherever |result| >= 2^-26.  Next to a zero of sin or cos it is NOT below one ulp of the (tiny) result: the tail line rounds
 * r0 - y0 at the scale of r0 when y0 has cancelled far below it, an error of ~1e-26 that is the whole relative error of a result
 * of ~1e-16.  DFT sums care about the absolute error only.  sin(-0) is +0, as on the device (r0 adds +0 to -0).
 */
#ifndef ORACLE_DET_TRIG_H
#define ORACLE_DET_TRIG_H

#include <math.h>

static inline void det_sincos(double x, double *s, double *c)
{
    const double two_over_pi = 6.36619772367581382433e-01;
    const double p1 = 1.57079632679489655800e+00, p2 = 6.12323399573676603587e-17, p3 = -1.49738490485916983766e-33;
    if (!(fabs(x) < 0x1p52)) { *s = *c = NAN; return; }
    const double k = rint(x * two_over_pi);
    const double r0 = fma(-k, p1, x);
    const double y0 = fma(-k, p2, r0);
    const double y1 = fma(-k, p3, fma(-k, p2, r0 - y0));
    const double z = y0 * y0;
    /* fdlibm __kernel_sin(y0, y1, 1) */
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
                 S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const double v = z * y0;
    const double rs = fma(z, fma(z, fma(z, fma(z, S6, S5), S4), S3), S2);
    const double sn = y0 - ((z * (0.5 * y1 - v * rs) - y1) - v * S1);
    /* fdlibm __kernel_cos(y0, y1) */
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
                 C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const double w = z * z;
    const double rc = z * fma(z, fma(z, C3, C2), C1) + (w * w) * fma(z, fma(z, C6, C5), C4);
    const double hz = 0.5 * z, w1 = 1.0 - hz;
    const double cs = w1 + (((1.0 - w1) - hz) + (z * rc - y0 * y1));
    const int q = (int)((long long)k & 3);
    const double a = (q & 1) ? cs : sn, b = (q & 1) ? sn : cs;
    *s = (q & 2) ? -a : a;
    *c = ((q + 1) & 2) ? -b : b;
}

#endif /* ORACLE_DET_TRIG_H */
