// arima_paths.hip -- sample paths simulated from fitted ARIMA models (DESIGN.md section 3 "ARIMA paths"): the fitted recursion
//   (1 - phi(B))(1 - Phi(B^m)) (w_t - c) = (1 - theta(B))(1 - Theta(B^m)) e_t,   w = (1 - B)^d (1 - B^m)^D y
// runs forward from the tails of the differenced series and of its in-sample innovations, h steps for each of n_paths paths per
// series, with innovations that are Gaussian (sigma = sqrt(css / nu)) or drawn from the model's own residuals; the differences are
// then integrated as arima_forecast_kernel integrates its forecasts.  The method is the textbook one (Box & Jenkins; Hyndman &
// Athanasopoulos, "Prediction intervals from simulated paths"), the names are this package's own; tests/arima_paths_ref.py is the
// definition, bit for bit.
//
// Arithmetic: plain fp64, one rounding per operation (-ffp-contract=off).  The two lag polynomials of a side are NOT multiplied out:
// a side is the sum over the terms (i, j), 0 <= i <= p, 0 <= j <= P, without (0, 0), of coefficient x value at lag i + j m, the
// coefficient phi_i, Phi_j or -(phi_i Phi_j), added j-major and i-minor from acc = 0.0 (ap_side).  x_t = (ar + e_t) - ma, w_t = x_t + c;
// in sample e_t = (x_t - ar) + ma.  A value before the differenced series is 0.0 and is multiplied and added like any other.
//
// Draws: Philox4x32-10 on counters (philox.hpp).  Gaussian: the rule of ets_paths.hip with the last counter word 3.  Bootstrap: the
// rule of paths.hip unchanged, on the series' own residuals; joint: draw j < pool_rows takes row nu - pool_rows + j of every series.
//
//   arima_fit_state_kernel     the selected orders and box-clipped coefficients of a run AutoARIMA batch as two time-major blocks.
//   arima_innovations_kernel   lanes over series, one series per lane, the CSS recursion serially in t: the five ordinary lags of x
//                              and e shift through registers, a seasonal lag of x is formed again from y (a row of the time-major
//                              block is one coalesced load) and a seasonal lag of e is read back from the residual block.
//   arima_paths_status_kernel  64 series x 4 slices per workgroup: NO_MODEL, then the pool statuses in the precedence of ets_paths.hip.
//   arima_paths_kernel         lanes over SERIES, a wavefront owns (64 series, one path at a time): the store of a step is one
//                              512-byte row segment.  The five ordinary lags live in registers.  The simulated x and e a later step
//                              reads at a seasonal lag go into LDS in STEP order: ring slot k % R of lane s, R = min(h, 2 m + 5), and
//                              with D = 1 and m < h the simulated y in a ring of m slots; all lanes of a wave touch ONE 512-byte LDS
//                              row per access and a lane reads only what it wrote itself: no barrier.  The history before the
//                              forecast origin is the same for every path of a series; it is NOT staged per workgroup: the five
//                              ordinary lags are loaded once per lane, a seasonal lag that still reaches behind the origin (step
//                              k < lag) is formed from y (L2-resident: the tile's tail is at most 3 m + 7 rows of 512 bytes) or
//                              read from the residual block.  Staging would cost 2 (2 m + 5) LDS rows per workgroup, more than the
//                              rings themselves at h < 2 m, for loads that only the first steps of a path make.
//                              (2 R + (m < h ? m : 0)) x 512 bytes per wave within 64 KiB give the waves of a workgroup.  The
//                              orders are per-lane values: the branches on them cost their union in a mixed wave; they choose
//                              operations, never their order.
//   arima_paths_broken_kernel  n_broken = the paths of a series that hold a NaN.
// No atomics, no per-lane array indexed by a run-time value.
#include "kernels.hpp"
#include "det_math.hpp"
#include "det_trig.hpp"
#include "philox.hpp"

namespace anofox {

namespace {

constexpr int AP_SLICES = 4;                              // slices of the status kernel
constexpr int AP_MAX_WAVES = 4;                           // waves per workgroup of the simulation kernel
constexpr int AP_COUNT_WAVES = 16;                        // waves per workgroup of the counting kernel

// the fit of one series as a lane holds it: orders, the lengths they give and the coefficients (0.0 beyond the orders)
struct ApFit {
    int p, d, q, P, D, Q, c, n, n_diff, La, Lb;
    bool model;
    double phi[5], theta[5], Phi[2], Theta[2], cst;
};

// `model`: orders inside p, q <= 5, P, Q <= 2, d <= 2, D <= 1, at least one observation, the block's n_diff = n - d - D m and at
// least one residual (nu = n_diff - p - m P >= 1); without a model every order is 0 and no loop below does anything
__device__ __forceinline__ void ap_load(const int32_t *orders, const double *coef, size_t ld, size_t s, int length, int t_rows, int m, ApFit &f)
{
    const int32_t *o = orders + s;
    f.p = o[0]; f.d = o[ld]; f.q = o[2 * ld]; f.P = o[3 * ld]; f.D = o[4 * ld]; f.Q = o[5 * ld]; f.c = o[6 * ld];
    const int nd = o[7 * ld];
    f.n = length < 0 ? 0 : (length > t_rows ? t_rows : length);
    const bool in = f.p >= 0 && f.p <= 5 && f.q >= 0 && f.q <= 5 && f.P >= 0 && f.P <= 2 && f.Q >= 0 && f.Q <= 2 && f.d >= 0 && f.d <= 2 &&
                    f.D >= 0 && f.D <= 1 && (f.c == 0 || f.c == 1);
    if (!in) f.p = f.d = f.q = f.P = f.D = f.Q = f.c = 0;
    f.n_diff = f.n - f.d - f.D * m;
    f.La = f.p + m * f.P;
    f.model = in && length >= 1 && f.n >= 1 && nd == f.n_diff && f.n_diff - f.La >= 1;
    if (!f.model) { f.p = f.d = f.q = f.P = f.D = f.Q = f.c = 0; f.n_diff = 0; f.La = 0; }
    f.Lb = f.q + m * f.Q;
    const double *x = coef + s;
#pragma unroll
    for (int i = 0; i < 5; i++) {
        f.phi[i] = i < f.p ? x[(size_t)i * ld] : 0.0;
        f.theta[i] = i < f.q ? x[(size_t)(5 + i) * ld] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < 2; i++) {
        f.Phi[i] = i < f.P ? x[(size_t)(10 + i) * ld] : 0.0;
        f.Theta[i] = i < f.Q ? x[(size_t)(12 + i) * ld] : 0.0;
    }
    f.cst = f.c ? x[(size_t)14 * ld] : 0.0;
}

// w_t of the differenced series from the column y (element i at y[i * ld]): the seasonal difference first, then the d ordinary
// ones, each a single subtraction; 0 <= t < n_diff
__device__ __forceinline__ double ap_w(const double *y, size_t ld, int t, int d, int D, int m)
{
    auto u = [&](int i) { return D ? y[(size_t)(i + m) * ld] - y[(size_t)i * ld] : y[(size_t)i * ld]; };
    if (d == 0) return u(t);
    if (d == 1) return u(t + 1) - u(t);
    const double lo = u(t + 1) - u(t), hi = u(t + 2) - u(t + 1);
    return hi - lo;
}

// x_t = w_t - c, 0.0 before the series
__device__ __forceinline__ double ap_x(const double *y, size_t ld, int t, const ApFit &f, int m)
{
    return t >= 0 ? ap_w(y, ld, t, f.d, f.D, m) - f.cst : 0.0;
}

// one side of the recursion: near[i - 1] is the value at the ordinary lag i, far(L) the value at a lag L = i + j m with j >= 1
template <class Far>
__device__ __forceinline__ double ap_side(const double (&c1)[5], const double (&c2)[2], int n1, int n2, int m, const double (&near)[5], Far far)
{
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j <= 2; j++)
#pragma unroll
        for (int i = 0; i <= 5; i++) {
            if (i == 0 && j == 0) continue;
            if (i <= n1 && j <= n2) {
                double coef, v;
                if (j == 0) { coef = c1[i > 0 ? i - 1 : 0]; v = near[i > 0 ? i - 1 : 0]; }
                else {
                    coef = i == 0 ? c2[j - 1] : -(c1[i > 0 ? i - 1 : 0] * c2[j - 1]);
                    v = far(i + j * m);
                }
                acc = acc + coef * v;
            }
        }
    return acc;
}

__device__ __forceinline__ void ap_shift(double (&r)[5], double v)
{
    r[4] = r[3]; r[3] = r[2]; r[2] = r[1]; r[1] = r[0]; r[0] = v;
}

__global__ __launch_bounds__(256) void arima_fit_state_kernel(const int32_t *status, const int32_t *model_code, const int32_t *order, const int32_t *d,
                                                              const int32_t *D, const int32_t *wlen, const double *x, const double *aicc, size_t ld,
                                                              int n_series, int32_t *orders, double *coef)
{
    const size_t s = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= (size_t)n_series) return;
    const double nan = __builtin_nan("");
    int32_t *o = orders + s;
    double *c = coef + s;
    if (!(status[s] == 0 && model_code[s] >= 1000000)) {            // nothing was fitted (or the fallback chain forecast it)
        for (int i = 0; i < 8; i++) o[(size_t)i * ld] = 0;
        for (int i = 0; i < 16; i++) c[(size_t)i * ld] = nan;
        return;
    }
    const int p = order[s], q = order[ld + s], P = order[2 * ld + s], Q = order[3 * ld + s], has_c = order[4 * ld + s];
    o[0] = p; o[ld] = d[s]; o[2 * ld] = q; o[3 * ld] = P; o[4 * ld] = D[s]; o[5 * ld] = Q; o[6 * ld] = has_c; o[7 * ld] = wlen[s];
    for (int i = 0; i < 14; i++) c[(size_t)i * ld] = 0.0;
    auto box = [](double a) { return a < -0.99 ? -0.99 : (a > 0.99 ? 0.99 : a); };      // arima.hip AR_COEF_BOX
    size_t k = 0;                                                   // (the batch keeps at most 6 coordinates per series)
    for (int i = 0; i < p && i < 5 && k < 6; i++) c[(size_t)i * ld] = box(x[(k++) * ld + s]);
    for (int i = 0; i < q && i < 5 && k < 6; i++) c[(size_t)(5 + i) * ld] = box(x[(k++) * ld + s]);
    for (int i = 0; i < P && i < 2 && k < 6; i++) c[(size_t)(10 + i) * ld] = box(x[(k++) * ld + s]);
    for (int i = 0; i < Q && i < 2 && k < 6; i++) c[(size_t)(12 + i) * ld] = box(x[(k++) * ld + s]);
    c[(size_t)14 * ld] = (has_c && k < 6) ? x[k * ld + s] : 0.0;
    c[(size_t)15 * ld] = aicc[s];
}

__global__ __launch_bounds__(64) void arima_innovations_kernel(const int32_t *orders, const double *coef, size_t ld, const double *y,
                                                               const int32_t *lengths, int t_rows, int m, int n_series, double *resid,
                                                               int32_t *resid_len, double *sigma)
{
    const size_t s = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (s >= (size_t)n_series) return;
    ApFit f;
    ap_load(orders, coef, ld, s, lengths[s], t_rows, m, f);
    if (!f.model) {
        resid_len[s] = 0;
        sigma[s] = __builtin_nan("");
        return;
    }
    const double *yc = y + s;
    double *rc = resid + s;
    const int La = f.La;
    double xr[5], er[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < 5; i++) xr[i] = ap_x(yc, ld, La - 1 - i, f, m);
    double css = 0.0;
    for (int t = La; t < f.n_diff; t++) {
        const double xt = ap_x(yc, ld, t, f, m);
        const double ar = ap_side(f.phi, f.Phi, f.p, f.P, m, xr, [&](int L) { return ap_x(yc, ld, t - L, f, m); });
        const double ma = ap_side(f.theta, f.Theta, f.q, f.Q, m, er, [&](int L) {
            const int j = t - L - La;                                // (row j of the compacted block is the residual of index La + j)
            return j >= 0 ? rc[(size_t)j * ld] : 0.0;
        });
        const double e = (xt - ar) + ma;
        rc[(size_t)(t - La) * ld] = e;                               // t - La < n_diff <= t_rows
        css = css + e * e;
        ap_shift(xr, xt);
        ap_shift(er, e);
    }
    const int nu = f.n_diff - La;
    resid_len[s] = nu;
    sigma[s] = sqrt(css / (double)nu);
}

__global__ __launch_bounds__(64 * AP_SLICES) void arima_paths_status_kernel(const ArimaPathsArgs a)
{
    __shared__ int has_nan[AP_SLICES][64];
    const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const size_t sl = (size_t)blockIdx.x * 64 + (size_t)lane;
    const bool in = sl < (size_t)a.n_series;
    const size_t s = in ? sl : 0;
    const bool boot = a.innovations == ARIMA_PATHS_BOOTSTRAP;
    ApFit f;
    ap_load(a.orders, a.coef, a.ld, s, in ? a.lengths[s] : 0, a.t_rows, a.m, f);
    const int nu = f.n_diff - f.La;
    const bool model = in && f.model && a.resid_len[s] == nu;
    bool bad = false;
    if (model) {
        const double *y = a.y + s, *e = a.resid + s;
        int tail = f.La + f.d + f.D * a.m;                           // the observations a path reads
        tail = tail > f.n ? f.n : tail;
        for (int t = f.n - tail + slice; t < f.n; t += AP_SLICES) {
            const double x = y[(size_t)t * a.ld];
            bad = bad || x != x;
        }
        // the residuals a path reads: the last q + m Q ones, and with the bootstrap the rows of its pool
        int first = nu - (f.Lb < nu ? f.Lb : nu);
        if (boot) first = a.joint ? (a.pool_rows <= nu && nu - a.pool_rows < first ? nu - a.pool_rows : first) : 0;
        for (int t = first + slice; t < nu; t += AP_SLICES) {
            const double x = e[(size_t)t * a.ld];
            bad = bad || x != x;
        }
        if (slice == 0) {
#pragma unroll
            for (int i = 0; i < 5; i++) bad = bad || f.phi[i] != f.phi[i] || f.theta[i] != f.theta[i];
#pragma unroll
            for (int i = 0; i < 2; i++) bad = bad || f.Phi[i] != f.Phi[i] || f.Theta[i] != f.Theta[i];
            bad = bad || f.cst != f.cst;
            if (!boot) { const double x = a.sigma[s]; bad = bad || x != x; }
        }
    }
    has_nan[slice][lane] = bad ? 1 : 0;
    __syncthreads();
    if (slice != 0 || !in) return;
    int any = 0;
#pragma unroll
    for (int i = 0; i < AP_SLICES; i++) any |= has_nan[i][lane];
    int32_t status = PATHS_OK;
    if (!model) status = ARIMA_PATHS_NO_MODEL;
    else if (boot && a.joint && nu < a.pool_rows) status = PATHS_RAGGED;
    else if (boot && a.joint && a.pool_rows == 0) status = PATHS_EMPTY;
    else if (any) status = PATHS_NAN;
    a.status[s] = status;
}

// two standard normal draws of two 32-bit words: the even step's and the odd step's (the rule of ets_paths.hip)
__device__ __forceinline__ void ap_normal_pair(uint32_t wa, uint32_t wb, double &z_even, double &z_odd)
{
    const double u1 = ((double)wa + 0.5) * 0x1p-32, u2 = ((double)wb + 0.5) * 0x1p-32;
    const double r = sqrt(-2.0 * dm_log(u1));
    double sn, cs;
    per_sincos(6.283185307179586 * u2, sn, cs);
    z_even = r * cs;
    z_odd = r * sn;
}

// blockDim.x / 64 = a.waves paths at a time per workgroup, (2 a.ring + a.yring) x 64 doubles of dynamic LDS per wave
__global__ __launch_bounds__(64 * AP_MAX_WAVES) void arima_paths_kernel(const ArimaPathsArgs a)
{
    extern __shared__ double ap_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int W = a.waves, R = a.ring, RY = a.yring;
    // workgroup b -> (tile of 64 series, group of W paths) as in ets_paths_kernel: the groups of a tile follow each other on one XCD
    const unsigned blk = blockIdx.x, groups = (unsigned)a.path_groups;
    const unsigned group = (blk >> 3) % groups;
    const size_t sl = ((size_t)((blk >> 3) / groups) * 8 + (blk & 7u)) * 64 + (size_t)lane;
    if (sl >= (size_t)a.n_series) return;                    // (the kernel has no barrier)
    const size_t s = sl, ld = a.ld;
    const int h = a.horizon, m = a.m;
    const bool ok = a.status[s] == PATHS_OK;
    const bool boot = a.innovations == ARIMA_PATHS_BOOTSTRAP;
    const double nan = __builtin_nan("");
    ApFit f;
    ap_load(a.orders, a.coef, ld, s, ok ? a.lengths[s] : 0, a.t_rows, m, f);       // (status 0: the model holds; else every order is 0)
    const double *y = a.y + s, *res = a.resid + s;
    const int n = f.n, nd = f.n_diff, La = f.La, nu = nd - La;
    const double sigma = (ok && !boot) ? a.sigma[s] : 0.0;
    // the origin: the five ordinary lags of x and e, and the start values of the integration (of the seasonally differenced series)
    double hx[5], he[5];
#pragma unroll
    for (int i = 0; i < 5; i++) {
        hx[i] = ok ? ap_x(y, ld, nd - 1 - i, f, m) : 0.0;
        he[i] = (ok && nu - 1 - i >= 0) ? res[(size_t)(nu - 1 - i) * ld] : 0.0;
    }
    double start0 = 0.0, start1 = 0.0;
    if (ok && f.d >= 1) {
        const int len = n - f.D * m;                                   // >= d + 1: the differenced series is not empty
        start0 = ap_w(y, ld, len - 1, 0, f.D, m);
        if (f.d == 2) start1 = start0 - ap_w(y, ld, len - 2, 0, f.D, m);
    }
    const uint64_t pool_n = (ok && boot) ? (uint64_t)(a.joint ? a.pool_rows : nu) : 0ull;
    const double *pool = res + (size_t)((ok && boot && a.joint) ? nu - a.pool_rows : 0) * ld;      // (status 0 in joint mode: nu >= pool_rows)
    const uint32_t c1 = (boot && a.joint) ? 0u : (uint32_t)s, c3 = boot ? (a.joint ? 1u : 0u) : 3u;
    double *ring = ap_lds + (size_t)wave * (size_t)(2 * R + RY) * 64 + (size_t)lane;        // x slot i at ring[i * 64]
    double *ering = ring + (size_t)R * 64, *yring = ring + (size_t)2 * R * 64;
    for (int p = (int)group * W + wave; p < a.n_paths; p += (int)groups * W) {
        double *out = a.paths + (size_t)p * (size_t)h * a.ld_out + s;
        if (!ok) {
            for (int k = 0; k < h; k++) out[(size_t)k * a.ld_out] = nan;
            continue;
        }
        double xr[5], er[5];
#pragma unroll
        for (int i = 0; i < 5; i++) { xr[i] = hx[i]; er[i] = he[i]; }
        double l0 = start0, l1 = start1;
        bool broken = false;
        int slot = 0, yslot = 0;
        for (int k0 = 0; k0 < h; k0 += 4) {
            uint32_t u[4];
            philox4x32_10((uint32_t)p, c1, (uint32_t)(k0 >> 2), c3, a.key0, a.key1, u);
            double dr[4];
            if (boot) {
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const uint64_t j = ((uint64_t)u[i] * pool_n) >> 32;                  // j < pool_n <= nu
                    dr[i] = k0 + i < h ? pool[(size_t)j * ld] : 0.0;
                }
            } else {
                double z[4] = {0.0, 0.0, 0.0, 0.0};
                ap_normal_pair(u[0], u[1], z[0], z[1]);
                if (k0 + 2 < h) ap_normal_pair(u[2], u[3], z[2], z[3]);
#pragma unroll
                for (int i = 0; i < 4; i++) dr[i] = sigma * z[i];
            }
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int k = k0 + i;
                if (k >= h) break;
                double *cell = out + (size_t)k * a.ld_out;
                if (broken) {
                    *cell = nan;
                    continue;
                }
                // a seasonal lag L <= 2 m + 5: simulated (step k - L, slot (k - L) % R with L <= R) or behind the origin
                const double ar = ap_side(f.phi, f.Phi, f.p, f.P, m, xr, [&](int L) {
                    if (k < L) return ap_x(y, ld, nd + k - L, f, m);
                    const int at = slot - L;
                    return ring[(size_t)(at < 0 ? at + R : at) * 64];
                });
                const double ma = ap_side(f.theta, f.Theta, f.q, f.Q, m, er, [&](int L) {
                    if (k < L) { const int j = nu + k - L; return j >= 0 ? res[(size_t)j * ld] : 0.0; }
                    const int at = slot - L;
                    return ering[(size_t)(at < 0 ? at + R : at) * 64];
                });
                const double e = dr[i];
                const double x = (ar + e) - ma;
                double v = x + f.cst;
                if (f.d == 2) { l1 = l1 + v; v = l1; }
                if (f.d >= 1) { l0 = l0 + v; v = l0; }
                if (f.D) v = v + (k < m ? y[(size_t)(n + k - m) * ld] : yring[(size_t)yslot * 64]);
                broken = !(v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308);
                *cell = broken ? nan : v;
                ring[(size_t)slot * 64] = x;
                ering[(size_t)slot * 64] = e;
                slot = slot + 1 == R ? 0 : slot + 1;
                if (RY > 0) {                                          // (m < h: slot k % m holds y of step k - m until it is replaced)
                    yring[(size_t)yslot * 64] = v;
                    yslot = yslot + 1 == RY ? 0 : yslot + 1;
                }
                ap_shift(xr, x);
                ap_shift(er, e);
            }
        }
    }
}

__global__ __launch_bounds__(64 * AP_COUNT_WAVES) void arima_paths_broken_kernel(const ArimaPathsArgs a)
{
    __shared__ int cnt[AP_COUNT_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t sl = (size_t)blockIdx.x * 64 + (size_t)lane;
    const bool in = sl < (size_t)a.n_series;
    const int h = a.horizon;
    int c = 0;
    if (in)
        for (int p = wave; p < a.n_paths; p += AP_COUNT_WAVES) {
            const double *col = a.paths + (size_t)p * (size_t)h * a.ld_out + sl;
            bool bad = false;
            for (int k = 0; k < h; k++) {
                const double x = col[(size_t)k * a.ld_out];
                bad = bad || x != x;
            }
            c += bad ? 1 : 0;
        }
    cnt[wave][lane] = c;
    __syncthreads();
    if (wave != 0 || !in) return;
    int total = 0;
#pragma unroll
    for (int i = 0; i < AP_COUNT_WAVES; i++) total += cnt[i][lane];
    a.n_broken[sl] = total;
}

} // namespace

int arima_paths_lds_rows(int m, int horizon)
{
    const int ring = horizon < 2 * m + 5 ? horizon : 2 * m + 5;
    return 2 * ring + (m < horizon ? m : 0);
}

int arima_paths_waves(int lds_rows)
{
    const int w = ARIMA_PATHS_MAX_LDS_ROWS / (lds_rows < 1 ? 1 : lds_rows);
    return w > AP_MAX_WAVES ? AP_MAX_WAVES : (w < 1 ? 1 : w);
}

void launch_arima_paths(const ArimaPathsArgs &a, hipStream_t stream)
{
    if (a.n_series <= 0) return;
    ArimaPathsArgs b = a;
    b.ring = a.horizon < 2 * a.m + 5 ? a.horizon : 2 * a.m + 5;
    if (b.ring < 1) b.ring = 1;
    b.yring = a.m < a.horizon ? a.m : 0;
    const int most_waves = arima_paths_waves(2 * b.ring + b.yring);
    b.waves = (a.waves >= 1 && a.waves < most_waves) ? a.waves : most_waves;       // (a.waves: the developer knob, 0 = as many as fit)
    const unsigned gx = (unsigned)(((size_t)a.n_series + 63) / 64);
    hipLaunchKernelGGL(arima_paths_status_kernel, dim3(gx), dim3(64 * AP_SLICES), 0, stream, b);
    if (a.n_paths <= 0 || a.horizon <= 0) return;
    const size_t tiles8 = ((size_t)gx + 7) / 8 * 8;                    // whole sets of 8 tiles; the workgroups of a missing tile return at once
    size_t groups = ((size_t)a.n_paths + (size_t)b.waves - 1) / (size_t)b.waves;
    const size_t most = (size_t)INT32_MAX / tiles8;
    groups = groups > most ? (most > 0 ? most : 1) : groups;
    b.path_groups = (int)groups;
    const size_t lds = (size_t)b.waves * (size_t)(2 * b.ring + b.yring) * 64 * sizeof(double);      // <= 64 KiB
    hipLaunchKernelGGL(arima_paths_kernel, dim3((unsigned)(tiles8 * groups)), dim3(64 * b.waves), lds, stream, b);
    hipLaunchKernelGGL(arima_paths_broken_kernel, dim3(gx), dim3(64 * AP_COUNT_WAVES), 0, stream, b);
}

void launch_arima_innovations(const int32_t *orders, const double *coef, size_t ld, const double *y, const int32_t *lengths, int t_rows, int m,
                              int n_series, double *resid, int32_t *resid_len, double *sigma, hipStream_t stream)
{
    if (n_series <= 0) return;
    hipLaunchKernelGGL(arima_innovations_kernel, dim3((unsigned)(((size_t)n_series + 63) / 64)), dim3(64), 0, stream, orders, coef, ld, y, lengths,
                       t_rows, m, n_series, resid, resid_len, sigma);
}

void launch_arima_fit_state(const int32_t *status, const int32_t *model_code, const int32_t *order, const int32_t *d, const int32_t *D,
                            const int32_t *wlen, const double *x, const double *aicc, size_t ld, int n_series, int32_t *orders, double *coef,
                            hipStream_t stream)
{
    if (n_series <= 0) return;
    hipLaunchKernelGGL(arima_fit_state_kernel, dim3((unsigned)(((size_t)n_series + 255) / 256)), dim3(256), 0, stream, status, model_code, order, d,
                       D, wlen, x, aicc, ld, n_series, orders, coef);
}

} // namespace anofox
