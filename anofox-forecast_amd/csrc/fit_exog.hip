// fit_exog.hip -- ARIMAX: forecasting with exogenous regressors (forecast.rs forecast_with_exog / forecast_arima_with_exog).
// OLS of y on K regressors with an intercept, the in-tree ARIMA (fixed-0.5 AR(1) on first differences, naive below 5 observations)
// on the OLS residuals, plus intercept + sum of beta_j * future_j.  The series block is the time-major fp64 block y[t * ld + s]; the
// regressor block has the same layout per regressor, x[(j * t_rows + t) * ld + s], the future block f[(j * h + i) * ld + s]: one lane
// per series, so the 64 lanes of a wave read 512 contiguous bytes per (regressor, row); lengths are ragged.
// The solver is ours (the reference's is an external crate): centred normal equations, Cholesky in column order without pivoting,
// a column whose pivot falls to 1e-10 of its own sum of squares (or is NaN) is left out everywhere (R's aliased coefficient).
// The arithmetic is restated op for op by tests/exog_ref.py (plain mul / add / div / sqrt, -ffp-contract=off): results are bit-identical.
#include "kernels.hpp"

namespace anofox {

namespace {

constexpr int EX_BLOCK = 64;            // one wave: a workgroup is a group of 64 consecutive series
constexpr double EX_TOL = 1e-10;        // pivot threshold relative to the column's centred sum of squares

// rows loaded ahead per step of a sweep: (K + 1) loads per row, 16 to 18 doubles of staging for every K
template <int K> struct ExRows { static constexpr int value = (K + 1) <= 2 ? 8 : ((K + 1) <= 4 ? 4 : ((K + 1) <= 6 ? 3 : 2)); };

// rows [t0, t0 + R) of the series and of its K regressors, range-checked against the series' own length
template <int K, int R>
__device__ __forceinline__ void ex_load(const double *y, const double *x, size_t ld, size_t reg_stride, int t0, int n, double (&yb)[R], double (&xb)[K][R])
{
#pragma unroll
    for (int u = 0; u < R; u++) {
        const bool in = t0 + u < n;
        const size_t row = (size_t)(t0 + u) * ld;
        yb[u] = in ? y[row] : 0.0;
#pragma unroll
        for (int j = 0; j < K; j++) xb[j][u] = in ? x[(size_t)j * reg_stride + row] : 0.0;
    }
}

// Three sweeps per series, everything between them in registers (every index below is a compile-time constant once unrolled):
//   1  the K + 1 means;  2  the centred Gram triangle S and g = X'y, then Cholesky and the two substitutions;
//   3  the residuals on the fly (never stored): running sum of their differences and the last two, then the h forecasts.
template <int K>
__global__ __launch_bounds__(EX_BLOCK) void exog_arimax_kernel(const ExogArgs a)
{
    constexpr int R = ExRows<K>::value;
    const int s = blockIdx.x * EX_BLOCK + threadIdx.x;
    if (s >= a.n_series) return;
    const int n = a.len[s];
    if (n <= 0 || (size_t)n > a.t_rows) return;     // (not part of this group / a block too short for the series: never read past it)
    const size_t ld = a.ld, reg_stride = a.t_rows * ld;
    const double *y = a.y + s, *x = a.x + s;
    const double dn = (double)n;

    // ---- sweep 1: means
    double ybar = 0.0, xbar[K];
#pragma unroll
    for (int j = 0; j < K; j++) xbar[j] = 0.0;
    for (int t0 = 0; t0 < n; t0 += R) {
        double yb[R], xb[K][R];
        ex_load<K, R>(y, x, ld, reg_stride, t0, n, yb, xb);
#pragma unroll
        for (int u = 0; u < R; u++) {
            if (t0 + u >= n) break;
            ybar = ybar + yb[u];
#pragma unroll
            for (int j = 0; j < K; j++) xbar[j] = xbar[j] + xb[j][u];
        }
    }
    ybar = ybar / dn;
#pragma unroll
    for (int j = 0; j < K; j++) xbar[j] = xbar[j] / dn;

    // ---- sweep 2: S (lower triangle, row j at L[j * (j + 1) / 2 + k]) and g
    double L[K * (K + 1) / 2], g[K];
#pragma unroll
    for (int i = 0; i < K * (K + 1) / 2; i++) L[i] = 0.0;
#pragma unroll
    for (int j = 0; j < K; j++) g[j] = 0.0;
    for (int t0 = 0; t0 < n; t0 += R) {
        double yb[R], xb[K][R];
        ex_load<K, R>(y, x, ld, reg_stride, t0, n, yb, xb);
#pragma unroll
        for (int u = 0; u < R; u++) {
            if (t0 + u >= n) break;
            const double dy = yb[u] - ybar;
            double d[K];
#pragma unroll
            for (int j = 0; j < K; j++) d[j] = xb[j][u] - xbar[j];
#pragma unroll
            for (int j = 0; j < K; j++) {
                g[j] = g[j] + d[j] * dy;
#pragma unroll
                for (int k = 0; k <= j; k++) L[j * (j + 1) / 2 + k] = L[j * (j + 1) / 2 + k] + d[j] * d[k];
            }
        }
    }

    // ---- Cholesky in place, column by column; an unused column is never multiplied again
    uint32_t used = 0u;
#pragma unroll
    for (int j = 0; j < K; j++) {
        const double sjj = L[j * (j + 1) / 2 + j];
        double v = sjj;
#pragma unroll
        for (int k = 0; k < j; k++)
            if (used & (1u << k)) v = v - L[j * (j + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
        if (!(v > EX_TOL * sjj)) continue;
        used |= 1u << j;
        const double ljj = sqrt(v);
        L[j * (j + 1) / 2 + j] = ljj;
#pragma unroll
        for (int i = j + 1; i < K; i++) {
            double w = L[i * (i + 1) / 2 + j];
#pragma unroll
            for (int k = 0; k < j; k++)
                if (used & (1u << k)) w = w - L[i * (i + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
            L[i * (i + 1) / 2 + j] = w / ljj;
        }
    }
    // forward substitution L z = g (z over g), back substitution L' beta = z
    double beta[K];
#pragma unroll
    for (int j = 0; j < K; j++) {
        beta[j] = 0.0;
        if (!(used & (1u << j))) continue;
        double w = g[j];
#pragma unroll
        for (int k = 0; k < j; k++)
            if (used & (1u << k)) w = w - L[j * (j + 1) / 2 + k] * g[k];
        g[j] = w / L[j * (j + 1) / 2 + j];
    }
#pragma unroll
    for (int j = K - 1; j >= 0; j--) {
        if (!(used & (1u << j))) continue;
        double w = g[j];
#pragma unroll
        for (int i = j + 1; i < K; i++)
            if (used & (1u << i)) w = w - L[i * (i + 1) / 2 + j] * beta[i];
        beta[j] = w / L[j * (j + 1) / 2 + j];
    }
    double b0 = ybar;
#pragma unroll
    for (int j = 0; j < K; j++)
        if (used & (1u << j)) b0 = b0 - beta[j] * xbar[j];

    // ---- sweep 3: residuals r_t = y_t - (b0 + sum beta_j x_jt), the in-tree ARIMA on them (forecast.rs:1391-1431)
    double sum_diff = 0.0, r_last = 0.0, r_prev = 0.0;
    for (int t0 = 0; t0 < n; t0 += R) {
        double yb[R], xb[K][R];
        ex_load<K, R>(y, x, ld, reg_stride, t0, n, yb, xb);
#pragma unroll
        for (int u = 0; u < R; u++) {
            if (t0 + u >= n) break;
            double e = b0;
#pragma unroll
            for (int j = 0; j < K; j++)
                if (used & (1u << j)) e = e + beta[j] * xb[j][u];
            const double r = yb[u] - e;
            if (t0 + u > 0) sum_diff = sum_diff + (r - r_last);
            r_prev = r_last;
            r_last = r;
        }
    }
    const double mean_diff = sum_diff / (double)(n - 1);
    double prev = r_last - r_prev, cum = r_last;
    double *out = a.yhat + (size_t)s * a.h;
    const double *f = a.f + s;
    for (int i = 0; i < a.h; i++) {
        double rf = r_last;
        if (n >= 5) {
            const double nd = mean_diff + 0.5 * (prev - mean_diff);
            cum = cum + nd;
            prev = nd;
            rf = cum;
        }
        double e = b0;
#pragma unroll
        for (int j = 0; j < K; j++)
            if (used & (1u << j)) e = e + beta[j] * f[((size_t)j * a.h + i) * ld];
        out[i] = rf + e;
    }
    a.status[s] = 0;
    a.model_code[s] = MODEL_CODE_ARIMAX;
    a.b0[s] = b0;
#pragma unroll
    for (int j = 0; j < K; j++) a.beta[(size_t)j * ld + s] = beta[j];
    a.used[s] = used;
}

} // namespace

void launch_exog_arimax(const ExogArgs &a, hipStream_t stream)
{
    if (a.n_series <= 0) return;
    const dim3 grid((unsigned)((a.n_series + EX_BLOCK - 1) / EX_BLOCK)), block(EX_BLOCK);
    switch (a.k) {
    case 1: hipLaunchKernelGGL(exog_arimax_kernel<1>, grid, block, 0, stream, a); break;
    case 2: hipLaunchKernelGGL(exog_arimax_kernel<2>, grid, block, 0, stream, a); break;
    case 3: hipLaunchKernelGGL(exog_arimax_kernel<3>, grid, block, 0, stream, a); break;
    case 4: hipLaunchKernelGGL(exog_arimax_kernel<4>, grid, block, 0, stream, a); break;
    case 5: hipLaunchKernelGGL(exog_arimax_kernel<5>, grid, block, 0, stream, a); break;
    case 6: hipLaunchKernelGGL(exog_arimax_kernel<6>, grid, block, 0, stream, a); break;
    case 7: hipLaunchKernelGGL(exog_arimax_kernel<7>, grid, block, 0, stream, a); break;
    case 8: hipLaunchKernelGGL(exog_arimax_kernel<8>, grid, block, 0, stream, a); break;
    default: throw std::runtime_error("ARIMAX: the number of regressors must be 1 to 8");
    }
}

} // namespace anofox
