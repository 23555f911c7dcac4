// fit_theta.hip -- the dynamic Theta models: DynamicTheta (DSTM: alpha 0.1, theta 2, l0 = y0) and DynamicOptimizedTheta (DOTM:
// (l0, alpha, theta) by the project's bounded Nelder-Mead), the state-space Theta method of Fiorucci et al. (2016).  One lane per
// series reads the time-major fp64 block y[t * ld + s], so the 64 lanes of a wave read 64 consecutive columns of one row; lengths
// are ragged.  A seasonal period m > 1 goes through theta_season_kernel first (season test + classical multiplicative indices).
// The arithmetic is restated op for op by tests/theta_ref.py (plain mul / add / div, -ffp-contract=off): results are bit-identical.
#include "kernels.hpp"

namespace anofox {

namespace {

constexpr int TH_BLOCK = 64;            // one wave per workgroup
constexpr int TH_ROWS = 8;              // rows loaded ahead per step of a row loop (fit_intermittent.hip: one wave per SIMD is
                                        // latency-bound on its loads, a block of loads in flight hides it)
constexpr int TH_D = 3;                 // DOTM coordinates (l0, alpha, theta)
constexpr int TH_MAX = 200 * TH_D;      // evaluations / iterations (nm.hpp)
constexpr double TH_SEASON_Z = 1.645;   // 90 % one-sided season test

__device__ __forceinline__ double th_lo(int i) { return i == 0 ? -1.0e10 : (i == 1 ? 0.1 : 1.0); }
__device__ __forceinline__ double th_hi(int i) { return i == 0 ? 1.0e10 : (i == 1 ? 0.99 : 1.0e10); }
__device__ __forceinline__ double th_clip(double v, int i)
{
    if (v < th_lo(i)) v = th_lo(i);
    if (v > th_hi(i)) v = th_hi(i);
    return v;
}

// One streamed pass of the dynamic model at (l0, alpha, theta): returns sse / (n - 1) (+inf when not finite).  With `out`, the
// pass continues h steps past the end, feeding mu back as the observation, and writes the forecasts (times the seasonal index of
// their phase when the series is adjusted).
__device__ double theta_pass(const double *y, size_t ld, int n, const double *sidx, int m, bool adj, double l0, double alpha,
                             double theta, double *out, int h)
{
    const double q = 1.0 - alpha;
    const double k = 1.0 - 1.0 / theta;
    double y0 = y[0];
    if (adj) y0 = y0 / sidx[0];
    double level = alpha * y0 + q * l0;
    double mean = y0, A = y0, B = 0.0, p = 1.0, sse = 0.0;
    int ph = m > 1 ? 1 % m : 0;
    for (int t0 = 1; t0 < n; t0 += TH_ROWS) {
        double vb[TH_ROWS];
#pragma unroll
        for (int u = 0; u < TH_ROWS; u++) vb[u] = t0 + u < n ? y[(size_t)(t0 + u) * ld] : 0.0;
#pragma unroll
        for (int u = 0; u < TH_ROWS; u++) {
            const int t = t0 + u;
            if (t >= n) break;
            double x = vb[u];
            if (adj) {
                x = x / sidx[(size_t)ph * ld];
                ph = ph + 1 == m ? 0 : ph + 1;
            }
            p = p * q;
            const double mu = level + k * (A * p + B * (1.0 - p * q) / alpha);
            const double e = x - mu;
            sse = sse + e * e;
            level = alpha * x + q * level;
            B = ((double)(t - 1) * B + 6.0 * (x - mean) / (double)(t + 1)) / (double)(t + 2);
            mean = ((double)t * mean + x) / (double)(t + 1);
            A = mean - B * (double)(t + 2) / 2.0;
        }
    }
    double f = sse / (double)(n - 1);
    if (!isfinite(f)) f = INFINITY;
    if (out) {
        for (int i = 0; i < h; i++) {
            const int t = n + i;
            p = p * q;
            const double mu = level + k * (A * p + B * (1.0 - p * q) / alpha);
            level = alpha * mu + q * level;
            B = ((double)(t - 1) * B + 6.0 * (mu - mean) / (double)(t + 1)) / (double)(t + 2);
            mean = ((double)t * mean + mu) / (double)(t + 1);
            A = mean - B * (double)(t + 2) / 2.0;
            out[i] = adj ? mu * sidx[(size_t)(t % m) * ld] : mu;
        }
    }
    return f;
}

// Season test and classical multiplicative indices of one series (period m = m_col[s], or the batch's m).  Adjusted only when
// n >= 2m, every y > 0, the series is not constant and |r_m| > 1.645 sqrt((1 + 2 sum_{k<m} r_k^2) / n).  The indices of an
// adjusted series rest at sidx[j * ld + s], j < m (the per-phase ratio sums first, in place).
__global__ __launch_bounds__(TH_BLOCK) void theta_season_kernel(const ThetaArgs a)
{
    const int s = blockIdx.x * TH_BLOCK + threadIdx.x;
    if (s >= a.n_series) return;
    const int n = a.len[s];
    a.adjusted[s] = 0;
    const int m = a.m_col ? a.m_col[s] : a.m;
    if (n <= 0 || m <= 1) return;
    const double *y = a.y + s;
    const size_t ld = a.ld;
    double tot = 0.0;
    bool pos = true;
    for (int t = 0; t < n; t++) {
        const double v = y[(size_t)t * ld];
        tot = tot + v;
        pos = pos && v > 0.0;
    }
    if (n < 2 * m || !pos) return;
    const double mean = tot / (double)n;
    double d = 0.0;
    for (int t = 0; t < n; t++) {
        const double dv = y[(size_t)t * ld] - mean;
        d = d + dv * dv;
    }
    if (!(d > 0.0)) return;
    double acc = 0.0, rm = 0.0;
    for (int k = 1; k <= m; k++) {
        double c = 0.0;
        for (int t = k; t < n; t++) c = c + (y[(size_t)t * ld] - mean) * (y[(size_t)(t - k) * ld] - mean);
        const double r = c / d;
        if (k < m) acc = acc + r * r;
        else rm = r;
    }
    const double lim = TH_SEASON_Z * sqrt((1.0 + 2.0 * acc) / (double)n);
    if (!(fabs(rm) > lim)) return;
    double *si = a.sidx + s;
    for (int j = 0; j < m; j++) si[(size_t)j * ld] = 0.0;
    const int hw = m / 2;
    const bool even = (m % 2) == 0;
    double W = 0.0;
    for (int j = 0; j < 2 * hw; j++) W = W + y[(size_t)j * ld];
    int ph = hw % m;
    for (int t = hw; t + hw < n; t++) {
        const double ya = y[(size_t)(t - hw) * ld], yb = y[(size_t)(t + hw) * ld];
        W = W + yb;
        const double tr = even ? (W - 0.5 * ya - 0.5 * yb) / (double)m : W / (double)m;
        si[(size_t)ph * ld] = si[(size_t)ph * ld] + y[(size_t)t * ld] / tr;
        W = W - ya;
        ph = ph + 1 == m ? 0 : ph + 1;
    }
    double ssum = 0.0;
    for (int j = 0; j < m; j++) {
        const int first = hw + ((j - hw) % m + m) % m, last = n - 1 - hw;
        const double cnt = last >= first ? (double)((last - first) / m + 1) : 0.0;
        const double v = si[(size_t)j * ld] / (cnt > 1.0 ? cnt : 1.0);
        si[(size_t)j * ld] = v;
        ssum = ssum + v;
    }
    const double mu = ssum / (double)m;
    for (int j = 0; j < m; j++) si[(size_t)j * ld] = si[(size_t)j * ld] / mu;
    a.adjusted[s] = 1;
}

enum { TP_INIT = 0, TP_REFL = 1, TP_EXP = 2, TP_OC = 3, TP_IC = 4, TP_SHRINK = 5, TP_DONE = 6 };

struct ThSimplex { double x[TH_D + 1][TH_D]; double f[TH_D + 1]; };

__device__ __forceinline__ void th_swap_if(ThSimplex &S, int i, int j, bool c)
{
    const double fi = S.f[i], fj = S.f[j];
    S.f[i] = c ? fj : fi; S.f[j] = c ? fi : fj;
#pragma unroll
    for (int d = 0; d < TH_D; d++) {
        const double xi = S.x[i][d], xj = S.x[j][d];
        S.x[i][d] = c ? xj : xi; S.x[j][d] = c ? xi : xj;
    }
}
// stable: TH_D bubble passes of strict compare-and-swap
__device__ __forceinline__ void th_sort_all(ThSimplex &S)
{
#pragma unroll
    for (int r = 0; r < TH_D; r++)
#pragma unroll
        for (int j = 0; j < TH_D; j++) th_swap_if(S, j, j + 1, S.f[j + 1] < S.f[j]);
}
// replace the worst vertex, one backward bubble pass (the new vertex goes after every equal value)
__device__ __forceinline__ void th_accept(ThSimplex &S, const double (&xn)[TH_D], double fn)
{
#pragma unroll
    for (int d = 0; d < TH_D; d++) S.x[TH_D][d] = xn[d];
    S.f[TH_D] = fn;
#pragma unroll
    for (int j = TH_D; j > 0; j--) th_swap_if(S, j - 1, j, S.f[j] < S.f[j - 1]);
}

// DynamicTheta: one pass at the fixed parameters.  DynamicOptimizedTheta: the Nelder-Mead of oracle/ets.c nm_minimize as a
// per-lane state machine that evaluates exactly ONE point per trip of the loop, so every lane of the wave streams the same rows
// together whatever step of its own iteration it is at (a straight-line iteration would stream one pass per divergent branch).
// Then one final pass at the best vertex writes the forecasts.
__global__ __launch_bounds__(TH_BLOCK) void theta_fit_kernel(const ThetaArgs a)
{
    const int s = blockIdx.x * TH_BLOCK + threadIdx.x;
    if (s >= a.n_series) return;
    const int n = a.len[s];
    if (n <= 0) return;
    const double *y = a.y + s;
    const size_t ld = a.ld;
    const int m = a.m_col ? a.m_col[s] : a.m;
    const bool adj = a.m > 1 && a.adjusted[s] != 0;          // (theta_season_kernel runs only for m > 1)
    const double *si = adj ? a.sidx + s : nullptr;
    double y0 = y[0];
    if (adj) y0 = y0 / si[0];
    double best[TH_D] = {y0, 0.1, 2.0};
    int evals = 0;
    if (a.kind == TK_DOTM) {
        ThSimplex S;
        const double x0[TH_D] = {y0 / 2.0, 0.5, 2.0};
#pragma unroll
        for (int i = 0; i < TH_D; i++) S.x[0][i] = th_clip(x0[i], i);
#pragma unroll
        for (int k = 0; k < TH_D; k++) {
#pragma unroll
            for (int i = 0; i < TH_D; i++) S.x[k + 1][i] = S.x[0][i];
            const double v = S.x[0][k];
            S.x[k + 1][k] = th_clip(v != 0.0 ? 1.05 * v : 0.00025, k);
        }
#pragma unroll
        for (int k = 0; k <= TH_D; k++) S.f[k] = 0.0;
        int phase = n >= 2 ? TP_INIT : TP_DONE, sub = 0, iters = 1;
        double xb[TH_D] = {0.0, 0.0, 0.0}, xr[TH_D] = {0.0, 0.0, 0.0}, fr = 0.0;
        auto begin_iteration = [&]() {
            bool small = true;
#pragma unroll
            for (int k = 1; k <= TH_D; k++) {
#pragma unroll
                for (int i = 0; i < TH_D; i++)
                    if (!(fabs(S.x[k][i] - S.x[0][i]) <= 1.0e-4)) small = false;
                if (!(fabs(S.f[0] - S.f[k]) <= 1.0e-8)) small = false;
            }
            if (evals >= TH_MAX || iters >= TH_MAX || small) { phase = TP_DONE; return; }
#pragma unroll
            for (int i = 0; i < TH_D; i++) {
                double c = S.x[0][i];
#pragma unroll
                for (int k = 1; k < TH_D; k++) c = c + S.x[k][i];
                xb[i] = c / (double)TH_D;
            }
            phase = TP_REFL;
        };
        while (phase != TP_DONE) {
            // the point of this trip: vertex `sub` (INIT / SHRINK) or a trial point of the current iteration
            double pt[TH_D];
            const double ca = phase == TP_REFL ? 2.0 : (phase == TP_EXP ? 3.0 : (phase == TP_OC ? 1.5 : 0.5));
            const double cb = phase == TP_REFL ? 1.0 : (phase == TP_EXP ? 2.0 : 0.5);
#pragma unroll
            for (int i = 0; i < TH_D; i++) {
                const double v = phase == TP_IC ? ca * xb[i] + cb * S.x[TH_D][i] : ca * xb[i] - cb * S.x[TH_D][i];
                const double xs = sub == 0 ? S.x[0][i] : (sub == 1 ? S.x[1][i] : (sub == 2 ? S.x[2][i] : S.x[3][i]));
                pt[i] = (phase == TP_INIT || phase == TP_SHRINK) ? xs : th_clip(v, i);
            }
            const double f = theta_pass(y, ld, n, si, m, adj, pt[0], pt[1], pt[2], nullptr, 0);
            evals++;
            bool end_it = false, shrink = false;
            if (phase == TP_INIT || phase == TP_SHRINK) {
#pragma unroll
                for (int k = 0; k <= TH_D; k++) S.f[k] = sub == k ? f : S.f[k];
                sub++;
                if (sub > TH_D) {
                    th_sort_all(S);
                    if (phase == TP_INIT) begin_iteration();
                    else end_it = true;
                }
            } else if (phase == TP_REFL) {
#pragma unroll
                for (int i = 0; i < TH_D; i++) xr[i] = pt[i];
                fr = f;
                if (f < S.f[0]) phase = TP_EXP;
                else if (f < S.f[TH_D - 1]) { th_accept(S, pt, f); end_it = true; }
                else if (f < S.f[TH_D]) phase = TP_OC;
                else phase = TP_IC;
            } else if (phase == TP_EXP) {
                if (f < fr) th_accept(S, pt, f);
                else th_accept(S, xr, fr);
                end_it = true;
            } else if (phase == TP_OC) {
                if (f <= fr) { th_accept(S, pt, f); end_it = true; }
                else shrink = true;
            } else {
                if (f < S.f[TH_D]) { th_accept(S, pt, f); end_it = true; }
                else shrink = true;
            }
            if (shrink) {
#pragma unroll
                for (int k = 1; k <= TH_D; k++)
#pragma unroll
                    for (int i = 0; i < TH_D; i++) S.x[k][i] = th_clip(S.x[0][i] + 0.5 * (S.x[k][i] - S.x[0][i]), i);
                sub = 1;
                phase = TP_SHRINK;
            }
            if (end_it) { iters++; begin_iteration(); }
        }
#pragma unroll
        for (int i = 0; i < TH_D; i++) best[i] = S.x[0][i];
    }
    double *out = a.yhat + (size_t)s * a.h;
    theta_pass(y, ld, n, si, m, adj, best[0], best[1], best[2], out, a.h);
    bool finite = true;
    for (int i = 0; i < a.h; i++) finite = finite && isfinite(out[i]);
    a.detail[s] = finite ? FIT_OK : FIT_NONFINITE;
    if (a.evals) a.evals[s] = evals;
}

} // namespace

void launch_theta(const ThetaArgs &a, hipStream_t stream)
{
    if (a.n_series <= 0) return;
    const unsigned blocks = (unsigned)((a.n_series + TH_BLOCK - 1) / TH_BLOCK);
    if (a.m > 1) hipLaunchKernelGGL(theta_season_kernel, dim3(blocks), dim3(TH_BLOCK), 0, stream, a);
    hipLaunchKernelGGL(theta_fit_kernel, dim3(blocks), dim3(TH_BLOCK), 0, stream, a);
}

} // namespace anofox
