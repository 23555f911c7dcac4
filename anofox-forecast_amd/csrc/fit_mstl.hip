// fit_mstl.hip -- the MSTL decomposition of the reference (decomposition.rs: stl_decompose, mstl_decompose; moving averages and
// per-phase means, no LOESS) and SeasonalWindowAverage.  One lane per series reads the time-major fp64 block y[t * ld + s], so the
// 64 lanes of a wave read 64 consecutive columns of one row; lengths are ragged.  Every window sum is a fresh sequential sum, as the
// reference writes it (no running sum), so tests/mstl_ref.py restates the kernels op for op (-ffp-contract=off): bit-identical.
#include "kernels.hpp"

namespace anofox {

namespace {

constexpr int MS_BLOCK = 64;            // one wave per workgroup

__device__ __forceinline__ int ms_state(const MstlArgs &a, int n)
{
    if (n <= 0) return a.mode == MSTL_MODE_FAIL ? MSTL_FAILED : MSTL_NOT_APPLIED;
    const bool insufficient = a.n_periods > 0 && a.min_period > 0 && (long long)n < 2LL * a.min_period;
    if (insufficient) return a.mode == MSTL_MODE_FAIL ? MSTL_FAILED : (a.mode == MSTL_MODE_NONE ? MSTL_NOT_APPLIED : MSTL_TREND_ONLY);
    return a.n_periods == 0 ? MSTL_TREND_ONLY : MSTL_APPLIED;
}

// The series after the seasonal components of the stages before `k` are removed, in stage order: y - s_0 - s_1 - ..., where
// s_j = avg_j[t mod p_j] - mean_j (the reference subtracts the stored component in place, stage after stage: the same bits).
// The phases advance with t (no division per row).
struct Deseason {
    int kk = 0;                             // stages taken into account
    int ph[MSTL_MAX_PERIODS], p[MSTL_MAX_PERIODS];
    const double *tab[MSTL_MAX_PERIODS];
    double mu[MSTL_MAX_PERIODS];
    bool on[MSTL_MAX_PERIODS];

    __device__ void init(const MstlArgs &a, int s, int k, int used, int t0)
    {
        kk = k;
#pragma unroll
        for (int i = 0; i < MSTL_MAX_PERIODS; i++) {
            on[i] = i < k && ((used >> i) & 1);
            p[i] = i < a.n_periods ? a.periods[i] : 1;
            ph[i] = on[i] ? t0 % p[i] : 0;
            tab[i] = a.tab + (size_t)a.tab_off[i < a.n_periods ? i : 0] * a.ld + s;
            mu[i] = on[i] ? a.mean[(size_t)i * a.ld + s] : 0.0;
        }
    }
    // value at the current row, then step to the next row
    __device__ __forceinline__ double take(double y, size_t ld)
    {
#pragma unroll
        for (int i = 0; i < MSTL_MAX_PERIODS; i++) {
            if (on[i]) {
                y = y - (tab[i][(size_t)ph[i] * ld] - mu[i]);
                ph[i] = ph[i] + 1 == p[i] ? 0 : ph[i] + 1;
            }
        }
        return y;
    }
};

// sum of the deseasonalised values y'[lo .. hi], sequential left to right (the reference's iter().sum())
__device__ double window_sum(const MstlArgs &a, int s, int k, int used, const double *y, int lo, int hi)
{
    const size_t ld = a.ld;
    double sum = 0.0;
    if (k == 0 || used == 0) {
#pragma unroll 8
        for (int j = lo; j <= hi; j++) sum += y[(size_t)j * ld];
        return sum;
    }
    Deseason d;
    d.init(a, s, k, used, lo);
    for (int j = lo; j <= hi; j++) sum += d.take(y[(size_t)j * ld], ld);
    return sum;
}

}  // namespace

// One stage of mstl_decompose (stage k: the k-th period of the descending list) for every series in the MSTL state whose length
// holds two seasons: the centred moving average of the current series (window p, or p + 1 for an even p; edges held at the first
// and last full window), the per-phase sums of the detrended values in time order (= the reference's phase-major loop: each phase's
// values are visited in increasing t either way), the phase means and the mean of the periodic component.  The phase table avg_k
// goes to a.tab rows [tab_off[k], tab_off[k] + p), the mean to a.mean[k].
__global__ __launch_bounds__(MS_BLOCK) void mstl_season_kernel(const MstlArgs a, int k)
{
    const int s = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (s >= a.n_series) return;
    const int n = a.len[s];
    const int state = ms_state(a, n);
    int used = k == 0 ? 0 : a.used[s];
    if (state != MSTL_APPLIED) return;
    const int p = a.periods[k];
    // (64-bit: the host only gives a phase table to 2 <= p <= t_rows / 2, and a stage without one never runs)
    if (p < 2 || (long long)n < 2LL * p || 2LL * p > (long long)a.t_rows) { if (k == 0) a.used[s] = 0; return; }
    const size_t ld = a.ld;
    const double *y = a.y + s;
    double *tab = a.tab + (size_t)a.tab_off[k] * ld + s;
    const int w = (p % 2 == 0) ? p + 1 : p;
    const int hw = w / 2;
    const double wd = (double)w;
    for (int ph = 0; ph < p; ph++) tab[(size_t)ph * ld] = 0.0;
    Deseason cur;
    cur.init(a, s, k, used, 0);
    int ph = 0;
    for (int t = 0; t < n; t++) {
        const double v = cur.take(y[(size_t)t * ld], ld);
        const int c = t < hw ? hw : (t > n - hw - 1 ? n - hw - 1 : t);
        const double tr = window_sum(a, s, k, used, y, c - hw, c + hw) / wd;
        double *cell = tab + (size_t)ph * ld;
        *cell = *cell + (v - tr);
        ph = ph + 1 == p ? 0 : ph + 1;
    }
    for (int q = 0; q < p; q++) {
        const int count = (n - q + p - 1) / p;
        tab[(size_t)q * ld] = tab[(size_t)q * ld] / (double)count;
    }
    double m = 0.0;
    ph = 0;
    for (int t = 0; t < n; t++) {
        m += tab[(size_t)ph * ld];
        ph = ph + 1 == p ? 0 : ph + 1;
    }
    a.mean[(size_t)k * ld + s] = m / (double)n;
    a.used[s] = used | (1 << k);
}

// The final trend and the outputs.  MSTL state: the moving average of window max(n / 5, 3).min(n) over the deseasonalised series,
// divided by the number of values summed (the reference's (end - start)), edges held; remainder = deseasonalised - trend; seasonal
// slot k = avg_k[t mod p_k] - mean_k where stage k ran (NaN where it did not).  Trend-only state (no periods, or too short in
// "trend" mode): the same window over y divided by the window length (the reference's other loop: an even window sums one value
// more than it divides by).  An empty window range leaves the trend NaN, as the reference's does.  info[s] = state << 8 | used.
__global__ __launch_bounds__(MS_BLOCK) void mstl_final_kernel(const MstlArgs a)
{
    const int s = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (s >= a.n_series) return;
    const int n = a.len[s];
    const int state = ms_state(a, n);
    const int used = (state == MSTL_APPLIED && a.n_periods > 0) ? a.used[s] : 0;
    a.info[s] = state << 8 | used;
    const size_t ld = a.ld, T = a.t_rows;
    const double *y = a.y + s;
    const double nan = __builtin_nan("");
    if (state == MSTL_FAILED || state == MSTL_NOT_APPLIED) {
        for (int t = 0; t < n; t++) {
            a.trend[(size_t)t * ld + s] = nan;
            a.remainder[(size_t)t * ld + s] = nan;
            for (int k = 0; k < a.n_periods; k++) a.seasonal[((size_t)k * T + t) * ld + s] = nan;
        }
        return;
    }
    int w = n / 5 > 3 ? n / 5 : 3;
    if (w > n) w = n;
    const int hw = w / 2;
    const bool any = hw < n - hw;
    const int kk = state == MSTL_APPLIED ? a.n_periods : 0;
    Deseason cur;
    cur.init(a, s, kk, used, 0);
    for (int t = 0; t < n; t++) {
        const double v = cur.take(y[(size_t)t * ld], ld);
        double tr = nan;
        if (any) {
            const int c = t < hw ? hw : (t > n - hw - 1 ? n - hw - 1 : t);
            const double sum = window_sum(a, s, kk, used, y, c - hw, c + hw);
            tr = sum / (state == MSTL_APPLIED ? (double)(2 * hw + 1) : (double)w);
        }
        a.trend[(size_t)t * ld + s] = tr;
        a.remainder[(size_t)t * ld + s] = v - tr;
        for (int k = 0; k < a.n_periods; k++) {
            double sv = nan;
            if ((used >> k) & 1) {
                const int p = a.periods[k];
                sv = a.tab[((size_t)a.tab_off[k] + (size_t)(t % p)) * ld + s] - a.mean[(size_t)k * ld + s];
            }
            a.seasonal[((size_t)k * T + t) * ld + s] = sv;
        }
    }
}

// SeasonalWindowAverage (forecast.rs:1234-1248): p = period.max(2).min(n), the n / p (at least 1) complete seasons that end the series;
// the forecast at step i is the mean of their values at phase i mod p, summed oldest first.
__global__ __launch_bounds__(MS_BLOCK) void swa_kernel(const SimpleArgs a)
{
    const int s = blockIdx.x * MS_BLOCK + threadIdx.x;
    if (s >= a.n_series) return;
    const int n = a.len[s];
    if (n <= 0) return;
    const double *y = a.y + s;
    const size_t ld = a.ld;
    double *out = a.yhat + (size_t)s * a.h;
    int p = a.period < 2 ? 2 : a.period;
    if (p > n) p = n;
    int ns = n / p;
    if (ns < 1) ns = 1;
    const int start = n - ns * p;
    for (int i = 0; i < a.h; i++) {
        if (i >= p) { out[i] = out[i - p]; continue; }
        double sum = 0.0;
        for (int c = 0; c < ns; c++) sum += y[(size_t)(start + c * p + i) * ld];
        out[i] = sum / (double)ns;
    }
    a.status[s] = 0;
}

void launch_mstl(const MstlArgs &a, hipStream_t stream)
{
    if (a.n_series <= 0) return;
    const unsigned blocks = (unsigned)((a.n_series + MS_BLOCK - 1) / MS_BLOCK);
    for (int k = 0; k < a.n_periods; k++) hipLaunchKernelGGL(mstl_season_kernel, dim3(blocks), dim3(MS_BLOCK), 0, stream, a, k);
    hipLaunchKernelGGL(mstl_final_kernel, dim3(blocks), dim3(MS_BLOCK), 0, stream, a);
}

void launch_swa(const SimpleArgs &a, hipStream_t stream)
{
    if (a.n_series <= 0) return;
    const unsigned blocks = (unsigned)((a.n_series + MS_BLOCK - 1) / MS_BLOCK);
    hipLaunchKernelGGL(swa_kernel, dim3(blocks), dim3(MS_BLOCK), 0, stream, a);
}

} // namespace anofox
