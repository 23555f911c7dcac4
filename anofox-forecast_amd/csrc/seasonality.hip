// seasonality.hip -- the reference's ts_detect_seasonality / ts_analyze_seasonality (seasonality.rs detect_seasonality,
// analyze_seasonality, compute_trend_strength) for every series of a time-major block, one workgroup per series.
//
// The contract is equality of bits with the source: which lags are peaks and in which order they come are step
// functions of the autocorrelation sums, so every sum runs in the source's order -- over i ascending, from 0.0, one accumulator,
// multiply and add separate (-ffp-contract=off; nothing in this file is fused) -- and the division and the square root are the
// correctly rounded ones.
//
//   1. the non-NULL values are compacted into the working buffer c in arrival order (`valid` may be null: a plain copy).  With a mask
//      every wave counts its own run of rows, then writes behind the waves before it (ballot + prefix count); n is the count
//   2. n < 4: SEASONALITY_SHORT, nothing else.  max_lag = min(max_period > 0 ? max_period : n / 2, n / 2)
//   3. the mean: ONE lane, the sequential sum.  It is the only chain the lag loop has to wait for.  All lanes centre c and clear
//      SE_PAD words behind it
//   4. side by side: waves 0 .. 3 run the lag sums, wave 4 the three remaining serial chains -- lane 0 the variance sum of d * d,
//      lane 1 ss_xy, lane 2 ss_xx, in one loop (one serial chain per lane, each in its own order; ss_yy of the trend strength is the
//      variance chain, the same operations on the same operands).  That wave issues one short dependent step per row and leaves the
//      SIMD it shares to a lag wave.
//      The lag loop: a wave owns 64 * SE_G consecutive lags; lane t carries the SE_G lags base + 1 + t + 64 k through ONE loop over
//      i, so the broadcast operand c[i] is read once for SE_G products and the other operand is 64 consecutive words (no bank
//      conflict).  The loop runs to the wave's longest sum; a lane whose own sum has ended multiplies by the zero tail, and x + (+-0.0)
//      leaves every bit of a sum that began at +0.0 as it is (such a sum is never -0.0).  With a non-finite value in c the mean, and
//      with it every c[i] and the variance, is non-finite, every ACF value is NaN with or without the tail, and nothing is a peak.
//   5. one barrier later: the sums are divided by the variance (all lanes), then wave 0 picks up to five peaks, each round the
//      largest remaining ACF value and among equal ones the smallest lag -- the order the source's stable descending sort leaves --
//      and lane 0 forms the strengths and the trend strength
//
// c and the lag sums live in dynamic LDS sized from the block's t_rows (seasonality_kernel<true>, t_rows <= SEASONALITY_LDS_ROWS)
// or in a slice of a global workspace (seasonality_kernel<false>); the body is the same, and so are the figures.  No scratch.
//
// ANOFOX_SEAS_LAGS (an experiment build only, tools/time_seasonality.py --ab): the lags per lane, SE_G.  Every value gives the same
// bits; the product is built with the default.
#include "kernels.hpp"

#ifndef ANOFOX_SEAS_LAGS
#define ANOFOX_SEAS_LAGS 4
#endif

namespace anofox {

namespace {

constexpr int SE_G = ANOFOX_SEAS_LAGS;                   // lags per lane of the lag loop
constexpr int SE_LAG_WAVES = 4;
constexpr int SE_WAVES = SE_LAG_WAVES + 1;               // the last wave runs the serial chains
constexpr int SE_THREADS = 64 * SE_WAVES;
constexpr int SE_PAD = 64 * SE_G;                        // zero words behind c: the furthest read is c[n + 64 SE_G - 2]
constexpr double SE_EPS = 2.220446049250313e-16;         // f64::EPSILON
static_assert(SE_G >= 1 && SE_G <= 8, "lags per lane");

__host__ __device__ __forceinline__ size_t se_stride(int t_rows)
{
    const size_t t = t_rows > 0 ? (size_t)t_rows : 0;
    return t + SE_PAD + t / 2 + 2;
}

// (v1, i1) comes before (v2, i2) in the source's order: larger ACF first, equal ACF by ascending lag; i == 0 is "none"
__device__ __forceinline__ bool se_before(double v1, int i1, double v2, int i2)
{
    return i1 != 0 && (i2 == 0 || v1 > v2 || (v1 == v2 && i1 < i2));
}

template <bool USE_LDS>
__global__ __launch_bounds__(SE_THREADS) void seasonality_kernel(const SeasonalityArgs a)
{
    extern __shared__ double se_lds[];
    __shared__ double sh_chain[4];                       // mean, variance sum, ss_xy, ss_xx
    __shared__ int sh_cnt[SE_WAVES];
    __shared__ int32_t sh_oi[SEASONALITY_N_INT];
    __shared__ double sh_of[SEASONALITY_N_FP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t ld = a.ld;
    double *c = USE_LDS ? se_lds : a.work + (size_t)blockIdx.x * se_stride(a.t_rows);
    double *acf = c + a.t_rows + SE_PAD;

    for (int s = blockIdx.x; s < a.n_series; s += gridDim.x) {
        int n_rows = a.len[s];
        n_rows = n_rows < 0 ? 0 : n_rows > a.t_rows ? a.t_rows : n_rows;
        if (tid < SEASONALITY_N_INT) sh_oi[tid] = 0;
        if (tid < SEASONALITY_N_FP) sh_of[tid] = 0.0;

        // ---- 1. load, compact ----
        int n = n_rows;
        if (!a.valid) {
            for (int i = tid; i < n_rows; i += SE_THREADS) c[i] = a.y[(size_t)i * ld + s];
        } else {
            const int per = ((n_rows + 63) / 64 + SE_WAVES - 1) / SE_WAVES * 64;      // rows per wave, whole chunks of 64
            const int r0 = wave * per < n_rows ? wave * per : n_rows, r1 = r0 + per < n_rows ? r0 + per : n_rows;
            int cnt = 0;
            for (int t0 = r0; t0 < r1; t0 += 64) {
                const int tl = t0 + lane;
                cnt += __popcll(__ballot(tl < r1 && a.valid[(size_t)tl * ld + s] != 0));
            }
            if (lane == 0) sh_cnt[wave] = cnt;
            __syncthreads();
            int k = 0;
            n = 0;
            for (int w = 0; w < SE_WAVES; w++) { if (w < wave) k += sh_cnt[w]; n += sh_cnt[w]; }
            for (int t0 = r0; t0 < r1; t0 += 64) {
                const int tl = t0 + lane;
                const bool keep = tl < r1 && a.valid[(size_t)tl * ld + s] != 0;
                const uint64_t mask = __ballot(keep);
                if (keep) c[k + __popcll(mask & ((1ull << lane) - 1ull))] = a.y[(size_t)tl * ld + s];
                k += __popcll(mask);
            }
        }
        __syncthreads();

        if (n < 4) {
            if (tid == 0) sh_oi[7] = SEASONALITY_SHORT;
        } else {
            // ---- 3. the mean, then centre ----
            if (tid == 64 * SE_LAG_WAVES) {
                double sum = 0.0;
#pragma unroll 8
                for (int i = 0; i < n; i++) sum += c[i];
                sh_chain[0] = sum / (double)n;
            }
            __syncthreads();
            const double mean = sh_chain[0];
            for (int i = tid; i < n; i += SE_THREADS) c[i] = c[i] - mean;
            for (int i = tid; i < SE_PAD; i += SE_THREADS) c[n + i] = 0.0;
            __syncthreads();

            const int half = n / 2;
            const int max_lag = a.max_period > 0 && a.max_period < half ? a.max_period : half;
            const bool lags = max_lag >= 2;

            // ---- 4. the serial chains beside the lag sums ----
            if (wave == SE_LAG_WAVES) {
                if (lane < 3) {
                    const double x_mean = ((double)n - 1.0) / 2.0;
                    double acc = 0.0;
#pragma unroll 8
                    for (int i = 0; i < n; i++) {
                        const double d = c[i], x = (double)i - x_mean;
                        const double p = lane == 0 ? d : x, q = lane == 2 ? x : d;      // d * d, x * d, x * x
                        acc += p * q;
                    }
                    sh_chain[1 + lane] = acc;
                }
            } else if (lags) {
                for (int base = wave * 64 * SE_G; base < max_lag; base += SE_LAG_WAVES * 64 * SE_G) {
                    const int cnt = n - (base + 1);          // the sum of lag base + 1, the longest of this wave's
                    const double *q = c + base + 1 + lane;
                    double sum[SE_G];
#pragma unroll
                    for (int k = 0; k < SE_G; k++) sum[k] = 0.0;
#pragma unroll 4
                    for (int i = 0; i < cnt; i++) {
                        const double x = c[i];
#pragma unroll
                        for (int k = 0; k < SE_G; k++) sum[k] += x * q[i + 64 * k];
                    }
#pragma unroll
                    for (int k = 0; k < SE_G; k++) {
                        const int lag = base + 1 + lane + 64 * k;
                        if (lag <= max_lag) acf[lag - 1] = sum[k];
                    }
                }
            }
            __syncthreads();

            // ---- 5. divide, pick the peaks, the strengths and the trend ----
            const double var = sh_chain[1];
            const bool have = lags && !(fabs(var) < SE_EPS);
            if (have)
                for (int j = tid; j < max_lag; j += SE_THREADS) acf[j] = acf[j] / var;
            __syncthreads();
            if (wave == 0) {
                int n_periods = 0;
                double last_v = 0.0;
                int last_i = 0;
                if (have) {
                    for (int r = 0; r < SEASONALITY_TOP; r++) {
                        double bv = 0.0;
                        int bi = 0;
                        for (int i = 1 + lane; i + 1 < max_lag; i += 64) {
                            const double v = acf[i];
                            if (v > acf[i - 1] && v > acf[i + 1] && v > 0.1 && (r == 0 || se_before(last_v, last_i, v, i)) &&
                                (bi == 0 || v > bv)) { bv = v; bi = i; }
                        }
#pragma unroll
                        for (int o = 32; o >= 1; o >>= 1) {
                            const double ov = __shfl_xor(bv, o);
                            const int oi = __shfl_xor(bi, o);
                            if (se_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
                        }
                        if (bi == 0) break;
                        if (lane == 0) {
                            const double strength = fabs(var) > SE_EPS ? (bv < 0.0 ? 0.0 : bv > 1.0 ? 1.0 : bv) : 0.0;
                            sh_oi[r] = bi + 1;
                            sh_of[r] = strength;
                            sh_of[SEASONALITY_TOP + r] = bv;
                            if (r == 0) { sh_oi[6] = bi + 1; sh_of[10] = strength; }
                        }
                        last_v = bv; last_i = bi;
                        n_periods = r + 1;
                    }
                }
                if (lane == 0) {
                    const double ss_xy = sh_chain[2], ss_xx = sh_chain[3], ss_yy = var;
                    double trend = 0.0;
                    if (!(fabs(ss_xx) < SE_EPS || fabs(ss_yy) < SE_EPS)) {
                        const double r = sqrt(ss_xy * ss_xy / (ss_xx * ss_yy));
                        trend = r < 0.0 ? 0.0 : r > 1.0 ? 1.0 : r;       // Rust's clamp: a NaN stays
                    }
                    sh_oi[5] = n_periods;
                    sh_of[11] = trend;
                }
            }
        }
        __syncthreads();
        if (tid < SEASONALITY_N_INT) a.out_int[(size_t)tid * ld + s] = sh_oi[tid];
        else if (tid >= 64 && tid < 64 + SEASONALITY_N_FP) a.out_fp[(size_t)(tid - 64) * ld + s] = sh_of[tid - 64];
        __syncthreads();                                     // the next series overwrites c and the result words
    }
}

} // namespace

size_t seasonality_work_stride(int t_rows) { return se_stride(t_rows); }

size_t seasonality_work_doubles(int n_series, int t_rows)
{
    if (t_rows <= SEASONALITY_LDS_ROWS || n_series <= 0) return 0;
    return (size_t)std::min(n_series, SEASONALITY_LONG_GRID) * seasonality_work_stride(t_rows);
}

void launch_seasonality(const SeasonalityArgs &a, hipStream_t stream)
{
    if (a.n_series <= 0) return;
    if (a.t_rows <= SEASONALITY_LDS_ROWS) {
        const size_t bytes = sizeof(double) * seasonality_work_stride(a.t_rows);
        if (bytes > 48 * 1024)
            anofox_check_attr(hipFuncSetAttribute((const void *)seasonality_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        hipLaunchKernelGGL(seasonality_kernel<true>, dim3((unsigned)std::min(a.n_series, 65536)), dim3(SE_THREADS), bytes, stream, a);
    } else {
        hipLaunchKernelGGL(seasonality_kernel<false>, dim3((unsigned)std::min(a.n_series, SEASONALITY_LONG_GRID)), dim3(SE_THREADS), 0, stream, a);
    }
}

} // namespace anofox
