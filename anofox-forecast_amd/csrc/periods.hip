// periods.hip -- period detection per series: the three methods of the reference that are written out in its own tree,
// lomb_scargle (periods.rs:522-644), aic_comparison (:660-786) and sazed_period (:1259-1361).
//
// One wavefront (one workgroup of 64 lanes) per series; the grid walks the batch with a stride, so the SAZED workspace is a
// fixed number of slices whatever n_series is.  The series is staged in LDS, PERIODS_TILE rows at a time: a series of at most
// PERIODS_TILE rows is staged once, a longer one is walked tile by tile with the sums kept in registers.  Lanes take frequencies
// (Lomb-Scargle), candidate periods (AIC) or DFT bins (SAZED), 64 per pass; every lane reads the same y[t], an LDS broadcast, and
// walks t in the source's order, so each of its sums has the source's order of additions.  The mean and the sums of squares are
// the source's sequential sums as well (every lane adds them redundantly from LDS).
//
// What differs from the source is the evaluation of the elementary functions only: sin / cos are per_sincos of det_trig.hpp (two-term
// Cody-Waite reduction by fused multiply-adds, exact in its first step, then fdlibm's kernels on [-pi/4, pi/4]: absolute error below
// 2^-53, which is what these sums need; not below one ulp of a result next to a zero, see det_trig.hpp), ln / exp are det_math.hpp's,
// the power (1 - p)^M of the false-alarm probability is exp(M ln(1 - p)), atan2 is the device library's.  SAZED evaluates the phase
// exactly: the padded length L is a power of two, so (k t) mod L is an integer operation and the angle -2 pi ((k t) mod L) / L is
// rounded once.  The inner sum of the DFT stops at n: the padded tail holds exact zeros.  The contract is therefore a tolerance on
// the figures plus equality of every decision (tests/periods_ref.py).
//
// Decisions: the first strict maximum of the power in frequency order (Lomb-Scargle), the first strict minimum of the AIC, the
// largest peak with ties to the lower bin (the source's stable sort).  A lane keeps the first strict extreme of its own ascending
// indices; lanes are merged by (value, lower index), a total order, so the butterfly's order does not matter.  SAZED's noise floor,
// element len / 2 of the sorted powers, is found by a radix selection on the bit patterns (powers are >= +0.0, whose patterns
// order like the values): 64 counting passes, integer sums.  No atomics, no floating-point reduction across lanes: the same bits
// on every run and through every entry.
//
// Non-finite input does what the source's arithmetic does with it (NaN sums lose every comparison); the one exception is the
// order of NaN powers inside SAZED's median, which the source leaves to its sort.
#include "kernels.hpp"
#include "det_math.hpp"
#include "det_trig.hpp"

namespace anofox {

namespace {

constexpr double PER_PI = 3.14159265358979323846;
constexpr double PER_EPS = 2.2204460492503131e-16;     // f64::EPSILON

__device__ __forceinline__ int per_wave_sum(int v)
{
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// merges (value, index) over the wave: the larger value (SIGN = 1) or the smaller (SIGN = -1) wins, ties go to the lower index; `aux`
// travels with the winner.  Every lane ends with the wave's result.
template <int SIGN>
__device__ __forceinline__ void per_wave_best(double &val, int &idx, double &aux)
{
    for (int o = 32; o >= 1; o >>= 1) {
        const double ov = __shfl_xor(val, o), oa = __shfl_xor(aux, o);
        const int oi = __shfl_xor(idx, o);
        const bool better = SIGN > 0 ? ov > val : ov < val;
        if (better || (ov == val && oi < idx)) { val = ov; idx = oi; aux = oa; }
    }
}

constexpr int STAGE_RAW = 0, STAGE_HANN = 1;

// rows [t0, t0 + PERIODS_TILE) of series s into the tile: the raw values, or SAZED's (v - mean) * Hann window
template <int MODE>
__device__ __forceinline__ void per_stage(double *tile, const PeriodsArgs &a, int s, int n, int t0, double mean)
{
    __syncthreads();                                               // the tile's previous content has been read
    const int rows = n - t0 < PERIODS_TILE ? n - t0 : PERIODS_TILE;
    for (int i = threadIdx.x; i < rows; i += 64) {
        const int t = t0 + i;
        double v = a.y[(size_t)t * a.ld + s];
        if (MODE == STAGE_HANN) {
            double sn, cs;
            per_sincos(2.0 * PER_PI * (double)t / (double)(n - 1), sn, cs);
            v = (v - mean) * (0.5 * (1.0 - cs));
        }
        tile[i] = v;
    }
    __syncthreads();
}

// the source's sequential sum of the series, and of its squared deviations from `mean`; leaves a short series staged (raw)
__device__ __forceinline__ double per_sum(double *tile, const PeriodsArgs &a, int s, int n, bool resident, bool squares, double mean)
{
    double acc = 0.0;
    for (int t0 = 0; t0 < n; t0 += PERIODS_TILE) {
        if (!resident) per_stage<STAGE_RAW>(tile, a, s, n, t0, 0.0);
        const int rows = n - t0 < PERIODS_TILE ? n - t0 : PERIODS_TILE;
        if (squares) {
            for (int i = 0; i < rows; i++) { const double d = tile[i] - mean; acc += d * d; }
        } else {
            for (int i = 0; i < rows; i++) acc += tile[i];
        }
    }
    return acc;
}

__device__ __forceinline__ int per_length(const PeriodsArgs &a, int s)
{
    int n = a.len[s];
    if (n < 0) n = 0;
    if ((size_t)n > a.t_rows) n = (int)a.t_rows;
    return n;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Lomb-Scargle (periods.rs:522-644)
// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void periods_ls_kernel(const PeriodsArgs a)
{
    __shared__ double tile[PERIODS_TILE];
    const int lane = threadIdx.x;
    for (int s = blockIdx.x; s < a.n_series; s += gridDim.x) {      // (uniform over the workgroup)
        const int n = per_length(a, s);
        if (n < 4) {
            if (lane == 0) a.status[s] = PERIODS_TOO_SHORT;
            continue;
        }
        const bool resident = n <= PERIODS_TILE;
        if (resident) per_stage<STAGE_RAW>(tile, a, s, n, 0, 0.0);
        const double nd = (double)n;
        const double mean = per_sum(tile, a, s, n, resident, false, 0.0) / nd;
        const double variance = per_sum(tile, a, s, n, resident, true, mean) / nd;
        if (fabs(variance) < PER_EPS) {
            if (lane == 0) {
                a.out_fp[0 * a.ld + s] = __builtin_nan("");
                a.out_fp[1 * a.ld + s] = __builtin_nan("");
                a.out_fp[2 * a.ld + s] = 0.0;
                a.out_fp[3 * a.ld + s] = 1.0;
                a.out_index[s] = -1;
                a.status[s] = PERIODS_OK;
            }
            continue;
        }
        const double t_span = (double)(n - 1) - 0.0;
        const double min_p = a.min_period > 0.0 ? a.min_period : 2.0;
        const double max_p = a.max_period > 0.0 ? a.max_period : t_span / 2.0;
        const double min_freq = 1.0 / max_p, max_freq = 1.0 / min_p;
        const double freq_step = (max_freq - min_freq) / (double)(a.n_grid - 1);
        double best = 0.0, unused = 0.0;
        int best_i = INT32_MAX;
        for (int64_t i0 = 0; i0 < a.n_grid; i0 += 64) {
            const int64_t i = i0 + lane;
            const double freq = min_freq + (double)i * freq_step;
            const double omega = 2.0 * PER_PI * freq;
            const double omega2 = 2.0 * omega;
            double s2 = 0.0, c2 = 0.0;
            for (int t = 0; t < n; t++) {
                double sn, cs;
                per_sincos(omega2 * (double)t, sn, cs);
                s2 += sn;
                c2 += cs;
            }
            const double tau = atan2(s2, c2) / (2.0 * omega);
            double cos_sum = 0.0, sin_sum = 0.0, cos2_sum = 0.0, sin2_sum = 0.0;
            for (int t0 = 0; t0 < n; t0 += PERIODS_TILE) {
                if (!resident) per_stage<STAGE_RAW>(tile, a, s, n, t0, 0.0);
                const int rows = n - t0 < PERIODS_TILE ? n - t0 : PERIODS_TILE;
                for (int j = 0; j < rows; j++) {
                    const double yc = tile[j] - mean;
                    double sn, cs;
                    per_sincos(omega * ((double)(t0 + j) - tau), sn, cs);
                    cos_sum += yc * cs;
                    sin_sum += yc * sn;
                    cos2_sum += cs * cs;
                    sin2_sum += sn * sn;
                }
            }
            const double power = (fabs(cos2_sum) > PER_EPS && fabs(sin2_sum) > PER_EPS)
                                     ? 0.5 * (cos_sum * cos_sum / cos2_sum + sin_sum * sin_sum / sin2_sum) / variance
                                     : 0.0;
            if (i < a.n_grid && power > best) { best = power; best_i = (int)i; }
        }
        per_wave_best<1>(best, best_i, unused);
        if (lane == 0) {
            const bool found = best_i != INT32_MAX;                // some power exceeded 0.0
            const double best_freq = found ? min_freq + (double)best_i * freq_step : 0.0;
            double fap = 1.0;
            if (best > 0.0) {
                const double prob_single = dm_exp(-best);
                fap = 1.0 - dm_exp((double)a.n_grid * dm_log(1.0 - prob_single));
            }
            a.out_fp[0 * a.ld + s] = best_freq > 0.0 ? 1.0 / best_freq : __builtin_nan("");
            a.out_fp[1 * a.ld + s] = best_freq;
            a.out_fp[2 * a.ld + s] = best;
            a.out_fp[3 * a.ld + s] = fmin(fap, 1.0);
            a.out_index[s] = found ? best_i : -1;
            a.status[s] = PERIODS_OK;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// AIC comparison of one-harmonic sinusoids (periods.rs:660-786)
// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void periods_aic_kernel(const PeriodsArgs a)
{
    __shared__ double tile[PERIODS_TILE];
    const int lane = threadIdx.x;
    for (int s = blockIdx.x; s < a.n_series; s += gridDim.x) {
        const int n = per_length(a, s);
        if (n < 8) {
            if (lane == 0) a.status[s] = PERIODS_TOO_SHORT;
            continue;
        }
        const bool resident = n <= PERIODS_TILE;
        if (resident) per_stage<STAGE_RAW>(tile, a, s, n, 0, 0.0);
        const double nd = (double)n;
        const double min_p = a.min_period > 0.0 ? a.min_period : 2.0;
        const double max_p = a.max_period > 0.0 ? a.max_period : nd / 2.0;
        const double period_step = (max_p - min_p) / (double)(a.n_grid - 1);
        const double mean = per_sum(tile, a, s, n, resident, false, 0.0) / nd;
        const double ss_total = per_sum(tile, a, s, n, resident, true, mean);
        const double kd = 3.0;                                     // 2 * harmonics + 1, one harmonic
        double best = __builtin_huge_val(), best_rss = 0.0;
        int best_i = INT32_MAX;
        for (int64_t i0 = 0; i0 < a.n_grid; i0 += 64) {
            const int64_t i = i0 + lane;
            const double period = min_p + (double)i * period_step;
            const double omega = 2.0 * PER_PI / period;
            double sum_y_cos = 0.0, sum_y_sin = 0.0, sum_cos2 = 0.0, sum_sin2 = 0.0;
            for (int t0 = 0; t0 < n; t0 += PERIODS_TILE) {
                if (!resident) per_stage<STAGE_RAW>(tile, a, s, n, t0, 0.0);
                const int rows = n - t0 < PERIODS_TILE ? n - t0 : PERIODS_TILE;
                for (int j = 0; j < rows; j++) {
                    const double yc = tile[j] - mean;
                    double sn, cs;
                    per_sincos(omega * (double)(t0 + j), sn, cs);
                    sum_y_cos += yc * cs;
                    sum_y_sin += yc * sn;
                    sum_cos2 += cs * cs;
                    sum_sin2 += sn * sn;
                }
            }
            const double ca = fabs(sum_cos2) > PER_EPS ? sum_y_cos / sum_cos2 : 0.0;
            const double cb = fabs(sum_sin2) > PER_EPS ? sum_y_sin / sum_sin2 : 0.0;
            double rss = 0.0;
            for (int t0 = 0; t0 < n; t0 += PERIODS_TILE) {
                if (!resident) per_stage<STAGE_RAW>(tile, a, s, n, t0, 0.0);
                const int rows = n - t0 < PERIODS_TILE ? n - t0 : PERIODS_TILE;
                for (int j = 0; j < rows; j++) {
                    double sn, cs;
                    per_sincos(omega * (double)(t0 + j), sn, cs);
                    const double fitted = mean + ca * cs + cb * sn;
                    const double d = tile[j] - fitted;
                    rss += d * d;
                }
            }
            const double aic = rss > 0.0 ? nd * dm_log(rss / nd) + 2.0 * kd : -__builtin_huge_val();
            if (i < a.n_grid && aic < best) { best = aic; best_i = (int)i; best_rss = rss; }
        }
        per_wave_best<-1>(best, best_i, best_rss);
        if (lane == 0) {
            const int idx = best_i == INT32_MAX ? 0 : best_i;      // no AIC below +inf: the source keeps index 0 and rss 0.0
            a.out_fp[0 * a.ld + s] = min_p + (double)idx * period_step;
            a.out_fp[1 * a.ld + s] = best;
            a.out_fp[2 * a.ld + s] = nd * dm_log(best_rss / nd) + kd * dm_log(nd);
            a.out_fp[3 * a.ld + s] = best_rss;
            a.out_fp[4 * a.ld + s] = ss_total > 0.0 ? 1.0 - best_rss / ss_total : 0.0;
            a.out_index[s] = idx;
            a.status[s] = PERIODS_OK;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// SAZED (periods.rs:1259-1361)
// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void periods_sazed_kernel(const PeriodsArgs a)
{
    __shared__ double tile[PERIODS_TILE];
    __shared__ double spec_lds[PERIODS_SPEC_LDS];
    const int lane = threadIdx.x;
    for (int s = blockIdx.x; s < a.n_series; s += gridDim.x) {
        const int n = per_length(a, s);
        if (n < 16) {
            if (lane == 0) a.status[s] = PERIODS_TOO_SHORT;
            continue;
        }
        // padded length: the next power of two of n * max(pad, 1); a factor beyond the limit is cut first so the product cannot overflow
        int64_t pad = a.s_pad > 0 ? a.s_pad : 4;
        if (pad > PERIODS_SAZED_MAX_PADDED) pad = PERIODS_SAZED_MAX_PADDED;
        const int64_t want = (int64_t)n * pad;
        int64_t L = 1;
        while (L < want) L <<= 1;
        const int64_t half = L / 2;
        const bool in_lds = half <= PERIODS_SPEC_LDS;
        if (L > PERIODS_SAZED_MAX_PADDED || (!in_lds && (a.work == nullptr || (size_t)half > a.work_stride || (int)blockIdx.x >= a.work_blocks))) {
            if (lane == 0) a.status[s] = PERIODS_OVER_LIMIT;
            continue;
        }
        double *spec = in_lds ? spec_lds : a.work + (size_t)blockIdx.x * a.work_stride;
        const bool resident = n <= PERIODS_TILE;
        if (resident) per_stage<STAGE_RAW>(tile, a, s, n, 0, 0.0);
        const double nd = (double)n, Ld = (double)L;
        const double mean = per_sum(tile, a, s, n, resident, false, 0.0) / nd;
        if (resident) per_stage<STAGE_HANN>(tile, a, s, n, 0, mean);
        // power spectrum, bins 1 .. L / 2 - 1 (bin 0 stays 0.0 as in the source)
        if (lane == 0) spec[0] = 0.0;
        const int64_t mask = L - 1;
        for (int64_t k0 = 1; k0 < half; k0 += 64) {
            const int64_t k = k0 + lane;
            double re = 0.0, im = 0.0;
            for (int t0 = 0; t0 < n; t0 += PERIODS_TILE) {
                if (!resident) per_stage<STAGE_HANN>(tile, a, s, n, t0, mean);
                const int rows = n - t0 < PERIODS_TILE ? n - t0 : PERIODS_TILE;
                for (int j = 0; j < rows; j++) {
                    const int64_t m = (k * (int64_t)(t0 + j)) & mask;          // (k t) mod L: the exact phase
                    double sn, cs;
                    per_sincos(-2.0 * PER_PI * (double)m / Ld, sn, cs);
                    const double v = tile[j];
                    re += v * cs;
                    im += v * sn;
                }
            }
            if (k < half) spec[k] = (re * re + im * im) / Ld;
        }
        __syncthreads();                                           // the spectrum is complete (LDS or global, workgroup scope)
        const int64_t min_p = a.s_min > 2 ? a.s_min : 2;
        int64_t max_p = a.s_max > 0 ? a.s_max : n / 2;
        if (max_p > n / 2) max_p = n / 2;
        const int64_t k_min = L / max_p, k_max = L / min_p;
        const int64_t lo = k_min > 1 ? k_min : 1, hi = k_max < half ? k_max : half;
        // the largest local maximum inside the period range; ties to the lower bin
        double best = -1.0, unused = 0.0;
        int best_k = INT32_MAX;
        for (int64_t k = lo + lane; k < hi; k += 64) {
            const double power = spec[k];
            const double period = Ld / (double)k;
            const bool is_peak = (k == 1 || power > spec[k - 1]) && (k + 1 >= half || power > spec[k + 1]);
            if (is_peak && period >= (double)min_p && period <= (double)max_p && power > best) { best = power; best_k = (int)k; }
        }
        per_wave_best<1>(best, best_k, unused);
        // noise floor: element count / 2 of the ascending powers of [lo, hi)
        double noise = 1.0;
        if (hi > lo) {
            int64_t rank = (hi - lo) / 2;
            uint64_t prefix = 0, known = 0;
            for (int bit = 63; bit >= 0; bit--) {
                const uint64_t b = (uint64_t)1 << bit;
                int c = 0;
                for (int64_t k = lo + lane; k < hi; k += 64) {
                    const uint64_t key = dm_bits(spec[k]);
                    c += ((key & known) == prefix && !(key & b)) ? 1 : 0;
                }
                c = per_wave_sum(c);
                if (rank >= c) { rank -= c; prefix |= b; }
                known |= b;
            }
            noise = dm_from_bits(prefix);
        }
        if (lane == 0) {
            const bool found = best_k != INT32_MAX;
            a.out_fp[0 * a.ld + s] = found ? Ld / (double)best_k : __builtin_nan("");
            a.out_fp[1 * a.ld + s] = found ? best : 0.0;
            a.out_fp[2 * a.ld + s] = found ? (noise > 0.0 ? best / noise : best) : 0.0;
            a.out_index[s] = found ? best_k : -1;
            a.status[s] = PERIODS_OK;
        }
        __syncthreads();                                           // the spectrum has been read before the next series overwrites it
    }
}

} // namespace

size_t periods_work_stride(size_t t_rows, int64_t s_pad)
{
    int64_t pad = s_pad > 0 ? s_pad : 4;
    if (pad > PERIODS_SAZED_MAX_PADDED) pad = PERIODS_SAZED_MAX_PADDED;
    const int64_t want = (int64_t)t_rows * pad;                    // t_rows <= 2^31, pad <= 2^24
    int64_t L = 1;
    while (L < want && L < PERIODS_SAZED_MAX_PADDED) L <<= 1;
    const int64_t half = L / 2;
    return half > PERIODS_SPEC_LDS ? (size_t)half : 0;
}

int periods_work_blocks(size_t work_stride, int n_series)
{
    if (!work_stride) return 0;
    size_t blocks = PERIODS_WORK_BYTES / (work_stride * sizeof(double));
    if (blocks < 1) blocks = 1;
    if (blocks > 2048) blocks = 2048;
    if (blocks > (size_t)n_series) blocks = (size_t)n_series;
    return (int)blocks;
}

void launch_periods(const PeriodsArgs &a, hipStream_t stream)
{
    if (a.n_series <= 0) return;
    int blocks = a.n_series;
    if (a.method == PERIODS_SAZED && a.work_blocks > 0 && blocks > a.work_blocks) blocks = a.work_blocks;
    if (a.method == PERIODS_LOMB_SCARGLE) hipLaunchKernelGGL(periods_ls_kernel, dim3(blocks), dim3(64), 0, stream, a);
    else if (a.method == PERIODS_AIC) hipLaunchKernelGGL(periods_aic_kernel, dim3(blocks), dim3(64), 0, stream, a);
    else hipLaunchKernelGGL(periods_sazed_kernel, dim3(blocks), dim3(64), 0, stream, a);
}

} // namespace anofox
