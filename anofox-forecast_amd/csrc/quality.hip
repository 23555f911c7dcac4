// quality.hip -- the eight data quality figures of the reference's ts_data_quality (quality.rs compute_data_quality as its FFI entry
// calls it: without dates, so n_gaps = 0 and temporal_score = 1) for every series of a time-major block, one wavefront per series.
//
// The contract is equality of bits with the source: the five scores are step functions of three counts and
// three comparisons (< EPSILON, > 0.95, > 4 std), so every floating-point sum runs in the source's order -- left to right over the
// non-NULL values, from 0.0 -- powi(2) is one multiplication, no operation is fused (-ffp-contract=off) and sqrt is the correctly
// rounded one.  The mean is formed once (the source forms the same bits three times); the centred sum of squares serves the
// deviation of magnitude_score, the variance of behavioral_score and the denominator of its autocorrelation, which are one chain.
//
//   1. load the series once (lane = row), compact the non-NULL values into the wave's buffer in arrival order (ballot + prefix
//      count), note a NaN
//   2. constancy: every |x_i - x_0| < EPSILON, all lanes (order-free)
//   3. the in-order sums.  Every lane walks the buffer from 0 to k - 1 with the same index (one broadcast read per value) and
//      carries the same running sum: first the sum, then, with the mean, the centred squares and the lag-1 products interleaved
//      (two independent add chains).  Nothing is reordered; the 64 lanes hold 64 copies of one serial computation.
//   4. the values become keys of the total order of wave_sort.hpp and are sorted in place by the bitonic network; q1 and q3 are two
//      reads, the outliers and the extremes two ballot counts over the sorted buffer (order-free).  -0.0 sorts below +0.0 where
//      the source's stable sort keeps arrival order: that can only change the sign of a zero q1 or q3, which no comparison sees.
//
// The buffer is `tile` words of dynamic LDS per wave (quality_kernel; the host sizes the tile from the batch's longest series, a
// power of two of at most QUALITY_RESIDENT = 2,048 words, and fits 64 KiB / tile bytes waves -- at most 16 -- into a workgroup) or a
// slice of a global workspace (quality_long_kernel, series above 2,048 rows; a fixed number of waves walks them).  The body is the
// same.
//
// Status per series: QUALITY_OK; QUALITY_NAN a valid value is NaN -- the source's sort_by(partial_cmp().unwrap_or(Equal)) leaves
// the order of such a vector to its sort's internals, so the five scores are NaN here; the counts and is_constant are written.
// +-inf are ordinary values and follow the source's arithmetic.
//
// ANOFOX_QUALITY_SKIP (an experiment build only, tools/time_quality.py --ab): bit 0 leaves out the sorting network of step 4, bit 1
// the in-order chains of step 3, so that the time of each can be read from the difference.  The figures of such a build are wrong
// by design; the product is built without the switch.
#include "kernels.hpp"
#include "det_math.hpp"
#include "wave_sort.hpp"

#ifndef ANOFOX_QUALITY_SKIP
#define ANOFOX_QUALITY_SKIP 0
#endif

namespace anofox {

namespace {

constexpr int QL_MAX_WAVES = 16;
constexpr int QL_LONG_WAVES = 4;
constexpr size_t QL_LDS_BYTES = 64 * 1024;               // dynamic LDS a workgroup may ask for without raising the limit
constexpr double QL_EPS = 2.220446049250313e-16;         // f64::EPSILON

__device__ __forceinline__ int ql_length(const QualityArgs &a, int s)
{
    int n = a.len[s];
    if (n < 0) n = 0;
    if ((size_t)n > a.t_rows) n = (int)a.t_rows;
    return n;
}

__device__ __forceinline__ double ql_clamp01(double x) { return x < 0.0 ? 0.0 : x > 1.0 ? 1.0 : x; }

// all figures of series s (n rows, n <= capacity of buf)
template <class B>
__device__ __forceinline__ void ql_series(const QualityArgs &a, int s, int n, B buf, int lane)
{
    const size_t ld = a.ld;
    double structural = 0.0, temporal = 0.0, magnitude = 0.0, behavioral = 0.0, overall = 0.0;
    int64_t n_missing = 0, constant = 0, status = QUALITY_OK;

    if (n > 0) {                                             // n == 0: DataQuality::default()
        // ---- 1. load, compact ----
        int k = 0;
        bool has_nan = false;
        for (int t0 = 0; t0 < n; t0 += 64) {
            const int tl = t0 + lane;
            const bool in = tl < n;
            const double v = in ? a.y[(size_t)tl * ld + s] : 0.0;
            const bool keep = in && (!a.valid || a.valid[(size_t)tl * ld + s] != 0);
            const uint64_t mask = __ballot(keep);
            if (__ballot(keep && v != v)) has_nan = true;
            if (keep) buf[k + __popcll(mask & ((1ull << lane) - 1ull))] = dm_bits(v);
            k += __popcll(mask);
        }
        st_sync();
        n_missing = n - k;
        const double kf = (double)k;

        // ---- 2. constancy ----
        bool differs = false;
        if (k >= 2) {
            const double first = dm_from_bits(buf[0]);
            for (int c0 = 0; c0 < k; c0 += 64) {
                const int i = c0 + lane;
                const bool in = i < k;
                const double v = in ? dm_from_bits(buf[i]) : first;
                if (__ballot(in && !(fabs(v - first) < QL_EPS))) differs = true;
            }
        }
        constant = differs ? 0 : 1;
        temporal = 1.0;                                      // clamp(1 - (0 / n) * 5)

        if (has_nan) {
            status = QUALITY_NAN;
            structural = temporal = magnitude = behavioral = overall = __builtin_nan("");
        } else if (k == 0) {
            behavioral = 0.5;                                // structural and magnitude stay 0
            overall = (structural + temporal + magnitude + behavioral) / 4.0;
        } else {
            const double completeness = kf / (double)(k + (int)n_missing);
            const double by30 = kf / 30.0;
            const double length_factor = by30 < 1.0 ? by30 : 1.0;
            structural = ql_clamp01(completeness * 0.7 + length_factor * 0.3);

            // ---- 3. the in-order sums: one serial computation, the same in every lane ----
            double sum = 0.0, denom = 0.0, num = 0.0;
            if (!(ANOFOX_QUALITY_SKIP & 2)) {
#pragma unroll 8
                for (int i = 0; i < k; i++) sum += dm_from_bits(buf[i]);
            }
            const double mean = sum / kf;
            if (!(ANOFOX_QUALITY_SKIP & 2)) {
                double prev = 0.0;
#pragma unroll 8
                for (int i = 0; i < k; i++) {
                    const double d = dm_from_bits(buf[i]) - mean;
                    denom += d * d;
                    if (i >= 1) num += d * prev;
                    prev = d;
                }
            }
            const double variance = denom / kf;
            const double sd = sqrt(variance);
            if (k < 3) behavioral = 0.5;
            else if (fabs(variance) < QL_EPS) behavioral = 0.0;
            else {
                const double acf1 = fabs(denom) < QL_EPS ? 0.0 : num / denom;
                behavioral = fabs(acf1) > 0.95 ? 1.0 - 0.2 : 1.0 - 0.0;      // (1.0 - acf_penalty), inside [0, 1] as it is
            }

            // ---- 4. sort, quartiles, the two counts ----
            st_sync();                                       // every lane has read the arrival order
            int p2 = 1;
            while (p2 < k) p2 <<= 1;
            for (int i = lane; i < p2; i += 64) buf[i] = i < k ? st_key(buf[i]) : ~0ull;
            st_sync();
            if (!(ANOFOX_QUALITY_SKIP & 1)) st_sort(buf, p2, lane);
            const int i1 = (int)(kf * 0.25), i3 = (int)(kf * 0.75);
            const double q1 = st_unkey(buf[i1]), q3 = st_unkey(buf[i3]);
            const double iqr = q3 - q1;
            const double lower = q1 - 1.5 * iqr, upper = q3 + 1.5 * iqr;
            const double far = 4.0 * sd;
            int outliers = 0, extreme = 0;
            for (int c0 = 0; c0 < k; c0 += 64) {
                const int i = c0 + lane;
                const bool in = i < k;
                const double v = in ? st_unkey(buf[i]) : 0.0;
                outliers += __popcll(__ballot(in && (v < lower || v > upper)));
                extreme += __popcll(__ballot(in && fabs(v - mean) > far));
            }
            const double outlier_ratio = (double)outliers / kf, extreme_ratio = (double)extreme / kf;
            magnitude = ql_clamp01(1.0 - outlier_ratio * 2.0 - extreme_ratio * 3.0);
            overall = (structural + temporal + magnitude + behavioral) / 4.0;
        }
    }
    if (lane == 0) {
        a.out_fp[0 * ld + s] = structural;
        a.out_fp[1 * ld + s] = temporal;
        a.out_fp[2 * ld + s] = magnitude;
        a.out_fp[3 * ld + s] = behavioral;
        a.out_fp[4 * ld + s] = overall;
        a.out_int[0 * ld + s] = 0;
        a.out_int[1 * ld + s] = n_missing;
        a.out_int[2 * ld + s] = constant;
        a.out_int[3 * ld + s] = status;
    }
}

// series of at most `tile` rows, the buffer in LDS: blockDim.x / 64 waves, a.tile words each
__global__ __launch_bounds__(64 * QL_MAX_WAVES) void quality_kernel(const QualityArgs a)
{
    extern __shared__ uint64_t ql_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = blockIdx.x * (int)(blockDim.x >> 6) + wave;
    if (s >= a.n_series) return;                             // (wave-uniform; the kernel has no workgroup barrier)
    const int n = ql_length(a, s);
    if (n > a.tile) return;                                  // quality_long_kernel answers it
    ql_series(a, s, n, ql_lds + (size_t)wave * a.tile, lane);
}

// longer series, the buffer in the global workspace: a.work_waves waves walk them
__global__ __launch_bounds__(64 * QL_LONG_WAVES) void quality_long_kernel(const QualityArgs a)
{
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * QL_LONG_WAVES + (threadIdx.x >> 6);
    if (w >= a.work_waves) return;
    uint64_t *buf = a.work + (size_t)w * a.work_stride;
    for (int s = w; s < a.n_series; s += a.work_waves) {
        const int n = ql_length(a, s);
        if (n <= a.tile || (size_t)n > a.work_stride) continue;
        ql_series(a, s, n, buf, lane);
        st_sync();
    }
}

} // namespace

int quality_tile(size_t t_rows)
{
    int tile = 64;
    while (tile < QUALITY_RESIDENT && (size_t)tile < t_rows) tile <<= 1;
    return tile;
}

size_t quality_work_stride(size_t t_rows)
{
    if (t_rows <= (size_t)QUALITY_RESIDENT) return 0;
    size_t p2 = 1;
    while (p2 < t_rows) p2 <<= 1;
    return p2;
}

int quality_work_waves(int n_series)
{
    return n_series < QUALITY_WORK_WAVES ? n_series : QUALITY_WORK_WAVES;
}

void launch_quality(const QualityArgs &a, hipStream_t stream)
{
    if (a.n_series <= 0) return;
    int waves = (int)(QL_LDS_BYTES / ((size_t)a.tile * sizeof(uint64_t)));
    waves = waves > QL_MAX_WAVES ? QL_MAX_WAVES : waves;
    const size_t lds = (size_t)waves * a.tile * sizeof(uint64_t);
    const int blocks = (a.n_series + waves - 1) / waves;
    hipLaunchKernelGGL(quality_kernel, dim3(blocks), dim3(64 * waves), lds, stream, a);
    if (a.t_rows > (size_t)QUALITY_RESIDENT && a.work && a.work_waves > 0) {
        const int lblocks = (a.work_waves + QL_LONG_WAVES - 1) / QL_LONG_WAVES;
        hipLaunchKernelGGL(quality_long_kernel, dim3(lblocks), dim3(64 * QL_LONG_WAVES), 0, stream, a);
    }
}

} // namespace anofox
