// features.hip -- the 117 per-series features of the reference's ts_features (features.rs extract_features) for every series of a
// time-major block.  One wavefront (a workgroup of 64 lanes) per series and FIVE kernels, one per family, so that each is small, is
// tested alone and keeps its registers and LDS readable in tools/resource_usage.py:
//
//   chains  every in-order sum of the source: moments, changes, energy, the linear trends, the ACF / PACF lags, time reversal
//           asymmetry, c3, the chunk means.  It also writes the presence bits and the status.
//   sort    median, the four quantiles, unique and duplicate counts, the reoccurring figures: the shared bitonic network on
//           total-order keys (wave_sort.hpp), then one walk over the runs of equal keys.
//   scan    counts, strikes, peaks, zero crossings, locations, Benford, binned and permutation patterns, Lempel-Ziv.
//   match   sample_entropy and approximate_entropy: O(n^2) template matching, integer counts.
//   dft     all n bins of the source's DFT (ten are reported, all feed the two spectral figures): O(n^2) sin / cos.
//
// Every kernel compacts the non-NULL values of its series into a buffer in arrival order (ballot + prefix count) -- `tile` words of
// dynamic LDS (features_*_kernel, series of at most FEATURES_RESIDENT = 2,048 rows) or a slice of a global workspace
// (features_*_long_kernel, up to 65,536 rows; a fixed number of waves walks those series).  The body is the same.
//
// The contract is equality of bits wherever the source has one answer: a sum runs in the source's order from
// 0.0, products are not fused (-ffp-contract=off), powi(2) is x*x, powi(3) x*(x*x), powi(4) (x*x)*(x*x), sqrt and / are the
// correctly rounded ones.  A serial chain is carried by all 64 lanes at once (64 copies of one computation, one broadcast read per
// value, as quality.hip does); chains of one shape run side by side in lanes instead: the ten ACF lags, the three lags of time
// reversal asymmetry and c3, the chunk means.  Counts are ballots or integer lane sums, so their order does not matter.  The mean
// and the standard deviation every family needs are formed again by the same chain and so have the same bits in every kernel.
// What passes through ln (det_math.hpp) or sin / cos (det_trig.hpp) has a tolerance; the integer counts under them are equal.
//
// Where the source is not deterministic the order is defined: the two reoccurring sums add the distinct bit
// patterns in ascending total order, permutation_entropy adds its six patterns in lexicographic order of the index vector.
//
// Status per series: FEATURES_OK; FEATURES_EMPTY no valid value (every feature NaN, no presence bit); FEATURES_NAN a valid value is
// NaN -- the source's sort_by(partial_cmp().unwrap_or(Equal)) leaves such a vector to its sort's internals -- `length` is written
// and is the only presence bit, every other feature is NaN.  +-inf are ordinary values and follow the source's arithmetic.
#include "kernels.hpp"
#include "det_math.hpp"
#include "det_trig.hpp"
#include "wave_sort.hpp"

namespace anofox {

namespace {

enum {
#define X(id, name, pos) F_##id,
#include "feature_names.inc"
#undef X
    F_COUNT
};
static_assert(F_COUNT == FEATURES_N, "feature_names.inc lists 117 names");

constexpr double FT_EPS = 2.220446049250313e-16;         // f64::EPSILON
constexpr double FT_PI = 3.14159265358979323846;
constexpr int FT_BITS_WORDS = (int)(FEATURES_MAX_ROWS / 64) + 2;

#define FT_NAN __builtin_nan("")
#define FT_V(i) dm_from_bits(buf[(i)])
#define FT_OUT(id, v) a.out_fp[(size_t)F_##id * ld + s] = (v)

__device__ __forceinline__ int ft_length(const FeaturesArgs &a, int s)
{
    int n = a.len[s];
    if (n < 0) n = 0;
    if ((size_t)n > a.t_rows) n = (int)a.t_rows;
    return n;
}

__device__ __forceinline__ long long ft_wave_sum(long long v)
{
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the non-NULL values of series s into buf in arrival order; returns their count
template <class B>
__device__ __forceinline__ int ft_compact(const FeaturesArgs &a, int s, int n, B buf, int lane, bool &has_nan)
{
    const size_t ld = a.ld;
    int k = 0;
    has_nan = false;
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
    return k;
}

// the source's sum, mean, centred sum of squares, minimum and maximum: one serial computation, the same in every lane
template <class B>
__device__ __forceinline__ void ft_moments(B buf, int k, double &sum, double &mean, double &css, double &lo, double &hi)
{
    sum = 0.0;
#pragma unroll 8
    for (int i = 0; i < k; i++) sum += FT_V(i);
    mean = sum / (double)k;
    css = 0.0;
    lo = __builtin_huge_val(); hi = -__builtin_huge_val();
#pragma unroll 4
    for (int i = 0; i < k; i++) {
        const double v = FT_V(i), d = v - mean;
        css += d * d;
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
    }
}

// linear_trend over m values read through `at`: slope, intercept, r squared (and ss_xx for the caller)
template <class At>
__device__ __forceinline__ void ft_linear_trend(int m, double ym, At at, double &slope, double &intercept, double &r2, double &sxx)
{
    const double xm = ((double)m - 1.0) / 2.0;
    double sxy = 0.0, syy = 0.0;
    sxx = 0.0;
    for (int i = 0; i < m; i++) {
        const double dx = (double)i - xm, dy = at(i) - ym;
        sxy += dx * dy;
        sxx += dx * dx;
        syy += dy * dy;
    }
    slope = fabs(sxx) > FT_EPS ? sxy / sxx : 0.0;
    intercept = ym - slope * xm;
    r2 = 0.0;
    if (fabs(sxx) > FT_EPS && fabs(syy) > FT_EPS) {
        const double q = (sxy * sxy) / (sxx * syy);
        r2 = q < 0.0 ? 0.0 : q > 1.0 ? 1.0 : q;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// 1. the in-order chains; presence bits and status
// ------------------------------------------------------------------------------------------------------------------------------
template <class B>
__device__ __forceinline__ void ft_chains(const FeaturesArgs &a, int s, int n, B buf, B, int lane)
{
    const size_t ld = a.ld;
    bool has_nan;
    const int k = ft_compact(a, s, n, buf, lane, has_nan);
    const double kf = (double)k;
    int64_t status = k == 0 ? FEATURES_EMPTY : has_nan ? FEATURES_NAN : FEATURES_OK;
    uint64_t present[2] = {0, 0};
#define FT_HAS(id) present[F_##id >> 6] |= 1ull << (F_##id & 63)

    double sum = FT_NAN, mean = FT_NAN, lo = FT_NAN, hi = FT_NAN, range = FT_NAN, variance = FT_NAN, sd = FT_NAN, cv = FT_NAN, large_sd = FT_NAN;
    double skew = FT_NAN, kurt = FT_NAN, mean_change = FT_NAN, mean_abs_change = FT_NAN, abs_changes = FT_NAN, cid = FT_NAN, msdc = FT_NAN;
    double energy = FT_NAN, rms = FT_NAN, first = FT_NAN, last = FT_NAN, lt_slope = FT_NAN, lt_icpt = FT_NAN, lt_r2 = FT_NAN;
    double acf = FT_NAN, pacf1 = FT_NAN, pacf2 = FT_NAN, tra = FT_NAN, c3 = FT_NAN;
    double ag_slope = FT_NAN, ag_icpt = FT_NAN, ag_r = FT_NAN, ag_err = FT_NAN;

    if (status == FEATURES_NAN) FT_HAS(length);
    if (status == FEATURES_OK) {
        double css;
        ft_moments(buf, k, sum, mean, css, lo, hi);
        range = hi - lo;
        variance = css / kf;
        sd = sqrt(variance);
        cv = fabs(mean) > FT_EPS ? sd / fabs(mean) : FT_NAN;
        large_sd = sd > 0.25 * range ? 1.0 : 0.0;
        first = FT_V(0);
        last = FT_V(k - 1);

        energy = 0.0;
#pragma unroll 8
        for (int i = 0; i < k; i++) { const double v = FT_V(i); energy += v * v; }
        rms = sqrt(energy / kf);

        if (sd > FT_EPS) {
            double s3 = 0.0, s4 = 0.0;
#pragma unroll 4
            for (int i = 0; i < k; i++) {
                const double z = (FT_V(i) - mean) / sd, zz = z * z;
                s3 += z * zz;
                s4 += zz * zz;
            }
            skew = s3 / kf;
            kurt = s4 / kf - 3.0;
        }

        if (k > 1) {
            double sch = 0.0, sab = 0.0, ssq = 0.0, sdd = 0.0;
            double v0 = FT_V(0), v1 = FT_V(1);
            for (int i = 0; i + 1 < k; i++) {
                const double ch = v1 - v0;
                sch += ch;
                sab += fabs(ch);
                ssq += ch * ch;
                if (i + 2 < k) {
                    const double v2 = FT_V(i + 2);
                    sdd += (v2 - 2.0 * v1) + v0;
                    v0 = v1; v1 = v2;
                }
            }
            mean_change = sch / (double)(k - 1);
            mean_abs_change = sab / (double)(k - 1);
            abs_changes = sab;
            cid = sqrt(ssq);
            if (k > 2) msdc = sdd / (double)(k - 2);
        }

        if (k < 2) { lt_slope = 0.0; lt_icpt = first; lt_r2 = 0.0; }
        else {
            double sxx;
            ft_linear_trend(k, mean, [&](int i) { return FT_V(i); }, lt_slope, lt_icpt, lt_r2, sxx);
        }

        // the ACF lags side by side: lane l < 10 carries lag l + 1 (the others repeat lag 1); the denominator is the chain of css
        {
            const int lag = lane < 10 ? lane + 1 : 1;
            double num = 0.0;
            for (int i = 0; i < k; i++) {
                const double d = FT_V(i) - mean;
                if (i >= lag) num += d * (FT_V(i - lag) - mean);
            }
            acf = fabs(css) < FT_EPS ? 0.0 : num / css;
            const double a1 = __shfl(acf, 0), a2 = __shfl(acf, 1);
            pacf1 = a1;
            const double a11 = a1 * a1;
            pacf2 = fabs(1.0 - a11) < FT_EPS ? 0.0 : (a2 - a11) / (1.0 - a11);
        }

        // time reversal asymmetry and c3: lane l < 3 carries lag l + 1
        {
            const int lag = lane < 3 ? lane + 1 : 1;
            double st = 0.0, sc = 0.0;
            if (k > 2 * lag) {
                for (int i = 0; i < k - lag; i++) {
                    if (i >= lag) {
                        const double xl = FT_V(i - lag), x = FT_V(i), xd = FT_V(i + lag);
                        st += (xd * xd) * x - xl * (x * x);
                    }
                    if (i < k - 2 * lag) sc += FT_V(i) * FT_V(i + lag) * FT_V(i + 2 * lag);
                }
                tra = st / (double)(k - 2 * lag);
                c3 = sc / (double)(k - 2 * lag);
            }
        }

        // aggregated linear trend: lane c carries the mean of chunk c (at most 15 chunks), the trend over them is one chain
        {
            const int cl = k / 10 > 2 ? k / 10 : 2;
            if (k < cl) { ag_slope = ag_icpt = ag_r = ag_err = 0.0; }
            else {
                const int nc = (k + cl - 1) / cl;
                const int c0 = lane * cl;
                const int len = lane < nc ? (k - c0 < cl ? k - c0 : cl) : 0;
                double cs = 0.0;
                for (int j = 0; j < len; j++) cs += FT_V(c0 + j);
                const double cm = len > 0 ? cs / (double)len : 0.0;
                if (nc < 2) { ag_slope = 0.0; ag_icpt = __shfl(cm, 0); ag_r = 0.0; ag_err = 0.0; }
                else {
                    double msum = 0.0;
                    for (int i = 0; i < nc; i++) msum += __shfl(cm, i);
                    const double ncf = (double)nc, ym = msum / ncf;
                    double r2, sxx;
                    ft_linear_trend(nc, ym, [&](int i) { return __shfl(cm, i); }, ag_slope, ag_icpt, r2, sxx);
                    double rss = 0.0;
                    for (int i = 0; i < nc; i++) {
                        const double d = __shfl(cm, i) - (ag_icpt + ag_slope * (double)i);
                        rss += d * d;
                    }
                    ag_err = (ncf > 2.0 && sxx > FT_EPS) ? sqrt(rss / (ncf - 2.0) / sxx) : 0.0;
                    ag_r = sqrt(r2);
                }
            }
        }

        // what the source inserts
        FT_HAS(length); FT_HAS(sum); FT_HAS(mean); FT_HAS(minimum); FT_HAS(maximum); FT_HAS(range); FT_HAS(variance);
        FT_HAS(standard_deviation); FT_HAS(variation_coefficient); FT_HAS(large_standard_deviation); FT_HAS(median);
        FT_HAS(quantile_0_1); FT_HAS(quantile_0_25); FT_HAS(quantile_0_75); FT_HAS(quantile_0_9);
        if (sd > FT_EPS) { FT_HAS(skewness); FT_HAS(kurtosis); }
        FT_HAS(count_above_mean); FT_HAS(count_below_mean); FT_HAS(percentage_above_mean); FT_HAS(zero_crossing_rate);
        if (k > 1) { FT_HAS(mean_change); FT_HAS(mean_abs_change); FT_HAS(cid_ce); FT_HAS(absolute_sum_of_changes); }
        if (k > 2) FT_HAS(mean_second_derivative_central);
        for (int lag = 1; lag <= 10; lag++)                       // the rows of the lags are not consecutive (lag10 sorts after lag1)
            if (k > lag) {
                const int f = lag == 1 ? F_autocorrelation_lag1 : lag == 2 ? F_autocorrelation_lag2 : lag == 3 ? F_autocorrelation_lag3 :
                              lag == 4 ? F_autocorrelation_lag4 : lag == 5 ? F_autocorrelation_lag5 : lag == 6 ? F_autocorrelation_lag6 :
                              lag == 7 ? F_autocorrelation_lag7 : lag == 8 ? F_autocorrelation_lag8 : lag == 9 ? F_autocorrelation_lag9 :
                              F_autocorrelation_lag10;
                present[f >> 6] |= 1ull << (f & 63);
            }
        if (k > 2) FT_HAS(partial_autocorrelation_lag1);
        if (k > 3) FT_HAS(partial_autocorrelation_lag2);
        if (k > 4) FT_HAS(partial_autocorrelation_lag3);
        if (k > 5) FT_HAS(partial_autocorrelation_lag4);
        if (k > 6) FT_HAS(partial_autocorrelation_lag5);
        FT_HAS(first_value); FT_HAS(last_value); FT_HAS(first_location_of_maximum); FT_HAS(last_location_of_maximum);
        FT_HAS(first_location_of_minimum); FT_HAS(last_location_of_minimum); FT_HAS(abs_energy); FT_HAS(root_mean_square);
        FT_HAS(longest_strike_above_mean); FT_HAS(longest_strike_below_mean); FT_HAS(number_peaks); FT_HAS(number_peaks_threshold_1);
        FT_HAS(number_peaks_threshold_2); FT_HAS(benford_correlation); FT_HAS(linear_trend_slope); FT_HAS(linear_trend_intercept);
        FT_HAS(linear_trend_r_squared); FT_HAS(binned_entropy); FT_HAS(sample_entropy); FT_HAS(approximate_entropy);
        FT_HAS(permutation_entropy); FT_HAS(ratio_beyond_r_sigma_1); FT_HAS(ratio_beyond_r_sigma_2); FT_HAS(ratio_beyond_r_sigma_3);
        FT_HAS(count_unique); FT_HAS(ratio_value_number_to_length); FT_HAS(has_duplicate); FT_HAS(has_duplicate_max);
        FT_HAS(has_duplicate_min); FT_HAS(percentage_of_reoccurring_datapoints_to_all_datapoints);
        FT_HAS(percentage_of_reoccurring_values_to_all_values); FT_HAS(sum_of_reoccurring_values); FT_HAS(sum_of_reoccurring_datapoints);
        if (k > 2) { FT_HAS(time_reversal_asymmetry_stat_1); FT_HAS(c3_lag1); }
        if (k > 4) { FT_HAS(time_reversal_asymmetry_stat_2); FT_HAS(c3_lag2); }
        if (k > 6) { FT_HAS(time_reversal_asymmetry_stat_3); FT_HAS(c3_lag3); }
        FT_HAS(lempel_ziv_complexity); FT_HAS(spectral_centroid); FT_HAS(spectral_variance);
        FT_HAS(agg_linear_trend_slope); FT_HAS(agg_linear_trend_intercept); FT_HAS(agg_linear_trend_rvalue); FT_HAS(agg_linear_trend_stderr);
        for (int i = 0; i < 10 && i < k; i++) {                   // take(10) of n coefficients; the 30 rows are consecutive
            const int f = F_fft_coefficient_0_abs + 3 * i;
            for (int j = 0; j < 3; j++) present[(f + j) >> 6] |= 1ull << ((f + j) & 63);
        }
    }
#undef FT_HAS

    // the lag features: one lane per lag writes its own row (a short series leaves NaN)
    {
        const bool ok = status == FEATURES_OK;
        const int lag = lane + 1;
        if (lane < 10) {
            const int f = lag == 1 ? F_autocorrelation_lag1 : lag == 2 ? F_autocorrelation_lag2 : lag == 3 ? F_autocorrelation_lag3 :
                          lag == 4 ? F_autocorrelation_lag4 : lag == 5 ? F_autocorrelation_lag5 : lag == 6 ? F_autocorrelation_lag6 :
                          lag == 7 ? F_autocorrelation_lag7 : lag == 8 ? F_autocorrelation_lag8 : lag == 9 ? F_autocorrelation_lag9 :
                          F_autocorrelation_lag10;
            a.out_fp[(size_t)f * ld + s] = ok && k > lag ? acf : FT_NAN;
        }
        if (lane < 3) {
            a.out_fp[(size_t)(F_time_reversal_asymmetry_stat_1 + lane) * ld + s] = tra;
            a.out_fp[(size_t)(F_c3_lag1 + lane) * ld + s] = c3;
        }
        if (lane < 5) a.out_fp[(size_t)(F_partial_autocorrelation_lag1 + lane) * ld + s] = ok && k > lag + 1 ? (lane == 0 ? pacf1 : pacf2) : FT_NAN;
    }
    if (lane == 0) {
        FT_OUT(length, status == FEATURES_EMPTY ? FT_NAN : kf);
        FT_OUT(sum, sum); FT_OUT(mean, mean); FT_OUT(minimum, lo); FT_OUT(maximum, hi); FT_OUT(range, range);
        FT_OUT(variance, variance); FT_OUT(standard_deviation, sd); FT_OUT(variation_coefficient, cv);
        FT_OUT(large_standard_deviation, large_sd); FT_OUT(skewness, skew); FT_OUT(kurtosis, kurt);
        FT_OUT(mean_change, mean_change); FT_OUT(mean_abs_change, mean_abs_change); FT_OUT(absolute_sum_of_changes, abs_changes);
        FT_OUT(cid_ce, cid); FT_OUT(mean_second_derivative_central, msdc); FT_OUT(abs_energy, energy); FT_OUT(root_mean_square, rms);
        FT_OUT(first_value, first); FT_OUT(last_value, last);
        FT_OUT(linear_trend_slope, lt_slope); FT_OUT(linear_trend_intercept, lt_icpt); FT_OUT(linear_trend_r_squared, lt_r2);
        FT_OUT(agg_linear_trend_slope, ag_slope); FT_OUT(agg_linear_trend_intercept, ag_icpt); FT_OUT(agg_linear_trend_rvalue, ag_r);
        FT_OUT(agg_linear_trend_stderr, ag_err);
        a.out_int[0 * ld + s] = (int64_t)present[0];
        a.out_int[1 * ld + s] = (int64_t)present[1];
        a.out_int[2 * ld + s] = status;
    }
}
static_assert(F_time_reversal_asymmetry_stat_3 == F_time_reversal_asymmetry_stat_1 + 2 && F_c3_lag3 == F_c3_lag1 + 2 &&
              F_partial_autocorrelation_lag5 == F_partial_autocorrelation_lag1 + 4 && F_fft_coefficient_9_real == F_fft_coefficient_0_abs + 29,
              "rows the kernels address by offset are consecutive in byte order");

// ------------------------------------------------------------------------------------------------------------------------------
// 2. the sort-based figures
// ------------------------------------------------------------------------------------------------------------------------------
template <class B>
__device__ __forceinline__ double ft_quantile(B buf, int k, double q)
{
    const double idx = q * (double)(k - 1);
    const double fl = floor(idx), ce = ceil(idx);
    const int lower = (int)fl, upper = (int)ce;
    const double frac = idx - fl;
    if (upper >= k) return st_unkey(buf[k - 1]);
    return st_unkey(buf[lower]) * (1.0 - frac) + st_unkey(buf[upper]) * frac;
}

template <class B>
__device__ __forceinline__ void ft_sort(const FeaturesArgs &a, int s, int n, B buf, B, int lane)
{
    const size_t ld = a.ld;
    bool has_nan;
    const int k = ft_compact(a, s, n, buf, lane, has_nan);
    const double kf = (double)k;
    double median = FT_NAN, q10 = FT_NAN, q25 = FT_NAN, q75 = FT_NAN, q90 = FT_NAN, uniq = FT_NAN, ratio = FT_NAN, has_dup = FT_NAN;
    double pct_dp = FT_NAN, pct_val = FT_NAN, sum_val = FT_NAN, sum_dp = FT_NAN;
    if (k > 0 && !has_nan) {
        int p2 = 1;
        while (p2 < k) p2 <<= 1;
        for (int i = lane; i < p2; i += 64) {
            const uint64_t w = i < k ? st_key(buf[i]) : ~0ull;
            buf[i] = w;
        }
        st_sync();
        st_sort(buf, p2, lane);
        median = (k & 1) ? st_unkey(buf[k / 2]) : (st_unkey(buf[k / 2 - 1]) + st_unkey(buf[k / 2])) / 2.0;
        q10 = ft_quantile(buf, k, 0.1);
        q25 = ft_quantile(buf, k, 0.25);
        q75 = ft_quantile(buf, k, 0.75);
        q90 = ft_quantile(buf, k, 0.9);
        // one walk over the runs of equal keys, in ascending order: the defined order of the two sums
        int n_unique = 0, n_re_val = 0, n_re_dp = 0, run = 0;
        uint64_t cur = 0;
        double sv = 0.0, sp = 0.0;
        for (int i = 0; i <= k; i++) {
            const uint64_t w = i < k ? buf[i] : 0;
            if (i == k || (run > 0 && w != cur)) {
                n_unique++;
                if (run > 1) {
                    const double v = st_unkey(cur);
                    n_re_val++;
                    n_re_dp += run;
                    sv += v;
                    sp += v * (double)run;
                }
                run = 0;
            }
            cur = w;
            run++;
        }
        uniq = (double)n_unique;
        ratio = uniq / kf;
        has_dup = n_unique < k ? 1.0 : 0.0;
        pct_dp = (double)n_re_dp / kf;
        pct_val = (double)n_re_val / (uniq > 1.0 ? uniq : 1.0);
        sum_val = sv;
        sum_dp = sp;
    }
    if (lane == 0) {
        FT_OUT(median, median); FT_OUT(quantile_0_1, q10); FT_OUT(quantile_0_25, q25); FT_OUT(quantile_0_75, q75); FT_OUT(quantile_0_9, q90);
        FT_OUT(count_unique, uniq); FT_OUT(ratio_value_number_to_length, ratio); FT_OUT(has_duplicate, has_dup);
        FT_OUT(percentage_of_reoccurring_datapoints_to_all_datapoints, pct_dp);
        FT_OUT(percentage_of_reoccurring_values_to_all_values, pct_val);
        FT_OUT(sum_of_reoccurring_values, sum_val); FT_OUT(sum_of_reoccurring_datapoints, sum_dp);
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// 3. the counting scans
// ------------------------------------------------------------------------------------------------------------------------------
// 64 bits of the bit string from position pos on (the two words after the string are zero)
__device__ __forceinline__ uint64_t ft_bits_at(const uint64_t *bw, int pos)
{
    const int w = pos >> 6, o = pos & 63;
    const uint64_t lo = bw[w] >> o;
    return o ? lo | (bw[w + 1] << (64 - o)) : lo;
}

__device__ __forceinline__ bool ft_bits_equal(const uint64_t *bw, int p, int q, int len)
{
    for (int off = 0; off < len; off += 64) {
        const int rest = len - off;
        const uint64_t m = rest >= 64 ? ~0ull : (1ull << rest) - 1ull;
        if ((ft_bits_at(bw, p + off) ^ ft_bits_at(bw, q + off)) & m) return false;
    }
    return true;
}

// first digit of Rust's to_string() of a finite v >= 1: the d with table[9 e + d - 1] <= v < the next threshold
__device__ __forceinline__ int ft_first_digit(const double *table, double v)
{
    int lo = 0, hi = FEATURES_BENFORD;                       // table[lo] <= v (table[0] = 1), table[hi] > v (beyond the end)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (table[mid] <= v) lo = mid; else hi = mid;
    }
    return lo % 9;                                            // digit - 1
}

template <class B>
__device__ __forceinline__ void ft_scan(const FeaturesArgs &a, int s, int n, B buf, B, int lane)
{
    __shared__ uint64_t bw[FT_BITS_WORDS];
    const size_t ld = a.ld;
    bool has_nan;
    const int k = ft_compact(a, s, n, buf, lane, has_nan);
    const double kf = (double)k;
    double above = FT_NAN, below = FT_NAN, pct_above = FT_NAN, zcr = FT_NAN, strike_a = FT_NAN, strike_b = FT_NAN;
    double peaks = FT_NAN, peaks1 = FT_NAN, peaks2 = FT_NAN, first_max = FT_NAN, last_max = FT_NAN, first_min = FT_NAN, last_min = FT_NAN;
    double dup_max = FT_NAN, dup_min = FT_NAN, beyond1 = FT_NAN, beyond2 = FT_NAN, beyond3 = FT_NAN, benford = FT_NAN, binned = FT_NAN;
    double perm = FT_NAN, lz = FT_NAN;
    if (k > 0 && !has_nan) {
        double sum, mean, css, lo, hi;
        ft_moments(buf, k, sum, mean, css, lo, hi);
        const double sd = sqrt(css / kf), range = hi - lo;
        const double t1 = 1.0 * sd, t2 = 2.0 * sd, t3 = 3.0 * sd;

        // strikes: one serial walk
        {
            int ba = 0, bb = 0, ca = 0, cb = 0;
#pragma unroll 4
            for (int i = 0; i < k; i++) {
                const double v = FT_V(i);
                ca = v > mean ? ca + 1 : 0;
                cb = v < mean ? cb + 1 : 0;
                ba = ca > ba ? ca : ba;
                bb = cb > bb ? cb : bb;
            }
            strike_a = (double)ba;
            strike_b = (double)bb;
        }

        int n_above = 0, n_below = 0, n_zc = 0, n_pk = 0, n_pk1 = 0, n_pk2 = 0, n_b1 = 0, n_b2 = 0, n_b3 = 0;
        int fmx = -1, lmx = 0, cmx = 0, fmn = -1, lmn = 0, cmn = 0, total = 0;
        int digits[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, bins[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, pats[6] = {0, 0, 0, 0, 0, 0};
        const bool binning = !(fabs(range) < FT_EPS);
        for (int c0 = 0; c0 < k; c0 += 64) {
            const int i = c0 + lane;
            const bool in = i < k;
            const double v = in ? FT_V(i) : 0.0;
            const double vp = in && i >= 1 ? FT_V(i - 1) : 0.0;              // the value before
            const double vn = i + 1 < k ? FT_V(i + 1) : 0.0, vnn = i + 2 < k ? FT_V(i + 2) : 0.0;
            const double dev = fabs(v - mean);
            n_above += __popcll(__ballot(in && v > mean));
            n_below += __popcll(__ballot(in && v < mean));
            n_zc += __popcll(__ballot(i + 1 < k && v != 0.0 && vn != 0.0 && (v < 0.0) != (vn < 0.0)));
            const bool peak = in && i >= 1 && i + 1 < k && v > vp && v > vn;
            n_pk += __popcll(__ballot(peak));
            n_pk1 += __popcll(__ballot(peak && dev > t1));
            n_pk2 += __popcll(__ballot(peak && dev > t2));
            n_b1 += __popcll(__ballot(in && dev > t1));
            n_b2 += __popcll(__ballot(in && dev > t2));
            n_b3 += __popcll(__ballot(in && dev > t3));
            const uint64_t mx = __ballot(in && fabs(v - hi) < FT_EPS), mn = __ballot(in && fabs(v - lo) < FT_EPS);
            if (mx) { if (fmx < 0) fmx = c0 + __ffsll((long long)mx) - 1; lmx = c0 + 63 - __clzll((long long)mx); cmx += __popcll(mx); }
            if (mn) { if (fmn < 0) fmn = c0 + __ffsll((long long)mn) - 1; lmn = c0 + 63 - __clzll((long long)mn); cmn += __popcll(mn); }
            // Benford: the first digit of |v| >= 1 (an infinity prints no digit)
            const double av = fabs(v);
            const bool counted = in && av >= 1.0 && av < __builtin_huge_val();
            const int dg = counted ? ft_first_digit(a.benford, av) : -1;
#pragma unroll
            for (int d = 0; d < 9; d++) digits[d] += __popcll(__ballot(dg == d));
            total += __popcll(__ballot(counted));
            // binned entropy: round() as usize saturates, a NaN becomes bin 0
            if (binning) {
                const double b = round(((v - lo) / range) * 9.0);
                const int bin = !in ? -1 : b != b ? 0 : b < 0.0 ? 0 : b > 9.0 ? 9 : (int)b;
#pragma unroll
                for (int d = 0; d < 10; d++) bins[d] += __popcll(__ballot(bin == d));
            }
            // permutation patterns of (v, vn, vnn): the stable order of the three indices
            {
                const bool b01 = !(vn < v), b02 = !(vnn < v), b12 = !(vnn < vn);
                const int pat = i + 2 < k ? ((b01 && b02) ? (b12 ? 0 : 1) : (!b01 && b12) ? (b02 ? 2 : 3) : (b01 ? 4 : 5)) : -1;
#pragma unroll
                for (int d = 0; d < 6; d++) pats[d] += __popcll(__ballot(pat == d));
            }
            // the bit string of Lempel-Ziv
            const uint64_t bit = __ballot(in && v >= mean);
            if (lane == 0) bw[c0 >> 6] = bit;
        }
        if (lane == 0) { bw[(k + 63) >> 6] = 0; bw[((k + 63) >> 6) + 1] = 0; }
        st_sync();

        above = (double)n_above; below = (double)n_below; pct_above = above / kf;
        zcr = (double)n_zc / (kf - 1.0 > 1.0 ? kf - 1.0 : 1.0);
        peaks = (double)n_pk; peaks1 = (double)n_pk1; peaks2 = (double)n_pk2;
        beyond1 = (double)n_b1 / kf; beyond2 = (double)n_b2 / kf; beyond3 = (double)n_b3 / kf;
        first_max = (double)(fmx < 0 ? 0 : fmx) / kf; last_max = (double)lmx / kf;
        first_min = (double)(fmn < 0 ? 0 : fmn) / kf; last_min = (double)lmn / kf;
        dup_max = cmx > 1 ? 1.0 : 0.0; dup_min = cmn > 1 ? 1.0 : 0.0;

        // benford_correlation
        if (total == 0) benford = 0.0;
        else {
            const double expected[9] = {0.301, 0.176, 0.125, 0.097, 0.079, 0.067, 0.058, 0.051, 0.046};
            double obs[9], se = 0.0, so = 0.0;
#pragma unroll
            for (int d = 0; d < 9; d++) { obs[d] = (double)digits[d] / (double)total; se += expected[d]; so += obs[d]; }
            const double me = se / 9.0, mo = so / 9.0;
            double num = 0.0, de = 0.0, dob = 0.0;
#pragma unroll
            for (int d = 0; d < 9; d++) {
                num += (expected[d] - me) * (obs[d] - mo);
                de += (expected[d] - me) * (expected[d] - me);
                dob += (obs[d] - mo) * (obs[d] - mo);
            }
            const double den = sqrt(de * dob);
            benford = fabs(den) < FT_EPS ? 0.0 : num / den;
        }

        binned = 0.0;
        if (binning) {
#pragma unroll
            for (int d = 0; d < 10; d++)
                if (bins[d] > 0) { const double p = (double)bins[d] / kf; binned -= p * dm_log(p); }
        }

        if (k >= 3) {
            const double tot = (double)(k - 2);
            double e = 0.0;
#pragma unroll
            for (int d = 0; d < 6; d++) {
                const double p = (double)pats[d] / tot;
                if (p > 0.0) e -= p * dm_log(p);
            }
            double mx = 0.0;
            mx += dm_log(1.0); mx += dm_log(2.0); mx += dm_log(3.0);
            perm = mx > 0.0 ? e / mx : e;
        }

        // Lempel-Ziv, the source's scan: is the substring [l, l + kk) equal to one that starts in 0 .. l?  lanes take the starts
        {
            int complexity = 1, l = 1, kk = 1, kmax = 1;
            while (l + kk <= k) {
                bool found = false;
                for (int s0 = 0; s0 < l && !found; s0 += 64) {
                    const int st = s0 + lane;
                    if (__ballot(st < l && ft_bits_equal(bw, st, l, kk))) found = true;
                }
                if (found) { kk++; kmax = kk > kmax ? kk : kmax; }
                else { complexity++; l += kmax; kk = 1; kmax = 1; }
            }
            const double b = dm_log(kf) / dm_log(2.0);
            lz = b > 0.0 ? (double)complexity * b / kf : 0.0;
        }
    }
    if (lane == 0) {
        FT_OUT(count_above_mean, above); FT_OUT(count_below_mean, below); FT_OUT(percentage_above_mean, pct_above);
        FT_OUT(zero_crossing_rate, zcr); FT_OUT(longest_strike_above_mean, strike_a); FT_OUT(longest_strike_below_mean, strike_b);
        FT_OUT(number_peaks, peaks); FT_OUT(number_peaks_threshold_1, peaks1); FT_OUT(number_peaks_threshold_2, peaks2);
        FT_OUT(first_location_of_maximum, first_max); FT_OUT(last_location_of_maximum, last_max);
        FT_OUT(first_location_of_minimum, first_min); FT_OUT(last_location_of_minimum, last_min);
        FT_OUT(has_duplicate_max, dup_max); FT_OUT(has_duplicate_min, dup_min);
        FT_OUT(ratio_beyond_r_sigma_1, beyond1); FT_OUT(ratio_beyond_r_sigma_2, beyond2); FT_OUT(ratio_beyond_r_sigma_3, beyond3);
        FT_OUT(benford_correlation, benford); FT_OUT(binned_entropy, binned); FT_OUT(permutation_entropy, perm);
        FT_OUT(lempel_ziv_complexity, lz);
    }
    st_sync();                                                   // the bit string is read before the next series overwrites it
}

// ------------------------------------------------------------------------------------------------------------------------------
// 4. template matching
// ------------------------------------------------------------------------------------------------------------------------------
template <class B>
__device__ __forceinline__ void ft_match(const FeaturesArgs &a, int s, int n, B buf, B, int lane)
{
    const size_t ld = a.ld;
    bool has_nan;
    const int k = ft_compact(a, s, n, buf, lane, has_nan);
    const double kf = (double)k;
    double sampen = FT_NAN, apen = FT_NAN;
    if (k > 0 && !has_nan) {
        double sum, mean, css, lo, hi;
        ft_moments(buf, k, sum, mean, css, lo, hi);
        const double r = 0.2 * sqrt(css / kf);
        if (k >= 3 && !(r <= 0.0)) {                                 // (a NaN r passes, as in the source)
            // sample entropy: pairs i < j < k - m, m = 2 and 3 in one pass; lanes take j.  A NaN difference is not > r: a match.
            long long c2 = 0, c3 = 0;
            for (int i = 0; i + 2 < k; i++) {
                const double x0 = FT_V(i), x1 = FT_V(i + 1), x2 = i + 3 < k ? FT_V(i + 2) : 0.0;
                for (int j0 = i + 1; j0 + 2 < k; j0 += 64) {
                    const int j = j0 + lane;
                    if (j + 2 < k) {
                        const bool m2 = !(fabs(x0 - FT_V(j)) > r) && !(fabs(x1 - FT_V(j + 1)) > r);
                        c2 += m2;
                        if (j + 3 < k) c3 += m2 && !(fabs(x2 - FT_V(j + 2)) > r);
                    }
                }
            }
            c2 = ft_wave_sum(c2);
            c3 = ft_wave_sum(c3);
            if (c2 != 0 && c3 != 0) {
                const long long n2 = (long long)(k - 2) * (k - 3) / 2, n3 = (long long)(k - 3) * (k - 4) / 2;
                if (n2 != 0 && n3 != 0) {
                    const double p2 = (double)c2 / (double)n2, p3 = (double)c3 / (double)n3;
                    sampen = -dm_log(p3 / p2);
                }
            }
            // approximate entropy: lanes take i, every lane walks all j; the logarithms are added in the order of i
            double cs2 = 0.0, cs3 = 0.0;
            const double t2 = (double)(k - 1), t3 = (double)(k - 2);     // n - m + 1 templates
            for (int i0 = 0; i0 + 1 < k; i0 += 64) {
                const int i = i0 + lane;
                const bool in2 = i + 1 < k, in3 = i + 2 < k;
                const double x0 = in2 ? FT_V(i) : 0.0, x1 = in2 ? FT_V(i + 1) : 0.0, x2 = in3 ? FT_V(i + 2) : 0.0;
                int n2 = 0, n3 = 0;
                double y0 = FT_V(0), y1 = FT_V(1);
                for (int j = 0; j + 1 < k; j++) {
                    const bool j3 = j + 2 < k;
                    const double y2 = j3 ? FT_V(j + 2) : 0.0;
                    const bool m2 = !(fabs(x0 - y0) > r) && !(fabs(x1 - y1) > r);
                    n2 += m2;
                    n3 += m2 && j3 && !(fabs(x2 - y2) > r);
                    y0 = y1; y1 = y2;
                }
                const double l2 = in2 && n2 > 0 ? dm_log((double)n2 / t2) : 0.0;
                const double l3 = in3 && n3 > 0 ? dm_log((double)n3 / t3) : 0.0;
                const int cnt = k - 1 - i0 < 64 ? k - 1 - i0 : 64;
                for (int l = 0; l < cnt; l++) {
                    cs2 += __shfl(l2, l);
                    if (i0 + l + 2 < k) cs3 += __shfl(l3, l);
                }
            }
            apen = cs2 / t2 - cs3 / t3;
        }
    }
    if (lane == 0) { FT_OUT(sample_entropy, sampen); FT_OUT(approximate_entropy, apen); }
}

// ------------------------------------------------------------------------------------------------------------------------------
// 5. the DFT
// ------------------------------------------------------------------------------------------------------------------------------
template <class B>
__device__ __forceinline__ void ft_dft(const FeaturesArgs &a, int s, int n, B buf, B pw, int lane)
{
    const size_t ld = a.ld;
    bool has_nan;
    const int k = ft_compact(a, s, n, buf, lane, has_nan);
    const double kf = (double)k;
    const bool ok = k > 0 && !has_nan;
    double centroid = FT_NAN, variance = FT_NAN;
    if (ok) {
        for (int b0 = 0; b0 < k; b0 += 64) {
            const int bin = b0 + lane;
            const double w = (-2.0 * FT_PI) * (double)bin;
            double re = 0.0, im = 0.0;
            for (int t = 0; t < k; t++) {
                double sn, cs;
                per_sincos(w * (double)t / kf, sn, cs);
                const double x = FT_V(t);
                re += x * cs;
                im += x * sn;
            }
            re = re / kf;
            im = im / kf;
            if (bin < k) pw[bin] = dm_bits(re * re + im * im);
            if (b0 == 0 && lane < 10) {                                  // rows abs, imag, real of coefficient `lane`
                double *o = a.out_fp + (size_t)(F_fft_coefficient_0_abs + 3 * lane) * ld + s;
                const bool has = bin < k;
                o[0 * ld] = has ? sqrt(re * re + im * im) : FT_NAN;
                o[1 * ld] = has ? im : FT_NAN;
                o[2 * ld] = has ? re : FT_NAN;
            }
        }
        st_sync();
        double total = 0.0;
#pragma unroll 8
        for (int i = 0; i < k; i++) total += dm_from_bits(pw[i]);
        if (total <= FT_EPS) centroid = variance = 0.0;
        else {
            double sc = 0.0;
#pragma unroll 4
            for (int i = 0; i < k; i++) sc += (double)i * dm_from_bits(pw[i]);
            centroid = sc / total;
            double sv = 0.0;
#pragma unroll 4
            for (int i = 0; i < k; i++) { const double d = (double)i - centroid; sv += (d * d) * dm_from_bits(pw[i]); }
            variance = sv / total;
        }
    } else if (lane < 30) {
        a.out_fp[(size_t)(F_fft_coefficient_0_abs + lane) * ld + s] = FT_NAN;
    }
    if (lane == 0) { FT_OUT(spectral_centroid, centroid); FT_OUT(spectral_variance, variance); }
    st_sync();                                                   // the powers are read before the next series overwrites them
}
static_assert(F_fft_coefficient_0_imag == F_fft_coefficient_0_abs + 1 && F_fft_coefficient_0_real == F_fft_coefficient_0_abs + 2 &&
              F_fft_coefficient_1_abs == F_fft_coefficient_0_abs + 3, "abs, imag, real per coefficient");

// a series of at most a.tile rows, the buffers in LDS (HALVES x tile words); and the longer ones, a.work_waves waves over the workspace
#define FT_KERNELS(NAME, BODY, HALVES)                                                                                            \
    __global__ __launch_bounds__(64) void features_##NAME##_kernel(const FeaturesArgs a)                                          \
    {                                                                                                                             \
        extern __shared__ uint64_t ft_lds[];                                                                                      \
        const int s = blockIdx.x;                                                                                                 \
        if (s >= a.n_series) return;                                                                                              \
        const int n = ft_length(a, s);                                                                                            \
        if (n > a.tile) return;                                                                                                   \
        BODY(a, s, n, ft_lds, ft_lds + (HALVES > 1 ? a.tile : 0), (int)threadIdx.x);                                              \
    }                                                                                                                             \
    __global__ __launch_bounds__(64) void features_##NAME##_long_kernel(const FeaturesArgs a)                                     \
    {                                                                                                                             \
        const int w = blockIdx.x;                                                                                                 \
        if (w >= a.work_waves) return;                                                                                            \
        uint64_t *buf = a.work + (size_t)w * 2 * a.work_stride;                                                                   \
        for (int s = w; s < a.n_series; s += a.work_waves) {                                                                      \
            const int n = ft_length(a, s);                                                                                        \
            if (n <= a.tile || (size_t)n > a.work_stride) continue;                                                               \
            BODY(a, s, n, buf, buf + a.work_stride, (int)threadIdx.x);                                                            \
            st_sync();                                                                                                            \
        }                                                                                                                         \
    }

FT_KERNELS(chains, ft_chains, 1)
FT_KERNELS(sort, ft_sort, 1)
FT_KERNELS(scan, ft_scan, 1)
FT_KERNELS(match, ft_match, 1)
FT_KERNELS(dft, ft_dft, 2)

} // namespace

int features_tile(size_t t_rows)
{
    int tile = 64;
    while (tile < FEATURES_RESIDENT && (size_t)tile < t_rows) tile <<= 1;
    return tile;
}

size_t features_work_stride(size_t t_rows)
{
    if (t_rows <= (size_t)FEATURES_RESIDENT) return 0;
    size_t p2 = 1;
    while (p2 < t_rows) p2 <<= 1;
    return p2;
}

int features_work_waves(int n_series)
{
    return n_series < FEATURES_WORK_WAVES ? n_series : FEATURES_WORK_WAVES;
}

void launch_features(const FeaturesArgs &a, hipStream_t stream, int families)
{
    if (a.n_series <= 0) return;
    const size_t lds = (size_t)a.tile * sizeof(uint64_t);
    const bool longer = a.t_rows > (size_t)FEATURES_RESIDENT && a.work && a.work_waves > 0;
#define FT_LAUNCH(FAM, NAME, HALVES)                                                                                              \
    if (families & (1 << FAM)) {                                                                                                  \
        hipLaunchKernelGGL(features_##NAME##_kernel, dim3(a.n_series), dim3(64), HALVES * lds, stream, a);                        \
        if (longer) hipLaunchKernelGGL(features_##NAME##_long_kernel, dim3(a.work_waves), dim3(64), 0, stream, a);                \
    }
    FT_LAUNCH(FEATURES_CHAINS, chains, 1)
    FT_LAUNCH(FEATURES_SORT, sort, 1)
    FT_LAUNCH(FEATURES_SCAN, scan, 1)
    FT_LAUNCH(FEATURES_MATCH, match, 1)
    FT_LAUNCH(FEATURES_DFT, dft, 2)
#undef FT_LAUNCH
}

} // namespace anofox
