// stats.hip -- the 36 per-series figures of the reference's ts_stats_by (stats.rs compute_ts_stats and
// compute_ts_stats_with_dates_and_type) for every series of a time-major block, one wavefront per series.
//
// A wave owns a buffer of 64-bit words: ST_RESIDENT words of LDS per wave in stats_kernel (4 waves, 64 KiB per workgroup),
// a slice of a global workspace in stats_long_kernel.  The body is the same; only the storage differs.  CROSSOVER: a series of
// at most ST_RESIDENT = 2,048 rows takes the LDS kernel, a longer one the workspace kernel (launched only when the block has more
// than 2,048 rows; a fixed number of waves walks the long series, so the workspace stays bounded).
//
//   1. load the series once (lane = row), count NULLs and NaNs, compact the remaining values into the buffer in arrival order
//      (ballot + prefix count); leading / trailing zeros come from the ballots of this pass (they walk the ORIGINAL rows)
//   2. arrival-order sweep: sign counts, sum, min, max, the two plateau figures (run boundaries by ballot, a run's length is the
//      distance to the previous boundary)
//   3. two-pass moments as the source: with the mean of step 2, one sweep gives the centred sums of powers 2, 3, 4, the lagged
//      products 1, 2, 4, 7, 12, the regression sums and the ten entropy bins
//   4. stability: the source sums every rolling window afresh (O(n w)).  Here a lane owns a block of consecutive windows, sums the
//      first one and slides; the values are centred by the mean first, so on data with a large level the window sums keep the
//      digits the figure is made of.  Second pass over the same windows for the population deviation (nothing is stored).
//   5. the values become keys of a total order (negatives: all bits flipped, others: sign bit flipped) and are sorted in place by a
//      bitonic network; median, quartiles, trimmed mean, the distinct count (key changes) and the Hill tail index (the k + 1 largest
//      magnitudes sit at the two ends: a short merge) read the sorted buffer
//   6. dates: the buffer is reused for the int64 dates, sorted by the same network unless a ballot shows that they ascend
//
// Every wave sum is an xor butterfly over per-lane partial sums: a fixed order, no atomics, the same bits on every run and through
// every entry.  The order differs from the source's left-to-right sums and ln is dm_log: the figures that are sums meet the
// restatement tests/stats_ref.py within the measured tolerance of DESIGN.md section 3; counts, min, max, range and the percentiles
// are exact.  A float -> index cast is clamped by hand where Rust's `as usize` saturates.
//
// The key functions and the network (st_key, st_unkey, st_sync, st_sort) live in wave_sort.hpp, shared with conformal.hip.
//
// ANOFOX_STATS_SKIP (an experiment build only, tools/time_stats.py --ab): bit 0 leaves out step 4, bit 1 the sorting network of step
// 5, so that the time of each can be read from the difference.  The figures of such a build are wrong by design; the product is
// built without the switch.
#include "kernels.hpp"
#include "det_math.hpp"
#include "civil_date.hpp"
#include "wave_sort.hpp"

#ifndef ANOFOX_STATS_SKIP
#define ANOFOX_STATS_SKIP 0
#endif

namespace anofox {

namespace {

constexpr int ST_WAVES = 4;
constexpr int ST_BLOCK = 64 * ST_WAVES;
constexpr double ST_EPS = 2.220446049250313e-16;             // f64::EPSILON

__device__ __forceinline__ double st_wave_sum(double v)
{
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int st_wave_max(int v)
{
    for (int o = 32; o >= 1; o >>= 1) { const int w = __shfl_xor(v, o); v = w > v ? w : v; }
    return v;
}
__device__ __forceinline__ double st_wave_fmin(double v)
{
    for (int o = 32; o >= 1; o >>= 1) { const double w = __shfl_xor(v, o); v = w < v ? w : v; }
    return v;
}
__device__ __forceinline__ double st_wave_fmax(double v)
{
    for (int o = 32; o >= 1; o >>= 1) { const double w = __shfl_xor(v, o); v = w > v ? w : v; }
    return v;
}
__device__ __forceinline__ int st_prev_bit(uint64_t mask, int lane)      // highest set bit below `lane`, -1 if none
{
    const uint64_t below = mask & ((1ull << lane) - 1ull);
    return below ? 63 - __clzll((long long)below) : -1;
}

// year * 12 + month, year * 4 + quarter or year of micros_to_datetime(us) (stats.rs:365-371; civil_date.hpp, shared with the gaps
// stage of dataprep.hip)
__device__ __forceinline__ int64_t st_period(int64_t us, int type)
{
    int64_t y, m;
    cd_year_month(us, y, m);
    return type == STATS_FREQ_MONTHLY ? y * 12 + m : type == STATS_FREQ_QUARTERLY ? y * 4 + (m - 1) / 3 : y;
}

template <class B>
__device__ __forceinline__ double st_percentile(B buf, int m, double p)
{
    if (m == 1) return st_unkey(buf[0]);
    const double n = (double)m;
    const double idx = p * (n - 1.0);
    const int lower = (int)floor(idx), upper = (int)ceil(idx);
    const double frac = idx - (double)lower;
    if (upper >= m) return st_unkey(buf[m - 1]);
    return st_unkey(buf[lower]) * (1.0 - frac) + st_unkey(buf[upper]) * frac;
}

// all figures of series s (n rows, 0 < n <= capacity of buf)
template <class B>
__device__ __forceinline__ void st_series(const StatsArgs &a, int s, int n, B buf, int lane)
{
    const double nan = __builtin_nan("");
    const size_t ld = a.ld;
    int64_t *oi = a.out_int + s;
    double *of = a.out_fp + s;

    // ---- 1. load, count, compact ----
    int m = 0, n_null = 0, n_nan = 0, first_brk = n, last_brk = -1;
    for (int t0 = 0; t0 < n; t0 += 64) {
        const int tl = t0 + lane;
        const bool in = tl < n;
        const double v = in ? a.y[(size_t)tl * ld + s] : 0.0;
        const bool ok = in && (!a.valid || a.valid[(size_t)tl * ld + s] != 0);
        const bool isn = ok && v != v;
        const bool keep = ok && !isn;
        const uint64_t mask = __ballot(keep);
        n_null += __popcll(__ballot(in && !ok));
        n_nan += __popcll(__ballot(isn));
        if (keep) buf[m + __popcll(mask & ((1ull << lane) - 1ull))] = dm_bits(v);
        m += __popcll(mask);
        const uint64_t brk = __ballot(in && !(keep && v == 0.0));
        if (brk) {
            if (last_brk < 0) first_brk = t0 + __ffsll((long long)brk) - 1;
            last_brk = t0 + 63 - __clzll((long long)brk);
        }
    }
    st_sync();

    int64_t iv[STATS_N_INT];
    double fv[STATS_N_FP];
#pragma unroll
    for (int i = 0; i < STATS_N_INT; i++) iv[i] = 0;
#pragma unroll
    for (int i = 0; i < STATS_N_FP; i++) fv[i] = 0.0;
    iv[0] = n; iv[1] = n_null; iv[2] = n_nan;

    if (m > 0) {
        // ---- 2. arrival-order sweep ----
        int n_zero = 0, n_pos = 0, n_neg = 0, n_abs = 0;
        double lsum = 0.0, lmin = __builtin_huge_val(), lmax = -__builtin_huge_val();
        int run_max = 0, run_start = 0;                      // plateau_size
        int nz_max = 0, nz_start = 0; bool nz_start_zero = false;   // plateau_size_nonzero: the last boundary and whether it is a zero
        for (int c0 = 0; c0 < m; c0 += 64) {
            const int i = c0 + lane;
            const bool in = i < m;
            const uint64_t b = in ? buf[i] : 0ull;
            const uint64_t pb = (in && i > 0) ? buf[i - 1] : 0ull;
            const double v = dm_from_bits(b), pv = dm_from_bits(pb);
            const bool z = in && v == 0.0;
            n_zero += __popcll(__ballot(z));
            n_pos += __popcll(__ballot(in && v > 0.0));
            n_neg += __popcll(__ballot(in && v < 0.0));
            n_abs += __popcll(__ballot(in && fabs(v) > ST_EPS));
            if (in) { lsum += v; lmin = v < lmin ? v : lmin; lmax = v > lmax ? v : lmax; }
            const bool start = in && (i == 0 || b != pb);
            const uint64_t smask = __ballot(start);
            if (start && i > 0) {
                const int pbit = st_prev_bit(smask, lane);
                const int len = i - (pbit >= 0 ? c0 + pbit : run_start);
                run_max = len > run_max ? len : run_max;
            }
            if (smask) run_start = c0 + 63 - __clzll((long long)smask);
            const bool bnd = in && (z || i == 0 || pv == 0.0 || b != pb);
            const uint64_t bmask = __ballot(bnd), zmask = __ballot(z);
            if (bnd && i > 0) {
                const int pbit = st_prev_bit(bmask, lane);
                const int p = pbit >= 0 ? c0 + pbit : nz_start;
                const bool pz = pbit >= 0 ? ((zmask >> pbit) & 1ull) != 0 : nz_start_zero;
                const int len = pz ? 0 : i - p;
                nz_max = len > nz_max ? len : nz_max;
            }
            if (bmask) {
                const int hb = 63 - __clzll((long long)bmask);
                nz_start = c0 + hb;
                nz_start_zero = ((zmask >> hb) & 1ull) != 0;
            }
        }
        run_max = st_wave_max(run_max);
        nz_max = st_wave_max(nz_max);
        if (m - run_start > run_max) run_max = m - run_start;
        if (!nz_start_zero && m - nz_start > nz_max) nz_max = m - nz_start;
        const double nf = (double)m;
        const double sum = st_wave_sum(lsum);
        const double mean = sum / nf;
        const double vmin = st_wave_fmin(lmin), vmax = st_wave_fmax(lmax);
        const double range = vmax - vmin;

        // ---- 3. centred sums, lagged products, regression sums, entropy bins ----
        double s2 = 0.0, s3 = 0.0, s4 = 0.0, l1 = 0.0, l2 = 0.0, l4 = 0.0, l7 = 0.0, l12 = 0.0, sxy = 0.0, sxx = 0.0;
        const double x_mean = (nf - 1.0) / 2.0;
        const bool want_bins = m >= 10 && !(fabs(range) < ST_EPS);
        int bins[10];
#pragma unroll
        for (int q = 0; q < 10; q++) bins[q] = 0;
        for (int c0 = 0; c0 < m; c0 += 64) {
            const int i = c0 + lane;
            const bool in = i < m;
            int bin = -1;
            if (in) {
                const double v = dm_from_bits(buf[i]);
                const double d = v - mean;
                const double d2 = d * d;
                s2 += d2; s3 += d2 * d; s4 += d2 * d2;
                if (i >= 1) l1 += d * (dm_from_bits(buf[i - 1]) - mean);
                if (i >= 2) l2 += d * (dm_from_bits(buf[i - 2]) - mean);
                if (i >= 4) l4 += d * (dm_from_bits(buf[i - 4]) - mean);
                if (i >= 7) l7 += d * (dm_from_bits(buf[i - 7]) - mean);
                if (i >= 12) l12 += d * (dm_from_bits(buf[i - 12]) - mean);
                const double x = (double)i - x_mean;
                sxy += x * d; sxx += x * x;
                const double r = round(((v - vmin) / range) * 9.0);
                bin = !(r >= 0.0) ? 0 : r >= 9.0 ? 9 : (int)r;         // Rust's saturating cast, then min(9)
            }
            if (want_bins) {
#pragma unroll
                for (int q = 0; q < 10; q++) bins[q] += __popcll(__ballot(bin == q));
            }
        }
        s2 = st_wave_sum(s2); s3 = st_wave_sum(s3); s4 = st_wave_sum(s4);
        l1 = st_wave_sum(l1); l2 = st_wave_sum(l2); l4 = st_wave_sum(l4); l7 = st_wave_sum(l7); l12 = st_wave_sum(l12);
        sxy = st_wave_sum(sxy); sxx = st_wave_sum(sxx);

        const double variance = m > 1 ? s2 / (double)(m - 1) : 0.0;
        const double sd = sqrt(variance);
        const double cv = fabs(mean) > ST_EPS ? sd / fabs(mean) : nan;
        double skew = nan, kurt = nan;
        if (m > 2 && sd > ST_EPS) {
            const double m3 = s3 / nf;
            const double g1 = m3 / (sd * sd * sd);
            skew = g1 * sqrt(nf * (nf - 1.0)) / (nf - 2.0);
        }
        if (m > 3 && sd > ST_EPS) {
            const double m4 = s4 / nf;
            const double sd2 = sd * sd;
            const double g2 = m4 / (sd2 * sd2) - 3.0;
            kurt = (nf - 1.0) / ((nf - 2.0) * (nf - 3.0)) * ((nf + 1.0) * g2 + 6.0);
        }
        const bool finite_sk = fabs(skew) < __builtin_huge_val(), finite_ku = fabs(kurt) < __builtin_huge_val();
        const double bimod = (m > 3 && finite_sk && finite_ku) ? (skew * skew + 1.0) / (kurt + 3.0) : nan;
        const bool flat = fabs(s2) < ST_EPS;
        const double acf1 = m <= 1 ? nan : flat ? 0.0 : l1 / s2;
        double trend = 0.0, season = 0.0;
        if (m >= 4) {
            if (fabs(sxx) > ST_EPS && fabs(s2) > ST_EPS) {
                const double r = sqrt((sxy * sxy) / (sxx * s2));
                trend = r < 0.0 ? 0.0 : r > 1.0 ? 1.0 : r;
            }
            const double lag[4] = {m <= 2 ? nan : flat ? 0.0 : fabs(l2 / s2), m <= 4 ? nan : flat ? 0.0 : fabs(l4 / s2),
                                   m <= 7 ? nan : flat ? 0.0 : fabs(l7 / s2), m <= 12 ? nan : flat ? 0.0 : fabs(l12 / s2)};
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (fabs(lag[q]) < __builtin_huge_val() && lag[q] > season) season = lag[q];
            season = season > 1.0 ? 1.0 : season;
        }
        double entropy = nan;
        if (m >= 10) {
            entropy = 0.0;
            if (want_bins) {
#pragma unroll
                for (int q = 0; q < 10; q++)
                    if (bins[q] > 0) {
                        const double p = (double)bins[q] / nf;
                        entropy -= p * dm_log(p);
                    }
            }
        }

        // ---- 4. stability ----
        double stab = nan;
        if (m >= 10 && !(ANOFOX_STATS_SKIP & 1)) {
            const int w = m / 5 > 3 ? m / 5 : 3;
            const int K = m - w + 1;
            const int per = ((K + 63) / 64) | 1;              // windows per lane; odd, so the lanes' strides spread over the LDS banks
            const int j0 = lane * per;
            const int j1 = j0 + per < K ? j0 + per : K;
            const double wf = (double)w, kf = (double)K;
            double acc = 0.0, rm_mean_c = 0.0;
            for (int pass = 0; pass < 2; pass++) {
                if (pass == 1) { rm_mean_c = st_wave_sum(acc) / kf; acc = 0.0; }
                if (j0 < K) {
                    double S = 0.0;
                    for (int i = j0; i < j0 + w; i++) S += dm_from_bits(buf[i]) - mean;
                    for (int j = j0;;) {
                        const double rm = S / wf;
                        if (pass == 0) acc += rm;
                        else { const double d = rm - rm_mean_c; acc += d * d; }
                        if (++j >= j1) break;
                        S += dm_from_bits(buf[j + w - 1]) - mean;
                        S -= dm_from_bits(buf[j - 1]) - mean;
                    }
                }
            }
            const double rm_std = sqrt(st_wave_sum(acc) / kf);
            const double rm_mean = mean + rm_mean_c;
            stab = fabs(rm_mean) > ST_EPS ? 1.0 / (rm_std / fabs(rm_mean) + 0.01) : nan;
        }

        // ---- 5. sort, selections ----
        int p2 = 1;
        while (p2 < m) p2 <<= 1;
        for (int i = lane; i < p2; i += 64) buf[i] = i < m ? st_key(buf[i]) : ~0ull;
        st_sync();
        if (!(ANOFOX_STATS_SKIP & 2)) st_sort(buf, p2, lane);
        int n_uni = 0;
        double tsum = 0.0;
        const int trim0 = (int)floor(nf * 0.1);
        const int trim = 2 * trim0 >= m ? 0 : trim0;
        for (int c0 = 0; c0 < m; c0 += 64) {
            const int i = c0 + lane;
            const bool in = i < m;
            const uint64_t k = in ? buf[i] : 0ull;
            n_uni += __popcll(__ballot(in && (i == 0 || k != buf[i - 1])));
            if (in && i >= trim && i < m - trim) tsum += st_unkey(k);
        }
        const double tmean = st_wave_sum(tsum) / (double)(m - 2 * trim);
        const double med = st_percentile(buf, m, 0.5), q1 = st_percentile(buf, m, 0.25), q3 = st_percentile(buf, m, 0.75);
        double tail = nan;
        if (m >= 10 && n_abs >= 10) {
            int k = (int)floor(sqrt((double)n_abs));
            k = k < 2 ? 2 : k;
            k = k > n_abs - 1 ? n_abs - 1 : k;
            double thr = 0.0;
            {
                int lo = 0, hi = m - 1;
                for (int r = 0; r <= k; r++) {
                    const double x = fabs(st_unkey(buf[lo])), y = fabs(st_unkey(buf[hi]));
                    if (x > y) { thr = x; lo++; } else { thr = y; hi--; }
                }
            }
            if (thr > ST_EPS) {
                double part = 0.0;
                int lo = 0, hi = m - 1;
                for (int r = 0; r < k; r++) {
                    const double x = fabs(st_unkey(buf[lo])), y = fabs(st_unkey(buf[hi]));
                    double big;
                    if (x > y) { big = x; lo++; } else { big = y; hi--; }
                    if ((r & 63) == lane) part += dm_log(big / thr);
                }
                const double h = st_wave_sum(part) / (double)k;
                tail = h <= ST_EPS ? nan : 1.0 / h;
            }
        }
        iv[3] = n_zero; iv[4] = n_pos; iv[5] = n_neg; iv[6] = n_uni; iv[7] = n_uni == 1 ? 1 : 0;
        iv[8] = first_brk; iv[9] = n - 1 - last_brk; iv[10] = run_max; iv[11] = nz_max;
        fv[0] = mean; fv[1] = med; fv[2] = sd; fv[3] = variance; fv[4] = vmin; fv[5] = vmax; fv[6] = range; fv[7] = sum;
        fv[8] = skew; fv[9] = kurt; fv[10] = tail; fv[11] = bimod; fv[12] = tmean; fv[13] = cv; fv[14] = q1; fv[15] = q3;
        fv[16] = q3 - q1; fv[17] = acf1; fv[18] = trend; fv[19] = season; fv[20] = entropy; fv[21] = stab;
    }

    // ---- 6. dates ----
    int64_t expected = -1, gaps = -1;
    if (a.dates) {
        st_sync();
        bool unsorted = false;
        for (int t0 = 0; t0 < n; t0 += 64) {
            const int tl = t0 + lane;
            const bool in = tl < n;
            const int64_t d = in ? a.dates[(size_t)tl * ld + s] : 0;
            const int64_t dp = (in && tl > 0) ? a.dates[(size_t)(tl - 1) * ld + s] : d;
            if (in) buf[tl] = (uint64_t)d ^ ST_SIGN;
            if (__ballot(in && d < dp)) unsorted = true;
        }
        int p2 = 1;
        while (p2 < n) p2 <<= 1;
        if (unsorted)
            for (int i = n + lane; i < p2; i += 64) buf[i] = ~0ull;
        st_sync();
        if (unsorted) st_sort(buf, p2, lane);
        if (n < 2) {
            expected = n; gaps = 0;
        } else if (a.freq_type != STATS_FREQ_FIXED) {
            const int type = a.freq_type;
            const int64_t pf = st_period((int64_t)(buf[0] ^ ST_SIGN), type), pl = st_period((int64_t)(buf[n - 1] ^ ST_SIGN), type);
            expected = (int64_t)(int32_t)((int32_t)pl - (int32_t)pf + 1);
            int g = 0;
            for (int c0 = 1; c0 < n; c0 += 64) {
                const int i = c0 + lane;
                const bool in = i < n;
                const int64_t p0 = in ? st_period((int64_t)(buf[i - 1] ^ ST_SIGN), type) : 0;
                const int64_t p1 = in ? st_period((int64_t)(buf[i] ^ ST_SIGN), type) : 0;
                g += __popcll(__ballot(in && p1 - p0 > 1));
            }
            gaps = g;
        } else if (a.freq_us > 0) {
            const uint64_t first = buf[0] ^ ST_SIGN, last = buf[n - 1] ^ ST_SIGN;
            const int64_t duration = (int64_t)(last - first);
            expected = duration / a.freq_us + 1;
            const double tf = (double)a.freq_us * 1.5;
            const int64_t thr = tf >= 9223372036854775807.0 ? INT64_MAX : (int64_t)tf;
            int g = 0;
            for (int c0 = 1; c0 < n; c0 += 64) {
                const int i = c0 + lane;
                const bool in = i < n;
                const int64_t step = in ? (int64_t)((buf[i] ^ ST_SIGN) - (buf[i - 1] ^ ST_SIGN)) : 0;
                g += __popcll(__ballot(in && step > thr));
            }
            gaps = g;
        }
    }
    iv[12] = expected; iv[13] = gaps;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < STATS_N_INT; i++) oi[(size_t)i * ld] = iv[i];
#pragma unroll
        for (int i = 0; i < STATS_N_FP; i++) of[(size_t)i * ld] = fv[i];
    }
}

// length == 0: the FFI wrapper's default (types.rs:238-279), counts 0 and every floating figure NaN, no date figures
__device__ __forceinline__ void st_empty(const StatsArgs &a, int s, int lane)
{
    if (lane != 0) return;
    for (int i = 0; i < STATS_N_INT; i++) a.out_int[(size_t)i * a.ld + s] = i < 12 ? 0 : -1;
    for (int i = 0; i < STATS_N_FP; i++) a.out_fp[(size_t)i * a.ld + s] = __builtin_nan("");
}

__device__ __forceinline__ int st_length(const StatsArgs &a, int s)
{
    int n = a.len[s];
    if (n < 0) n = 0;
    if ((size_t)n > a.t_rows) n = (int)a.t_rows;
    return n;
}

// series of at most STATS_RESIDENT rows, the buffer in LDS
__global__ __launch_bounds__(ST_BLOCK) void stats_kernel(const StatsArgs a)
{
    __shared__ uint64_t lds[ST_WAVES * STATS_RESIDENT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = blockIdx.x * ST_WAVES + wave;
    if (s >= a.n_series) return;                               // (wave-uniform; the kernel has no workgroup barrier)
    const int n = st_length(a, s);
    if (n > STATS_RESIDENT) return;                            // stats_long_kernel answers it
    if (n == 0) { st_empty(a, s, lane); return; }
    st_series(a, s, n, lds + wave * STATS_RESIDENT, lane);
}

// longer series, the buffer in the global workspace: a.work_waves waves walk them
__global__ __launch_bounds__(ST_BLOCK) void stats_long_kernel(const StatsArgs a)
{
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * ST_WAVES + (threadIdx.x >> 6);
    if (w >= a.work_waves) return;
    uint64_t *buf = a.work + (size_t)w * a.work_stride;
    for (int s = w; s < a.n_series; s += a.work_waves) {
        const int n = st_length(a, s);
        if (n <= STATS_RESIDENT || (size_t)n > a.work_stride) continue;
        st_series(a, s, n, buf, lane);
        st_sync();
    }
}

} // namespace

size_t stats_work_stride(size_t t_rows)
{
    if (t_rows <= (size_t)STATS_RESIDENT) return 0;
    size_t p2 = 1;
    while (p2 < t_rows) p2 <<= 1;
    return p2;
}

int stats_work_waves(int n_series)
{
    return n_series < STATS_WORK_WAVES ? n_series : STATS_WORK_WAVES;
}

void launch_stats(const StatsArgs &a, hipStream_t stream)
{
    if (a.n_series <= 0) return;
    const int blocks = (a.n_series + ST_WAVES - 1) / ST_WAVES;
    hipLaunchKernelGGL(stats_kernel, dim3(blocks), dim3(ST_BLOCK), 0, stream, a);
    if (a.t_rows > (size_t)STATS_RESIDENT && a.work && a.work_waves > 0) {
        const int lblocks = (a.work_waves + ST_WAVES - 1) / ST_WAVES;
        hipLaunchKernelGGL(stats_long_kernel, dim3(lblocks), dim3(ST_BLOCK), 0, stream, a);
    }
}

} // namespace anofox
