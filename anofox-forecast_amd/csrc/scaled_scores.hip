// scaled_scores.hip -- the in-sample scale of every column of a time-major block and the scaled, weighted scores of column ranges
// (DESIGN.md section 3 "Scaled scores"): what RMSSE, MASE and the scaled pinball loss divide by, the weight mass of a column, and the
// weighted mean of the scaled losses over the columns of a level -- WRMSSE and WSPL of the M5 competition (Makridakis et al., the
// competitors' guide).  The names are this package's own; tests/scaled_scores_ref.py is the definition, bit for bit.
//
// Plain fp64 operations (-ffp-contract=off: a product is rounded, then added), the compiled division and sqrt (both correctly
// rounded).  The sums over rows are serial from 0.0 in row order; the sums over the columns of a range are the wave sum W of
// path_scores.hip: lane l adds the terms i = l (mod 64) serially from 0.0, and the partials are combined in lane order.
//
//   scale_kernel             one lane per column, one wavefront per workgroup (an M5 block is some 500 to 700 wavefronts on 256 CUs:
//                            whole workgroups of one wave spread them widest).  The chains sq += d * d, ab += |d| are serial by contract,
//                            but the loads do not depend on them: the lane issues the loads of R rows (ANOFOX_SCALE_ROWS, 16), each a
//                            coalesced 512-byte row segment of the wave, and only then runs the R steps of the chains.  Every load is
//                            unconditional, to a row clamped into the block; what a row past the lane's length returns is dropped by a
//                            select.  The lagged value y[t - lag] is the previous row's register for lag 1 and a second stream of
//                            loads, `lag` rows behind and served by the cache, otherwise.  Trimming is a flag per lane: the first row
//                            with y != 0.0 sets t0 and the selects take rows t >= t0 + lag.  The tail is a second short loop over the
//                            last rows of w_src.  No LDS; the rows in flight are registers with compile-time indices (no scratch).
//                            R does not show in the bits: the order of the chain is the row order whatever the block of loads.
//   weighted_ranges_kernel   one wavefront per (range, loss row): lanes stride the columns of the range, form the scaled loss (and
//                            write it), the rounded product with the weight, and the two wave sums.
//   weighted_totals_kernel   one lane: the serial means over the ranges and over the loss rows.
// No atomics.
#include "kernels.hpp"
#include "det_math.hpp"

#ifndef ANOFOX_SCALE_ROWS
#define ANOFOX_SCALE_ROWS 16                                 // rows in flight per lane: measured, profiles/scaled_scores_m5.txt
#endif

namespace anofox {

namespace {

constexpr int SCALE_ROWS = ANOFOX_SCALE_ROWS;
static_assert(SCALE_ROWS == 1 || SCALE_ROWS == 4 || SCALE_ROWS == 8 || SCALE_ROWS == 16 || SCALE_ROWS == 32, "rows in flight: 1, 4, 8, 16 or 32");

__device__ __forceinline__ double ss_lane_value(double v, int l)
{
    const uint64_t u = dm_bits(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, l), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), l);
    return dm_from_bits(((uint64_t)hi << 32) | (uint64_t)lo);
}

// ((a_0 + a_1) + a_2) + ... + a_63 of the lanes' partials; every lane gets the sum
__device__ __forceinline__ double ss_combine(double a)
{
    double w = ss_lane_value(a, 0);
#pragma unroll
    for (int l = 1; l < 64; l++) w = w + ss_lane_value(a, l);
    return w;
}

__device__ __forceinline__ int ss_wave_max(int n)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int o = __shfl_xor(n, off, 64);
        n = o > n ? o : n;
    }
    return n;
}

__device__ __forceinline__ int ss_wave_add(int n)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
    return n;
}

template <int R, bool LAG1>
__global__ __launch_bounds__(64) void scale_kernel(const ScaleArgs a)
{
    const size_t cl = (size_t)blockIdx.x * 64 + threadIdx.x;
    const bool mine = cl < (size_t)a.n_cols;
    const size_t c = mine ? cl : (size_t)a.n_cols - 1;       // (a lane past the block reads the last column and writes nothing)
    int n = mine ? a.len[c] : 0;
    n = n < 0 ? 0 : (n > a.t_rows ? a.t_rows : n);
    const int rows = ss_wave_max(n);                          // (wave-uniform; at most t_rows)
    const int last = a.t_rows - 1, lag = a.lag;
    const size_t ld = a.ld;
    const double *col = a.y + c;
    bool started = a.trim == 0, has_nan = false;
    int t0 = a.trim ? n : 0;
    double sq = 0.0, ab = 0.0, carry = 0.0;
#pragma unroll 1
    for (int b = 0; b < rows; b += R) {
        double v[R], p[R];
#pragma unroll
        for (int i = 0; i < R; i++) {
            const int r = b + i < last ? b + i : last;
            v[i] = col[(size_t)r * ld];
        }
        if (!LAG1) {
#pragma unroll
            for (int i = 0; i < R; i++) {
                int r = (b + i < last ? b + i : last) - lag;
                r = r < 0 ? 0 : r;
                p[i] = col[(size_t)r * ld];
            }
        }
#pragma unroll
        for (int i = 0; i < R; i++) {
            const int t = b + i;
            const double x = v[i];
            const double prev = LAG1 ? (i ? v[i ? i - 1 : 0] : carry) : p[i];
            const bool inside = t < n;
            has_nan = has_nan || (inside && x != x);
            const bool opens = inside && !started && x != 0.0;
            t0 = opens ? t : t0;
            started = started || opens;
            const bool take = inside && t - lag >= t0;
            const double d = x - prev;
            const double dd = d * d;
            const double sq1 = sq + dd, ab1 = ab + fabs(d);
            sq = take ? sq1 : sq;
            ab = take ? ab1 : ab;
        }
        carry = v[R - 1];
    }
    // the tail: rows n - m .. n - 1 of w_src, m = min(tail_rows, n)
    const int m = a.tail_rows < n ? a.tail_rows : n;
    const int m_rows = ss_wave_max(m);
    const int start = n - m;
    const double *wcol = a.w_src + c;
    double tail = 0.0;
#pragma unroll 1
    for (int b = 0; b < m_rows; b += R) {
        double w[R];
#pragma unroll
        for (int i = 0; i < R; i++) {
            int r = start + b + i;
            r = r < last ? r : last;
            w[i] = wcol[(size_t)r * ld];
        }
#pragma unroll
        for (int i = 0; i < R; i++) {
            const bool inside = b + i < m;
            has_nan = has_nan || (inside && w[i] != w[i]);
            const double t1 = tail + w[i];
            tail = inside ? t1 : tail;
        }
    }
    if (!mine) return;
    const double nan = __builtin_nan("");
    const long long n_terms = (long long)n - (long long)t0 - (long long)lag;
    const double dn = (double)n_terms;
    double msd = nan, mad = nan;
    int32_t status = SCALE_SHORT;
    if (n_terms > 0) {
        msd = sq / dn;
        mad = ab / dn;
        status = msd == 0.0 ? SCALE_CONSTANT : SCALE_OK;
        if (status == SCALE_CONSTANT) mad = 0.0;              // (a difference whose square underflows: both scales say constant)
    }
    double terms = dn;
    if (has_nan) { msd = nan; mad = nan; terms = nan; tail = nan; status = SCALE_NAN; }
    a.out[c] = msd;
    a.out[a.ld_out + c] = mad;
    a.out[2 * a.ld_out + c] = terms;
    a.out[3 * a.ld_out + c] = tail;
    a.first[c] = t0;
    a.status[c] = status;
}

// workgroup (g, r): range g, loss row r
__global__ __launch_bounds__(64) void weighted_ranges_kernel(const WeightedScoresArgs a)
{
    const int lane = threadIdx.x;
    const size_t g = blockIdx.x, r = blockIdx.y;
    const size_t cell = g * (size_t)a.n_loss + r;
    const int begin = a.ranges[2 * g], end = a.ranges[2 * g + 1];
    const double nan = __builtin_nan("");
    if (begin < 0 || end <= begin || end > a.n_cols) {         // (wave-uniform) never a cut sum
        if (lane == 0) { a.score[cell] = nan; a.weight_sum[cell] = nan; a.left[cell] = -1; }
        return;
    }
    const double *loss = a.loss + r * a.ld;
    double *scaled = a.scaled ? a.scaled + r * a.ld : nullptr;
    const double inf = __builtin_inf();
    double num = 0.0, den = 0.0;
    int left = 0;
    for (long long c = (long long)begin + lane; c < (long long)end; c += 64) {
        const double sc = a.scale[c], w = a.weight[c];
        const double q = loss[c] / sc;
        const double s = a.transform == 1 ? sqrt(q) : q;
        const bool out = (a.col_status && a.col_status[c] != 0) || !(sc > 0.0 && sc < inf) || !(w >= 0.0) || !(fabs(s) < inf);
        const double term = w * s;
        num = num + (out ? 0.0 : term);
        den = den + (out ? 0.0 : w);
        left += out ? 1 : 0;
        if (scaled) scaled[c] = out ? nan : s;
    }
    const double N = ss_combine(num), D = ss_combine(den);
    left = ss_wave_add(left);
    if (lane == 0) {
        a.score[cell] = D > 0.0 ? N / D : nan;
        a.weight_sum[cell] = D;
        a.left[cell] = left;
    }
}

__global__ __launch_bounds__(64) void weighted_totals_kernel(const WeightedScoresArgs a)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double all = 0.0;
    for (int r = 0; r < a.n_loss; r++) {
        double total = 0.0;
        long long count = 0;
        for (size_t g = 0; g < (size_t)a.n_ranges; g++) {
            const double v = a.score[g * (size_t)a.n_loss + (size_t)r];
            if (v == v) { total = total + v; count++; }
        }
        const double t = count > 0 ? total / (double)count : __builtin_nan("");
        a.total[r] = t;
        all = all + t;
    }
    a.total[a.n_loss] = all / (double)a.n_loss;
}

} // namespace

void launch_scale(const ScaleArgs &a, hipStream_t stream)
{
    if (a.n_cols <= 0) return;
    const unsigned blocks = (unsigned)(((size_t)a.n_cols + 63) / 64);
    if (a.lag == 1) hipLaunchKernelGGL((scale_kernel<SCALE_ROWS, true>), dim3(blocks), dim3(64), 0, stream, a);
    else hipLaunchKernelGGL((scale_kernel<SCALE_ROWS, false>), dim3(blocks), dim3(64), 0, stream, a);
}

void launch_weighted_scores(const WeightedScoresArgs &a, hipStream_t stream)
{
    if (a.n_ranges <= 0 || a.n_loss <= 0) return;
    hipLaunchKernelGGL(weighted_ranges_kernel, dim3((unsigned)a.n_ranges, (unsigned)a.n_loss), dim3(64), 0, stream, a);
    hipLaunchKernelGGL(weighted_totals_kernel, dim3(1), dim3(64), 0, stream, a);
}

} // namespace anofox
