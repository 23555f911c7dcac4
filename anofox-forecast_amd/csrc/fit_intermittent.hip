// fit_intermittent.hip -- the intermittent-demand models: CrostonClassic, CrostonSBA, TSB (one streamed pass) and ADIDA, IMAPA
// (SES with a bounded grid-refined alpha on temporally aggregated series).  Every kernel reads the time-major fp64 block
// y[t * ld + s] with one lane per series, so the 64 lanes of a wave read 64 consecutive columns of one row; lengths are ragged.
// The arithmetic is restated op for op by tests/intermittent_ref.py (plain mul / add, -ffp-contract=off): results are bit-identical.
#include "kernels.hpp"

namespace anofox {

namespace {

constexpr int IM_BLOCK = 64;            // one wave: a workgroup is a group of 64 consecutive series
constexpr double IM_ALPHA = 0.1;        // Croston / SBA / TSB smoothing of sizes, intervals and the demand indicator
constexpr double IM_SBA = 0.95;         // Syntetos-Boylan bias correction
constexpr int IM_PASSES = 16;           // SESopt: 16 passes of a 9-point grid refine of alpha over [0.1, 0.3]
constexpr int IM_POINTS = 9;
constexpr int IM_ROWS = 16;             // rows loaded ahead per step of a row loop: one wave per SIMD is latency-bound on its loads,
                                        // a block of loads in flight hides it (measured on the M5 block: ADIDA 19.7 ms with one at a time)

// One pass over the rows per series: SES(0.1) of the demand sizes, of the inter-demand intervals and of the demand indicator, the
// demand count c and the aggregation level K = round half up of (i_last + 1) / c (the mean interval).  Writes the point forecast of
// CrostonClassic / CrostonSBA / TSB, and for ADIDA / IMAPA the 0.0 forecast of a series without demand (the others come later);
// level[s] = K (0: no demand), group_max[g] / group_max[n_groups] = largest K of the group / of the batch.
__global__ __launch_bounds__(IM_BLOCK) void croston_kernel(const IntermittentArgs a)
{
    const int s = blockIdx.x * IM_BLOCK + threadIdx.x;
    if (s >= a.n_series) return;
    const int n = a.len[s];
    if (n <= 0) { a.level[s] = 0; return; }
    const double *y = a.y + s;
    const size_t ld = a.ld;
    double lz = 0.0, lp = 0.0, ldem = 0.0;
    int c = 0, last = -1;
    for (int t0 = 0; t0 < n; t0 += IM_ROWS) {
        double vb[IM_ROWS];
#pragma unroll
        for (int u = 0; u < IM_ROWS; u++) vb[u] = t0 + u < n ? y[(size_t)(t0 + u) * ld] : 0.0;
#pragma unroll
        for (int u = 0; u < IM_ROWS; u++) {
            const int t = t0 + u;
            if (t >= n) break;
            const double v = vb[u];
            const bool dem = v != 0.0;
            const double d = dem ? 1.0 : 0.0;
            if (t == 0) ldem = d;
            else { const double e = d - ldem; ldem = ldem + IM_ALPHA * e; }
            const double p = (double)(t - last);
            const double ez = v - lz, ep = p - lp;
            const double uz = lz + IM_ALPHA * ez, up = lp + IM_ALPHA * ep;
            lz = dem ? (c == 0 ? v : uz) : lz;
            lp = dem ? (c == 0 ? p : up) : lp;
            c += dem ? 1 : 0;
            last = dem ? t : last;
        }
    }
    const int K = c > 0 ? (2 * (last + 1) + c) / (2 * c) : 0;
    a.level[s] = K;
    a.detail[s] = FIT_OK;
    if (K > 0) {
        atomicMax(a.group_max + blockIdx.x, K);
        atomicMax(a.group_max + a.n_groups, K);
    }
    double f = 0.0;
    if (c > 0) {
        switch (a.kind) {
        case IK_CROSTON: f = lz / lp; break;
        case IK_SBA: f = IM_SBA * (lz / lp); break;
        case IK_TSB: f = ldem * lz; break;
        default: return;                // ADIDA / IMAPA: agg_ses_kernel writes it
        }
    }
    double *out = a.yhat + (size_t)s * a.h;
    for (int i = 0; i < a.h; i++) out[i] = f;
}

// SESopt of the level-k sums of one series: drop the first n % k rows, sum each following block of k rows (left to right, from
// 0.0), run SES on those sums for the 9 grid points of every pass (l = x[0]; e = x - l; sse += e*e; l += a*e), keep the first
// minimum of sse and narrow [lo, hi] to its neighbours; the result is the final level at the last pass's best point.  The 9
// levels and sse accumulators live in registers; the sums are formed on the fly from the block, no aggregated copy is stored.
__device__ double ses_opt_level(const double *y, size_t ld, int n, int k)
{
    const int off = n % k;
    double lo = 0.1, hi = 0.3, f = 0.0;
    for (int pass = 0; pass < IM_PASSES; pass++) {
        const double step = (hi - lo) / 8.0;
        double al[IM_POINTS], l[IM_POINTS], sse[IM_POINTS];
#pragma unroll
        for (int j = 0; j < IM_POINTS - 1; j++) al[j] = lo + (double)j * step;
        al[IM_POINTS - 1] = hi;
#pragma unroll
        for (int j = 0; j < IM_POINTS; j++) { l[j] = 0.0; sse[j] = 0.0; }
        double acc = 0.0;
        int cnt = 0;
        bool first = true;
        for (int t0 = off; t0 < n; t0 += IM_ROWS) {
            double vb[IM_ROWS];
#pragma unroll
            for (int u = 0; u < IM_ROWS; u++) vb[u] = t0 + u < n ? y[(size_t)(t0 + u) * ld] : 0.0;
#pragma unroll
            for (int u = 0; u < IM_ROWS; u++) {
                if (t0 + u >= n) break;
                acc = acc + vb[u];
                if (++cnt == k) {
                    if (first) {
#pragma unroll
                        for (int j = 0; j < IM_POINTS; j++) l[j] = acc;
                        first = false;
                    } else {
#pragma unroll
                        for (int j = 0; j < IM_POINTS; j++) {
                            const double e = acc - l[j];
                            sse[j] = sse[j] + e * e;
                            l[j] = l[j] + al[j] * e;
                        }
                    }
                    acc = 0.0;
                    cnt = 0;
                }
            }
        }
        // first minimum (constant indices only: the arrays stay in registers)
        double best = sse[0], nlo = al[0], nhi = al[1];
        f = l[0];
#pragma unroll
        for (int j = 1; j < IM_POINTS; j++) {
            if (sse[j] < best) {
                best = sse[j]; f = l[j];
                nlo = al[j - 1]; nhi = al[j + 1 < IM_POINTS ? j + 1 : IM_POINTS - 1];
            }
        }
        lo = nlo; hi = nhi;
    }
    return f;
}

// ADIDA: one workgroup per group of 64 series, each lane at its own level K.  IMAPA: one workgroup per (group, level k), enumerated
// level-major (all groups at k = 1, then k = 2, ...); a workgroup whose group has no series with K >= k leaves at once, and the
// lanes of one workgroup share k.  IMAPA stores SESopt / k of every (series, level) at level_fc[(k - 1) * ld + s]: the per-series
// mean adds them in level order (imapa_mean_kernel), so the result does not depend on which workgroup finished first.
__global__ __launch_bounds__(IM_BLOCK) void agg_ses_kernel(const IntermittentArgs a)
{
    const bool imapa = a.kind == IK_IMAPA;
    const int g = imapa ? (int)(blockIdx.x % (unsigned)a.n_groups) : (int)blockIdx.x;
    const int kw = imapa ? (int)(blockIdx.x / (unsigned)a.n_groups) + 1 : 0;
    if (imapa && (kw > a.group_max[g] || kw > a.n_levels)) return;
    const int s = g * IM_BLOCK + threadIdx.x;
    if (s >= a.n_series) return;
    const int n = a.len[s];
    const int K = a.level[s];
    if (n <= 0 || K <= 0 || (imapa && K < kw)) return;
    const int k = imapa ? kw : K;
    const double f = ses_opt_level(a.y + s, a.ld, n, k) / (double)k;
    if (imapa) {
        a.level_fc[(size_t)(k - 1) * a.ld + s] = f;
    } else {
        double *out = a.yhat + (size_t)s * a.h;
        for (int i = 0; i < a.h; i++) out[i] = f;
    }
}

// IMAPA: (sum over k = 1..K of SESopt_k / k, in level order) / K
__global__ __launch_bounds__(256) void imapa_mean_kernel(const IntermittentArgs a)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= a.n_series || a.len[s] <= 0) return;
    const int K = a.level[s];
    if (K <= 0) return;                 // no demand: croston_kernel wrote 0.0
    double acc = 0.0;
    for (int k = 1; k <= K; k++) acc = acc + a.level_fc[(size_t)(k - 1) * a.ld + s];
    const double f = acc / (double)K;
    double *out = a.yhat + (size_t)s * a.h;
    for (int i = 0; i < a.h; i++) out[i] = f;
}

} // namespace

int intermittent_groups(int n_series) { return (n_series + IM_BLOCK - 1) / IM_BLOCK; }

void launch_croston(const IntermittentArgs &a, hipStream_t stream)
{
    if (a.n_series <= 0) return;
    hipLaunchKernelGGL(croston_kernel, dim3((unsigned)a.n_groups), dim3(IM_BLOCK), 0, stream, a);
}

void launch_agg_ses(const IntermittentArgs &a, hipStream_t stream)
{
    if (a.n_series <= 0) return;
    if (a.kind == IK_ADIDA) {
        hipLaunchKernelGGL(agg_ses_kernel, dim3((unsigned)a.n_groups), dim3(IM_BLOCK), 0, stream, a);
        return;
    }
    if (a.n_levels <= 0) return;        // no series has a demand
    const unsigned long long blocks = (unsigned long long)a.n_groups * (unsigned long long)a.n_levels;
    if (blocks > 0xffffffffull) throw std::runtime_error("IMAPA: too many (group, level) workgroups for one launch");
    hipLaunchKernelGGL(agg_ses_kernel, dim3((unsigned)blocks), dim3(IM_BLOCK), 0, stream, a);
    hipLaunchKernelGGL(imapa_mean_kernel, dim3((unsigned)((a.n_series + 255) / 256)), dim3(256), 0, stream, a);
}

} // namespace anofox
