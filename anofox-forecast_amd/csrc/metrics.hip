// metrics.hip -- the twelve forecast accuracy metrics of the reference (metrics.rs: mae, mse, rmse, mape, smape, r2, bias, rmae, mase,
// quantile_loss, mqloss, coverage), every requested figure of a group from ONE pass over its rows.
//
// One lane per group, 64 groups per one-wave workgroup.  The contract is equality of bits with the source's arithmetic, so a lane
// walks its rows in order and every sum is the sequential one from 0.0 that `iter().sum()` forms: the time axis is not split and no
// sum is reordered.  Only + - * /, fabs, sqrt and comparisons occur (-ffp-contract=off, no fused multiply-add anywhere); all running
// sums live in registers, no scratch.  A figure that is not requested is behind a wave-uniform branch; the second sweep over
// `actual` happens only when R^2 is requested (its mean comes first, as in the source).
//
// Two layouts, one arithmetic (metrics_row / metrics_finish are shared).  Element (group s, row t) is at s * stride_s + t * stride_t:
//   * metrics_direct_kernel reads the element itself.  With stride_s == 1 (the project's time-major block) the 64 lanes of a wave
//     read 64 consecutive columns of one row, as croston_kernel does; eight rows are loaded ahead per step (fewer with quantile blocks).
//   * metrics_staged_kernel is for stride_t == 1 (series-major, the [n_series x horizon] layout of the forecast results): there a
//     lane's rows are contiguous and a wave's rows are far apart, so tiles of 64 groups x TR rows go through LDS -- loaded along the
//     contiguous axis, then every lane reads its own row.  A tile row is TR + 1 doubles long: an odd pitch, so the 32 lanes of
//     one LDS access (64-bit reads go half a wave at a time) hit 32 different bank pairs.  TR is the largest power of two for which
//     the tiles of all supplied blocks fit 64 KB.  The lane sees the same values in the same order, hence the same bits.
//
// Row filter (drop_nan): a row in which any supplied block holds a NaN is skipped for every figure and does not count; the order of
// the remaining rows is unchanged.  A block that is not supplied reads as 0.0 and never filters.  With drop_nan the R^2 sweep has to
// read every supplied block again to know which rows count; without it, it reads `actual` alone.
//
// Not part of the contract: the sign of a zero result (Rust's Sum started from 0.0 in older compilers and
// from -0.0 in newer ones; here it is 0.0) and NaN payloads.
#include "kernels.hpp"

namespace anofox {

namespace {

constexpr int MT_BLOCK = 64;
constexpr double MT_EPS = 2.220446049250313e-16;         // f64::EPSILON
constexpr size_t MT_LDS_BYTES = 64 * 1024;               // dynamic LDS the staged kernel may ask for without raising the limit

// which sums the requested figures need: wave-uniform, decided once
struct MtWant {
    bool abs1, sq, mape, smape, act, bias, abs2, ql, mql, cov;
    __device__ explicit MtWant(uint32_t m)
    {
        auto has = [m](int k) { return (m >> k & 1u) != 0; };
        abs1 = has(MF_MAE) || has(MF_RMAE) || has(MF_MASE);
        sq = has(MF_MSE) || has(MF_RMSE) || has(MF_R2);
        mape = has(MF_MAPE); smape = has(MF_SMAPE); act = has(MF_R2); bias = has(MF_BIAS);
        abs2 = has(MF_RMAE) || has(MF_MASE);
        ql = has(MF_QUANTILE_LOSS); mql = has(MF_MQLOSS); cov = has(MF_COVERAGE);
    }
};

template <int NQ> struct MtAcc {
    int n = 0, n_mape = 0, n_smape = 0, n_cov = 0;
    double abs1 = 0.0, sq = 0.0, mape = 0.0, smape = 0.0, act = 0.0, bias = 0.0, abs2 = 0.0, ql = 0.0, tot = 0.0;
    double q[NQ > 0 ? NQ : 1];
};

template <int NQ> struct MtRow {
    double a, f, s, l, u;
    double q[NQ > 0 ? NQ : 1];
};

template <int NQ> __device__ __forceinline__ bool mt_row_has_nan(const MtRow<NQ> &r, int nq)
{
    bool nan = r.a != r.a || r.f != r.f || r.s != r.s || r.l != r.l || r.u != r.u;
#pragma unroll
    for (int k = 0; k < NQ; k++) nan = nan || (k < nq && r.q[k] != r.q[k]);
    return nan;
}

// one row of the first sweep, in the source's operations (metrics.rs:46-54, 70-78, 113-126, 142-159, 225-229, 275-298, 343-362)
template <int NQ> __device__ __forceinline__ void metrics_row(MtAcc<NQ> &c, const MtWant &w, const MetricsArgs &a, const MtRow<NQ> &r, int nq)
{
    if (a.drop_nan && mt_row_has_nan<NQ>(r, nq)) return;
    c.n++;
    const double e = r.a - r.f;
    if (w.abs1) c.abs1 += fabs(e);
    if (w.sq) c.sq += e * e;
    if (w.mape && fabs(r.a) > MT_EPS) { c.mape += fabs(e / r.a); c.n_mape++; }
    if (w.smape) {
        const double den = fabs(r.a) + fabs(r.f);
        if (den > MT_EPS) { c.smape += 2.0 * fabs(e) / den; c.n_smape++; }
    }
    if (w.act) c.act += r.a;
    if (w.bias) c.bias += r.f - r.a;
    if (w.abs2) c.abs2 += fabs(r.a - r.s);
    if (w.ql) c.ql += e >= 0.0 ? a.quantile * e : (a.quantile - 1.0) * e;
    if (w.mql) {
#pragma unroll
        for (int k = 0; k < NQ; k++)
            if (k < nq) {
                const double ek = r.a - r.q[k];
                c.q[k] += ek >= 0.0 ? a.levels[k] * ek : (a.levels[k] - 1.0) * ek;
            }
    }
    if (w.cov && r.a >= r.l && r.a <= r.u) c.n_cov++;
}

template <int NQ> __device__ __forceinline__ void metrics_finish(const MtAcc<NQ> &c, const MetricsArgs &a, int s, int nq)
{
    const double nan = __builtin_nan("");
    const uint32_t m = a.mask;
    auto put = [&](int k, double v) { if (m >> k & 1u) a.figures[(size_t)k * a.ld + s] = v; };
    a.status[s] = c.n > 0 ? METRICS_OK : METRICS_EMPTY;
    if (c.n <= 0) {
        for (int k = 0; k < METRICS_N_FIG; k++) put(k, nan);
        return;
    }
    const double nf = (double)c.n;
    const double mae = c.abs1 / nf, mse = c.sq / nf;
    put(MF_MAE, mae);
    put(MF_MSE, mse);
    if (m >> MF_RMSE & 1u) put(MF_RMSE, sqrt(mse));
    put(MF_MAPE, c.n_mape == 0 ? nan : c.mape / (double)c.n_mape * 100.0);
    put(MF_SMAPE, c.n_smape == 0 ? nan : c.smape / (double)c.n_smape * 100.0);
    put(MF_R2, fabs(c.tot) < MT_EPS ? nan : 1.0 - c.sq / c.tot);
    put(MF_BIAS, c.bias / nf);
    const double mae2 = c.abs2 / nf;
    const double ratio = fabs(mae2) < MT_EPS ? nan : mae / mae2;
    put(MF_RMAE, ratio);
    put(MF_MASE, ratio);
    put(MF_QUANTILE_LOSS, c.ql / nf);
    if (m >> MF_MQLOSS & 1u) {
        double total = 0.0;
#pragma unroll
        for (int k = 0; k < NQ; k++)
            if (k < nq) total += c.q[k] / nf;
        put(MF_MQLOSS, total / (double)nq);
    }
    put(MF_COVERAGE, (double)c.n_cov / nf);
}

template <int NQ> __device__ __forceinline__ void mt_acc_init(MtAcc<NQ> &c)
{
#pragma unroll
    for (int k = 0; k < (NQ > 0 ? NQ : 1); k++) c.q[k] = 0.0;
}

__device__ __forceinline__ int mt_length(const MetricsArgs &a, int s)
{
    if (s >= a.n_groups) return 0;
    const int n = a.len[s];
    const int cap = a.t_rows > (size_t)INT32_MAX ? INT32_MAX : (int)a.t_rows;
    return n < 0 ? 0 : (n > cap ? cap : n);
}

// the blocks a sweep reads: all supplied ones, or (second sweep without the row filter) `actual` alone
struct MtBlocks {
    const double *a, *f, *s, *l, *u, *q;
    int nq;
    __device__ MtBlocks(const MetricsArgs &x, bool all)
        : a(x.actual), f(all ? x.forecast : nullptr), s(all ? x.second : nullptr), l(all ? x.lower : nullptr), u(all ? x.upper : nullptr),
          q(all ? x.quant : nullptr), nq(all && x.quant ? x.n_levels : 0) {}
};

// ------------------------------------------------------------------------------------------------------------------------------
// direct reads (any strides; coalesced when stride_s == 1)
// ------------------------------------------------------------------------------------------------------------------------------
template <int NQ, int ROWS, bool SECOND>
__device__ __forceinline__ void mt_direct_sweep(MtAcc<NQ> &c, const MtWant &w, const MetricsArgs &a, const MtBlocks &b, int s, int n, double mean)
{
    const size_t base = (size_t)s * a.stride_s, st = a.stride_t;
    for (int t0 = 0; t0 < n; t0 += ROWS) {
        MtRow<NQ> r[ROWS];
#pragma unroll
        for (int i = 0; i < ROWS; i++) {
            const bool in = t0 + i < n;
            const size_t off = base + (size_t)(t0 + i) * st;
            r[i].a = in ? b.a[off] : 0.0;
            r[i].f = in && b.f ? b.f[off] : 0.0;
            r[i].s = in && b.s ? b.s[off] : 0.0;
            r[i].l = in && b.l ? b.l[off] : 0.0;
            r[i].u = in && b.u ? b.u[off] : 0.0;
#pragma unroll
            for (int k = 0; k < NQ; k++) r[i].q[k] = in && k < b.nq ? b.q[(size_t)k * a.stride_q + off] : 0.0;
        }
#pragma unroll
        for (int i = 0; i < ROWS; i++) {
            if (t0 + i >= n) break;
            if (!SECOND) metrics_row<NQ>(c, w, a, r[i], b.nq);
            else if (!(a.drop_nan && mt_row_has_nan<NQ>(r[i], b.nq))) { const double d = r[i].a - mean; c.tot += d * d; }
        }
    }
}

template <int NQ, int ROWS>
__global__ __launch_bounds__(MT_BLOCK) void metrics_direct_kernel(const MetricsArgs a)
{
    const int s = blockIdx.x * MT_BLOCK + threadIdx.x;
    if (s >= a.n_groups) return;
    const int n = mt_length(a, s);
    const MtWant w(a.mask);
    MtAcc<NQ> c;
    mt_acc_init<NQ>(c);
    const MtBlocks all(a, true);
    mt_direct_sweep<NQ, ROWS, false>(c, w, a, all, s, n, 0.0);
    if (w.act && c.n > 0) {                  // R^2: the mean first, then ss_tot (metrics.rs:193-201)
        const double mean = c.act / (double)c.n;
        const MtBlocks again(a, a.drop_nan != 0);
        mt_direct_sweep<NQ, ROWS, true>(c, w, a, again, s, n, mean);
    }
    metrics_finish<NQ>(c, a, s, all.nq);
}

// ------------------------------------------------------------------------------------------------------------------------------
// series-major blocks (stride_t == 1) through LDS tiles of 64 groups x TR rows
// ------------------------------------------------------------------------------------------------------------------------------
// tile[r * (TR + 1) + c] = p[(g0 + r) * stride_s + t0 + c]: lane j loads column c = j % TR of the rows j / TR, j / TR + 64 / TR, ...
// A cell beyond its group's length is 0.0 and is never read back (the lane stops at its length).
__device__ __forceinline__ void mt_stage(double *tile, const double *p, const MetricsArgs &a, int g0, int t0, int n, int tr_log2)
{
    const int lane = threadIdx.x, TR = 1 << tr_log2, c = lane & (TR - 1), r0 = lane >> tr_log2, step = MT_BLOCK >> tr_log2;
    for (int i = 0; i < TR; i++) {
        const int r = r0 + i * step;
        const int nr = __shfl(n, r);         // the length of group g0 + r (0 beyond the batch)
        const int t = t0 + c;
        tile[r * (TR + 1) + c] = t < nr ? p[(size_t)(g0 + r) * a.stride_s + t] : 0.0;
    }
}

template <int NQ, bool SECOND>
__device__ __forceinline__ void mt_staged_sweep(MtAcc<NQ> &c, const MtWant &w, const MetricsArgs &a, const MtBlocks &b, double *lds, int g0, int n,
                                                int nmax, int tr_log2, double mean)
{
    const int lane = threadIdx.x, TR = 1 << tr_log2, pitch = TR + 1;
    const size_t tile = (size_t)MT_BLOCK * pitch;
    // one tile per supplied block, in this order (wave-uniform)
    int slots = 0;
    double *ta = lds + tile * slots++;
    double *tf = b.f ? lds + tile * slots++ : nullptr;
    double *ts = b.s ? lds + tile * slots++ : nullptr;
    double *tl = b.l ? lds + tile * slots++ : nullptr;
    double *tu = b.u ? lds + tile * slots++ : nullptr;
    double *tq = lds + tile * slots;
    for (int t0 = 0; t0 < nmax; t0 += TR) {
        __syncthreads();                     // the previous tile has been read
        mt_stage(ta, b.a, a, g0, t0, n, tr_log2);
        if (tf) mt_stage(tf, b.f, a, g0, t0, n, tr_log2);
        if (ts) mt_stage(ts, b.s, a, g0, t0, n, tr_log2);
        if (tl) mt_stage(tl, b.l, a, g0, t0, n, tr_log2);
        if (tu) mt_stage(tu, b.u, a, g0, t0, n, tr_log2);
        for (int k = 0; k < b.nq; k++) mt_stage(tq + tile * k, b.q + (size_t)k * a.stride_q, a, g0, t0, n, tr_log2);
        __syncthreads();
        const int rows = n - t0 < TR ? n - t0 : TR;
        const int at = lane * pitch;
        for (int i = 0; i < rows; i++) {
            MtRow<NQ> r;
            r.a = ta[at + i];
            r.f = tf ? tf[at + i] : 0.0;
            r.s = ts ? ts[at + i] : 0.0;
            r.l = tl ? tl[at + i] : 0.0;
            r.u = tu ? tu[at + i] : 0.0;
#pragma unroll
            for (int k = 0; k < NQ; k++) r.q[k] = k < b.nq ? tq[tile * k + at + i] : 0.0;
            if (!SECOND) metrics_row<NQ>(c, w, a, r, b.nq);
            else if (!(a.drop_nan && mt_row_has_nan<NQ>(r, b.nq))) { const double d = r.a - mean; c.tot += d * d; }
        }
    }
}

template <int NQ>
__global__ __launch_bounds__(MT_BLOCK) void metrics_staged_kernel(const MetricsArgs a, int tr_log2)
{
    extern __shared__ double mt_lds[];
    const int g0 = blockIdx.x * MT_BLOCK, s = g0 + threadIdx.x;
    const int n = mt_length(a, s);           // 0 for the lanes beyond the batch: they stage and wait with the wave, and write nothing
    int nmax = n;
    for (int o = 32; o >= 1; o >>= 1) { const int v = __shfl_xor(nmax, o); nmax = v > nmax ? v : nmax; }
    const MtWant w(a.mask);
    MtAcc<NQ> c;
    mt_acc_init<NQ>(c);
    const MtBlocks all(a, true);
    mt_staged_sweep<NQ, false>(c, w, a, all, mt_lds, g0, n, nmax, tr_log2, 0.0);
    if (w.act) {                             // wave-uniform: every lane takes part in the staging of the second sweep
        const double mean = c.n > 0 ? c.act / (double)c.n : 0.0;
        const MtBlocks again(a, a.drop_nan != 0);
        mt_staged_sweep<NQ, true>(c, w, a, again, mt_lds, g0, n, nmax, tr_log2, mean);
    }
    if (s < a.n_groups) metrics_finish<NQ>(c, a, s, all.nq);
}

} // namespace

void launch_metrics(const MetricsArgs &a, hipStream_t stream)
{
    if (a.n_groups <= 0) return;
    const int nq = a.quant ? a.n_levels : 0;
    const dim3 grid((unsigned)((a.n_groups + MT_BLOCK - 1) / MT_BLOCK)), block(MT_BLOCK);
    const bool staged = a.stride_t == 1 && (a.staging > 0 || (a.staging < 0 && a.stride_s != 1));
    if (staged) {
        const int blocks = 1 + (a.forecast != nullptr) + (a.second != nullptr) + (a.lower != nullptr) + (a.upper != nullptr) + nq;
        int tr_log2 = 6;
        while (tr_log2 > 0 && (size_t)blocks * MT_BLOCK * ((1u << tr_log2) + 1) * sizeof(double) > MT_LDS_BYTES) tr_log2--;
        const size_t lds = (size_t)blocks * MT_BLOCK * ((1u << tr_log2) + 1) * sizeof(double);
        if (nq == 0) hipLaunchKernelGGL(metrics_staged_kernel<0>, grid, block, lds, stream, a, tr_log2);
        else if (nq <= 4) hipLaunchKernelGGL(metrics_staged_kernel<4>, grid, block, lds, stream, a, tr_log2);
        else hipLaunchKernelGGL(metrics_staged_kernel<METRICS_MAX_LEVELS>, grid, block, lds, stream, a, tr_log2);
        return;
    }
    if (nq == 0) hipLaunchKernelGGL((metrics_direct_kernel<0, 8>), grid, block, 0, stream, a);
    else if (nq <= 4) hipLaunchKernelGGL((metrics_direct_kernel<4, 4>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((metrics_direct_kernel<METRICS_MAX_LEVELS, 1>), grid, block, 0, stream, a);
}

} // namespace anofox
