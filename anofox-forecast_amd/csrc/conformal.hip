// conformal.hip -- split / cross-validation / Jackknife+ conformal prediction intervals of the reference (conformal.rs conformal_learn,
// conformal_apply, conformal_coverage, winkler_score, conformal_evaluate) for every group of a block, in three kernels.
//
// The contract is equality of bits with the source: every figure of conformal.rs is a function of a SORTED residual vector, the
// quantile level ceil((n + 1)(1 - alpha)) / n and the two-point interpolation are single IEEE operations (-ffp-contract=off, no
// fused multiply-add anywhere), and every sum is the sequential one from 0.0 in row order.
//
// Element (group s, row t) of every block is at s * stride_s + t * stride_t: stride_s = 1 is the project's time-major block,
// stride_t = 1 the series-major [n_series x horizon] layout of the forecast results.  The arithmetic does not depend on the layout.
//
//   learn     one wavefront per group.  The residual of a row is the supplied value or actual - forecast; a row whose validity
//             byte is 0 is dropped.  The kept values become keys of the total order of wave_sort.hpp and are compacted into the
//             wave's buffer in arrival order (ballot + prefix count), padded with the largest key and sorted by the bitonic network.
//             Symmetric / adaptive: keys of |r|; lane k < n_alphas then reads the two neighbours of its level.  Asymmetric: ONE sort
//             of the signed keys -- the tail of the buffer is the sorted positives, the head read backwards the sorted magnitudes of
//             the negatives; zeros of either sign lie between and belong to neither.  When the sorted |r| are wanted as well
//             (Jackknife+'s state vector), the asymmetric method sorts twice.
//             The buffer is `tile` words of dynamic LDS per wave (conformal_kernel; the host sizes the tile from the batch's longest
//             group, a power of two of at most CONFORMAL_RESIDENT = 2,048 keys, and fits 64 KiB / tile bytes waves -- at most 16 --
//             into a workgroup) or a slice of a global workspace (conformal_long_kernel, groups above 2,048 rows; a fixed number of
//             waves walks them).  The body is the same.
//   apply     one lane per (group, step): lower = f - score_lower[k] * d, upper = f + score_upper[k] * d for every level k, d = 1
//             unless the method is adaptive; then d = difficulty / mean, the mean from the group's sequential sum, which every lane
//             of the group forms for itself by the same serial loop (no butterfly).  A difficulty <= 0 gives NaN and a status.
//   evaluate  one lane per group walks its rows in order with running values in registers.
//
// Status per group: CONFORMAL_OK; CONFORMAL_EMPTY no row (left), figures NaN; CONFORMAL_NAN a residual is NaN -- the source's
// sort_by(partial_cmp().unwrap_or(Equal)) leaves the order of such a vector to its sort's internals, so the scores are NaN here
// (DESIGN.md section 7); CONFORMAL_DIFFICULTY a difficulty <= 0.  +-inf are ordinary values.
#include "kernels.hpp"
#include "det_math.hpp"
#include "wave_sort.hpp"

namespace anofox {

namespace {

constexpr int CF_MAX_WAVES = 16;
constexpr int CF_LONG_WAVES = 4;
constexpr size_t CF_LDS_BYTES = 64 * 1024;               // dynamic LDS a workgroup may ask for without raising the limit
constexpr int CF_BLOCK = 64;                              // apply / evaluate

__device__ __forceinline__ int cf_length(const int32_t *len, int s, size_t t_rows)
{
    int n = len[s];
    if (n < 0) n = 0;
    if ((size_t)n > t_rows) n = (int)t_rows;
    return n;
}

// compute_quantile(sorted, clamp(ceil((n + 1)(1 - alpha)) / n, 0, 1)) (conformal.rs:137-144, 429-449); element i of the sorted
// vector is get(i), n > 0
template <class G>
__device__ __forceinline__ double cf_score(G get, int n, double alpha)
{
    const double nf = (double)n;
    double q = ceil((nf + 1.0) * (1.0 - alpha)) / nf;
    q = q < 0.0 ? 0.0 : q;
    q = q > 1.0 ? 1.0 : q;
    if (q <= 0.0) return get(0);
    if (q >= 1.0) return get(n - 1);
    const double index = q * (double)(n - 1);
    int lo = (int)floor(index);
    lo = lo < 0 ? 0 : (lo > n - 1 ? n - 1 : lo);          // (in range for 0 < q < 1; the clamp keeps a read inside the buffer whatever happens)
    const int up = lo + 1 < n - 1 ? lo + 1 : n - 1;
    const double frac = index - (double)lo;
    return get(lo) * (1.0 - frac) + get(up) * frac;
}

// load group s, drop the masked rows, compact the keys of |r| (magnitude) or r (signed) into buf.  Returns the rows kept; counts the
// positives and negatives and notes a NaN.
template <class B>
__device__ __forceinline__ int cf_load(const ConformalLearnArgs &a, int s, int n, B buf, int lane, bool magnitude, int &n_pos, int &n_neg,
                                       bool &has_nan)
{
    const size_t base = (size_t)s * a.stride_s;
    int m = 0;
    n_pos = 0; n_neg = 0; has_nan = false;
    for (int t0 = 0; t0 < n; t0 += 64) {
        const int tl = t0 + lane;
        const bool in = tl < n;
        const size_t off = base + (size_t)tl * a.stride_t;
        double r = 0.0;
        if (in) r = a.residual ? a.residual[off] : a.actual[off] - a.forecast[off];
        const bool keep = in && (!a.valid || a.valid[off] != 0);
        const uint64_t mask = __ballot(keep);
        if (__ballot(keep && r != r)) has_nan = true;
        n_pos += __popcll(__ballot(keep && r > 0.0));
        n_neg += __popcll(__ballot(keep && r < 0.0));
        if (keep) buf[m + __popcll(mask & ((1ull << lane) - 1ull))] = st_key(dm_bits(magnitude ? fabs(r) : r));
        m += __popcll(mask);
    }
    return m;
}

template <class B>
__device__ __forceinline__ void cf_pad_sort(B buf, int m, int lane)
{
    int p2 = 1;
    while (p2 < m) p2 <<= 1;
    for (int i = m + lane; i < p2; i += 64) buf[i] = ~0ull;
    st_sync();
    st_sort(buf, p2, lane);
}

// all outputs of group s (n rows, n <= capacity of buf)
template <class B>
__device__ __forceinline__ void cf_group(const ConformalLearnArgs &a, int s, int n, B buf, int lane)
{
    const double nan = __builtin_nan("");
    // lane k's level, picked by constant indices (the argument block stays in scalar registers)
    double alpha = 0.0;
#pragma unroll
    for (int k = 0; k < CONFORMAL_MAX_LEVELS; k++) alpha = lane == k ? a.alphas[k] : alpha;
    const bool mine = lane < a.n_alphas;
    const bool asym = a.method == CONFORMAL_ASYMMETRIC;

    int n_pos, n_neg;
    bool has_nan;
    int m = cf_load(a, s, n, buf, lane, !asym || a.sorted != nullptr, n_pos, n_neg, has_nan);
    const int32_t status = m == 0 ? CONFORMAL_EMPTY : has_nan ? CONFORMAL_NAN : CONFORMAL_OK;
    if (lane == 0) {
        a.status[s] = status;
        if (a.n_kept) a.n_kept[s] = m;
    }
    double lo = nan, up = nan;
    if (status == CONFORMAL_OK) {                            // (wave-uniform)
        if (!asym || a.sorted) {
            cf_pad_sort(buf, m, lane);
            if (a.sorted) {
                const size_t base = (size_t)s * a.stride_s;
                for (int i = lane; i < m; i += 64) a.sorted[base + (size_t)i * a.stride_t] = st_unkey(buf[i]);
            }
            if (!asym && mine) lo = up = cf_score([&](int i) { return st_unkey(buf[i]); }, m, alpha);
        }
        if (asym) {
            if (a.sorted) {
                st_sync();                                   // the magnitudes have been read
                m = cf_load(a, s, n, buf, lane, false, n_pos, n_neg, has_nan);
            }
            cf_pad_sort(buf, m, lane);
            if (mine) {
                const double half = alpha / 2.0;
                const int p0 = m - n_pos, q0 = n_neg - 1;
                up = n_pos == 0 ? 0.0 : cf_score([&](int i) { return st_unkey(buf[p0 + i]); }, n_pos, half);
                lo = n_neg == 0 ? 0.0 : cf_score([&](int i) { return fabs(st_unkey(buf[q0 - i])); }, n_neg, half);
            }
        }
    }
    if (mine) {
        a.scores_lower[(size_t)lane * a.ld + s] = lo;
        a.scores_upper[(size_t)lane * a.ld + s] = up;
    }
}

// groups of at most `tile` rows, the buffer in LDS: blockDim.x / 64 waves, a.tile words each
__global__ __launch_bounds__(64 * CF_MAX_WAVES) void conformal_kernel(const ConformalLearnArgs a)
{
    extern __shared__ uint64_t cf_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = blockIdx.x * (int)(blockDim.x >> 6) + wave;
    if (s >= a.n_groups) return;                             // (wave-uniform; the kernel has no workgroup barrier)
    const int n = cf_length(a.len, s, a.t_rows);
    if (n > a.tile) return;                                  // conformal_long_kernel answers it
    cf_group(a, s, n, cf_lds + (size_t)wave * a.tile, lane);
}

// longer groups, the buffer in the global workspace: a.work_waves waves walk them
__global__ __launch_bounds__(64 * CF_LONG_WAVES) void conformal_long_kernel(const ConformalLearnArgs a)
{
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * CF_LONG_WAVES + (threadIdx.x >> 6);
    if (w >= a.work_waves) return;
    uint64_t *buf = a.work + (size_t)w * a.work_stride;
    for (int s = w; s < a.n_groups; s += a.work_waves) {
        const int n = cf_length(a.len, s, a.t_rows);
        if (n <= a.tile || (size_t)n > a.work_stride) continue;
        cf_group(a, s, n, buf, lane);
        st_sync();
    }
}

// one lane per (group, step); SM: the steps of a group are neighbours (stride_t == 1), else the groups of a step are
template <bool SM>
__global__ __launch_bounds__(CF_BLOCK) void conformal_apply_kernel(const ConformalApplyArgs a)
{
    const size_t i = (size_t)blockIdx.x * CF_BLOCK + threadIdx.x;
    if (i >= (size_t)a.n_groups * (size_t)a.h_rows) return;
    const int s = SM ? (int)(i / (size_t)a.h_rows) : (int)(i % (size_t)a.n_groups);
    const int t = SM ? (int)(i % (size_t)a.h_rows) : (int)(i / (size_t)a.n_groups);
    int h = a.len ? a.len[s] : a.h_rows;
    h = h < 0 ? 0 : (h > a.h_rows ? a.h_rows : h);
    const size_t base = (size_t)s * a.stride_s;
    const double nan = __builtin_nan("");
    int32_t status = h == 0 ? CONFORMAL_EMPTY : CONFORMAL_OK;
    double d = 1.0;
    const bool adaptive = a.method == CONFORMAL_ADAPTIVE;
    if (adaptive && h > 0) {
        double sum = 0.0;                                    // difficulty.iter().sum() (conformal.rs:934), and any(|x| x <= 0.0)
        bool bad = false;
        for (int j = 0; j < h; j++) {
            const double x = a.difficulty[base + (size_t)j * a.stride_t];
            bad = bad || x <= 0.0;
            sum += x;
        }
        if (bad) status = CONFORMAL_DIFFICULTY;
        else if (t < h) d = a.difficulty[base + (size_t)t * a.stride_t] / (sum / (double)h);
    }
    if (t == 0) a.status[s] = status;
    if (t >= h) return;
    const size_t off = base + (size_t)t * a.stride_t;
    const double f = a.forecast[off];
    for (int k = 0; k < a.n_alphas; k++) {
        const double sl = a.scores_lower[(size_t)k * a.ld + s], su = a.scores_upper[(size_t)k * a.ld + s];
        const bool ok = status == CONFORMAL_OK;
        a.lower[(size_t)k * a.stride_q + off] = !ok ? nan : adaptive ? f - sl * d : f - sl;
        a.upper[(size_t)k * a.stride_q + off] = !ok ? nan : adaptive ? f + su * d : f + su;
    }
}

// one lane per group (conformal.rs:1083-1090 coverage, 459-465 mean width, 1130-1146 Winkler)
__global__ __launch_bounds__(CF_BLOCK) void conformal_evaluate_kernel(const ConformalEvalArgs a)
{
    const int s = blockIdx.x * CF_BLOCK + threadIdx.x;
    if (s >= a.n_groups) return;
    const int n = cf_length(a.len, s, a.t_rows);
    const size_t base = (size_t)s * a.stride_s;
    const double penalty = 2.0 / a.alpha;
    int covered = 0;
    double width_sum = 0.0, total = 0.0;
    for (int t = 0; t < n; t++) {
        const size_t off = base + (size_t)t * a.stride_t;
        const double y = a.actual[off], l = a.lower[off], u = a.upper[off];
        if (y >= l && y <= u) covered++;
        const double width = u - l;
        width_sum += width;
        double score = width;
        if (y < l) score += penalty * (l - y);
        else if (y > u) score += penalty * (y - u);
        total += score;
    }
    const double nan = __builtin_nan("");
    const double nf = (double)n;
    const double coverage = n > 0 ? (double)covered / nf : nan;
    a.figures[0 * a.ld + s] = coverage;
    a.figures[1 * a.ld + s] = n > 0 ? 1.0 - coverage : nan;
    a.figures[2 * a.ld + s] = n > 0 ? width_sum / nf : nan;
    a.figures[3 * a.ld + s] = n > 0 ? total / nf : nan;
    a.figures[4 * a.ld + s] = nf;
    a.status[s] = n > 0 ? CONFORMAL_OK : CONFORMAL_EMPTY;
}

} // namespace

int conformal_tile(size_t t_rows)
{
    int tile = 64;
    while (tile < CONFORMAL_RESIDENT && (size_t)tile < t_rows) tile <<= 1;
    return tile;
}

size_t conformal_work_stride(size_t t_rows)
{
    if (t_rows <= (size_t)CONFORMAL_RESIDENT) return 0;
    size_t p2 = 1;
    while (p2 < t_rows) p2 <<= 1;
    return p2;
}

int conformal_work_waves(int n_groups)
{
    return n_groups < CONFORMAL_WORK_WAVES ? n_groups : CONFORMAL_WORK_WAVES;
}

void launch_conformal_learn(const ConformalLearnArgs &a, hipStream_t stream)
{
    if (a.n_groups <= 0) return;
    int waves = (int)(CF_LDS_BYTES / ((size_t)a.tile * sizeof(uint64_t)));
    waves = waves > CF_MAX_WAVES ? CF_MAX_WAVES : waves;
    const size_t lds = (size_t)waves * a.tile * sizeof(uint64_t);
    const int blocks = (a.n_groups + waves - 1) / waves;
    hipLaunchKernelGGL(conformal_kernel, dim3(blocks), dim3(64 * waves), lds, stream, a);
    if (a.t_rows > (size_t)CONFORMAL_RESIDENT && a.work && a.work_waves > 0) {
        const int lblocks = (a.work_waves + CF_LONG_WAVES - 1) / CF_LONG_WAVES;
        hipLaunchKernelGGL(conformal_long_kernel, dim3(lblocks), dim3(64 * CF_LONG_WAVES), 0, stream, a);
    }
}

void launch_conformal_apply(const ConformalApplyArgs &a, hipStream_t stream)
{
    if (a.n_groups <= 0 || a.h_rows <= 0) return;
    const size_t cells = (size_t)a.n_groups * (size_t)a.h_rows;
    const dim3 grid((unsigned)((cells + CF_BLOCK - 1) / CF_BLOCK)), block(CF_BLOCK);
    if (a.stride_t == 1 && a.stride_s != 1) hipLaunchKernelGGL(conformal_apply_kernel<true>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(conformal_apply_kernel<false>, grid, block, 0, stream, a);
}

void launch_conformal_evaluate(const ConformalEvalArgs &a, hipStream_t stream)
{
    if (a.n_groups <= 0) return;
    hipLaunchKernelGGL(conformal_evaluate_kernel, dim3((unsigned)((a.n_groups + CF_BLOCK - 1) / CF_BLOCK)), dim3(CF_BLOCK), 0, stream, a);
}

} // namespace anofox
