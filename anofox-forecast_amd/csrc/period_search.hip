// period_search.hip -- the two period detectors of the reference that search instead of transforming: ssa_period (periods.rs:800-937)
// and stl_period (:952-1120).  Both are restated op for op: no fused multiply-add (-ffp-contract=off), every sum the source's
// sequential sum from 0.0 in index order, sqrt and / as IEEE.  tests/period_search_ref.py performs the same operations, so the
// contract is equality of bits, on every run, through every entry and on every route.  No atomics.
//
// ssa_period_kernel<BS>: one workgroup of BS lanes per series, the grid walks the batch with a stride (persistent workgroups), so
// the matrix workspace is a fixed number of slices whatever n_series is: at most SSA_WORK_BYTES = 1 GiB (one slice where a single
// matrix is larger: 32 MiB at the window limit of 2,048), never more than 1,024 slices.  At the M5 default (n = 1,913, l = 637,
// 3.25 MB per matrix) that is 330 slices: more than one workgroup for each of the 256 compute units.
//   * The L x L lag-covariance chains are the parallelism of the first phase: a lane owns an element (i <= j) of the upper triangle
//     and adds y[i + t] * y[j + t] for t ascending.  a * b == b * a, so the mirror element has the same bits and is copied.
//   * The matrix is stored with the row index fastest (element (i, j) at M[j * l + i]): in the matvec a lane owns row i and walks j,
//     so the loads of neighbouring lanes are contiguous and v[j] is an LDS broadcast.  After a deflation the matrix is no longer
//     symmetric ((lambda * v_i) * v_j != (lambda * v_j) * v_i), so every element is updated on its own, by the lane of its row.
//   * The three serial reductions of a step (norm, diff, lambda) are carried by every lane redundantly from LDS broadcasts: every
//     lane holds the same sum, so the three breaks are uniform over the workgroup.  They are not reordered.
//   * The LDS pool holds three vectors (v, C v, the normalised C v), the series when it has at most PSEARCH_TILE rows (a longer one
//     is read from global memory), and the matrix when the rest has room for it (host_period_search.hpp ssa_matrix_in_lds: with the
//     default window up to l = 86); otherwise the matrix lives in the workgroup's slice of the workspace.
//   * BS = 64: windows up to SSA_WAVE_WINDOW run with one wavefront per series, the matrix always in LDS.  BS = 256 runs the rest
//     (and every window under SSA_ROUTE_GROUP).  The two instantiate the same code, so they give the same bits.
//
// stl_period_kernel: one workgroup of STL_WAVES waves per series; the candidates are spread over the waves, one candidate at a time
// per wave.  Within a candidate lanes run over rows for the window sums (each a fresh sequential sum, as fit_mstl.hip and the source
// write them), over phases for the per-phase sums (t ascending), and the serial sums (the mean of the periodic component, the
// three means and the three variances -- the source computes Var(remainder) twice, with the same bits) run side by side in lanes.
// Per wave the rows `current` and `trend` and the phase table live in LDS while four of them fit beside the series (n <= 721),
// else in the workgroup's slice of a workspace of at most STL_WORK_BYTES = 256 MiB; the bits are the same.  The candidate list is
// computed per series from its own length; the winner is picked in candidate order with the source's strict >.
//
// Non-finite input does what the source's arithmetic does with it.
#include "kernels.hpp"

#include <cmath>
#include <string>
#include <vector>

#include "host_period_search.hpp"

namespace anofox {

namespace {

static_assert(PSEARCH_HOST_MAX_ROWS == PSEARCH_MAX_ROWS && PSEARCH_HOST_MAX_COMPONENTS == SSA_MAX_COMPONENTS &&
              PSEARCH_HOST_MAX_CANDIDATES == STL_MAX_CANDIDATES && PSEARCH_HOST_MAX_WINDOW == SSA_MAX_WINDOW && PSEARCH_HOST_TILE == PSEARCH_TILE &&
              PSEARCH_HOST_LDS_DOUBLES == PSEARCH_LDS_DOUBLES && PSEARCH_HOST_STL_WAVES == STL_WAVES, "host_period_search.hpp limits");

constexpr double PS_EPS = 2.2204460492503131e-16;      // f64::EPSILON
constexpr int SSA_WAVE_POOL = SSA_WAVE_WINDOW * SSA_WAVE_WINDOW + 3 * SSA_WAVE_WINDOW + PSEARCH_TILE;

__device__ __forceinline__ int ps_length(const int32_t *len, int s, size_t t_rows)
{
    int n = len[s];
    if (n < 0) n = 0;
    if ((size_t)n > t_rows) n = (int)t_rows;
    return n;
}

// ------------------------------------------------------------------------------------------------------------------------------
// SSA (periods.rs:800-937)
// ------------------------------------------------------------------------------------------------------------------------------
template <int BS, int POOL>
__global__ __launch_bounds__(BS) void ssa_period_kernel(const SsaArgs a)
{
    __shared__ double pool[POOL];
    __shared__ double eig[SSA_MAX_COMPONENTS];
    __shared__ double det[SSA_N_DETECTED];
    const int tid = threadIdx.x;
    const double nan = __builtin_nan("");
    for (int s = blockIdx.x; s < a.n_series; s += gridDim.x) {      // (everything that decides a path below is uniform over the workgroup)
        const int n = ps_length(a.len, s, a.t_rows);
        const int64_t l64 = n < 16 ? 4 : ssa_window(n, a.window);
        const bool wave_route = a.route != SSA_ROUTE_GROUP && l64 <= SSA_WAVE_WINDOW;
        if (wave_route != (BS == 64)) continue;                    // the other instantiation's series
        if (n < 16) {
            if (tid == 0) a.status[s] = PSEARCH_TOO_SHORT;
            continue;
        }
        if (l64 > SSA_MAX_WINDOW) {
            if (tid == 0) a.status[s] = PSEARCH_OVER_LIMIT;
            continue;
        }
        const int l = (int)l64;
        const int k = n - l + 1;
        const bool y_lds = n <= PSEARCH_TILE;
        const int vec_end = 3 * l + (y_lds ? n : 0);
        const bool m_lds = l * l + vec_end <= POOL;
        if (!m_lds && (a.work == nullptr || (size_t)l * (size_t)l > a.work_stride || (int)blockIdx.x >= a.work_blocks)) {
            if (tid == 0) a.status[s] = PSEARCH_OVER_LIMIT;        // (the host sizes the workspace for every window it lets through)
            continue;
        }
        double *v = pool, *w = pool + l, *u = pool + 2 * l;
        double *ys = pool + 3 * l;
        double *M = m_lds ? pool + vec_end : a.work + (size_t)blockIdx.x * a.work_stride;
        const double *yg = a.y + s;
        const size_t ld = a.ld;
        if (y_lds) {
            for (int t = tid; t < n; t += BS) ys[t] = yg[(size_t)t * ld];
        }
        __syncthreads();
        // lag covariance C[i][j] = (sum_t y[i + t] y[j + t]) / k, upper triangle; rows r and l - 1 - r together hold l + 1 elements
        {
            const int half = (l + 1) / 2, width = l + 1;
            const double kd = (double)k;
            for (int idx = tid; idx < half * width; idx += BS) {
                const int r = idx / width, c = idx - r * width;
                int i, j;
                if (c < l - r) { i = r; j = r + c; }
                else {
                    i = l - 1 - r; j = i + (c - (l - r));
                    if (i == r) continue;                          // the middle row of an odd window is complete already
                }
                double sum = 0.0;
                if (y_lds) {
                    for (int t = 0; t < k; t++) sum += ys[i + t] * ys[j + t];
                } else {
                    for (int t = 0; t < k; t++) sum += yg[(size_t)(i + t) * ld] * yg[(size_t)(j + t) * ld];
                }
                const double cv = sum / kd;
                M[(size_t)j * l + i] = cv;
                M[(size_t)i * l + j] = cv;
            }
        }
        __syncthreads();
        const int n_comp = a.n_components < l ? a.n_components : l;
        int n_eig = 0, n_det = 0;
        for (int c = 0; c < n_comp; c++) {
            for (int i = tid; i < l; i += BS) u[i] = 1.0 / (double)(i + 1);
            __syncthreads();
            double acc = 0.0;
            for (int i = 0; i < l; i++) acc += u[i] * u[i];
            const double v_norm = sqrt(acc);
            for (int i = tid; i < l; i += BS) v[i] = u[i] / v_norm;
            __syncthreads();
            for (int it = 0; it < 100; it++) {
                for (int i = tid; i < l; i += BS) {
                    double r = 0.0;
                    const double *col = M + i;
#pragma unroll 8                                                   // (the loads of several steps in flight; the additions keep their order)
                    for (int j = 0; j < l; j++) r += col[(size_t)j * l] * v[j];
                    w[i] = r;
                }
                __syncthreads();
                double nn = 0.0;
                for (int i = 0; i < l; i++) nn += w[i] * w[i];
                const double norm = sqrt(nn);
                if (norm < PS_EPS) break;
                for (int i = tid; i < l; i += BS) u[i] = w[i] / norm;
                __syncthreads();
                double diff = 0.0;
                for (int i = 0; i < l; i++) diff += fabs(v[i] - u[i]);
                double *tmp = v; v = u; u = tmp;                   // v = v_new
                if (diff < 1e-10) break;
            }
            // (every lane has left the loop with the same v; w and u are free, M's element (i, j) is only ever touched by row i's lane)
            __syncthreads();
            for (int i = tid; i < l; i += BS) {
                double r = 0.0;
                const double *col = M + i;
#pragma unroll 8
                for (int j = 0; j < l; j++) r += col[(size_t)j * l] * v[j];
                w[i] = r;
            }
            __syncthreads();
            double lambda = 0.0;
            for (int i = 0; i < l; i++) lambda += v[i] * w[i];
            if (fabs(lambda) < PS_EPS) break;
            if (tid == 0) eig[n_eig] = lambda;
            n_eig++;
            if (c < SSA_N_DETECTED) {
                int crossings = 0;
                double prev = v[0];
                for (int i = 1; i < l; i++) {
                    const double cur = v[i];
                    if ((prev >= 0.0 && cur < 0.0) || (prev < 0.0 && cur >= 0.0)) crossings++;
                    prev = cur;
                }
                if (crossings > 0) {
                    const double period = 2.0 * (double)l / (double)crossings;
                    if (period > 2.0 && period < (double)n / 2.0) {
                        if (tid == 0) det[n_det] = period;
                        n_det++;
                    }
                }
            }
            for (int i = tid; i < l; i += BS) {
                const double lv = lambda * v[i];
                double *col = M + i;
#pragma unroll 8
                for (int j = 0; j < l; j++) col[(size_t)j * l] -= lv * v[j];
            }
            __syncthreads();                                       // v has been read before the next component overwrites it
        }
        if (tid == 0) {
            double total = 0.0;
            for (int c = 0; c < n_eig; c++) total += eig[c];
            double ve = 0.0;
            if (n_eig > 0 && total > 0.0) {
                double two = 0.0;
                for (int c = 0; c < n_eig && c < 2; c++) two += eig[c];
                ve = two / total;
            }
            a.out_fp[0 * ld + s] = n_det > 0 ? det[0] : nan;
            a.out_fp[1 * ld + s] = ve;
            a.out_fp[2 * ld + s] = (double)n_eig;
            if (a.out_eig)
                for (int c = 0; c < a.n_components; c++) a.out_eig[(size_t)c * ld + s] = c < n_eig ? eig[c] : nan;
            if (a.out_det)
                for (int c = 0; c < SSA_N_DETECTED; c++) a.out_det[(size_t)c * ld + s] = c < n_det ? det[c] : nan;
            a.status[s] = PSEARCH_OK;
        }
        __syncthreads();                                           // the pool, eig and det have been read before the next series
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// STL (periods.rs:952-1120; the decomposition is decomposition.rs mstl_decompose with one period, as fit_mstl.hip restates it)
// ------------------------------------------------------------------------------------------------------------------------------
constexpr int STL_BLOCK = STL_WAVES * 64;

__global__ __launch_bounds__(STL_BLOCK) void stl_period_kernel(const StlPeriodArgs a)
{
    __shared__ double pool[PSEARCH_LDS_DOUBLES];
    __shared__ double s_strength[STL_MAX_CANDIDATES], t_strength[STL_MAX_CANDIDATES];
    __shared__ int cand[STL_MAX_CANDIDATES];
    __shared__ int list_info[2];                                   // the number of candidates, the status
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const double nan = __builtin_nan("");
    const size_t ld = a.ld;
    for (int s = blockIdx.x; s < a.n_series; s += gridDim.x) {      // (uniform over the workgroup)
        const int n = ps_length(a.len, s, a.t_rows);
        if (n < 16) {
            if (tid == 0) a.status[s] = PSEARCH_TOO_SHORT;
            continue;
        }
        if (tid == 0) {                                            // the candidate list (host_period_search.hpp stl_candidates)
            int64_t min_p = a.min_period > 0 ? a.min_period : 4;
            if (min_p < 2) min_p = 2;
            int64_t max_p = a.max_period > 0 ? a.max_period : n / 3;
            if (max_p > n / 2) max_p = n / 2;
            int count = 0, st = PSEARCH_OK;
            if (min_p >= max_p) st = PSEARCH_STL_RANGE;
            else {
                double step = (double)(max_p - min_p) / (double)a.n_cand;
                if (!(step >= 1.0)) step = 1.0;
                int64_t last = -1;
                for (int i = 0; i < a.n_cand; i++) {
                    const double x = (double)min_p + (double)i * step;
                    const double f = floor(x);
                    const int64_t p = (int64_t)f + (x - f >= 0.5 ? 1 : 0);
                    if (p >= min_p && p <= max_p && p >= 2 && (int64_t)n >= 2 * p && p != last) {
                        cand[count++] = (int)p;
                        last = p;
                    }
                }
                if (count == 0) st = PSEARCH_STL_NO_CANDIDATE;
            }
            list_info[0] = count;
            list_info[1] = st;
        }
        __syncthreads();
        const int n_list = list_info[0], list_status = list_info[1];
        const bool y_lds = n <= PSEARCH_TILE;
        const int wave_doubles = 2 * n + n / 2;
        const bool rows_lds = STL_WAVES * wave_doubles + (y_lds ? n : 0) <= PSEARCH_LDS_DOUBLES;
        const bool no_room = !rows_lds && (a.work == nullptr || (size_t)STL_WAVES * (size_t)wave_doubles > a.work_stride || (int)blockIdx.x >= a.work_blocks);
        if (list_status != PSEARCH_OK || no_room) {
            if (tid == 0) a.status[s] = list_status != PSEARCH_OK ? list_status : PSEARCH_OVER_LIMIT;
            __syncthreads();                                       // list_info has been read
            continue;
        }
        const double *yg = a.y + s;
        double *ys = pool;
        double *rows = rows_lds ? pool + (y_lds ? n : 0) : a.work + (size_t)blockIdx.x * a.work_stride;
        double *A = rows + (size_t)wave * wave_doubles, *B = A + n, *P = B + n;
        if (y_lds) {
            for (int t = tid; t < n; t += STL_BLOCK) ys[t] = yg[(size_t)t * ld];
        }
        __syncthreads();
        const double nd = (double)n;
        double acc = 0.0;
        if (y_lds) { for (int t = 0; t < n; t++) acc += ys[t]; }
        else { for (int t = 0; t < n; t++) acc += yg[(size_t)t * ld]; }
        const double mean = acc / nd;
        acc = 0.0;
        if (y_lds) { for (int t = 0; t < n; t++) { const double d = ys[t] - mean; acc += d * d; } }
        else { for (int t = 0; t < n; t++) { const double d = yg[(size_t)t * ld] - mean; acc += d * d; } }
        const double total_var = acc / nd;
        if (total_var < PS_EPS) {                                  // a constant series: no seasonality
            if (tid == 0) {
                a.out_fp[0 * ld + s] = nan;
                a.out_fp[1 * ld + s] = 0.0;
                a.out_fp[2 * ld + s] = 0.0;
                a.out_index[s] = -1;
                for (int c = 0; c < a.n_cand; c++) {
                    if (a.out_cand) a.out_cand[(size_t)c * ld + s] = c < n_list ? cand[c] : -1;
                    if (a.out_strength) a.out_strength[(size_t)c * ld + s] = c < n_list ? 0.0 : nan;
                }
                a.status[s] = PSEARCH_OK;
            }
            __syncthreads();
            continue;
        }
        int w2 = n / 5 > 3 ? n / 5 : 3;                            // the final trend's window: max(n / 5, 3).min(n)
        if (w2 > n) w2 = n;
        const int hw2 = w2 / 2;
        const double w2d = (double)(2 * hw2 + 1);                  // the source divides by (end - start)
        for (int c0 = 0; c0 < n_list; c0 += STL_WAVES) {
            const int ci = c0 + wave;
            const bool active = ci < n_list;                       // (uniform over the wave; every wave meets every barrier)
            const int p = active ? cand[ci] : 2;
            const int w1 = (p % 2 == 0) ? p + 1 : p;
            const int hw = w1 / 2;
            const double w1d = (double)w1;
            // stl_decompose: the centred moving average (edges held), the detrended series
            if (active) {
                for (int t = lane; t < n; t += 64) {
                    const int c = t < hw ? hw : (t > n - hw - 1 ? n - hw - 1 : t);
                    double sum = 0.0;
                    double yt;
                    if (y_lds) { for (int j = c - hw; j <= c + hw; j++) sum += ys[j]; yt = ys[t]; }
                    else { for (int j = c - hw; j <= c + hw; j++) sum += yg[(size_t)j * ld]; yt = yg[(size_t)t * ld]; }
                    A[t] = yt - sum / w1d;
                }
            }
            __syncthreads();
            // the phase means, each phase in increasing t
            if (active) {
                for (int q = lane; q < p; q += 64) {
                    double sum = 0.0;
                    int count = 0;
                    for (int t = q; t < n; t += p) { sum += A[t]; count++; }
                    P[q] = sum / (double)count;
                }
            }
            __syncthreads();
            // the mean of the periodic component (serial, every lane the same sum), then current = y - seasonal
            double smean = 0.0;
            if (active) {
                double m = 0.0;
                int ph = 0;
                for (int t = 0; t < n; t++) {
                    m += P[ph];
                    ph = ph + 1 == p ? 0 : ph + 1;
                }
                smean = m / nd;
                for (int t = lane; t < n; t += 64) {
                    const double yt = y_lds ? ys[t] : yg[(size_t)t * ld];
                    A[t] = yt - (P[t % p] - smean);
                }
            }
            __syncthreads();
            // mstl_decompose's final trend over the deseasonalised series
            if (active) {
                for (int t = lane; t < n; t += 64) {
                    const int c = t < hw2 ? hw2 : (t > n - hw2 - 1 ? n - hw2 - 1 : t);
                    double sum = 0.0;
                    for (int j = c - hw2; j <= c + hw2; j++) sum += A[j];
                    B[t] = sum / w2d;
                }
            }
            __syncthreads();
            // lane 0: seasonal + remainder, lane 1: remainder, lane 2 (and the rest): trend + remainder -- mean, then variance
            if (active) {
                double sum = 0.0;
                int ph = 0;
                for (int t = 0; t < n; t++) {
                    const double sv = P[ph] - smean, tr = B[t];
                    const double r = A[t] - tr;
                    sum += lane == 0 ? sv + r : (lane == 1 ? r : tr + r);
                    ph = ph + 1 == p ? 0 : ph + 1;
                }
                const double fm = sum / nd;
                double sq = 0.0;
                ph = 0;
                for (int t = 0; t < n; t++) {
                    const double sv = P[ph] - smean, tr = B[t];
                    const double r = A[t] - tr;
                    const double d = (lane == 0 ? sv + r : (lane == 1 ? r : tr + r)) - fm;
                    sq += d * d;
                    ph = ph + 1 == p ? 0 : ph + 1;
                }
                const double var = sq / nd;
                const double var_detrended = __shfl(var, 0), var_remainder = __shfl(var, 1), var_with_trend = __shfl(var, 2);
                if (lane == 0) {
                    s_strength[ci] = var_detrended > PS_EPS ? fmax(1.0 - var_remainder / var_detrended, 0.0) : 0.0;
                    t_strength[ci] = var_with_trend > PS_EPS ? fmax(1.0 - var_remainder / var_with_trend, 0.0) : 0.0;
                }
            }
            __syncthreads();                                       // the strengths are written; the rows may be reused
        }
        if (tid == 0) {
            int best = 0;
            double best_s = 0.0, best_t = 0.0;
            for (int c = 0; c < n_list; c++)
                if (s_strength[c] > best_s) { best_s = s_strength[c]; best_t = t_strength[c]; best = c; }
            a.out_fp[0 * ld + s] = (double)cand[best];
            a.out_fp[1 * ld + s] = best_s;
            a.out_fp[2 * ld + s] = best_t;
            a.out_index[s] = best;
            for (int c = 0; c < a.n_cand; c++) {
                if (a.out_cand) a.out_cand[(size_t)c * ld + s] = c < n_list ? cand[c] : -1;
                if (a.out_strength) a.out_strength[(size_t)c * ld + s] = c < n_list ? s_strength[c] : nan;
            }
            a.status[s] = PSEARCH_OK;
        }
        __syncthreads();                                           // cand, the strengths and the pool have been read
    }
}

} // namespace

size_t ssa_work_stride(size_t t_rows, int64_t window)
{
    int64_t l = ssa_window((int64_t)t_rows, window);               // the largest window a series of the call can have
    if (l > SSA_MAX_WINDOW) l = SSA_MAX_WINDOW;
    return l <= SSA_WAVE_WINDOW ? 0 : (size_t)l * (size_t)l;       // (up to SSA_WAVE_WINDOW the matrix fits in LDS on both routes)
}

int ssa_work_blocks(size_t work_stride, int n_series)
{
    if (!work_stride) return 0;
    size_t blocks = SSA_WORK_BYTES / (work_stride * sizeof(double));
    if (blocks < 1) blocks = 1;
    if (blocks > 1024) blocks = 1024;
    if (blocks > (size_t)n_series) blocks = (size_t)n_series;
    return (int)blocks;
}

void launch_ssa_period(const SsaArgs &a, hipStream_t stream)
{
    if (a.n_series <= 0) return;
    if (a.route != SSA_ROUTE_GROUP) {
        const int blocks = a.n_series < 4096 ? a.n_series : 4096;
        hipLaunchKernelGGL((ssa_period_kernel<64, SSA_WAVE_POOL>), dim3(blocks), dim3(64), 0, stream, a);
    }
    if (a.route == SSA_ROUTE_GROUP || ssa_window((int64_t)a.t_rows, a.window) > SSA_WAVE_WINDOW) {
        int blocks = a.n_series < 2048 ? a.n_series : 2048;
        if (a.work_blocks > 0 && blocks > a.work_blocks) blocks = a.work_blocks;
        hipLaunchKernelGGL((ssa_period_kernel<256, PSEARCH_LDS_DOUBLES>), dim3(blocks), dim3(256), 0, stream, a);
    }
}

size_t stl_period_work_stride(size_t t_rows)
{
    return stl_rows_in_lds((int64_t)t_rows) ? 0 : (size_t)STL_WAVES * (size_t)stl_wave_doubles((int64_t)t_rows);
}

int stl_period_work_blocks(size_t work_stride, int n_series)
{
    if (!work_stride) return 0;
    size_t blocks = STL_WORK_BYTES / (work_stride * sizeof(double));
    if (blocks < 1) blocks = 1;
    if (blocks > 2048) blocks = 2048;
    if (blocks > (size_t)n_series) blocks = (size_t)n_series;
    return (int)blocks;
}

void launch_stl_period(const StlPeriodArgs &a, hipStream_t stream)
{
    if (a.n_series <= 0) return;
    int blocks = a.n_series < 2048 ? a.n_series : 2048;
    if (a.work_blocks > 0 && blocks > a.work_blocks) blocks = a.work_blocks;
    hipLaunchKernelGGL(stl_period_kernel, dim3(blocks), dim3(STL_BLOCK), 0, stream, a);
}

} // namespace anofox
