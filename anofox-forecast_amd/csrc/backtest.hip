// backtest.hip -- the walk-forward backtest of _ts_backtest_native (ts_backtest_native.cpp:623-711, 768-880, 280-373) on a resident
// time-major block.  Fold boundaries are positions, the same for every series, so fold f's training window of series s is rows
// train_start_f .. train_end_f of column s and its test rows are rows test_start_f .. test_end_f: both cuts are strided copies.
//
// Pair p = s * F + f is series s in fold index f (n_pairs = N * F, ld_pairs = n_pairs rounded up to 64).  With this order the
// batch's series-major result [n_pairs x h] IS the series-major block [N x F * h] of one group per series, and the lanes of a wave
// hold the folds of the same few series.
//
//   backtest_expand_kernel      source block -> training block [t_train x ld_pairs], len_pairs, n_test.  One thread per column p and
//                               row tile (stores coalesced, F neighbouring lanes read the same source element).  A pair is live when
//                               train_end < len, test_start < len and train_start <= train_end (the operator's rule, :785-790); every
//                               other cell of the block -- rows past the window, dead pairs, padding columns -- is 0.0 with both counts 0.
//   backtest_collect_kernel     after the batch has run: row i of pair p exists when n_test[p] > 0 (live), status[p] == 0 and
//                               i < min(n_test[p], h).  actual, error = yhat - actual, abs_error; every row that does not exist is NaN
//                               in all three (the row filter of the metrics entry is drop_nan); n_rows[p] counts the existing rows.
//   backtest_fold_score_kernel  ComputeMetric (:280-373) per fold over its existing rows in the operator's row order (series in order,
//                               steps in order), one wavefront per fold.  The contract is equality of bits with
//                               backtest_metrics.backtest_metric: every lane forms the term of one candidate row (one IEEE operation
//                               per step of the formula, nothing fused: -ffp-contract=off), the wave compacts the kept terms of 64
//                               candidates into LDS in row order (ballot + prefix count) and then every lane walks that tile from 0
//                               to k - 1 and carries the SAME running sum -- 64 copies of one serial computation, as quality.hip does
//                               it.  Nothing is reordered: the order is the contract.  The running sum starts from -0.0, the identity
//                               of the addition, so that the first term enters unchanged as in the host's cumulative sum.
#include "kernels.hpp"
#include "det_math.hpp"
#include "wave_sort.hpp"

namespace anofox {

namespace {

constexpr int BT_COLS = 256;                 // columns (threads) per workgroup of the expand kernel
constexpr int BT_ROWS = 16;                  // rows per tile of the expand kernel
constexpr unsigned BT_MAX_GRID_Y = 65535u;
constexpr int BT_R2_MEAN = 100, BT_R2_SUMS = 101;       // the two sweeps of r2

__device__ __forceinline__ int bt_length(const BacktestArgs &a, int s)
{
    int n = a.len[s];
    if (n < 0) n = 0;
    if ((size_t)n > a.t_rows) n = (int)a.t_rows;
    return n;
}

__global__ __launch_bounds__(BT_COLS) void backtest_expand_kernel(const BacktestArgs a)
{
    const size_t p = (size_t)blockIdx.x * BT_COLS + threadIdx.x;
    if (p >= a.ld_pairs) return;
    int L = 0, nt = 0, s = 0, tr0 = 0;
    if (p < (size_t)a.n_pairs) {
        s = (int)(p / (size_t)a.n_folds);
        const BacktestFoldPos q = a.folds[p % (size_t)a.n_folds];
        const int n = bt_length(a, s);
        if (q.train_start >= 0 && q.test_start >= 0 && q.train_end < n && q.test_start < n && q.train_start <= q.train_end) {
            const int last = q.test_end < n - 1 ? q.test_end : n - 1;
            const int rows = last - q.test_start + 1;
            const int w = q.train_end - q.train_start + 1;
            if (rows > 0 && (size_t)w <= a.t_train) { L = w; nt = rows; tr0 = q.train_start; }
        }
    }
    if (blockIdx.y == 0) { a.len_pairs[p] = L; a.n_test[p] = nt; }
    const size_t n_tiles = (a.t_train + BT_ROWS - 1) / BT_ROWS;
    for (size_t tile = blockIdx.y; tile < n_tiles; tile += gridDim.y) {
        const size_t t0 = tile * BT_ROWS, t1 = t0 + BT_ROWS < a.t_train ? t0 + BT_ROWS : a.t_train;
        for (size_t t = t0; t < t1; t++)                     // (tr0 + t <= train_end < len <= t_rows)
            a.y_out[t * a.ld_pairs + p] = t < (size_t)L ? a.y[((size_t)tr0 + t) * a.ld_src + (size_t)s] : 0.0;
    }
}

__global__ __launch_bounds__(256) void backtest_collect_kernel(const BacktestArgs a)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t h = (size_t)a.h;
    if (e >= (size_t)a.n_pairs * h) return;
    const size_t p = e / h;
    const int i = (int)(e % h);
    const size_t s = p / (size_t)a.n_folds;
    const BacktestFoldPos q = a.folds[p % (size_t)a.n_folds];
    const int nt = a.n_test[p];
    int cnt = 0;
    if (nt > 0 && a.status[p] == 0 && q.test_start >= 0 && (size_t)q.test_start < a.t_rows) {
        cnt = nt < a.h ? nt : a.h;
        const size_t room = a.t_rows - (size_t)q.test_start;                 // the block's rows from test_start on
        if ((size_t)cnt > room) cnt = (int)room;
    }
    const bool exists = i < cnt;
    const double nan = __builtin_nan("");
    double act = nan, err = nan, abs_err = nan;
    if (exists) {
        act = a.y[((size_t)q.test_start + (size_t)i) * a.ld_src + s];
        err = a.yhat[e] - act;
        abs_err = fabs(err);
    }
    a.actual[e] = act;
    a.error[e] = err;
    a.abs_error[e] = abs_err;
    if (a.valid) a.valid[e] = exists ? 1 : 0;
    if (i == 0) a.n_rows[p] = cnt;
}

// one sweep over the existing rows of fold f in row order: sum_a (and sum_b, BT_R2_SUMS) over the kept rows, their number, and the
// rows inside [lower, upper] (BT_COVERAGE).  Every lane returns the same figures.
__device__ __forceinline__ void bt_sweep(const BacktestArgs &a, int f, int mode, double mean, double *tile_a, double *tile_b, int lane,
                                         double &sum_a, double &sum_b, long long &kept, long long &hits)
{
    const size_t h = (size_t)a.h, cand = (size_t)a.n_series * h;
    double sa = -0.0, sb = -0.0;
    long long k_all = 0, k_hit = 0;
    for (size_t c0 = 0; c0 < cand; c0 += 64) {
        const size_t c = c0 + (size_t)lane;
        bool keep = false, hit = false;
        double x = 0.0, y = 0.0;
        if (c < cand) {
            const size_t s = c / h;
            const int i = (int)(c % h);
            const size_t p = s * (size_t)a.n_folds + (size_t)f;
            if (i < a.n_rows[p]) {
                const size_t e = p * h + (size_t)i;
                const double av = a.actual[e], fv = a.yhat[e];
                keep = true;
                switch (mode) {
                case BT_MAE: x = fabs(av - fv); break;
                case BT_MAPE: keep = av != 0.0; x = fabs((av - fv) / av); break;
                case BT_SMAPE: { const double d = fabs(av) + fabs(fv); keep = d > 0.0; x = fabs(av - fv) / d; break; }
                case BT_BIAS: x = fv - av; break;
                case BT_R2_MEAN: x = av; break;
                case BT_R2_SUMS: { const double r = av - fv, d = av - mean; x = r * r; y = d * d; break; }
                case BT_COVERAGE: hit = av >= a.lower[e] && av <= a.upper[e]; break;
                default: { const double r = av - fv; x = r * r; break; }          // BT_MSE, BT_RMSE
                }
            }
        }
        const uint64_t mask = __ballot(keep);
        const int k = __popcll(mask);
        k_all += k;
        if (mode == BT_COVERAGE) { k_hit += __popcll(__ballot(hit)); continue; }
        if (k == 0) continue;
        st_sync();                                           // every lane has read the previous tile
        if (keep) {
            const int at = __popcll(mask & ((1ull << lane) - 1ull));
            tile_a[at] = x;
            if (mode == BT_R2_SUMS) tile_b[at] = y;
        }
        st_sync();
#pragma unroll 8
        for (int j = 0; j < k; j++) sa += tile_a[j];
        if (mode == BT_R2_SUMS) {
#pragma unroll 8
            for (int j = 0; j < k; j++) sb += tile_b[j];
        }
    }
    sum_a = sa; sum_b = sb; kept = k_all; hits = k_hit;
}

__global__ __launch_bounds__(64) void backtest_fold_score_kernel(const BacktestArgs a)
{
    __shared__ double tile_a[64], tile_b[64];
    const int lane = threadIdx.x, f = blockIdx.x;
    if (f >= a.n_folds) return;
    const double nan = __builtin_nan("");
    double sum = 0.0, sum_b = 0.0, score = nan;
    long long k = 0, hits = 0;
    const int metric = a.metric;
    if (metric == BT_COVERAGE) {
        if (a.lower && a.upper) {
            bt_sweep(a, f, BT_COVERAGE, 0.0, tile_a, tile_b, lane, sum, sum_b, k, hits);
            if (k > 0) score = (double)hits / (double)k;
        }
    } else if (metric == BT_R2) {
        bt_sweep(a, f, BT_R2_MEAN, 0.0, tile_a, tile_b, lane, sum, sum_b, k, hits);
        if (k > 0) {
            const double mean = sum / (double)k;
            double res = 0.0, tot = 0.0;
            bt_sweep(a, f, BT_R2_SUMS, mean, tile_a, tile_b, lane, res, tot, k, hits);
            if (tot > 0.0) score = 1.0 - res / tot;
        }
    } else {
        bt_sweep(a, f, metric, 0.0, tile_a, tile_b, lane, sum, sum_b, k, hits);
        if (k > 0) {
            const double kf = (double)k;
            switch (metric) {
            case BT_MAPE: score = sum / kf * 100.0; break;
            case BT_SMAPE: score = sum / kf * 200.0; break;
            case BT_MAE: case BT_MSE: case BT_BIAS: score = sum / kf; break;
            default: score = sqrt(sum / kf); break;          // BT_RMSE
            }
        }
    }
    if (lane == 0) a.scores[f] = score;
}

} // namespace

void launch_backtest_expand(const BacktestArgs &a, hipStream_t stream)
{
    if (a.ld_pairs == 0) return;
    const size_t n_tiles = (a.t_train + BT_ROWS - 1) / BT_ROWS;
    const unsigned gy = (unsigned)(n_tiles < 1 ? 1 : n_tiles > BT_MAX_GRID_Y ? BT_MAX_GRID_Y : n_tiles);
    const unsigned gx = (unsigned)((a.ld_pairs + BT_COLS - 1) / BT_COLS);
    hipLaunchKernelGGL(backtest_expand_kernel, dim3(gx, gy), dim3(BT_COLS), 0, stream, a);
}

void launch_backtest_collect(const BacktestArgs &a, hipStream_t stream)
{
    const size_t total = (size_t)a.n_pairs * (size_t)a.h;
    if (total > 0)
        hipLaunchKernelGGL(backtest_collect_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, a);
    if (a.scores && a.n_folds > 0)
        hipLaunchKernelGGL(backtest_fold_score_kernel, dim3((unsigned)a.n_folds), dim3(64), 0, stream, a);
}

} // namespace anofox
