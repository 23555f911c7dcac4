// select.hip -- choose the forecast method per series from backtest scores (DESIGN.md section 3 "Selection"): the winner of every
// series, the stable partition of the series by winner, the gather of a winner's columns into a dense block, the scatter of the
// sub-batch's results back to series order, and the combination of the methods' forecasts.  The reference has no such operator; the
// contract is equality of bits with the serial restatement tests/select_ref.py.  Nothing here adds floating-point numbers except the
// combine sums, whose order is the method order (-ffp-contract=off: a product and the addition that takes it stay two operations).
// No floating-point atomics, and no atomic decides an order anywhere.
//
//   select_winner_kernel      one thread per series, 256 per workgroup.  Method m is admissible when status[m * N + s] == 0 and its
//                             score is not NaN; the winner is the admissible method with the smallest score, the lowest m among
//                             equals (x < y is false for -0.0 against +0.0: a tie), `fallback` when none is admissible.  The same
//                             workgroup counts its winners per method (ballot + popcount per wave, the waves' counts added in LDS) and
//                             writes them to counts[m * n_wg + wg]: the exclusive scan of that array in ITS order is, for (m, wg),
//                             the place of the workgroup's first series in `members`.
//   select_scan_*_kernel      the exclusive scan of int32 counts of any length: chunks of 1,024 (256 threads x 4), the chunk sums scanned
//                             by the same two kernels one level up (select_scan below: 1,024^3 covers every N), then added on the
//                             way down.  Integer sums: the grouping cannot change a bit.
//   select_partition_kernel   the scatter: series s goes to members[scan[m * n_wg + wg] + rank], rank = the series of the workgroup
//                             before it with the same winner (the waves before it from LDS, the lanes before it from the ballot), so
//                             every method's list ascends.  offsets[m] = scan[m * n_wg], offsets[M] = the total.
//   select_gather_kernel      y_m[t * ld_m + j] = y[t * ld_src + members[off + j]]: a thread per output column and row tile as in
//                             backtest_expand_kernel (stores coalesced, the loads of one row stay inside that row); columns from n_m
//                             on are 0.0 with length 0.
//   select_scatter_kernel     the inverse for results: cell (j, i) of a series-major [n_m x h] block goes to row members[off + j].
//   select_unchosen_kernel    rows of the series nobody won (winner -1): NaN, model code 0, status INSUFFICIENT_DATA.
//   combine_kernel            one thread per cell of the [R x h] blocks; at most 16 members, whose values live in registers.  The median
//                             sorts total-order keys (wave_sort.hpp's st_key) with a 16-wide bitonic network unrolled over registers.
//   combine_row_status_kernel row r: 1 when every cell of the row is NaN, else 0.
#include "kernels.hpp"
#include "det_math.hpp"
#include "wave_sort.hpp"

namespace anofox {

namespace {

constexpr int SEL_WG = 256;                  // series per workgroup of the winner and partition kernels
constexpr int SEL_WAVES = SEL_WG / 64;
constexpr int SEL_SCAN_PER_THREAD = 4;
constexpr int SEL_SCAN_CHUNK = SEL_WG * SEL_SCAN_PER_THREAD;
constexpr int SEL_COLS = 256;                // columns (threads) per workgroup of the gather kernel
constexpr int SEL_ROWS = 16;                 // rows per tile of the gather kernel
constexpr unsigned SEL_MAX_GRID_Y = 65535u;
constexpr int32_t SEL_STATUS_UNCHOSEN = 6;   // INSUFFICIENT_DATA (include/anofox_fcst_hip.h)

// the winners of this workgroup's series per method: every thread of the workgroup calls it; cnt is [SEL_WAVES][SELECT_MAX_METHODS]
__device__ __forceinline__ void sel_wave_counts(int w, int n_methods, int (*cnt)[SELECT_MAX_METHODS])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int m = 0; m < n_methods; m++) {
        const uint64_t mask = __ballot(w == m);
        if (lane == 0) cnt[wave][m] = __popcll(mask);
    }
    __syncthreads();
}

__global__ __launch_bounds__(SEL_WG) void select_winner_kernel(const SelectWinnerArgs a)
{
    __shared__ int cnt[SEL_WAVES][SELECT_MAX_METHODS];
    const size_t s = (size_t)blockIdx.x * SEL_WG + threadIdx.x;
    const size_t N = (size_t)a.n_series;
    int w = -2;                                              // (a thread without a series wins nothing)
    if (s < N) {
        int best = -1;
        double best_score = __builtin_nan("");
        for (int m = 0; m < a.n_methods; m++) {
            const double x = a.scores[(size_t)m * a.ld + s];
            if (a.score_status[(size_t)m * N + s] != 0 || x != x) continue;
            if (best < 0 || x < best_score) { best = m; best_score = x; }
        }
        const bool fell = best < 0;
        w = fell ? a.fallback : best;
        a.winner[s] = w;
        a.best_score[s] = best_score;                        // NaN when nothing was admissible
        a.from_fallback[s] = (fell && a.fallback >= 0) ? 1 : 0;
    }
    sel_wave_counts(w, a.n_methods, cnt);
    const int m = threadIdx.x;
    if (m < a.n_methods) {
        int c = 0;
        for (int k = 0; k < SEL_WAVES; k++) c += cnt[k][m];
        a.counts[(size_t)m * a.n_wg + blockIdx.x] = c;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) a.counts[(size_t)a.n_methods * a.n_wg] = 0;     // the scan turns it into the total
}

// the inclusive scan of one value per thread over the workgroup, in thread order; *total: the workgroup's sum
__device__ __forceinline__ int sel_block_scan(int v, int *wave_sum, int *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int d = 1; d < 64; d <<= 1) {
        const int u = __shfl_up(v, d);
        if (lane >= d) v += u;
    }
    __syncthreads();                                         // (wave_sum of an earlier call has been read)
    if (lane == 63) wave_sum[wave] = v;
    __syncthreads();
    int before = 0, all = 0;
    for (int k = 0; k < SEL_WAVES; k++) {
        if (k < wave) before += wave_sum[k];
        all += wave_sum[k];
    }
    *total = all;
    return v + before;
}

__global__ __launch_bounds__(SEL_WG) void select_scan_reduce_kernel(const int32_t *data, size_t n, int32_t *sums)
{
    __shared__ int wave_sum[SEL_WAVES];
    const size_t base = (size_t)blockIdx.x * SEL_SCAN_CHUNK + (size_t)threadIdx.x * SEL_SCAN_PER_THREAD;
    int v = 0;
    for (int k = 0; k < SEL_SCAN_PER_THREAD; k++)
        if (base + k < n) v += data[base + k];
    int total;
    sel_block_scan(v, wave_sum, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// in place: data[i] = chunk_offset[chunk of i] + the sum of the chunk's elements before i (chunk_offset null: 0)
__global__ __launch_bounds__(SEL_WG) void select_scan_apply_kernel(int32_t *data, size_t n, const int32_t *chunk_offset)
{
    __shared__ int wave_sum[SEL_WAVES];
    const size_t base = (size_t)blockIdx.x * SEL_SCAN_CHUNK + (size_t)threadIdx.x * SEL_SCAN_PER_THREAD;
    int x[SEL_SCAN_PER_THREAD], v = 0;
#pragma unroll
    for (int k = 0; k < SEL_SCAN_PER_THREAD; k++) {
        x[k] = base + k < n ? data[base + k] : 0;
        v += x[k];
    }
    int total;
    int run = sel_block_scan(v, wave_sum, &total) - v + (chunk_offset ? chunk_offset[blockIdx.x] : 0);
#pragma unroll
    for (int k = 0; k < SEL_SCAN_PER_THREAD; k++) {
        if (base + k < n) data[base + k] = run;
        run += x[k];
    }
}

__global__ __launch_bounds__(SEL_WG) void select_partition_kernel(const SelectWinnerArgs a)
{
    __shared__ int cnt[SEL_WAVES][SELECT_MAX_METHODS];
    const size_t s = (size_t)blockIdx.x * SEL_WG + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int w = -2;
    if (s < (size_t)a.n_series) {
        w = a.winner[s];
        if (w < 0 || w >= a.n_methods) w = -2;
    }
    sel_wave_counts(w, a.n_methods, cnt);
    // (every lane takes part in every ballot: the loop bound is uniform)
    int rank = 0;
    for (int m = 0; m < a.n_methods; m++) {
        const uint64_t mask = __ballot(w == m);
        if (w == m) rank = __popcll(mask & ((1ull << lane) - 1ull));
    }
    if (w >= 0) {
        for (int k = 0; k < wave; k++) rank += cnt[k][w];
        const size_t at = (size_t)a.counts[(size_t)w * a.n_wg + blockIdx.x] + (size_t)rank;
        if (at < (size_t)a.n_series) a.members[at] = (int32_t)s;         // (always: the counts add up to at most n_series)
    }
    if (blockIdx.x == 0 && threadIdx.x <= a.n_methods) a.offsets[threadIdx.x] = a.counts[(size_t)threadIdx.x * a.n_wg];
}

__global__ __launch_bounds__(SEL_COLS) void select_gather_kernel(const SelectMoveArgs a)
{
    const size_t j = (size_t)blockIdx.x * SEL_COLS + threadIdx.x;
    if (j >= a.ld_m) return;
    int s = -1, L = 0;
    if (j < a.n_m) {
        s = a.members[a.off + j];
        if (s < 0 || s >= a.n_series) s = -1;                // (not a series of the block: an empty column)
        else {
            L = a.len[s];
            if (L < 0) L = 0;
            if ((size_t)L > a.t_rows) L = (int)a.t_rows;
        }
    }
    if (blockIdx.y == 0) a.len_out[j] = L;
    const size_t n_tiles = (a.t_rows + SEL_ROWS - 1) / SEL_ROWS;
    for (size_t tile = blockIdx.y; tile < n_tiles; tile += gridDim.y) {
        const size_t t0 = tile * SEL_ROWS, t1 = t0 + SEL_ROWS < a.t_rows ? t0 + SEL_ROWS : a.t_rows;
        for (size_t t = t0; t < t1; t++) a.y_out[t * a.ld_m + j] = s >= 0 ? a.y[t * a.ld_src + (size_t)s] : 0.0;
    }
}

__global__ __launch_bounds__(256) void select_scatter_kernel(const SelectMoveArgs a)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t h = (size_t)a.h;
    if (e >= a.n_m * h) return;
    const size_t j = e / h, i = e % h;
    const int s = a.members[a.off + j];
    if (s < 0 || s >= a.n_series) return;
    const size_t to = (size_t)s * h + i;
    if (a.yhat) a.yhat[to] = a.yhat_m[e];
    if (a.lower) a.lower[to] = a.lower_m[e];
    if (a.upper) a.upper[to] = a.upper_m[e];
    if (i == 0) {
        if (a.model_code) a.model_code[s] = a.code_m[j];
        if (a.status) a.status[s] = a.status_m[j];
    }
}

__global__ __launch_bounds__(256) void select_unchosen_kernel(const SelectMoveArgs a)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t h = (size_t)a.h;
    if (e >= (size_t)a.n_series * h) return;
    const size_t s = e / h;
    const int w = a.winner[s];
    if (w >= 0) return;
    const double nan = __builtin_nan("");
    if (a.yhat) a.yhat[e] = nan;
    if (a.lower) a.lower[e] = nan;
    if (a.upper) a.upper[e] = nan;
    if (e % h == 0) {
        if (a.model_code) a.model_code[s] = 0;
        if (a.status) a.status[s] = SEL_STATUS_UNCHOSEN;
    }
}

// ascending bitonic network over 16 keys in registers: every index is a compile-time constant once the loops are unrolled
__device__ __forceinline__ void sel_sort16(uint64_t (&v)[SELECT_MAX_METHODS])
{
#pragma unroll
    for (int k = 2; k <= SELECT_MAX_METHODS; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (int p = 0; p < SELECT_MAX_METHODS / 2; p++) {
                const int lo = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                const int hi = lo | j;
                const bool up = (lo & k) == 0;
                const uint64_t x = v[lo], y = v[hi];
                const bool swap = (x > y) == up;
                v[lo] = swap ? y : x;
                v[hi] = swap ? x : y;
            }
        }
    }
}

// v[at] without a dynamic register index (which would send the array to scratch)
__device__ __forceinline__ uint64_t sel_pick16(const uint64_t (&v)[SELECT_MAX_METHODS], int at)
{
    uint64_t r = 0;
#pragma unroll
    for (int k = 0; k < SELECT_MAX_METHODS; k++) r = k == at ? v[k] : r;
    return r;
}

__global__ __launch_bounds__(256) void combine_kernel(const SelectCombineArgs a)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t h = (size_t)a.h;
    if (e >= a.n_rows * h) return;
    const size_t r = e / h, g = r / a.group_div;
    const double nan = __builtin_nan("");
    double out = nan;
    if (a.mode == SELECT_PICK) {
        const int w = a.winner[g];
        if (w >= 0 && w < a.n_methods) out = a.blocks[w][e];
    } else if (a.mode == SELECT_MEDIAN) {
        uint64_t key[SELECT_MAX_METHODS];
        int cnt = 0;
#pragma unroll
        for (int m = 0; m < SELECT_MAX_METHODS; m++) {
            key[m] = ~0ull;                                  // the padding sorts behind every value
            if (m < a.n_methods && a.member_status[(size_t)m * a.n_rows + r] == 0) {
                const double x = a.blocks[m][e];
                if (x == x) { key[m] = st_key(dm_bits(x)); cnt++; }
            }
        }
        if (cnt > 0) {
            sel_sort16(key);
            const double hi = st_unkey(sel_pick16(key, cnt >> 1));
            out = hi;
            if ((cnt & 1) == 0) out = (st_unkey(sel_pick16(key, (cnt >> 1) - 1)) + hi) * 0.5;
        }
    } else {
        const bool weighted = a.mode == SELECT_INVERSE_SCORE;
        double sum = 0.0, wsum = 0.0, wy = 0.0, zsum = 0.0;
        int cnt = 0, zcnt = 0;
        for (int m = 0; m < a.n_methods; m++) {
            if (a.member_status[(size_t)m * a.n_rows + r] != 0) continue;
            const double x = a.blocks[m][e];
            if (x != x) continue;
            if (weighted) {
                const double sc = a.weights[(size_t)m * a.ld_w + g];
                if (sc != sc) continue;                      // not admissible
                if (sc == 0.0) { zsum += x; zcnt++; }
                const double w = 1.0 / sc;
                const double t = w * x;
                wy += t;
                wsum += w;
            } else {
                sum += x;
            }
            cnt++;
        }
        if (cnt > 0) {
            if (!weighted) out = sum / (double)cnt;
            else if (zcnt > 0) out = zsum / (double)zcnt;
            else out = wy / wsum;
        }
    }
    a.out[e] = out;
}

__global__ __launch_bounds__(256) void combine_row_status_kernel(const SelectCombineArgs a)
{
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.n_rows) return;
    const size_t h = (size_t)a.h;
    bool any = false;
    for (size_t i = 0; i < h; i++) {
        const double x = a.out[r * h + i];
        any = any || x == x;
    }
    a.row_status[r] = any ? 0 : 1;
}

// in-place exclusive scan of data[0 .. n); `levels` has room for select_scan_scratch(n) values
void select_scan(int32_t *data, size_t n, int32_t *levels, hipStream_t stream)
{
    const size_t chunks = (n + SEL_SCAN_CHUNK - 1) / SEL_SCAN_CHUNK;
    if (chunks <= 1) {
        hipLaunchKernelGGL(select_scan_apply_kernel, dim3(1), dim3(SEL_WG), 0, stream, data, n, (const int32_t *)nullptr);
        return;
    }
    hipLaunchKernelGGL(select_scan_reduce_kernel, dim3((unsigned)chunks), dim3(SEL_WG), 0, stream, (const int32_t *)data, n, levels);
    select_scan(levels, chunks, levels + chunks, stream);
    hipLaunchKernelGGL(select_scan_apply_kernel, dim3((unsigned)chunks), dim3(SEL_WG), 0, stream, data, n, (const int32_t *)levels);
}

} // namespace

size_t select_workgroups(size_t n_series) { return (n_series + SEL_WG - 1) / SEL_WG; }

size_t select_counts_size(size_t n_series, int n_methods)
{
    size_t n = select_workgroups(n_series) * (size_t)n_methods + 1, total = n;
    while (n > (size_t)SEL_SCAN_CHUNK) {
        n = (n + SEL_SCAN_CHUNK - 1) / SEL_SCAN_CHUNK;
        total += n;
    }
    return total;
}

void launch_select_winner(const SelectWinnerArgs &a, hipStream_t stream)
{
    if (a.n_series <= 0) return;
    const size_t n = a.n_wg * (size_t)a.n_methods + 1;
    hipLaunchKernelGGL(select_winner_kernel, dim3((unsigned)a.n_wg), dim3(SEL_WG), 0, stream, a);
    select_scan(a.counts, n, a.counts + n, stream);
    hipLaunchKernelGGL(select_partition_kernel, dim3((unsigned)a.n_wg), dim3(SEL_WG), 0, stream, a);
}

void launch_select_gather(const SelectMoveArgs &a, hipStream_t stream)
{
    if (a.ld_m == 0) return;
    const size_t n_tiles = (a.t_rows + SEL_ROWS - 1) / SEL_ROWS;
    const unsigned gy = (unsigned)(n_tiles < 1 ? 1 : n_tiles > SEL_MAX_GRID_Y ? SEL_MAX_GRID_Y : n_tiles);
    hipLaunchKernelGGL(select_gather_kernel, dim3((unsigned)((a.ld_m + SEL_COLS - 1) / SEL_COLS), gy), dim3(SEL_COLS), 0, stream, a);
}

void launch_select_scatter(const SelectMoveArgs &a, hipStream_t stream)
{
    const size_t h = (size_t)a.h, moved = a.n_m * h, all = (size_t)a.n_series * h;
    if (moved > 0) hipLaunchKernelGGL(select_scatter_kernel, dim3((unsigned)((moved + 255) / 256)), dim3(256), 0, stream, a);
    if (a.winner && all > 0) hipLaunchKernelGGL(select_unchosen_kernel, dim3((unsigned)((all + 255) / 256)), dim3(256), 0, stream, a);
}

void launch_select_combine(const SelectCombineArgs &a, hipStream_t stream)
{
    const size_t cells = a.n_rows * (size_t)a.h;
    if (cells == 0) return;
    hipLaunchKernelGGL(combine_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, a);
    if (a.row_status) hipLaunchKernelGGL(combine_row_status_kernel, dim3((unsigned)((a.n_rows + 255) / 256)), dim3(256), 0, stream, a);
}

} // namespace anofox
