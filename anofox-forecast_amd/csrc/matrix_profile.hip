// matrix_profile.hip -- the reference's matrix_profile_period (periods.rs:1134-1244), restated op for op: no fused multiply-add
// (-ffp-contract=off), every sum the source's sequential sum from 0.0 in index order, / and sqrt as IEEE (the compiled fp64 division:
// a std of DBL_EPSILON and non-finite values are ordinary operands).  tests/matrix_profile_ref.py performs the same operations, so
// the contract is equality of bits, on every run and through every entry.  No floating-point atomics.
//
// What makes the pairs free to walk in any order: (a - b)^2 == (b - a)^2, so d(i, j) is symmetric, and the source's two strict <
// updates leave in mp[x] the minimum over x's admissible partners and in mpi[x] the SMALLEST partner that attains it.  So every
// update here is a lexicographic (distance, index) minimum; only finite distances take part (a NaN never updates in the source, and
// an entry that stays +inf keeps the source's index 0).  The comparison is made on the square roots, as the source makes it: two
// different sums can round to the same root.  Every distance is its own serial chain over k; nothing is updated incrementally.
//
// matrix_profile_kernel<HOME_LDS>: one workgroup of 256 lanes per series, the grid walks the batch with a stride (persistent
// workgroups), so the workspace is a fixed number of slices whatever n_series is (host_matrix_profile.hpp).
//   pass 1  the mean and std of every subsequence, lanes over i, each a serial chain; they go to the workgroup's workspace slice.
//   pass 2  tiles of 64 rows i x 64 columns j, walked from the first column tile that holds a pair with j - i >= excl.  Per chunk
//           of MPROF_KCHUNK steps of k the z values of the tile's 128 subsequences are computed ONCE into LDS (k-major: zt[k][sub]),
//           so a division is paid per (subsequence, k, tile) and not per pair-step.  A lane owns column j0 + lane and carries the 16
//           rows of its wave in registers across the chunks: the column value is one conflict-free LDS read (neighbouring lanes,
//           neighbouring addresses), the 16 row values are broadcasts of 16 neighbouring doubles.  A pair's chain is computed once
//           and serves both sides: the column side is reduced in the lane and then over the four waves through LDS, the row side
//           over the wave's lanes by shuffles.  Rows first, then columns, a barrier between (a diagonal tile holds both).
//   pass 3  the finite count, sorted[count / 4] by rank counting (exact, any selection has the one answer), the lag histogram
//           (integer LDS / global atomics on counts), the arg max with the smallest lag among equal counts, and how many tie.
// The series, mp, mpi and the histogram (in the series' place, once pass 2 is done) live in LDS while they fit (HOME_LDS, up to
// n = 2,341 at the default m), else in the slice; both instantiate the same code, so they give the same bits.
//
// MATRIX_PROFILE_RECOMPUTE_Z (an experiment build, make EXTRA=-DMATRIX_PROFILE_RECOMPUTE_Z): the tiles hold the raw values and both
// z are recomputed at every pair-step, as the source does.  The same bits; it measures what the tiles buy.
#include "kernels.hpp"

#include <cmath>
#include <string>
#include <vector>

#include "host_matrix_profile.hpp"

namespace anofox {

namespace {

static_assert(MPROF_HOST_MAX_ROWS == MPROF_MAX_ROWS && MPROF_HOST_MIN_ROWS == MPROF_MIN_ROWS && MPROF_HOST_MAX_M == MPROF_MAX_M &&
              MPROF_HOST_TILE == MPROF_TILE && MPROF_HOST_KCHUNK == MPROF_KCHUNK && MPROF_HOST_HOME_DOUBLES == MPROF_HOME_DOUBLES &&
              MPROF_HOST_WORK_BYTES == MPROF_WORK_BYTES, "host_matrix_profile.hpp limits");

constexpr double MP_EPS = 2.2204460492503131e-16;      // f64::EPSILON
constexpr int MP_BLOCK = 256, MP_WAVES = 4;
constexpr int MP_WAVE_ROWS = MPROF_TILE / MP_WAVES;    // rows a lane carries
constexpr int MP_SUBS = 2 * MPROF_TILE;                // subsequences of a tile: 64 rows, then 64 columns
constexpr int MP_NONE = 0x7fffffff;                    // the index of "no partner yet"
static_assert(MPROF_TILE == 64 && MP_SUBS * MPROF_KCHUNK % MP_BLOCK == 0, "a lane is a column; the z fill is an even share");

template <bool HOME_LDS>
__global__ __launch_bounds__(MP_BLOCK) void matrix_profile_kernel(const MatrixProfileArgs a)
{
    __shared__ double zt[MPROF_KCHUNK * MP_SUBS];
    __shared__ double home[HOME_LDS ? MPROF_HOME_DOUBLES : 1];
    __shared__ double col_d[MP_WAVES * MPROF_TILE];
    __shared__ int col_i[MP_WAVES * MPROF_TILE];
    __shared__ unsigned long long best_key;
    __shared__ double selected;
    __shared__ int counts[3];                                      // finite profile values, motifs, lags that share the best count
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const double nan = __builtin_nan(""), inf = __builtin_inf();
    const size_t ld = a.ld;
    for (int s = blockIdx.x; s < a.n_series; s += gridDim.x) {      // (everything that decides a path below is uniform over the workgroup)
        int n = a.len[s];
        if (n < 0) n = 0;
        if ((size_t)n > a.t_rows) n = (int)a.t_rows;
        const int64_t m64 = mprof_subsequence(n, a.subsequence);
        int fail = MPROF_OK;
        if (n < MPROF_MIN_ROWS) fail = MPROF_TOO_SHORT;
        else if (m64 > MPROF_MAX_M) fail = MPROF_OVER_LIMIT;
        if (fail != MPROF_OK && !HOME_LDS) continue;               // (reported by the instantiation that always runs)
        if (fail == MPROF_OK) {
            if (mprof_in_lds(n, a.subsequence) != HOME_LDS) continue;                  // the other instantiation's series
            if (a.work == nullptr || (int)blockIdx.x >= a.work_blocks || a.work_stride < mprof_work_stride(a.t_rows, a.subsequence))
                fail = MPROF_OVER_LIMIT;                           // (the host sizes the workspace for everything it lets through)
        }
        if (fail != MPROF_OK) {
            for (int x = tid; x < a.profile_rows; x += MP_BLOCK) {
                if (a.out_profile) a.out_profile[(size_t)x * ld + s] = nan;
                if (a.out_index) a.out_index[(size_t)x * ld + s] = -1;
            }
            if (tid == 0) a.status[s] = fail;
            continue;
        }
        const int m = (int)m64;
        const int P = n - m + 1;
        const int64_t excl64 = mprof_exclusion(m, a.n_best);
        const int excl = excl64 < (int64_t)P ? (int)excl64 : P;     // an exclusion of P or more leaves no pair
        const size_t T = a.t_rows;
        double *ws = a.work + (size_t)blockIdx.x * a.work_stride;
        double *mean = ws, *sd = ws + T;
        double *v, *mp;
        int *mpi, *hist;
        if constexpr (HOME_LDS) {
            v = home; mp = home + n; mpi = (int *)(home + n + P); hist = (int *)home;
        } else {
            v = ws + 2 * T; mp = ws + 3 * T; mpi = (int *)(ws + 4 * T); hist = (int *)(ws + 4 * T + (T + 1) / 2);
        }
        const double *yg = a.y + s;
        for (int t = tid; t < n; t += MP_BLOCK) v[t] = yg[(size_t)t * ld];
        for (int x = tid; x < P; x += MP_BLOCK) { mp[x] = inf; mpi[x] = MP_NONE; }
        __syncthreads();
        // pass 1: mean and std of every subsequence
        {
            const double md = (double)m;
            for (int x = tid; x < P; x += MP_BLOCK) {
                double sum = 0.0;
                for (int k = 0; k < m; k++) sum += v[x + k];
                const double mu = sum / md;
                double sq = 0.0;
                for (int k = 0; k < m; k++) { const double d = v[x + k] - mu; sq += d * d; }
                mean[x] = mu;
                sd[x] = fmax(sqrt(sq / md), MP_EPS);               // (f64::max: a NaN variance gives EPSILON)
            }
        }
        __syncthreads();
        // pass 2: the pairs, tile by tile
        const int tiles = (P + MPROF_TILE - 1) / MPROF_TILE;
        const int sub = tid & (MP_SUBS - 1), k_first = tid / MP_SUBS;
        for (int rt = 0; rt < tiles; rt++) {
            const int i0 = rt * MPROF_TILE;
            const int64_t first = mprof_first_col_tile(rt, excl);
            for (int ct = (int)(first < tiles ? first : tiles); ct < tiles; ct++) {
                const int j0 = ct * MPROF_TILE;
                const int g = sub < MPROF_TILE ? i0 + sub : j0 + sub - MPROF_TILE;     // the subsequence this lane fills
                const bool g_ok = g < P;
                const double g_mu = g_ok ? mean[g] : 0.0, g_sd = g_ok ? sd[g] : 1.0;
#ifdef MATRIX_PROFILE_RECOMPUTE_Z
                double r_mu[MP_WAVE_ROWS], r_sd[MP_WAVE_ROWS];
#pragma unroll
                for (int r = 0; r < MP_WAVE_ROWS; r++) {
                    const int i = i0 + wave * MP_WAVE_ROWS + r;
                    r_mu[r] = i < P ? mean[i] : 0.0;
                    r_sd[r] = i < P ? sd[i] : 1.0;
                }
                const double c_mu = j0 + lane < P ? mean[j0 + lane] : 0.0, c_sd = j0 + lane < P ? sd[j0 + lane] : 1.0;
#endif
                double acc[MP_WAVE_ROWS];
#pragma unroll
                for (int r = 0; r < MP_WAVE_ROWS; r++) acc[r] = 0.0;
                for (int kc = 0; kc < m; kc += MPROF_KCHUNK) {
                    __syncthreads();                               // the previous chunk has been read
#pragma unroll
                    for (int e = 0; e < MP_SUBS * MPROF_KCHUNK / MP_BLOCK; e++) {
                        const int k = k_first + e * (MP_BLOCK / MP_SUBS), kk = kc + k;
                        double z = 0.0;
                        if (g_ok && kk < m) {
#ifdef MATRIX_PROFILE_RECOMPUTE_Z
                            z = v[g + kk];
#else
                            z = (v[g + kk] - g_mu) / g_sd;
#endif
                        }
                        zt[k * MP_SUBS + sub] = z;
                    }
                    __syncthreads();
                    const int k_end = m - kc < MPROF_KCHUNK ? m - kc : MPROF_KCHUNK;
                    const double *zr = zt + wave * MP_WAVE_ROWS, *zc = zt + MPROF_TILE + lane;
                    for (int k = 0; k < k_end; k++) {
#ifdef MATRIX_PROFILE_RECOMPUTE_Z
                        const double zj = (zc[k * MP_SUBS] - c_mu) / c_sd;
#else
                        const double zj = zc[k * MP_SUBS];
#endif
#pragma unroll
                        for (int r = 0; r < MP_WAVE_ROWS; r++) {
#ifdef MATRIX_PROFILE_RECOMPUTE_Z
                            const double d = (zr[k * MP_SUBS + r] - r_mu[r]) / r_sd[r] - zj;
#else
                            const double d = zr[k * MP_SUBS + r] - zj;
#endif
                            acc[r] += d * d;
                        }
                    }
                }
                // the roots; the column side in the lane (i ascending, strict <), the row side over the wave's lanes
                const int j = j0 + lane;
                double cd = inf, keep_d = inf;
                int ci = MP_NONE, keep_j = MP_NONE;
#pragma unroll
                for (int r = 0; r < MP_WAVE_ROWS; r++) {
                    const int i = i0 + wave * MP_WAVE_ROWS + r;
                    const double d = sqrt(acc[r]);
                    const bool takes_part = i < P && j < P && j - i >= excl && d < inf;        // (a NaN is not < inf)
                    double rd = takes_part ? d : inf;
                    int rj = takes_part ? j : MP_NONE;
                    if (rd < cd) { cd = rd; ci = i; }
#pragma unroll
                    for (int off = 32; off >= 1; off >>= 1) {
                        const double od = __shfl_xor(rd, off);
                        const int oj = __shfl_xor(rj, off);
                        if (od < rd || (od == rd && oj < rj)) { rd = od; rj = oj; }
                    }
                    if (lane == r) { keep_d = rd; keep_j = rj; }
                }
                if (lane < MP_WAVE_ROWS) {
                    const int i = i0 + wave * MP_WAVE_ROWS + lane;
                    if (i < P && (keep_d < mp[i] || (keep_d == mp[i] && keep_j < mpi[i]))) { mp[i] = keep_d; mpi[i] = keep_j; }
                }
                col_d[wave * MPROF_TILE + lane] = cd;
                col_i[wave * MPROF_TILE + lane] = ci;
                __syncthreads();                                   // the rows are updated, the columns' candidates are written
                if (tid < MPROF_TILE && j < P) {
                    double bd = mp[j];
                    int bi = mpi[j];
                    for (int w = 0; w < MP_WAVES; w++) {
                        const double d = col_d[w * MPROF_TILE + tid];
                        const int i = col_i[w * MPROF_TILE + tid];
                        if (d < bd || (d == bd && i < bi)) { bd = d; bi = i; }
                    }
                    mp[j] = bd;
                    mpi[j] = bi;
                }
                // (the next tile meets two barriers before it touches mp or the candidates again: m >= 4 gives at least one chunk)
            }
        }
        __syncthreads();
        // pass 3: the profile as the source leaves it, the threshold, the lags
        if (tid == 0) { counts[0] = 0; counts[1] = 0; counts[2] = 0; best_key = 0ull; selected = inf; }
        __syncthreads();
        for (int x = tid; x < P; x += MP_BLOCK) {
            const double d = mp[x];
            if (d < inf) atomicAdd(&counts[0], 1);
            else mpi[x] = 0;                                       // never updated: the source's initial index
            if (x < a.profile_rows) {
                if (a.out_profile) a.out_profile[(size_t)x * ld + s] = d;
                if (a.out_index) a.out_index[(size_t)x * ld + s] = mpi[x];
            }
        }
        for (int x = P + tid; x < a.profile_rows; x += MP_BLOCK) {
            if (a.out_profile) a.out_profile[(size_t)x * ld + s] = nan;
            if (a.out_index) a.out_index[(size_t)x * ld + s] = -1;
        }
        const int half = n / 2;
        for (int l = tid; l < half; l += MP_BLOCK) hist[l] = 0;    // (in LDS the histogram takes the series' place)
        __syncthreads();
        const int n_finite = counts[0];
        double threshold = inf;
        if (n_finite > 10) {
            const int q = n_finite / 4;
            for (int x = tid; x < P; x += MP_BLOCK) {
                const double d = mp[x];
                if (!(d < inf)) continue;
                int lt = 0, eq = 0;
                for (int y = 0; y < P; y++) {
                    const double e = mp[y];
                    lt += e < d ? 1 : 0;
                    eq += e == d ? 1 : 0;
                }
                if (lt <= q && q < lt + eq) selected = d;          // (every lane that writes writes the same value)
            }
            __syncthreads();
            threshold = selected * 2.0;
        }
        for (int x = tid; x < P; x += MP_BLOCK) {
            const double d = mp[x];
            if (d < threshold && d < inf) {
                const int p = mpi[x];
                const int lag = p > x ? p - x : x - p;
                if ((int64_t)lag > excl64 && lag < half) {
                    atomicAdd(&hist[lag], 1);
                    atomicAdd(&counts[1], 1);
                }
            }
        }
        __syncthreads();
        for (int l = tid; l < half; l += MP_BLOCK) {
            const int c = hist[l];
            if (c > 0) atomicMax(&best_key, ((unsigned long long)c << 32) | (unsigned long long)(0xffffffffu - (unsigned)l));
        }
        __syncthreads();
        const int best_count = (int)(best_key >> 32);
        for (int l = tid; l < half; l += MP_BLOCK)
            if (best_count > 0 && hist[l] == best_count) atomicAdd(&counts[2], 1);
        __syncthreads();
        if (tid == 0) {
            const int n_motifs = counts[1];
            const unsigned best_lag = 0xffffffffu - (unsigned)(best_key & 0xffffffffull);
            a.out_fp[0 * ld + s] = best_count > 0 ? (double)best_lag : nan;
            a.out_fp[1 * ld + s] = n_motifs > 0 ? (double)best_count / (double)n_motifs : 0.0;
            a.out_fp[2 * ld + s] = (double)n_motifs;
            a.out_fp[3 * ld + s] = (double)m;
            a.out_fp[4 * ld + s] = (double)best_count;
            a.out_fp[5 * ld + s] = (double)counts[2];
            a.status[s] = MPROF_OK;
        }
        __syncthreads();                                           // the counters and the home have been read before the next series
    }
}

} // namespace

size_t matrix_profile_work_stride(size_t t_rows, int64_t subsequence) { return mprof_work_stride(t_rows, subsequence); }

int matrix_profile_work_blocks(size_t work_stride, int n_series) { return mprof_work_blocks(work_stride, n_series > 0 ? (size_t)n_series : 0); }

void launch_matrix_profile(const MatrixProfileArgs &a, hipStream_t stream)
{
    if (a.n_series <= 0) return;
    int blocks = a.n_series < MPROF_HOST_MAX_BLOCKS ? a.n_series : MPROF_HOST_MAX_BLOCKS;
    if (a.work_blocks > 0 && blocks > a.work_blocks) blocks = a.work_blocks;
    hipLaunchKernelGGL(matrix_profile_kernel<true>, dim3(blocks), dim3(MP_BLOCK), 0, stream, a);
    if (!mprof_in_lds((int64_t)a.t_rows, a.subsequence))            // (a series of fewer rows takes no more room)
        hipLaunchKernelGGL(matrix_profile_kernel<false>, dim3(blocks), dim3(MP_BLOCK), 0, stream, a);
}

} // namespace anofox
