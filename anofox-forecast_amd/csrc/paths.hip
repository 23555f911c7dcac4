// paths.hip -- residual-bootstrap sample paths of a block of forecasts and the quantiles of a block of paths (DESIGN.md section 3
// "Sample paths").  The method is the published one (residual bootstrap with cumulative resampling; the joint bootstrap across
// series of Panagiotelis et al. 2023), the names are this package's own; tests/paths_ref.py is the definition.
//
// Random numbers: Philox4x32-10 (Salmon et al. 2011), counter-based: the draw of (series s, path p, step k) is output word k & 3
// of the block with counter (p, joint ? 0 : s, k >> 2, joint ? 1 : 0) under the key (seed low word, seed high word).  There is no
// state and no draw order, so the launch shape cannot change a bit.  The pool row is j = (u * n) >> 32 on 64-bit integers, n the
// pool length of the series (joint: the call's pool_rows, so that every series of a path takes the SAME row at a step).  The path
// is plain fp64 additions in step order (-ffp-contract=off): cumulative acc = acc + e[j_k], path[k] = point[k] + acc from acc =
// 0.0; independent path[k] = point[k] + e[j_k].
//
//   paths_status_kernel     64 series x 4 row slices per workgroup: the status of every series -- PATHS_RAGGED (joint and a pool
//                           length other than pool_rows), PATHS_EMPTY (no pool row), PATHS_NAN (a NaN among the pool's first
//                           `length` rows or in the point row), in that order of precedence.  The slices meet in LDS by OR.
//   paths_kernel            lanes over SERIES, one wavefront per (64 series, path): the store of a step is one 512-byte row segment
//                           of the time-major block paths[(p * h + k) * ld_out + s] -- the layout the hierarchy entry takes as it
//                           lies -- and in joint mode the 64 pool loads of a step are one segment of a time-major pool as well.
//                           In independent mode the pool loads are scattered (one row per lane).  A lane draws one Philox block
//                           per four steps, then issues the four pool loads together.  A series whose status is not 0 gets NaN.
//                           The workgroups of one tile of 64 series follow each other on one XCD, so that the tile's slice of the
//                           pool is served by that L2 (measured: profiles/paths_m5.txt).
//   path_quantiles_kernel   a workgroup owns a tile of columns, one wavefront per column, and walks the steps: the n_paths rows of
//                           the tile's columns at step k are staged into LDS as total-order keys by all lanes together (lanes
//                           along the columns of a row, then down the rows), padded to a power of two with ~0, sorted per column
//                           by the network of wave_sort.hpp, and lane l < n_levels reads the two neighbours of its level:
//                           out[(l * n_cols + c) * h + k].  A NaN sorts beyond the infinity of its sign, so the first and the last
//                           real key tell whether the column holds one; such a column has status PATHS_NAN and NaN in EVERY
//                           quantile of every step, which is why one wavefront owns all the steps of a column.  A column of keys is
//                           pitched at p2 + 1 words, so the columns of a staged row fall into different banks.
// No floating-point atomics, no atomic at all.
#include "kernels.hpp"
#include "det_math.hpp"
#include "philox.hpp"
#include "wave_sort.hpp"

namespace anofox {

namespace {

constexpr int PT_SLICES = 4;                              // row slices of the status kernel
constexpr int PQ_MAX_WAVES = 16;                          // columns (wavefronts) per workgroup of the quantile kernel
constexpr size_t PQ_LDS_BYTES = 64 * 1024;               // dynamic LDS a workgroup may ask for without raising the limit

// the rows of series s' pool that the draws index: pool_len cut to [0, pool_rows]
__device__ __forceinline__ int pt_length(const PathsArgs &a, int s)
{
    if (!a.pool_len) return a.pool_rows;
    int n = a.pool_len[s];
    if (n < 0) n = 0;
    if (n > a.pool_rows) n = a.pool_rows;
    return n;
}

__global__ __launch_bounds__(64 * PT_SLICES) void paths_status_kernel(const PathsArgs a)
{
    __shared__ int has_nan[PT_SLICES][64];
    const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const size_t sl = (size_t)blockIdx.x * 64 + (size_t)lane;
    const bool in = sl < (size_t)a.n_series;
    const int s = in ? (int)sl : 0;
    const int n = in ? pt_length(a, s) : 0;
    bool bad = false;
    if (in) {
        const double *e = a.pool + (size_t)s * a.pool_stride_s;
        for (int t = slice; t < n; t += PT_SLICES) {
            const double x = e[(size_t)t * a.pool_stride_t];
            bad = bad || x != x;
        }
        const double *f = a.point + (size_t)s * a.point_stride_s;
        for (int k = slice; k < a.horizon; k += PT_SLICES) {
            const double x = f[(size_t)k * a.point_stride_t];
            bad = bad || x != x;
        }
    }
    has_nan[slice][lane] = bad ? 1 : 0;
    __syncthreads();
    if (slice != 0 || !in) return;
    int any = 0;
#pragma unroll
    for (int i = 0; i < PT_SLICES; i++) any |= has_nan[i][lane];
    int32_t status = PATHS_OK;
    if (a.joint && a.pool_len && a.pool_len[s] != a.pool_rows) status = PATHS_RAGGED;
    else if (n == 0) status = PATHS_EMPTY;
    else if (any) status = PATHS_NAN;
    a.status[s] = status;
}

template <bool CUMULATIVE>
__global__ __launch_bounds__(256) void paths_kernel(const PathsArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // Workgroup b -> (tile of 64 series, group of 4 paths).  Consecutive workgroups are dealt round-robin over the 8 XCDs, so b % 8
    // picks the tile within a set of 8 and the groups of one tile follow each other on ONE XCD: the tile's slice of the pool (64
    // series x pool_rows, 1 MB at 1,913 rows) is then read from memory once per XCD and afterwards from that XCD's L2, instead of
    // once per (path, step).  Only speed depends on the placement.
    const unsigned b = blockIdx.x, groups = (unsigned)a.path_groups;
    const unsigned group = (b >> 3) % groups;
    const size_t sl = ((size_t)((b >> 3) / groups) * 8 + (b & 7u)) * 64 + (size_t)lane;
    if (sl >= (size_t)a.n_series) return;                    // (the kernel has no barrier)
    const int s = (int)sl;
    const int h = a.horizon;
    const bool ok = a.status[s] == PATHS_OK;
    const uint64_t n = ok ? (uint64_t)pt_length(a, s) : 0ull;
    const double *e = a.pool + (size_t)s * a.pool_stride_s;
    const double *f = a.point + (size_t)s * a.point_stride_s;
    const double nan = __builtin_nan("");
    const uint32_t c1 = a.joint ? 0u : (uint32_t)s, c3 = a.joint ? 1u : 0u;
    for (int p = (int)group * 4 + wave; p < a.n_paths; p += (int)groups * 4) {
        double *out = a.paths + (size_t)p * (size_t)h * a.ld_out + (size_t)s;
        if (!ok) {
            for (int k = 0; k < h; k++) out[(size_t)k * a.ld_out] = nan;
            continue;
        }
        double acc = 0.0;
        for (int k0 = 0; k0 < h; k0 += 4) {
            uint32_t u[4];
            philox4x32_10((uint32_t)p, c1, (uint32_t)(k0 >> 2), c3, a.key0, a.key1, u);
            double x[4], y[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const bool in = k0 + i < h;
                const uint64_t j = ((uint64_t)u[i] * n) >> 32;                           // j < n <= pool_rows
                x[i] = in ? e[(size_t)j * a.pool_stride_t] : 0.0;
                y[i] = in ? f[(size_t)(k0 + i) * a.point_stride_t] : 0.0;
            }
#pragma unroll
            for (int i = 0; i < 4; i++) {
                if (k0 + i >= h) break;
                double v;
                if (CUMULATIVE) { acc = acc + x[i]; v = y[i] + acc; }
                else v = y[i] + x[i];
                out[(size_t)(k0 + i) * a.ld_out] = v;
            }
        }
    }
}

__device__ __forceinline__ int pq_pow2(int n)
{
    int p2 = 1;
    while (p2 < n) p2 <<= 1;
    return p2;
}

// compute_quantile on the sorted keys of one column: s[lo] * (1 - frac) + s[up] * frac at index = q * (P - 1)
__device__ __forceinline__ double pq_quantile(const uint64_t *buf, int P, double q)
{
    if (q <= 0.0) return st_unkey(buf[0]);
    if (q >= 1.0) return st_unkey(buf[P - 1]);
    const double index = q * (double)(P - 1);
    int lo = (int)floor(index);
    lo = lo < 0 ? 0 : (lo > P - 1 ? P - 1 : lo);            // (in range for 0 < q < 1; the clamp keeps the read inside the buffer)
    const int up = lo + 1 < P - 1 ? lo + 1 : P - 1;
    const double frac = index - (double)lo;
    return st_unkey(buf[lo]) * (1.0 - frac) + st_unkey(buf[up]) * frac;
}

// blockDim.x / 64 columns per workgroup, (p2 + 1) words of dynamic LDS each
__global__ __launch_bounds__(64 * PQ_MAX_WAVES) void path_quantiles_kernel(const PathQuantilesArgs a)
{
    extern __shared__ uint64_t pq_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int W = (int)(blockDim.x >> 6);
    const int P = a.n_paths, h = a.horizon;
    const int p2 = pq_pow2(P);
    const size_t pitch = (size_t)p2 + 1;
    const size_t c0 = (size_t)blockIdx.x * (size_t)W;
    // staging: this thread fills column c0 + scol, rows srow, srow + 64, ...
    const int scol = (int)threadIdx.x % W, srow = (int)threadIdx.x / W;
    const bool sin = c0 + (size_t)scol < (size_t)a.n_cols;
    uint64_t *sbuf = pq_lds + (size_t)scol * pitch;
    // sorting: this wave owns column c0 + wave
    const size_t c = c0 + (size_t)wave;
    const bool mine = c < (size_t)a.n_cols;
    uint64_t *buf = pq_lds + (size_t)wave * pitch;
    double q = 0.0;
#pragma unroll
    for (int l = 0; l < PATHS_MAX_LEVELS; l++) q = lane == l ? a.levels[l] : q;
    const bool level = mine && lane < a.n_levels;
    double *out = a.out + ((size_t)lane * (size_t)a.n_cols + c) * (size_t)h;      // (dereferenced only where `level`)
    bool has_nan = false;
    for (int k = 0; k < h; k++) {
        __syncthreads();                                     // every wave has read the previous step's keys
        for (int p = srow; p < p2; p += 64) {
            uint64_t key = ~0ull;
            if (p < P) key = st_key(dm_bits(sin ? a.paths[((size_t)p * (size_t)h + (size_t)k) * a.ld + c0 + (size_t)scol] : 0.0));
            sbuf[p] = key;
        }
        __syncthreads();
        if (!mine) continue;                                 // (wave-uniform; the barriers above are met by every wave)
        st_sort(buf, p2, lane);
        const double first = st_unkey(buf[0]), last = st_unkey(buf[P - 1]);
        has_nan = has_nan || first != first || last != last;
        if (level) out[k] = pq_quantile(buf, P, q);
    }
    if (!mine) return;
    if (has_nan && level) {
        const double nan = __builtin_nan("");
        for (int k = 0; k < h; k++) out[k] = nan;
    }
    if (lane == 0) a.status[c] = has_nan ? PATHS_NAN : PATHS_OK;
}

} // namespace

void launch_paths(const PathsArgs &a, hipStream_t stream)
{
    if (a.n_series <= 0) return;
    const unsigned gx = (unsigned)(((size_t)a.n_series + 63) / 64);
    hipLaunchKernelGGL(paths_status_kernel, dim3(gx), dim3(64 * PT_SLICES), 0, stream, a);
    if (a.n_paths <= 0 || a.horizon <= 0) return;
    PathsArgs b = a;
    const size_t tiles8 = ((size_t)gx + 7) / 8 * 8;                    // whole sets of 8 tiles; the workgroups of a missing tile return at once
    size_t groups = ((size_t)a.n_paths + 3) / 4;                       // n_paths <= 2,048: at most 512
    const size_t most = (size_t)INT32_MAX / tiles8;                    // (a grid of at most 2^31 - 1 workgroups: a wave then walks several groups)
    groups = groups > most ? (most > 0 ? most : 1) : groups;
    b.path_groups = (int)groups;
    const dim3 grid((unsigned)(tiles8 * groups));
    if (a.mode == PATHS_CUMULATIVE) hipLaunchKernelGGL(paths_kernel<true>, grid, dim3(256), 0, stream, b);
    else hipLaunchKernelGGL(paths_kernel<false>, grid, dim3(256), 0, stream, b);
}

void launch_path_quantiles(const PathQuantilesArgs &a, hipStream_t stream)
{
    if (a.n_cols <= 0 || a.n_paths <= 0 || a.horizon <= 0) return;
    size_t p2 = 1;
    while (p2 < (size_t)a.n_paths) p2 <<= 1;
    const size_t column = (p2 + 1) * sizeof(uint64_t);
    int waves = (int)(PQ_LDS_BYTES / column);                // 2,048 keys: 3 columns; 1,024: 7; 512: 15; fewer: 16
    waves = waves > PQ_MAX_WAVES ? PQ_MAX_WAVES : waves;
    const unsigned blocks = (unsigned)(((size_t)a.n_cols + (size_t)waves - 1) / (size_t)waves);
    hipLaunchKernelGGL(path_quantiles_kernel, dim3(blocks), dim3(64 * waves), (size_t)waves * column, stream, a);
}

} // namespace anofox
