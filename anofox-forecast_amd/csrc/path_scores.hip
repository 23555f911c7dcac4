// path_scores.hip -- the scores of a block of sample paths against the actuals (DESIGN.md section 3 "Path scores"): the CRPS of every
// (column, step) in its sorted form, the rank of the actual among the paths, the pinball loss of the sample's quantiles, and the
// energy score of a range of columns in the estimator of Panagiotelis et al. 2023 (consecutive paths as the independent copy).  The
// names are this package's own; tests/path_scores_ref.py is the definition, bit for bit.
//
// ONE order of addition serves every sum over paths and over columns, the wave sum W: lane l adds the terms i = l (mod 64) serially
// from 0.0, ascending in i, and the 64 partials are combined in lane order, ((a_0 + a_1) + a_2) + ... + a_63.  It is what a wavefront
// does naturally and it has one answer whatever the launch shape.  Plain fp64 operations (-ffp-contract=off), the compiled division
// and sqrt (both correctly rounded).
//
//   path_scores_kernel       the staging, padding, pitch and sort of path_quantiles_kernel (paths.hip): a workgroup owns a tile of
//                            columns, one wavefront per column, and walks the steps.  After the sort of a step the lanes stride the
//                            sorted column in LDS for W(|d_i|) and W((2i - P + 1) * d_i), d_i = x_(i) - y, and for the counts of
//                            x < y and x == y (added as integers); lane l < n_levels reads its quantile as the quantile kernel does
//                            and keeps the running sum of its pinball terms, every lane that of the CRPS.  A step whose actual is NaN
//                            has NaN / -1 and does not enter the means.  A column with a NaN among its paths has status 2 and NaN in
//                            every figure, which is why one wavefront owns all the steps of a column.  Every output but the status
//                            may be NULL: a caller who wants quantiles and scores pays one sort.
//   path_energy_rows_kernel  one wavefront per row (path p, step k) of the time-major block, four rows p .. p + 3 of one step per
//                            workgroup: lanes stride the column range in 512-byte segments, form (x - y)^2 and (x - x')^2 against row
//                            p + 1 in one pass, combine the partials in lane order and write the two roots into the workspace.  The
//                            partner row is the next wave's own row, so its second read is served by the cache.
//   path_energy_steps_kernel one lane per step: the serial sums over p, es[k].
//   path_energy_mean_kernel  one lane: the serial mean of the non-NaN es[k].
// No atomics, no floating-point atomics.
#include "kernels.hpp"
#include "det_math.hpp"
#include "wave_sort.hpp"

namespace anofox {

namespace {

constexpr int PS_MAX_WAVES = 16;                          // columns (wavefronts) per workgroup, as the quantile kernel
constexpr size_t PS_LDS_BYTES = 64 * 1024;               // dynamic LDS a workgroup may ask for without raising the limit
constexpr int PE_WAVES = 4;                               // rows per workgroup of the energy pass

__device__ __forceinline__ double ps_lane_value(double v, int l)
{
    const uint64_t u = dm_bits(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, l), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), l);
    return dm_from_bits(((uint64_t)hi << 32) | (uint64_t)lo);
}

// ((a_0 + a_1) + a_2) + ... + a_63 of the lanes' partials; every lane gets the sum
__device__ __forceinline__ double ps_combine(double a)
{
    double w = ps_lane_value(a, 0);
#pragma unroll
    for (int l = 1; l < 64; l++) w = w + ps_lane_value(a, l);
    return w;
}

__device__ __forceinline__ int ps_count(int n)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
    return n;
}

__device__ __forceinline__ int ps_pow2(int n)
{
    int p2 = 1;
    while (p2 < n) p2 <<= 1;
    return p2;
}

// level q of the sorted keys of one column, as pq_quantile of paths.hip: s[lo] * (1 - frac) + s[up] * frac at index = q * (P - 1)
__device__ __forceinline__ double ps_quantile(const uint64_t *buf, int P, double q)
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
__global__ __launch_bounds__(64 * PS_MAX_WAVES) void path_scores_kernel(const PathScoresArgs a)
{
    extern __shared__ uint64_t ps_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int W = (int)(blockDim.x >> 6);
    const int P = a.n_paths, h = a.horizon;
    const int p2 = ps_pow2(P);
    const size_t pitch = (size_t)p2 + 1;
    const size_t c0 = (size_t)blockIdx.x * (size_t)W;
    // staging: this thread fills column c0 + scol, rows srow, srow + 64, ...
    const int scol = (int)threadIdx.x % W, srow = (int)threadIdx.x / W;
    const bool sin = c0 + (size_t)scol < (size_t)a.n_cols;
    uint64_t *sbuf = ps_lds + (size_t)scol * pitch;
    // sorting and scoring: this wave owns column c0 + wave
    const size_t c = c0 + (size_t)wave;
    const bool mine = c < (size_t)a.n_cols;
    const uint64_t *buf = ps_lds + (size_t)wave * pitch;
    double q = 0.0;
#pragma unroll
    for (int l = 0; l < PATHS_MAX_LEVELS; l++) q = lane == l ? a.levels[l] : q;
    const bool level = mine && lane < a.n_levels;
    const size_t cell = c * (size_t)h;                                           // (column c, step 0) of the per-step outputs
    double *out_q = a.quantiles ? a.quantiles + ((size_t)lane * (size_t)a.n_cols + c) * (size_t)h : nullptr;   // (dereferenced only where `level`)
    const double *actual = a.actual + (mine ? c : 0) * a.actual_stride_c;
    const double dP = (double)P, dPP = (double)P * (double)P;
    const double nan = __builtin_nan("");
    bool has_nan = false;
    double crps_sum = 0.0, pin_sum = 0.0;
    int steps = 0;
    for (int k = 0; k < h; k++) {
        __syncthreads();                                     // every wave has read the previous step's keys
        for (int p = srow; p < p2; p += 64) {
            uint64_t key = ~0ull;
            if (p < P) key = st_key(dm_bits(sin ? a.paths[((size_t)p * (size_t)h + (size_t)k) * a.ld + c0 + (size_t)scol] : 0.0));
            sbuf[p] = key;
        }
        __syncthreads();
        if (!mine) continue;                                 // (wave-uniform; the barriers above are met by every wave)
        st_sort(ps_lds + (size_t)wave * pitch, p2, lane);
        const double first = st_unkey(buf[0]), last = st_unkey(buf[P - 1]);
        has_nan = has_nan || first != first || last != last;
        const double y = actual[(size_t)k * a.actual_stride_k];
        const bool have = y == y;                            // (wave-uniform)
        double quant = 0.0;
        if (level) {
            quant = ps_quantile(buf, P, q);
            if (out_q) out_q[k] = quant;
        }
        if (!have) {
            if (lane == 0) {
                if (a.crps) a.crps[cell + (size_t)k] = nan;
                if (a.below) a.below[cell + (size_t)k] = -1;
                if (a.equal) a.equal[cell + (size_t)k] = -1;
            }
            continue;
        }
        double s1 = 0.0, s2 = 0.0;
        int below = 0, equal = 0;
        for (int i = lane; i < P; i += 64) {
            const double x = st_unkey(buf[i]);
            const double d = x - y;
            s1 = s1 + fabs(d);
            s2 = s2 + (double)(2 * i - P + 1) * d;
            below += x < y ? 1 : 0;
            equal += x == y ? 1 : 0;
        }
        const double w1 = ps_combine(s1), w2 = ps_combine(s2);
        const double crps = w1 / dP - w2 / dPP;
        below = ps_count(below);
        equal = ps_count(equal);
        crps_sum = crps_sum + crps;
        if (level) {
            const double e = y - quant;
            pin_sum = pin_sum + (e >= 0.0 ? q * e : (q - 1.0) * e);
        }
        steps++;
        if (lane == 0) {
            if (a.crps) a.crps[cell + (size_t)k] = crps;
            if (a.below) a.below[cell + (size_t)k] = below;
            if (a.equal) a.equal[cell + (size_t)k] = equal;
        }
    }
    if (!mine) return;
    if (has_nan) {
        for (int k = 0; k < h; k++) {
            if (level && out_q) out_q[k] = nan;
            if (lane == 0) {
                if (a.crps) a.crps[cell + (size_t)k] = nan;
                if (a.below) a.below[cell + (size_t)k] = -1;
                if (a.equal) a.equal[cell + (size_t)k] = -1;
            }
        }
    }
    if (a.column) {
        const double n = (double)steps;
        const bool none = has_nan || steps == 0;
        if (lane == 0) {
            a.column[c] = none ? nan : crps_sum / n;
            a.column[a.ld_column + c] = has_nan ? nan : n;
        }
        if (level) a.column[(size_t)(2 + lane) * a.ld_column + c] = none ? nan : pin_sum / n;
    }
    if (lane == 0) a.status[c] = has_nan ? PATH_SCORES_NAN : (steps == 0 ? PATH_SCORES_NO_ACTUAL : PATH_SCORES_OK);
}

// workgroup b: step k = b % h, paths 4 * (b / h) + wave
__global__ __launch_bounds__(64 * PE_WAVES) void path_energy_rows_kernel(const PathEnergyArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = a.horizon, P = a.n_paths;
    const int k = (int)(blockIdx.x % (unsigned)h);
    const size_t pl = (size_t)(blockIdx.x / (unsigned)h) * PE_WAVES + (size_t)wave;
    if (pl >= (size_t)P) return;                             // (the kernel has no barrier)
    const int p = (int)pl;
    const bool partner = p + 1 < P;
    const double *row = a.paths + ((size_t)p * (size_t)h + (size_t)k) * a.ld;
    const double *next = partner ? row + (size_t)h * a.ld : row;
    const double *actual = a.actual + (size_t)k * a.actual_stride_k;
    double s1 = 0.0, s2 = 0.0;
    for (size_t c = (size_t)a.col_begin + (size_t)lane; c < (size_t)a.col_end; c += 64) {
        const double x = row[c], x2 = next[c], y = actual[c * a.actual_stride_c];
        const double d1 = x - y, d2 = x - x2;
        s1 = s1 + d1 * d1;
        s2 = s2 + d2 * d2;
    }
    const double w1 = ps_combine(s1), w2 = ps_combine(s2);
    if (lane == 0) {
        const size_t r = (size_t)p * (size_t)h + (size_t)k;
        a.workspace[r] = sqrt(w1);
        a.workspace[(size_t)P * (size_t)h + r] = partner ? sqrt(w2) : 0.0;
    }
}

__global__ __launch_bounds__(256) void path_energy_steps_kernel(const PathEnergyArgs a)
{
    const size_t kl = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (kl >= (size_t)a.horizon) return;
    const size_t h = (size_t)a.horizon;
    const int P = a.n_paths;
    const double *d1 = a.workspace + kl, *d2 = a.workspace + (size_t)P * h + kl;
    double s1 = 0.0, s2 = 0.0;
    for (int p = 0; p < P; p++) s1 = s1 + d1[(size_t)p * h];
    for (int p = 0; p + 1 < P; p++) s2 = s2 + d2[(size_t)p * h];
    a.es[kl] = P == 1 ? s1 : s1 / (double)P - s2 / (2.0 * (double)(P - 1));
}

__global__ __launch_bounds__(64) void path_energy_mean_kernel(const PathEnergyArgs a)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double total = 0.0;
    long long count = 0;
    for (int k = 0; k < a.horizon; k++) {
        const double v = a.es[k];
        if (v == v) { total = total + v; count++; }
    }
    a.summary[0] = count > 0 ? total / (double)count : __builtin_nan("");
    a.summary[1] = (double)count;
}

} // namespace

void launch_path_scores(const PathScoresArgs &a, hipStream_t stream)
{
    if (a.n_cols <= 0 || a.n_paths <= 0 || a.horizon <= 0) return;
    size_t p2 = 1;
    while (p2 < (size_t)a.n_paths) p2 <<= 1;
    const size_t column = (p2 + 1) * sizeof(uint64_t);
    int waves = (int)(PS_LDS_BYTES / column);                // 2,048 keys: 3 columns; 1,024: 7; 512: 15; fewer: 16
    waves = waves > PS_MAX_WAVES ? PS_MAX_WAVES : waves;
    const unsigned blocks = (unsigned)(((size_t)a.n_cols + (size_t)waves - 1) / (size_t)waves);
    hipLaunchKernelGGL(path_scores_kernel, dim3(blocks), dim3(64 * waves), (size_t)waves * column, stream, a);
}

void launch_path_energy(const PathEnergyArgs &a, hipStream_t stream)
{
    if (a.n_paths <= 0 || a.horizon <= 0 || a.col_end <= a.col_begin) return;
    const size_t groups = ((size_t)a.n_paths + PE_WAVES - 1) / PE_WAVES;           // n_paths * horizon <= 2^30: the grid fits
    hipLaunchKernelGGL(path_energy_rows_kernel, dim3((unsigned)(groups * (size_t)a.horizon)), dim3(64 * PE_WAVES), 0, stream, a);
    hipLaunchKernelGGL(path_energy_steps_kernel, dim3((unsigned)(((size_t)a.horizon + 255) / 256)), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(path_energy_mean_kernel, dim3(1), dim3(64), 0, stream, a);
}

} // namespace anofox
