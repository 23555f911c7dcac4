// ets_paths.hip -- sample paths simulated from fitted ETS models (DESIGN.md section 3 "Model paths"): the state equations of the
// fitted spec run forward from the final states, h steps for each of n_paths paths per series, with innovations that are Gaussian
// (sigma = sqrt(sse / n)) or drawn from a pool of the model's own in-sample innovations.  The method is the textbook one (Hyndman,
// Koehler, Ord & Snyder 2008, section 6.1), the names are this package's own; tests/ets_paths_ref.py is the definition, bit for bit.
//
// Draws: Philox4x32-10 on counters, no state and no draw order, so the launch shape cannot change a bit.  Bootstrap: the rule of
// paths.hip unchanged -- word k & 3 of counter (p, joint ? 0 : s, k >> 2, joint ? 1 : 0), pool row j = (u * n) >> 32.  Gaussian:
// counter (p, s, k >> 2, 2); words (w0, w1) serve steps 4j and 4j + 1, (w2, w3) steps 4j + 2 and 4j + 3 by Box-Muller: u1 = (wa + 0.5)
// 2^-32, u2 = (wb + 0.5) 2^-32 (exact), r = sqrt(-2 dm_log(u1)), (sin, cos) = per_sincos(6.283185307179586 u2), the even step takes
// r cos, the odd one r sin, e = sigma z.  The 32-bit uniform cuts the tails at |z| = sqrt(66 ln 2) = 6.76.
//
// Recursion: the state-space form that tests/ets_ref.py replay_many writes out, the drawn innovation in place of the observed one;
// plain fp64, one rounding per operation (-ffp-contract=off), divisions are `/`.  A damped multiplicative trend takes b^phi =
// dm_pow_pos(b, phi); where b is not a finite positive number the path is broken: that step and every later one are NaN.
//
//   ets_paths_status_kernel   64 series x 4 slices per workgroup: ETS_PATHS_NO_MODEL (a spec that is none of the 25, or no observation),
//                             then the pool statuses of paths.hip in their precedence (PATHS_RAGGED, PATHS_EMPTY, PATHS_NAN); PATHS_NAN
//                             also for a NaN in a parameter or state the spec reads (Gaussian: in sigma).
//   ets_paths_kernel          lanes over SERIES, a wavefront owns (64 series, one path at a time): the store of a step is one 512-byte
//                             row segment of paths[(p * h + k) * ld_out + s].  Level and growth live in registers.  The seasonal states a
//                             path touches are the R = min(m, h) phases of its horizon, kept in LDS in STEP order: slot k % R of lane s
//                             holds phase (n_s + k) % m, so at a step all lanes of a wave read ONE 512-byte LDS row whatever their
//                             lengths (8 bytes per lane, consecutive lanes: every half-wave covers the 64 banks once).  A lane reads
//                             only what it wrote itself: no barrier.  64 lanes x R x 8 bytes per wave within 64 KiB give the waves of a
//                             workgroup (ets_paths_waves: 4 up to R = 32, 3 up to 42, 2 up to 64, 1 up to 128).  The spec is a per-lane
//                             value (AutoETS picks per series): the branches on it are uniform in a uniform batch and cost their union
//                             in a mixed wave; they choose operations, never their order.
//   ets_paths_broken_kernel   64 series x 16 waves per workgroup over the finished block: n_broken = the paths of a series that hold a
//                             NaN.  The waves meet in LDS.
// No atomics.
#include "kernels.hpp"
#include "det_math.hpp"
#include "det_trig.hpp"
#include "philox.hpp"

namespace anofox {

namespace {

constexpr int EP_SLICES = 4;                              // slices of the status kernel
constexpr int EP_MAX_WAVES = 4;                           // waves per workgroup of the simulation kernel
constexpr int EP_COUNT_WAVES = 16;                        // waves per workgroup of the counting kernel
constexpr size_t EP_LDS_BYTES = 64 * 1024;                // dynamic LDS a workgroup may ask for without raising the limit

// one of the 25 specs of the project: error * 15 + trend * 3 + season, no multiplicative error with an additive season
__device__ __forceinline__ bool ep_spec_ok(int id) { return id >= 0 && id < 30 && !(id / 15 == 1 && id % 3 == 1); }

// the rows of series s' pool that the draws index: pool_len cut to [0, pool_rows]
__device__ __forceinline__ int ep_length(const EtsPathsArgs &a, int s)
{
    if (!a.pool_len) return a.pool_rows;
    int n = a.pool_len[s];
    if (n < 0) n = 0;
    if (n > a.pool_rows) n = a.pool_rows;
    return n;
}

__global__ __launch_bounds__(64 * EP_SLICES) void ets_paths_status_kernel(const EtsPathsArgs a)
{
    __shared__ int has_nan[EP_SLICES][64];
    const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const size_t sl = (size_t)blockIdx.x * 64 + (size_t)lane;
    const bool in = sl < (size_t)a.n_series;
    const int s = in ? (int)sl : 0;
    const int id = in ? a.spec[s] : -1;
    const int len = in ? a.lengths[s] : 0;
    const bool model = in && ep_spec_ok(id) && len >= 1;
    const bool boot = a.innovations == ETS_PATHS_BOOTSTRAP;
    const int n = (in && boot) ? ep_length(a, s) : 0;
    bool bad = false;
    if (in && boot) {
        const double *e = a.pool + (size_t)s * a.pool_stride_s;
        for (int t = slice; t < n; t += EP_SLICES) {
            const double x = e[(size_t)t * a.pool_stride_t];
            bad = bad || x != x;
        }
    }
    if (model) {
        const int T = id % 15 / 3, S = id % 3;
        const double *o = a.info + s, *st = a.states + s;
        if (slice == 0) {
            double x = o[0];
            bad = bad || x != x;
            x = st[0];
            bad = bad || x != x;
            if (T != 0) {
                x = o[a.ld];
                bad = bad || x != x;
                x = st[a.ld];
                bad = bad || x != x;
            }
            if (S != 0) { x = o[2 * a.ld]; bad = bad || x != x; }
            if (T == 2 || T == 4) { x = o[3 * a.ld]; bad = bad || x != x; }
            if (!boot) { x = sqrt(o[7 * a.ld] / (double)len); bad = bad || x != x; }
        }
        if (S != 0) {
            const int ph0 = len % a.m;
            for (int k = slice; k < a.ring; k += EP_SLICES) {
                const double x = st[(size_t)(2 + (ph0 + k) % a.m) * a.ld];
                bad = bad || x != x;
            }
        }
    }
    has_nan[slice][lane] = bad ? 1 : 0;
    __syncthreads();
    if (slice != 0 || !in) return;
    int any = 0;
#pragma unroll
    for (int i = 0; i < EP_SLICES; i++) any |= has_nan[i][lane];
    int32_t status = PATHS_OK;
    if (!model) status = ETS_PATHS_NO_MODEL;
    else if (boot && a.joint && a.pool_len && a.pool_len[s] != a.pool_rows) status = PATHS_RAGGED;
    else if (boot && n == 0) status = PATHS_EMPTY;
    else if (any) status = PATHS_NAN;
    a.status[s] = status;
}

// two standard normal draws of two 32-bit words: the even step's and the odd step's
__device__ __forceinline__ void ep_normal_pair(uint32_t wa, uint32_t wb, double &z_even, double &z_odd)
{
    const double u1 = ((double)wa + 0.5) * 0x1p-32, u2 = ((double)wb + 0.5) * 0x1p-32;
    const double r = sqrt(-2.0 * dm_log(u1));
    double sn, cs;
    per_sincos(6.283185307179586 * u2, sn, cs);
    z_even = r * cs;
    z_odd = r * sn;
}

// blockDim.x / 64 = a.waves paths at a time per workgroup, a.ring x 64 doubles of dynamic LDS per wave
__global__ __launch_bounds__(64 * EP_MAX_WAVES) void ets_paths_kernel(const EtsPathsArgs a)
{
    extern __shared__ double ep_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int W = a.waves, R = a.ring;
    // workgroup b -> (tile of 64 series, group of W paths), the groups of a tile following each other on one XCD as in paths_kernel:
    // the tile's slice of a pool stays in that XCD's L2.  Only speed depends on the placement.
    const unsigned blk = blockIdx.x, groups = (unsigned)a.path_groups;
    const unsigned group = (blk >> 3) % groups;
    const size_t sl = ((size_t)((blk >> 3) / groups) * 8 + (blk & 7u)) * 64 + (size_t)lane;
    if (sl >= (size_t)a.n_series) return;                    // (the kernel has no barrier)
    const int s = (int)sl;
    const int h = a.horizon, m = a.m;
    const bool ok = a.status[s] == PATHS_OK;
    const bool boot = a.innovations == ETS_PATHS_BOOTSTRAP;
    const double nan = __builtin_nan("");
    const int id = ok ? a.spec[s] : 0;
    const int E = id / 15, T = id % 15 / 3, S = id % 3;
    const int len = ok ? a.lengths[s] : 1;
    const double *o = a.info + s, *st = a.states + s;
    const double alpha = ok ? o[0] : 0.0;
    const double beta = (ok && T != 0) ? o[a.ld] : 0.0;
    const double gamma = (ok && S != 0) ? o[2 * a.ld] : 0.0;
    const double phi = (ok && (T == 2 || T == 4)) ? o[3 * a.ld] : 1.0;
    const double sigma = (ok && !boot) ? sqrt(o[7 * a.ld] / (double)len) : 0.0;
    const double l0 = ok ? st[0] : 0.0;
    const double b0 = (ok && T != 0) ? st[a.ld] : 0.0;
    const int ph0 = len % m;
    const uint64_t n = (ok && boot) ? (uint64_t)ep_length(a, s) : 0ull;
    const double *e = boot ? a.pool + (size_t)s * a.pool_stride_s : nullptr;
    const uint32_t c1 = boot ? (a.joint ? 0u : (uint32_t)s) : (uint32_t)s, c3 = boot ? (a.joint ? 1u : 0u) : 2u;
    double *ring = ep_lds + (size_t)wave * (size_t)R * 64 + (size_t)lane;       // slot i at ring[i * 64]
    for (int p = (int)group * W + wave; p < a.n_paths; p += (int)groups * W) {
        double *out = a.paths + (size_t)p * (size_t)h * a.ld_out + (size_t)s;
        if (!ok) {
            for (int k = 0; k < h; k++) out[(size_t)k * a.ld_out] = nan;
            continue;
        }
        if (S != 0) {
            int ph = ph0;
            for (int i = 0; i < R; i++) {
                ring[(size_t)i * 64] = st[(size_t)(2 + ph) * a.ld];
                ph = ph + 1 == m ? 0 : ph + 1;
            }
        }
        double l = l0, b = b0;
        bool broken = false;
        int slot = 0;
        for (int k0 = 0; k0 < h; k0 += 4) {
            uint32_t u[4];
            philox4x32_10((uint32_t)p, c1, (uint32_t)(k0 >> 2), c3, a.key0, a.key1, u);
            double x[4];
            if (boot) {
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const uint64_t j = ((uint64_t)u[i] * n) >> 32;                       // j < n <= pool_rows
                    x[i] = k0 + i < h ? e[(size_t)j * a.pool_stride_t] : 0.0;
                }
            } else {
                double z[4] = {0.0, 0.0, 0.0, 0.0};
                ep_normal_pair(u[0], u[1], z[0], z[1]);
                if (k0 + 2 < h) ep_normal_pair(u[2], u[3], z[2], z[3]);
#pragma unroll
                for (int i = 0; i < 4; i++) x[i] = sigma * z[i];
            }
#pragma unroll
            for (int i = 0; i < 4; i++) {
                if (k0 + i >= h) break;
                double *cell = out + (size_t)(k0 + i) * a.ld_out;
                double *sp = ring + (size_t)slot * 64;
                slot = slot + 1 == R ? 0 : slot + 1;
                // q: what the level and the trend give; pt: the trend's part of it
                double pt = 0.0, q = l;
                if (T == 1 || T == 2) {
                    pt = phi * b;
                    q = l + pt;
                } else if (T == 3) {
                    pt = b;
                    q = l * pt;
                } else if (T == 4) {
                    broken = broken || !(b > 0.0 && b <= 1.7976931348623157e308);
                    if (!broken) {
                        pt = dm_pow_pos(b, phi);
                        q = l * pt;
                    }
                }
                if (broken) {
                    *cell = nan;
                    continue;
                }
                const double sj = S != 0 ? *sp : 0.0;
                const double mu = S == 0 ? q : (S == 1 ? q + sj : q * sj);
                const double v = x[i];
                double y, l_new, b_new = 0.0, s_new = 0.0;
                if (E == 0) {
                    y = mu + v;
                    const double vs = S == 2 ? v / sj : v;
                    l_new = q + alpha * vs;
                    if (T == 1 || T == 2) b_new = pt + beta * vs;
                    else if (T >= 3) b_new = pt + beta * (S == 2 ? v / (sj * l) : v / l);
                    if (S == 1) s_new = sj + gamma * v;
                    else if (S == 2) s_new = sj + gamma * v / q;
                } else {
                    y = mu * (1.0 + v);
                    l_new = q * (1.0 + alpha * v);
                    if (T == 1 || T == 2) b_new = pt + beta * q * v;
                    else if (T >= 3) b_new = pt * (1.0 + beta * v);
                    if (S != 0) s_new = sj * (1.0 + gamma * v);
                }
                l = l_new;
                b = b_new;
                if (S != 0) *sp = s_new;
                *cell = y;
            }
        }
    }
}

__global__ __launch_bounds__(64 * EP_COUNT_WAVES) void ets_paths_broken_kernel(const EtsPathsArgs a)
{
    __shared__ int cnt[EP_COUNT_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t sl = (size_t)blockIdx.x * 64 + (size_t)lane;
    const bool in = sl < (size_t)a.n_series;
    const int h = a.horizon;
    int c = 0;
    if (in)
        for (int p = wave; p < a.n_paths; p += EP_COUNT_WAVES) {
            const double *col = a.paths + (size_t)p * (size_t)h * a.ld_out + sl;
            bool bad = false;
            for (int k = 0; k < h; k++) {
                const double x = col[(size_t)k * a.ld_out];
                bad = bad || x != x;
            }
            c += bad ? 1 : 0;
        }
    cnt[wave][lane] = c;
    __syncthreads();
    if (wave != 0 || !in) return;
    int total = 0;
#pragma unroll
    for (int i = 0; i < EP_COUNT_WAVES; i++) total += cnt[i][lane];
    a.n_broken[sl] = total;
}

// lanes over series, the waves of the grid over the rows
__global__ __launch_bounds__(256) void ets_innovations_kernel(const double *y, const double *fitted, size_t ld, const int32_t *lengths,
                                                              const int32_t *spec, int n_series, int t_rows, double *pool, int32_t *pool_len)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t sl = (size_t)blockIdx.x * 64 + (size_t)lane;
    if (sl >= (size_t)n_series) return;
    const int id = spec[sl];
    int len = lengths[sl];
    len = len < 0 ? 0 : (len > t_rows ? t_rows : len);
    if (!ep_spec_ok(id)) len = 0;
    if (blockIdx.y == 0 && wave == 0) pool_len[sl] = len;
    const bool mul = id / 15 == 1;
    for (int t = (int)blockIdx.y * 4 + wave; t < len; t += (int)gridDim.y * 4) {
        const size_t at = (size_t)t * ld + sl;
        const double f = fitted[at];
        double v = y[at] - f;
        if (mul) v = v / f;
        pool[at] = v;
    }
}

__global__ __launch_bounds__(256) void ets_spec_of_kernel(const int32_t *model_code, const int32_t *status, int auto_ets, int explicit_spec,
                                                          int n_series, int32_t *spec)
{
    const size_t s = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= (size_t)n_series) return;
    spec[s] = status[s] == 0 ? (auto_ets ? model_code[s] - 100 : explicit_spec) : -1;
}

__global__ __launch_bounds__(256) void fill_f64_kernel(double *p, size_t n, double value)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = value;
}

} // namespace

int ets_paths_waves(int ring)
{
    const size_t per_wave = (size_t)(ring < 1 ? 1 : ring) * 64 * sizeof(double);
    const size_t w = EP_LDS_BYTES / per_wave;
    return w > (size_t)EP_MAX_WAVES ? EP_MAX_WAVES : (w < 1 ? 1 : (int)w);
}

void launch_ets_paths(const EtsPathsArgs &a, hipStream_t stream)
{
    if (a.n_series <= 0) return;
    EtsPathsArgs b = a;
    b.ring = a.m < a.horizon ? a.m : a.horizon;
    if (b.ring < 1) b.ring = 1;
    b.waves = ets_paths_waves(b.ring);
    const unsigned gx = (unsigned)(((size_t)a.n_series + 63) / 64);
    hipLaunchKernelGGL(ets_paths_status_kernel, dim3(gx), dim3(64 * EP_SLICES), 0, stream, b);
    if (a.n_paths <= 0 || a.horizon <= 0) return;
    const size_t tiles8 = ((size_t)gx + 7) / 8 * 8;                    // whole sets of 8 tiles; the workgroups of a missing tile return at once
    size_t groups = ((size_t)a.n_paths + (size_t)b.waves - 1) / (size_t)b.waves;
    const size_t most = (size_t)INT32_MAX / tiles8;                    // (a grid of at most 2^31 - 1 workgroups: a wave then walks several groups)
    groups = groups > most ? (most > 0 ? most : 1) : groups;
    b.path_groups = (int)groups;
    const size_t lds = (size_t)b.waves * (size_t)b.ring * 64 * sizeof(double);
    hipLaunchKernelGGL(ets_paths_kernel, dim3((unsigned)(tiles8 * groups)), dim3(64 * b.waves), lds, stream, b);
    hipLaunchKernelGGL(ets_paths_broken_kernel, dim3(gx), dim3(64 * EP_COUNT_WAVES), 0, stream, b);
}

void launch_ets_innovations(const double *y, const double *fitted, size_t ld, const int32_t *lengths, const int32_t *spec, int n_series,
                            int t_rows, double *pool, int32_t *pool_len, hipStream_t stream)
{
    if (n_series <= 0) return;
    const unsigned gx = (unsigned)(((size_t)n_series + 63) / 64);
    unsigned gy = (unsigned)((t_rows + 31) / 32);                      // about eight rows per wave
    gy = gy < 1 ? 1 : (gy > 1024 ? 1024 : gy);
    hipLaunchKernelGGL(ets_innovations_kernel, dim3(gx, gy), dim3(256), 0, stream, y, fitted, ld, lengths, spec, n_series, t_rows, pool, pool_len);
}

void launch_ets_spec_of(const int32_t *model_code, const int32_t *status, int auto_ets, int explicit_spec, int n_series, int32_t *spec,
                        hipStream_t stream)
{
    if (n_series <= 0) return;
    hipLaunchKernelGGL(ets_spec_of_kernel, dim3((unsigned)(((size_t)n_series + 255) / 256)), dim3(256), 0, stream, model_code, status, auto_ets,
                       explicit_spec, n_series, spec);
}

void launch_fill_f64(double *p, size_t n, double value, hipStream_t stream)
{
    if (n == 0) return;
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(fill_f64_kernel, dim3((unsigned)(blocks > 65536 ? 65536 : blocks)), dim3(256), 0, stream, p, n, value);
}

} // namespace anofox
