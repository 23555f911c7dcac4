// changepoint.hip -- Bayesian online changepoint detection (BOCPD) per series, the reference's detect_changepoints_bocpd
// (changepoint.rs:198-356): Normal-Gamma prior mu0 = 0, kappa0 = alpha0 = beta0 = 0.01, constant hazard 1 / max(lambda, 1), the
// Student-t predictive weight (1 + z^2 / nu)^(-(nu + 1) / 2) without its normalising constant, at most 500 tracked run lengths.
//
// One wavefront per series.  The reference shifts its vectors by one run length per step (entry r becomes entry r + 1, entry 0 is
// born empty, entry 500 is cut).  Here an entry never moves: the hypothesis born at step b rests at position b mod 500 for its whole
// life -- lane (position & 63), register slot (position >> 6), 64 lanes x 8 slots -- and its run length at step t is (t - b).  Its
// count equals its run length (changepoint.rs: run_counts[r] == r always), so kappa_n, alpha_n and nu come from r and need no
// storage; sum_x and sum_x2 grow by x and x * x per step exactly as the reference's "old entry r - 1 plus x" does, in the same
// order of additions.  The entry cut at run length 500 is the one whose position the newborn takes, so the cut is the overwrite.
// State is 3 doubles x 8 slots per lane, in registers; nothing lives in LDS or scratch.
//
// While a series is younger than 500 steps only positions <= t are alive: the slot loop skips (wave-uniformly) the slots that hold
// none, and a dead position of a live slot contributes exactly 0.0 to both sums.
//
// The two sums of a step (changepoint mass and the mass that grows) are added per lane in slot order and then across the wave by an
// xor butterfly: a fixed order, no atomics, the same bits on every run and through every entry point.  The order differs from the
// reference's sequential sum, and the power is dm_exp(e * dm_log(b)) (det_math.hpp) instead of libm's pow: the two documented
// differences to the numpy restatement tests/changepoint_ref.py (tolerance 1e-12).  Divisions and the square
// root are the IEEE operations of the source, in its order; the kernel is bound by fp64 issue (profiles/changepoints_m5.txt).
//
// Non-finite input: nothing the source does not do.  A NaN enters sum_x / sum_x2 and the weights, the sum is NaN, `total > 1e-300`
// is false, so the step is left unnormalised (as changepoint.rs:286-290) and `P > 0.5` is false on a NaN.
#include "kernels.hpp"
#include "det_math.hpp"

namespace anofox {

namespace {

constexpr int CP_WAVES = 4;              // series per workgroup: neighbouring columns of the time-major block share cache lines
constexpr int CP_BLOCK = 64 * CP_WAVES;
constexpr int CP_SLOTS = 8;              // 64 lanes x 8 slots = 512 >= BOCPD_MAX_RUN positions
static_assert(64 * CP_SLOTS >= BOCPD_MAX_RUN, "positions");

__device__ __forceinline__ double cp_wave_sum(double v)
{
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the value of `v` in lane `lane` (wave-uniform), as a scalar
__device__ __forceinline__ double cp_lane_value(double v, int lane)
{
    const uint64_t u = dm_bits(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), lane);
    return dm_from_bits(((uint64_t)hi << 32) | lo);
}

// predictive weight of observation x under the run of length r with sums sx, sx2 (changepoint.rs:243-271, run_counts[r] = r)
__device__ __forceinline__ double cp_pred(double x, int r, double sx, double sx2)
{
    const double mu0 = 0.0, kappa0 = 0.01, alpha0 = 0.01, beta0 = 0.01;
    const double c = (double)r;
    const double kappa_n = kappa0 + c;
    const double alpha_n = alpha0 + c / 2.0;
    const double mu_n = r > 0 ? (kappa0 * mu0 + sx) / kappa_n : mu0;
    const double ss = r > 0 ? sx2 - sx * sx / c : 0.0;
    const double dm = mu0 - mu_n;
    const double beta_n = beta0 + 0.5 * fmax(ss, 0.0) + kappa0 * c * (dm * dm) / (2.0 * kappa_n);
    const double scale = sqrt((beta_n * (kappa_n + 1.0)) / (alpha_n * kappa_n));
    const double z = (x - mu_n) / fmax(scale, 1e-10);
    const double nu = 2.0 * alpha_n;
    return dm_exp(-(nu + 1.0) / 2.0 * dm_log(1.0 + z * z / nu));
}

__global__ __launch_bounds__(CP_BLOCK) void bocpd_kernel(const ChangepointArgs a)
{
    const int lane = threadIdx.x & 63;
    const int s = blockIdx.x * CP_WAVES + (threadIdx.x >> 6);
    if (s >= a.n_series) return;                                   // (wave-uniform; the kernel has no barrier)
    int n = a.len[s];
    if ((size_t)(n < 0 ? 0 : n) > a.t_rows) n = (int)a.t_rows;
    if (n < 3) {
        if (lane == 0) a.count[s] = -1;
        return;
    }
    const double hazard = a.hazard, keep = 1.0 - hazard;
    double p[CP_SLOTS], sx[CP_SLOTS], sx2[CP_SLOTS];
#pragma unroll
    for (int j = 0; j < CP_SLOTS; j++) { p[j] = 0.0; sx[j] = 0.0; sx2[j] = 0.0; }
    if (lane == 0) p[0] = 1.0;                                     // run length 0 at position 0
    int tm = 0;                                                    // t mod 500: the position of the entry of run length 0
    int count = 0;
    for (int t0 = 0; t0 < n; t0 += 64) {
        // 64 rows of the series with one load, one row per lane; a step reads its row from the lane that holds it
        const int tl = t0 + lane;
        const double xv = tl < n ? a.y[(size_t)tl * a.ld + s] : 0.0;
        double pv = 0.0;
        const int steps = n - t0 < 64 ? n - t0 : 64;
        for (int i = 0; i < steps; i++) {
            const int t = t0 + i;
            const double x = cp_lane_value(xv, i);
            const double xx = x * x;
            double g[CP_SLOTS];
            double cp_part = 0.0, grow_part = 0.0;
#pragma unroll
            for (int j = 0; j < CP_SLOTS; j++) {
                g[j] = 0.0;
                if (j * 64 <= t) {                                 // (wave-uniform) the slot holds a live entry
                    const int pos = j * 64 + lane;
                    int r = tm - pos;
                    if (r < 0) r += BOCPD_MAX_RUN;
                    const bool live = pos < BOCPD_MAX_RUN && pos <= t;
                    const double pred = cp_pred(x, r, sx[j], sx2[j]);
                    const double w = live ? p[j] * pred : 0.0;
                    g[j] = w * keep;
                    grow_part += g[j];
                    cp_part += w * hazard;
                }
            }
            const double cp = cp_wave_sum(cp_part);
            const double total = cp + cp_wave_sum(grow_part);
            const bool norm = total > 1e-300;
            const int nb = tm + 1 == BOCPD_MAX_RUN ? 0 : tm + 1;   // where the entry of run length 0 of the next step is born
            const double born = norm ? cp / total : cp;
            double first = 0.0;                                    // the new P(run length = 1), in the lane that holds it
#pragma unroll
            for (int j = 0; j < CP_SLOTS; j++) {
                if (j * 64 <= t + 1) {                             // (wave-uniform) live entries and the newborn
                    const int pos = j * 64 + lane;
                    const double q = norm ? g[j] / total : g[j];
                    if (pos == tm) first = q;
                    const bool is_born = pos == nb;
                    p[j] = is_born ? born : q;
                    sx[j] = is_born ? 0.0 : sx[j] + x;
                    sx2[j] = is_born ? 0.0 : sx2[j] + xx;
                }
            }
            const double p1 = cp_lane_value(first, tm & 63);
            if (lane == i) pv = p1;
            tm = nb;
        }
        const bool mine = tl < n;
        const bool fl = mine && pv > 0.5 && tl > 0;
        if (mine) {
            a.prob[(size_t)tl * a.ld + s] = pv;
            a.flag[(size_t)tl * a.ld + s] = fl ? 1 : 0;
        }
        count += __popcll(__ballot(fl));
    }
    if (lane == 0) a.count[s] = count;
}

} // namespace

void launch_bocpd(const ChangepointArgs &a, hipStream_t stream)
{
    if (a.n_series <= 0) return;
    const int blocks = (a.n_series + CP_WAVES - 1) / CP_WAVES;
    hipLaunchKernelGGL(bocpd_kernel, dim3(blocks), dim3(CP_BLOCK), 0, stream, a);
}

} // namespace anofox
