// pelt.hip -- changepoints of a series by the reference's detect_changepoints with the L2 cost (changepoint.rs:26-41, 102-175), the
// optimal-partitioning recurrence it calls PELT:
//     f[0] = -pen;   f[t*] = min over tau of (f[tau] + cost(tau, t*)) + pen,   tau <= t* - ms and (tau == 0 or tau >= ms)
//     cost(tau, t*) = sum of (v[j] - mean)^2 over [tau, t*),  mean = (serial sum of the segment) / len
// The source builds its pruning sets and never reads them, so every (tau, t*) pair pays a pass over its segment: n^3 / 6
// subtract-multiply-add steps per series.  The contract is equality of bits, decisions included: every sum
// below is the source's serial left-to-right chain from 0.0, multiply and add stay apart (-ffp-contract=off), the mean is one IEEE
// division, the candidate is (f[tau] + cost) + pen in that association, and the minimum is the FIRST strict minimum in ascending
// tau, so a NaN candidate is never taken and a t* without a finite candidate gets f = +inf, cp = 0.
//
// One workgroup of 256 lanes per series.  Per row the workgroup keeps v, f, cp and S[tau], the running sum of [tau, t*): the serial
// sum of [tau, t*) is the serial sum of [tau, t* - 1) plus v[t* - 1], so the source's first pass over a segment is one addition.
// Only the second pass is O(len).  Storage: 26 bytes per row in LDS for series of at most PELT_RESIDENT = 2,048 rows (the launch
// sizes the LDS from min(t_rows, 2,048), so a block of short series keeps more workgroups per CU), a slice of a global workspace for
// longer ones (pelt_long_kernel: a fixed number of workgroups walks them).  The body is the same; only the storage differs.
//
// The segment costs do not depend on f, so the workgroup takes PELT_TSTAR consecutive t* in one sweep: a lane owns tau = 256 k + tid
// (consecutive tau per wave: segment lengths within a wave differ by at most 63), reads each v[j] once and feeds PELT_TSTAR
// independent chains with it -- one per t*, each with its own mean.  Each chain is the source's order for its pair.  The lane folds
// its candidates in ascending tau (strict <), the wave and then the workgroup reduce (candidate, tau) pairs by "smaller candidate,
// then smaller tau", which is the first strict minimum because no lane ever holds a NaN (a NaN never passes `<`) and a lane without
// a finite candidate holds (+inf, 0).  Candidates whose tau lies INSIDE the sweep (only when ms < PELT_TSTAR; their segments have
// fewer than PELT_TSTAR rows) need an f of the same sweep: lane 0 adds them serially after the reduction, in ascending tau.
#include "kernels.hpp"
#include <algorithm>

#ifndef PELT_TSTAR
#define PELT_TSTAR 4                     // t* per sweep (1, 2, 4 measured: profiles/pelt_m5.txt)
#endif

namespace anofox {

namespace {

constexpr int PL_BLOCK = 256;
constexpr int PL_WAVES = PL_BLOCK / 64;
constexpr int PL_B = PELT_TSTAR;
constexpr int PL_LONG_GROUPS = 512;      // workgroups (and workspace slices) that walk the series longer than PELT_RESIDENT
static_assert(PL_B >= 1 && PL_B <= 8, "t* per sweep");
static_assert(PELT_RESIDENT <= 65535, "cp in LDS is uint16");

// "smaller candidate, then smaller tau": (c, t) replaces (bc, bt)
__device__ __forceinline__ bool pl_better(double c, int t, double bc, int bt) { return c < bc || (c == bc && t < bt); }

// The recurrence of one series of n >= 2 ms rows; v holds the series.  f, cp: n + 1 entries; S: n.  All lanes of the workgroup call.
// (CP: uint16_t in LDS, where tau <= PELT_RESIDENT, so that three workgroups of M5's 1,913 rows share a CU; int in the workspace.)
template <class CP>
__device__ __forceinline__ void pl_series(const double *v, double *f, double *S, CP *cp, double *red_c, int *red_t, int n, int ms,
                                          double pen)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double inf = __builtin_inf();
    for (int i = tid; i <= n; i += PL_BLOCK) { f[i] = inf; cp[i] = 0; }
    // S[tau] for tau < ms (only tau = 0 is ever a candidate there, the others cost nothing to keep): serial sums of [tau, ms)
    for (int tau = tid; tau < ms; tau += PL_BLOCK) {
        double s = 0.0;
        for (int j = tau; j < ms; j++) s += v[j];
        S[tau] = s;
    }
    __syncthreads();
    if (tid == 0) f[0] = -pen;
    for (int t0 = ms; t0 <= n; t0 += PL_B) {
        __syncthreads();                                           // f, cp, S of the sweep before
        const int nb = n - t0 + 1 < PL_B ? n - t0 + 1 : PL_B;      // t* of this sweep: t0 + b, b < nb
        double vt[PL_B];                                           // v[t0 + b]: what extends a segment from t0 + b to t0 + b + 1
#pragma unroll
        for (int b = 0; b < PL_B; b++) vt[b] = t0 + b < n ? v[t0 + b] : 0.0;
        double best[PL_B];
        int best_t[PL_B];
#pragma unroll
        for (int b = 0; b < PL_B; b++) { best[b] = inf; best_t[b] = 0; }
        const int tau_last = t0 + nb - 1 - ms;                     // the largest candidate of the sweep's last t*
        for (int base = wave * 64; base < t0; base += PL_BLOCK) {  // (wave-uniform)
            const int tau = base + lane;
            const bool mine = tau < t0;
            // the sums and means of [tau, t0 + b)
            double s[PL_B], m[PL_B], c[PL_B];
            s[0] = mine ? S[tau] : 0.0;
#pragma unroll
            for (int b = 1; b < PL_B; b++) s[b] = s[b - 1] + vt[b - 1];
            if (mine) S[tau] = s[PL_B - 1] + vt[PL_B - 1];          // [tau, t0 + PL_B): the next sweep's s[0] (unused after a short last sweep)
            const bool cand = mine && (tau == 0 || tau >= ms) && tau <= tau_last;
            if (!__any(cand)) continue;                            // (wave-uniform)
#pragma unroll
            for (int b = 0; b < PL_B; b++) { m[b] = s[b] / (double)(t0 + b - tau); c[b] = 0.0; }
            // second pass: rows [tau, t0) feed every chain; the first 63 rows of the wave's span start lane by lane
            int j = base;
            const int ramp = base + 63 < t0 ? base + 63 : t0;
            for (; j < ramp; j++) {
                const double x = v[j];
                if (j >= tau) {
#pragma unroll
                    for (int b = 0; b < PL_B; b++) { const double d = x - m[b]; c[b] += d * d; }
                }
            }
#pragma unroll 4
            for (; j < t0; j++) {
                const double x = v[j];
#pragma unroll
                for (int b = 0; b < PL_B; b++) { const double d = x - m[b]; c[b] += d * d; }
            }
            // rows [t0, t0 + b) feed the chains of the later t* only
#pragma unroll
            for (int i = 0; i + 1 < PL_B; i++) {
#pragma unroll
                for (int b = i + 1; b < PL_B; b++) { const double d = vt[i] - m[b]; c[b] += d * d; }
            }
            if (cand) {
                const double ft = f[tau];
#pragma unroll
                for (int b = 0; b < PL_B; b++) {
                    const double x = (ft + c[b]) + pen;
                    if (b < nb && tau <= t0 + b - ms && x < best[b]) { best[b] = x; best_t[b] = tau; }
                }
            }
        }
#pragma unroll
        for (int b = 0; b < PL_B; b++) {
            for (int o = 32; o >= 1; o >>= 1) {
                const double oc = __shfl_xor(best[b], o);
                const int ot = __shfl_xor(best_t[b], o);
                if (pl_better(oc, ot, best[b], best_t[b])) { best[b] = oc; best_t[b] = ot; }
            }
            if (lane == 0) { red_c[wave * PL_B + b] = best[b]; red_t[wave * PL_B + b] = best_t[b]; }
        }
        __syncthreads();
        if (tid == 0) {
            for (int b = 0; b < nb; b++) {
                double bc = red_c[b];
                int bt = red_t[b];
                for (int w = 1; w < PL_WAVES; w++)
                    if (pl_better(red_c[w * PL_B + b], red_t[w * PL_B + b], bc, bt)) { bc = red_c[w * PL_B + b]; bt = red_t[w * PL_B + b]; }
                // candidates inside the sweep, after every earlier tau: t0 <= tau <= t0 + b - ms (t0 >= ms, so they are valid)
                for (int tau = t0; tau <= t0 + b - ms; tau++) {
                    double sum = 0.0;
                    for (int j = tau; j < t0 + b; j++) sum += v[j];
                    const double mean = sum / (double)(t0 + b - tau);
                    double cost = 0.0;
                    for (int j = tau; j < t0 + b; j++) { const double d = v[j] - mean; cost += d * d; }
                    const double x = (f[tau] + cost) + pen;
                    if (x < bc) { bc = x; bt = tau; }
                }
                f[t0 + b] = bc;
                cp[t0 + b] = (CP)bt;
            }
            // S of the taus born in this sweep: serial sums of [tau, t0 + PL_B) (no sweep follows a short one)
            if (t0 + PL_B <= n)
                for (int tau = t0; tau < t0 + PL_B; tau++) {
                    double sum = 0.0;
                    for (int j = tau; j < t0 + PL_B; j++) sum += v[j];
                    S[tau] = sum;
                }
        }
    }
    __syncthreads();
}

// what the series gets: zero flags on its rows, then the backtrack from n (lane 0), the count and f[n]
template <class CP>
__device__ __forceinline__ void pl_emit(const PeltArgs &a, int s, int n, const CP *cp, double cost)
{
    for (int t = threadIdx.x; t < n; t += PL_BLOCK) a.flag[(size_t)t * a.ld + s] = 0;
    __syncthreads();
    if (threadIdx.x == 0) {
        int count = 0;
        if (cp)
            for (int idx = n; idx > 0;) {
                const int tau = (int)cp[idx];
                if (tau > 0) { a.flag[(size_t)tau * a.ld + s] = 1; count++; }
                idx = tau;
            }
        a.count[s] = count;
        a.cost[s] = cost;
    }
}

__device__ __forceinline__ int pl_length(const PeltArgs &a, int s)
{
    int n = a.len[s];
    if (n < 0) n = 0;
    if ((size_t)n > a.t_rows) n = (int)a.t_rows;
    return n;
}

__device__ __forceinline__ double pl_penalty(const PeltArgs &a, int n) { return a.pen_tab ? a.pen_tab[n] : a.penalty; }

extern __shared__ double pl_lds[];

// series of at most a.resident rows: v, f, S (fp64) and cp (uint16) in LDS, (a.resident + 1) rows of each
__global__ __launch_bounds__(PL_BLOCK) void pelt_kernel(const PeltArgs a)
{
    __shared__ double red_c[PL_WAVES * PL_B];
    __shared__ int red_t[PL_WAVES * PL_B];
    const int s = blockIdx.x;
    const int n = pl_length(a, s);
    if (n > a.resident) return;                                    // pelt_long_kernel's
    if ((int64_t)n < 2 * a.min_size) { pl_emit(a, s, n, (const int *)nullptr, 0.0); return; }
    const int rows = a.resident + 1;
    double *v = pl_lds, *f = v + rows, *S = f + rows;
    uint16_t *cp = (uint16_t *)(S + rows);
    for (int t = threadIdx.x; t < n; t += PL_BLOCK) v[t] = a.y[(size_t)t * a.ld + s];
    __syncthreads();
    pl_series(v, f, S, cp, red_c, red_t, n, (int)a.min_size, pl_penalty(a, n));
    pl_emit(a, s, n, (const uint16_t *)cp, f[n]);
}

// longer series: the same arrays in a slice of the global workspace, a.work_groups workgroups walk them
__global__ __launch_bounds__(PL_BLOCK) void pelt_long_kernel(const PeltArgs a)
{
    __shared__ double red_c[PL_WAVES * PL_B];
    __shared__ int red_t[PL_WAVES * PL_B];
    const size_t rows = a.t_rows + 1;
    double *v = a.work + (size_t)blockIdx.x * a.work_stride, *f = v + rows, *S = f + rows;
    int *cp = (int *)(S + rows);
    for (int s = blockIdx.x; s < a.n_series; s += a.work_groups) {
        const int n = pl_length(a, s);
        if (n <= a.resident) continue;                             // (workgroup-uniform)
        if ((int64_t)n < 2 * a.min_size) { pl_emit(a, s, n, (const int *)nullptr, 0.0); continue; }
        __syncthreads();                                           // the series before has been read out
        for (int t = threadIdx.x; t < n; t += PL_BLOCK) v[t] = a.y[(size_t)t * a.ld + s];
        __syncthreads();
        pl_series(v, f, S, cp, red_c, red_t, n, (int)a.min_size, pl_penalty(a, n));
        pl_emit(a, s, n, (const int *)cp, f[n]);
    }
}

} // namespace

int pelt_resident(size_t t_rows) { return (int)std::min<size_t>(t_rows, (size_t)PELT_RESIDENT); }

// doubles per workspace slice (0: every series fits the LDS): v, f, S of t_rows + 1 rows and cp in half as many words
size_t pelt_work_stride(size_t t_rows)
{
    if (t_rows <= (size_t)PELT_RESIDENT) return 0;
    const size_t rows = t_rows + 1;
    return 3 * rows + (rows + 1) / 2;
}

int pelt_work_groups(int n_series) { return n_series < PL_LONG_GROUPS ? n_series : PL_LONG_GROUPS; }

void launch_pelt(const PeltArgs &a, hipStream_t stream)
{
    if (a.n_series <= 0) return;
    const size_t rows = (size_t)a.resident + 1;
    const size_t lds = rows * (3 * sizeof(double) + sizeof(uint16_t)) + 8;
    hipLaunchKernelGGL(pelt_kernel, dim3(a.n_series), dim3(PL_BLOCK), lds, stream, a);
    if (a.t_rows > (size_t)a.resident && a.work && a.work_groups > 0)
        hipLaunchKernelGGL(pelt_long_kernel, dim3(a.work_groups), dim3(PL_BLOCK), 0, stream, a);
}

} // namespace anofox
