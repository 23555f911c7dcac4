// reconcile.hip -- reconciliation of the forecasts of a hierarchy in its constraint form (DESIGN.md section 3 "Reconciliation";
// Hyndman et al. 2011 for OLS, Wickramasuriya et al. 2019 for a diagonal W).  With A[i][s] = how often series s occurs among the
// members of aggregate i and one weight w > 0 per column, a row of base forecasts yhat becomes
//     r_i      = yhat_i - (((0.0 + yhat_b(m0)) + yhat_b(m1)) + ...)          members of i in plan order
//     M        = diag(w_a) + A diag(w_b) A^T,   lambda = M^-1 r              Cholesky, M = L L^T
//     btilde_s = yhat_b(s) + w_b(s) * (((0.0 + lambda_i0) + lambda_i1) + ...)     the aggregates that hold s, ascending, with multiplicity
//     ytilde_i = ((0.0 + btilde(m0)) + btilde(m1)) + ...                     the same chain as anofox_hip_hierarchy_device
// so the output is coherent to the bit whatever the solve's rounding was.  No floating-point atomics: every sum has one fixed order,
// and a run gives the same bits every time (-ffp-contract=off; an fma stands only where one is written).
//
// The factor (launch_reconcile_factor):
//   rec_weights_kernel    a weight of a participating column that is not finite and positive -> info[0] (integer atomicMin)
//   rec_assemble_kernel   one wavefront per row i of M: it walks the members of i in plan order and adds w_b(s) to an LDS accumulator
//                         per entry of leaf_aggs[s] (lanes over those entries; equal neighbours, a series listed twice, are added by
//                         one lane one after the other).  The accumulator holds RA_CHUNK columns; a longer row takes several passes.
//   rec_potrf_kernel      the 64 x 64 diagonal block of panel p, in LDS, lane <-> row; a pivot that is not positive -> info[1]
//   rec_trsm_kernel       the panel below it: one workgroup per 64 rows, X L11^T = A21 in LDS, right-looking over the 64 columns
//   rec_syrk_kernel       the trailing lower triangle in 64 x 64 tiles, 256 threads, K staged in halves of 32:
//                         TRAILING_FMA: 4 x 4 outputs per thread; TRAILING_MFMA: v_mfma_f64_16x16x4_f64, 4 sub-tiles per wavefront
// The apply (launch_reconcile_apply), nothing waits on the host:
//   rec_status_kernel     row t: a base forecast that is not finite in a column with members -> row_status 2, else 0
//   rec_chain_kernel<0>   one wavefront per (aggregate, 64 rows): the member chain over the base bottoms through an LDS tile (lanes
//                         over members on the load, lane <-> row on the sum: the staging of hierarchy.hip's tile route) -> residuals
//   rec_subst_kernel      blocked substitution for all rows at once, one launch per 64-wide panel: workgroup g takes the panel
//                         solved by the previous launch out of the 64 unknowns of block g (32 right-hand sides per workgroup),
//                         and workgroup 0 then solves its block, the next panel, in LDS.  Forward with L, then backward with L^T.
//   rec_bottom_kernel     every column: an empty one is copied, a bottom column gets yhat + w * chain(lambda); aggregates wait for
//   rec_chain_kernel<1>   the member chain over the OUTPUT's bottoms -> the aggregate columns
#include "reconcile_device.hpp"               // the tile sizes and the guarded plan reads, shared with reconcile_mint.hip

namespace anofox {

namespace {

constexpr int ZP = RC + 1;                   // pitch of the substitution's panel of right-hand sides (stored with lanes along the unknowns)
constexpr int RA_CHUNK = 4096;               // columns of M that the assembly accumulates per pass (32 KiB of LDS)

__global__ void rec_init_kernel(int32_t *info)
{
    if (threadIdx.x < 2) info[threadIdx.x] = RECONCILE_NONE;
}

__global__ __launch_bounds__(256) void rec_weights_kernel(const ReconcileFactorArgs a)
{
    const size_t cc = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (cc >= (size_t)a.p.n_out || !a.p.weights) return;
    int o0, o1;
    rec_column(a.p, (int)cc, o0, o1);
    if (o1 == o0) return;
    const double w = a.p.weights[cc];
    if (!(w > 0.0) || !isfinite(w)) atomicMin(&a.info[0], (int32_t)cc);
}

__global__ __launch_bounds__(64) void rec_assemble_kernel(const ReconcileFactorArgs a)
{
    __shared__ double acc[RA_CHUNK];
    const int i = blockIdx.x, lane = threadIdx.x, na = a.p.n_agg;
    if (i >= na) return;
    const int c = a.p.agg_cols[i];
    int o0, o1;
    rec_column(a.p, c, o0, o1);
    const double wa = (a.p.weights && c >= 0 && c < a.p.n_out) ? a.p.weights[c] : 1.0;
    for (int j0 = 0; j0 <= i; j0 += RA_CHUNK) {
        for (int k = lane; k < RA_CHUNK; k += 64) acc[k] = 0.0;
        __syncthreads();
        for (int m0 = o0; m0 < o1; m0 += 64) {
            // 64 members at a time: their leaf ranges and weights are loaded by the lanes, then walked in order
            const int cnt = o1 - m0 < 64 ? o1 - m0 : 64;
            int e0 = 0, e1 = 0;
            double w = 1.0;
            if (lane < cnt) {
                const int s = a.p.members[m0 + lane];
                const int b = rec_bottom_of(a.p, s);
                if (b >= 0) {
                    rec_leaf_range(a.p, s, e0, e1);
                    if (a.p.weights) w = a.p.weights[b];
                }
            }
            for (int q = 0; q < cnt; q++) {
                const int q0 = __shfl(e0, q), q1 = __shfl(e1, q);
                const double wq = __shfl(w, q);
                for (int eb = q0; eb < q1; eb += 64) {
                    const int e = eb + lane;
                    if (e < q1) {
                        const int j = a.p.leaf_aggs[e];
                        const bool first = e == q0 || a.p.leaf_aggs[e - 1] != j;
                        if (first && j >= j0 && j < j0 + RA_CHUNK && j <= i) {
                            double v = acc[j - j0];
                            for (int f = e; f < q1 && a.p.leaf_aggs[f] == j; f++) v += wq;
                            acc[j - j0] = v;
                        }
                    }
                    __syncthreads();             // (one wavefront: the next member reads what this one wrote)
                }
            }
        }
        for (int k = lane; k < RA_CHUNK; k += 64) {
            const int j = j0 + k;
            if (j <= i) a.L[(size_t)i * a.ld_a + (size_t)j] = j == i ? acc[k] + wa : acc[k];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void rec_potrf_kernel(const ReconcileFactorArgs a, int p)
{
    __shared__ double T[RB * RP];
    const int lane = threadIdx.x, na = a.p.n_agg, k0 = p * RB;
    const int kn = na - k0 < RB ? na - k0 : RB;
    for (int r = 0; r < RB; r++) T[r * RP + lane] = (r < kn && lane <= r) ? a.L[(size_t)(k0 + r) * a.ld_a + (size_t)(k0 + lane)] : 0.0;
    __syncthreads();
    for (int k = 0; k < kn; k++) {
        const double d = T[k * RP + k];
        if (!(d > 0.0) && lane == 0 && a.info[1] == RECONCILE_NONE) a.info[1] = k0 + k;
        const double sd = sqrt(d);
        __syncthreads();
        if (lane == k) T[k * RP + k] = sd;
        else if (lane > k && lane < kn) T[lane * RP + k] = T[lane * RP + k] / sd;
        __syncthreads();
        if (lane > k && lane < kn) {
            const double lk = T[lane * RP + k];
            for (int j = k + 1; j <= lane; j++) T[lane * RP + j] = __builtin_fma(-lk, T[j * RP + k], T[lane * RP + j]);
        }
        __syncthreads();
    }
    for (int r = 0; r < kn; r++)
        if (lane <= r) a.L[(size_t)(k0 + r) * a.ld_a + (size_t)(k0 + lane)] = T[r * RP + lane];
}

// X L11^T = A21 for 64 rows of the panel, right-looking so that all 256 threads work: once column k of X is final, thread
// (row, part) takes it out of its 16 columns j > k.  Every element still receives its terms in ascending k, as a row-by-row
// substitution would give them.
__global__ __launch_bounds__(256) void rec_trsm_kernel(const ReconcileFactorArgs a, int p)
{
    __shared__ double D[RB * RP], T[RB * RP];
    const int tid = threadIdx.x, na = a.p.n_agg, k0 = p * RB;
    const int q0 = (p + 1 + (int)blockIdx.x) * RB;
    if (q0 >= na) return;
    const int kn = na - k0 < RB ? na - k0 : RB, qn = na - q0 < RB ? na - q0 : RB;
    for (int e = tid; e < RB * RB; e += 256) {
        const int r = e / RB, c = e % RB;
        D[r * RP + c] = (r < kn && c <= r) ? a.L[(size_t)(k0 + r) * a.ld_a + (size_t)(k0 + c)] : 0.0;
        T[r * RP + c] = (r < qn && c < kn) ? a.L[(size_t)(q0 + r) * a.ld_a + (size_t)(k0 + c)] : 0.0;
    }
    __syncthreads();
    const int row = tid & 63, part = tid >> 6, j_lo = part * (RB / 4), j_hi = j_lo + RB / 4;
    for (int k = 0; k < kn; k++) {
        if (part == k / (RB / 4) && row < qn) T[row * RP + k] = T[row * RP + k] / D[k * RP + k];
        __syncthreads();
        if (row < qn) {
            const double xk = T[row * RP + k];
            for (int j = k + 1 > j_lo ? k + 1 : j_lo; j < j_hi && j < kn; j++) T[row * RP + j] = __builtin_fma(-xk, D[j * RP + k], T[row * RP + j]);
        }
        __syncthreads();
    }
    for (int e = tid; e < RB * RB; e += 256) {
        const int r = e / RB, c = e % RB;
        if (r < qn && c < kn) a.L[(size_t)(q0 + r) * a.ld_a + (size_t)(k0 + c)] = T[r * RP + c];
    }
}

// tile (I, J), J <= I, of the trailing matrix: A_IJ -= L_I,p L_J,p^T.  As / Bs hold [row][k] at an odd pitch: the staging stores run
// along k as the global loads do, without a bank conflict, and the reads go down the rows.
template <int TRAILING> __global__ __launch_bounds__(256) void rec_syrk_kernel(const ReconcileFactorArgs a, int p)
{
    __shared__ double As[RB * KP], Bs[RB * KP];
    const int bi = p + 1 + (int)blockIdx.y, bj = p + 1 + (int)blockIdx.x;
    if (bj > bi) return;
    const int tid = threadIdx.x, na = a.p.n_agg, k0 = p * RB, i0 = bi * RB, j0 = bj * RB;
    if (i0 >= na) return;
    const int kn = na - k0 < RB ? na - k0 : RB;
    const int tx = tid & 15, ty = tid >> 4, wave = tid >> 6, l = tid & 63;
    double acc[4][4];
    rec_double4 macc[4];
#pragma unroll
    for (int x = 0; x < 4; x++) {
        macc[x] = (rec_double4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int y = 0; y < 4; y++) acc[x][y] = 0.0;
    }
    for (int kh = 0; kh < RB; kh += RK) {
        __syncthreads();
        for (int e = tid; e < RB * RK; e += 256) {
            const int row = e / RK, k = e % RK;
            const bool kin = kh + k < kn;
            As[row * KP + k] = (kin && i0 + row < na) ? a.L[(size_t)(i0 + row) * a.ld_a + (size_t)(k0 + kh + k)] : 0.0;
            Bs[row * KP + k] = (kin && j0 + row < na) ? a.L[(size_t)(j0 + row) * a.ld_a + (size_t)(k0 + kh + k)] : 0.0;
        }
        __syncthreads();
        if (TRAILING == RECONCILE_TRAILING_MFMA) {
            // A operand: lane l holds A[row l & 15][k = l >> 4], B operand: B[k = l >> 4][col l & 15]
#pragma unroll
            for (int k = 0; k < RK; k += 4) {
                const int kk = k + (l >> 4);
                const double av = As[(16 * wave + (l & 15)) * KP + kk];
#pragma unroll
                for (int cb = 0; cb < 4; cb++)
                    macc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, Bs[(16 * cb + (l & 15)) * KP + kk], macc[cb], 0, 0, 0);
            }
        } else {
#pragma unroll 8
            for (int k = 0; k < RK; k++) {
                double av[4], bv[4];
#pragma unroll
                for (int x = 0; x < 4; x++) { av[x] = As[(ty * 4 + x) * KP + k]; bv[x] = Bs[(tx * 4 + x) * KP + k]; }
#pragma unroll
                for (int x = 0; x < 4; x++)
#pragma unroll
                    for (int y = 0; y < 4; y++) acc[x][y] = __builtin_fma(av[x], bv[y], acc[x][y]);
            }
        }
    }
    if (TRAILING == RECONCILE_TRAILING_MFMA) {
        // C/D of the f64 form: col = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
        for (int cb = 0; cb < 4; cb++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int gi = i0 + 16 * wave + (l >> 4) + 4 * reg, gj = j0 + 16 * cb + (l & 15);
                if (gi < na && gj <= gi) {
                    double *at = a.L + (size_t)gi * a.ld_a + (size_t)gj;
                    *at = *at - macc[cb][reg];
                }
            }
    } else {
#pragma unroll
        for (int x = 0; x < 4; x++)
#pragma unroll
            for (int y = 0; y < 4; y++) {
                const int gi = i0 + ty * 4 + x, gj = j0 + tx * 4 + y;
                if (gi < na && gj <= gi) {
                    double *at = a.L + (size_t)gi * a.ld_a + (size_t)gj;
                    *at = *at - acc[x][y];
                }
            }
    }
}

// ---- apply ----

__device__ __forceinline__ size_t rec_at(const ReconcileApplyArgs &a, int c, size_t t) { return (size_t)c * a.stride_s + t * a.stride_t; }

__global__ __launch_bounds__(256) void rec_status_kernel(const ReconcileApplyArgs a)
{
    const size_t n_chunks = ((size_t)a.p.n_out + 255) / 256;
    for (size_t t = blockIdx.x; t < a.n_rows; t += gridDim.x) {
        int bad = 0;
        for (size_t chunk = 0; chunk < n_chunks; chunk++) {
            const size_t cc = chunk * 256 + threadIdx.x;
            if (cc >= (size_t)a.p.n_out) continue;
            int o0, o1;
            rec_column(a.p, (int)cc, o0, o1);
            if (o1 > o0 && !isfinite(a.base[rec_at(a, (int)cc, t)])) bad = 1;
        }
        bad = __syncthreads_or(bad);
        if (threadIdx.x == 0) a.row_status[t] = bad ? 2 : 0;
    }
}

// MODE 0: work[t][i] = yhat_i - chain over the base bottoms; MODE 1: out_i = chain over the output's bottoms
template <int MODE> __global__ __launch_bounds__(64) void rec_chain_kernel(const ReconcileApplyArgs a)
{
    __shared__ double tile[RB * RP];
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= a.p.n_agg) return;
    const int c = a.p.agg_cols[i];
    int o0, o1;
    rec_column(a.p, c, o0, o1);
    const double *src = MODE == 0 ? a.base : a.out;
    const size_t n_tiles = (a.n_rows + RB - 1) / RB;
    for (size_t rt = blockIdx.y; rt < n_tiles; rt += gridDim.y) {
        const size_t r0 = rt * RB;
        const int nr = a.n_rows - r0 < (size_t)RB ? (int)(a.n_rows - r0) : RB;
        double sum = 0.0;
        for (int m0 = o0; m0 < o1; m0 += RB) {
            const int cnt = o1 - m0 < RB ? o1 - m0 : RB;
            const int b = lane < cnt ? rec_bottom_of(a.p, a.p.members[m0 + lane]) : -1;
            const size_t off = b >= 0 ? (size_t)b * a.stride_s : 0;
            __syncthreads();                                             // every lane has summed the previous tile
#pragma unroll 8
            for (int k = 0; k < nr; k++) tile[k * RP + lane] = b >= 0 ? src[off + (r0 + (size_t)k) * a.stride_t] : 0.0;
            __syncthreads();
            if (lane < nr) {
                const double *row = tile + lane * RP;
#pragma unroll 8
                for (int j = 0; j < cnt; j++) sum += row[j];
            }
        }
        const size_t r = r0 + (size_t)lane;
        if (lane < nr && c >= 0 && c < a.p.n_out) {
            if (MODE == 0) a.work[r * a.ld_work + (size_t)i] = a.base[rec_at(a, c, r)] - sum;
            else a.out[rec_at(a, c, r)] = a.row_status[r] ? __builtin_nan("") : sum;
        }
    }
}

// One step of the substitution.  BACK = false: L z = r, walking the panels down; BACK = true: L^T lambda = z, walking them up.
// `prev` is the panel that the previous step solved (-1 / the panel count: none yet).  Workgroup g takes the solved panel out of
// the 64 unknowns of block q = prev + 1 + g (prev - 1 - g), and workgroup 0, whose block is the next panel, then solves that
// block's triangle in LDS.  Nothing a step reads is written by another workgroup of the same step.
template <bool BACK> __global__ __launch_bounds__(256) void rec_subst_kernel(const ReconcileApplyArgs a, int prev, int nb)
{
    __shared__ double Lt[RB * RP], Z[RB * ZP];
    const int tid = threadIdx.x, na = a.p.n_agg;
    const bool have_prev = BACK ? prev < nb : prev >= 0;
    const int q = BACK ? prev - 1 - (int)blockIdx.x : prev + 1 + (int)blockIdx.x;
    if (q < 0 || q >= nb) return;
    const int q0 = q * RB, qn = na - q0 < RB ? na - q0 : RB;
    const int k0 = have_prev ? prev * RB : 0;
    const int kn = have_prev ? (na - k0 < RB ? na - k0 : RB) : 0;
    const size_t n_chunks = (a.n_rows + RC - 1) / RC;
    for (size_t ch = blockIdx.y; ch < n_chunks; ch += gridDim.y) {
        const size_t t0 = ch * RC;
        const int nc = a.n_rows - t0 < (size_t)RC ? (int)(a.n_rows - t0) : RC;
        if (have_prev) {
            __syncthreads();
            // Lt[r][k]: what multiplies unknown k of the solved panel in equation r of block q; Z: the solved panel
            for (int e = tid; e < RB * RB; e += 256) {
                if (!BACK) {
                    const int r = e / RB, k = e % RB;
                    Lt[r * RP + k] = (r < qn && k < kn) ? a.L[(size_t)(q0 + r) * a.ld_a + (size_t)(k0 + k)] : 0.0;
                } else {
                    const int k = e / RB, r = e % RB;                    // (block q lies above the panel: lanes along a row of L)
                    Lt[r * RP + k] = (k < kn && r < qn) ? a.L[(size_t)(k0 + k) * a.ld_a + (size_t)(q0 + r)] : 0.0;
                }
            }
            for (int e = tid; e < RB * RC; e += 256) {
                const int c = e / RB, r = e % RB;                        // (lanes along the unknowns: work is [row t][unknown])
                Z[r * ZP + c] = (r < kn && c < nc) ? a.work[(t0 + (size_t)c) * a.ld_work + (size_t)(k0 + r)] : 0.0;
            }
            __syncthreads();
            const int r = tid & 63, c0 = (tid >> 6) * (RC / 4);
            if (r < qn) {
                for (int c = c0; c < c0 + RC / 4 && c < nc; c++) {
                    double *at = a.work + (t0 + (size_t)c) * a.ld_work + (size_t)(q0 + r);
                    double s = *at;
                    for (int k = 0; k < kn; k++) s = __builtin_fma(-Lt[r * RP + k], Z[k * ZP + c], s);
                    *at = s;
                }
            }
        }
        if (blockIdx.x != 0) continue;
        __syncthreads();                                                 // (the block's own stores above are visible to it after this)
        for (int e = tid; e < RB * RB; e += 256) {
            const int r = e / RB, c = e % RB;
            Lt[r * RP + c] = (r < qn && c <= r) ? a.L[(size_t)(q0 + r) * a.ld_a + (size_t)(q0 + c)] : 0.0;
        }
        for (int e = tid; e < RB * RC; e += 256) {
            const int c = e / RB, r = e % RB;
            Z[r * ZP + c] = (r < qn && c < nc) ? a.work[(t0 + (size_t)c) * a.ld_work + (size_t)(q0 + r)] : 0.0;
        }
        __syncthreads();
        // right-looking in LDS, all 256 threads: once unknown k is final, thread (r, cg) takes it out of equation r for its 8
        // right-hand sides (those past nc hold zeros)
        {
            const int r = tid & 63, c_lo = (tid >> 6) * (RC / 4);
            for (int kk = 0; kk < qn; kk++) {
                const int k = BACK ? qn - 1 - kk : kk;
                if (tid < RC) Z[k * ZP + tid] = Z[k * ZP + tid] / Lt[k * RP + k];      // (one division per lane, not eight in a row)
                __syncthreads();
                if (r < qn && (BACK ? r < k : r > k)) {
                    const double lk = BACK ? Lt[k * RP + r] : Lt[r * RP + k];
                    for (int c = c_lo; c < c_lo + RC / 4; c++) Z[r * ZP + c] = __builtin_fma(-lk, Z[k * ZP + c], Z[r * ZP + c]);
                }
                __syncthreads();
            }
        }
        for (int e = tid; e < RB * RC; e += 256) {
            const int c = e / RB, r = e % RB;
            if (r < qn && c < nc) a.work[(t0 + (size_t)c) * a.ld_work + (size_t)(q0 + r)] = Z[r * ZP + c];
        }
        __syncthreads();                                                 // (Z is read to the end before a next chunk overwrites it)
    }
}

__global__ __launch_bounds__(256) void rec_bottom_kernel(const ReconcileApplyArgs a)
{
    const size_t cc = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (cc >= (size_t)a.p.n_out) return;
    const int c = (int)cc;
    int o0, o1;
    rec_column(a.p, c, o0, o1);
    const bool empty = o1 == o0;
    int s = -1;
    if (o1 - o0 == 1) {
        s = a.p.members[o0];
        if (rec_bottom_of(a.p, s) != c) s = -1;
    }
    if (!empty && s < 0) return;                                         // an aggregate: rec_chain_kernel<1>
    int e0 = 0, e1 = 0;
    double w = 1.0;
    if (s >= 0 && a.method != RECONCILE_BOTTOM_UP) {
        rec_leaf_range(a.p, s, e0, e1);
        if (a.p.weights) w = a.p.weights[c];
    }
    for (size_t t = blockIdx.y; t < a.n_rows; t += gridDim.y) {
        const size_t at = rec_at(a, c, t);
        double v = a.base[at];
        if (!empty) {
            if (a.method != RECONCILE_BOTTOM_UP) {
                double acc = 0.0;
                for (int e = e0; e < e1; e++) {
                    const int i = a.p.leaf_aggs[e];
                    if (i >= 0 && i < a.p.n_agg) acc += a.work[t * a.ld_work + (size_t)i];
                }
                v = v + w * acc;
            }
            if (a.row_status[t]) v = __builtin_nan("");
        }
        a.out[at] = v;
    }
}

} // namespace

void launch_reconcile_assemble(const ReconcileFactorArgs &a, hipStream_t stream)
{
    if (a.p.n_agg > 0) hipLaunchKernelGGL(rec_assemble_kernel, dim3((unsigned)a.p.n_agg), dim3(64), 0, stream, a);
}

void launch_reconcile_panels(const ReconcileFactorArgs &a, hipStream_t stream)
{
    const int na = a.p.n_agg;
    if (na <= 0) return;
    const int nb = (na + RB - 1) / RB;
    for (int p = 0; p < nb; p++) {
        hipLaunchKernelGGL(rec_potrf_kernel, dim3(1), dim3(64), 0, stream, a, p);
        const int below = nb - p - 1;
        if (below == 0) break;
        hipLaunchKernelGGL(rec_trsm_kernel, dim3((unsigned)below), dim3(256), 0, stream, a, p);
        if (a.trailing == RECONCILE_TRAILING_MFMA)
            hipLaunchKernelGGL(rec_syrk_kernel<RECONCILE_TRAILING_MFMA>, dim3((unsigned)below, (unsigned)below), dim3(256), 0, stream, a, p);
        else
            hipLaunchKernelGGL(rec_syrk_kernel<RECONCILE_TRAILING_FMA>, dim3((unsigned)below, (unsigned)below), dim3(256), 0, stream, a, p);
    }
}

void launch_reconcile_factor(const ReconcileFactorArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(rec_init_kernel, dim3(1), dim3(64), 0, stream, a.info);
    if (a.p.n_out > 0) hipLaunchKernelGGL(rec_weights_kernel, dim3((unsigned)(((size_t)a.p.n_out + 255) / 256)), dim3(256), 0, stream, a);
    launch_reconcile_assemble(a, stream);
    launch_reconcile_panels(a, stream);
}

// the grid's y extent over n units of work, walked with a stride past the limit
static unsigned rec_grid_y(size_t n) { return (unsigned)(n > REC_MAX_GRID_Y ? REC_MAX_GRID_Y : n); }

void launch_reconcile_status(const ReconcileApplyArgs &a, hipStream_t stream)
{
    if (a.n_rows > 0) hipLaunchKernelGGL(rec_status_kernel, dim3(rec_grid_y(a.n_rows)), dim3(256), 0, stream, a);
}

void launch_reconcile_incoherence(const ReconcileApplyArgs &a, hipStream_t stream)
{
    if (a.n_rows == 0 || a.p.n_agg <= 0) return;
    hipLaunchKernelGGL(rec_chain_kernel<0>, dim3((unsigned)a.p.n_agg, rec_grid_y((a.n_rows + RB - 1) / RB)), dim3(64), 0, stream, a);
}

void launch_reconcile_substitute(const ReconcileApplyArgs &a, hipStream_t stream)
{
    if (a.n_rows == 0 || a.p.n_agg <= 0) return;
    const unsigned gy_chunks = rec_grid_y((a.n_rows + RC - 1) / RC);
    const int nb = (a.p.n_agg + RB - 1) / RB;
    for (int prev = -1; prev < nb - 1; prev++)               // step: take panel `prev` out of the blocks below it, solve panel prev + 1
        hipLaunchKernelGGL(rec_subst_kernel<false>, dim3((unsigned)(prev < 0 ? 1 : nb - 1 - prev), gy_chunks), dim3(256), 0, stream, a, prev, nb);
    for (int prev = nb; prev > 0; prev--)                    // the same upwards with L^T
        hipLaunchKernelGGL(rec_subst_kernel<true>, dim3((unsigned)(prev == nb ? 1 : prev), gy_chunks), dim3(256), 0, stream, a, prev, nb);
}

void launch_reconcile_aggregates(const ReconcileApplyArgs &a, hipStream_t stream)
{
    if (a.n_rows == 0 || a.p.n_agg <= 0) return;
    hipLaunchKernelGGL(rec_chain_kernel<1>, dim3((unsigned)a.p.n_agg, rec_grid_y((a.n_rows + RB - 1) / RB)), dim3(64), 0, stream, a);
}

void launch_reconcile_apply(const ReconcileApplyArgs &a, hipStream_t stream)
{
    if (a.n_rows == 0) return;
    launch_reconcile_status(a, stream);
    if (a.p.n_out <= 0) return;
    if (a.method != RECONCILE_BOTTOM_UP) {
        launch_reconcile_incoherence(a, stream);
        launch_reconcile_substitute(a, stream);
    }
    hipLaunchKernelGGL(rec_bottom_kernel, dim3((unsigned)(((size_t)a.p.n_out + 255) / 256), rec_grid_y(a.n_rows)), dim3(256), 0, stream, a);
    launch_reconcile_aggregates(a, stream);
}

} // namespace anofox
