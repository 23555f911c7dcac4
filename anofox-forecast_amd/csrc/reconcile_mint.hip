// reconcile_mint.hip -- MinT with the shrinkage covariance (Wickramasuriya et al. 2019; Schaefer and Strimmer 2005 for the intensity),
// in the constraint form of reconcile.hip (DESIGN.md section 3 "MinT-shrink").  X is the [n_res x n_p] block of base-forecast
// residuals of the participating columns (every bottom, then every aggregate), v_c the uncentred variance of column c:
//     W  = lambda diag(v) + (1 - lambda) X^T X / n_res                          never formed: it is n_p x n_p
//     E  = X_a - chain over the members of X_b                                  the residuals' own incoherence, [n_res x n_agg]
//     M  = lambda (diag(v_a) + A diag(v_b) A^T) + ((1 - lambda) / n_res) E^T E  n_agg x n_agg, M = L L^T
//     mu = M^-1 r,   g = E mu
//     btilde_s = (yhat_b(s) + (lambda v_b(s)) chain(mu over the aggregates that hold s)) - ((1 - lambda) / n_res) sum_t x_t,b(s) g_t
// and the aggregates are the chain over the output's own bottoms, so the output is coherent to the bit.  The shrinkage intensity
// needs sums over all n_p^2 correlation pairs; with xs_tc = x_tc / sqrt(v_c) and G = Xs Xs^T (n_res x n_res) they collapse into
//     fro = sum G_tu^2,  q = sum G_tt^2,  f4 = sum xs_tc^4
//     sum_v = ((q - f4) - (fro - n_p T^2) / T) / (T (T - 1)),  sum_d = fro / T^2 - n_p,  lambda = clamp(sum_v / sum_d, 0, 1)
// No floating-point atomics; every sum has one fixed order, the same in both layouts of the residual block (the layouts differ only
// in which index the lanes of a staging load run along).  An fma stands only where one is written (-ffp-contract=off).
//
// The factor (launch_reconcile_mint_factor):
//   mint_var_kernel          64 columns per wavefront through a 64 x 64 LDS tile; lane <-> column on the sum: the serial chain
//                            ((0.0 + x_0^2) + x_1^2) + ... / n_res.  A residual that is not finite -> info[0], a variance that is
//                            not finite and positive -> info[1] (integer atomicMin).  A second pass, when lambda is estimated: the
//                            column's sum of xs^4
//   mint_gram_kernel         tile (I, J), J <= I, of G for one slice of the participating columns (the inner dimension is cut into
//                            gram_splits slices so that a short block still fills the device); the scaling by 1 / sqrt(v_c) is
//                            applied on the staging load; v_mfma_f64_16x16x4_f64
//   mint_gram_reduce_kernel  per tile: the slices added in slice order, then the tile's sum of squares and of squared diagonal
//                            entries by a fixed tree (a tile below the diagonal counts twice)
//   mint_lambda_kernel       one workgroup: the three sums by a fixed tree, then the intensity
//   rec_chain_kernel<0>      (reconcile.hip) E from the residual block
//   rec_assemble_kernel      (reconcile.hip) diag(v_a) + A diag(v_b) A^T
//   mint_ete_kernel          tile (I, J), J <= I: M = lambda M + ((1 - lambda) / n_res) E^T E, the t terms in ascending order;
//                            RECONCILE_TRAILING_MFMA: v_mfma_f64_16x16x4_f64, 4 sub-tiles per wavefront; RECONCILE_TRAILING_FMA: 4 x 4
//                            outputs per thread (the developer knob reconcile_mint_ete of ANOFOX_HIP_TUNE)
//   rec_potrf / trsm / syrk  (reconcile.hip) the panels of the factor
// The apply (launch_reconcile_mint_apply), nothing waits on the host:
//   rec_status, rec_chain<0>, rec_subst   (reconcile.hip) row_status, r, mu
//   mint_g_kernel            g[row][t] = sum_i E[t][i] mu[row][i], i ascending, 64 t x 32 rows per workgroup
//   mint_bottom_kernel       every column: an empty one is copied, a bottom column gets the update above (sum over t ascending)
//   rec_chain_kernel<1>      (reconcile.hip) the aggregate columns
#include "reconcile_device.hpp"

namespace anofox {

namespace {

constexpr int MINT_ROWS_PER_THREAD = RC / 4; // forecast rows per thread of the two thin products

__global__ void mint_init_kernel(int32_t *info)
{
    if (threadIdx.x < 4) info[threadIdx.x] = RECONCILE_NONE;
}

__global__ void mint_set_lambda_kernel(double *lambda, double value)
{
    if (threadIdx.x == 0) *lambda = value;
}

// participant k: the bottoms in series order, then the aggregates; -1 when the plan is not what the planner wrote
__device__ __forceinline__ int mint_participant(const ReconcilePlan &p, int k)
{
    if (k < 0) return -1;
    if (k < p.n_series) return rec_bottom_of(p, k);
    const int i = k - p.n_series;
    if (i >= p.n_agg) return -1;
    const int c = p.agg_cols[i];
    return (c < 0 || c >= p.n_out) ? -1 : c;
}

__global__ __launch_bounds__(64) void mint_var_kernel(const ReconcileMintArgs a)
{
    __shared__ double tile[RB * RP];
    const int lane = threadIdx.x, nres = a.n_res;
    const size_t c0 = (size_t)blockIdx.x * RB, cc = c0 + (size_t)lane;
    const bool inside = cc < (size_t)a.p.n_out;
    int part = 0;
    if (inside) {
        int o0, o1;
        rec_column(a.p, (int)cc, o0, o1);
        part = o1 > o0;
    }
    const bool along_t = a.res_stride_t < a.res_stride_s;              // a series-major block: the lanes of a load run along the rows
    const int passes = a.gram ? 2 : 1;
    double rs = 0.0;
    for (int pass = 0; pass < passes; pass++) {
        double acc = 0.0;
        int bad = 0;
        for (int t0 = 0; t0 < nres; t0 += RB) {
            const int nt = nres - t0 < RB ? nres - t0 : RB;
            __syncthreads();                                             // every lane has summed the previous tile
            if (along_t) {
                for (int k = 0; k < RB; k++) {
                    const int pk = __shfl(part, k);                      // (an empty column is never read)
                    tile[k * RP + lane] = (pk && lane < nt) ? a.res[(c0 + (size_t)k) * a.res_stride_s + (size_t)(t0 + lane) * a.res_stride_t] : 0.0;
                }
            } else {
                for (int k = 0; k < nt; k++) tile[lane * RP + k] = part ? a.res[cc * a.res_stride_s + (size_t)(t0 + k) * a.res_stride_t] : 0.0;
            }
            __syncthreads();
            if (part) {
                const double *row = tile + lane * RP;
                if (pass == 0) {
                    for (int j = 0; j < nt; j++) {
                        const double x = row[j];
                        if (!isfinite(x)) bad = 1;
                        acc = acc + x * x;
                    }
                } else {
                    for (int j = 0; j < nt; j++) {
                        const double xs = row[j] * rs, x2 = xs * xs;
                        acc = acc + x2 * x2;
                    }
                }
            }
        }
        if (!inside) continue;
        if (pass == 0) {
            const double v = part ? acc / (double)nres : 0.0;
            if (part && bad) atomicMin(&a.info[MINT_INFO_RESIDUAL], (int32_t)cc);
            else if (part && (!(v > 0.0) || !isfinite(v))) atomicMin(&a.info[MINT_INFO_VARIANCE], (int32_t)cc);
            rs = part ? 1.0 / sqrt(v) : 0.0;
            a.var[cc] = v;
            a.rsd[cc] = rs;
        } else {
            a.f4col[cc] = acc;
        }
    }
}

// One 64 x 64 product tile C += A B^T over K = RK staged values, both operands [row][k] at pitch KP.
// MFMA: wavefront `wave` owns rows 16 wave .. 16 wave + 15 and four 16-column sub-tiles; FMA: thread (ty, tx) owns 4 x 4 outputs.
template <bool MFMA> struct MintTile {
    double acc[4][4];
    rec_double4 macc[4];
    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int x = 0; x < 4; x++) {
            macc[x] = (rec_double4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int y = 0; y < 4; y++) acc[x][y] = 0.0;
        }
    }
    __device__ __forceinline__ void step(const double *As, const double *Bs, int tid)
    {
        const int tx = tid & 15, ty = tid >> 4, wave = tid >> 6, l = tid & 63;
        if (MFMA) {
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
    // element e in [0, 16) of this thread: its row and column inside the tile and its value
    __device__ __forceinline__ double at(int e, int tid, int &row, int &col) const
    {
        const int tx = tid & 15, ty = tid >> 4, wave = tid >> 6, l = tid & 63;
        if (MFMA) {
            // C/D of the f64 form: col = lane & 15, row = (lane >> 4) + 4 * reg
            const int cb = e >> 2, reg = e & 3;
            row = 16 * wave + (l >> 4) + 4 * reg;
            col = 16 * cb + (l & 15);
            return macc[cb][reg];
        }
        row = ty * 4 + (e >> 2);
        col = tx * 4 + (e & 3);
        return acc[e >> 2][e & 3];
    }
};

__global__ __launch_bounds__(256) void mint_gram_kernel(const ReconcileMintArgs a)
{
    __shared__ double As[RB * KP], Bs[RB * KP], ks[RK];
    __shared__ int kc[RK];
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bj > bi) return;
    const int tid = threadIdx.x, nres = a.n_res, i0 = bi * RB, j0 = bj * RB;
    const int np = a.p.n_series + a.p.n_agg;
    const int per = (np + a.gram_splits - 1) / a.gram_splits, chunk = (per + RK - 1) / RK * RK;
    const long long lo = (long long)blockIdx.z * chunk;
    const int k_lo = lo < np ? (int)lo : np, k_hi = np - k_lo < chunk ? np : k_lo + chunk;
    const bool along_t = a.res_stride_t < a.res_stride_s;
    const bool diag = bi == bj;
    MintTile<true> tile;
    tile.clear();
    for (int kk = k_lo; kk < k_hi; kk += RK) {
        __syncthreads();
        if (tid < RK) {
            const int c = kk + tid < k_hi ? mint_participant(a.p, kk + tid) : -1;
            kc[tid] = c;
            ks[tid] = c >= 0 ? a.rsd[c] : 0.0;
        }
        __syncthreads();
        for (int e = tid; e < RB * RK; e += 256) {
            const int row = along_t ? e & 63 : e >> 5, k = along_t ? e >> 6 : e & 31;
            const int c = kc[k];
            const size_t off = c >= 0 ? (size_t)c * a.res_stride_s : 0;
            As[row * KP + k] = (c >= 0 && i0 + row < nres) ? a.res[off + (size_t)(i0 + row) * a.res_stride_t] * ks[k] : 0.0;
            if (!diag) Bs[row * KP + k] = (c >= 0 && j0 + row < nres) ? a.res[off + (size_t)(j0 + row) * a.res_stride_t] * ks[k] : 0.0;
        }
        __syncthreads();
        tile.step(As, diag ? As : Bs, tid);
    }
    double *G = a.gram + (size_t)blockIdx.z * (size_t)nres * (size_t)nres;
#pragma unroll
    for (int e = 0; e < 16; e++) {
        int row, col;
        const double v = tile.at(e, tid, row, col);
        if (i0 + row < nres && j0 + col < nres) G[(size_t)(i0 + row) * (size_t)nres + (size_t)(j0 + col)] = v;
    }
}

// a fixed tree over the 256 values of a workgroup; the sum is in s[0] afterwards
__device__ __forceinline__ void mint_tree(double *s, int tid)
{
    for (int w = 128; w > 0; w >>= 1) {
        __syncthreads();
        if (tid < w) s[tid] = s[tid] + s[tid + w];
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void mint_gram_reduce_kernel(const ReconcileMintArgs a)
{
    __shared__ double sf[256], sq[256];
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bj > bi) return;
    const int tid = threadIdx.x, nres = a.n_res, i0 = bi * RB, j0 = bj * RB;
    const size_t plane = (size_t)nres * (size_t)nres;
    double fro = 0.0, q = 0.0;
    for (int e = tid; e < RB * RB; e += 256) {
        const int gi = i0 + (e >> 6), gj = j0 + (e & 63);
        if (gi >= nres || gj >= nres) continue;
        double g = 0.0;
        for (int z = 0; z < a.gram_splits; z++) g = g + a.gram[(size_t)z * plane + (size_t)gi * (size_t)nres + (size_t)gj];
        const double g2 = g * g;
        fro = fro + g2;
        if (gi == gj) q = q + g2;
    }
    sf[tid] = fro; sq[tid] = q;
    mint_tree(sf, tid);
    mint_tree(sq, tid);
    if (tid == 0) {
        const int nt = (nres + RB - 1) / RB;
        const size_t tiles = (size_t)nt * (size_t)(nt + 1) / 2, at = (size_t)bi * (size_t)(bi + 1) / 2 + (size_t)bj;
        double *part = a.gram + (size_t)a.gram_splits * plane;
        part[at] = bi == bj ? sf[0] : 2.0 * sf[0];                       // (G is symmetric: the tile above the diagonal holds the same values)
        part[tiles + at] = sq[0];
    }
}

__global__ __launch_bounds__(256) void mint_lambda_kernel(const ReconcileMintArgs a)
{
    __shared__ double s[256];
    const int tid = threadIdx.x, nres = a.n_res, np = a.p.n_series + a.p.n_agg;
    const int nt = (nres + RB - 1) / RB;
    const size_t tiles = (size_t)nt * (size_t)(nt + 1) / 2;
    const double *part = a.gram + (size_t)a.gram_splits * (size_t)nres * (size_t)nres;
    double sums[3];
    for (int which = 0; which < 3; which++) {
        double acc = 0.0;
        if (which < 2) {
            for (size_t k = tid; k < tiles; k += 256) acc = acc + part[(size_t)which * tiles + k];
        } else {
            for (int k = tid; k < np; k += 256) {
                const int c = mint_participant(a.p, k);
                if (c >= 0) acc = acc + a.f4col[c];
            }
        }
        __syncthreads();                                                 // (s[0] of the previous sum has been read)
        s[tid] = acc;
        mint_tree(s, tid);
        sums[which] = s[0];
    }
    if (tid == 0) {
        const double fro = sums[0], q = sums[1], f4 = sums[2], T = (double)nres, n = (double)np;
        const double sum_v = ((q - f4) - (fro - n * (T * T)) / T) / (T * (T - 1.0));
        const double sum_d = fro / (T * T) - n;
        double lam = 1.0;
        if (isfinite(sum_d) && sum_d > 0.0) {
            lam = sum_v / sum_d;
            lam = lam > 0.0 ? lam : 0.0;
            lam = lam < 1.0 ? lam : 1.0;
        }
        *a.lambda = lam;
    }
}

// tile (I, J), J <= I: M_IJ = lambda M_IJ + ((1 - lambda) / n_res) (E^T E)_IJ.  As / Bs hold [column of E][t] at pitch KP.
template <int VARIANT> __global__ __launch_bounds__(256) void mint_ete_kernel(const ReconcileMintArgs a)
{
    __shared__ double As[RB * KP], Bs[RB * KP];
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bj > bi) return;
    const int tid = threadIdx.x, na = a.p.n_agg, nres = a.n_res, i0 = bi * RB, j0 = bj * RB;
    if (i0 >= na) return;
    const bool diag = bi == bj;
    MintTile<VARIANT == RECONCILE_TRAILING_MFMA> tile;
    tile.clear();
    for (int t0 = 0; t0 < nres; t0 += RK) {
        __syncthreads();
        for (int e = tid; e < RB * RK; e += 256) {
            const int row = e & 63, k = e >> 6;                          // (lanes along a row of E)
            const bool tin = t0 + k < nres;
            const size_t off = (size_t)(t0 + k) * a.ld_e;
            As[row * KP + k] = (tin && i0 + row < na) ? a.E[off + (size_t)(i0 + row)] : 0.0;
            if (!diag) Bs[row * KP + k] = (tin && j0 + row < na) ? a.E[off + (size_t)(j0 + row)] : 0.0;
        }
        __syncthreads();
        tile.step(As, diag ? As : Bs, tid);
    }
    const double lam = *a.lambda, cf = (1.0 - lam) / (double)nres;
#pragma unroll
    for (int e = 0; e < 16; e++) {
        int row, col;
        const double v = tile.at(e, tid, row, col);
        const int gi = i0 + row, gj = j0 + col;
        if (gi < na && gj <= gi) {
            double *at = a.L + (size_t)gi * a.ld_a + (size_t)gj;
            *at = lam * *at + cf * v;
        }
    }
}

// ---- apply ----

// g[row][t] = sum_i E[t][i] mu[row][i]: workgroup (64 t, 32 rows), thread (t, 8 rows); the fma chain runs over i ascending
__global__ __launch_bounds__(256) void mint_g_kernel(const ReconcileMintApplyArgs m)
{
    __shared__ double Es[RB * RP], Mu[RC * RP];
    const int tid = threadIdx.x, tl = tid & 63, rg = tid >> 6, na = m.a.p.n_agg, nres = m.n_res;
    const int t0 = (int)blockIdx.x * RB;
    const size_t n_chunks = (m.a.n_rows + RC - 1) / RC;
    for (size_t ch = blockIdx.y; ch < n_chunks; ch += gridDim.y) {
        const size_t r0 = ch * RC;
        const int nc = m.a.n_rows - r0 < (size_t)RC ? (int)(m.a.n_rows - r0) : RC;
        double acc[MINT_ROWS_PER_THREAD];
#pragma unroll
        for (int c = 0; c < MINT_ROWS_PER_THREAD; c++) acc[c] = 0.0;
        for (int i0 = 0; i0 < na; i0 += RB) {
            __syncthreads();
            for (int e = tid; e < RB * RB; e += 256) {
                const int r = e >> 6, c = e & 63;
                Es[r * RP + c] = (t0 + r < nres && i0 + c < na) ? m.E[(size_t)(t0 + r) * m.ld_e + (size_t)(i0 + c)] : 0.0;
            }
            for (int e = tid; e < RC * RB; e += 256) {
                const int r = e >> 6, c = e & 63;
                Mu[r * RP + c] = (r < nc && i0 + c < na) ? m.a.work[(r0 + (size_t)r) * m.a.ld_work + (size_t)(i0 + c)] : 0.0;
            }
            __syncthreads();
#pragma unroll 4
            for (int i = 0; i < RB; i++) {
                const double ev = Es[tl * RP + i];
#pragma unroll
                for (int c = 0; c < MINT_ROWS_PER_THREAD; c++) acc[c] = __builtin_fma(ev, Mu[(rg * MINT_ROWS_PER_THREAD + c) * RP + i], acc[c]);
            }
        }
        if (t0 + tl < nres) {
#pragma unroll
            for (int c = 0; c < MINT_ROWS_PER_THREAD; c++) {
                const int r = rg * MINT_ROWS_PER_THREAD + c;
                if (r < nc) m.g[(r0 + (size_t)r) * (size_t)nres + (size_t)(t0 + tl)] = acc[c];
            }
        }
    }
}

// every column of 64 per workgroup, 32 rows at a time: thread (column, 8 rows); the fma chain of a bottom column runs over t ascending
__global__ __launch_bounds__(256) void mint_bottom_kernel(const ReconcileMintApplyArgs m)
{
    __shared__ double Xs[RB * RP], Gs[RC * RP];
    __shared__ int isb[RB];
    const ReconcileApplyArgs &a = m.a;
    const int tid = threadIdx.x, cl = tid & 63, rg = tid >> 6, na = a.p.n_agg, nres = m.n_res;
    const size_t c0 = (size_t)blockIdx.x * RB, cc = c0 + (size_t)cl;
    const int c = (int)cc;
    int kind = 0, e0 = 0, e1 = 0;                                        // 0: an aggregate or past n_out, 1: empty, 2: a bottom column
    double vb = 0.0;
    if (cc < (size_t)a.p.n_out) {
        int o0, o1;
        rec_column(a.p, c, o0, o1);
        if (o1 == o0) kind = 1;
        else if (o1 - o0 == 1) {
            const int s = a.p.members[o0];
            if (rec_bottom_of(a.p, s) == c) {
                kind = 2;
                rec_leaf_range(a.p, s, e0, e1);
                vb = m.var[c];
            }
        }
    }
    if (tid < RB) isb[tid] = kind == 2;
    const bool along_t = m.res_stride_t < m.res_stride_s;
    const double lam = m.lambda, cf = (1.0 - lam) / (double)nres, lv = lam * vb;
    const size_t n_chunks = (a.n_rows + RC - 1) / RC;
    for (size_t ch = blockIdx.y; ch < n_chunks; ch += gridDim.y) {
        const size_t r0 = ch * RC;
        const int nc = a.n_rows - r0 < (size_t)RC ? (int)(a.n_rows - r0) : RC;
        double acc[MINT_ROWS_PER_THREAD];
#pragma unroll
        for (int k = 0; k < MINT_ROWS_PER_THREAD; k++) acc[k] = 0.0;
        for (int t0 = 0; na > 0 && t0 < nres; t0 += RB) {
            __syncthreads();                                             // (isb is written; the previous tile has been read)
            for (int e = tid; e < RB * RB; e += 256) {
                const int col = along_t ? e >> 6 : e & 63, t = along_t ? e & 63 : e >> 6;
                Xs[col * RP + t] = (isb[col] && t0 + t < nres) ? m.res[(c0 + (size_t)col) * m.res_stride_s + (size_t)(t0 + t) * m.res_stride_t] : 0.0;
            }
            for (int e = tid; e < RC * RB; e += 256) {
                const int r = e >> 6, t = e & 63;
                Gs[r * RP + t] = (r < nc && t0 + t < nres) ? m.g[(r0 + (size_t)r) * (size_t)nres + (size_t)(t0 + t)] : 0.0;
            }
            __syncthreads();
#pragma unroll 4
            for (int t = 0; t < RB; t++) {
                const double x = Xs[cl * RP + t];
#pragma unroll
                for (int k = 0; k < MINT_ROWS_PER_THREAD; k++) acc[k] = __builtin_fma(x, Gs[(rg * MINT_ROWS_PER_THREAD + k) * RP + t], acc[k]);
            }
        }
        if (kind == 0) continue;
#pragma unroll
        for (int k = 0; k < MINT_ROWS_PER_THREAD; k++) {
            const int r = rg * MINT_ROWS_PER_THREAD + k;
            if (r >= nc) continue;
            const size_t row = r0 + (size_t)r, at = (size_t)c * a.stride_s + row * a.stride_t;
            double v = a.base[at];
            if (kind == 2) {
                if (na > 0) {
                    double chain = 0.0;
                    for (int e = e0; e < e1; e++) {
                        const int i = a.p.leaf_aggs[e];
                        if (i >= 0 && i < na) chain += a.work[row * a.ld_work + (size_t)i];
                    }
                    v = (v + lv * chain) - cf * acc[k];
                }
                if (a.row_status[row]) v = __builtin_nan("");
            }
            a.out[at] = v;
        }
    }
}

} // namespace

void launch_reconcile_mint_factor(const ReconcileMintArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(mint_init_kernel, dim3(1), dim3(64), 0, stream, a.info);
    if (a.p.n_out <= 0 || a.n_res <= 0) return;
    hipLaunchKernelGGL(mint_var_kernel, dim3((unsigned)(((size_t)a.p.n_out + RB - 1) / RB)), dim3(64), 0, stream, a);
    const unsigned nt = (unsigned)((a.n_res + RB - 1) / RB);
    if (a.gram) {
        hipLaunchKernelGGL(mint_gram_kernel, dim3(nt, nt, (unsigned)a.gram_splits), dim3(256), 0, stream, a);
        hipLaunchKernelGGL(mint_gram_reduce_kernel, dim3(nt, nt), dim3(256), 0, stream, a);
        hipLaunchKernelGGL(mint_lambda_kernel, dim3(1), dim3(256), 0, stream, a);
    } else {
        hipLaunchKernelGGL(mint_set_lambda_kernel, dim3(1), dim3(64), 0, stream, a.lambda, a.lambda_in);
    }
    const int na = a.p.n_agg;
    if (na <= 0) return;
    ReconcileApplyArgs e{};
    e.p = a.p; e.base = a.res; e.stride_s = a.res_stride_s; e.stride_t = a.res_stride_t; e.n_rows = (size_t)a.n_res;
    e.work = a.E; e.ld_work = a.ld_e;
    launch_reconcile_incoherence(e, stream);
    ReconcileFactorArgs f{};
    f.p = a.p; f.p.weights = a.var; f.L = a.L; f.ld_a = a.ld_a; f.info = a.info + MINT_INFO_WEIGHT; f.trailing = a.trailing;
    launch_reconcile_assemble(f, stream);
    const unsigned nb = (unsigned)((na + RB - 1) / RB);
    if (a.ete == RECONCILE_TRAILING_MFMA) hipLaunchKernelGGL(mint_ete_kernel<RECONCILE_TRAILING_MFMA>, dim3(nb, nb), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(mint_ete_kernel<RECONCILE_TRAILING_FMA>, dim3(nb, nb), dim3(256), 0, stream, a);
    launch_reconcile_panels(f, stream);
}

void launch_reconcile_mint_apply(const ReconcileMintApplyArgs &m, hipStream_t stream)
{
    const ReconcileApplyArgs &a = m.a;
    if (a.n_rows == 0) return;
    launch_reconcile_status(a, stream);
    if (a.p.n_out <= 0) return;
    const size_t n_chunks = (a.n_rows + RC - 1) / RC;
    const unsigned gy = (unsigned)(n_chunks > REC_MAX_GRID_Y ? REC_MAX_GRID_Y : n_chunks);
    if (a.p.n_agg > 0) {
        launch_reconcile_incoherence(a, stream);
        launch_reconcile_substitute(a, stream);
        hipLaunchKernelGGL(mint_g_kernel, dim3((unsigned)((m.n_res + RB - 1) / RB), gy), dim3(256), 0, stream, m);
    }
    hipLaunchKernelGGL(mint_bottom_kernel, dim3((unsigned)(((size_t)a.p.n_out + RB - 1) / RB), gy), dim3(256), 0, stream, m);
    launch_reconcile_aggregates(a, stream);
}

} // namespace anofox
